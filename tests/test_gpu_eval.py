"""Policy evaluation on the MI355X: the lgx_eval_* kernels (csrc/lgx_env.hip) against the float64
restatement and the host backend on scripted inputs (tests/eval_case.py, the host test's bounds:
the backends sum the joints in different orders), and PolicyEvaluator end to end — eager steps
against the restatement fed from the env's public tensors, the student / teacher action against
the torch modules, graph replay against the eager loop bit for bit, and the parkour cell grid."""
import types

import pytest
import torch

import eval_case as E
from test_eval_host import _scripted_env, eval_error_paths

pytestmark = pytest.mark.gpu
dev = "cuda:0"


@pytest.mark.parametrize("n", [1, 63, 130])
def test_kernels_match_the_restatement_and_the_host_backend(n):
    env, gen = _scripted_env(n, dev)
    ref = E.run_script(env, gen)
    E.check_records(env.eval_acc, env.eval_status, ref, f"hip n={n}")
    host, hgen = _scripted_env(n, "cpu")  # the same generator seed: the same grid and script
    E.run_script(host, hgen)
    assert torch.equal(host.terrain_levels, env.terrain_levels.cpu())
    href = types.SimpleNamespace(acc=host.eval_acc.double(), status=host.eval_status, absfwd=ref.absfwd)
    E.check_records(env.eval_acc, env.eval_status, href, f"hip vs host n={n}")
    cells = env.eval_cells()
    E.check_cells(cells, env.eval_acc, env.eval_status, env.terrain_levels, env.terrain_types)
    assert torch.equal(env.eval_cells(), cells)  # fixed order, fixed tree: bit-identical


def test_error_paths_fail_cleanly():
    eval_error_paths(dev)


def _evaluator(task="go2", n=66, policy="student", **over):
    from legged_gym_custom_amd.utils.evaluator import PolicyEvaluator
    over.setdefault("env.episode_length_s", 0.19)  # ceil(0.19 / 0.02) = 10 steps
    env, tcfg, args = E.make_env(task, n, dev, **over)
    assert int(env.max_episode_length) == 10
    runner = E.make_runner(env, tcfg, args)  # randomly initialised networks
    return PolicyEvaluator(env, runner, policy=policy)


def _inputs(env):
    return dict(commands=env.commands, base_lin_vel=env.base_lin_vel, base_ang_vel=env.base_ang_vel,
                torques=env.torques, dof_state=env.dof_state, contact_forces=env.contact_forces, reset=env.reset_buf,
                time_out=env.time_out_buf, blew_up=env.blew_up_buf)


def test_go2_eager_steps_match_the_restatement():
    ev = _evaluator()
    env = ev.env
    assert ev._fused is not None  # the one-launch act kernel covers the Go2 networks
    ev.begin()
    assert int(env.episode_length_buf.abs().sum()) == 0
    ref = E.Restatement(env.num_envs, env.dt, env.feet_indices)
    for _ in range(int(env.max_episode_length) + 1):
        ev.step()
        ref.accumulate(_inputs(env))
    E.check_records(env.eval_acc, env.eval_status, ref, "go2 end to end")
    assert int((ref.status == 0).sum()) == 0 and int((ref.status == 1).sum()) > 0
    rep = ev.report(env.eval_cells())
    assert rep["total"]["running"] == 0 and rep["total"]["episodes"] == env.num_envs
    assert all(v is not None and v == v for v in rep["total"].values())


@pytest.mark.parametrize("policy", ["student", "teacher"])
def test_action_is_the_deployed_composition(policy):
    """One step only: later steps diverge chaotically. 1e-5 absolute is the bound
    tests/test_gpu_s8_act.py holds this kernel to."""
    ev = _evaluator(policy=policy)
    env, ac, est = ev.env, ev.alg.actor_critic, ev.alg.estimator
    ev.begin()
    obs, priv, scan = env.obs_buf.clone(), env.privileged_obs_buf.clone(), env.scan_obs_buf.clone()
    ev.step()
    with torch.no_grad():
        want = ac.act_inference(obs, priv, est(obs), scan, adaptation_mode=policy == "student")
        other = ac.act_inference(obs, priv, est(obs), scan, adaptation_mode=policy != "student")
    err = float((env.actions_in - want).abs().max())
    print(f"{policy}: max |action - act_inference| {err:.3e}; to the other policy {float((env.actions_in - other).abs().max()):.3e}")
    assert err <= 1e-5


def test_graph_replay_equals_the_eager_loop_and_repeats():
    a, b = _evaluator(), _evaluator()
    for (k, x), (_, y) in zip(a.alg.actor_critic.state_dict().items(), b.alg.actor_critic.state_dict().items()):
        assert torch.equal(x, y), k
    ra = a.run()
    assert ra["graph"] is True and ra["num_steps"] == 11 and ra["total"]["running"] == 0
    first = a.last_cells.clone()
    rb = b.run(graph=False)
    assert rb["graph"] is False
    assert torch.equal(first, b.last_cells)
    a.run()
    assert torch.equal(first, a.last_cells)
    assert float(first[..., 4].sum()) > 0


def test_parkour_envs_land_in_their_terrain_cells():
    ev = _evaluator("go2_parkour", 64, **{"terrain.curriculum": False, "commands.curriculum": False})
    env = ev.env
    t = env.cfg.terrain
    rep = ev.run(3)
    cells = ev.last_cells
    assert cells.shape == (t.num_rows, t.num_cols, 12) and rep["terrain_levels"] == t.num_rows
    want = torch.bincount((env.terrain_levels * t.num_cols + env.terrain_types).cpu(), minlength=t.num_rows * t.num_cols)
    assert torch.equal(cells[..., 0].reshape(-1).long(), want)
    assert int(cells[..., 0].sum()) == 64
    E.check_cells(cells, env.eval_acc, env.eval_status, env.terrain_levels, env.terrain_types)
    empty = rep["cells"][int((want == 0).nonzero()[0]) // t.num_cols][int((want == 0).nonzero()[0]) % t.num_cols]
    assert empty["episodes"] == 0 and empty["survival_rate"] is None
