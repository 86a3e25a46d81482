"""Shared by tests/test_gpu_actuator.py (device "cuda:0") and tests/test_actuator_host.py (the same
bodies on the host backend): actuation latency and motor strength (include/lgx.h, ABI 8).

The feature has no oracle. Every test reduces feature-on behaviour to feature-off behaviour, which
the oracle and the golden fixtures pin:
  * a latency of k whole control steps is the ideal actuator fed the action of k steps ago: bit-exact;
  * a latency of d physics substeps is a decimation-1 env fed, substep by substep, the action the rule
    a[t - ceil(max(d - s, 0) / n)] prescribes, from the test's own record of past actions;
  * a motor strength m in P mode is both gain multipliers scaled by m; with the actuator net it is
    the net's output scale scaled by m.
Bounds: where two different instruction sequences are compared, those of tests/test_gpu_pairing.py
(2e-3 + 1e-3 |ref|; contact forces 0.5 + 2e-2 |ref|), the repository's bound for one step of two
equivalent formulations; everything else is exact.

Measured worst differences (64 envs; each test prints its own): a 4-substep step against four
1-substep steps, Go2 12 steps: 4.3e-5 joint state, 4.8e-5 N m, 3.8e-4 N on the MI355X (4.5e-4,
4.1e-4, 1.3e-3 on the host backend), and a switch one substep late misses by 7000-7800 x the
bound; ANYmal 8 steps: 6.1e-5 and 9.9e-3 N (host 2.6e-4, 0.13 N), late switch 250-600 x. Strength
against scaled gains: 8.3e-4 joint state (unscaled gains: 6700 x the bound); strength 0.5 against
half the net's output scale: identical bits. Kernel against host backend, both features on, 16
steps: 2.1e-3 in a joint velocity of magnitude > 1 (63 envs), contact forces 2.8e-3 N."""
import math

import torch

PHYSICS = ("root_states", "dof_state", "torques", "contact_forces", "rigid_body_states")
DISCRETE = ("reset", "time_out", "episode_length", "last_contacts", "terrain_levels", "blew_up")
TOL = {"contact_forces": (0.5, 2e-2)}
DEFAULT_TOL = (2e-3, 1e-3)
H = 3  # control steps of history in the latency tests


def make_env(task, n, device, tmp_path=None, seed=1, sea_out_scale=1.0, **over):
    """go2 / go2_parkour through the registry (eval_case.make_env); anymal_c_rough with the synthetic
    actuator archive of tests/test_gpu_terrain.py. over: 'section.key' -> value; the value may be a
    callable of the fresh config (for values derived from sim.dt or control.decimation)."""
    from legged_gym_custom_amd.envs import task_registry_configs
    cfg = task_registry_configs(task)[0]
    over = {k: (v(cfg) if callable(v) else v) for k, v in over.items()}
    if task != "anymal_c_rough":
        import eval_case as E
        return E.make_env(task, n, device, seed=seed, **over)[0]
    from legged_gym_custom_amd import actuator as act
    from legged_gym_custom_amd.envs.anymal_c.anymal import Anymal
    from legged_gym_custom_amd.utils.helpers import SimParams, class_to_dict, set_seed
    w = act.random_sea_weights(1, scale=0.3)
    w["out_scale"] = w["out_scale"] * sea_out_scale
    path = str(tmp_path / f"sea_{sea_out_scale}.pt")
    act.save_sea_archive(w, path)
    cfg.env.num_envs = n
    cfg.terrain.num_rows, cfg.terrain.num_cols = 6, 6
    cfg.control.actuator_net_file = path
    for k, v in over.items():
        sec, key = k.split(".")
        setattr(getattr(cfg, sec), key, v)
    set_seed(seed)
    return Anymal(cfg, SimParams(class_to_dict(cfg.sim)), 1, device, True)


def capacity(h=H):
    """domain_rand.max_action_delay_s for h control steps of history."""
    return lambda cfg: h * cfg.control.decimation * cfg.sim.dt


def bound(env):
    return {k: t for k, t in env._native._keep.items() if not k.startswith("_") and torch.is_tensor(t)}


def copy_state(src, dst, skip=()):
    """Every tensor both envs have bound, src -> dst (across devices too)."""
    bs, bd = bound(src), bound(dst)
    for k in bs:
        if k in bd and k not in skip:
            bd[k].copy_(bs[k])


def worst_ratio(got, ref, names, worst=None):
    """max over names and elements of |got - ref| / (atol + rtol |ref|); worst collects max |got - ref|."""
    r = 0.0
    for name in names:
        atol, rtol = TOL.get(name, DEFAULT_TOL)
        a, b = got[name].detach().cpu().double(), ref[name].detach().cpu().double()
        d = (a - b).abs()
        if worst is not None:
            worst[name] = max(worst.get(name, 0.0), float(d.max()))
        r = max(r, float((d / (atol + rtol * b.abs())).max()))
    return r


def assert_equal(a, b, names, what):
    for name in names:
        assert torch.equal(a[name].cpu(), b[name].cpu()), (what, name, float((a[name].cpu() - b[name].cpu()).abs().max()))


# ------------------------------------------------------------------ 2. whole-step shift, bit-exact
def whole_step_shift(task, n, device, steps, tmp_path=None):
    X = make_env(task, n, device, tmp_path, **{"domain_rand.max_action_delay_s": capacity()})
    Y = make_env(task, n, device, tmp_path)
    assert X.action_history.shape == (n, H, X.num_actions) and Y.action_history is None
    dec = int(X.cfg.control.decimation)
    k = (torch.arange(n) * 7 % (H + 1)).to(device)  # 0..H mixed
    X.set_action_delay(k.double() * dec * X.sim_params.dt)
    assert torch.equal(X.action_delay_substeps.long(), k * dec)
    X.reset()
    Y.reset()
    gen = torch.Generator().manual_seed(3)
    past = []
    names = PHYSICS + (("sea_hidden", "sea_cell") if task == "anymal_c_rough" else ())
    for t in range(steps):
        a = (0.3 * torch.randn(n, X.num_actions, generator=gen)).to(device)
        past.append(a)
        ay = torch.zeros_like(a)
        for kk in range(H + 1):
            if t - kk >= 0:
                ay[k == kk] = past[t - kk][k == kk]
        X.step(a.clone())
        Y.step(ay)
        assert int(Y.reset_buf.sum()) == 0, f"step {t}: the reference env reset; choose other inputs"
        assert_equal(bound(X), bound(Y), names, f"{task} n={n} step {t}")
        assert torch.equal(X.action_history[:, 0], X.last_actions) and torch.equal(X.last_actions, a)
        for i in range(1, H):
            want = past[t - i] if t - i >= 0 else torch.zeros_like(a)
            assert torch.equal(X.action_history[:, i], want), (t, i)
    assert float(bound(X)["torques"].abs().max()) > 0


# ------------------------------------------------------------------ 3. sub-step delays against a split step
def rule_age(d, s, n):
    """ceil(max(d - s, 0) / n), the rule of include/lgx.h, on integer tensors."""
    return (torch.clamp(d - s, min=0) + n - 1) // n


def substep_delays(task, n, device, steps, tmp_path=None):
    X = make_env(task, n, device, tmp_path, **{"domain_rand.max_action_delay_s": capacity()})
    Y = make_env(task, n, device, tmp_path, **{"control.decimation": 1})
    dec = int(X.cfg.control.decimation)
    assert dec == 4 and int(Y.cfg.control.decimation) == 1 and Y.action_history is None
    for name in ("friction", "mass_params", "kp_kd"):  # the same setup draws
        assert torch.equal(bound(X)[name], bound(Y)[name]), name
    d = (torch.arange(n) * 5 % (H * dec + 1)).to(device)  # 0..H*4, non-multiples included
    X.set_action_delay(d.double() * X.sim_params.dt)
    assert torch.equal(X.action_delay_substeps.long(), d) and int((d % dec != 0).sum()) > n // 2
    X.reset()
    Y.reset()
    sea = ("sea_hidden", "sea_cell") if task == "anymal_c_rough" else ()
    start = ("root_states", "dof_state", "last_dof_vel") + sea
    compare = ("root_states", "dof_state", "torques", "contact_forces")
    gen = torch.Generator().manual_seed(4)
    past, worst, late = [], {}, 0.0
    zero = torch.zeros(n, X.num_actions, device=device)

    def split(shift):
        """Four one-substep steps of Y from X's pre-step state; substep s sees the action of age
        rule(d, s - shift): shift 0 is the rule, 1 switches one substep late."""
        for name in start:
            bound(Y)[name].copy_(bound(X)[name])
        for s in range(dec):
            age = rule_age(d, s - shift, dec)
            a = zero.clone()
            for g in range(H + 2):
                if len(past) - 1 - g >= 0:
                    a[age == g] = past[len(past) - 1 - g][age == g]
            Y.step(a)
            assert int(Y.reset_buf.sum()) == 0, "the reference env reset; choose other inputs"
        return {name: bound(Y)[name].clone() for name in compare}

    for t in range(steps):
        past.append(torch.clamp(0.3 * torch.randn(n, X.num_actions, generator=gen), -X.cfg.normalization.clip_actions,
                                X.cfg.normalization.clip_actions).to(device))
        wrong = split(1)
        ref = split(0)
        X.step(past[-1].clone())
        assert int(X.reset_buf.sum()) == 0, f"step {t}: env X reset; choose other inputs"
        got = {name: bound(X)[name] for name in compare}
        r = worst_ratio(got, ref, compare, worst)
        late = max(late, worst_ratio(wrong, ref, compare))
        assert r <= 1.0, (task, t, r, worst)
    print(f"{task} {device} worst |X - split| per buffer:", {k: f"{v:.1e}" for k, v in worst.items()},
          f"; a switch one substep late: {late:.0f} x the bound")
    assert late >= 100.0, late


# ------------------------------------------------------------------ 4. motor strength
def motor_strength_go2(device):
    n = 64
    on = {"domain_rand.randomize_kp_kd": True}
    X, Y = make_env("go2", n, device, **on), make_env("go2", n, device, **on)
    assert not torch.equal(Y.kp_kd_multipliers, torch.ones_like(Y.kp_kd_multipliers))
    gen = torch.Generator().manual_seed(5)
    m = (0.7 + 0.6 * torch.rand(n, X.num_dof, generator=gen)).to(device)
    X.reset()
    X.set_motor_strength(m)
    assert torch.equal(X.motor_strengths, m) and Y.motor_strengths is None
    a = torch.randn(n, X.num_actions, generator=gen).to(device)
    snap = {k: t.clone() for k, t in bound(X).items()}
    X.step(a.clone())

    def y_step(scale):
        for k, t in bound(Y).items():
            if k in snap:
                t.copy_(snap[k])
        Y.common_step_counter = X.common_step_counter - 1
        Y.kp_kd_multipliers.mul_(scale)
        Y.step(a.clone())
        return {k: bound(Y)[k].clone() for k in PHYSICS}

    ref = y_step(m.unsqueeze(0))
    assert int((ref["torques"].abs() == Y.torque_limits).sum()) > 0  # the multiply sits before the clip
    worst = {}
    r = worst_ratio(bound(X), ref, PHYSICS, worst)
    plain = worst_ratio(bound(X), y_step(1.0), PHYSICS)
    print(f"go2 {device} motor strength: worst |X - scaled gains| per buffer", {k: f"{v:.1e}" for k, v in worst.items()},
          f"; unscaled gains: {plain:.0f} x the bound")
    assert r <= 1.0, (r, worst)
    assert plain > 1.0


def motor_strength_anymal(device, tmp_path):
    n = 64
    X = make_env("anymal_c_rough", n, device, tmp_path)
    Y = make_env("anymal_c_rough", n, device, tmp_path, sea_out_scale=0.5)
    X.reset()
    X.set_motor_strength(0.5)
    gen = torch.Generator().manual_seed(6)
    a = torch.randn(n, X.num_actions, generator=gen).to(device)
    copy_state(X, Y)
    Y.common_step_counter = X.common_step_counter
    X.step(a.clone())
    Y.step(a.clone())
    names = PHYSICS + ("sea_hidden", "sea_cell")
    worst = {}
    r = worst_ratio(bound(X), bound(Y), names, worst)
    print(f"anymal {device} motor strength 0.5 vs half output scale:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert r <= 1.0 and float(bound(X)["torques"].abs().max()) > 0


# ------------------------------------------------------------------ 5. the device's backend against the host backend
def backend_vs_host(n, device):
    over = {"domain_rand.max_action_delay_s": capacity(), "domain_rand.randomize_kp_kd": True}
    X, Yh = make_env("go2", n, device, **over), make_env("go2", n, "cpu", **over)
    dec = int(X.cfg.control.decimation)
    gen = torch.Generator().manual_seed(7)
    d = torch.arange(n) * 5 % (H * dec + 1)
    m = 0.7 + 0.6 * torch.rand(n, X.num_dof, generator=gen)
    for env in (X, Yh):
        env.set_action_delay(d.double() * env.sim_params.dt)
        env.set_motor_strength(m.to(env.device))
        env.reset()
    cont = PHYSICS + ("obs", "rew", "last_dof_vel", "last_torques", "commands")
    worst = {}
    for t in range(16):
        a = 0.3 * torch.randn(n, X.num_actions, generator=gen)
        copy_state(X, Yh)
        Yh.common_step_counter = X.common_step_counter
        X.step(a.to(device))
        Yh.step(a.clone())
        bx, by = bound(X), bound(Yh)
        assert_equal(bx, by, [k for k in DISCRETE if k in bx] + ["action_history", "last_actions", "actions"], f"step {t}")
        r = worst_ratio(bx, by, cont, worst)
        assert r <= 1.0, (t, r, worst)
        assert torch.equal(X.action_history[:, 0], X.last_actions)
    print(f"go2 n={n} {device} vs host, feature on:", {k: f"{v:.1e}" for k, v in worst.items() if v > 0})
    assert float(X.action_history[:, 1:].abs().sum()) > 0
    ids = torch.arange(0, n, 3, device=X.device)
    X.reset_idx(ids)
    assert float(X.action_history[ids].abs().sum()) == 0 and float(X.action_history[1::3].abs().sum()) > 0
    assert torch.equal(X.action_history[:, 0], X.last_actions)


# ------------------------------------------------------------------ 6. identity and hygiene
def identity(device):
    n = 64
    X = make_env("go2", n, device, **{"domain_rand.max_action_delay_s": capacity(1)})
    Y = make_env("go2", n, device)
    X.set_motor_strength(1.0)
    assert int(X.action_delay_substeps.abs().sum()) == 0 and X.action_history.shape[1] == 1
    X.reset()
    Y.reset()
    gen = torch.Generator().manual_seed(8)
    for t in range(8):
        a = torch.randn(n, X.num_actions, generator=gen).to(device)
        X.step(a.clone())
        Y.step(a.clone())
        bx, by = bound(X), bound(Y)
        assert_equal(bx, by, [k for k in by if k in bx], f"step {t}")


def setup_draws(device, monkeypatch):
    n = 64
    base = {"domain_rand.randomize_kp_kd": True, "domain_rand.randomize_base_mass": True}
    on = dict(base, **{"domain_rand.randomize_action_delay": True, "domain_rand.action_delay_range_s": [0.0, 0.03],
                       "domain_rand.randomize_motor_strength": True})
    X, Y = make_env("go2", n, device, **on), make_env("go2", n, device, **base)
    for name in ("friction", "mass_params", "kp_kd"):
        assert torch.equal(bound(X)[name], bound(Y)[name]), name
    assert Y.action_delay_substeps is None and Y.motor_strengths is None
    dly, ms = X.action_delay_substeps, X.motor_strengths
    assert dly.dtype == torch.int32 and int(dly.min()) >= 0 and int(dly.max()) <= 6 and len(dly.unique()) > 2
    assert X.action_history.shape == (n, 2, X.num_actions)  # ceil(round(0.03 / 0.005) / 4)
    assert float(ms.min()) >= 0.9 and float(ms.max()) <= 1.1 and ms.shape == (n, X.num_dof) and len(ms.unique()) > n
    # two ranks of 32 envs draw rows [0, 32) and [32, 64) of the single-process draw
    import torch.distributed as dist
    for rank in (0, 1):
        monkeypatch.setattr(dist, "is_initialized", lambda: True)
        monkeypatch.setattr(dist, "get_rank", lambda group=None, rank=rank: rank)
        monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
        S = make_env("go2", n // 2, device, **on)
        monkeypatch.undo()
        sl = slice(rank * n // 2, (rank + 1) * n // 2)
        assert S.env_id_offset == rank * n // 2 and S.num_envs_total == n
        assert torch.equal(S.action_delay_substeps, dly[sl]) and torch.equal(S.motor_strengths, ms[sl])
        assert torch.equal(S.kp_kd_multipliers, X.kp_kd_multipliers[:, sl])


def refusals(device):
    import pytest
    from legged_gym_custom_amd import _native
    with pytest.raises(ValueError, match="LGX_MAX_ACTION_HISTORY"):
        make_env("go2", 8, device, **{"domain_rand.max_action_delay_s": capacity(5)})
    make_env("go2", 8, device, **{"domain_rand.max_action_delay_s": capacity(4)})  # H = 4 is allowed
    plain = make_env("go2", 8, device)
    with pytest.raises(ValueError, match="without actuation latency"):
        plain.set_action_delay(0.01)
    plain.action_delay_substeps = torch.zeros(8, dtype=torch.int32, device=device)
    with pytest.raises(_native.LgxError, match="action_delay needs action_history"):
        plain._bind()
    plain.action_delay_substeps = None
    plain.action_history = torch.zeros(8, 1, plain.num_actions, device=device)
    with pytest.raises(_native.LgxError, match="action_history_len = 0"):
        plain._bind()
    env = make_env("go2", 8, device, **{"domain_rand.max_action_delay_s": capacity(2)})
    env.set_action_delay(0.04)  # 8 substeps: the capacity
    assert int(env.action_delay_substeps.min()) == 8
    for bad in (0.045, -0.005, float("nan"), torch.zeros(7)):
        with pytest.raises(ValueError):
            env.set_action_delay(bad)
    assert int(env.action_delay_substeps.min()) == 8  # a refused value writes nothing
    for bad in (-0.1, float("inf"), torch.ones(7, 12)):
        with pytest.raises(ValueError):
            env.set_motor_strength(bad)
    # the kernel clamps what the Python layer would refuse: a raw out-of-range tensor is H * n substeps
    ref = make_env("go2", 8, device, **{"domain_rand.max_action_delay_s": capacity(2)})
    ref.set_action_delay(0.04)
    env.action_delay_substeps.fill_(1 << 30)
    env.action_delay_substeps[::2] = -5
    ref.action_delay_substeps[::2] = 0
    gen = torch.Generator().manual_seed(9)
    for e in (env, ref):
        e.reset()
    for _ in range(4):
        a = torch.randn(8, env.num_actions, generator=gen).to(device)
        env.step(a.clone())
        ref.step(a.clone())
        assert_equal(bound(env), bound(ref), PHYSICS + ("action_history",), "clamped delay")


# ------------------------------------------------------------------ 8. training smoke
def training_smoke(device, num_steps_per_env=None):
    import eval_case as E
    over = {"domain_rand.randomize_action_delay": True, "domain_rand.action_delay_range_s": [0.0, 0.02],
            "domain_rand.randomize_motor_strength": True}
    env, tcfg, args = E.make_env("go2", 64, device, **over)
    assert int(env.action_delay_substeps.max()) > 0 and env.motor_strengths is not None
    if num_steps_per_env:
        tcfg.runner.num_steps_per_env = num_steps_per_env
    runner = E.make_runner(env, tcfg, args)
    runner.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    if device != "cpu":
        assert env.graph_capturable and len(runner._graphs) > 0  # the rollout was captured and replayed
    assert torch.isfinite(env.obs_buf).all() and torch.isfinite(env.root_states).all()
    assert all(torch.isfinite(p).all() for p in runner.alg.actor_critic.parameters())
    assert torch.equal(env.action_history[:, 0], env.last_actions)
    assert math.isfinite(float(env.action_history.abs().sum())) and float(env.action_history.abs().sum()) > 0
