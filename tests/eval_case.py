"""Shared by tests/test_eval_host.py and tests/test_gpu_eval.py: a scripted sequence of
lgx_eval_accumulate inputs written straight into the env's tensors (no physics step), a float64
torch restatement of include/lgx.h's lgx_eval_accumulate / lgx_eval_reduce, and the bounds.

Bounds (from the number formats, not from the code under test): a record column is an fp32
running sum of T <= 11 non-negative terms, each holding a <= 14-term fp32 joint sum, so its
relative error is at most about (T + 14) * 2^-24 = 1.5e-6; rtol 1e-5 is about 7x that. The signed
column 3 is bounded against the sum of its terms' magnitudes instead. Column 7 is a maximum of
fp32 norms of 3 components (error about 2.5 * 2^-24): rtol 1e-6. Counts and statuses are exact."""
import torch

ROWS, COLS, CALLS = 3, 2, 6


def make_env(task, n, device, seed=1, **over):
    """The task's env through the registry on a fresh config; over: 'section.key' -> value."""
    from legged_gym_custom_amd.envs import task_registry, task_registry_configs
    from legged_gym_custom_amd.utils.helpers import get_args
    cfg, tcfg = task_registry_configs(task)
    cfg.seed = tcfg.seed = seed
    for k, v in over.items():
        sec, key = k.split(".")
        setattr(getattr(cfg, sec), key, v)
    args = get_args([f"--task={task}", "--headless", f"--num_envs={n}", f"--sim_device={device}",
                     f"--rl_device={device}", f"--seed={seed}"])
    env, _ = task_registry.make_env(task, args, env_cfg=cfg)
    return env, tcfg, args


def make_runner(env, tcfg, args):
    from legged_gym_custom_amd.envs import task_registry
    runner, _ = task_registry.make_alg_runner(env, args=args, train_cfg=tcfg, log_root=None)
    return runner


def bind_grid(env, gen):
    """The flat task binds no terrain grid: bind random levels in {0,1,2} and types in {0,1}
    (cells 3 x 2) before the eval tensors are made."""
    n = env.num_envs
    env.cfg.terrain.num_rows, env.cfg.terrain.num_cols = ROWS, COLS
    env.terrain_levels = torch.randint(0, ROWS, (n,), generator=gen).to(env.device)
    env.terrain_types = torch.randint(0, COLS, (n,), generator=gen).to(env.device)
    env._bind()


def script(n, gen):
    """CALLS steps of inputs (CPU tensors). Flags: for n >= 63 env 0 finishes at the first call
    (no sample, timed out), env 1 falls at call 2 and resets again (as a time-out) at call 4,
    env 2 blows up at call 3 (its time_out flag is set too: blow-up wins), env 3 times out at the
    last call; envs with e % 5 == 4 never reset; the rest reset once at a random call, half of
    them as time-outs."""
    steps = []
    when = torch.randint(0, CALLS, (n,), generator=gen)
    as_timeout = torch.rand(n, generator=gen) < 0.5
    never = torch.arange(n) % 5 == 4
    for t in range(CALLS):
        r = lambda *s, k=1.0: k * torch.randn(*s, generator=gen)  # noqa: E731
        reset = (when == t) & ~never
        tout = reset & as_timeout
        blew = torch.zeros(n, dtype=torch.bool)
        if n >= 63:
            reset[:4] = torch.tensor([t == 0, t in (2, 4), t == 3, t == CALLS - 1])
            tout[:4] = torch.tensor([t == 0, t == 4, t == 3, t == CALLS - 1])
            blew[2] = t == 3
        steps.append(dict(commands=r(n, 4), base_lin_vel=r(n, 3), base_ang_vel=r(n, 3), torques=r(n, 12, k=20.0),
                          dof_state=r(n, 12, 2, k=5.0), contact_forces=r(n, 19, 3, k=80.0), reset=reset, time_out=tout,
                          blew_up=blew))
    return steps


def write_inputs(env, s):
    """One scripted step into the tensors the native env is bound to."""
    assert env._contact3.shape[1:] == s["contact_forces"].shape[1:] and env.torques.shape[1] == 12
    for dst, k in ((env.commands, "commands"), (env.base_lin_vel, "base_lin_vel"), (env.base_ang_vel, "base_ang_vel"),
                   (env.torques, "torques"), (env._dof_state3, "dof_state"), (env._contact3, "contact_forces"),
                   (env.reset_buf, "reset"), (env.time_out_buf, "time_out"), (env.blew_up_buf, "blew_up")):
        dst.copy_(s[k])


class Restatement:
    """lgx_eval_accumulate in float64 torch, on CPU copies of the inputs."""

    def __init__(self, n, dt, feet):
        self.acc = torch.zeros(n, 8, dtype=torch.float64)
        self.absfwd = torch.zeros(n, dtype=torch.float64)  # sum |v0 * dt|: the bound of the signed column
        self.status = torch.zeros(n, dtype=torch.uint8)
        self.dt, self.feet = float(dt), feet.cpu().long()

    def accumulate(self, s):
        d = lambda k: s[k].detach().cpu().double()  # noqa: E731
        c, v, w, tq = d("commands"), d("base_lin_vel"), d("base_ang_vel"), d("torques")
        qd = d("dof_state").reshape(tq.shape[0], -1, 2)[..., 1]
        cf = d("contact_forces").reshape(tq.shape[0], -1, 3)
        reset, tout, blew = (s[k].detach().cpu().bool() for k in ("reset", "time_out", "blew_up"))
        running = self.status == 0
        fin = running & reset
        new = torch.where(blew, 3, torch.where(tout, 1, 2)).to(torch.uint8)
        self.status = torch.where(fin, new, self.status)
        m = (running & ~reset).double()
        a, dt = self.acc, self.dt
        a[:, 0] += m
        a[:, 1] += m * ((c[:, 0] - v[:, 0]) ** 2 + (c[:, 1] - v[:, 1]) ** 2)
        a[:, 2] += m * (c[:, 2] - w[:, 2]) ** 2
        a[:, 3] += m * v[:, 0] * dt
        a[:, 4] += m * torch.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2) * dt
        a[:, 5] += m * dt * (tq * qd).abs().sum(1)
        a[:, 6] += m * (tq ** 2).sum(1)
        peak = cf[:, self.feet].norm(dim=-1).max(dim=1).values
        a[:, 7] = torch.where(m > 0, torch.maximum(a[:, 7], peak), a[:, 7])
        self.absfwd += m * (v[:, 0] * dt).abs()


def check_records(acc, status, ref, what=""):
    """Records of the code under test against the restatement, at the bounds of the module docstring."""
    acc, status = acc.detach().cpu().double(), status.detach().cpu()
    assert torch.equal(status, ref.status), f"{what} status"
    assert torch.equal(acc[:, 0], ref.acc[:, 0]), f"{what} sample counts"
    for k in (1, 2, 4, 5, 6):
        err = (acc[:, k] - ref.acc[:, k]).abs()
        print(f"{what} acc[{k}] max rel err {float((err / ref.acc[:, k].clamp_min(1e-300)).max()):.3e}")
        assert bool((err <= 1e-5 * ref.acc[:, k].abs()).all()), f"{what} acc[{k}]"
    err = (acc[:, 3] - ref.acc[:, 3]).abs()
    print(f"{what} acc[3] max err / sum|v0 dt| {float((err / ref.absfwd.clamp_min(1e-300)).max()):.3e}")
    assert bool((err <= 1e-5 * ref.absfwd).all()), f"{what} acc[3]"
    err = (acc[:, 7] - ref.acc[:, 7]).abs()
    print(f"{what} acc[7] max rel err {float((err / ref.acc[:, 7].clamp_min(1e-300)).max()):.3e}")
    assert bool((err <= 1e-6 * ref.acc[:, 7]).all()), f"{what} acc[7]"


def cells_of(acc, status, levels, types, rows, cols):
    """lgx_eval_reduce restated: float64 torch sums of the given records per cell."""
    acc, status = acc.detach().cpu().double(), status.detach().cpu().long()
    n = acc.shape[0]
    cell = (torch.zeros(n, dtype=torch.long) if levels is None else levels.cpu().long() * cols + types.cpu().long())
    out = torch.zeros(rows * cols, 12, dtype=torch.float64)
    for c in range(rows * cols):
        m = cell == c
        out[c, 0] = m.sum()
        for st in (1, 2, 3):
            out[c, st] = (m & (status == st)).sum()
        out[c, 4:] = acc[m & (status != 0)].sum(0)
    return out.reshape(rows, cols, 12)


def check_cells(cells, acc, status, levels, types):
    rows, cols = cells.shape[:2]
    want = cells_of(acc, status, levels, types, rows, cols)
    assert torch.equal(cells[..., :4], want[..., :4]), "cell counts"
    torch.testing.assert_close(cells[..., 4:], want[..., 4:], rtol=1e-12, atol=0.0)
    assert int(cells[..., 0].sum()) == acc.shape[0]


def run_script(env, gen):
    """eval_begin, the scripted calls, and the restatement alongside. Returns the restatement."""
    steps = script(env.num_envs, gen)
    ref = Restatement(env.num_envs, env.dt, env.feet_indices)
    env.eval_begin()
    for s in steps:
        write_inputs(env, s)
        env.eval_accumulate()
        ref.accumulate(s)
    return ref
