"""Shared by tests/test_gpu_command.py (device "cuda:0") and tests/test_command_host.py (the same
bodies on the host backend): the command schedule of the env step (lgx_buffers.cmd_step / cmd_val)
and the command-response evaluation (lgx_eval_buffers.cmd_switch_step / cmd_rec / cmd_cells),
include/lgx.h ABI 10.

The feature has no oracle. Every test reduces it to feature-off behaviour, which the oracle and
the golden fixtures pin:
  * a schedule {0: c} for all envs is commands.user_command = c: two envs, every bound buffer bit for
    bit at every step, resets included (resampling every 5 steps, so the draws the schedule
    overwrites do happen);
  * rows without a used entry are the rows of an env without the buffers, bit for bit; bound
    buffers with no used entry change nothing;
  * the schedule is literal: after every step commands[:, :4] is the active segment's row exactly
    (also with the heading controller on) and the observation carries it;
  * the records and cells are compared with a float64 torch restatement on scripted inputs.
Bounds. Record columns 0, 1, 2, 4 hold small integers: exact (the scripted errors stay more than
1e-4 relative away from the tolerances, a thousand times the fp32 error of err, so no decision can
tie). Columns 5..7 are fp32 running sums of n = rec[4] terms: |diff| <= n 2^-23 sum|term| (each of
the n - 1 additions rounds by at most 2^-24 of a partial sum, itself at most sum|term|; 2x margin).
Column 3 is a maximum of single atan2f results in [0, pi]: 4 2^-23 pi (a few ulp of pi). Cells: fp64
sums of at most 130 fp32 values, 1e-12 relative. Kernel against host backend: the bounds of
tests/actuator_case.py, as tests/push_case.py uses them.

Measured worst differences (each test prints its own) are recorded in DESIGN.md section 4.8."""
import math

import torch

import eval_case as E
from actuator_case import DEFAULT_TOL, DISCRETE, PHYSICS, TOL, assert_equal, bound, copy_state, make_env, worst_ratio
from push_case import per_env, rows

assert DEFAULT_TOL and TOL  # (the bounds worst_ratio applies)
ON = {"commands.scheduled_commands": True}
FAST = {"commands.resampling_time": 0.1}  # a resample every 5 steps: the overwritten draws happen
OWN = ("cmd_step", "cmd_val")             # bound only by an env with the feature
GRID = (3, 4)
CALLS, SETTLE_TOL, YAW_TOL, STEADY = 20, 1.5, 0.9, 5
UPSIDE_DOWN = (1.0, 0.0, 0.0, 0.0)


def flip(env, ids):
    env.root_states[ids, 3:7] = torch.tensor(UPSIDE_DOWN, device=env.device)


def active_rows(steps, values, ep):
    """The rule of include/lgx.h on CPU tensors: values[e][largest k with 0 <= steps[e][k] <= ep[e]],
    and whether there is such a k."""
    ok = (steps >= 0) & (steps <= ep.view(-1, 1))
    k = (ok * torch.arange(1, steps.shape[1] + 1)).max(dim=1).values - 1
    return values[torch.arange(steps.shape[0]), k.clamp_min(0)], k >= 0


# ------------------------------------------------------------------ 1. a schedule {0: c} is user_command = c
def equals_user_command(task, n, device):
    c = [0.8, -0.3, 0.4, 0.0]
    over = dict(FAST, **({"commands.heading_command": False} if task == "go2_parkour" else {}))
    A = make_env(task, n, device, **over, **{"commands.user_command": c})
    B = make_env(task, n, device, **over, **ON)
    assert not A.cfg.commands.heading_command and A.cmd_step is None and B.cmd_step.dtype == torch.int32
    assert bool((B.cmd_step == -1).all()) and int(A.task_params.resample_interval) == 5
    B.set_command_schedule([0], [c])  # before reset(): its reset sees segment 0
    A.reset()
    B.reset()
    for env in (A, B):
        flip(env, [6, 13])
    names = [k for k in bound(A) if k in bound(B)]
    assert "commands" in names and "obs" in names and all(k in bound(B) and k not in bound(A) for k in OWN)
    assert_equal(bound(A), bound(B), names, "after reset")
    gen = torch.Generator().manual_seed(21)
    nreset = 0
    for t in range(40):
        a = (0.3 * torch.randn(n, A.num_actions, generator=gen)).to(device)
        A.step(a.clone())
        B.step(a.clone())
        assert_equal(bound(A), bound(B), names, f"{task} n={n} step {t}")
        nreset += int(B.reset_buf.sum())
    want = torch.tensor(c).expand(n, 4)
    assert torch.equal(B.commands.cpu()[:, :4], want) and nreset >= 2
    print(f"command {task} n={n} {device}: {nreset} resets in 40 steps, every bound buffer equal")


# ------------------------------------------------------------------ 2. mixed rows, identity
def mixed_rows(n, device):
    X, Y, Z = make_env("go2", n, device, **FAST, **ON), make_env("go2", n, device, **FAST), \
        make_env("go2", n, device, **FAST, **ON)
    gen = torch.Generator().manual_seed(22)
    X.set_command_schedule(torch.tensor([0, 4, 11]).expand(n, 3), torch.randn(n, 3, 4, generator=gen))
    off = torch.arange(n) % 2 == 1
    X.cmd_step[off.to(device)] = -1  # half of the rows: no used entry
    for env in (X, Y, Z):
        env.reset()
        flip(env, [5, 6])  # one unscheduled and one scheduled env reset in the run
    assert "cmd_step" in bound(Z) and "cmd_step" not in bound(Y) and bool((Z.cmd_step == -1).all())
    changed = 0
    for t in range(16):
        a = (0.3 * torch.randn(n, X.num_actions, generator=gen)).to(device)
        for env in (X, Y, Z):
            env.step(a.clone())
        bx, by, bz = bound(X), bound(Y), bound(Z)
        assert_equal(bz, by, [k for k in by if k in bz], f"step {t}: buffers bound, no entry used")
        for k in per_env(bx, by):
            assert torch.equal(rows(bx[k], n).cpu()[off], rows(by[k], n).cpu()[off]), (t, k, "unscheduled rows")
        changed += int((rows(bx["commands"], n).cpu()[~off] != rows(by["commands"], n).cpu()[~off]).any(1).sum())
    assert changed >= 16 * (n // 2 - 1)  # and the scheduled rows do differ
    Z.clear_command_schedule()
    Y.clear_command_schedule()  # a no-op without the buffers
    assert Y.cmd_step is None and bool((Z.cmd_step == -1).all())
    X.clear_command_schedule()
    assert bool((X.cmd_step == -1).all())


# ------------------------------------------------------------------ 3. switch timing, heading bypass
def switch_timing(n, device):
    X = make_env("go2_parkour", n, device, **FAST, **ON, **{"noise.add_noise": False})
    assert X.cfg.commands.heading_command
    gen = torch.Generator().manual_seed(23)
    steps = torch.tensor([0, 5, 9]).expand(n, 3).contiguous()
    values = torch.randn(n, 3, 4, generator=gen)
    # the heading entries in [0, 3]: the heading reward wraps commands[:, 3] to (-pi, pi] in place after
    # the schedule is applied (the reference's side effect, go2.py:744); in fp32 that wrap is the identity
    # on [0, pi] and off by an ulp of 2 pi for a negative heading
    values[..., 3] = values[..., 3].abs().clamp(max=3.0)
    X.set_command_schedule(steps, values)
    X.reset()
    flip(X, [3])
    P = X.task_params
    o0 = int(P.history_len) * int(P.num_proprio) + 5
    scale = torch.tensor(list(P.commands_scale))
    assert torch.equal(X.commands.cpu()[:, :4], values[:, 0]), "after reset: segment 0"
    seen, after_reset = set(), []
    for t in range(14):
        X.step((0.3 * torch.randn(n, X.num_actions, generator=gen)).to(device))
        ep = X.episode_length_buf.cpu().long()
        want, has = active_rows(steps, values, ep)
        assert bool(has.all())
        cmd = X.commands.cpu()
        assert torch.equal(cmd[:, :4], want), (t, "commands are the active segment, yaw rate and heading included")
        assert torch.equal(X.obs_buf.cpu()[:, o0:o0 + 3], cmd[:, :3] * scale), (t, "observation command slots")
        seen |= set(((steps <= ep.view(-1, 1)).sum(1) - 1).tolist())
        if t == 0:
            assert bool(X.reset_buf[3]) and int(ep[3]) == 0 and torch.equal(cmd[3, :4], values[3, 0])
        after_reset.append((int(ep[3]), torch.equal(cmd[3, :4], values[3, 1])))
    assert seen == {0, 1, 2}
    assert (4, False) in after_reset and (5, True) in after_reset  # c1 again five steps after its reset


# ------------------------------------------------------------------ 3b. the command curriculum's redraw
def curriculum_redraw(n, device):
    """lgx_command_curriculum on a curriculum step whose mean passes the threshold: the range widens
    and the reset envs' commands are redrawn. Scheduled rows keep segment 0 (commands, observation,
    critic and history slots); unscheduled rows are an env's without the buffers, bit for bit."""
    over = {"commands.curriculum": True, "commands.max_forward_vel": 2.0, "noise.add_noise": False}  # room to widen
    X, Y = make_env("go2", n, device, **over, **ON), make_env("go2", n, device, **over)
    gen = torch.Generator().manual_seed(25)
    values = torch.randn(n, 2, 4, generator=gen)
    X.set_command_schedule([0, 7], values)
    off = torch.arange(n) % 2 == 1
    X.cmd_step[off.to(device)] = -1
    reset = (torch.arange(n) % 3 != 0).to(device)
    for env in (X, Y):
        env.reset()
        env.step(torch.zeros(n, env.num_actions, device=device))
        env.reset_buf.copy_(reset)
        env._curriculum_vals.fill_(1e6)  # far past the threshold
    before, before_x = ({k: t.clone() for k, t in bound(env).items()} for env in (Y, X))
    for env in (X, Y):
        env._native.command_curriculum(env.seed, int(env.max_episode_length), None, env._stream())
    bx, by = bound(X), bound(Y)
    assert not torch.equal(by["command_ranges"], before["command_ranges"]), "the range did not change"
    assert torch.equal(bx["command_ranges"], by["command_ranges"])
    r, on = reset.cpu(), ~off
    for k in (k for k in per_env(bx, by) if k not in ("command_ranges", "command_range_log")):
        assert torch.equal(rows(bx[k], n).cpu()[off], rows(by[k], n).cpu()[off]), (k, "unscheduled rows")
        for got, was in ((bx, before_x), (by, before)):
            assert torch.equal(rows(got[k], n).cpu()[~r], rows(was[k], n).cpu()[~r]), (k, "not reset: untouched")
    assert int((by["commands"].cpu()[r] != before["commands"].cpu()[r]).any(1).sum()) > 0  # a redraw did happen
    P = X.task_params
    H, Pp = int(P.history_len), int(P.num_proprio)
    want = values[:, 0][on & r]
    slots = want[:, :3] * torch.tensor(list(P.commands_scale))
    assert torch.equal(X.commands.cpu()[on & r][:, :4], want) and int((on & r).sum()) > n // 4
    assert torch.equal(X.obs_buf.cpu()[on & r][:, H * Pp + 5:H * Pp + 8], slots)
    assert torch.equal(X.critic_obs_buf.cpu()[on & r][:, H * Pp + 5:H * Pp + 8], slots)
    hist = rows(bx["obs_history"], n).cpu()[on & r].view(-1, H, Pp)
    assert torch.equal(hist[:, :, 5:8], slots.view(-1, 1, 3).expand(-1, H, 3))


# ------------------------------------------------------------------ 4. the device's backend against the host backend
def backend_vs_host(n, device):
    X, Yh = make_env("go2", n, device, **FAST, **ON), make_env("go2", n, "cpu", **FAST, **ON)
    gen = torch.Generator().manual_seed(24)
    steps = (torch.tensor([0, 3, 7, 12]) + torch.arange(n).view(n, 1) % 3).contiguous()
    steps[:, 0] = 0
    values = torch.randn(n, 4, 4, generator=gen)
    for env in (X, Yh):
        env.set_command_schedule(steps.to(env.device), values.to(env.device))
        env.reset()
    cont = PHYSICS + ("obs", "rew", "last_dof_vel", "last_torques", "last_root_vel")
    worst = {}
    for t in range(16):
        a = 0.3 * torch.randn(n, X.num_actions, generator=gen)
        copy_state(X, Yh)
        Yh.common_step_counter = X.common_step_counter
        X.step(a.to(device))
        Yh.step(a.clone())
        bx, by = bound(X), bound(Yh)
        assert_equal(bx, by, [k for k in DISCRETE if k in bx] + ["last_actions", "actions", "commands", "cmd_step",
                                                                 "cmd_val"], f"step {t}")
        want, has = active_rows(steps, values, X.episode_length_buf.cpu().long())
        assert bool(has.all()) and torch.equal(X.commands.cpu()[:, :4], want)
        r = worst_ratio(bx, by, cont, worst)
        assert r <= 1.0, (t, r, worst)
    ratio = {k: v / TOL.get(k, DEFAULT_TOL)[0] for k, v in worst.items() if v > 0}
    print(f"command go2 n={n} {device} vs host, schedule on:", {k: f"{v:.1e}" for k, v in worst.items() if v > 0},
          "worst |diff| / atol:", {k: f"{v:.3f}" for k, v in ratio.items()})
    return worst


# ------------------------------------------------------------------ 5. records and cells
def command_script(n, gen):
    """CALLS steps of lgx_eval_accumulate inputs (CPU tensors, the style of eval_case.script) with
    projected_gravity (unit vectors, some past 90 degrees) and episode_length per call, a switch
    step per env and cell ids on the GRID. For n >= 63: env 1 resets at call 1, before its switch
    step 6; env 2 has switch step 0 (no record); envs with e % 5 == 4 never finish; the rest finish
    once at a call in 8..19, about two thirds of them as time-outs."""
    when = torch.randint(8, CALLS, (n,), generator=gen)
    as_timeout = torch.rand(n, generator=gen) < 0.67
    never = torch.arange(n) % 5 == 4
    switch = torch.randint(1, 8, (n,), generator=gen).to(torch.int32)
    if n >= 63:
        when[1], never[1], switch[1] = 1, False, 6
        switch[2] = 0
    cell_ids = torch.randint(0, GRID[0] * GRID[1], (n,), generator=gen).to(torch.int32)
    steps = []
    for t in range(CALLS):
        r = lambda *s, k=1.0: k * torch.randn(*s, generator=gen)  # noqa: E731
        reset = (when == t) & ~never
        pg = r(n, 3)
        steps.append(dict(commands=r(n, 4), base_lin_vel=r(n, 3), base_ang_vel=r(n, 3), torques=r(n, 12, k=20.0),
                          dof_state=r(n, 12, 2, k=5.0), contact_forces=r(n, 19, 3, k=80.0), reset=reset,
                          time_out=reset & as_timeout, blew_up=torch.zeros(n, dtype=torch.bool),
                          projected_gravity=pg / pg.norm(dim=1, keepdim=True),
                          episode_length=t + 1 + torch.arange(n) % 2))
    return steps, switch, cell_ids


class CommandRestatement(E.Restatement):
    """lgx_eval_accumulate's step-response record in float64 torch, next to the plain record."""

    def __init__(self, n, dt, feet, switch):
        super().__init__(n, dt, feet)
        self.rec = torch.zeros(n, 8, dtype=torch.float64)
        self.mag = torch.zeros(n, 3, dtype=torch.float64)  # sum |term| of columns 5..7
        self.switch, self.min_gap = switch.long(), math.inf
        self.sides = {k: 0 for k in ("lin_off", "lin_on", "yaw_off", "yaw_on", "steady", "early")}

    def accumulate(self, s):
        sample = (self.status == 0) & ~s["reset"].detach().cpu().bool()
        super().accumulate(s)
        d = lambda k: s[k].detach().cpu().double()  # noqa: E731
        c, v, w, pg = d("commands"), d("base_lin_vel"), d("base_ang_vel"), d("projected_gravity")
        k = s["episode_length"].detach().cpu().long() - self.switch
        on = sample & (self.switch > 0) & (k >= 0)
        err = torch.sqrt((c[:, 0] - v[:, 0]) ** 2 + (c[:, 1] - v[:, 1]) ** 2)
        yerr = (c[:, 2] - w[:, 2]).abs()
        tilt = torch.atan2(pg[:, :2].norm(dim=1), -pg[:, 2])
        st = on & (k >= STEADY)
        r = self.rec
        r[:, 0] += on.double()
        r[:, 1] = torch.where(on & (err > SETTLE_TOL), (k + 1).double(), r[:, 1])
        r[:, 2] = torch.where(on & (yerr > YAW_TOL), (k + 1).double(), r[:, 2])
        r[:, 3] = torch.where(on, torch.maximum(r[:, 3], tilt), r[:, 3])
        r[:, 4] += st.double()
        terms = torch.stack([v[:, 0], v[:, 1], w[:, 2]], 1) * st.double().view(-1, 1)
        r[:, 5:8] += terms
        self.mag += terms.abs()
        for name, m in (("lin_off", on & (err > SETTLE_TOL)), ("lin_on", on & (err <= SETTLE_TOL)),
                        ("yaw_off", on & (yerr > YAW_TOL)), ("yaw_on", on & (yerr <= YAW_TOL)), ("steady", st),
                        ("early", on & ~st)):
            self.sides[name] += int(m.sum())
        if bool(on.any()):
            gap = torch.minimum((err - SETTLE_TOL).abs() / SETTLE_TOL, (yerr - YAW_TOL).abs() / YAW_TOL)
            self.min_gap = min(self.min_gap, float(gap[on].min()))


def check_command_records(rec, ref, what=""):
    rec = rec.detach().cpu().double()
    for k, name in ((0, "post-switch samples"), (1, "linear settle step"), (2, "yaw settle step"), (4, "steady samples")):
        assert torch.equal(rec[:, k], ref.rec[:, k]), f"{what} cmd_rec[{k}] {name}"
    err = (rec[:, 3] - ref.rec[:, 3]).abs()
    print(f"{what} cmd_rec[3] max err {float(err.max()):.3e} (bound {4 * 2 ** -23 * math.pi:.3e})")
    assert bool((err <= 4 * 2 ** -23 * math.pi).all()), f"{what} cmd_rec[3] peak tilt"
    for j in range(3):
        err = (rec[:, 5 + j] - ref.rec[:, 5 + j]).abs()
        lim = ref.rec[:, 4] * 2 ** -23 * ref.mag[:, j]
        print(f"{what} cmd_rec[{5 + j}] worst err / bound {float((err / lim.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= lim).all()), f"{what} cmd_rec[{5 + j}]"


def command_cells_of(rec, status, cell_ids, rows_, cols):
    """lgx_eval_reduce's command cells restated: float64 torch sums of the given records per cell."""
    rec, status, cell = rec.detach().cpu().double(), status.detach().cpu().long(), cell_ids.detach().cpu().long()
    out = torch.zeros(rows_ * cols, 9, dtype=torch.float64)
    for c in range(rows_ * cols):
        m = (cell == c) & (status != 0) & (rec[:, 0] > 0)
        s = m & (status == 1)
        out[c] = torch.cat([torch.stack([m.sum().double(), s.sum().double(), rec[s, 1].sum(), rec[s, 2].sum(),
                                         rec[m, 3].sum()]), rec[s, 4:8].sum(0)])
    return out.reshape(rows_, cols, 9)


def scripted_env(n, device):
    env = make_env("go2", n, device)
    gen = torch.Generator().manual_seed(300 + n)
    steps, switch, cell_ids = command_script(n, gen)
    ev = env.cmd_eval_buffers(*GRID, SETTLE_TOL, YAW_TOL, STEADY)
    env.cmd_switch_step.copy_(switch)
    env.cmd_cell_ids.copy_(cell_ids)
    ref = CommandRestatement(n, env.dt, env.feet_indices, switch)
    env.cmd_rec.fill_(3.0)  # eval_begin zeroes it
    env.eval_begin(ev)
    for s in steps:
        E.write_inputs(env, s)
        env.projected_gravity.copy_(s["projected_gravity"])
        env.episode_length_buf = s["episode_length"]
        env.eval_accumulate(ev)
        ref.accumulate(s)
    return env, ev, ref


def records_and_cells(n, device):
    from legged_gym_custom_amd import _native
    env, ev, ref = scripted_env(n, device)
    assert ref.min_gap > 1e-4, ref.min_gap  # no scripted sample near a tolerance: no decision can tie
    if n >= 63:
        assert all(v > n // 4 for v in ref.sides.values()), ref.sides  # samples on both sides of all three
        assert float(ref.rec[:, 3].max()) > math.pi / 2
        assert ref.status[1] != 0 and ref.rec[1, 0] == 0 and ref.rec[2, 0] == 0 and ref.acc[2, 0] > 0
        assert int((ref.status == 0).sum()) > 0  # some envs never finish: they are in no command cell
    E.check_records(env.cmd_eval_acc, env.cmd_eval_status, ref, f"{device} n={n}")
    check_command_records(env.cmd_rec, ref, f"{device} n={n}")
    cells, ccells = env.eval_command_cells()
    assert env._cmd_eval_overflow.item() == 0
    assert cells.shape == GRID + (12,) and ccells.shape == GRID + (9,) and ccells.dtype == torch.float64
    ids = env.cmd_cell_ids.cpu().long()
    E.check_cells(cells, env.cmd_eval_acc, env.cmd_eval_status, ids // GRID[1], ids % GRID[1])
    want = command_cells_of(env.cmd_rec, env.cmd_eval_status, ids, *GRID)
    assert torch.equal(ccells[..., :2], want[..., :2]), "command cell counts"
    torch.testing.assert_close(ccells, want, rtol=1e-12, atol=0.0)
    again = env.eval_command_cells()
    assert torch.equal(again[0], cells) and torch.equal(again[1], ccells)  # fixed order, fixed tree
    # one cell id outside the grid: counted, never used as an index, both tables untouched
    env._cmd_eval_cells.fill_(-7.0)
    env._cmd_cells.fill_(-7.0)
    env.cmd_cell_ids[0] = GRID[0] * GRID[1]
    try:
        env._native.eval_reduce(ev, env._stream())  # (the host backend also fails the call)
    except _native.LgxError as e:
        assert device == "cpu" and "1 envs" in str(e)
    assert int(env._cmd_eval_overflow.item()) == 1
    assert bool((env._cmd_eval_cells == -7.0).all()) and bool((env._cmd_cells == -7.0).all())
    env.cmd_cell_ids[0] = int(ids[0])
    again = env.eval_command_cells()  # and usable again
    assert int(env._cmd_eval_overflow.item()) == 0
    assert torch.equal(again[0], cells) and torch.equal(again[1], ccells)
    return env, ref


# ------------------------------------------------------------------ 6. refusals
def refusals(device):
    import pytest
    from legged_gym_custom_amd import _native
    n = 8
    env = make_env("go2", n, device, **ON)
    top = int(env.max_episode_length)
    ok = torch.ones(2, 4)
    env.set_command_schedule([0, top - 1], ok)  # the last step of an episode is allowed
    env.set_command_schedule(torch.tensor([2, 2, 7, 9]).expand(n, 4), torch.ones(n, 4, 4))  # equal steps too
    before = (env.cmd_step.clone(), env.cmd_val.clone())
    nan, inf = float("nan"), float("inf")
    for bad_steps, bad_values in (([], torch.zeros(0, 4)), ([0, 1, 2, 3, 4], torch.zeros(5, 4)), ([0.0, 2.5], ok),
                                  ([0, 3], torch.ones(3, 4)), ([0, 3], torch.ones(2, 3)), ([0, 3], torch.ones(n - 1, 2, 4)),
                                  (torch.zeros(n - 1, 2, dtype=torch.int64), ok), ([3, 2], ok), ([-1, 2], ok),
                                  ([0, top], ok), ([0, 3], torch.tensor([[0.0, nan, 0.0, 0.0]] * 2)),
                                  ([0, 3], torch.tensor([[inf, 0.0, 0.0, 0.0]] * 2))):
        with pytest.raises(ValueError):
            env.set_command_schedule(bad_steps, bad_values)
    assert torch.equal(env.cmd_step, before[0]) and torch.equal(env.cmd_val, before[1])  # a refused call writes nothing
    env.set_command_schedule([4], torch.full((1, 4), 2.0))  # fewer segments: the rest are padded with -1
    assert env.cmd_step[0].tolist() == [4, -1, -1, -1] and env.cmd_val[0, 0].tolist() == [2.0] * 4
    env.clear_command_schedule()
    assert bool((env.cmd_step == -1).all())
    # lgx_bind refuses one pointer without the other, by name
    plain = make_env("go2", n, device)
    assert plain.cmd_step is None and plain.cmd_val is None
    plain.cmd_step = torch.full((n, 4), -1, dtype=torch.int32, device=device)
    with pytest.raises(_native.LgxError, match="cmd_step without cmd_val"):
        plain._bind()
    plain.cmd_step, plain.cmd_val = None, torch.zeros(n, 4, 4, device=device)
    with pytest.raises(_native.LgxError, match="cmd_val without cmd_step"):
        plain._bind()
    plain.cmd_val = None
    plain._bind()
    # lgx_eval_* refuses cmd_rec without cmd_switch_step or a buffer it needs, by name, and writes nothing
    ev = plain.cmd_eval_buffers(1, 2, 0.3, 0.3, 5)
    plain.cmd_rec.fill_(5.0)
    noswitch = plain._native.eval_buffers(plain.cmd_eval_acc, plain.cmd_eval_status, plain._cmd_eval_cells,
                                          plain._cmd_eval_overflow, cmd_rec=plain.cmd_rec)
    for call in (plain._native.eval_begin, plain._native.eval_accumulate, plain._native.eval_reduce):
        with pytest.raises(_native.LgxError, match="cmd_rec needs cmd_switch_step"):
            call(noswitch, plain._stream())
    keep = plain.projected_gravity
    plain.projected_gravity = None
    plain._bind()
    with pytest.raises(_native.LgxError, match="projected_gravity"):
        plain.eval_begin(ev)
    assert bool((plain.cmd_rec == 5.0).all())
    plain.projected_gravity = keep
    plain._bind()
    plain.eval_begin(ev)
    assert bool((plain.cmd_rec == 0.0).all())
    with pytest.raises(_native.LgxError, match="cmd_cells needs cmd_rec"):
        plain._native.eval_buffers(plain.cmd_eval_acc, plain.cmd_eval_status, plain._cmd_eval_cells,
                                   plain._cmd_eval_overflow, cmd_cells=plain._cmd_cells)
    for kw in ({"yaw_tol": -0.1}, {"yaw_tol": nan}, {"settle_tol": -1.0}, {"steady_after": -1}):
        with pytest.raises(_native.LgxError):
            plain._native.eval_buffers(plain.cmd_eval_acc, plain.cmd_eval_status, plain._cmd_eval_cells,
                                       plain._cmd_eval_overflow, cmd_switch_step=plain.cmd_switch_step,
                                       cmd_rec=plain.cmd_rec, **kw)


def evaluator(n, device, **over):
    from legged_gym_custom_amd.utils.evaluator import PolicyEvaluator
    over.setdefault("env.episode_length_s", 0.59)  # ceil(0.59 / 0.02) = 30 steps
    env, tcfg, args = E.make_env("go2", n, device, **over)
    assert int(env.max_episode_length) == 30
    return PolicyEvaluator(env, E.make_runner(env, tcfg, args), policy="student")


def command_test_refusals(device):
    import pytest
    ev = evaluator(8, device, **ON)
    for at in (0.0, 0.004, 0.6, 5.0, -1.0, float("nan")):  # steps 0, 0, 30 (= max_episode_length), 250, -50
        with pytest.raises(ValueError, match="at_s"):
            ev.run_command_test([1.0], at_s=at)
    for kw in (dict(vx=[]), dict(vx=[1.0], vy=[]), dict(vx=[1.0], yaw=[]), dict(vx=[float("inf")]),
               dict(vx=[1.0], yaw=[float("nan")]), dict(vx=[1.0], start=(0.0, 0.0)), dict(vx=[1.0], settle_tol=-0.1),
               dict(vx=[1.0], yaw_tol=-0.1), dict(vx=[1.0], steady_after_s=-1.0)):
        with pytest.raises(ValueError):
            ev.run_command_test(**{"at_s": 0.1, **kw})
    assert bool((ev.env.cmd_step == -1).all())


# ------------------------------------------------------------------ 7. evaluator end to end
def end_to_end(device):
    """run_command_test on 64 envs, 30-step episodes, vx [0, 1] x yaw [0, 0.5], switched at step 5,
    steady from 3 steps on, 40 steps. On the GPU the first evaluator replays its captured loop and
    the second runs eagerly; on the host both run eagerly."""
    import json
    from legged_gym_custom_amd.utils.evaluator import REPORT_KEYS
    n, vx, yaw = 64, [0.0, 1.0], [0.0, 0.5]
    a, b, fresh = evaluator(n, device, **ON), evaluator(n, device, **ON), evaluator(n, device)
    gpu, dt = device != "cpu", float(a.env.dt)
    kw = dict(yaw=yaw, at_s=5 * dt, steady_after_s=3 * dt, num_steps=40)
    ra = a.run_command_test(vx, **kw)
    cells, ccells, bins = a.last_cells.clone(), a.last_cmd_cells.clone(), a.last_cmd_bins.clone()
    assert ra["graph"] is gpu and ra["num_steps"] == 40 and ra["switch_step"] == 5 and ra["steady_after"] == 3
    assert ra["vx"] == vx and ra["vy"] == [0.0] and ra["yaw"] == yaw and ra["total"]["running"] == 0
    rb = b.run_command_test(vx, graph=False, **kw)
    assert rb["graph"] is False
    assert torch.equal(b.last_cells, cells) and torch.equal(b.last_cmd_cells, ccells)  # replay = eager loop
    a.run_command_test(vx, **kw)
    assert torch.equal(a.last_cells, cells) and torch.equal(a.last_cmd_cells, ccells)  # and it repeats
    if gpu:
        assert a._cmd_graph is not None and a._graph is None  # a graph of its own, captured once
    # the bins: randperm % 4, every env in its bin, its schedule {0: start, 5: the bin's command}
    want = torch.bincount(bins, minlength=4)
    assert int(want.max() - want.min()) <= 1 and int(want.sum()) == n
    assert torch.equal(cells[..., 0].reshape(-1).long(), want) and cells.shape == (2, 2, 12) and ccells.shape == (2, 2, 9)
    env = a.env
    assert torch.equal(env.cmd_cell_ids.cpu().long(), bins) and bool((env.cmd_switch_step == 5).all())
    grid = torch.tensor([[x, 0.0, w, 0.0] for x in vx for w in yaw])
    assert torch.equal(env.cmd_val.cpu()[:, 1], grid[bins]) and bool((env.cmd_val[:, 0] == 0).all())
    assert sum(c["episodes"] + c["running"] for row in ra["bins"] for col in row for c in col) == n
    assert all(c["switched"] <= c["episodes"] + c["running"] for row in ra["bins"] for col in row for c in col)
    fin = (env.cmd_eval_status != 0) & (env.cmd_rec[:, 0] > 0)
    assert int(ccells[..., 0].sum()) == int(fin.sum()) == ra["total"]["switched"] and int(fin.sum()) > 0
    torch.testing.assert_close(ccells, command_cells_of(env.cmd_rec, env.cmd_eval_status, bins, 2, 2), rtol=1e-12, atol=0.0)
    assert float(env.cmd_rec[:, 0].max()) <= 26.0  # steps 5..30 of an env that ran to its time-out at step 31
    # the report: documented keys, no NaN anywhere (None where there is no data)
    keys = set(REPORT_KEYS) | {"switched", "survivors", "mean_settle_s", "mean_yaw_settle_s", "mean_peak_tilt_rad"}
    assert keys <= set(ra["total"]) and all(keys | {"achieved", "gain"} <= set(c) for row in ra["bins"] for col in row for c in col)
    assert len(ra["bins"]) == 2 and len(ra["bins"][0]) == 1 and len(ra["bins"][0][0]) == 2
    assert all(c["gain"] is None for c in ra["bins"][0][0]) and "NaN" not in json.dumps(ra)
    for c in ra["bins"][1][0]:
        assert (c["gain"] is None) == (c["achieved"] is None)
        if c["achieved"] is not None:
            assert c["gain"] == c["achieved"][0] / 1.0
    # afterwards: no schedule, and the plain evaluation is a fresh evaluator's, bit for bit
    assert bool((env.cmd_step == -1).all())
    a.run()
    fresh.run()
    assert fresh.env.cmd_step is None and torch.equal(a.last_cells, fresh.last_cells)
    assert float(fresh.last_cells[..., 4].sum()) > 0
