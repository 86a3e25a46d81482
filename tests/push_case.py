"""Shared by tests/test_gpu_push.py (device "cuda:0") and tests/test_push_host.py (the same bodies
on the host backend): the scheduled push of the env step (lgx_buffers.push_step / push_dvel) and
the push-recovery evaluation (lgx_eval_buffers.cell_ids / push_rec / push_cells), include/lgx.h ABI 9.

The feature has no oracle. Every test reduces it to feature-off behaviour, which the oracle and
the golden fixtures pin:
  * a scheduled push is an edit of three root velocity entries at the end of one step: an env with
    a schedule against one without, rows that were not pushed bit for bit, pushed rows bit for bit
    except root_states[:, 7:9] / [:, 12], which equal the unpushed env's plus the impulse computed
    in float64 torch from its quaternion; the pushed rows are then copied over, so every later step
    compares bit for bit again;
  * with no env scheduled, the bound buffers change nothing;
  * the records and cells are compared with a float64 torch restatement on scripted inputs.
Bounds: the impulse 2e-6 (|a| + |b| + |v|) per element: about 10 roundings of 2^-24 in the frame
construction (quat_apply, norm, two divisions, two products and a difference) plus the final add,
with a 3x margin; records rtol 1e-5 (tests/eval_case.py: fp32 record columns; here a maximum of
single fp32 expressions, error a few 2^-24); counts, rec[0] and rec[3] exact: the scripted
inputs keep every tracking error more than 1e-4 (relative) away from settle_tol, 800x the fp32
error of err, so the rec[3] decision cannot tie. Kernel against host backend: tests/actuator_case.py.

Measured worst differences (each test prints its own) are recorded in DESIGN.md section 4.7."""
import math

import torch

import eval_case as E
from actuator_case import DEFAULT_TOL, DISCRETE, PHYSICS, TOL, assert_equal, bound, copy_state, make_env, worst_ratio

assert DEFAULT_TOL and TOL  # (the bounds worst_ratio applies)
ON = {"domain_rand.scheduled_pushes": True}
GLOBAL = ("kp_kd", "episode_stats", "blowup_count")  # bound buffers that are not one row per env
GRID = (3, 4)
SETTLE_TOL = 1.0  # m/s; the scripted errors are |randn - randn| in two components (median about 1.7)


def rows(t, n):
    """A bound per-env tensor as [n, -1] (a view: rigid_body_states is [n * bodies, 13])."""
    return t.view(n, -1)


def per_env(bx, by):
    return [k for k in by if k in bx and k not in GLOBAL]


def heading_impulse(quat, dvel):
    """The rule of include/lgx.h in float64: (d root[7], d root[8], d root[12])."""
    q, d = quat.detach().cpu().double(), dvel.detach().cpu().double()
    x, y, z, w = q.unbind(1)
    fx, fy = 1.0 - 2.0 * (y * y + z * z), 2.0 * (w * z + x * y)  # quat_apply(q, (1, 0, 0))
    nrm = torch.sqrt(fx * fx + fy * fy)
    ok = nrm > 1e-6
    hx, hy = torch.where(ok, fx / nrm, torch.ones_like(fx)), torch.where(ok, fy / nrm, torch.zeros_like(fy))
    a, b, c = d.unbind(1)
    return torch.stack([a * hx - b * hy, a * hy + b * hx, c], 1)


def schedule(n, gen, lo=0, span=7):
    step = lo + torch.arange(n) * 5 % span
    return step, 0.5 * torch.randn(n, 3, generator=gen)


# ------------------------------------------------------------------ 1. a scheduled push is a velocity edit
def velocity_edit(n, device):
    X, Y = make_env("go2", n, device, **ON), make_env("go2", n, device)
    assert X.push_step is not None and X.push_step.dtype == torch.int32 and Y.push_step is None
    gen = torch.Generator().manual_seed(11)
    step, dvel = schedule(n, gen)
    assert int((step == 0).sum()) > 0
    X.reset()
    Y.reset()
    # envs 6 and 13 (push_step 2) start upside down: they reset in the very step that would push them
    for env in (X, Y):
        env.root_states[[6, 13], 3:7] = torch.tensor([1.0, 0.0, 0.0, 0.0], device=device)
    X.set_push_schedule(step.to(device), dvel.to(device))
    assert step[6] == 2 and step[13] == 2 and int(X.episode_length_buf[0]) == 1
    assert_equal(bound(X), bound(Y), per_env(bound(X), bound(Y)), "after reset")
    keep = ("root_states",)
    same_when_pushed = tuple(DISCRETE) + ("obs", "base_lin_vel") + tuple(k for k in PHYSICS if k not in keep)
    npushed, nreset, lost, worst = torch.zeros(n, dtype=torch.bool), 0, 0, 0.0
    for t in range(12):
        a = (0.3 * torch.randn(n, X.num_actions, generator=gen)).to(device)
        X.step(a.clone())
        Y.step(a.clone())
        bx, by = bound(X), bound(Y)
        names = per_env(bx, by)
        assert torch.equal(X.reset_buf, Y.reset_buf)
        pushed = ((X.episode_length_buf == X.push_step) & ~X.reset_buf).cpu()
        nreset += int(X.reset_buf.sum())
        lost += int((X.reset_buf.cpu() & (step == 2) & (t == 0)).sum())
        assert_equal(bx, by, [k for k in GLOBAL if k in bx and k in by], f"step {t} global")
        for k in names:  # rows that were not pushed: every per-env buffer, bit for bit
            assert torch.equal(rows(bx[k], n).cpu()[~pushed], rows(by[k], n).cpu()[~pushed]), (t, k)
        if bool(pushed.any()):
            for k in same_when_pushed:
                if k in by:
                    assert torch.equal(rows(bx[k], n).cpu()[pushed], rows(by[k], n).cpu()[pushed]), (t, k, "pushed rows")
            rx, ry = X.root_states.cpu()[pushed], Y.root_states.cpu()[pushed]
            other = [i for i in range(13) if i not in (7, 8, 12)]
            assert torch.equal(rx[:, other], ry[:, other]), (t, "root_states outside the pushed entries")
            d = dvel[pushed].double()
            v = ry[:, [7, 8, 12]].double()
            want = v + heading_impulse(ry[:, 3:7], dvel[pushed])
            err = (rx[:, [7, 8, 12]].double() - want).abs()
            lim = 2e-6 * (d[:, 0:1].abs() + d[:, 1:2].abs() + v.abs())
            worst = max(worst, float((err / lim).max()))
            assert bool((err <= lim).all()), (t, float((err / lim).max()))
            assert torch.equal(rx[:, 12], ry[:, 12] + dvel[pushed][:, 2])  # one fp32 add
            assert float((rx[:, 7:9] - ry[:, 7:9]).abs().max()) > 1e-3  # and it is an edit
            for k in names:  # X's pushed rows onto Y: later steps compare bit for bit again
                rows(by[k], n)[pushed.to(device)] = rows(bx[k], n)[pushed.to(device)]
        npushed |= pushed
    print(f"push n={n} {device}: {int(npushed.sum())} envs pushed, {nreset} resets, worst impulse error "
          f"{worst:.3f} x the bound (2e-6 (|a| + |b| + |v|))")
    assert int(npushed.sum()) >= n // 2 and nreset >= 1 and lost == 2
    return worst


# ------------------------------------------------------------------ 2. identity
def identity(device):
    n = 64
    X, Y = make_env("go2", n, device, **ON), make_env("go2", n, device)
    X.set_push_schedule(0, torch.ones(3))
    X.push_step[5] = 500  # beyond the run
    assert "push_step" in bound(X) and "push_step" not in bound(Y)
    X.reset()
    Y.reset()
    gen = torch.Generator().manual_seed(12)
    for t in range(8):
        a = torch.randn(n, X.num_actions, generator=gen).to(device)
        X.step(a.clone())
        Y.step(a.clone())
        bx, by = bound(X), bound(Y)
        assert_equal(bx, by, [k for k in by if k in bx], f"step {t}")
    X.clear_push_schedule()
    assert int(X.push_step.abs().sum()) == 0
    Y.clear_push_schedule()  # a no-op without the buffers
    assert Y.push_step is None


# ------------------------------------------------------------------ 3. the device's backend against the host backend
def backend_vs_host(n, device):
    X, Yh = make_env("go2", n, device, **ON), make_env("go2", n, "cpu", **ON)
    gen = torch.Generator().manual_seed(13)
    step, dvel = schedule(n, gen, lo=2, span=15)  # every env is pushed within the 16 steps
    for env in (X, Yh):
        env.reset()
        env.set_push_schedule(step.to(env.device), dvel.to(env.device))
    cont = PHYSICS + ("obs", "rew", "last_dof_vel", "last_torques", "commands", "last_root_vel")
    worst, npushed = {}, 0
    for t in range(16):
        a = 0.3 * torch.randn(n, X.num_actions, generator=gen)
        copy_state(X, Yh)
        Yh.common_step_counter = X.common_step_counter
        X.step(a.to(device))
        Yh.step(a.clone())
        bx, by = bound(X), bound(Yh)
        assert_equal(bx, by, [k for k in DISCRETE if k in bx] + ["last_actions", "actions", "push_step", "push_dvel"],
                     f"step {t}")
        r = worst_ratio(bx, by, cont, worst)
        assert r <= 1.0, (t, r, worst)
        npushed += int(((X.episode_length_buf == X.push_step) & ~X.reset_buf).sum())
    print(f"push go2 n={n} {device} vs host, schedule on:", {k: f"{v:.1e}" for k, v in worst.items() if v > 0})
    assert npushed >= n - 2
    return worst


# ------------------------------------------------------------------ 4. records and cells
def push_script(n, gen):
    """eval_case.script extended with projected_gravity (unit vectors, some past 90 degrees) and
    episode_length per call, a push_step in 0..3 and random cell ids on the GRID."""
    steps = E.script(n, gen)
    for t, s in enumerate(steps):
        pg = torch.randn(n, 3, generator=gen)
        s["projected_gravity"] = pg / pg.norm(dim=1, keepdim=True)
        s["episode_length"] = t + 1 + torch.arange(n) % 2
    push_step = torch.randint(0, 4, (n,), generator=gen).to(torch.int32)
    cell_ids = torch.randint(0, GRID[0] * GRID[1], (n,), generator=gen).to(torch.int32)
    return steps, push_step, cell_ids


class PushRestatement(E.Restatement):
    """lgx_eval_accumulate's push-recovery record in float64 torch, next to the plain record."""

    def __init__(self, n, dt, feet, push_step, settle_tol):
        super().__init__(n, dt, feet)
        self.rec = torch.zeros(n, 4, dtype=torch.float64)
        self.push_step, self.tol, self.min_gap = push_step.long(), float(settle_tol), math.inf

    def accumulate(self, s):
        sample = (self.status == 0) & ~s["reset"].detach().cpu().bool()
        super().accumulate(s)
        d = lambda k: s[k].detach().cpu().double()  # noqa: E731
        c, v, pg = d("commands"), d("base_lin_vel"), d("projected_gravity")
        k = s["episode_length"].detach().cpu().long() - self.push_step
        on = sample & (self.push_step > 0) & (k > 0)
        err = torch.sqrt((c[:, 0] - v[:, 0]) ** 2 + (c[:, 1] - v[:, 1]) ** 2)
        tilt = torch.atan2(pg[:, :2].norm(dim=1), -pg[:, 2])
        r = self.rec
        r[:, 0] += on.double()
        r[:, 1] = torch.where(on, torch.maximum(r[:, 1], tilt), r[:, 1])
        r[:, 2] = torch.where(on, torch.maximum(r[:, 2], err), r[:, 2])
        r[:, 3] = torch.where(on & (err > self.tol), k.double(), r[:, 3])
        if bool(on.any()):
            self.min_gap = min(self.min_gap, float(((err - self.tol).abs() / self.tol)[on].min()))


def check_push_records(rec, ref, what=""):
    rec = rec.detach().cpu().double()
    assert torch.equal(rec[:, 0], ref.rec[:, 0]), f"{what} post-push sample counts"
    assert torch.equal(rec[:, 3], ref.rec[:, 3]), f"{what} last step off the command"
    for k in (1, 2):
        err = (rec[:, k] - ref.rec[:, k]).abs()
        print(f"{what} push_rec[{k}] max rel err {float((err / ref.rec[:, k].clamp_min(1e-300)).max()):.3e}")
        assert bool((err <= 1e-5 * ref.rec[:, k].abs()).all()), f"{what} push_rec[{k}]"


def push_cells_of(rec, status, cell_ids, rows_, cols):
    """lgx_eval_reduce's push cells restated: float64 torch sums of the given records per cell."""
    rec, status, cell = rec.detach().cpu().double(), status.detach().cpu().long(), cell_ids.detach().cpu().long()
    out = torch.zeros(rows_ * cols, 5, dtype=torch.float64)
    for c in range(rows_ * cols):
        m = (cell == c) & (status != 0) & (rec[:, 0] > 0)
        surv = m & (status == 1)
        out[c] = torch.stack([m.sum().double(), rec[m, 1].sum(), rec[m, 2].sum(), surv.sum().double(), rec[surv, 3].sum()])
    return out.reshape(rows_, cols, 5)


def scripted_env(n, device):
    env = make_env("go2", n, device, **ON)
    gen = torch.Generator().manual_seed(200 + n)
    steps, push_step, cell_ids = push_script(n, gen)
    ev = env.push_eval_buffers(*GRID, SETTLE_TOL)
    env.push_step.copy_(push_step)
    env.push_cell_ids.copy_(cell_ids)
    ref = PushRestatement(n, env.dt, env.feet_indices, push_step, SETTLE_TOL)
    env.push_rec.fill_(3.0)  # eval_begin zeroes it
    env.eval_begin(ev)
    for s in steps:
        E.write_inputs(env, s)
        env.projected_gravity.copy_(s["projected_gravity"])
        env.episode_length_buf = s["episode_length"]
        env.eval_accumulate(ev)
        ref.accumulate(s)
    return env, ev, ref


def records_and_cells(n, device):
    env, ev, ref = scripted_env(n, device)
    assert ref.min_gap > 1e-4, ref.min_gap  # no scripted sample near settle_tol: rec[3] cannot tie
    if n >= 63:
        assert int((ref.rec[:, 0] > 0).sum()) > n // 4 and int((ref.rec[:, 3] > 0).sum()) > 0
        assert float(ref.rec[:, 1].max()) > math.pi / 2 and int(((ref.rec[:, 0] > 0) & (ref.rec[:, 3] == 0)).sum()) > 0
    E.check_records(env.push_eval_acc, env.push_eval_status, ref, f"{device} n={n}")
    check_push_records(env.push_rec, ref, f"{device} n={n}")
    cells, pcells = env.eval_push_cells()
    assert cells.shape == GRID + (12,) and pcells.shape == GRID + (5,) and pcells.dtype == torch.float64
    ids = env.push_cell_ids.cpu().long()
    E.check_cells(cells, env.push_eval_acc, env.push_eval_status, ids // GRID[1], ids % GRID[1])
    want = push_cells_of(env.push_rec, env.push_eval_status, ids, *GRID)
    assert torch.equal(pcells[..., [0, 3]], want[..., [0, 3]]), "push cell counts"
    torch.testing.assert_close(pcells, want, rtol=1e-12, atol=0.0)
    again = env.eval_push_cells()
    assert torch.equal(again[0], cells) and torch.equal(again[1], pcells)  # fixed order, fixed tree
    # one cell id outside the grid: counted, never used as an index, both tables untouched
    from legged_gym_custom_amd import _native
    env._push_eval_cells.fill_(-7.0)
    env._push_cells.fill_(-7.0)
    env.push_cell_ids[n // 2] = GRID[0] * GRID[1]
    try:
        env._native.eval_reduce(ev, env._stream())  # (the host backend also fails the call)
    except _native.LgxError as e:
        assert device == "cpu" and "1 envs" in str(e)
    assert int(env._push_eval_overflow.item()) == 1
    assert bool((env._push_eval_cells == -7.0).all()) and bool((env._push_cells == -7.0).all())
    env.push_cell_ids[n // 2] = -1
    try:
        env.eval_push_cells()
        raise AssertionError("a negative cell id went through")
    except _native.LgxError as e:
        assert "1 envs" in str(e)
    assert bool((env._push_eval_cells == -7.0).all()) and bool((env._push_cells == -7.0).all())
    env.push_cell_ids[n // 2] = int(ids[n // 2])
    again = env.eval_push_cells()  # and usable again
    assert torch.equal(again[0], cells) and torch.equal(again[1], pcells)
    return env, ref


# ------------------------------------------------------------------ 6. refusals
def refusals(device):
    import pytest
    from legged_gym_custom_amd import _native
    n = 8
    env = make_env("go2", n, device, **ON)
    top = int(env.max_episode_length)
    env.set_push_schedule(top, torch.zeros(3))  # the last step of an episode is allowed
    env.set_push_schedule(torch.full((n,), 3, dtype=torch.int64), torch.ones(n, 3))
    before = (env.push_step.clone(), env.push_dvel.clone())
    for bad_step, bad_dvel in ((torch.zeros(n - 1, dtype=torch.int32), torch.zeros(3)), (2.5, torch.zeros(3)),
                               (3, torch.zeros(2)), (3, torch.zeros(n - 1, 3)), (3, torch.zeros(n, 4)),
                               (torch.zeros(n, 1, dtype=torch.int32), torch.zeros(3)),
                               (top + 1, torch.zeros(3)), (3, torch.tensor([0.0, float("nan"), 0.0])),
                               (3, torch.tensor([float("inf"), 0.0, 0.0]))):
        with pytest.raises(ValueError):
            env.set_push_schedule(bad_step, bad_dvel)
    assert torch.equal(env.push_step, before[0]) and torch.equal(env.push_dvel, before[1])  # a refused call writes nothing
    env.clear_push_schedule()
    assert int(env.push_step.abs().sum()) == 0 and torch.equal(env.push_dvel, before[1])
    # lgx_bind refuses one pointer without the other, by name
    plain = make_env("go2", n, device)
    assert plain.push_step is None and plain.push_dvel is None
    plain.push_step = torch.zeros(n, dtype=torch.int32, device=device)
    with pytest.raises(_native.LgxError, match="push_step without push_dvel"):
        plain._bind()
    plain.push_step, plain.push_dvel = None, torch.zeros(n, 3, device=device)
    with pytest.raises(_native.LgxError, match="push_dvel without push_step"):
        plain._bind()
    plain.push_dvel = None
    plain._bind()
    # lgx_eval_* refuses push_rec while a buffer it needs is not bound, by name, and writes nothing
    ev = plain.push_eval_buffers(1, 2, 0.3)
    plain.push_rec.fill_(5.0)
    for call in (plain._native.eval_begin, plain._native.eval_accumulate, plain._native.eval_reduce):
        with pytest.raises(_native.LgxError, match="push_step"):
            call(ev, plain._stream())
    plain.set_push_schedule(0, torch.zeros(3))  # allocates and re-binds (nothing was captured)
    keep = plain.projected_gravity
    plain.projected_gravity = None
    plain._bind()
    with pytest.raises(_native.LgxError, match="projected_gravity"):
        plain.eval_begin(ev)
    assert bool((plain.push_rec == 5.0).all())
    plain.projected_gravity = keep
    plain._bind()
    plain.eval_begin(ev)
    assert bool((plain.push_rec == 0.0).all())
    with pytest.raises(_native.LgxError, match="push_cells needs push_rec"):
        plain._native.eval_buffers(plain.push_eval_acc, plain.push_eval_status, plain._push_eval_cells,
                                   plain._push_eval_overflow, push_cells=plain._push_cells)


def evaluator(n, device, **over):
    from legged_gym_custom_amd.utils.evaluator import PolicyEvaluator
    over.setdefault("env.episode_length_s", 0.19)  # ceil(0.19 / 0.02) = 10 steps
    env, tcfg, args = E.make_env("go2", n, device, **over)
    assert int(env.max_episode_length) == 10
    return PolicyEvaluator(env, E.make_runner(env, tcfg, args), policy="student")


def push_test_refusals(device):
    import pytest
    ev = evaluator(8, device, **ON)
    for at in (0.0, 0.004, 0.2, 5.0, -1.0, float("nan")):  # steps 0, 0, 10 (= max_episode_length), 250, -50
        with pytest.raises(ValueError, match="at_s"):
            ev.run_push_test([1.0], directions=4, at_s=at)
    for speeds, dirs in (([], 4), ([1.0], 0), ([-0.5], 4), ([float("inf")], 4)):
        with pytest.raises(ValueError):
            ev.run_push_test(speeds, directions=dirs, at_s=0.06)
    assert int(ev.env.push_step.abs().sum()) == 0


# ------------------------------------------------------------------ 5. evaluator end to end
def end_to_end(device):
    """run_push_test on 66 envs, 10-step episodes, 2 speeds x 4 directions, pushed at step 3. On the
    GPU the first evaluator replays its captured loop and the second runs eagerly; on the host both
    run eagerly."""
    import json
    from legged_gym_custom_amd.utils.evaluator import REPORT_KEYS
    n, speeds, dirs = 66, [0.0, 1.0], 4
    a, b, fresh = evaluator(n, device, **ON), evaluator(n, device, **ON), evaluator(n, device)
    gpu = device != "cpu"
    ra = a.run_push_test(speeds, directions=dirs, at_s=0.06)
    cells, pcells, bins = a.last_cells.clone(), a.last_push_cells.clone(), a.last_push_bins.clone()
    assert ra["graph"] is gpu and ra["num_steps"] == 11 and ra["push_step"] == 3 and ra["total"]["running"] == 0
    assert ra["speeds"] == speeds and ra["directions_deg"] == [0.0, 90.0, 180.0, 270.0]
    rb = b.run_push_test(speeds, directions=dirs, at_s=0.06, graph=False)
    assert rb["graph"] is False
    assert torch.equal(b.last_cells, cells) and torch.equal(b.last_push_cells, pcells)  # replay = eager loop
    a.run_push_test(speeds, directions=dirs, at_s=0.06)
    assert torch.equal(a.last_cells, cells) and torch.equal(a.last_push_cells, pcells)  # and it repeats
    if gpu:
        assert a._push_graph is not None and a._graph is None  # a graph of its own, captured once
    # the bins: randperm % (S * D), sizes within one of each other, every env in its bin
    want = torch.bincount(bins, minlength=len(speeds) * dirs)
    assert int(want.max() - want.min()) <= 1 and int(want.sum()) == n
    assert torch.equal(cells[..., 0].reshape(-1).long(), want) and cells.shape == (len(speeds), dirs, 12)
    env = a.env
    assert torch.equal(env.push_cell_ids.cpu().long(), bins)
    th = 2 * math.pi * (bins % dirs).double() / dirs
    sp = torch.tensor(speeds, dtype=torch.float64)[bins // dirs]
    assert torch.allclose(env.push_dvel.cpu().double(), torch.stack([sp * th.cos(), sp * th.sin(), 0 * sp], 1), atol=1e-7)
    # the push cells count the finished envs that have post-push samples
    fin = (env.push_eval_status != 0) & (env.push_rec[:, 0] > 0)
    assert int(pcells[..., 0].sum()) == int(fin.sum()) and int(fin.sum()) > n // 2
    torch.testing.assert_close(pcells, push_cells_of(env.push_rec, env.push_eval_status, bins, len(speeds), dirs),
                               rtol=1e-12, atol=0.0)
    assert float(env.push_rec[:, 0].max()) == 7.0  # steps 4..10 of an env that ran to its time-out at step 11
    # the pushed rows were shoved harder than the control row
    assert float(pcells[1, :, 2].sum() / pcells[1, :, 0].sum()) > float(pcells[0, :, 2].sum() / pcells[0, :, 0].sum())
    # the report: documented keys, no NaN anywhere (None where there is no data)
    keys = set(REPORT_KEYS) | {"pushed", "mean_peak_tilt_rad", "mean_peak_lin_vel_err", "survivors", "mean_settle_s"}
    assert keys <= set(ra["total"]) and all(keys <= set(c) for row in ra["bins"] for c in row)
    assert len(ra["bins"]) == len(speeds) and len(ra["bins"][0]) == dirs
    assert "NaN" not in json.dumps(ra) and ra["total"]["pushed"] == int(fin.sum())
    # afterwards: no schedule, and the plain evaluation is a fresh evaluator's, bit for bit
    assert int(env.push_step.abs().sum()) == 0
    a.run()
    fresh.run()
    assert fresh.env.push_step is None and torch.equal(a.last_cells, fresh.last_cells)
    assert float(fresh.last_cells[..., 4].sum()) > 0
