"""Shared by tests/test_joint_host.py and tests/test_gpu_joint.py: the joint-load record (include/lgx.h
ABI 13: lgx_joint_begin / lgx_joint_record / lgx_joint_reduce) on one device. A scripted sequence of
inputs written straight into the env's tensors (no physics step, the style of gait_case.py), a
restatement of the rule text in plain Python lists of float64, and the test bodies, parameterised by
the device.

Bounds (from the number formats, not from the code under test; u = 2^-24):
* joint columns 0, 10 and 11 are copies, 3 and 7 maxima of |copies|, 1, 8, 9, 13 and 14 counts below
  2^24 of comparisons of copies (p < 0 is decided by the signs of tau and qd unless the product
  underflows, which the scripts' magnitudes exclude); body 0, 2 and 3 are counts: all exact.
* columns 2 and 15 are fp32 running sums of T non-negative terms with at most one rounding per term
  (tau*tau; |qd| has none), columns 4, 5 and 12 with at most two (the product tau*qd, then * dt;
  the difference a - r0, then its square): relative error at most (T + 2) u for all five, T being the
  restatement's count of the entry's non-zero terms (a zero term adds nothing and rounds nothing).
* column 6 is a maximum of fp32 products: relative error at most u, bound 2 u.
* body 1 is a maximum of P, a sum of 16 non-negative products by a tree of depth four: one rounding
  per product and four levels, relative error at most 5 u, bound 6 u.
* cells: the sums are fp64 sums of at most 130 fp32 records by a fixed tree: against the float64 sum
  of the device's own records, |error| <= 1e-12 sum |term|. The env count and every maximum /
  minimum column are order-independent: exactly equal."""
import math
import types

import pytest
import torch

import eval_case as E
from legged_gym_custom_amd import _abi, _native

CALLS, D = 12, 12
U = 2.0 ** -24
EXACT = [0, 1, 3, 7, 8, 9, 10, 11, 13, 14]
SUMS = [2, 4, 5, 12, 15]
BODY_EXACT = [0, 2, 3]
NCOL = _abi.JOINT_CELL_COLS
SOURCES = ("torques", "dof_state", "actions", "reset", "time_out", "blew_up")
INF = float("inf")


def limits(env):
    """The record's limits as the library holds them (fp32 values of lgx_task_params), CPU tensors."""
    p = env._native.params
    f = lambda v: torch.tensor(list(v), dtype=torch.float32)  # noqa: E731
    pos = torch.tensor([[p.dof_pos_limits[j][0], p.dof_pos_limits[j][1]] for j in range(D)], dtype=torch.float32)
    return types.SimpleNamespace(L=f(p.torque_limits)[:D], V=f(p.dof_vel_limits)[:D], lo=pos[:, 0], hi=pos[:, 1],
                                 C=torch.tensor(p.clip_actions, dtype=torch.float32), dt=float(p.dt),
                                 num_actions=int(p.num_actions))


def _next(x, towards):
    return torch.nextafter(x, torch.tensor(towards, dtype=torch.float32))


def edge_env(n):
    """The env that carries the planted edges: it records every call but the last, where it times out."""
    return 1 if n >= 63 else 0


def script(n, gen, lim, calls=CALLS, scripted=True):
    """`calls` steps of inputs (CPU tensors): torques randn x 20 N m, angles over 1.2 x the soft range
    about its middle, speeds randn x half the speed limit, actions randn x 0.4 x clip_actions, so that
    every counter sees events. For n >= 63 (and scripted): env 0 resets at the first call (no sample);
    env 1 times out at the last call; env 2 falls at call 5; env 3 falls at call 2 and resets again at
    call 6; env 4 blows up at call 4 with time_out also set; env 5 never resets; the rest reset once
    at a random call, half of them as time-outs. A single env times out at the last call.

    The edge env (edge_env(n); scripted only) has small inputs (a tenth of each limit, angles in the
    middle half of the range) except for the planted edges, by joint and call:
      joint 0  torque     L, -nextafter(L, 0), -L               -> 2 saturated samples
      joint 1  speed      V, nextafter(V, inf), -nextafter(V, inf)  -> 2 samples over the speed limit
      joint 2  angle      lo, hi, nextafter(lo, -inf), nextafter(hi, inf)  -> 2 samples out of range
      joint 3  action     C, -C, nextafter(C, 0)                -> 2 clipped samples
      joint 4  (torque, speed)  (2, 3), (2, -3), (0, 3), then torque 0  -> p > 0, p < 0, p = 0"""
    steps = []
    when = torch.randint(0, calls, (n,), generator=gen)
    as_timeout = torch.rand(n, generator=gen) < 0.5
    fixed = scripted and n >= 63
    mid, half = 0.5 * (lim.lo + lim.hi), 0.5 * (lim.hi - lim.lo)
    ee = edge_env(n)
    for t in range(calls):
        u = lambda *s: 2.0 * torch.rand(*s, generator=gen) - 1.0  # noqa: E731
        tq = 20.0 * torch.randn(n, D, generator=gen)
        q = mid + 1.2 * half * u(n, D)
        qd = 0.5 * lim.V * torch.randn(n, D, generator=gen)
        act = 0.4 * lim.C * torch.randn(n, D, generator=gen)
        reset = when == t
        tout = reset & as_timeout
        blew = torch.zeros(n, dtype=torch.bool)
        if scripted and n < 63:
            reset[:] = tout[:] = t == calls - 1
        if fixed:
            reset[:6] = torch.tensor([t == 0, t == calls - 1, t == 5, t in (2, 6), t == 4, False])
            tout[:6] = torch.tensor([False, t == calls - 1, False, False, t == 4, False])
            blew[4] = t == 4
        if scripted:
            tq[ee], q[ee], qd[ee], act[ee] = 0.1 * lim.L * u(D), mid + 0.5 * half * u(D), 0.1 * lim.V * u(D), 0.1 * lim.C * u(D)
            L, V, lo, hi, C = lim.L[0], lim.V[1], lim.lo[2], lim.hi[2], lim.C
            tq[ee, 0] = [L, -_next(L, 0.0), -L][t] if t < 3 else tq[ee, 0]
            qd[ee, 1] = [V, _next(V, INF), -_next(V, INF)][t] if t < 3 else qd[ee, 1]
            q[ee, 2] = [lo, hi, _next(lo, -INF), _next(hi, INF)][t] if t < 4 else q[ee, 2]
            act[ee, 3] = [C, -C, _next(C, 0.0)][t] if t < 3 else act[ee, 3]
            tq[ee, 4] = [2.0, 2.0, 0.0][t] if t < 3 else 0.0
            qd[ee, 4] = [3.0, -3.0, 3.0][t] if t < 3 else qd[ee, 4]
        steps.append(dict(torques=tq, dof_state=torch.stack([q, qd], 2), actions=act, reset=reset, time_out=tout,
                          blew_up=blew))
    return steps


def _tensors(env):
    """The env tensors the record reads, by lgx_buffers name."""
    return dict(torques=env.torques, dof_state=env._dof_state3, actions=env.actions, reset=env.reset_buf,
                time_out=env.time_out_buf, blew_up=env.blew_up_buf)


def write_inputs(env, s):
    """One scripted step into the tensors the native env is bound to."""
    dst = _tensors(env)
    assert dst["torques"].shape[1:] == (D,) and dst["dof_state"].shape[1:] == (D, 2) and dst["actions"].shape[1:] == (D,)
    for k in SOURCES:
        dst[k].copy_(s[k])


def read_inputs(env):
    """The same tensors after a real step, as CPU copies."""
    return {k: t.detach().cpu().clone() for k, t in _tensors(env).items()}


def _tree(s):
    """The fixed pairwise tree of 16 slots."""
    while len(s) > 1:
        s = [s[i] + s[i + 1] for i in range(0, len(s), 2)]
    return s[0]


class Restatement:
    """lgx_joint_record restated from the rule text: plain Python lists of float64 per env and joint."""

    def __init__(self, n, lim):
        self.n, self.dt = n, lim.dt
        self.L, self.V, self.lo, self.hi = (v.double().tolist() for v in (lim.L, lim.V, lim.lo, lim.hi))
        self.C, self.num_actions = float(lim.C), lim.num_actions
        self.joint = [[[0.0] * 16 for _ in range(D)] for _ in range(n)]
        self.body = [[0.0] * 4 for _ in range(n)]
        self.status = [0] * n
        self.terms = [[{k: 0 for k in SUMS} for _ in range(D)] for _ in range(n)]  # non-zero terms of each sum

    def record(self, s):
        n = self.n
        tq = s["torques"].detach().cpu().double().reshape(n, D).tolist()
        ds = s["dof_state"].detach().cpu().double().reshape(n, D, 2).tolist()
        ac = s["actions"].detach().cpu().double().reshape(n, -1).tolist()
        reset, tout, blew = (s[k].detach().cpu().bool().tolist() for k in ("reset", "time_out", "blew_up"))
        dt, C = self.dt, self.C
        for e in range(n):
            if self.status[e] != 0:
                continue
            if reset[e]:
                self.status[e] = 3 if blew[e] else (1 if tout[e] else 2)
                continue
            body = self.body[e]
            first = body[0] == 0
            slots, any_sat, any_out = [0.0] * 16, False, False
            for j in range(D):
                tau, (q, qd), r, T = tq[e][j], ds[e][j], self.joint[e][j], self.terms[e][j]
                a = ac[e][j] if j < self.num_actions else 0.0
                p = tau * qd
                sat, out = abs(tau) >= self.L[j], q < self.lo[j] or q > self.hi[j]
                adds = {2: tau * tau, 4: max(p, 0.0) * dt, 5: max(-p, 0.0) * dt, 12: 0.0 if first else (a - r[0]) ** 2,
                        15: abs(qd)}
                for k, v in adds.items():
                    r[k] += v
                    T[k] += v != 0
                r[0] = a
                r[1] += sat
                r[3] = max(r[3], abs(tau))
                r[6] = max(r[6], abs(p))
                r[7] = max(r[7], abs(qd))
                r[8] += abs(qd) > self.V[j]
                r[9] += out
                r[10] = q if first else min(r[10], q)
                r[11] = q if first else max(r[11], q)
                r[13] += abs(a) >= C
                r[14] += p < 0
                slots[j] = abs(p)
                any_sat, any_out = any_sat or sat, any_out or out
            body[0] += 1
            body[1] = max(body[1], _tree(slots))
            body[2] += any_sat
            body[3] += any_out


def check_records(env, ref, what, scale=1.0):
    """The device's records against the restatement's at the bounds of the module docstring (scale:
    2 for a comparison of two fp32 implementations)."""
    rec, body = env.joint_rec.detach().cpu().double(), env.joint_body.detach().cpu().double()
    assert env.joint_status.cpu().tolist() == ref.status, f"{what}: status"
    want, wbody = torch.tensor(ref.joint, dtype=torch.float64), torch.tensor(ref.body, dtype=torch.float64)
    assert rec.shape == want.shape == (ref.n, D, 16) and body.shape == wbody.shape == (ref.n, 4)
    assert torch.equal(body[:, BODY_EXACT], wbody[:, BODY_EXACT]), f"{what}: exact body columns"
    assert torch.equal(rec[..., EXACT], want[..., EXACT]), f"{what}: exact joint columns"
    terms = torch.tensor([[[t[k] for k in SUMS] for t in je] for je in ref.terms], dtype=torch.float64)
    err = (rec[..., SUMS] - want[..., SUMS]).abs()
    assert bool((err <= scale * (terms + 2) * U * want[..., SUMS]).all()), f"{what}: sum columns {float(err.max()):.3e}"
    assert bool(((rec[..., 6] - want[..., 6]).abs() <= scale * 2 * U * want[..., 6]).all()), f"{what}: column 6"
    assert bool(((body[:, 1] - wbody[:, 1]).abs() <= scale * 6 * U * wbody[:, 1]).all()), f"{what}: body 1"


def _cell_row(envs):
    """The cell row [246] of a list of (body [4], joint [12][16]) records, and sum |term| likewise:
    lgx_joint_reduce restated with math.fsum, max and min."""
    if not envs:
        return [0.0] * NCOL, [0.0] * NCOL
    cols = [[1.0] * len(envs)] + [[b[k] for b, _ in envs] for k in range(4)]
    row = [math.fsum(c) for c in cols] + [max(b[1] for b, _ in envs)]
    mag = [math.fsum(abs(v) for v in c) for c in cols] + [0.0]
    for j in range(D):
        for k in range(1, 16):
            c = [r[j][k] for _, r in envs]
            row.append(math.fsum(c))
            mag.append(math.fsum(abs(v) for v in c))
        row += [max(r[j][3] for _, r in envs), max(r[j][6] for _, r in envs), max(r[j][7] for _, r in envs),
                min(r[j][10] for _, r in envs), max(r[j][11] for _, r in envs)]
        mag += [0.0] * 5  # (exact columns)
    return row, mag


def cells_of(env, ncells, cell_of):
    """The cells of the device's own records in float64: (cells [ncells, 246], sum |term| likewise)."""
    rec, body = env.joint_rec.cpu().double().tolist(), env.joint_body.cpu().double().tolist()
    status = env.joint_status.cpu().tolist()
    members = [[] for _ in range(ncells)]
    for e in range(env.num_envs):
        if status[e] != 0 and body[e][0] > 0:
            members[cell_of(e)].append((body[e], rec[e]))
    rows = [_cell_row(m) for m in members]
    return (torch.tensor([r for r, _ in rows], dtype=torch.float64), torch.tensor([m for _, m in rows], dtype=torch.float64))


def exact_cell_columns():
    """The env count and the maximum / minimum columns of a cell row."""
    return [0, 5] + [6 + 20 * j + k for j in range(D) for k in range(15, 20)]


def check_cells(got, env, cell_of, what):
    got = got.reshape(-1, NCOL)
    want, mag = cells_of(env, got.shape[0], cell_of)
    assert bool(((got - want).abs() <= 1e-12 * mag).all()), f"{what}: cells"
    ex = exact_cell_columns()
    assert torch.equal(got[:, ex], want[:, ex]), f"{what}: count and max / min columns"
    return want


def scripted_env(n, device, grid=True, seed=500):
    env, _, _ = E.make_env("go2", n, device)
    assert env.num_dof == D and env.num_actions == D
    if grid:
        E.bind_grid(env, torch.Generator().manual_seed(seed + n))
    return env


def run_script(env, steps, every_call=None):
    ref = Restatement(env.num_envs, limits(env))
    env.joint_begin()
    for t, s in enumerate(steps):
        write_inputs(env, s)
        env.joint_record()
        ref.record(s)
        if every_call is not None:
            every_call(t, ref)
    return ref


def scripted(n, device, every_call=False):
    """The script on a fresh env of the device with the terrain-grid cells: (env, restatement, steps)."""
    env = scripted_env(n, device)
    env.joint_buffers()
    steps = script(n, torch.Generator().manual_seed(900 + n), limits(env))
    check = (lambda t, ref: check_records(env, ref, f"{device} n={n} call {t}")) if every_call else None
    return env, run_script(env, steps, check), steps


# ------------------------------------------------------------------ test bodies
def records_and_cells(n, device):
    """Case 1."""
    env, ref, steps = scripted(n, device, every_call=True)
    lim, ee = limits(env), edge_env(n)
    joint, body, status = ref.joint, ref.body, ref.status
    # the script has the edges ...
    tq = [float(s["torques"][ee, 0]) for s in steps[:3]]
    assert tq[0] == float(lim.L[0]) and -tq[1] < float(lim.L[0]) and -tq[1] == float(_next(lim.L[0], 0.0)) and tq[2] == -tq[0]
    qd = [float(s["dof_state"][ee, 1, 1]) for s in steps[:3]]
    assert qd[0] == float(lim.V[1]) and qd[1] > qd[0] and qd[1] == float(_next(lim.V[1], INF)) and qd[2] == -qd[1]
    q = [float(s["dof_state"][ee, 2, 0]) for s in steps[:4]]
    assert q[0] == float(lim.lo[2]) and q[1] == float(lim.hi[2]) and q[2] < q[0] and q[3] > q[1]
    act = [float(s["actions"][ee, 3]) for s in steps[:3]]
    assert act[0] == float(lim.C) and act[1] == -act[0] and 0 < act[2] < act[0]
    # ... and the record counts them as the rule says
    r = joint[ee]
    assert body[ee][0] == CALLS - 1 and status[ee] == 1
    assert r[0][1] == 2 and r[0][3] == float(lim.L[0])                      # |tau| == L counts, just below does not
    assert r[1][8] == 2 and r[1][7] == float(_next(lim.V[1], INF))          # |qd| == V is not over
    assert r[2][9] == 2 and (r[2][10], r[2][11]) == (q[2], q[3])            # lo and hi are inside
    assert r[3][13] == 2 and r[3][0] == float(steps[CALLS - 2]["actions"][ee, 3])  # |a| == C is clipped
    assert r[4][14] == 1 and r[4][4] > 0 and r[4][5] > 0 and r[4][6] == 6.0 and ref.terms[ee][4][4] == 1
    assert body[ee][2] == 2 and body[ee][3] == 2                            # calls 0, 2 and calls 2, 3
    assert all(r[j][12] > 0 for j in range(D)) and ref.terms[ee][0][12] == CALLS - 2  # the first sample has no rate
    if n >= 63:
        assert status[:6] == [2, 1, 2, 2, 3, 0] and set(status) == {0, 1, 2, 3}
        assert [body[e][0] for e in range(5)] == [0, CALLS - 1, 5, 2, 4] and body[5][0] == CALLS
        assert joint[0] == [[0.0] * 16] * D  # reset at call 0: no sample
        every = [sum(joint[e][j][k] for e in range(n) for j in range(D)) for k in (1, 8, 9, 13, 14)]
        assert all(v > 0 for v in every), every  # the random envs meet every counter
    rows, cols = E.ROWS, E.COLS
    lv, ty = env.terrain_levels.cpu().tolist(), env.terrain_types.cpu().tolist()
    cells = env.joint_cells()
    assert cells.shape == (rows, cols, NCOL) and cells.dtype == torch.float64
    want = check_cells(cells, env, lambda e: lv[e] * cols + ty[e], f"{device} n={n} grid")
    counted = sum(1 for e in range(n) if status[e] != 0 and body[e][0] > 0)
    assert int(want[:, 0].sum()) == counted and (n < 63 or counted < n - 1)  # envs 0 and 5 are in no cell
    assert n >= 63 or bool((want[:, 0] == 0).any())  # a single env leaves empty cells: all zero
    assert bool((cells.reshape(-1, NCOL)[want[:, 0] == 0] == 0).all())
    # a free cell key
    ids = torch.randint(0, 6, (n,), generator=torch.Generator().manual_seed(3), dtype=torch.int32).to(env.device)
    grid_set = env._joint
    env.joint_buffers(2, 3, ids)
    assert env._joint is not grid_set
    run_script(env, steps)
    idl = ids.cpu().tolist()
    cells = env.joint_cells()
    assert cells.shape == (2, 3, NCOL)
    check_cells(cells, env, lambda e: idl[e], f"{device} n={n} cell_ids")
    # one id outside the grid: counted, cells untouched
    ids[7 % n] = 6
    env._joint_cells.fill_(7.0)
    with pytest.raises(_native.LgxError, match="outside"):
        env.joint_cells()
    assert int(env._joint_overflow.item()) == 1 and bool((env._joint_cells == 7.0).all())
    ids[7 % n] = 0
    env.joint_cells()
    assert int(env._joint_overflow.item()) == 0
    # the first set kept its tensors
    assert env.joint_buffers() is grid_set and env._joint_cells.shape == (rows, cols, NCOL)


def frozen_means_frozen(n, device):
    """Case 2: once every env has finished, nothing is written again."""
    env = scripted_env(n, device)
    env.joint_buffers()
    gen, lim = torch.Generator().manual_seed(1000 + n), limits(env)
    last = script(n, gen, lim, calls=1, scripted=False)[0]
    last["reset"] = torch.ones(n, dtype=torch.bool)  # everyone still recording ends here
    run_script(env, script(n, gen, lim) + [last])
    assert int((env.joint_status == 0).sum()) == 0
    cells = env.joint_cells()
    tensors = lambda: (env.joint_rec, env.joint_body, env.joint_status, env._joint_cells)  # noqa: E731
    before = [t.clone() for t in tensors()]
    for s in script(n, gen, lim, calls=3, scripted=False):
        write_inputs(env, s)
        env.joint_record()
    for a, b in zip(before, tensors()):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))  # no byte changed
    assert torch.equal(env.joint_cells(), cells)


def reduce_is_deterministic(n, device):
    """Case 3."""
    env, ref, _ = scripted(n, device)
    a = env.joint_cells()
    env._joint_cells.fill_(-1.0)
    b = env.joint_cells()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    out = [e for e in range(n) if ref.status[e] == 0 or ref.body[e][0] == 0]
    assert n < 63 or {0, 5} <= set(out)
    # the cells do not change when the records of the excluded envs do
    for e in out:
        env.joint_rec[e] = 1e6
        env.joint_body[e, 1:] = 1e6
    assert torch.equal(env.joint_cells(), a)
    # ... and do when they become countable
    if out:
        env.joint_status[out[0]] = 1
        env.joint_body[out[0], 0] = 1.0
        assert not torch.equal(env.joint_cells(), a)


def kernels_match_host(n):
    """Case 4 (GPU file): the kernels against the host backend on the same script."""
    env, ref, _ = scripted(n, "cuda:0")
    host, _, _ = scripted(n, "cpu")
    assert torch.equal(env.joint_status.cpu(), host.joint_status)
    rec, hrec = env.joint_rec.cpu(), host.joint_rec
    body, hbody = env.joint_body.cpu(), host.joint_body
    assert torch.equal(rec[..., EXACT], hrec[..., EXACT]) and torch.equal(body[:, BODY_EXACT], hbody[:, BODY_EXACT])
    check_records(env, ref, f"hip n={n}")
    check_records(host, ref, f"host n={n}")  # both within the bound: within twice the bound of each other
    terms = torch.tensor([[[t[k] for k in SUMS] for t in je] for je in ref.terms], dtype=torch.float64)
    d = (rec.double() - hrec.double()).abs()
    assert bool((d[..., SUMS] <= 2 * (terms + 2) * U * hrec[..., SUMS].double()).all())
    assert bool((d[..., 6] <= 4 * U * hrec[..., 6].double()).all())
    assert bool(((body[:, 1].double() - hbody[:, 1].double()).abs() <= 12 * U * hbody[:, 1].double()).all())
    a, b = env.joint_cells().reshape(-1, NCOL), host.joint_cells().reshape(-1, NCOL)
    # the env counts and the maxima / minima: both backends round each product and each level of the
    # P tree the same way, so the peaks of column 6 and body 1 are equal too
    ex = exact_cell_columns()
    assert torch.equal(a[:, ex], b[:, ex])
    # each backend's sums against its own records (the grids are equal: the same seed)
    lv, ty = env.terrain_levels.cpu().tolist(), env.terrain_types.cpu().tolist()
    check_cells(a, env, lambda e: lv[e] * E.COLS + ty[e], f"hip n={n} cells")
    check_cells(b, host, lambda e: lv[e] * E.COLS + ty[e], f"host n={n} cells")


def evaluator(task, n, device, **over):
    from legged_gym_custom_amd.utils.evaluator import PolicyEvaluator
    over.setdefault("env.episode_length_s", 0.59)  # ceil(0.59 / 0.02) = 30 steps
    if task == "go2_parkour":
        over.update({"terrain.curriculum": False, "commands.curriculum": False})
    env, tcfg, args = E.make_env(task, n, device, **over)
    assert int(env.max_episode_length) == 30
    return PolicyEvaluator(env, E.make_runner(env, tcfg, args))


def _strip(t):
    return {k: v for k, v in t.items() if k != "joints"}


def end_to_end(task, n, device):
    """Case 5: real physics. The eager loop with the source tensors copied after each step into the
    restatement, the same as a run, a run without the record; on the GPU a second evaluator replays
    its graph."""
    plain = evaluator(task, n, device)
    rp = plain.run(graph=False)
    base_cells = plain.last_cells.clone()
    assert plain.last_joint_cells is None and "joints" not in rp["total"]
    a = evaluator(task, n, device)
    env = a.env
    steps = int(env.max_episode_length) + 1
    ref = Restatement(n, limits(env))
    a._set_trace(None, False, True)
    env.joint_buffers()
    a.begin()
    for _ in range(steps):
        a.step()
        ref.record(read_inputs(env))
    check_records(env, ref, f"{device} {task} n={n} end to end")
    rec, body, status = (t.clone() for t in (env.joint_rec, env.joint_body, env.joint_status))
    ra = a.run(graph=False, joints=True)
    assert ra["graph"] is False and ra["num_steps"] == steps and ra["total"]["running"] == 0
    cells, jcells = a.last_cells.clone(), a.last_joint_cells.clone()
    for x, y in zip((env.joint_rec, env.joint_body, env.joint_status), (rec, body, status)):
        assert torch.equal(x, y)  # bit for bit
    assert torch.equal(status, env.eval_status) and int((status == 0).sum()) == 0
    assert torch.equal(body[:, 0], env.eval_acc[:, 0])
    got = a.joint_records()
    assert got["joint"].shape == (n, D, 16) and got["body"].shape == (n, 4) and got["status"].shape == (n,)
    # the existing, independent record: the same non-negative terms in another order
    r, acc = rec.cpu().double(), env.eval_acc.cpu().double()
    T = body[:, 0].cpu().double()
    bound = (12 * T + 8) * U
    work, heat = (r[..., 4] + r[..., 5]).sum(1), r[..., 2].sum(1)
    print(f"{task} n={n}: work vs eval_acc[5] max rel {float(((work - acc[:, 5]).abs() / acc[:, 5].clamp_min(1e-300)).max()):.3e}, "
          f"heat vs eval_acc[6] max rel {float(((heat - acc[:, 6]).abs() / acc[:, 6].clamp_min(1e-300)).max()):.3e}, "
          f"bound {float(bound.min()):.3e}..{float(bound.max()):.3e}")
    assert bool(((work - acc[:, 5]).abs() <= bound * acc[:, 5]).all())
    assert bool(((heat - acc[:, 6]).abs() <= bound * acc[:, 6]).all())
    print(f"{task} n={n}: {int(r[..., 1].sum())} saturated, {int(r[..., 8].sum())} over-speed, "
          f"{int(r[..., 9].sum())} out-of-range joint samples of {int(T.sum()) * D}; statuses "
          f"{torch.bincount(status.cpu().long(), minlength=4).tolist()}")
    j = ra["total"]["joints"]
    assert j["envs"] == int((T > 0).sum()) and j["samples"] == int(T.sum()) and set(j["joints"]) == set(env.dof_names)
    assert len(ra["cells"]) == jcells.shape[0] and all("joints" in c for row in ra["cells"] for c in row)
    # the record perturbs nothing
    assert torch.equal(cells, base_cells)
    assert _strip(ra["total"]) == rp["total"]
    assert [[_strip(c) for c in row] for row in ra["cells"]] == rp["cells"]
    rq = a.run(graph=False)
    assert torch.equal(a.last_cells, cells) and a.last_joint_cells is None and rq["total"] == rp["total"]
    if device == "cpu":
        return
    b2 = evaluator(task, n, device)
    rb = b2.run(joints=True)
    assert rb["graph"] is True
    assert torch.equal(b2.last_cells, cells)
    assert torch.equal(b2.last_joint_cells.view(torch.int64), jcells.view(torch.int64))
    for x, y in zip((b2.env.joint_rec, b2.env.joint_body, b2.env.joint_status), (rec, body, status)):
        assert torch.equal(x, y)  # graph replay = the eager loop, bit for bit
    with_joints = b2._graph
    b2.run()
    assert b2._graph is not with_joints and torch.equal(b2.last_cells, cells)  # keyed by the flag: recaptured


def composition(device):
    """Case 6."""
    import json
    ev = evaluator("go2", 64, device, **{"domain_rand.scheduled_pushes": True, "commands.scheduled_commands": True})
    plain = ev.run()
    assert "joints" not in plain["total"]
    rc = ev.run_command_test([0.0, 1.0], vy=(0.0,), yaw=(0.0, 0.5), at_s=0.1, steady_after_s=0.1, joints=True)
    assert rc["total"]["joints"]["envs"] == 64
    got = [rc["bins"][ix][0][iw]["joints"] for ix in range(2) for iw in range(2)]
    assert [g["envs"] for g in got] == [16] * 4 and all(g["samples"] > 0 for g in got)
    rp = ev.run_push_test([0.0, 1.0], directions=2, at_s=0.1, joints=True)
    got = [rp["bins"][s][d]["joints"] for s in range(2) for d in range(2)]
    assert [g["envs"] for g in got] == [16] * 4 and rp["total"]["joints"]["envs"] == 64
    rt = ev.run(joints=True, gait=True, trace_depth=4)
    assert rt["total"]["joints"]["envs"] == 64 and rt["total"]["gait"]["envs"] == 64
    assert ev.traces([0])["trace"].shape == (1, 4, 76)
    assert all("joints" in c and "gait" in c for row in rt["cells"] for c in row)
    assert sum(c["joints"]["envs"] for row in rt["cells"] for c in row) == 64
    json.dumps([rc, rp, rt], allow_nan=False)
    again = ev.run()
    assert "joints" not in again["total"] and all("joints" not in c for row in again["cells"] for c in row)
    assert again["total"] == plain["total"] and again["cells"] == plain["cells"]
    with pytest.raises(RuntimeError, match="joint"):
        ev.joint_records()


def _hand_row(envs=2, samples=200):
    """A joint cell row [246] made by hand for joints with L = 20, V = 10, range [-1, 1]: joint 0 busy,
    joint 1 idle but once over speed, the rest untouched at angle 0."""
    row = [0.0] * NCOL
    row[0:6] = [envs, samples, 300.0, 50.0, 4.0, 180.0]
    b = 6
    row[b:b + 20] = [20.0, 200.0 * 16.0, 40.0, 30.0, 10.0, 200.0, 16.0, 0.0, 4.0, -1.5, 1.7, 198.0 * 0.25, 10.0, 50.0,
                     400.0, 21.0, 120.0, 9.0, -1.25, 0.9]
    b = 26
    row[b:b + 20] = [0.0, 200.0 * 1.0, 2.0, 10.0, 0.0, 20.0, 22.0, 1.0, 0.0, -0.2, 0.2, 0.0, 0.0, 0.0, 100.0,
                     1.0, 10.0, 12.0, -0.125, 0.125]
    return row


def report():
    """Case 7: joint_cell_report on hand-made rows, without a device."""
    import json
    from legged_gym_custom_amd.utils import evaluator as M
    names = [f"j{i}" for i in range(D)]
    params = types.SimpleNamespace(torque_limits=[20.0] * D, dof_vel_limits=[10.0] * D, dof_pos_limits=[[-1.0, 1.0]] * D,
                                   clip_actions=3.0)
    assert (M.JOINT_FLAG_SATURATION, M.JOINT_FLAG_RANGE, M.JOINT_FLAG_CLIP) == (0.05, 0.01, 0.01)
    r = M.joint_cell_report(_hand_row(), 0.02, names, params)
    json.dumps(r, allow_nan=False)
    assert r["envs"] == 2 and r["samples"] == 200 and set(r["joints"]) == set(names)
    assert r["mean_peak_power_w"] == 150.0 and r["max_peak_power_w"] == 180.0
    assert r["any_saturation_share"] == 0.25 and r["any_out_of_range_share"] == 0.02
    a = r["joints"]["j0"]
    assert a["torque_saturation_share"] == 0.1 and a["rms_torque"] == 4.0 and a["rms_torque_over_limit"] == 0.2
    assert a["mean_peak_torque"] == 20.0 and a["max_peak_torque"] == 21.0 and a["max_peak_torque_over_limit"] == 1.05
    assert a["mean_positive_power_w"] == 7.5 and a["mean_negative_power_w"] == 2.5 and a["work_share"] == 0.75
    assert a["max_peak_power_w"] == 120.0 and a["max_peak_speed"] == 9.0 and a["max_peak_speed_over_limit"] == 0.9
    assert a["over_speed_share"] == 0.0 and a["out_of_range_share"] == 0.02
    assert a["range_used"] == [-1.25, 0.9] and a["range_margin_rad"] == -0.25
    assert a["action_rate_rms"] == 0.5 and a["action_clip_share"] == 0.05 and a["braking_share"] == 0.25
    assert a["mean_speed"] == 2.0
    b = r["joints"]["j1"]
    assert b["torque_saturation_share"] == 0.0 and b["rms_torque"] == 1.0 and b["work_share"] == 0.25
    assert b["over_speed_share"] == 0.005 and b["max_peak_speed_over_limit"] == 1.2 and b["range_margin_rad"] == 0.875
    assert b["action_rate_rms"] == 0.0
    idle = r["joints"]["j5"]
    assert idle["rms_torque"] == 0.0 and idle["range_used"] == [0.0, 0.0] and idle["range_margin_rad"] == 1.0
    flags = r["flags"]
    assert len(flags) == 4 and [f.split(":")[0] for f in flags] == ["j0", "j0", "j0", "j1"]
    assert "torque" in flags[0] and "position" in flags[1] and "clip" in flags[2] and "speed" in flags[3]
    # below the thresholds: no flag
    quiet = _hand_row()
    quiet[6], quiet[6 + 8], quiet[6 + 12], quiet[26 + 7] = 10.0, 2.0, 2.0, 0.0
    assert M.joint_cell_report(quiet, 0.02, names, params)["flags"] == []
    # an empty row: None everywhere, JSON without NaN
    empty = M.joint_cell_report([0.0] * NCOL, 0.02, names, params)
    assert "NaN" not in json.dumps(empty, allow_nan=False)
    assert empty["envs"] == 0 and empty["samples"] == 0
    assert all(v is None for k, v in empty.items() if k not in ("envs", "samples", "joints"))
    assert all(v is None for j in empty["joints"].values() for v in j.values())
    # the total: sums added, max of maxima and min of minima over the non-empty cells only
    one, two = _hand_row(), _hand_row(envs=3, samples=100)
    two[5], two[6 + 15], two[6 + 18], two[6 + 19], two[26 + 18] = 100.0, 30.0, -0.5, 1.5, 0.5
    total = M.joint_total_row(torch.tensor([one, [0.0] * NCOL, two], dtype=torch.float64))
    assert total.shape == (NCOL,) and total[0] == 5 and total[1] == 300 and total[6] == 40.0
    assert total[5] == 180.0 and total[6 + 15] == 30.0 and total[6 + 18] == -1.25 and total[6 + 19] == 1.5
    # (the empty cell's zeros are not angles: joint 1's lowest angle is the smaller of -0.125 and 0.5,
    # joint 5's range is 0..0 because the two cells with envs say so)
    assert total[26 + 18] == -0.125 and total[26 + 19] == 0.125
    only = M.joint_total_row(torch.tensor([[0.0] * NCOL, two], dtype=torch.float64))
    assert only[26 + 18] == 0.5 and only[6 + 18] == -0.5  # min over the non-empty cell, not min(0, 0.5)
    assert bool((M.joint_total_row(torch.zeros(2, 3, NCOL, dtype=torch.float64)) == 0).all())


def refusals(device):
    """Case 8: each failure raises with a message naming its cause and writes nothing."""
    env, _, _ = scripted(63, device)
    tensors = lambda: (env.joint_rec, env.joint_body, env.joint_status, env._joint_cells)  # noqa: E731
    env.joint_cells()
    before = [t.clone() for t in tensors()]
    same = lambda: all(torch.equal(a, b) for a, b in zip(before, tensors()))  # noqa: E731
    env.reset_buf.zero_()  # a record that went ahead would add a sample to every recording env
    nat, st = env._native, env._stream()
    good = dict(joint=env.joint_rec, body=env.joint_body, status=env.joint_status, cells=env._joint_cells,
                overflow=env._joint_overflow)

    def raw(rows=E.ROWS, cols=E.COLS, **over):
        jb = _abi.JointBuffers()
        for k, t in {**good, **over}.items():
            setattr(jb, k, None if t is None else t.data_ptr())
        jb.cell_rows, jb.cell_cols = rows, cols
        return jb

    calls = {"begin": lambda jb: nat.joint_begin(jb, st), "record": lambda jb: nat.joint_record(jb, st),
             "reduce": lambda jb: nat.joint_reduce(jb, st)}
    for member in ("joint", "body", "status", "overflow"):
        for name, call in calls.items():
            with pytest.raises(_native.LgxError, match=f"lgx_joint_{name}: {member} is NULL"):
                call(raw(**{member: None}))
    with pytest.raises(_native.LgxError, match="lgx_joint_reduce: cells is NULL"):
        calls["reduce"](raw(cells=None))
    for rows, cols in ((0, 2), (3, 0), (-1, 2), (1 << 11, 1 << 10)):
        for name, call in calls.items():
            with pytest.raises(_native.LgxError, match=f"lgx_joint_{name}: cell_rows and cell_cols"):
                call(raw(rows, cols))
    # 4 bytes off a 16-byte boundary (never dereferenced: the call refuses first)
    off_joint = torch.zeros(63 * D * 16 + 1, device=env.device)[1:].view(63, D, 16)
    off_body = torch.zeros(63 * 4 + 1, device=env.device)[1:].view(63, 4)
    for name, call in calls.items():
        with pytest.raises(_native.LgxError, match=f"lgx_joint_{name}: joint must be 16-byte aligned"):
            call(raw(joint=off_joint))
        with pytest.raises(_native.LgxError, match=f"lgx_joint_{name}: body must be 16-byte aligned"):
            call(raw(body=off_body))
    L = _native.lib()
    for fn in (L.lgx_joint_begin, L.lgx_joint_record, L.lgx_joint_reduce):
        assert fn(nat.handle, None, None) < 0 and b"joint buffers are NULL" in L.lgx_last_error(nat.handle)
    for member in ("joint", "body", "status", "cells", "overflow"):
        with pytest.raises(_native.LgxError, match=f"joint buffer {member} is required"):
            nat.joint_buffers(**{**good, member: None})
    with pytest.raises(_native.LgxError, match="joint buffer joint must be"):
        nat.joint_buffers(**{**good, "joint": env.joint_rec[:, :3].contiguous()})
    with pytest.raises(_native.LgxError, match="joint buffer body must be"):
        nat.joint_buffers(**{**good, "body": env.joint_body.double()})
    with pytest.raises(_native.LgxError, match="joint buffer cells must be"):
        nat.joint_buffers(**{**good, "cells": env._joint_cells[..., :61].contiguous()})
    with pytest.raises(_native.LgxError, match="joint buffer cell_ids must be"):
        nat.joint_buffers(**good, cell_ids=torch.zeros(63, dtype=torch.int64, device=env.device))
    assert same()
    # unbound source buffers
    for attr, name in (("torques", "torques"), ("_dof_state3", "dof_state"), ("actions", "actions"),
                       ("reset_buf", "reset"), ("time_out_buf", "time_out")):
        keep = getattr(env, attr)
        setattr(env, attr, None)
        try:
            env._bind()
        except _native.LgxError as err:  # lgx_bind itself requires this one
            assert name in str(err)
        else:
            for call, cname in ((env.joint_begin, "begin"), (env.joint_record, "record"), (env.joint_cells, "reduce")):
                with pytest.raises(_native.LgxError, match=f"lgx_joint_{cname}.*not bound: {name}"):
                    call()
        setattr(env, attr, keep)
        env._bind()
    assert same()
    # more joints than a record holds (a second native env whose params say 13 joints)
    import ctypes
    params = type(nat.params)()
    ctypes.memmove(ctypes.byref(params), ctypes.byref(nat.params), ctypes.sizeof(params))
    params.num_dof = _abi.MAX_DOF + 1
    try:
        bad = _native.NativeEnv(nat.model, params, nat.device_index)
    except _native.LgxError as err:  # lgx_create itself takes 12 joints only
        assert "12 dof" in str(err)
    else:
        bad.bind(nat._keep)
        jb = bad.joint_buffers(**good)
        for call in (bad.joint_begin, bad.joint_record, bad.joint_reduce):
            with pytest.raises(_native.LgxError, match="more joints than a record holds"):
                call(jb, st)
    assert same()
    # no record yet
    other, _, _ = E.make_env("go2", 8, device)
    for call in (other.joint_begin, other.joint_record, other.joint_cells):
        with pytest.raises(RuntimeError, match="joint_buffers"):
            call()
    env.joint_record()  # and the first env's record is still usable
    assert not same()
