"""Shared by tests/test_contact_host.py and tests/test_gpu_contact.py: the contact record (include/lgx.h
ABI 14: lgx_contact_begin / lgx_contact_record / lgx_contact_reduce) on one device. A scripted sequence
of inputs written straight into the env's tensors (no physics step, the style of joint_case.py), a
restatement of the rule text of include/lgx.h in numpy (one array operation per operation of the
rule text), and the test bodies, parameterised by the device.

Bounds (from the number formats, not from the code under test; u = 2^-24). The rule text is fp32
without contraction, every operation of it correctly rounded (+, -, *, / and sqrtf are, in IEEE
arithmetic), so the restatement evaluates each per-sample quantity (fn, fh, 5*|F.z|, z - h, the cell
index, the relief) in numpy float32, operation by operation in the order of the text, and these are
the device's bits:
* body columns 0, 1, 2, 5, 8, 11 and env columns 0, 1, 2, 7 are counts below 2^24 of comparisons of
  such quantities; body 4, 7, 10 and env 3, 5 are maxima / minima / copies of them; env 4 and 6 are
  body indices chosen by comparisons of them: all exact. (fn = sqrtf(x^2 + y^2 + z^2) is three
  roundings of non-negative terms and a square root; for an axis-aligned force sqrtf(z^2) = |z|
  exactly, which the planted thresholds use.)
* body columns 3, 6 and 9 are fp32 running sums of T non-zero terms, the restatement's in float64.
  Column 3's term fn*dt is one fp32 rounding of the exact product (c = 1); column 6's term z - h and
  column 9's term relief are per-sample quantities as above (c = 0). With c = 1 for all three:
  |error| <= g * sum |term|, g = (T + 1) u / (1 - (T + 1) u), the standard bound of a recursive sum
  (column 6's terms are signed, hence sum |term| and not the sum).
* cells: the sums are fp64 sums of at most 130 fp32 records by a fixed tree: against the float64 sum
  of the device's own records, |error| <= 1e-12 sum |term|. Counts, maxima and minima: exactly equal."""
import math

import numpy as np
import pytest
import torch

import eval_case as E
from legged_gym_custom_amd import _abi, _native
from legged_gym_custom_amd.utils.evaluator import EDGE_RELIEF_M

CALLS, MB = 13, _abi.MAX_BODIES
U = 2.0 ** -24
EXACT = [0, 1, 2, 4, 5, 7, 8, 10, 11]
SUMS = [3, 6, 9]
NCOL = _abi.CONTACT_CELL_COLS
SOURCES = ("contact_forces", "rigid_body_states", "reset", "time_out", "blew_up")
INF = float("inf")
f32 = np.float32
BEGIN_ENV = [0.0, 0.0, 0.0, 0.0, -1.0, 0.0, -1.0, 0.0]
# the planted terrain of the scripted heightfield instance (cells of height_samples)
KX, YLO, YHI, YMID = 512, 1000, 1040, 1020  # the cell boundary px / horizontal_scale == 512 exactly; the y band
STEP_AT, STEP_OVER = 612, 712               # steps of 10 units (relief == edge_tol) and of 11 units (its neighbour)


def par(env):
    """What the rule text reads from lgx_task_params, and the height samples (a CPU numpy view's copy is
    taken at every use: the scripted tests rewrite the field)."""
    p = env._native.params
    plane = p.mesh_type == _abi.MESH_PLANE or env.height_samples is None
    return dict(nb=int(p.num_bodies), dt=f32(p.dt), plane=plane, feet=[int(p.feet_idx[i]) for i in range(p.num_feet)],
                term=[int(p.termination_idx[i]) for i in range(p.n_termination)],
                pen=[int(p.penalised_idx[i]) for i in range(p.n_penalised)], border=f32(p.border_size),
                hscale=f32(p.horizontal_scale), vscale=f32(p.vertical_scale), rows=int(p.hf_rows), cols=int(p.hf_cols))


def _nx(x, towards):
    return float(np.nextafter(f32(x), f32(towards)))


def edge_env(n):
    """The env that carries the planted edges: it records every call but the last, where it times out."""
    return 1 if n >= 63 else 0


def plant_terrain(env):
    """The scripted heightfield: random 4 x 4 blocks of random heights (flat inside a block: relief 0;
    edges between blocks), then, in the y band, a cell boundary at row KX (0 below, 40 from it on) and
    two steps of 10 and of 11 units. Written in place: the native env is bound to this tensor."""
    hs = env.height_samples
    R, C = hs.shape
    g = torch.Generator().manual_seed(77)
    blocks = torch.randint(-40, 41, ((R + 3) // 4, (C + 3) // 4), generator=g, dtype=torch.int16)
    field = blocks.repeat_interleave(4, 0).repeat_interleave(4, 1)[:R, :C].clone()
    field[KX - 12:KX, YLO:YHI], field[KX:KX + 12, YLO:YHI] = 0, 40
    field[STEP_AT - 12:STEP_AT, YLO:YHI], field[STEP_AT:STEP_AT + 12, YLO:YHI] = 0, 10
    field[STEP_OVER - 12:STEP_OVER, YLO:YHI], field[STEP_OVER:STEP_OVER + 12, YLO:YHI] = 0, 11
    hs.copy_(field.to(hs.device))


def x_of_cell(P, k, frac=0.5):
    """An x (or y) whose cell index is k: the middle of the cell (fp32)."""
    return float(f32(f32(k + frac) * P["hscale"]) - P["border"])


def script(n, gen, P, calls=CALLS, scripted=True):
    """`calls` steps of inputs (CPU tensors). Forces: a body is touched with probability 0.35, by a
    force of randn x 30 N or (one in three) of a magnitude around the 0.1 N and 1 N thresholds;
    positions: x, y uniform over the field and 3 m beyond its borders (on a plane: +-5 m), z in
    [-0.2, 0.6]. For n >= 63 (and scripted): env 0 falls at the first call with no force at all (no
    sample; terminal columns -1, 0, -1, 0 with status 2); env 1 (the edge env) times out at the last
    call; env 2 falls at call 5 with termination-list bodies 1 and 2 at an equal 7 N, body 0 at 3 N and
    a foot at 50 N; env 3 falls at call 2 with body 0 at exactly 1 N and nothing else (no termination
    contact) and resets again at call 6 with large forces; env 4 blows up at call 4 with time_out set
    and forces present; env 5 never resets; env 6 times out at call 7 with forces present; the rest
    reset once at a random call, half of them as time-outs. A single env times out at the last call.

    The edge env has no force and random positions inside the field except, by body and call:
      body 3  F.z   0.1+, 0.1+, 0.1, 0.1+ (0.1+ = nextafter(0.1f, inf))   onset at the first sample, held,
                                                                        released, re-made
      body 4  F.y   1, nextafter(1, inf), -1                            1 hard sample, 3 face hits
      body 5  F = (10, 0, 2), (nextafter(10, inf), 0, 2), (nextafter(10, 0), 0, 2)   fh = 5|F.z| and neighbours
      body 6  x on the cell boundary KX (call 0) and 2^-18 m below it (call 1), y in the band
      body 7  touches down at call 0 beside the 10-unit step; body 8 beside the 11-unit step
      bodies 9..12  touch down at call 0 beyond the -x, +x, -y, +y borders of the field"""
    nb, steps = P["nb"], []
    when = torch.randint(0, calls, (n,), generator=gen)
    as_timeout = torch.rand(n, generator=gen) < 0.5
    fixed = scripted and n >= 63
    ee = edge_env(n)
    if P["plane"]:
        xlo, xhi, ylo, yhi = -5.0, 5.0, -5.0, 5.0
    else:
        b = float(P["border"])
        xlo, xhi = -b - 3.0, P["rows"] * float(P["hscale"]) - b + 3.0
        ylo, yhi = -b - 3.0, P["cols"] * float(P["hscale"]) - b + 3.0
    foot0 = P["feet"][0]
    for t in range(calls):
        rnd = lambda *s: torch.rand(*s, generator=gen)  # noqa: E731
        touched = rnd(n, nb, 1) < 0.35
        big = 30.0 * torch.randn(n, nb, 3, generator=gen)
        small = (2.0 * rnd(n, nb, 3) - 1.0) * torch.tensor([0.08, 0.5, 0.9])[torch.randint(0, 3, (n, nb, 1), generator=gen)]
        cf = torch.where(touched, torch.where(rnd(n, nb, 1) < 1.0 / 3.0, small, big), torch.zeros(n, nb, 3))
        rb = torch.randn(n, nb, 13, generator=gen)
        rb[..., 0] = xlo + (xhi - xlo) * rnd(n, nb)
        rb[..., 1] = ylo + (yhi - ylo) * rnd(n, nb)
        rb[..., 2] = -0.2 + 0.8 * rnd(n, nb)
        reset = when == t
        tout = reset & as_timeout
        blew = torch.zeros(n, dtype=torch.bool)
        if scripted and n < 63:
            reset[:] = tout[:] = t == calls - 1
        if fixed:
            reset[:7] = torch.tensor([t == 0, t == calls - 1, t == 5, t in (2, 6), t == 4, False, t == 7])
            tout[:7] = torch.tensor([False, t == calls - 1, False, False, t == 4, False, t == 7])
            blew[4] = t == 4
            if t == 0:
                cf[0] = 0.0
            if t == 5:
                cf[2] = 0.0
                cf[2, 0], cf[2, 1], cf[2, 2], cf[2, foot0] = (torch.tensor(v) for v in
                                                            ((0.0, 0.0, 3.0), (0.0, 7.0, 0.0), (7.0, 0.0, 0.0), (0.0, 0.0, 50.0)))
            if t == 2:
                cf[3] = 0.0
                cf[3, 0] = torch.tensor((0.0, 0.0, 1.0))
            if t == 6:
                cf[3] = 40.0
            if t == 4:
                cf[4] = 25.0
            if t == 7:
                cf[6] = 25.0
        if scripted:
            cf[ee] = 0.0
            if not P["plane"]:
                rb[ee, :, 0] = x_of_cell(P, 100) + 50.0 * rnd(nb)
                rb[ee, :, 1] = x_of_cell(P, 100) + 50.0 * rnd(nb)
            a, one, ten = _nx(0.1, INF), 1.0, 10.0
            cf[ee, 3, 2] = [a, a, float(f32(0.1)), a][t] if t < 4 else 0.0
            cf[ee, 4, 1] = [one, _nx(one, INF), -one][t] if t < 3 else 0.0
            if t < 3:
                cf[ee, 5] = torch.tensor(([ten, _nx(ten, INF), _nx(ten, 0.0)][t], 0.0, 2.0))
            for b_, v in ((7, 5.0), (8, 5.0), (9, 5.0), (10, 5.0), (11, 5.0), (12, 5.0)):
                cf[ee, b_, 2] = v if t < 2 else 0.0
            if not P["plane"]:
                px = float(f32(KX) * P["hscale"])           # 512 * 0.1f: exact (a power of two)
                xb = float(f32(px) - P["border"])             # exact, and xb + border == px exactly
                ymid = x_of_cell(P, YMID)
                rb[ee, 6, 0], rb[ee, 6, 1] = (xb if t == 0 else xb - 2.0 ** -18), ymid
                rb[ee, 7, 0], rb[ee, 7, 1] = x_of_cell(P, STEP_AT - 1), ymid
                rb[ee, 8, 0], rb[ee, 8, 1] = x_of_cell(P, STEP_OVER - 1), ymid
                rb[ee, 9, 0], rb[ee, 10, 0] = xlo + 0.5, xhi - 0.5
                rb[ee, 11, 1], rb[ee, 12, 1] = ylo + 0.5, yhi - 0.5
        steps.append(dict(contact_forces=cf, rigid_body_states=rb, reset=reset, time_out=tout, blew_up=blew))
    return steps


def _tensors(env):
    """The env tensors the record reads, by lgx_buffers name."""
    return dict(contact_forces=env._contact3, rigid_body_states=env.rigid_body_states_view, reset=env.reset_buf,
                time_out=env.time_out_buf, blew_up=env.blew_up_buf)


def write_inputs(env, s):
    """One scripted step into the tensors the native env is bound to."""
    dst = _tensors(env)
    for k in SOURCES:
        assert dst[k].shape == s[k].shape, k
        dst[k].copy_(s[k])


def read_inputs(env):
    """The same tensors after a real step, as CPU copies."""
    return {k: t.detach().cpu().clone() for k, t in _tensors(env).items()}


class Restatement:
    """lgx_contact_record restated from the rule text of include/lgx.h. Per-sample quantities in numpy
    float32, one array operation per operation of the text; the running sums in float64."""

    def __init__(self, env, edge_tol):
        self.P, self.n = par(env), env.num_envs
        self.hs = None if self.P["plane"] else env.height_samples.detach().cpu().numpy().astype(np.int64)
        self.tol = f32(edge_tol)
        self.body = np.zeros((self.n, MB, 12))
        self.env = np.tile(np.array(BEGIN_ENV), (self.n, 1))
        self.status = np.zeros(self.n, dtype=np.int64)
        self.terms = np.zeros((self.n, MB, 3))  # non-zero terms of the sum columns 3, 6, 9
        self.mag = np.zeros((self.n, MB, 3))    # sum |term| of them

    def terrain(self, x, y):
        """(h, relief, ix, iy) under the fp32 positions x, y."""
        P = self.P
        if P["plane"]:
            z = np.zeros_like(x)
            return z, z, None, None
        hs, rows, cols = self.hs, P["rows"], P["cols"]
        ix = np.clip(np.trunc((x + P["border"]) / P["hscale"]).astype(np.int64), 0, rows - 2)
        iy = np.clip(np.trunc((y + P["border"]) / P["hscale"]).astype(np.int64), 0, cols - 2)
        h = np.minimum(np.minimum(hs[ix, iy], hs[ix + 1, iy]), hs[ix, iy + 1]).astype(f32) * P["vscale"]
        cx, cy = np.clip(ix, 1, rows - 2), np.clip(iy, 1, cols - 2)
        nine = np.stack([hs[cx + i, cy + j] for i in (-1, 0, 1) for j in (-1, 0, 1)])
        relief = (nine.max(0) - nine.min(0)).astype(f32) * P["vscale"]
        return h, relief, ix, iy

    def record(self, s):
        P, n, nb = self.P, self.n, self.P["nb"]
        F = s["contact_forces"].detach().cpu().numpy().astype(f32).reshape(n, nb, 3)
        X = s["rigid_body_states"].detach().cpu().numpy().astype(f32).reshape(n, nb, 13)
        reset, tout, blew = (s[k].detach().cpu().numpy().astype(bool) for k in ("reset", "time_out", "blew_up"))
        fx, fy, fz = F[..., 0], F[..., 1], F[..., 2]
        fn = np.sqrt(fx * fx + fy * fy + fz * fz)
        fh = np.sqrt(fx * fx + fy * fy)
        assert fn.dtype == f32 and fh.dtype == f32
        c, hard = fn > f32(0.1), fn > f32(1.0)
        face = c & (fh > f32(5.0) * np.abs(fz))
        h, relief, _, _ = self.terrain(X[..., 0], X[..., 1])
        dz = X[..., 2] - h
        assert dz.dtype == f32 and relief.dtype == f32
        is_foot = np.isin(np.arange(nb), P["feet"])
        is_term = np.isin(np.arange(nb), P["term"])
        pen_mult = np.array([P["pen"].count(b) for b in range(nb)])
        term_mult = np.array([P["term"].count(b) for b in range(nb)])
        open_ = self.status == 0
        # the envs that end here
        for e in np.nonzero(open_ & reset)[0]:
            self.status[e] = 3 if blew[e] else (1 if tout[e] else 2)
            if self.status[e] == 2:
                cand = np.where(is_term & hard[e], fn[e], f32(0))
                tb = int(np.argmax(cand)) if cand.max() > 0 else -1   # argmax: the first, i.e. lowest, index of the maximum
                cand6 = np.where(~is_foot & (fn[e] > 0), fn[e], f32(0))
                nb6 = int(np.argmax(cand6)) if cand6.max() > 0 else -1
                self.env[e, 4:8] = [tb, float(cand.max()), nb6, float((term_mult * hard[e]).sum())]
        # the envs that take a sample
        m = open_ & ~reset
        first = self.env[:, 0] == 0
        r = self.body[:, :nb]
        onset = c & (first[:, None] | (r[..., 0] == 0))
        new = r.copy()
        new[..., 0] = c
        new[..., 1] += c
        new[..., 2] += onset
        t3, t6, t9 = np.where(c, (fn * P["dt"]).astype(np.float64), 0.0), dz.astype(np.float64), np.where(onset, relief, f32(0)).astype(np.float64)
        new[..., 3] += t3
        new[..., 4] = np.maximum(r[..., 4], fn)
        new[..., 5] += face
        new[..., 6] += t6
        new[..., 7] = np.where(first[:, None], dz, np.minimum(r[..., 7], dz))
        new[..., 8] += onset & (relief > self.tol)
        new[..., 9] += t9
        new[..., 10] = np.where(onset, np.maximum(r[..., 10], relief), r[..., 10])
        new[..., 11] += hard
        self.body[:, :nb] = np.where(m[:, None, None], new, r)
        tt = np.stack([t3, t6, t9], -1)
        self.terms[:, :nb] += np.where(m[:, None, None], tt != 0, 0)
        self.mag[:, :nb] += np.where(m[:, None, None], np.abs(tt), 0.0)
        ev = self.env.copy()
        ev[:, 0] += 1
        ev[:, 1] += (pen_mult[None, :] * c).sum(1)
        ev[:, 2] += (c & ~is_foot[None, :]).any(1)
        ev[:, 3] = np.maximum(ev[:, 3], np.where(~is_foot[None, :], fn, f32(0)).max(1))
        self.env = np.where(m[:, None], ev, self.env)


def records_of(env):
    return (env.contact_body.detach().cpu().double(), env.contact_env.detach().cpu().double(),
            env.contact_status.cpu().long())


def check_records(env, ref, what):
    """The device's records against the restatement's at the bounds of the module docstring."""
    body, envr, status = records_of(env)
    assert status.tolist() == ref.status.tolist(), f"{what}: status"
    want, wenv = torch.from_numpy(ref.body), torch.from_numpy(ref.env)
    assert body.shape == want.shape == (ref.n, MB, 12) and envr.shape == wenv.shape == (ref.n, 8)
    assert torch.equal(envr, wenv), f"{what}: env columns {(envr != wenv).nonzero()[:4].tolist()}"
    assert torch.equal(body[..., EXACT], want[..., EXACT]), \
        f"{what}: exact body columns {(body[..., EXACT] != want[..., EXACT]).nonzero()[:4].tolist()}"
    k = torch.from_numpy(ref.terms) + 1.0
    g = k * U / (1.0 - k * U)
    err = (body[..., SUMS] - want[..., SUMS]).abs()
    assert bool((err <= g * torch.from_numpy(ref.mag)).all()), f"{what}: sum columns {float(err.max()):.3e}"
    assert bool((body[:, ref.P["nb"]:] == 0).all()), f"{what}: slots past num_bodies stay zero"


SUM_COLS = (1, 2, 3, 5, 6, 8, 9, 11)


def _cell_row(envs):
    """The cell row [320] of a list of (status, env [8], body [24][12]) records, and sum |term| likewise:
    lgx_contact_reduce restated with math.fsum, max and min."""
    row, mag = [0.0] * NCOL, [0.0] * NCOL
    if not envs:
        return row, mag
    fallen = [(v, b) for st, v, b in envs if st == 2]
    sampled = [(v, b) for _, v, b in envs if v[0] > 0]
    row[0] = mag[0] = float(len(envs))
    for k in range(3):
        row[1 + k] = math.fsum(v[k] for _, v, _ in envs)
        mag[1 + k] = math.fsum(abs(v[k]) for _, v, _ in envs)
    row[4] = max(v[3] for _, v, _ in envs)
    row[5] = mag[5] = float(len(fallen))
    row[6] = mag[6] = float(sum(1 for v, _ in fallen if v[4] < 0))
    row[7] = mag[7] = math.fsum(v[7] for v, _ in fallen)
    for b in range(MB):
        o = 8 + 13 * b
        for k, col in enumerate(SUM_COLS):
            row[o + k] = math.fsum(r[b][col] for _, _, r in envs)
            mag[o + k] = math.fsum(abs(r[b][col]) for _, _, r in envs)
        row[o + 8] = max(r[b][4] for _, _, r in envs)
        row[o + 9] = max(r[b][10] for _, _, r in envs)
        row[o + 10] = min(r[b][7] for _, r in sampled) if sampled else 0.0
        row[o + 11] = mag[o + 11] = float(sum(1 for v, _ in fallen if v[4] == b))
        row[o + 12] = mag[o + 12] = float(sum(1 for v, _ in fallen if v[6] == b))
    return row, mag


def cells_of(env, ncells, cell_of):
    """The cells of the device's own records in float64: (cells [ncells, 320], sum |term| likewise)."""
    body, envr, status = (t.tolist() for t in records_of(env))
    members = [[] for _ in range(ncells)]
    for e in range(env.num_envs):
        if status[e] != 0:
            members[cell_of(e)].append((status[e], envr[e], body[e]))
    rows = [_cell_row(m) for m in members]
    return (torch.tensor([r for r, _ in rows], dtype=torch.float64), torch.tensor([m for _, m in rows], dtype=torch.float64))


def exact_cell_columns():
    """The counts and the maximum / minimum columns of a cell row."""
    return [0, 4, 5, 6] + [8 + 13 * b + k for b in range(MB) for k in (8, 9, 10, 11, 12)]


def check_cells(got, env, cell_of, what):
    got = got.reshape(-1, NCOL)
    want, mag = cells_of(env, got.shape[0], cell_of)
    assert bool(((got - want).abs() <= 1e-12 * mag).all()), f"{what}: cells"
    ex = exact_cell_columns()
    assert torch.equal(got[:, ex], want[:, ex]), f"{what}: counts and max / min columns"
    return want


def scripted_env(task, n, device, seed=500):
    over = {"terrain.curriculum": False, "commands.curriculum": False} if task == "go2_parkour" else {}
    env, _, _ = E.make_env(task, n, device, **over)
    if task == "go2":
        E.bind_grid(env, torch.Generator().manual_seed(seed + n))
        assert par(env)["plane"]
    else:
        # the task's own grid is the cell key; levels and types redrawn over the 3 x 2 corner of it
        g = torch.Generator().manual_seed(seed + n)
        env.terrain_levels.copy_(torch.randint(0, E.ROWS, (n,), generator=g).to(env.device))
        env.terrain_types.copy_(torch.randint(0, E.COLS, (n,), generator=g).to(env.device))
        assert not par(env)["plane"]
        plant_terrain(env)
    return env


def script_tol(env):
    """The scripted runs' edge_tol: the relief of a 10-unit step, bit for bit (10 * vertical_scale in
    fp32), so that the planted 10-unit step is AT the tolerance and the 11-unit step its neighbour."""
    return float(f32(10) * par(env)["vscale"])


def run_script(env, steps, tol, every_call=None):
    ref = Restatement(env, tol)
    env.contact_begin()
    for t, s in enumerate(steps):
        write_inputs(env, s)
        env.contact_record()
        ref.record(s)
        if every_call is not None:
            every_call(t, ref)
    return ref


def scripted(task, n, device, every_call=False):
    """The script on a fresh env of the device: (env, restatement, steps)."""
    env = scripted_env(task, n, device)
    tol = script_tol(env)
    rows, cols = (E.ROWS, E.COLS)
    env.contact_buffers(rows, cols, edge_tol=tol)
    steps = script(n, torch.Generator().manual_seed(900 + n), par(env))
    check = (lambda t, ref: check_records(env, ref, f"{device} {task} n={n} call {t}")) if every_call else None
    return env, run_script(env, steps, tol, check), steps


def _grid_key(env):
    lv, ty = env.terrain_levels.cpu().tolist(), env.terrain_types.cpu().tolist()
    return lambda e: lv[e] * E.COLS + ty[e]


# ------------------------------------------------------------------ test bodies
def records_and_cells(task, n, device):
    """Case 1."""
    env, ref, steps = scripted(task, n, device, every_call=True)
    P, ee, tol = par(env), edge_env(n), script_tol(env)
    body, envr, status = ref.body, ref.env, ref.status
    r = body[ee]
    a = _nx(0.1, INF)
    # begin wrote the terminal columns' "none" and the edge env timed out with them untouched
    assert status[ee] == 1 and envr[ee, 0] == CALLS - 1 and envr[ee, 4:].tolist() == [-1.0, 0.0, -1.0, 0.0]
    # body 3: 0.1 N is no contact, its neighbour is; onset at the first sample, held, released, re-made
    assert a > float(f32(0.1)) and [float(s["contact_forces"][ee, 3, 2]) for s in steps[:4]] == [a, a, float(f32(0.1)), a]
    assert r[3, 1] == 3 and r[3, 2] == 2 and r[3, 0] == 0 and r[3, 4] == a and r[3, 11] == 0
    # body 4: 1 N is not over the termination threshold, its neighbour is; F.z = 0: every contact sample is a face hit
    assert r[4, 1] == 3 and r[4, 11] == 1 and r[4, 5] == 3 and r[4, 2] == 1 and r[4, 4] == _nx(1.0, INF)
    # body 5: fh == 5|F.z| is no face hit, its upper neighbour is
    assert r[5, 1] == 3 and r[5, 5] == 1
    assert r[7, 2] == 1 and r[7, 1] == 2 and r[8, 2] == 1
    if P["plane"]:
        assert bool((body[..., 8:11] == 0).all())  # a plane has no relief
        z = torch.stack([s["rigid_body_states"][ee, :P["nb"], 2] for s in steps[:CALLS - 1]]).double()
        assert r[:P["nb"], 7].tolist() == z.min(0).values.tolist()  # h = 0: column 7 is the lowest z
    else:
        hs = ref.hs
        # body 6 stood exactly on the boundary of cell KX (h from row KX: 40 units) and then below it (row KX - 1: 0)
        x0 = np.array([float(steps[0]["rigid_body_states"][ee, 6, 0]), float(steps[1]["rigid_body_states"][ee, 6, 0])], dtype=f32)
        y0 = np.full(2, float(steps[0]["rigid_body_states"][ee, 6, 1]), dtype=f32)
        h, _, ix, iy = ref.terrain(x0, y0)
        assert (x0[0] + P["border"]) / P["hscale"] == f32(KX) and ix.tolist() == [KX, KX - 1] and iy.tolist() == [YMID] * 2
        assert h.tolist() == [float(f32(40) * P["vscale"]), 0.0]
        # bodies 7, 8: the onset beside the 10-unit step is AT edge_tol (no edge), beside the 11-unit step over it
        assert r[7, 10] == tol and r[7, 9] == tol and r[7, 8] == 0
        assert r[8, 10] == float(f32(11) * P["vscale"]) > tol and r[8, 8] == 1
        # bodies 9..12: beyond the four borders, the clamped cells
        xs = np.array([float(steps[0]["rigid_body_states"][ee, b, 0]) for b in (9, 10, 11, 12)], dtype=f32)
        ys = np.array([float(steps[0]["rigid_body_states"][ee, b, 1]) for b in (9, 10, 11, 12)], dtype=f32)
        _, _, ix, iy = ref.terrain(xs, ys)
        assert ix[0] == 0 and ix[1] == P["rows"] - 2 and iy[2] == 0 and iy[3] == P["cols"] - 2
        assert xs[0] + P["border"] < 0 and ys[2] + P["border"] < 0
        assert (xs[1] + P["border"]) / P["hscale"] > P["rows"] and (ys[3] + P["border"]) / P["hscale"] > P["cols"]
        assert all(r[b, 2] == 1 for b in (9, 10, 11, 12))
        assert bool((body[..., 8] > 0).any()) and bool(((body[..., 2] > 0) & (body[..., 10] == 0)).any())
        assert hs.shape == (P["rows"], P["cols"])
    if n >= 63:
        assert status[:7].tolist() == [2, 1, 2, 2, 3, 0, 1] and set(status.tolist()) == {0, 1, 2, 3}
        assert envr[:7, 0].tolist() == [0, CALLS - 1, 5, 2, 4, CALLS, 7]
        assert envr[0].tolist() == [0, 0, 0, 0, -1, 0, -1, 0] and not body[0].any()  # fell at call 0 without any force
        # env 2: bodies 1 and 2 tie at 7 N: the lowest index of the termination list wins; the foot's 50 N is ignored
        multi = len(P["term"]) > 1
        assert P["term"] == ([0, 1, 2] if multi else [0])
        assert envr[2, 4:].tolist() == ([1.0, 7.0, 1.0, 3.0] if multi else [0.0, 3.0, 1.0, 1.0])
        # env 3: body 0 at exactly 1 N is no termination contact, but it is the hardest-hit non-foot body;
        # its second reset (call 6, 40 N everywhere) changed nothing
        assert envr[3, 4:].tolist() == [-1.0, 0.0, 0.0, 0.0]
        # envs 4 (blow-up) and 6 (time-out) ended with forces present: the begin values stay
        assert envr[4, 4:].tolist() == [-1.0, 0.0, -1.0, 0.0] and envr[6, 4:].tolist() == [-1.0, 0.0, -1.0, 0.0]
        nbd = P["nb"]
        assert all(body[:, :nbd, k].sum() > 0 for k in (1, 2, 5, 11)) and envr[:, 1].sum() > 0 and envr[:, 2].sum() > 0
        fell = status == 2
        assert bool((envr[fell, 4] >= 0).any()) and bool((envr[fell, 4] < 0).any())
    rows, cols = E.ROWS, E.COLS
    cells = env.contact_cells()
    assert cells.shape == (rows, cols, NCOL) and cells.dtype == torch.float64
    want = check_cells(cells, env, _grid_key(env), f"{device} {task} n={n} grid")
    counted = int((status != 0).sum())
    assert int(want[:, 0].sum()) == counted and (n < 63 or counted == n - 1)  # env 5 is in no cell
    assert n >= 63 or bool((want[:, 0] == 0).any())  # a single env leaves empty cells: all zero
    assert bool((cells.reshape(-1, NCOL)[want[:, 0] == 0] == 0).all())
    if n >= 63:
        assert want[:, 5].sum() == int((status == 2).sum()) and want[:, 6].sum() >= 2
        assert want[:, [8 + 13 * b + 11 for b in range(MB)]].sum() == want[:, 5].sum() - want[:, 6].sum()
    # a free cell key
    ids = torch.randint(0, 6, (n,), generator=torch.Generator().manual_seed(3), dtype=torch.int32).to(env.device)
    grid_set = env._contact
    env.contact_buffers(2, 3, ids, edge_tol=tol)
    assert env._contact is not grid_set
    run_script(env, steps, tol)
    idl = ids.cpu().tolist()
    cells = env.contact_cells()
    assert cells.shape == (2, 3, NCOL)
    check_cells(cells, env, lambda e: idl[e], f"{device} {task} n={n} cell_ids")
    # one id outside the grid: counted, cells untouched (the host backend fails the call too)
    ids[7 % n] = 6
    env._contact_cells.fill_(7.0)
    with pytest.raises(_native.LgxError, match="outside"):
        env.contact_cells()
    assert int(env._contact_overflow.item()) == 1 and bool((env._contact_cells == 7.0).all())
    ids[7 % n] = 0
    env.contact_cells()
    assert int(env._contact_overflow.item()) == 0
    # the first set kept its tensors
    assert env.contact_buffers(rows, cols, edge_tol=tol) is grid_set and env._contact_cells.shape == (rows, cols, NCOL)


def frozen_means_frozen(n, device):
    """Case 2: once every env has finished, nothing is written again."""
    env = scripted_env("go2", n, device)
    tol, P = script_tol(env), par(env)
    env.contact_buffers(E.ROWS, E.COLS, edge_tol=tol)
    gen = torch.Generator().manual_seed(1000 + n)
    last = script(n, gen, P, calls=1, scripted=False)[0]
    last["reset"] = torch.ones(n, dtype=torch.bool)  # everyone still recording ends here
    run_script(env, script(n, gen, P) + [last], tol)
    assert int((env.contact_status == 0).sum()) == 0
    cells = env.contact_cells()
    tensors = lambda: (env.contact_body, env.contact_env, env.contact_status, env._contact_cells)  # noqa: E731
    before = [t.clone() for t in tensors()]
    for i, s in enumerate(script(n, gen, P, calls=4, scripted=False)):
        s["reset"] = torch.full((n,), i % 2 == 1)  # samples and second resets (falls: time_out is clear)
        s["time_out"] = torch.zeros(n, dtype=torch.bool)
        write_inputs(env, s)
        env.contact_record()
    for a, b in zip(before, tensors()):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))  # no byte changed
    assert torch.equal(env.contact_cells(), cells)


def reduce_is_deterministic(n, device):
    """Case 3."""
    env, ref, _ = scripted("go2", n, device)
    a = env.contact_cells()
    env._contact_cells.fill_(-1.0)
    b = env.contact_cells()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    out = [e for e in range(n) if ref.status[e] == 0]
    assert n < 63 or 5 in out
    # the cells do not change when the records of the recording envs do
    for e in out:
        env.contact_body[e] = 1e6
        env.contact_env[e] = 1e6
    assert torch.equal(env.contact_cells(), a)
    # ... and do when they become countable
    if out:
        env.contact_status[out[0]] = 1
        assert not torch.equal(env.contact_cells(), a)


def kernels_match_host(task, n):
    """Case 4 (GPU file): the kernels against the host backend on the same script: statuses, records
    and cells bit for bit (the host backend forms its sums by cell_reduce's tree)."""
    env, ref, _ = scripted(task, n, "cuda:0")
    host, href, _ = scripted(task, n, "cpu")
    check_records(env, ref, f"hip {task} n={n}")
    check_records(host, href, f"host {task} n={n}")
    for x, y in ((env.contact_status, host.contact_status), (env.contact_env, host.contact_env),
                 (env.contact_body, host.contact_body)):
        assert torch.equal(x.cpu().view(torch.uint8), y.view(torch.uint8))
    a, b = env.contact_cells(), host.contact_cells()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))  # every column, sums included
    check_cells(a, env, _grid_key(env), f"hip {task} n={n} cells")
    # ... and under a free cell key (the same records in both backends' second set of buffers)
    ids = torch.randint(0, 6, (n,), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
    saved = [t.clone() for t in (host.contact_body, host.contact_env, host.contact_status)]
    for dev_env in (env, host):
        dev_env.contact_buffers(2, 3, ids.to(dev_env.device), edge_tol=script_tol(dev_env))
        for dst, src in zip((dev_env.contact_body, dev_env.contact_env, dev_env.contact_status), saved):
            dst.copy_(src)
    a, b = env.contact_cells(), host.contact_cells()
    assert a.shape == (2, 3, NCOL) and bool((a[..., 0] > 0).all())
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))


# The physics runs use the seed-1 initial networks (they stand and shuffle: foot onsets, time-outs) and
# make every second env limp (motor strength LIMP): it drops onto its trunk within the 30-step
# episode, a fall that a termination contact ends. Chosen on the host backend; the test bodies assert
# the outcome.
LIMP = 0.0


def evaluator(task, n, device, seed=1, **over):
    from legged_gym_custom_amd.utils.evaluator import PolicyEvaluator
    over.setdefault("env.episode_length_s", 0.59)  # ceil(0.59 / 0.02) = 30 steps
    if task == "go2_parkour":
        # roughness on every tile: the start platforms are flat otherwise, and no onset would see relief
        over.update({"terrain.curriculum": False, "commands.curriculum": False,
                     "terrain.add_roughness_to_selected_terrain": True})
    env, tcfg, args = E.make_env(task, n, device, seed=seed, **over)
    assert int(env.max_episode_length) == 30
    strength = torch.ones(n)
    strength[::2] = LIMP
    env.set_motor_strength(strength.to(env.device))
    return PolicyEvaluator(env, E.make_runner(env, tcfg, args))


def _strip(t):
    return {k: v for k, v in t.items() if k != "contacts"}


def end_to_end(task, n, device):
    """Case 5: real physics. The eager loop with the source tensors copied after each step into the
    restatement, the same as a run, a run without the record; on the GPU a second evaluator replays
    its graph."""
    plain = evaluator(task, n, device)
    rp = plain.run(graph=False)
    base_cells = plain.last_cells.clone()
    assert plain.last_contact_cells is None and "contacts" not in rp["total"]
    a = evaluator(task, n, device)
    env = a.env
    P = par(env)
    steps = int(env.max_episode_length) + 1
    a._set_trace(None, False, False, True)
    env.contact_buffers(edge_tol=EDGE_RELIEF_M)
    ref = Restatement(env, EDGE_RELIEF_M)
    a.begin()
    for _ in range(steps):
        a.step()
        ref.record(read_inputs(env))
    check_records(env, ref, f"{device} {task} n={n} end to end")
    body, envr, status = (t.clone() for t in (env.contact_body, env.contact_env, env.contact_status))
    ra = a.run(graph=False, contacts=True)
    assert ra["graph"] is False and ra["num_steps"] == steps and ra["total"]["running"] == 0
    cells, ccells = a.last_cells.clone(), a.last_contact_cells.clone()
    for x, y in zip((env.contact_body, env.contact_env, env.contact_status), (body, envr, status)):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))  # bit for bit
    assert torch.equal(status, env.eval_status) and int((status == 0).sum()) == 0
    assert torch.equal(envr[:, 0], env.eval_acc[:, 0])
    if getattr(env, "terrain_levels", None) is None:
        key = lambda e: 0  # noqa: E731  (no terrain grid: one cell)
    else:
        lv, ty, ncols = env.terrain_levels.cpu().tolist(), env.terrain_types.cpu().tolist(), ccells.shape[1]
        key = lambda e: lv[e] * ncols + ty[e]  # noqa: E731
    check_cells(ccells, env, key, f"{device} {task} n={n} cells")
    got = a.contact_records()
    assert got["body"].shape == (n, MB, 12) and got["env"].shape == (n, 8) and got["status"].shape == (n,)
    # the conditions the seed and the policy were chosen for
    b, v, st = body.cpu(), envr.cpu(), status.cpu()
    fell = st == 2
    caused = fell & (v[:, 4] >= 0)
    print(f"{task} n={n}: statuses {torch.bincount(st.long(), minlength=4).tolist()}, falls with a termination contact "
          f"{int(caused.sum())}, foot onsets {int(b[:, P['feet'], 2].sum())}, onsets with relief "
          f"{int((b[..., 10] > 0).sum())} bodies, on an edge {int(b[..., 8].sum())}")
    assert int(fell.sum()) >= 1 and int(caused.sum()) >= 1
    for e in caused.nonzero().flatten().tolist():
        assert int(v[e, 4]) in P["term"] and float(v[e, 5]) > 1.0 and float(v[e, 7]) >= 1.0
    assert float(b[:, P["feet"], 2].sum()) >= 1
    if not P["plane"]:
        assert bool((b[..., 10] > 0).any())
    c = ra["total"]["contacts"]
    assert c["envs"] == n and c["samples"] == int(v[:, 0].sum()) and set(c["bodies"]) == set(env.body_names)
    assert c["falls"] == int(fell.sum()) and abs(sum(c["fall_causes"].values()) - 1.0) < 1e-12
    assert len(ra["cells"]) == ccells.shape[0] and all("contacts" in x for row in ra["cells"] for x in row)
    # the record perturbs nothing
    assert torch.equal(cells, base_cells)
    assert _strip(ra["total"]) == rp["total"]
    assert [[_strip(x) for x in row] for row in ra["cells"]] == rp["cells"]
    rq = a.run(graph=False)
    assert torch.equal(a.last_cells, cells) and a.last_contact_cells is None and rq["total"] == rp["total"]
    if device == "cpu":
        return
    b2 = evaluator(task, n, device)
    rb = b2.run(contacts=True)
    assert rb["graph"] is True
    assert torch.equal(b2.last_cells, cells)
    assert torch.equal(b2.last_contact_cells.view(torch.int64), ccells.view(torch.int64))
    for x, y in zip((b2.env.contact_body, b2.env.contact_env, b2.env.contact_status), (body, envr, status)):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))  # graph replay = the eager loop, bit for bit
    with_contacts = b2._graph
    b2.run()
    assert b2._graph is not with_contacts and torch.equal(b2.last_cells, cells)  # keyed by the flag: recaptured


def terminal_forces(device, n=64):
    """Case 6: at the step that resets an env, contact_forces[e] still holds the forces of that step's
    physics: every fall is explained by a termination body over 1 N in the tensor read back or by
    projected_gravity.z > 0 (go2 is no parkour task: there is no third cause), and the recorded env
    column 4 is the argmax over that tensor. projected_gravity read back after the step is the value the
    termination check saw: the step computes it before the check and stores it after the in-step reset,
    which rewrites the root state but not it (as the reference's reset leaves it), so a fall by
    orientation alone shows z > 0 here. Both kinds of fall happen in this set-up and both are asserted."""
    a = evaluator("go2", n, device)
    env = a.env
    P = par(env)
    a._set_trace(None, False, False, True)
    env.contact_buffers(edge_tol=EDGE_RELIEF_M)
    a.begin()
    seen = by_contact = by_orientation = 0
    done = torch.zeros(n, dtype=torch.bool)
    for _ in range(int(env.max_episode_length) + 1):
        a.step()
        reset, tout = env.reset_buf.cpu().bool(), env.time_out_buf.cpu().bool()
        F = env._contact3.detach().cpu().numpy().astype(f32)
        pg = env.projected_gravity.detach().cpu()
        fn = np.sqrt(F[..., 0] * F[..., 0] + F[..., 1] * F[..., 1] + F[..., 2] * F[..., 2])
        v = env.contact_env.cpu()
        for e in (reset & ~tout & ~done).nonzero().flatten().tolist():
            over = [b for b in P["term"] if fn[e, b] > f32(1.0)]
            assert over or float(pg[e, 2]) > 0.0, f"env {e}: a fall that neither the forces nor the orientation explain"
            want = max(over, key=lambda b: (fn[e, b], -b)) if over else -1
            assert int(v[e, 4]) == want and float(v[e, 5]) == (float(fn[e, want]) if over else 0.0)
            assert int(env.contact_status[e]) == 2
            seen, by_contact = seen + 1, by_contact + bool(over)
            by_orientation += (not over) and float(pg[e, 2]) > 0.0
        done |= reset
    print(f"terminal forces on {device}: {seen} falls, {by_contact} by a termination contact, "
          f"{by_orientation} by orientation alone")
    assert seen >= 1 and by_contact >= 1 and by_orientation >= 1 and by_contact + by_orientation == seen


def composition(device):
    """Case 7."""
    import json
    ev = evaluator("go2", 64, device, **{"domain_rand.scheduled_pushes": True, "commands.scheduled_commands": True})
    plain = ev.run()
    assert "contacts" not in plain["total"]
    solo = ev.run(gait=True, joints=True, trace_depth=4)
    gait, joints, trace = ev.last_gait_cells.clone(), ev.last_joint_cells.clone(), ev.traces([0])["trace"].copy()
    key_without, graph_without = ev._graph_key, ev._graph
    rt = ev.run(gait=True, joints=True, trace_depth=4, contacts=True)
    assert rt["graph"] == (device != "cpu")
    if rt["graph"]:  # distinct graph keys: switching the flag re-captures
        assert ev._graph_key != key_without and ev._graph is not graph_without
    assert torch.equal(ev.last_gait_cells.view(torch.int64), gait.view(torch.int64))
    assert torch.equal(ev.last_joint_cells.view(torch.int64), joints.view(torch.int64))
    assert (ev.traces([0])["trace"].view(np.uint32) == trace.view(np.uint32)).all()
    assert _strip(rt["total"]) == solo["total"]
    assert rt["total"]["contacts"]["envs"] == 64 and rt["total"]["gait"]["envs"] == 64
    assert all("contacts" in c and "gait" in c and "joints" in c for row in rt["cells"] for c in row)
    assert sum(c["contacts"]["envs"] for row in rt["cells"] for c in row) == 64
    kw = dict(at_s=0.1, gait=True, joints=True, trace_depth=4)
    rc0 = ev.run_command_test([0.0, 1.0], vy=(0.0,), yaw=(0.0, 0.5), steady_after_s=0.1, **kw)
    gait, joints = ev.last_gait_cells.clone(), ev.last_joint_cells.clone()
    rc = ev.run_command_test([0.0, 1.0], vy=(0.0,), yaw=(0.0, 0.5), steady_after_s=0.1, contacts=True, **kw)
    assert torch.equal(ev.last_gait_cells, gait) and torch.equal(ev.last_joint_cells, joints)
    assert _strip(rc["total"]) == rc0["total"] and rc["total"]["contacts"]["envs"] == 64
    got = [rc["bins"][ix][0][iw]["contacts"] for ix in range(2) for iw in range(2)]
    assert [g["envs"] for g in got] == [16] * 4 and all(g["samples"] > 0 for g in got)
    rp0 = ev.run_push_test([0.0, 1.0], directions=2, **kw)
    gait, joints = ev.last_gait_cells.clone(), ev.last_joint_cells.clone()
    rp = ev.run_push_test([0.0, 1.0], directions=2, contacts=True, **kw)
    assert torch.equal(ev.last_gait_cells, gait) and torch.equal(ev.last_joint_cells, joints)
    assert _strip(rp["total"]) == rp0["total"]
    got = [rp["bins"][s][d]["contacts"] for s in range(2) for d in range(2)]
    assert [g["envs"] for g in got] == [16] * 4 and rp["total"]["contacts"]["envs"] == 64
    json.dumps([rc, rp, rt], allow_nan=False)
    again = ev.run()
    assert "contacts" not in again["total"] and all("contacts" not in c for row in again["cells"] for c in row)
    assert again["total"] == plain["total"] and again["cells"] == plain["cells"]
    with pytest.raises(RuntimeError, match="contact"):
        ev.contact_records()


def _hand_row(envs=4, samples=400, falls=4):
    """A contact cell row [320] made by hand for a 5-body robot (base, thigh, calf, foot_a, foot_b)."""
    row = [0.0] * NCOL
    row[0:8] = [envs, samples, 100.0, 40.0, 55.0, falls, 1.0, 5.0]
    blocks = {0: [20.0, 4.0, 8.0, 5.0, 120.0, 0.0, 0.0, 16.0, 44.0, 0.0, 0.25, 2.0, 3.0],
              1: [40.0, 10.0, 4.0, 30.0, 80.0, 4.0, 0.5, 8.0, 55.0, 0.125, 0.0625, 1.0, 1.0],
              3: [200.0, 50.0, 400.0, 2.0, 20.0, 5.0, 1.0, 200.0, 90.0, 0.25, 0.0, 0.0, 0.0],
              4: [300.0, 50.0, 600.0, 0.0, 24.0, 15.0, 3.0, 300.0, 95.0, 0.5, 0.015625, 0.0, 0.0]}
    for b, v in blocks.items():
        row[8 + 13 * b: 8 + 13 * (b + 1)] = v
    return row


def report():
    """Case 8: contact_cell_report and contact_total_row on hand-made rows, without a device."""
    import json
    from legged_gym_custom_amd.utils import evaluator as M
    assert M.EDGE_RELIEF_M == 0.05
    names = ["base", "thigh", "calf", "foot_a", "foot_b"]
    args = (0.02, names, [3, 4], [0, 1], [0, 1, 2])
    r = M.contact_cell_report(_hand_row(), *args)
    json.dumps(r, allow_nan=False)
    assert r["envs"] == 4 and r["samples"] == 400 and r["falls"] == 4 and list(r["bodies"]) == names  # the name mapping
    assert r["collision_share"] == 0.1 and r["mean_penalised_in_contact"] == 0.25 and r["peak_nonfoot_force"] == 55.0
    assert r["mean_termination_bodies_at_fall"] == 1.25
    assert r["fall_causes"] == {"base": 0.5, "thigh": 0.25, "no_contact": 0.25} and sum(r["fall_causes"].values()) == 1.0
    assert r["hardest_hit_at_fall"] == {"base": 0.75, "thigh": 0.25, "calf": 0.0, "no_contact": 0.0}
    assert r["foot_edge_onset_share"] == 0.2
    t = r["bodies"]["thigh"]
    assert t["contact_share"] == 0.1 and t["onsets_per_s"] == 1.25 and t["mean_force_in_contact"] == 5.0
    assert t["peak_force"] == 55.0 and t["face_hit_share"] == 0.75 and t["hard_share"] == 0.02
    assert t["mean_height_above_terrain_m"] == 0.2 and t["min_height_above_terrain_m"] == 0.0625
    assert t["edge_onset_share"] == 0.4 and t["mean_onset_relief_m"] == 0.05 and t["max_onset_relief_m"] == 0.125
    assert t["roles"] == ["termination", "penalised"] and r["bodies"]["foot_a"]["roles"] == ["foot"]
    assert r["bodies"]["foot_b"]["edge_onset_share"] == 0.3 and r["bodies"]["calf"]["roles"] == ["penalised"]
    idle = r["bodies"]["calf"]
    assert idle["contact_share"] == 0.0 and idle["mean_force_in_contact"] is None and idle["edge_onset_share"] is None
    assert idle["max_onset_relief_m"] is None and idle["peak_force"] == 0.0
    # no falls: no causes
    calm = _hand_row(falls=0)
    calm[6] = calm[7] = 0.0
    rc = M.contact_cell_report(calm, *args)
    assert rc["falls"] == 0 and rc["fall_causes"] is None and rc["hardest_hit_at_fall"] is None
    assert rc["mean_termination_bodies_at_fall"] is None
    # an empty row: None everywhere, JSON without NaN
    empty = M.contact_cell_report([0.0] * NCOL, *args)
    assert "NaN" not in json.dumps(empty, allow_nan=False)
    assert empty["envs"] == 0 and empty["samples"] == 0 and empty["falls"] == 0
    assert all(v is None for k, v in empty.items() if k not in ("envs", "samples", "falls", "bodies"))
    assert all(v is None for b in empty["bodies"].values() for k, v in b.items() if k != "roles")
    # the total: sums added, max of maxima, min of minima over the cells with samples only
    one, two = _hand_row(), _hand_row(envs=2, samples=100)
    two[4], two[8 + 13 + 8], two[8 + 13 + 9], two[8 + 13 + 10], two[8 + 10] = 70.0, 20.0, 0.5, 0.03125, 0.5
    nosamples = [0.0] * NCOL
    nosamples[0] = nosamples[5] = nosamples[6] = 1.0  # one env that fell at its first step
    total = M.contact_total_row(torch.tensor([one, [0.0] * NCOL, two, nosamples], dtype=torch.float64))
    assert total.shape == (NCOL,) and total[0] == 7 and total[1] == 500 and total[5] == 9 and total[6] == 3
    assert total[4] == 70.0 and total[8 + 13 + 8] == 55.0 and total[8 + 13 + 9] == 0.5
    assert total[8 + 13 + 10] == 0.03125 and total[8 + 10] == 0.25  # not the 0 of the cells without samples
    assert total[8 + 13 * 3] == 400.0
    assert bool((M.contact_total_row(torch.zeros(2, 3, NCOL, dtype=torch.float64)) == 0).all())
    # ... which is the report of the concatenated envs: the same row as one cell holding all of them
    both = M.contact_cell_report(total, *args)
    assert both["envs"] == 7 and both["falls"] == 9 and abs(sum(both["fall_causes"].values()) - 1.0) < 1e-12
    assert both["bodies"]["thigh"]["contact_share"] == 80.0 / 500.0


def total_matches_concatenation(device, n=63):
    """Case 8, second half: contact_total_row over the grid's cells = the cells of the same envs under
    one key (a 1 x 1 grid), sums to the reduce's bound, counts and extremes exactly."""
    from legged_gym_custom_amd.utils import evaluator as M
    env, ref, steps = scripted("go2", n, device)
    tol = script_tol(env)
    total = M.contact_total_row(env.contact_cells())
    env.contact_buffers(1, 1, torch.zeros(n, dtype=torch.int32, device=env.device), edge_tol=tol)
    run_script(env, steps, tol)
    one = env.contact_cells().reshape(NCOL)
    _, mag = cells_of(env, 1, lambda e: 0)
    assert bool(((total - one).abs() <= 2e-12 * mag[0]).all())
    ex = exact_cell_columns()
    assert torch.equal(total[ex], one[ex])
    args = (float(env.dt), env.body_names, env.feet_indices.tolist(), env.termination_contact_indices.tolist(),
            env.penalised_contact_indices.tolist())
    ra, rb = M.contact_cell_report(total, *args), M.contact_cell_report(one, *args)
    assert ra["fall_causes"] == rb["fall_causes"] and ra["hardest_hit_at_fall"] == rb["hardest_hit_at_fall"]
    assert ra["falls"] == rb["falls"] == int((ref.status == 2).sum())


def refusals(device):
    """Case 9: each failure raises with a message naming its cause and writes nothing."""
    import ctypes
    env, _, _ = scripted("go2", 63, device)
    tol = script_tol(env)
    tensors = lambda: (env.contact_body, env.contact_env, env.contact_status, env._contact_cells)  # noqa: E731
    env.contact_cells()
    before = [t.clone() for t in tensors()]
    same = lambda: all(torch.equal(a, b) for a, b in zip(before, tensors()))  # noqa: E731
    env.reset_buf.zero_()  # a record that went ahead would add a sample to every recording env
    nat, st = env._native, env._stream()
    good = dict(body=env.contact_body, env=env.contact_env, status=env.contact_status, cells=env._contact_cells,
                overflow=env._contact_overflow)

    def raw(rows=E.ROWS, cols=E.COLS, edge_tol=tol, **over):
        cb = _abi.ContactBuffers()
        for k, t in {**good, **over}.items():
            setattr(cb, k, None if t is None else t.data_ptr())
        cb.cell_rows, cb.cell_cols, cb.edge_tol = rows, cols, edge_tol
        return cb

    calls = {"begin": lambda cb: nat.contact_begin(cb, st), "record": lambda cb: nat.contact_record(cb, st),
             "reduce": lambda cb: nat.contact_reduce(cb, st)}
    for member in ("body", "env", "status", "overflow"):
        for name, call in calls.items():
            with pytest.raises(_native.LgxError, match=f"lgx_contact_{name}: {member} is NULL"):
                call(raw(**{member: None}))
    with pytest.raises(_native.LgxError, match="lgx_contact_reduce: cells is NULL"):
        calls["reduce"](raw(cells=None))
    for rows, cols in ((0, 2), (3, 0), (-1, 2), (1 << 11, 1 << 10)):
        for name, call in calls.items():
            with pytest.raises(_native.LgxError, match=f"lgx_contact_{name}: cell_rows and cell_cols"):
                call(raw(rows, cols))
    for bad_tol in (float("nan"), INF, -INF, -1e-6):
        for name, call in calls.items():
            with pytest.raises(_native.LgxError, match=f"lgx_contact_{name}: edge_tol"):
                call(raw(edge_tol=bad_tol))
    # 4 bytes off a 16-byte boundary (never dereferenced: the call refuses first)
    off_body = torch.zeros(63 * MB * 12 + 1, device=env.device)[1:].view(63, MB, 12)
    off_env = torch.zeros(63 * 8 + 1, device=env.device)[1:].view(63, 8)
    for name, call in calls.items():
        with pytest.raises(_native.LgxError, match=f"lgx_contact_{name}: body must be 16-byte aligned"):
            call(raw(body=off_body))
        with pytest.raises(_native.LgxError, match=f"lgx_contact_{name}: env must be 16-byte aligned"):
            call(raw(env=off_env))
    L = _native.lib()
    for fn in (L.lgx_contact_begin, L.lgx_contact_record, L.lgx_contact_reduce):
        assert fn(nat.handle, None, None) < 0 and b"contact buffers are NULL" in L.lgx_last_error(nat.handle)
    for member in ("body", "env", "status", "cells", "overflow"):
        with pytest.raises(_native.LgxError, match=f"contact buffer {member} is required"):
            nat.contact_buffers(**{**good, member: None})
    with pytest.raises(_native.LgxError, match="contact buffer body must be"):
        nat.contact_buffers(**{**good, "body": env.contact_body[:, :3].contiguous()})
    with pytest.raises(_native.LgxError, match="contact buffer env must be"):
        nat.contact_buffers(**{**good, "env": env.contact_env.double()})
    with pytest.raises(_native.LgxError, match="contact buffer cells must be"):
        nat.contact_buffers(**{**good, "cells": env._contact_cells[..., :61].contiguous()})
    with pytest.raises(_native.LgxError, match="contact buffer cell_ids must be"):
        nat.contact_buffers(**good, cell_ids=torch.zeros(63, dtype=torch.int64, device=env.device))
    assert same()
    # unbound source buffers
    for attr, name in (("_contact3", "contact_forces"), ("rigid_body_states", "rigid_body_states"),
                       ("reset_buf", "reset"), ("time_out_buf", "time_out")):
        keep = getattr(env, attr)
        setattr(env, attr, None)
        try:
            env._bind()
        except _native.LgxError as err:  # lgx_bind itself requires this one
            assert name in str(err)
        else:
            for call, cname in ((env.contact_begin, "begin"), (env.contact_record, "record"), (env.contact_cells, "reduce")):
                with pytest.raises(_native.LgxError, match=f"lgx_contact_{cname}.*not bound: {name}"):
                    call()
        setattr(env, attr, keep)
        env._bind()
    assert same()

    # params the record cannot use (a second native env on the same tensors, never stepped). Returns
    # the layer that refused: "record" (each of the three calls, with a message matching `match`), or
    # "create" / "bind" with that layer's message.
    def with_params(native, change, match, keep=None, bufs=None):
        params = type(native.params)()
        ctypes.memmove(ctypes.byref(params), ctypes.byref(native.params), ctypes.sizeof(params))
        change(params)
        try:
            bad = _native.NativeEnv(native.model, params, native.device_index)
        except _native.LgxError as err:
            return "create", str(err)
        try:
            bad.bind(native._keep if keep is None else keep)
        except _native.LgxError as err:
            return "bind", str(err)
        cb = bad.contact_buffers(**(good if bufs is None else bufs), edge_tol=tol)
        for name, call in (("begin", bad.contact_begin), ("record", bad.contact_record), ("reduce", bad.contact_reduce)):
            with pytest.raises(_native.LgxError, match=f"lgx_contact_{name}: {match}"):
                call(cb, st)
        return "record", match

    nbd = int(nat.params.num_bodies)
    # lgx_create and lgx_bind take any index tables and counts: each of these reaches the record's own check
    for change, match in (
            (lambda p: p.feet_idx.__setitem__(1, nbd), "feet_idx outside the bodies"),
            (lambda p: p.termination_idx.__setitem__(0, nbd), "termination_idx outside the bodies"),
            (lambda p: p.termination_idx.__setitem__(0, -1), "termination_idx outside the bodies"),
            (lambda p: p.penalised_idx.__setitem__(2, nbd), "penalised_idx outside the bodies"),
            (lambda p: p.penalised_idx.__setitem__(0, -1), "penalised_idx outside the bodies"),
            (lambda p: setattr(p, "n_termination", _abi.MAX_TERMINATION + 1), "n_termination outside termination_idx"),
            (lambda p: setattr(p, "n_termination", -1), "n_termination outside termination_idx"),
            (lambda p: setattr(p, "n_penalised", _abi.MAX_PENALISED + 1), "n_penalised outside penalised_idx"),
            (lambda p: setattr(p, "n_penalised", -1), "n_penalised outside penalised_idx"),
            (lambda p: setattr(p, "num_bodies", MB + 1), r"num_bodies outside \[0, LGX_MAX_BODIES\]"),
            (lambda p: setattr(p, "num_bodies", -1), r"num_bodies outside \[0, LGX_MAX_BODIES\]")):
        assert with_params(nat, change, match)[0] == "record", match
    assert same()
    # a heightfield too small for the nine samples
    park = scripted_env("go2_parkour", 8, device)
    pn = park._native

    def small_rows(p):
        p.hf_rows = 2

    def small_cols(p):
        p.hf_cols = 2
    pk = park.contact_buffers(E.ROWS, E.COLS, edge_tol=tol)
    pbufs = dict(zip(("body", "env", "status", "cells", "overflow"), pk._keep[:5]))
    assert with_params(pn, small_rows, "hf_rows and hf_cols must be >= 3", bufs=pbufs)[0] == "record"
    assert with_params(pn, small_cols, "hf_rows and hf_cols must be >= 3", bufs=pbufs)[0] == "record"
    # a mesh without height samples: lgx_bind itself refuses it and names the buffer, so the record's own
    # check of it (contact_check, "not bound: height_samples") is a guard that the public API cannot reach
    no_hs = {k: v for k, v in pn._keep.items() if k != "height_samples"}
    layer, msg = with_params(pn, lambda p: None, "not bound: height_samples", keep=no_hs, bufs=pbufs)
    assert layer == "bind" and "height_samples" in msg
    # no record yet
    other, _, _ = E.make_env("go2", 8, device)
    for call in (other.contact_begin, other.contact_record, other.contact_cells):
        with pytest.raises(RuntimeError, match="contact_buffers"):
            call()
    env.contact_record()  # and the first env's record is still usable
    assert not same()
