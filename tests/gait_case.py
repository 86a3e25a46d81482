"""Shared by tests/test_gait_host.py and tests/test_gpu_gait.py: the gait record (include/lgx.h ABI 12:
lgx_gait_begin / lgx_gait_record / lgx_gait_reduce) on one device. A scripted sequence of inputs
written straight into the env's tensors (no physics step, the style of trace_case.write_inputs), a
restatement of the rule text in plain Python lists of float64, and the test bodies, parameterised
by the device.

Bounds (from the number formats, not from the code under test; u = 2^-24):
* foot columns 0, 1, 4-9 and 15 and every body column are integers below 2^24: exact. Columns 2 and
  3 are copies (column 3 a maximum of copies): exact.
* columns 11, 12 and 14 are fp32 running sums of T non-negative terms, each term at most 4 u off
  (two squares, their sum, the square root, the product with the fp32 dt): relative error at most
  (T + 3) u, T taken per entry from the restatement's count of terms.
* column 13 is a maximum of fp32 3-norms: rtol 1e-6, eval_case.py's bound.
* column 10 is a signed fp32 sum of k differences of copies: absolute error at most
  (k + 1) u sum |term|.
* the contact test F.z > 1.0f on a copied value is exact. The stumble test compares two rounded
  fp32 values: the restatement must find no sample with |fh - 5 |F.z|| <= 1e-5 fh (all-zero
  samples excluded); the seeds are fixed so that it finds none, and the tests assert it.
* cells are fp64 sums of at most 130 fp32 records by a fixed tree: against the float64 sum of the
  device's own records (which the tests above bound), |error| <= 1e-12 sum |term|."""
import math

import pytest
import torch

import eval_case as E
from legged_gym_custom_amd import _abi, _native

CALLS, NB = 12, 19
U = 2.0 ** -24
EXACT = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15]
SUMS = [11, 12, 14]
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
SOURCES = ("contact_forces", "rigid_body_states", "reset", "time_out", "blew_up")


def script(n, gen, feet, calls=CALLS, scripted=True):
    """`calls` steps of inputs (CPU tensors): forces randn x 80, foot heights in [0, 1] m, foot
    velocities with |v| <= 2 m/s. For n >= 63 (and scripted): env 0 resets at the first call; env 1 has
    foot 0 always in stance, foot 1 always in swing, foot 2 alternating every call, foot 3 stance 3 /
    swing 2, and times out at the last call; env 2's foot 0 swings, stands for two calls, lifts off
    at call 3 and the env falls at call 5, in the middle of that observed swing; env 3 falls at call
    2 and resets again at call 6; env 4 blows up at call 4 with time_out also set; env 5 never
    resets; the rest reset once at a random call, half of them as time-outs. A single env times out
    at the last call."""
    steps = []
    when = torch.randint(0, calls, (n,), generator=gen)
    as_timeout = torch.rand(n, generator=gen) < 0.5
    fixed = scripted and n >= 63
    for t in range(calls):
        cf = 80.0 * torch.randn(n, NB, 3, generator=gen)
        rb = torch.randn(n, NB, 13, generator=gen)
        rb[..., 2] = torch.rand(n, NB, generator=gen)
        rb[..., 7:9] = (2.0 * torch.rand(n, NB, 2, generator=gen) - 1.0) * math.sqrt(2.0)
        reset = when == t
        tout = reset & as_timeout
        blew = torch.zeros(n, dtype=torch.bool)
        if scripted and n < 63:
            reset[:] = tout[:] = t == calls - 1
        if fixed:
            reset[:6] = torch.tensor([t == 0, t == calls - 1, t == 5, t in (2, 6), t == 4, False])
            tout[:6] = torch.tensor([False, t == calls - 1, False, False, t == 4, False])
            blew[4] = t == 4
            want = {(1, 0): True, (1, 1): False, (1, 2): t % 2 == 0, (1, 3): t % 5 < 3, (2, 0): t in (1, 2)}
            for (e, f), stance in want.items():
                z = cf[e, feet[f], 2].abs()
                cf[e, feet[f], 2] = 2.0 + z if stance else 0.25
        steps.append(dict(contact_forces=cf, rigid_body_states=rb, reset=reset, time_out=tout, blew_up=blew))
    return steps


def _tensors(env):
    """The env tensors the record reads, by lgx_buffers name."""
    return dict(contact_forces=env._contact3, rigid_body_states=env.rigid_body_states_view, reset=env.reset_buf,
                time_out=env.time_out_buf, blew_up=env.blew_up_buf)


def write_inputs(env, s):
    """One scripted step into the tensors the native env is bound to."""
    dst = _tensors(env)
    assert dst["contact_forces"].shape[1:] == (NB, 3) and dst["rigid_body_states"].shape[1:] == (NB, 13)
    for k in SOURCES:
        dst[k].copy_(s[k])


def read_inputs(env):
    """The same tensors after a real step, as CPU copies."""
    return {k: t.detach().cpu().clone() for k, t in _tensors(env).items()}


class Restatement:
    """lgx_gait_record restated from the rule text: plain Python lists of float64 per env and foot."""

    def __init__(self, n, feet, dt):
        self.n, self.feet = n, [int(f) for f in feet]
        self.dt = float(torch.tensor(float(dt), dtype=torch.float32))  # params.dt is an fp32
        self.foot = [[[0.0] * 16 for _ in range(4)] for _ in range(n)]
        self.body = [[0.0] * 12 for _ in range(n)]
        self.status = [0] * n
        self.terms = [[{11: 0, 12: 0, 14: 0} for _ in range(4)] for _ in range(n)]  # terms of each sum
        self.abs10 = [[0.0] * 4 for _ in range(n)]  # sum |term| of column 10
        self.near_ties = 0  # samples whose stumble test fp32 could decide differently

    def record(self, s):
        cf = s["contact_forces"].detach().cpu().double().reshape(self.n, -1, 3).tolist()
        rb = s["rigid_body_states"].detach().cpu().double().reshape(self.n, -1, 13).tolist()
        reset, tout, blew = (s[k].detach().cpu().bool().tolist() for k in ("reset", "time_out", "blew_up"))
        dt = self.dt
        for e in range(self.n):
            if self.status[e] != 0:
                continue
            if reset[e]:
                self.status[e] = 3 if blew[e] else (1 if tout[e] else 2)
                continue
            body = self.body[e]
            first = body[0] == 0
            cs = []
            for f, b in enumerate(self.feet):
                F, R, r = cf[e][b], rb[e][b], self.foot[e][f]
                c = F[2] > 1.0
                z = R[2]
                vh = math.sqrt(R[7] ** 2 + R[8] ** 2)
                fh = math.sqrt(F[0] ** 2 + F[1] ** 2)
                fn = math.sqrt(F[0] ** 2 + F[1] ** 2 + F[2] ** 2)
                if first:
                    r[0], r[1] = float(c), 0.0
                else:
                    p = r[0] != 0
                    if c and not p:
                        r[5] += 1
                        r[13] = max(r[13], fn)
                        if r[1] > 0:
                            r[8] += 1
                            r[9] += r[1]
                            r[10] += r[3] - r[2]
                            self.abs10[e][f] += abs(r[3] - r[2])
                        r[1] = 1.0
                    elif p and not c:
                        if r[1] > 0:
                            r[6] += 1
                            r[7] += r[1]
                        r[1] = 1.0
                        r[3] = z
                    else:
                        r[1] = r[1] + 1 if r[1] > 0 else 0.0
                    r[0] = float(c)
                if c:
                    r[4] += 1
                    r[11] += vh * dt
                    r[12] += F[2]
                    r[2] = z
                    self.terms[e][f][11] += 1
                    self.terms[e][f][12] += 1
                else:
                    r[3] = z if first else max(r[3], z)
                    r[14] += vh * dt
                    self.terms[e][f][14] += 1
                if fh > 5 * abs(F[2]):
                    r[15] += 1
                if (fh != 0 or F[2] != 0) and abs(fh - 5 * abs(F[2])) <= 1e-5 * fh:
                    self.near_ties += 1
                cs.append(c)
            body[0] += 1
            body[1 + sum(cs)] += 1
            for i, (a, b) in enumerate(PAIRS):
                if b < len(cs):
                    body[6 + i] += cs[a] == cs[b]


def check_records(env, ref, what, scale=1.0):
    """The device's records against the restatement's at the bounds of the module docstring (scale:
    2 for a comparison of two fp32 implementations)."""
    foot, body = env.gait_foot.detach().cpu().double(), env.gait_body.detach().cpu().double()
    assert env.gait_status.cpu().tolist() == ref.status, f"{what}: status"
    assert torch.equal(body, torch.tensor(ref.body, dtype=torch.float64)), f"{what}: body columns"
    want = torch.tensor(ref.foot, dtype=torch.float64)
    assert foot.shape == want.shape == (ref.n, 4, 16)
    assert torch.equal(foot[..., EXACT], want[..., EXACT]), f"{what}: exact foot columns"
    terms = torch.tensor([[[t[k] for k in SUMS] for t in fe] for fe in ref.terms], dtype=torch.float64)
    err = (foot[..., SUMS] - want[..., SUMS]).abs()
    assert bool((err <= scale * (terms + 3) * U * want[..., SUMS]).all()), f"{what}: sum columns {float(err.max()):.3e}"
    assert bool(((foot[..., 13] - want[..., 13]).abs() <= scale * 1e-6 * want[..., 13]).all()), f"{what}: column 13"
    bound = scale * (want[..., 8] + 1) * U * torch.tensor(ref.abs10, dtype=torch.float64)
    assert bool(((foot[..., 10] - want[..., 10]).abs() <= bound).all()), f"{what}: column 10"


def cells_of(env, ncells, cell_of):
    """The float64 cell sums of the device's own records: (cells [ncells, 61], sum |term| likewise)."""
    foot, body = env.gait_foot.cpu().double().tolist(), env.gait_body.cpu().double().tolist()
    status = env.gait_status.cpu().tolist()
    terms = [[[] for _ in range(61)] for _ in range(ncells)]
    for e in range(env.num_envs):
        if status[e] == 0 or not body[e][0] > 0:
            continue
        row = [1.0] + body[e] + [v for f in range(4) for v in foot[e][f][4:]]
        for k, v in enumerate(row):
            terms[cell_of(e)][k].append(v)
    cells = torch.tensor([[math.fsum(t) for t in cell] for cell in terms], dtype=torch.float64)
    mag = torch.tensor([[math.fsum(abs(v) for v in t) for t in cell] for cell in terms], dtype=torch.float64)
    return cells, mag


def check_cells(got, env, cell_of, what):
    got = got.reshape(-1, 61)
    want, mag = cells_of(env, got.shape[0], cell_of)
    assert bool(((got - want).abs() <= 1e-12 * mag).all()), f"{what}: cells"
    assert torch.equal(got[:, :10], want[:, :10])  # (counts: exact)
    return want


def scripted_env(n, device, grid=True, seed=500):
    env, _, _ = E.make_env("go2", n, device)
    assert env.num_bodies == NB
    if grid:
        E.bind_grid(env, torch.Generator().manual_seed(seed + n))
    return env


def run_script(env, steps, every_call=None):
    ref = Restatement(env.num_envs, env.feet_indices.tolist(), env.dt)
    env.gait_begin()
    for t, s in enumerate(steps):
        write_inputs(env, s)
        env.gait_record()
        ref.record(s)
        if every_call is not None:
            every_call(t, ref)
    return ref


def scripted(n, device, every_call=False):
    """The script on a fresh env of the device with the terrain-grid cells: (env, restatement)."""
    env = scripted_env(n, device)
    env.gait_buffers()
    steps = script(n, torch.Generator().manual_seed(700 + n), env.feet_indices.tolist())
    check = (lambda t, ref: check_records(env, ref, f"{device} n={n} call {t}")) if every_call else None
    return env, run_script(env, steps, check)


# ------------------------------------------------------------------ test bodies
def records_and_cells(n, device):
    """Case 1."""
    env, ref = scripted(n, device, every_call=True)
    assert ref.near_ties == 0, "the script must leave no sample near the stumble threshold"
    foot, body, status = ref.foot, ref.body, ref.status
    if n >= 63:
        assert status[:6] == [2, 1, 2, 2, 3, 0] and set(status) == {0, 1, 2, 3}
        assert body[0][0] == 0 and body[1][0] == CALLS - 1 and body[2][0] == 5 and body[3][0] == 2 and body[4][0] == 4
        f = foot[1]
        assert f[0][4] == 11 and f[0][1] == 0 and f[0][5] == 0 and f[1][4] == 0 and f[1][14] > 0
        assert f[2][5] == 5 and (f[2][8], f[2][9]) == (5, 5) and (f[2][6], f[2][7]) == (4, 4)  # phases of length 1
        assert f[3][5] == 2 and (f[3][8], f[3][9]) == (2, 4) and (f[3][6], f[3][7]) == (1, 3)
        f = foot[2][0]  # the swing the fall interrupts is not counted; the first one began unobserved
        assert f[5] == 1 and f[8] == 0 and (f[6], f[7]) == (1, 2) and f[0] == 0 and f[1] == 2
    else:
        assert status == [1] and body[0][0] == CALLS - 1
    rows, cols = E.ROWS, E.COLS
    lv, ty = env.terrain_levels.cpu().tolist(), env.terrain_types.cpu().tolist()
    cells = env.gait_cells()
    assert cells.shape == (rows, cols, 61) and cells.dtype == torch.float64
    want = check_cells(cells, env, lambda e: lv[e] * cols + ty[e], f"{device} n={n} grid")
    counted = sum(1 for e in range(n) if status[e] != 0 and body[e][0] > 0)
    assert int(want[:, 0].sum()) == counted and (n < 63 or counted < n - 1)  # envs 0 and 5 are in no cell
    # a free cell key
    ids = torch.randint(0, 6, (n,), generator=torch.Generator().manual_seed(3), dtype=torch.int32).to(env.device)
    grid_set = env._gait
    env.gait_buffers(2, 3, ids)
    assert env._gait is not grid_set
    run_script(env, script(n, torch.Generator().manual_seed(700 + n), env.feet_indices.tolist()))
    idl = ids.cpu().tolist()
    cells = env.gait_cells()
    assert cells.shape == (2, 3, 61)
    check_cells(cells, env, lambda e: idl[e], f"{device} n={n} cell_ids")
    # one id outside the grid: counted, cells untouched
    ids[7 % n] = 6
    env._gait_cells.fill_(7.0)
    with pytest.raises(_native.LgxError, match="outside"):
        env.gait_cells()
    assert int(env._gait_overflow.item()) == 1 and bool((env._gait_cells == 7.0).all())
    ids[7 % n] = 0
    env.gait_cells()
    assert int(env._gait_overflow.item()) == 0
    # the first set kept its tensors
    assert env.gait_buffers() is grid_set and env._gait_cells.shape == (rows, cols, 61)


def frozen_means_frozen(n, device):
    """Case 2: once every env has finished, nothing is written again."""
    env = scripted_env(n, device)
    env.gait_buffers()
    gen = torch.Generator().manual_seed(800 + n)
    feet = env.feet_indices.tolist()
    last = script(n, gen, feet, calls=1, scripted=False)[0]
    last["reset"] = torch.ones(n, dtype=torch.bool)  # everyone still recording ends here
    run_script(env, script(n, gen, feet) + [last])
    assert int((env.gait_status == 0).sum()) == 0
    cells = env.gait_cells()
    before = [t.clone() for t in (env.gait_foot, env.gait_body, env.gait_status)]
    for s in script(n, gen, feet, calls=3, scripted=False):
        write_inputs(env, s)
        env.gait_record()
    for a, b in zip(before, (env.gait_foot, env.gait_body, env.gait_status)):
        assert torch.equal(a, b)
    assert torch.equal(env.gait_cells(), cells)


def reduce_is_deterministic(n, device):
    """Case 3."""
    env, ref = scripted(n, device)
    a = env.gait_cells()
    env._gait_cells.fill_(-1.0)
    b = env.gait_cells()
    assert torch.equal(a, b)
    out = [e for e in range(n) if ref.status[e] == 0 or ref.body[e][0] == 0]
    assert n < 63 or {0, 5} <= set(out)
    # the cells do not change when the records of the excluded envs do
    for e in out:
        env.gait_foot[e] = 1e6
        env.gait_body[e, 1:] = 1e6
    assert torch.equal(env.gait_cells(), a)
    # ... and do when they become countable
    if out:
        env.gait_status[out[0]] = 1
        env.gait_body[out[0], 0] = 1.0
        assert not torch.equal(env.gait_cells(), a)


def kernels_match_host(n):
    """Case 4 (GPU file): the kernels against the host backend on the same script."""
    env, ref = scripted(n, "cuda:0")
    host, _ = scripted(n, "cpu")
    assert torch.equal(env.gait_status.cpu(), host.gait_status)
    assert torch.equal(env.gait_body.cpu(), host.gait_body)
    foot, hfoot = env.gait_foot.cpu(), host.gait_foot
    assert torch.equal(foot[..., EXACT], hfoot[..., EXACT])
    check_records(env, ref, f"hip n={n}")
    check_records(host, ref, f"host n={n}")  # both within the bound: within twice the bound of each other
    terms = torch.tensor([[[t[k] for k in SUMS] for t in fe] for fe in ref.terms], dtype=torch.float64)
    d = (foot.double() - hfoot.double()).abs()
    assert bool((d[..., SUMS] <= 2 * (terms + 3) * U * hfoot[..., SUMS].double()).all())
    assert bool((d[..., 13] <= 2e-6 * hfoot[..., 13].double()).all())
    assert bool((d[..., 10] <= 2 * (hfoot[..., 8].double() + 1) * U * torch.tensor(ref.abs10, dtype=torch.float64)).all())
    a, b = env.gait_cells(), host.gait_cells()
    assert torch.equal(a[..., :10], b[..., :10])


def evaluator(task, n, device, **over):
    from legged_gym_custom_amd.utils.evaluator import PolicyEvaluator
    over.setdefault("env.episode_length_s", 0.59)  # ceil(0.59 / 0.02) = 30 steps
    if task == "go2_parkour":
        over.update({"terrain.curriculum": False, "commands.curriculum": False})
    env, tcfg, args = E.make_env(task, n, device, **over)
    assert int(env.max_episode_length) == 30
    return PolicyEvaluator(env, E.make_runner(env, tcfg, args))


def end_to_end(task, n, device):
    """Case 5: real physics. The eager loop with the source tensors copied after each step into the
    restatement, the same as a run, a run without the record; on the GPU a second evaluator replays
    its graph."""
    a = evaluator(task, n, device)
    env = a.env
    steps = int(env.max_episode_length) + 1
    ref = Restatement(n, env.feet_indices.tolist(), env.dt)
    a._set_trace(None, True)
    env.gait_buffers()
    a.begin()
    for _ in range(steps):
        a.step()
        ref.record(read_inputs(env))
    check_records(env, ref, f"{device} {task} n={n} end to end")
    foot, body, status = (t.clone() for t in (env.gait_foot, env.gait_body, env.gait_status))
    ra = a.run(graph=False, gait=True)
    assert ra["graph"] is False and ra["num_steps"] == steps and ra["total"]["running"] == 0
    cells, gcells = a.last_cells.clone(), a.last_gait_cells.clone()
    for x, y in zip((env.gait_foot, env.gait_body, env.gait_status), (foot, body, status)):
        assert torch.equal(x, y)
    assert torch.equal(status, env.eval_status) and int((status == 0).sum()) == 0
    assert torch.equal(body[:, 0], env.eval_acc[:, 0])
    rec = a.gait_records()
    assert rec["foot"].shape == (n, 4, 16) and rec["body"].shape == (n, 12) and rec["status"].shape == (n,)
    # invariants
    f, b = foot.cpu().double(), body.cpu().double()
    assert torch.equal(b[:, 1:6].sum(1), b[:, 0])  # the histogram sums to the samples
    assert bool((f[..., 4] <= b[:, :1]).all())  # stance samples (the rest are swing samples) <= samples
    assert torch.equal(f[..., 4].sum(1), (b[:, 1:6] * torch.arange(5.0, dtype=torch.float64)).sum(1))
    assert bool((f[..., 8] <= f[..., 5]).all()) and bool((b[:, 6:] <= b[:, :1]).all())
    swings = int(f[..., 8].sum())
    print(f"{task} n={n}: {swings} completed swings, {int(f[..., 5].sum())} touchdowns, statuses "
          f"{torch.bincount(status.cpu().long(), minlength=4).tolist()}, near ties {ref.near_ties}")
    assert swings >= 1, "the run must see a completed swing"
    g = ra["total"]["gait"]
    assert g["envs"] == int((b[:, 0] > 0).sum()) and g["samples"] == int(b[:, 0].sum())
    assert len(ra["cells"]) == gcells.shape[0] and all("gait" in c for row in ra["cells"] for c in row)
    # the record perturbs nothing
    rp = a.run(graph=False)
    assert torch.equal(a.last_cells, cells) and a.last_gait_cells is None
    assert "gait" not in rp["total"] and all("gait" not in c for row in rp["cells"] for c in row)
    strip = lambda t: {k: v for k, v in t.items() if k != "gait"}  # noqa: E731
    assert strip(ra["total"]) == rp["total"]
    if device == "cpu":
        return
    b2 = evaluator(task, n, device)
    rb = b2.run(gait=True)
    assert rb["graph"] is True
    assert torch.equal(b2.last_cells, cells) and torch.equal(b2.last_gait_cells, gcells)
    for x, y in zip((b2.env.gait_foot, b2.env.gait_body, b2.env.gait_status), (foot, body, status)):
        assert torch.equal(x, y)  # graph replay = the eager loop, bit for bit
    with_gait = b2._graph
    b2.run()
    assert b2._graph is not with_gait and torch.equal(b2.last_cells, cells)  # keyed by (depth, gait): recaptured


def composition(device):
    """Case 6."""
    import json
    ev = evaluator("go2", 64, device, **{"domain_rand.scheduled_pushes": True, "commands.scheduled_commands": True})
    plain = ev.run()
    assert "gait" not in plain["total"]
    rc = ev.run_command_test([0.0, 1.0], vy=(0.0,), yaw=(0.0, 0.5), at_s=0.1, steady_after_s=0.1, gait=True)
    assert rc["total"]["gait"]["envs"] == 64
    got = [rc["bins"][ix][0][iw]["gait"] for ix in range(2) for iw in range(2)]
    assert [g["envs"] for g in got] == [16] * 4 and all(g["samples"] > 0 for g in got)
    rp = ev.run_push_test([0.0, 1.0], directions=2, at_s=0.1, gait=True)
    got = [rp["bins"][s][d]["gait"] for s in range(2) for d in range(2)]
    assert [g["envs"] for g in got] == [16] * 4 and rp["total"]["gait"]["envs"] == 64
    rt = ev.run(gait=True, trace_depth=4)
    assert rt["total"]["gait"]["envs"] == 64 and ev.traces([0])["trace"].shape == (1, 4, 76)
    json.dumps([rc, rp, rt])
    again = ev.run()
    assert "gait" not in again["total"] and all("gait" not in c for row in again["cells"] for c in row)
    assert again["total"] == plain["total"]
    with pytest.raises(RuntimeError, match="gait"):
        ev.gait_records()


def _row(pattern, steps=100, envs=2, dt=0.02):
    """A gait cell row [61] made by hand: `envs` envs that each repeat pattern (a list of 4-tuples of
    contact bits, one per sample) for `steps` samples. Completed phases are counted as the rule would
    for a long episode (every transition closes a phase, the first of each kind excepted)."""
    row = [0.0] * 61
    row[0] = envs
    for _ in range(envs):
        prev, run = None, [0] * 4
        for t in range(steps):
            c = pattern[t % len(pattern)]
            row[1] += 1
            row[2 + sum(c)] += 1
            for i, (a, b) in enumerate(PAIRS):
                row[7 + i] += c[a] == c[b]
            for f in range(4):
                base = 13 + 12 * f
                if prev is not None and c[f] != prev[f]:
                    if c[f]:
                        row[base + 1] += 1
                        row[base + 9] += 60.0
                    if run[f] > 0:
                        k = 4 if c[f] else 2  # a swing ends at a touchdown, a stance at a lift-off
                        row[base + k] += 1
                        row[base + k + 1] += run[f]
                        if c[f]:
                            row[base + 6] += 0.05
                    run[f] = 1
                elif run[f] > 0:
                    run[f] += 1
                if c[f]:
                    row[base + 0] += 1
                    row[base + 7] += 0.001
                    row[base + 8] += 30.0
                else:
                    row[base + 10] += 0.02
            prev = c
    return row


def report():
    """Case 7: gait_cell_report on hand-made rows."""
    import json
    from legged_gym_custom_amd.utils.evaluator import gait_cell_report, gait_label
    go2 = ["FL_foot", "FR_foot", "RL_foot", "RR_foot"]
    anymal = ["LF_FOOT", "LH_FOOT", "RF_FOOT", "RH_FOOT"]
    half = lambda a, b: [a] * 5 + [b] * 5  # noqa: E731
    cases = {"trot": half((1, 0, 0, 1), (0, 1, 1, 0)), "pace": half((1, 0, 1, 0), (0, 1, 0, 1)),
             "bound": half((1, 1, 0, 0), (0, 0, 1, 1)), "pronk": half((1, 1, 1, 1), (0, 0, 0, 0)),
             "stand": [(1, 1, 1, 1)] * 49 + [(1, 1, 1, 0)]}
    for label, pattern in cases.items():
        r = gait_cell_report(_row(pattern), 0.02, go2)
        json.dumps(r, allow_nan=False)
        assert r["gait"] == label, (label, r)
        assert r["envs"] == 2 and r["samples"] == 200 and len(r["pair_sync"]) == 6
        assert all(0.0 <= v <= 1.0 for v in r["pair_sync"]) and set(r["feet"]) == set(go2)
        if label not in ("stand",):
            fl = r["feet"]["FL_foot"]
            # a 10-sample cycle at 50 Hz: 9 touchdowns in an env's 100 samples (2 s)
            assert fl["duty_factor"] == 0.5 and abs(fl["stride_hz"] - 4.5) < 1e-12
            assert abs(fl["mean_stance_s"] - 0.1) < 1e-12 and abs(fl["mean_swing_s"] - 0.1) < 1e-12
            assert abs(fl["mean_clearance_m"] - 0.05) < 1e-12 and abs(fl["load_share"] - 0.25) < 1e-12
            assert abs(fl["slip_m_per_stance_s"] - 0.05) < 1e-12 and fl["stumble_share"] == 0.0
            assert abs(fl["mean_step_length_m"] - 0.1) < 0.02 and fl["mean_touchdown_force"] > 0
            assert r["mean_feet_in_contact"] == 2.0 and r["flight_share"] == (0.5 if label == "pronk" else 0.0)
    # the same trot in anymal's foot order (LF, LH, RF, RH): feet 0 and 3 are a diagonal there too
    assert gait_cell_report(_row(cases["trot"]), 0.02, anymal)["gait"] == "trot"
    # feet 0 and 1 together: a bound for go2's order (FL, FR), a pace for anymal's (LF, LH)
    assert gait_cell_report(_row(cases["bound"]), 0.02, anymal)["gait"] == "pace"
    assert gait_cell_report(_row(cases["trot"]), 0.02, ["a", "b", "c", "d"])["gait"] is None
    assert gait_label(0.5, [0.5] * 6, go2) == "mixed" and gait_label(None, [0.5] * 6, go2) is None
    empty = gait_cell_report([0.0] * 61, 0.02, go2)
    json.dumps(empty, allow_nan=False)
    assert empty["envs"] == 0 and empty["samples"] == 0 and empty["gait"] is None
    assert all(v is None for k, v in empty.items() if k not in ("envs", "samples", "feet", "pair_sync"))
    assert empty["pair_sync"] == [None] * 6
    assert all(v is None for foot in empty["feet"].values() for v in foot.values())


def refusals(device):
    """Case 8: each failure raises with a message naming its cause and writes nothing."""
    env, _ = scripted(63, device)
    tensors = lambda: (env.gait_foot, env.gait_body, env.gait_status)  # noqa: E731
    before = [t.clone() for t in tensors()]
    same = lambda: all(torch.equal(a, b) for a, b in zip(before, tensors()))  # noqa: E731
    env.reset_buf.zero_()  # a record that went ahead would add a sample to every recording env
    nat, st = env._native, env._stream()
    good = dict(foot=env.gait_foot, body=env.gait_body, status=env.gait_status, cells=env._gait_cells,
                overflow=env._gait_overflow)

    def raw(rows=E.ROWS, cols=E.COLS, **over):
        gb = _abi.GaitBuffers()
        for k, t in {**good, **over}.items():
            setattr(gb, k, None if t is None else t.data_ptr())
        gb.cell_rows, gb.cell_cols = rows, cols
        return gb

    calls = {"begin": lambda gb: nat.gait_begin(gb, st), "record": lambda gb: nat.gait_record(gb, st),
             "reduce": lambda gb: nat.gait_reduce(gb, st)}
    for member in ("foot", "body", "status", "overflow"):
        for name, call in calls.items():
            with pytest.raises(_native.LgxError, match=f"lgx_gait_{name}: {member} is NULL"):
                call(raw(**{member: None}))
    with pytest.raises(_native.LgxError, match="lgx_gait_reduce: cells is NULL"):
        calls["reduce"](raw(cells=None))
    for rows, cols in ((0, 2), (3, 0), (-1, 2)):
        for name, call in calls.items():
            with pytest.raises(_native.LgxError, match=f"lgx_gait_{name}: cell_rows and cell_cols"):
                call(raw(rows, cols))
    shifted = torch.zeros(63 * 64 + 1, device=env.device)[1:].view(63, 4, 16)  # 4 bytes off a 16-byte boundary
    with pytest.raises(_native.LgxError, match="lgx_gait_record: foot must be 16-byte aligned"):
        calls["record"](raw(foot=shifted))
    L = _native.lib()
    assert L.lgx_gait_record(nat.handle, None, None) < 0 and b"NULL" in L.lgx_last_error(nat.handle)
    for member in ("foot", "body", "status", "cells", "overflow"):
        with pytest.raises(_native.LgxError, match=f"gait buffer {member} is required"):
            nat.gait_buffers(**{**good, member: None})
    with pytest.raises(_native.LgxError, match="gait buffer foot must be"):
        nat.gait_buffers(**{**good, "foot": env.gait_foot[:, :3].contiguous()})
    assert same()
    # unbound source buffers
    for attr, name in (("_contact3", "contact_forces"), ("rigid_body_states", "rigid_body_states"),
                       ("time_out_buf", "time_out")):
        keep = getattr(env, attr)
        setattr(env, attr, None)
        try:
            env._bind()
        except _native.LgxError as err:  # lgx_bind itself requires this one
            assert name in str(err)
        else:
            with pytest.raises(_native.LgxError, match=f"lgx_gait_record.*{name}"):
                env.gait_record()
        setattr(env, attr, keep)
        env._bind()
    assert same()
    # a foot index outside the bodies
    # (a second native env on the same tensors, never stepped, whose params name body NB as foot 1)
    import ctypes
    params = type(nat.params)()
    ctypes.memmove(ctypes.byref(params), ctypes.byref(nat.params), ctypes.sizeof(params))
    params.feet_idx[1] = NB
    bad = _native.NativeEnv(nat.model, params, nat.device_index)
    bad.bind(nat._keep)
    gb = bad.gait_buffers(**good)
    for call in (bad.gait_begin, bad.gait_record, bad.gait_reduce):
        with pytest.raises(_native.LgxError, match="feet_idx outside the bodies"):
            call(gb, st)
    assert same()
    # no record yet
    other, _, _ = E.make_env("go2", 8, device)
    for call in (other.gait_begin, other.gait_record, other.gait_cells):
        with pytest.raises(RuntimeError, match="gait_buffers"):
            call()
    env.gait_record()  # and the first env's record is still usable
    assert not same()
