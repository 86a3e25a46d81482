"""Shared by tests/test_trace_host.py and tests/test_gpu_trace.py: the flight recorder
(include/lgx.h ABI 11: lgx_trace_begin / lgx_trace_record / lgx_trace_gather) on one device. A
scripted sequence of inputs written straight into the env's tensors (no physics step, the style of
eval_case.write_inputs), a restatement that keeps plain Python lists of float64 rows, and the test
bodies, parameterised by the device.

Bounds (from the number formats, not from the code under test): columns 0-68 and 73 are copies of
fp32 values (column 0 an integer below 2^24 as a float), so they match bit for bit. Columns 69-72 and
74 are fp32 norms of 3 components (error about 2.5 * 2^-24): rtol 1e-6, the bound eval_case.py
derives. Column 75 is the index of the largest non-foot norm: exact wherever the float64 reference's
two largest non-foot norms differ by more than 1e-5 relative (100x the fp32 norm error, so fp32
cannot order them differently); a row whose peak is 0 has index -1 exactly. The script's seeds are
such that the reference excludes no row, and the test asserts it."""
import torch

import eval_case as E
from legged_gym_custom_amd import _abi, _native

CALLS, DEPTH, COLS = 11, 4, 76
COPIED = list(range(0, 69)) + [73]
NORMS = [69, 70, 71, 72, 74]
SOURCES = ("root_states", "base_lin_vel", "base_ang_vel", "projected_gravity", "commands", "dof_state", "torques",
           "actions", "contact_forces", "rew", "episode_length", "reset", "time_out", "blew_up")


def script(n, gen, calls=CALLS):
    """`calls` steps of inputs (CPU tensors). Flags, for n >= 63: env 0 resets at the first call
    (count 0, timed out); env 1 falls at call DEPTH (count == DEPTH); env 2 times out at call
    DEPTH + 1 (count == DEPTH + 1); env 3 falls at call 2 and resets again (as a time-out) at call 6,
    which must change nothing; env 4 blows up at call 3 with its time_out flag set too (blow-up
    wins); envs with e % 5 == 0 from 5 on never reset, so their rings wrap twice; the rest reset
    once at a random call, half of them as time-outs. A single env never resets."""
    steps = []
    when = torch.randint(0, calls, (n,), generator=gen)
    as_timeout = torch.rand(n, generator=gen) < 0.5
    never = (torch.arange(n) % 5 == 0) | (n < 63)
    for t in range(calls):
        r = lambda *s, k=1.0: k * torch.randn(*s, generator=gen)  # noqa: E731
        reset = (when == t) & ~never
        tout = reset & as_timeout
        blew = torch.zeros(n, dtype=torch.bool)
        if n >= 63:
            reset[:5] = torch.tensor([t == 0, t == DEPTH, t == DEPTH + 1, t in (2, 6), t == 3])
            tout[:5] = torch.tensor([t == 0, False, t == DEPTH + 1, t == 6, t == 3])
            blew[4] = t == 3
        steps.append(dict(root_states=r(n, 13), base_lin_vel=r(n, 3), base_ang_vel=r(n, 3), projected_gravity=r(n, 3),
                          commands=r(n, 4), dof_state=r(n, 12, 2, k=5.0), torques=r(n, 12, k=20.0), actions=r(n, 12),
                          contact_forces=r(n, 19, 3, k=80.0), rew=r(n),
                          episode_length=torch.randint(0, 1000, (n,), generator=gen), reset=reset, time_out=tout,
                          blew_up=blew))
    return steps


def _tensors(env):
    """The env tensors the recorder reads, by lgx_buffers name."""
    return dict(root_states=env.root_states, base_lin_vel=env.base_lin_vel, base_ang_vel=env.base_ang_vel,
                projected_gravity=env.projected_gravity, commands=env.commands, dof_state=env._dof_state3,
                torques=env.torques, actions=env.actions, contact_forces=env._contact3, rew=env.rew_buf,
                episode_length=env.episode_length_buf, reset=env.reset_buf, time_out=env.time_out_buf,
                blew_up=env.blew_up_buf)


def write_inputs(env, s):
    """One scripted step into the tensors the native env is bound to."""
    dst = _tensors(env)
    assert dst["contact_forces"].shape[1:] == s["contact_forces"].shape[1:] and env.torques.shape[1] == 12
    for k in SOURCES:
        dst[k].copy_(s[k])


def read_inputs(env):
    """The same tensors after a real step, as CPU copies."""
    return {k: t.detach().cpu().clone() for k, t in _tensors(env).items()}


class Restatement:
    """lgx_trace_record restated: plain Python lists of float64 rows per env."""

    def __init__(self, n, feet, num_bodies):
        self.n, self.feet = n, [int(f) for f in feet]
        self.others = [b for b in range(num_bodies) if b not in self.feet]
        self.rows = [[] for _ in range(n)]
        self.close = [[] for _ in range(n)]  # per row: the two largest non-foot norms are within 1e-5 relative
        self.status = [0] * n

    def row_matrix(self, s):
        d = lambda k: s[k].detach().cpu().double()  # noqa: E731
        n = self.n
        ds, cf = d("dof_state").reshape(n, -1, 2), d("contact_forces").reshape(n, -1, 3)
        norms = cf.norm(dim=-1)
        rest = norms[:, self.others]
        top = rest.sort(dim=1, descending=True).values
        peak, arg = rest.max(dim=1)  # (the first of equal maxima: the lowest body index)
        idx = torch.where(peak > 0, torch.tensor(self.others)[arg].double(), torch.tensor(-1.0, dtype=torch.float64))
        close = (peak > 0) & ((top[:, 0] - top[:, 1]) <= 1e-5 * top[:, 0])
        R = torch.cat([d("episode_length").reshape(n, 1), d("root_states")[:, :7], d("base_lin_vel"), d("base_ang_vel"),
                       d("projected_gravity"), d("commands")[:, :4], ds[..., 0], ds[..., 1], d("torques"), d("actions"),
                       norms[:, self.feet], d("rew").reshape(n, 1), peak.reshape(n, 1), idx.reshape(n, 1)], 1)
        assert R.shape == (n, COLS)
        return R, close

    def record(self, s):
        R, close = self.row_matrix(s)
        reset, tout, blew = (s[k].detach().cpu().bool().tolist() for k in ("reset", "time_out", "blew_up"))
        for e in range(self.n):
            if self.status[e] != 0:
                continue
            if reset[e]:
                self.status[e] = 3 if blew[e] else (1 if tout[e] else 2)
            else:
                self.rows[e].append(R[e])
                self.close[e].append(bool(close[e]))

    @property
    def count(self):
        return [len(r) for r in self.rows]

    def ring(self, depth):
        """(the ring [n, depth, 76] float64 the rows leave, the mask [n, depth] of its close rows)"""
        ring = torch.zeros(self.n, depth, COLS, dtype=torch.float64)
        close = torch.zeros(self.n, depth, dtype=torch.bool)
        for e, rows in enumerate(self.rows):
            for i in range(max(0, len(rows) - depth), len(rows)):
                ring[e, i % depth], close[e, i % depth] = rows[i], self.close[e][i]
        return ring, close

    def unrolled(self, e, depth):
        rows = self.rows[e][-depth:]
        out = torch.zeros(depth, COLS, dtype=torch.float64)
        for j, row in enumerate(rows):
            out[depth - len(rows) + j] = row
        return out, len(rows)


def check_rows(got, want, close, what, norms=True):
    """Rows of the code under test (fp32, any leading shape) against the restatement's at the bounds
    of the module docstring; close: the rows whose column 75 is not compared."""
    got = got.detach().cpu().double()
    assert got.shape == want.shape, what
    assert torch.equal(got[..., COPIED], want[..., COPIED]), f"{what}: copied columns"
    if not norms:
        return
    err = (got[..., NORMS] - want[..., NORMS]).abs()
    print(f"{what}: norm columns max rel err {float((err / want[..., NORMS].clamp_min(1e-300)).max()):.3e}")
    assert bool((err <= 1e-6 * want[..., NORMS]).all()), f"{what}: norm columns"
    assert torch.equal(got[..., 75][~close], want[..., 75][~close]), f"{what}: peak body index"


def scripted_env(n, device, depth=DEPTH):
    env, _, _ = E.make_env("go2", n, device)
    env.trace_buffers(depth)
    return env


def run_script(env, steps):
    ref = Restatement(env.num_envs, env.feet_indices.tolist(), env.num_bodies)
    env.trace_begin()
    for s in steps:
        write_inputs(env, s)
        env.trace_record()
        ref.record(s)
    return ref


def scripted(n, device):
    """The script on a fresh env of the device: (env, restatement)."""
    env = scripted_env(n, device)
    return env, run_script(env, script(n, torch.Generator().manual_seed(300 + n)))


# ------------------------------------------------------------------ test bodies
def ring_matches_restatement(n, device):
    """Test 1, and test 2 on its records."""
    env, ref = scripted(n, device)
    count, status = env.trace_count.cpu().tolist(), env.trace_status.cpu().tolist()
    assert count == ref.count and status == ref.status
    if n >= 63:
        assert count[:5] == [0, DEPTH, DEPTH + 1, 2, 3] and status[:5] == [1, 2, 1, 2, 3]
        assert count[5] == CALLS and status[5] == 0 and CALLS > 2 * DEPTH  # never reset: wrapped twice
        assert set(status) == {0, 1, 2, 3}
    else:
        assert count == [CALLS] and status == [0]
    want, close = ref.ring(DEPTH)
    assert int(close.sum()) == 0, "the script must leave no row out of the column-75 comparison"
    check_rows(env.trace_ring, want, close, f"{device} n={n} ring")
    gather_matches(env, ref)
    return env, ref


def gather_matches(env, ref):
    n, ring, count = env.num_envs, env.trace_ring.cpu(), ref.count
    gen = torch.Generator().manual_seed(7)
    for m in sorted({1, 7, n}):
        ids = torch.randint(0, n, (m,), generator=gen)
        if m == n:
            ids = torch.randperm(n, generator=gen)
        if m >= 7:
            ids[3] = ids[1]  # a duplicate
        out, out_len = env.trace_gather(ids if m != 7 else ids.tolist())  # a tensor or a list
        assert out.shape == (m, DEPTH, COLS) and out.dtype == torch.float32 and out_len.dtype == torch.int32
        out, out_len = out.cpu(), out_len.cpu().tolist()
        for i, e in enumerate(ids.tolist()):
            want, L = ref.unrolled(e, DEPTH)
            assert out_len[i] == L == min(count[e], DEPTH)
            assert int(out[i, :DEPTH - L].abs().sum()) == 0  # the rows in front are zero
            for j in range(L):  # bit-equal to the ring's rows, oldest first
                assert torch.equal(out[i, DEPTH - L + j], ring[e, (count[e] - L + j) % DEPTH])
            check_rows(out[i], want, torch.zeros(DEPTH, dtype=torch.bool), f"gather env {e}", norms=False)
    # the raw call never indexes with an id outside [0, N): zero rows, out_len -1
    dev = env.device
    ids = torch.tensor([0, -1, n, n - 1, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device=dev)
    out = torch.full((ids.shape[0], DEPTH, COLS), 7.0, device=dev)
    out_len = torch.full((ids.shape[0],), 7, dtype=torch.int32, device=dev)
    env._native.trace_gather(env._trace, ids, out, out_len, env._stream())
    assert out_len.cpu().tolist() == [min(count[0], DEPTH), -1, -1, min(count[n - 1], DEPTH), -1, -1]
    assert int(out[[1, 2, 4, 5]].abs().sum()) == 0
    assert torch.equal(out[3].cpu(), env.trace_gather([n - 1])[0][0].cpu())
    # the env's own call refuses them, naming the id
    import pytest
    for bad in (-1, n):
        with pytest.raises(ValueError, match=rf"env id {bad} "):
            env.trace_gather([0, bad])
    out, out_len = env.trace_gather([])
    assert out.shape == (0, DEPTH, COLS) and out_len.shape == (0,)


def frozen_means_frozen(n, device):
    """Test 3: once every env has finished, nothing is written again."""
    env = scripted_env(n, device)
    gen = torch.Generator().manual_seed(400 + n)
    steps = script(n, gen)
    last = script(n, gen, calls=1)[0]
    last["reset"] = torch.ones(n, dtype=torch.bool)  # everyone still recording ends here
    run_script(env, steps + [last])
    assert int((env.trace_status == 0).sum()) == 0
    before = [t.clone() for t in (env.trace_ring, env.trace_count, env.trace_status)]
    for s in script(n, gen, calls=2):
        s["reset"] = torch.rand(n, generator=gen) < 0.5
        write_inputs(env, s)
        env.trace_record()
    for a, b in zip(before, (env.trace_ring, env.trace_count, env.trace_status)):
        assert torch.equal(a, b)


def peak_ties(device):
    """Columns 74 / 75 where the answer is exact: no force at all, two equal largest forces (the
    lowest index wins), a foot that carries the largest force (ignored), the last body."""
    n = 8
    env = scripted_env(n, device)
    feet = env.feet_indices.tolist()
    others = [b for b in range(env.num_bodies) if b not in feet]
    s = script(n, torch.Generator().manual_seed(9), calls=1)[0]
    s["reset"] = torch.zeros(n, dtype=torch.bool)
    cf = torch.zeros(n, env.num_bodies, 3)
    cf[1, others[2]] = cf[1, others[5]] = cf[1, others[9]] = torch.tensor([3.0, 4.0, 12.0])  # norm 13, three times
    cf[1, others[0]] = torch.tensor([1.0, 2.0, 2.0])
    cf[2, feet[1]] = torch.tensor([0.0, 0.0, 500.0])
    cf[2, others[4]] = torch.tensor([0.0, 3.0, 4.0])
    cf[3, others[-1]] = torch.tensor([0.0, 0.0, 2.0])
    cf[4, feet[0]] = torch.tensor([6.0, 0.0, 8.0])  # only a foot: no other body is hit
    s["contact_forces"] = cf
    env.trace_begin()
    write_inputs(env, s)
    env.trace_record()
    row = env.trace_ring[:, 0].cpu()
    assert row[:, 74].tolist() == [0.0, 13.0, 5.0, 2.0, 0.0, 0.0, 0.0, 0.0]
    assert row[:, 75].tolist() == [-1.0, others[2], others[4], others[-1], -1.0, -1.0, -1.0, -1.0]
    assert float(row[2, 69 + 1]) == 500.0 and float(row[4, 69]) == 10.0


def refusals(device):
    """Test 7: each failure raises with a message naming its cause and writes nothing."""
    import pytest
    env, _ = scripted(63, device)
    snap = lambda: [t.clone() for t in (env.trace_ring, env.trace_count, env.trace_status)]  # noqa: E731
    before = snap()
    same = lambda: all(torch.equal(a, b) for a, b in zip(before, snap()))  # noqa: E731
    env.reset_buf.zero_()  # a record that went ahead would add a row to every recording env
    nat, st = env._native, env._stream()
    ids = torch.zeros(1, dtype=torch.int32, device=env.device)
    out_len = torch.zeros(1, dtype=torch.int32, device=env.device)

    def raw(ring, count, status, depth):
        tb = _abi.TraceBuffers()
        tb.ring, tb.count, tb.status = (None if t is None else t.data_ptr() for t in (ring, count, status))
        tb.depth = depth
        return tb

    calls = (lambda tb: nat.trace_begin(tb, st), lambda tb: nat.trace_record(tb, st),
             lambda tb: nat.trace_gather(tb, ids, torch.zeros(1, tb.depth, COLS, device=env.device), out_len, st))
    # depth = 0, and a NULL member
    with pytest.raises(ValueError, match="depth"):
        env.trace_buffers(0)
    with pytest.raises(_native.LgxError, match="depth"):
        nat.trace_buffers(env.trace_ring[:, :0].contiguous(), env.trace_count, env.trace_status)
    for tb, match in ((raw(env.trace_ring, env.trace_count, env.trace_status, 0), "depth"),
                      (raw(None, env.trace_count, env.trace_status, DEPTH), "ring"),
                      (raw(env.trace_ring, None, env.trace_status, DEPTH), "count"),
                      (raw(env.trace_ring, env.trace_count, None, DEPTH), "status")):
        for call in calls:
            with pytest.raises(_native.LgxError, match=match):
                call(tb)
    L = _native.lib()
    assert L.lgx_trace_record(nat.handle, None, None) < 0 and b"NULL" in L.lgx_last_error(nat.handle)
    assert same()
    # an unbound source buffer: rew is one lgx_bind itself requires; projected_gravity is the recorder's
    keep = env.rew_buf
    env.rew_buf = None
    with pytest.raises(_native.LgxError, match="rew"):
        env._bind()
    env.rew_buf = keep
    keep = env.projected_gravity
    env.projected_gravity = None
    env._bind()
    with pytest.raises(_native.LgxError, match="lgx_trace_record.*projected_gravity"):
        env.trace_record()
    env.projected_gravity = keep
    env._bind()
    assert same()
    # no recorder yet, and traces() before any traced run
    fresh, tcfg, args = E.make_env("go2", 8, device)
    for call in (fresh.trace_begin, fresh.trace_record, lambda: fresh.trace_gather([0])):
        with pytest.raises(RuntimeError, match="trace_buffers"):
            call()
    from legged_gym_custom_amd.utils.evaluator import PolicyEvaluator
    ev = PolicyEvaluator(fresh, E.make_runner(fresh, tcfg, args))
    with pytest.raises(RuntimeError, match="not traced"):
        ev.traces()
    ev.run(2, trace_depth=2)
    assert ev.traces([0])["trace"].shape == (1, 2, COLS)
    ev.run(2)  # an untraced run: the rings no longer belong to the last run
    with pytest.raises(RuntimeError, match="not traced"):
        ev.traces()
    ev.run(2, trace_depth=2)
    with pytest.raises(ValueError, match="which"):
        ev.traces("all")
    env.trace_record()  # and the first env's recorder is still usable
    assert not same()


def evaluator(task, n, device, **over):
    from legged_gym_custom_amd.utils.evaluator import PolicyEvaluator
    over.setdefault("env.episode_length_s", 0.19)  # ceil(0.19 / 0.02) = 10 steps
    if task == "go2_parkour":
        over.update({"terrain.curriculum": False, "commands.curriculum": False})
    env, tcfg, args = E.make_env(task, n, device, **over)
    assert int(env.max_episode_length) == 10
    return PolicyEvaluator(env, E.make_runner(env, tcfg, args))


def end_to_end(task, n, device):
    """Test 5: real physics. The eager traced loop with the env tensors recorded in Python after each
    step, the same as a run, an untraced run; on the GPU a second evaluator replays its graphs."""
    a = evaluator(task, n, device)
    env = a.env
    steps = int(env.max_episode_length) + 1
    # the eager loop, the env's tensors recorded in Python after each step
    ref = Restatement(n, env.feet_indices.tolist(), env.num_bodies)
    a._set_trace(DEPTH)
    a.begin()
    for _ in range(steps):
        a.step()
        ref.record(read_inputs(env))
    ring, count, status = (t.clone() for t in (env.trace_ring, env.trace_count, env.trace_status))
    assert count.cpu().tolist() == ref.count and status.cpu().tolist() == ref.status
    # the same as a run (begin rewinds the env: it repeats exactly)
    ra = a.run(graph=False, trace_depth=DEPTH)
    assert ra["graph"] is False and ra["num_steps"] == steps and ra["total"]["running"] == 0
    assert a.last_trace_depth == DEPTH
    cells = a.last_cells.clone()
    for x, y in zip((env.trace_ring, env.trace_count, env.trace_status), (ring, count, status)):
        assert torch.equal(x, y)
    assert torch.equal(status, env.eval_status) and int((status == 0).sum()) == 0
    assert torch.equal(count.float(), env.eval_acc[:, 0])
    assert int((count > DEPTH).sum()) > 0  # rings that wrapped
    newest = ring[torch.arange(n, device=ring.device), (count.long() - 1) % DEPTH, 0]
    assert torch.equal(newest[count > 0], count[count > 0].float())  # the episode length at an env's newest row
    want, close = ref.ring(DEPTH)
    print(f"{task} n={n}: {int(close.sum())} rows with two near-equal peak bodies; statuses "
          f"{torch.bincount(status.cpu().long(), minlength=4).tolist()}")
    check_rows(ring, want, close, f"{device} {task} n={n} end to end", norms=False)
    tr = a.traces([0, n - 1])
    for i, e in enumerate((0, n - 1)):
        want_e, L = ref.unrolled(e, DEPTH)
        assert int(tr["length"][i]) == L and int(tr["status"][i]) == ref.status[e]
        check_rows(torch.from_numpy(tr["trace"][i]), want_e, torch.zeros(DEPTH, dtype=torch.bool), "traces()", norms=False)
    # the recorder perturbs nothing
    a.run(graph=False)
    assert torch.equal(a.last_cells, cells) and a.last_trace_depth is None
    if device == "cpu":
        return
    b = evaluator(task, n, device)
    rb = b.run(trace_depth=DEPTH)
    assert rb["graph"] is True
    assert torch.equal(b.last_cells, cells)
    for x, y in zip((b.env.trace_ring, b.env.trace_count, b.env.trace_status), (ring, count, status)):
        assert torch.equal(x, y)  # graph replay = the eager loop, bit for bit
    b.run(trace_depth=2)  # another depth in between: rings and a graph of its own
    assert torch.equal(b.last_cells, cells) and b.env.trace_ring.shape[1] == 2
    assert torch.equal(b.env.trace_count, count)
    b.run(trace_depth=DEPTH)
    assert torch.equal(b.env.trace_ring, ring) and torch.equal(b.env.trace_status, status)
    traced = b._graph
    b.run()
    assert b._graph is not traced and torch.equal(b.last_cells, cells)  # keyed by the depth: recaptured


def selection(device):
    """Test 6, the selection: traces("falls") on scripted statuses and counts."""
    ev = evaluator("go2", 8, device)
    env = ev.env
    ev.run(2, graph=False, trace_depth=DEPTH)
    env.trace_status.copy_(torch.tensor([2, 0, 3, 2, 1, 2, 2, 3], dtype=torch.uint8))
    env.trace_count.copy_(torch.tensor([5, 1, 2, 5, 0, 2, 9, 0], dtype=torch.int32))
    order = [7, 2, 5, 0, 3, 6]  # falls and blow-ups by (count, env id)
    for cap in (4, 6, 16, 0):
        tr = ev.traces("falls", max_envs=cap)
        m = min(cap, 6)
        assert tr["env_id"].tolist() == order[:m]
        assert tr["status"].tolist() == [[2, 0, 3, 2, 1, 2, 2, 3][e] for e in order[:m]]
        assert tr["length"].tolist() == [min([5, 1, 2, 5, 0, 2, 9, 0][e], DEPTH) for e in order[:m]]
        assert tr["trace"].shape == (m, DEPTH, COLS) and tr["trace"].dtype.name == "float32"
        assert tr["terrain_level"].tolist() == [-1] * m and tr["terrain_type"].tolist() == [-1] * m
        assert len(tr["columns"]) == COLS == len(set(tr["columns"].tolist())) and float(tr["dt"]) == float(env.dt)
    tr = ev.traces([3, 3, 1])
    assert tr["env_id"].tolist() == [3, 3, 1] and tr["status"].tolist() == [2, 2, 0]
    from legged_gym_custom_amd.utils.evaluator import TRACE_COLUMNS
    assert tr["columns"].tolist() == list(TRACE_COLUMNS)
    assert TRACE_COLUMNS[0] == "episode_length" and TRACE_COLUMNS[21] == "dof_pos_0" and TRACE_COLUMNS[73] == "reward"
    # a depth keeps its tensors (a loop captured at that depth replays on them) while another is in use
    tb, ptr = env._trace, env.trace_ring.data_ptr()
    env.trace_buffers(2)
    assert env.trace_ring.shape == (8, 2, COLS) and env.trace_ring.data_ptr() != ptr
    assert env.trace_buffers(DEPTH) is tb and env.trace_ring.data_ptr() == ptr
