"""The reduce tree of the evaluation (csrc/lgx_env.hip) on the MI355X, pinned bit for bit:
eval_reduce_kernel (12 + 5 push columns), eval_cmd_reduce_kernel (9 columns), gait_reduce_kernel
(61 columns), joint_reduce_kernel (246 columns) and contact_reduce_kernel (320 columns) against a
NumPy float64 restatement of the documented order. One block of 256 threads
per cell; thread t adds its envs t, t + 256, ... in increasing order; inside each wave of 64,
for o = 32, 16, ..., 1: a[:o] += a[o:2 * o]; then ((w0 + w1) + w2) + w3.

No env step is run: the record tensors are written directly, fp32 values randn x 10^uniform(-3, 6)
(nine decades, so the order of the additions shows in the last bits), gates positive for about three
quarters of the envs, statuses from 0..3. 300 envs: threads 0..43 own two envs, the last wave is
partly empty. No tolerance: float64 addition is exact to the bit once its order is fixed, and the
fp32 -> fp64 conversion of the inputs is exact. The test also shows that its inputs tell orders
apart: the plain env-order sum differs from the tree in every one of the sets.

The joint and contact cells also hold maxima and minima, which ride the same scan: they do not
depend on the order, so the reference takes them with plain max / min over the contributing envs (a
cell without one is all zero; the contact set leaves its last cell empty to show it). Those two sets
are compared on the int64 view of the cells."""
import numpy as np
import pytest
import torch

import eval_case as E
from legged_gym_custom_amd import _abi

pytestmark = pytest.mark.gpu
N, ROWS, COLS = 300, 2, 2


def values(gen, *shape):
    return (torch.randn(*shape, generator=gen) * 10.0 ** (torch.rand(*shape, generator=gen) * 9.0 - 3.0)).float()


def gate(gen, x):
    """Column 0 of x made positive for about three quarters of the rows, negative for the rest."""
    x[:, 0] = x[:, 0].abs().clamp_min(1e-3) * torch.where(torch.rand(x.shape[0], generator=gen) < 0.75, 1.0, -1.0)
    return x


def tree_sum(C, ids, cells):
    """The documented tree over the contributions C [N, K] float64 of the envs with cell ids[e]."""
    out = np.zeros((cells, C.shape[1]))
    for c in range(cells):
        X = np.where((ids == c)[:, None], C, 0.0)
        part = np.zeros((256, C.shape[1]))
        for base in range(0, len(X), 256):  # thread t: envs t, t + 256, ... in increasing order
            blk = X[base:base + 256]
            part[:len(blk)] += blk
        a = part.reshape(4, 64, -1)
        for o in (32, 16, 8, 4, 2, 1):  # shuffle-down inside each wave
            a[:, :o] += a[:, o:2 * o]
        out[c] = ((a[0, 0] + a[1, 0]) + a[2, 0]) + a[3, 0]
    return out


def env_order_sum(C, ids, cells):
    out = np.zeros((cells, C.shape[1]))
    for e in range(len(C)):
        out[ids[e]] += C[e]
    return out


def eval_contrib(acc, status):
    """lgx_eval_reduce's 12 cell columns: env count, the three finish counts, the 8 record sums."""
    fin = (status != 0)[:, None]
    return np.concatenate([np.ones((len(acc), 1)), np.stack([status == k for k in (1, 2, 3)], 1) * 1.0,
                           np.where(fin, acc, 0.0)], 1)


def push_contrib(rec, status):
    on, surv = (status != 0) & (rec[:, 0] > 0), status == 1
    C = np.stack([np.ones(len(rec)), rec[:, 1], rec[:, 2], surv * 1.0, np.where(surv, rec[:, 3], 0.0)], 1)
    return np.where(on[:, None], C, 0.0)


def cmd_contrib(rec, status):
    on, surv = (status != 0) & (rec[:, 0] > 0), (status == 1)[:, None]
    C = np.concatenate([np.ones((len(rec), 1)), surv * 1.0, np.where(surv, rec[:, 1:3], 0.0), rec[:, 3:4],
                        np.where(surv, rec[:, 4:], 0.0)], 1)
    return np.where(on[:, None], C, 0.0)


def gait_contrib(foot, body, status):
    on = (status != 0) & (body[:, 0] > 0)
    C = np.concatenate([np.ones((len(body), 1)), body, foot[:, :, 4:].reshape(len(body), -1)], 1)
    return np.where(on[:, None], C, 0.0)


def joint_inputs(gen):
    """joint [N, 12, 16], body [N, 4] (column 0 gated), status, cell ids: lgx_joint_buffers' records."""
    return (values(gen, N, _abi.MAX_DOF, _abi.JOINT_COLS), gate(gen, values(gen, N, _abi.JOINT_BODY_COLS)),
            torch.randint(0, 4, (N,), generator=gen).to(torch.uint8), torch.randint(0, ROWS * COLS, (N,), generator=gen).int())


def joint_want(joint, body, status, ids):
    """lgx_joint_reduce's 246 cell columns in the layout of include/lgx.h: the sums by the tree, the
    extremes by max / min. Returns (cells, the sum columns' contributions)."""
    assert _abi.JOINT_CELL_COLS == 2 + 4 + 12 * 20
    on = (status != 0) & (body[:, 0] > 0)
    C = np.where(on[:, None], np.concatenate([np.ones((N, 1)), body, joint[:, :, 1:].reshape(N, -1)], 1), 0.0)
    cols = [0, 1, 2, 3, 4] + [6 + 20 * j + k for j in range(12) for k in range(15)]
    want = np.zeros((ROWS * COLS, _abi.JOINT_CELL_COLS))
    want[:, cols] = tree_sum(C, ids, ROWS * COLS)
    for c in range(ROWS * COLS):
        m = on & (ids == c)
        if not m.any():
            continue
        want[c, 5] = body[m, 1].max()
        for j in range(12):
            r = joint[m, j]
            want[c, 6 + 20 * j + 15:6 + 20 * j + 20] = (r[:, 3].max(), r[:, 6].max(), r[:, 7].max(), r[:, 10].min(),
                                                        r[:, 11].max())
    return want, C


def contact_inputs(gen):
    """body [N, 24, 12], env [N, 8] (column 0, "sampled", gated; columns 4 and 6 body indices from
    -1..23), status, cell ids (the last cell stays empty): lgx_contact_buffers' records."""
    env = gate(gen, values(gen, N, _abi.CONTACT_ENV_COLS))
    env[:, 4] = torch.randint(-1, 24, (N,), generator=gen).float()
    env[:, 6] = torch.randint(-1, 24, (N,), generator=gen).float()
    return (values(gen, N, _abi.MAX_BODIES, _abi.CONTACT_COLS), env, torch.randint(0, 4, (N,), generator=gen).to(torch.uint8),
            torch.randint(0, ROWS * COLS - 1, (N,), generator=gen).int())


def contact_want(body, env, status, ids):
    """lgx_contact_reduce's 320 cell columns in the layout of include/lgx.h: the sums (7 of the env
    part, 10 per body, the two fall histograms among them) by the tree over the finished envs, the
    extremes by max / min, column 7's over the sampled envs only."""
    assert _abi.CONTACT_CELL_COLS == 8 + 24 * 13
    on, fell, b = status != 0, (status == 2)[:, None], np.arange(24)[None, :]
    per_body = np.stack([body[:, :, k] for k in (1, 2, 3, 5, 6, 8, 9, 11)]
                        + [(fell & (env[:, 4:5] == b)) * 1.0, (fell & (env[:, 6:7] == b)) * 1.0], 2)
    C = np.concatenate([np.ones((N, 1)), env[:, :3], fell * 1.0, (fell & (env[:, 4:5] < 0)) * 1.0,
                        np.where(fell, env[:, 7:8], 0.0), per_body.reshape(N, -1)], 1)
    C = np.where(on[:, None], C, 0.0)
    cols = [0, 1, 2, 3, 5, 6, 7] + [8 + 13 * j + k for j in range(24) for k in (0, 1, 2, 3, 4, 5, 6, 7, 11, 12)]
    want = np.zeros((ROWS * COLS, _abi.CONTACT_CELL_COLS))
    want[:, cols] = tree_sum(C, ids, ROWS * COLS)
    for c in range(ROWS * COLS):
        m = on & (ids == c)
        if not m.any():
            continue
        want[c, 4] = env[m, 3].max()
        ms = m & (env[:, 0] > 0)
        for j in range(24):
            want[c, 8 + 13 * j + 8:8 + 13 * j + 11] = (body[m, j, 4].max(), body[m, j, 10].max(),
                                                       body[ms, j, 7].min() if ms.any() else 0.0)
    return want, C


@pytest.fixture(scope="module")
def env():
    env, _, _ = E.make_env("go2", N, "cuda:0", **{"domain_rand.scheduled_pushes": True,
                                                  "commands.scheduled_commands": True})
    assert env.num_envs == N
    return env


@pytest.fixture(scope="module")
def record_sets(env):
    """The joint and the contact set: (name, the cells the kernel wrote, the wanted cells, the sum
    columns' contributions, the cell ids)."""
    out = []
    for name, seed, inputs, want, buffers, rec, cells in (
            ("joint set", 11, joint_inputs, joint_want, env.joint_buffers, ("joint_rec", "joint_body", "joint_status"),
             env.joint_cells),
            ("contact set", 13, contact_inputs, contact_want, env.contact_buffers,
             ("contact_body", "contact_env", "contact_status"), env.contact_cells)):
        *src, ids = inputs(torch.Generator().manual_seed(seed))
        dev_ids = torch.zeros(N, dtype=torch.int32, device=env.device)
        buffers(ROWS, COLS, dev_ids)
        for attr, t in zip(rec, src):
            dst = getattr(env, attr)
            assert dst.shape == t.shape and dst.dtype == t.dtype, attr
            dst.copy_(t)
        dev_ids.copy_(ids)
        w, C = want(*(t.numpy().astype(np.float64 if t.dtype == torch.float32 else np.int64) for t in src), ids.numpy())
        out.append((name, cells().reshape(ROWS * COLS, -1), w, C, ids.numpy()))
    return out


@pytest.fixture(scope="module")
def sets(env):
    """Per set: (name, the cells the kernels wrote, the contributions, the cell ids)."""
    gen = torch.Generator().manual_seed(7)
    env.push_eval_buffers(ROWS, COLS, 0.3)
    env.cmd_eval_buffers(ROWS, COLS, 0.3, 0.3, 0)
    gait_ids = torch.zeros(N, dtype=torch.int32, device=env.device)
    env.gait_buffers(ROWS, COLS, gait_ids)
    host = {}

    def put(name, dst, src):
        assert dst.shape == src.shape and dst.dtype == src.dtype, name
        dst.copy_(src)
        host[name] = src.numpy().astype(np.float64 if src.dtype == torch.float32 else np.int64)

    for p, rec in (("push", env.push_rec), ("cmd", env.cmd_rec)):
        put(p + "_acc", getattr(env, p + "_eval_acc"), values(gen, *getattr(env, p + "_eval_acc").shape))
        put(p + "_status", getattr(env, p + "_eval_status"), torch.randint(0, 4, (N,), generator=gen).to(torch.uint8))
        put(p + "_ids", getattr(env, p + "_cell_ids"), torch.randint(0, ROWS * COLS, (N,), generator=gen).int())
        put(p + "_rec", rec, gate(gen, values(gen, *rec.shape)))
    put("gait_foot", env.gait_foot, values(gen, *env.gait_foot.shape))
    put("gait_body", env.gait_body, gate(gen, values(gen, *env.gait_body.shape)))
    put("gait_status", env.gait_status, torch.randint(0, 4, (N,), generator=gen).to(torch.uint8))
    put("gait_ids", gait_ids, torch.randint(0, ROWS * COLS, (N,), generator=gen).int())
    pcells, push = env.eval_push_cells()
    ccells, cmd = env.eval_command_cells()
    gait = env.gait_cells()
    flat = lambda t: t.numpy().reshape(ROWS * COLS, -1)  # noqa: E731
    h = host
    return [
        ("push set, cells", flat(pcells), eval_contrib(h["push_acc"], h["push_status"]), h["push_ids"]),
        ("push set, push cells", flat(push), push_contrib(h["push_rec"], h["push_status"]), h["push_ids"]),
        ("command set, cells", flat(ccells), eval_contrib(h["cmd_acc"], h["cmd_status"]), h["cmd_ids"]),
        ("command set, command cells", flat(cmd), cmd_contrib(h["cmd_rec"], h["cmd_status"]), h["cmd_ids"]),
        ("gait set", flat(gait), gait_contrib(h["gait_foot"], h["gait_body"], h["gait_status"]), h["gait_ids"]),
    ]


def test_cells_equal_the_documented_tree(sets):
    assert [s[1].shape[1] for s in sets] == [12, 5, 12, 9, 61]
    for name, got, C, ids in sets:
        want = tree_sum(C, ids, ROWS * COLS)
        diff = np.argwhere(got != want)
        print(f"{name}: {got.size} sums, {len(diff)} differ from the tree")
        assert np.array_equal(got, want), f"{name}: (cell, column) {diff[:8].tolist()} differ from the tree"


def test_inputs_tell_orders_apart(sets):
    for names in (("push set, cells", "push set, push cells"), ("command set, cells", "command set, command cells"),
                  ("gait set",)):
        n = 0
        for name, _, C, ids in sets:
            if name in names:
                n += int((tree_sum(C, ids, ROWS * COLS) != env_order_sum(C, ids, ROWS * COLS)).sum())
        print(f"{names[0].split(',')[0]}: the env-order sum differs from the tree in {n} (cell, column) sums")
        assert n >= 1


def test_record_cells_equal_the_documented_tree(record_sets):
    assert [s[1].shape[1] for s in record_sets] == [246, 320]
    for name, got, want, _, _ in record_sets:
        want = torch.from_numpy(want)
        diff = (got.view(torch.int64) != want.view(torch.int64)).nonzero()
        print(f"{name}: {got.numel()} cell entries, {len(diff)} differ from the tree and the extremes")
        assert torch.equal(got.view(torch.int64), want.view(torch.int64)), \
            f"{name}: (cell, column) {diff[:8].tolist()} differ from the tree or the extremes"


def test_record_inputs_tell_orders_apart(record_sets):
    for name, _, _, C, ids in record_sets:
        n = int((tree_sum(C, ids, ROWS * COLS) != env_order_sum(C, ids, ROWS * COLS)).sum())
        print(f"{name}: the env-order sum differs from the tree in {n} (cell, column) sums")
        assert n >= 1
