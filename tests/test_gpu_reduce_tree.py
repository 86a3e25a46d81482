"""The reduce tree of the evaluation (csrc/lgx_env.hip) on the MI355X, pinned bit for bit:
eval_reduce_kernel (12 + 5 push columns), eval_cmd_reduce_kernel (9 columns) and gait_reduce_kernel
(61 columns) against a NumPy float64 restatement of the documented order. One block of 256 threads
per cell; thread t adds its envs t, t + 256, ... in increasing order; inside each wave of 64,
for o = 32, 16, ..., 1: a[:o] += a[o:2 * o]; then ((w0 + w1) + w2) + w3.

No env step is run: the record tensors are written directly, fp32 values randn x 10^uniform(-3, 6)
(nine decades, so the order of the additions shows in the last bits), gates positive for about three
quarters of the envs, statuses from 0..3. 300 envs: threads 0..43 own two envs, the last wave is
partly empty. No tolerance: float64 addition is exact to the bit once its order is fixed, and the
fp32 -> fp64 conversion of the inputs is exact. The test also shows that its inputs tell orders
apart: the plain env-order sum differs from the tree in every one of the three sets."""
import numpy as np
import pytest
import torch

import eval_case as E

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


@pytest.fixture(scope="module")
def sets():
    """Per set: (name, the cells the kernels wrote, the contributions, the cell ids)."""
    env, _, _ = E.make_env("go2", N, "cuda:0", **{"domain_rand.scheduled_pushes": True,
                                                  "commands.scheduled_commands": True})
    assert env.num_envs == N
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
