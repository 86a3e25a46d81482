"""The loss heads in the last forward level's epilogue (lgx_s8_heads_fwd, include/lgx_s8.h) against
the launches it replaces: the forward level (lgx_s8_gemm_group) followed by lgx_loss_heads_tail.

The contract is bit equality on the raw words (torch.equal), with everything no producer writes
poisoned (NaN in fp32 buffers, 0x7fc0 in both S8 planes). Every output of the fused launch is
bit-equal to the replaced launches': no sum's order moved (the row arithmetic is one copy,
csrc/lgx_heads_row.h; the partials stay per 32 rows, summed in row order).

Shapes: rows 64 (one partial tile, the executor's ROW_ALIGN minimum), 192 (a full tile and a half
tile: row masking, partials that do not exist), 320 (three tiles, the last partial); hidden
256 -> 128 -> {A, 1} (K = 256: 8 K steps, across the 2-stage pipeline's wrap), once 256 -> 96 (pad
columns of the tile), A = 12 and A = 3.
"""
import functools

import pytest
import torch

import learner_case as LC
import learner_replay as R

pytestmark = pytest.mark.gpu
dev = "cuda:0"
POISON = 0x7FC07FC0  # bf16 NaN in both halves of a word: both S8 planes
K_IN = 256
CASES = [(64, 128, 12), (192, 128, 12), (320, 128, 12), (192, 96, 12), (192, 128, 3)]


def _mods():
    from legged_gym_custom_amd.rsl_rl.modules import hip_mlp as H
    from legged_gym_custom_amd.rsl_rl.modules import hip_s8 as S
    return H, S


@functools.lru_cache(maxsize=None)
def _inputs(M, Hd, A):
    H, S = _mods()
    g = torch.Generator(device=dev).manual_seed(1000 * M + 10 * Hd + A)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    L, E = 20, 3
    d = dict(M=M, Hd=Hd, A=A, L=L, E=E)
    for n in ("x", "xc"):  # the layer below's S8 outputs, one spare block of pad rows
        d[n] = S.to_s8_torch(torch.nn.functional.elu(r(M, K_IN)), rows_pad=M + 64)
    for n in ("W2", "Wc2"):
        d[n] = S.to_s8_torch(0.08 * r(Hd, K_IN))
    d.update(b2=0.3 * r(Hd), bc2=0.3 * r(Hd), W=0.1 * r(A, Hd), b=r(A), Wc=0.1 * r(1, Hd), bc=r(1),
             std=r(A).abs() + 0.5, actions=r(M, A), old_logp=r(M, 1), adv=r(M, 1), tv=r(M, 1), ret=r(M, 1),
             old_mu=r(M, A), old_sigma=r(M, A).abs() + 0.5, p_lat=r(M, L), a_lat=r(M, L), pred=r(M, E), t_est=r(M, E),
             seeds=torch.tensor([1.0, 1.3, -0.01, 0.05, 1.0], device=dev))
    return d


def _s8_out(S, rows, cols, poison):
    buf = S.empty(rows + 64, cols, dev)
    if poison:
        buf.fill_(POISON)
    return buf


def _run(M, Hd, A, fused, poison=False, dec_in=None):
    """One pass: the forward level + lgx_loss_heads_tail, or lgx_s8_heads_fwd + the aux head (lgx_s8_dx_group_aux);
    then the reduce launch. Returns the consumer-visible outputs (valid regions, cloned)."""
    H, S = _mods()
    d = _inputs(M, Hd, A)
    L, E = d["L"], d["E"]
    nt, nblk = (M + 31) // 32, (M + 255) // 256
    nan = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731
    x, xc = d["x"].clone(), d["xc"].clone()
    if poison:
        x[M:] = POISON
        xc[M:] = POISON
    o = dict(y8=_s8_out(S, M, Hd, poison), yc8=_s8_out(S, M, Hd, poison), dy8=_s8_out(S, M, Hd, poison),
             dyc8=_s8_out(S, M, Hd, poison), dmu8=_s8_out(S, M, A, poison), dv8=_s8_out(S, M, 1, poison),
             de8=_s8_out(S, M, E, poison), mu=nan(M, A), value=nan(M, 1), cs_y=nan(nt, Hd), cs_yc=nan(nt, Hd),
             cs_mu=nan(nt, A), cs_v=nan(nt, 1), cs_e=nan(nblk, E), ws=nan(19 * nt), wsa=nan(2 * nblk), out=nan(4),
             out_aux=nan(2), kl=nan(1), dstd=nan(A), dp=nan(M, L),
             dec=torch.zeros(M, dtype=torch.uint8, device=dev), dec_c=torch.zeros(M, dtype=torch.uint8, device=dev))
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    h = H.HeadArgs(mu=o["mu"].data_ptr(), value=o["value"].data_ptr(), std=d["std"].data_ptr(),
                   actions=d["actions"].data_ptr(), old_logp=d["old_logp"].data_ptr(), adv=d["adv"].data_ptr(),
                   target_values=d["tv"].data_ptr(), returns=d["ret"].data_ptr(), old_mu=d["old_mu"].data_ptr(),
                   old_sigma=d["old_sigma"].data_ptr(), B=M, A=A, clip=0.2, clipped_value=1, out=o["out"].data_ptr(),
                   g=d["seeds"].data_ptr(), dstd=o["dstd"].data_ptr(), ws=o["ws"].data_ptr(), counter=cnt.data_ptr(),
                   accumulate_dstd=0)
    ax = H.AuxArgs(p=d["p_lat"].data_ptr(), a=d["a_lat"].data_ptr(), L=L, e=d["pred"].data_ptr(),
                   t=d["t_est"].data_ptr(), E=E, B=M, out=o["out_aux"].data_ptr(), g=d["seeds"].data_ptr() + 12,
                   dp=o["dp"].data_ptr(), ws=o["wsa"].data_ptr(), counter=cnt.data_ptr() + 4, ld_p=L)
    s8 = H.HeadsS8Args(dmu_s8=o["dmu8"].data_ptr(), ld_dmu=o["dmu8"].shape[1], dmu_cs=o["cs_mu"].data_ptr(),
                       dvalue_s8=o["dv8"].data_ptr(), ld_dvalue=o["dv8"].shape[1], dvalue_cs=o["cs_v"].data_ptr(),
                       de_s8=o["de8"].data_ptr(), ld_de=o["de8"].shape[1], de_cs=o["cs_e"].data_ptr(),
                       decisions_out=o["dec"].data_ptr(), decisions_in=None if dec_in is None else dec_in.data_ptr())
    t = H.HeadsTailArgs(y=o["y8"].data_ptr(), ld_y=o["y8"].shape[1], W=d["W"].data_ptr(), b=d["b"].data_ptr(),
                        dy=o["dy8"].data_ptr(), ld_dy=o["dy8"].shape[1], dy_cs=o["cs_y"].data_ptr(),
                        yc=o["yc8"].data_ptr(), ld_yc=o["yc8"].shape[1], Wc=d["Wc"].data_ptr(), bc=d["bc"].data_ptr(),
                        dyc=o["dyc8"].data_ptr(), ld_dyc=o["dyc8"].shape[1], dyc_cs=o["cs_yc"].data_ptr(),
                        mu_out=o["mu"].data_ptr(), value_out=o["value"].data_ptr(), H=Hd, Hc=Hd)

    def fwd(xin, W8, bias, y8, head):
        return S.GemmArgs(A=xin.data_ptr(), lda=xin.shape[1], B=W8.data_ptr(), ldb=W8.shape[1], M=M, N=Hd, K=K_IN,
                          epilogue=S.EPI_BIAS | S.EPI_ELU | head, C=y8.data_ptr(), ldc=y8.shape[1], bias=bias.data_ptr())
    if fused:
        S.heads_fwd([fwd(x, d["W2"], d["b2"], o["y8"], S.EPI_HEAD_ACTOR),
                     fwd(xc, d["Wc2"], d["bc2"], o["yc8"], S.EPI_HEAD_CRITIC)], h, s8, t,
                    decisions_critic=o["dec_c"].data_ptr())
        S.dx_group_aux([], ax, s8)  # the aux head alone (the executor: in front of an input-gradient level)
        o["dec"] |= o["dec_c"]
    else:
        S.gemm_group([fwd(x, d["W2"], d["b2"], o["y8"], 0), fwd(xc, d["Wc2"], d["bc2"], o["yc8"], 0)], S.FWD)
        H._check(H.lib().lgx_loss_heads_tail(H.C.byref(h), H.C.byref(ax), H.C.byref(s8), H.C.byref(t), H._stream()),
                 "lgx_loss_heads_tail")
    ws = o["ws"].data_ptr()  # the head's totals, as the executor reduces them (s8_update.py)
    S.reduce([S.flat_reduce(ws, 19, o["out"].data_ptr(), 2, nt), S.flat_reduce(ws + 8, 19, o["out"].data_ptr() + 12, 1, nt),
              S.flat_reduce(ws + 8, 19, o["kl"].data_ptr(), 1, nt), S.flat_reduce(ws + 12, 19, o["dstd"].data_ptr(), A, nt)])
    torch.cuda.synchronize()
    r8 = lambda n: (n + 7) // 8 * 8  # noqa: E731
    res = {k: o[k] for k in ("mu", "value", "cs_y", "cs_yc", "cs_mu", "cs_v", "cs_e", "out", "out_aux", "kl", "dstd",
                             "dp", "dec")}
    res["ws"] = o["ws"].view(nt, 19)[:, :3 + A].clone()
    for k, n in (("y8", Hd), ("yc8", Hd), ("dy8", Hd), ("dyc8", Hd), ("dmu8", A), ("dv8", 1), ("de8", E)):
        res[k] = o[k][:M, :r8(n)].clone()      # the words a producer writes: whole groups of the M rows
        res[k + ".pad"] = torch.stack(S.planes(o[k], M, r8(n)))[..., n:].clone()  # the last group's pad columns
    return res


@functools.lru_cache(maxsize=None)
def _reference(M, Hd, A):
    return _run(M, Hd, A, fused=False)


def _assert_equal(got, ref, what):
    for k, v in ref.items():
        a, b = got[k], v
        if a.is_floating_point():  # raw words: NaN == NaN, -0 != +0
            a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
        assert torch.equal(a, b), f"{what}: {k} differs in {int((a != b).sum())} of {a.numel()} words"


@pytest.mark.parametrize("M,Hd,A", CASES)
def test_fused_launch_equals_the_launches_it_replaces(M, Hd, A):
    """y2 / y2_c S8, mu, value, dy2 / dy2_c S8, every column-sum partial, the head's partial rows and
    its totals after the reduce launch, dstd, the KL output, the aux head's outputs and the
    recorded decisions: bit for bit."""
    ref = _reference(M, Hd, A)
    for k, v in ref.items():
        if v.is_floating_point():
            assert torch.isfinite(v).all(), f"reference {k}"
    assert ref["dec"].ne(0).any()
    _assert_equal(_run(M, Hd, A, fused=True), ref, "fused")


@pytest.mark.parametrize("M,Hd,A", CASES)
def test_poisoned_pads(M, Hd, A):
    """With the inputs' pad rows and every output buffer poisoned before the run, every
    consumer-visible output is finite and equal to the unpoisoned reference's; the pad columns of
    the S8 outputs' last groups are zero."""
    got = _run(M, Hd, A, fused=True, poison=True)
    for k, v in got.items():
        if v.is_floating_point():
            assert torch.isfinite(v).all(), k
        if k.endswith(".pad"):
            assert not v.any(), k
    _assert_equal(got, _reference(M, Hd, A), "poisoned")


def test_recorded_decisions_replay_the_same_gradients():
    """decisions_out of the fused launch (the actor tiles' and the critic tiles' bits, ORed), fed
    back as decisions_in, reproduces every output; a record with all decisions flipped does not
    (the hook is live in both kinds of tile)."""
    M, Hd, A = 192, 128, 12
    first = _run(M, Hd, A, fused=True)
    again = _run(M, Hd, A, fused=True, dec_in=first["dec"].clone())
    _assert_equal(again, first, "replay")
    flipped = (first["dec"] ^ 0x24).clone()  # the ratio-in-band and value-in-band bits
    other = _run(M, Hd, A, fused=True, dec_in=flipped)
    assert not torch.equal(other["dy8"], first["dy8"]) and not torch.equal(other["dyc8"], first["dyc8"])
    _assert_equal(other, _run(M, Hd, A, fused=False, dec_in=flipped), "forced decisions")


# ------------------------------------------------------------------ the executor
def _case(name, **over):
    """A temporary learner case (tests/learner_case.py), registered for the caller's lifetime."""
    class _Ctx:
        def __enter__(self):
            LC.CASES[name] = dict(LC.CASES["go2"], **over)
            return name

        def __exit__(self, *exc):
            del LC.CASES[name]
    return _Ctx()


def _poison_columns(buf, c0, c1):
    """bf16 NaN into both planes of S8 columns [c0, c1) of every row (column c of group g: hi at
    bf16 16 g + c % 8 of the row, lo 8 further)."""
    v = buf.view(torch.bfloat16).view(buf.shape[0], buf.shape[1] // 8, 2, 8)
    for c in range(c0, c1):
        v[:, c // 8, :, c % 8] = float("nan")


def _prepared(case, use_s8=True):
    alg = R.build(case, dev, use_graphs=False)
    alg.use_s8 = use_s8
    R.rollout(alg, case, 1, {}, False, dev)
    alg.total_updates = LC.TOTAL_UPDATES
    alg._reg_coef.fill_(alg.reg_coef())
    alg._perm.copy_(torch.from_numpy(LC.permutation(case, 1)).to(dev))
    alg._precompute()
    return alg


def _snapshot(alg):
    return ([p.grad.detach().clone() for n, p in R.named_params(alg) if not n.startswith("adaptation")] +
            [alg._head_out.clone(), alg._aux_out.clone()])


def test_graph_equals_eager_with_poisoned_pads():
    """One whole minibatch (192 rows, both networks) captured in a torch.cuda.graph and replayed
    twice equals its eager run bit for bit, and the eager run equals the replaced launches'
    (heads_fwd = False on the same buffers); the segmented actor input's gaps, the pad columns of
    the activations and gradients the fused launch reads or writes, and the fp32 outputs poisoned."""
    from legged_gym_custom_amd.rsl_rl.modules import hip_s8 as S
    with _case("go2_rows192", N=32) as case:
        alg = _prepared(case)
        mb = alg._s8
        assert mb is not None and mb.mb == 192 and mb.heads_fwd
        # poison, then let the per-update producers rewrite what they own (prepare)
        for c0, c1 in ((mb.nobs, mb.P0), (mb.P0 + mb.nlat, mb.P1), (mb.P1 + mb.nscan, mb.P2), (mb.P2 + mb.nest, mb.W8)):
            _poison_columns(mb.ain, c0, c1)
        for p in (mb.actor, mb.critic):
            for buf, n in ((p.out[-1], p.W[-2].shape[0]), (p.dy[-2], p.W[-2].shape[0]), (p.dy[-1], p.W[-1].shape[0])):
                buf[:, (n + 7) // 8 * 8:] = POISON
            for cs in p.cs[-2:]:
                cs.fill_(float("nan"))
        for t in (mb.mu, mb.value, mb.head_ws):
            t.fill_(float("nan"))
        alg._precompute()
        idx = alg._minibatches()[1]

        def once():
            alg._minibatch_grads(idx)
            torch.cuda.synchronize()
            return _snapshot(alg)
        eager = once()
        assert all(torch.isfinite(t).all() for t in eager)
        mb.heads_fwd = False
        replaced = once()
        mb.heads_fwd = True
        assert all(torch.equal(a, b) for a, b in zip(eager, replaced))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            alg._minibatch_grads(idx)
        for _ in range(2):
            for _n, p in R.named_params(alg):
                if p.grad is not None:
                    p.grad.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(_snapshot(alg)[:len(eager)], eager))
        # the S8 outputs' own pad columns are zero (A = 12: columns 12..15 of dmu; 1..7 of dvalue)
        for buf, n in ((mb.actor.dy[-1], 12), (mb.critic.dy[-1], 1)):
            hi, lo = S.planes(buf, mb.mb, (n + 7) // 8 * 8)
            assert not hi[:, n:].any() and not lo[:, n:].any()


def test_wider_last_hidden_layer_falls_back_to_heads_tail():
    """Hidden width 160 (> one 128-column tile): the executor selects lgx_loss_heads_tail, and the
    update matches the autograd path within tests/test_gpu_s8_update.py's bound."""
    with _case("go2_h160", actor=[512, 256, 160], critic_h=[512, 256, 160]) as case:
        out = []
        for use_s8 in (False, True):
            alg = _prepared(case, use_s8)
            assert (alg._s8 is not None) == use_s8
            if use_s8:
                assert alg._s8.tail and not alg._s8.heads_fwd
            alg._minibatch_grads(alg._minibatches()[0])
            torch.cuda.synchronize()
            out.append(({n: p.grad.detach().clone() for n, p in R.named_params(alg) if not n.startswith("adaptation")},
                        alg._head_out.clone(), alg._aux_out.clone()))
        (g0, h0, a0), (g1, h1, a1) = out
        for n, r in g0.items():
            scale = float(r.abs().max())
            err = float((g1[n] - r).abs().max())
            assert err <= 1e-4 * scale + 1e-8, (n, err, scale)
        torch.testing.assert_close(h1, h0, rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(a1, a0, rtol=1e-5, atol=1e-7)
