"""tests/s8_case.py checked on the CPU: its statement of the S8 format against torch's bf16 rounding
and against hip_s8's torch helpers, its fp64 references against a plain matmul, its operands'
guards, and the sensitivity condition of every GEMM case that tests/test_gpu_s8_ref.py compares
with a bound. fp32 subnormals are out of scope: no case draws one, and what the kernels do with
them is the hardware's choice."""
import pytest
import torch

import s8_case as C
from legged_gym_custom_amd.rsl_rl.modules import hip_s8 as S


def _i32(bits):
    return torch.tensor(bits, dtype=torch.int64).add(2 ** 31).remainder(2 ** 32).sub(2 ** 31).to(torch.int32)


def test_split_ref_is_torch_bf16_rounding_bit_for_bit():
    g = torch.Generator().manual_seed(1)
    # +-0; exact ties (mantissa tail 0x8000) after an even and after an odd kept bit, both signs; tails
    # next to a tie; the largest finite bf16 and the carry into the exponent
    bits = [0x00000000, 0x80000000, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001,
            0x3F817FFF, 0x3F818001, 0x3FFF8000, 0x7F7F0000, 0x40490FDB]
    edge = _i32(bits).view(torch.float32)
    mags = torch.logspace(-30, 30, 61).float()
    rnd = torch.randn(4096, generator=g) * mags[torch.randint(0, 61, (4096,), generator=g)]
    x = torch.cat([edge, mags, -mags, rnd])
    hi, lo = C.split_ref(x)
    thi = x.to(torch.bfloat16)
    tlo = (x - thi.float()).to(torch.bfloat16)
    assert torch.equal(hi.view(torch.int16), thi.view(torch.int16))
    assert torch.equal(lo.view(torch.int16), tlo.view(torch.int16))
    # the ties went to even: 0x3F80 8000 -> 0x3F80, 0x3F81 8000 -> 0x3F82
    assert hi.view(torch.int16)[2:4].tolist() == [0x3F80, 0x3F82]


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 8), (5, 13), (70, 65)])
def test_pack_rows_is_to_s8_torch(rows, cols):
    x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows + cols)) * 3
    ld = C.rup(cols, 8)
    buf = C.pack_rows(x)
    assert torch.equal(buf, S.to_s8_torch(x, ld=ld, rows_pad=rows))
    hi, lo = C.unpack_rows(buf, cols)
    shi, slo = S.planes(buf, rows, cols)
    assert torch.equal(hi, shi) and torch.equal(lo, slo)
    assert torch.equal(hi + lo, S.from_s8(buf, rows, cols))
    assert torch.equal((hi.double() + lo.double()), C.dequant(x))


@pytest.mark.parametrize("N,K", C.PACK_SHAPES)
def test_pack_frag_is_pack_ref(N, K):
    from test_gpu_s8 import _pack_ref
    W = torch.randn(N, K, generator=torch.Generator().manual_seed(N + K))
    assert torch.equal(C.pack_frag(W), _pack_ref(S.to_s8_torch(W), N, K))
    assert torch.equal(C.pack_frag(W.t().contiguous(), transpose=True), _pack_ref(S.to_s8_torch(W), N, K))


def test_references_agree_with_a_plain_matmul():
    """To 1e-12 of sum |a b|, on the dequantised values."""
    for kind, M, N, K in (("fwd", 65, 63, 31), ("dx", 129, 120, 65), ("dw", 20, 29, 160)):
        P = C.Gemm(kind, M, N, K)
        am, bm = C.dequant(P.am), C.dequant(P.bm)
        if kind == "fwd":
            hi, lo = C.unpack_rows(C.pack_rows(P.a), K)
            plain = (hi.double() + lo.double()) @ C.dequant(P.b).t()
        elif kind == "dx":
            plain = C.dequant(P.a) @ C.dequant(P.b)
        else:
            plain = C.dequant(P.a).t() @ C.dequant(P.b)
        assert (P.ref - plain).abs().le(1e-12 * (am.abs() @ bm.abs()) + 1e-300).all()
    # the epilogues, the column sums and the chain on top of it
    P = C.Gemm("fwd", 65, 63, 31, bias=True, elu=True)
    z = P.A.value @ P.B.value.t() + P.bias.double()
    assert torch.equal(P.ref, torch.nn.functional.elu(z))
    P = C.Gemm("dx", 65, 63, 31, use_delu=True, add_cols=17)
    y = P.act.value
    ref = (P.A.value @ P.B.value) * torch.where(y > 0, 1.0, y + 1.0)
    ref[:, :17] += P.add.double()
    assert torch.equal(P.ref, ref)
    cs, asum = C.colsums(ref)
    assert cs.shape == (2, 63) and torch.equal(cs[1], ref[64:].sum(0)) and torch.equal(asum[0], ref[:64].abs().sum(0))
    x = C.dequant(torch.randn(5, 20))
    w1, w2 = C.dequant(torch.randn(16, 20)), C.dequant(torch.randn(7, 16))
    b1 = torch.randn(16)
    (y1, e1), (y2, e2) = C.chain_ref(x, [(w1, b1, 1, None), (w2, None, 0, None)])
    assert torch.equal(y1, torch.nn.functional.elu(x @ w1.t() + b1.double()))
    assert torch.equal(y2, y1 @ w2.t())
    assert (e2 >= (e1 + 1e-5 * y1.abs()) @ w2.abs().t()).all() and (e1 > 0).all()


CASES = list(C.all_gemm_cases())


@pytest.mark.parametrize("name,kind,M,N,K,seed", CASES, ids=[c[0] for c in CASES])
def test_sensitivity_condition(name, kind, M, N, K, seed):
    """A condition on the drawn inputs: the CPU emulation of the kernel's product stays within half
    the bound, and with the lo*hi term of one 16x16x32 fragment dropped, in the first and in the last
    K step, it leaves the bound by 4 times somewhere in that fragment. K = 0 has no product."""
    if K == 0:
        return
    P = C.Gemm(kind, M, N, K, seed=seed)
    av, bv = C.dequant(P.am), C.dequant(P.bm)
    ref, bd = av @ bv, C.bound(av, bv)
    assert ((C.emulate(P.am, P.bm) - ref).abs() <= 0.5 * bd).all()
    for step in (0, C.cdiv(K, 32) - 1):
        r = ((C.emulate(P.am, P.bm, drop=(step, 0, 0)) - ref).abs() / bd)[:16, :16].max()
        assert r > 4.0, (step, float(r))


def test_every_gpu_gemm_shape_is_listed():
    listed = {c[1:] for c in CASES}
    for M, N, K in C.SHAPES + C.XCD_SHAPES + C.SPAN_SHAPES:
        assert ("fwd", M, N, K, 0) in listed and ("dx", M, N, K, 0) in listed
    for M, N, K in C.SPAN_SHAPES:
        assert ("dw", N, M, K, 0) in listed
    for shapes in (C.GROUP_SHAPES, C.one_tile_group(21)):
        for i, (M, N, K) in enumerate(shapes):
            assert ("fwd", M, N, K, i) in listed and ("dx", M, N, K, i) in listed
    for M, N, K, _s in C.DW_SHAPES + C.SPLIT_CONTRACT:
        assert ("dw", M, N, K, 0) in listed
    for i, (M, N, K, _s) in enumerate(C.DW_GROUP):
        assert ("dw", M, N, K, i) in listed


@pytest.mark.parametrize("mode,shape,c0,extra", [("row", (5, 33), 0, 0), ("row", (5, 33), 8, 8), ("row", (3, 64), 64, 0),
                                                  ("tr", (33, 5), 0, 0), ("tr", (33, 13), 64, 8), ("tr", (64, 16), 8, 0),
                                                  ("act", (5, 13), 0, 0), ("row", (4, 0), 0, 0), ("tr", (0, 9), 0, 0)])
@pytest.mark.parametrize("pad", ["zero", "finite"])
def test_operand_guards(mode, shape, c0, extra, pad):
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(7))
    op = C.Operand(x, mode, pad, extra, c0)
    assert op.first % 4 == 0 and op.first > 0 and op.ld % 8 == 0
    words = op.flat.view(torch.bfloat16).view(-1, 2).float()
    allowed = op.allowed_mask()
    assert torch.isnan(words[~allowed]).all() and not torch.isnan(words[allowed]).any()
    for name, m in op.guard_regions().items():
        assert not (m & allowed).any() and torch.isnan(words[m]).any(), name
    assert "front" in op.guard_regions() and "behind" in op.guard_regions()
    if c0:
        assert "left" in op.guard_regions()
    if extra:
        assert "right" in op.guard_regions()
    # every element the reference multiplies is there, finite, at its place
    if min(shape) > 0:
        v = op.flat.as_strided(*op.geom).contiguous()
        hi, lo = C.unpack_rows(v, op.width)
        got = (hi.double() + lo.double())
        assert torch.equal(got[:shape[0], :shape[1]], op.value) and torch.isfinite(op.value).all()
        padv = C.FIN if pad == "finite" else 0.0
        mask = torch.ones_like(got, dtype=torch.bool)
        mask[:shape[0], :shape[1]] = False
        assert (got[mask] == padv).all()
        exp_rows = C.rup(shape[0], 32) if mode == "tr" else shape[0]
        exp_w = C.rup(shape[1], {"row": 32, "tr": 8, "act": 8}[mode])
        assert (op.rows, op.width) == (exp_rows, exp_w)


def test_out_masks():
    o = C.Out("s8", 5, 13, ld=24, off=4)
    m = o.written_mask().as_strided((7, 24), (24, 1), 4)
    assert m[:5, :16].all() and not m[:5, 16:].any() and not m[5:].any() and not o.written_mask()[:4].any()
    assert o.untouched() and o.outside_intact()
    o.view().fill_(0)
    assert o.outside_intact() and not o.untouched()
    o.flat[4 + 16] = 0
    assert not o.outside_intact()
    f = C.Out("f32", 3, 5, ld=8, off=3, init=torch.ones(3, 5))
    assert f.outside_intact() and f.values().eq(1).all() and int(f.written_mask().sum()) == 15
    f.flat[3 + 5] = 0.0
    assert not f.outside_intact()
