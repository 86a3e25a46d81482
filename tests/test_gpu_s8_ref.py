"""The S8 GEMM core (liblgx_s8.so: lgx_s8_gemm_group, lgx_s8_split, lgx_s8_reduce, lgx_s8_chain,
lgx_s8_dx_group_aux) against the fp64 references of tests/s8_case.py, at its tile edges.

Every operand is contract-tight (s8_case.Operand: exactly the rows and groups include/lgx_s8.h
promises, NaN everywhere else, the readable pads zero in one operand and finite in the other), every
output a view inside a sentinel-filled buffer (s8_case.Out). After every launch: no NaN in what was
written (a read outside the contract would bring one in), every element outside written_mask()
still the sentinel, every written element within its bound (s8_case's docstring states the bounds),
the S8 output bit-equal to the split of the fp32 copy where both are requested, pads of the last
group zero. Every comparison prints max |err| / bound."""
import ctypes as Ct

import pytest
import torch

import s8_case as C

pytestmark = pytest.mark.gpu

dev = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def S():
    from legged_gym_custom_amd.rsl_rl.modules import hip_s8
    hip_s8.lib()
    return hip_s8


def _report(kind, name, err, bd):
    r = float((err / bd).max()) if err.numel() else 0.0
    print(f"{kind} {name}: max |err| / bound = {r:.3f}")
    return r


def _within(kind, name, got, ref, bd):
    assert not torch.isnan(got).any(), (kind, name, "NaN in the written part")
    err = (got - ref).abs()
    r = _report(kind, name, err, bd)
    assert (err <= bd).all(), (kind, name, r)


def _up(op):
    """An Operand on the device: (the flat buffer, the operand's address)."""
    t = op.flat.to(dev)
    return t, t.data_ptr() + 4 * op.first


def _nanpad(x, extra=3):
    """fp32 x on the device as a view of rows with `extra` NaN columns behind."""
    t = torch.full((x.shape[0], x.shape[1] + extra), NAN, device=dev)
    t[:, :x.shape[1]] = x.to(dev)
    return t


class Job:
    """One FWD / DX problem on the device: operands, fresh guarded outputs, its lgx_s8_gemm_args."""

    def __init__(self, S, P, c=True, c32=True, cs=True):
        self.P, self.keep = P, []
        M, N, K = P.M, P.N, P.K
        ta, pa = _up(P.A)
        tb, pb = _up(P.B)
        self.keep += [ta, tb]
        a = S.GemmArgs(A=pa, lda=P.A.ld, B=pb, ldb=P.B.ld, M=M, N=N, K=K)
        epi = 0
        if P.bias is not None:
            b = torch.cat([torch.full((3,), NAN), P.bias, torch.full((3,), NAN)]).to(dev)
            self.keep.append(b)
            a.bias, epi = b.data_ptr() + 12, epi | S.EPI_BIAS
        if P.elu:
            epi |= S.EPI_ELU
        if P.act is not None:
            ty, py = _up(P.act)
            self.keep.append(ty)
            a.act, a.ld_act, epi = py, P.act.ld, epi | S.EPI_DELU
        if P.add is not None:
            ad = _nanpad(P.add)
            self.keep.append(ad)
            a.addend, a.ld_add, a.add_cols = ad.data_ptr(), ad.stride(0), P.add_cols
        a.epilogue = epi
        self.c = C.Out("s8", M, N, ld=C.rup(N, 8) + 8, off=4, device=dev) if c else None
        self.c32 = C.Out("f32", M, N, ld=N + 3, off=3, device=dev) if c32 else None
        self.cs = C.Out("f32", C.cdiv(M, C.TILE_M), N, ld=N, off=5, device=dev) if cs else None
        if c:
            a.C, a.ldc = self.c.ptr, self.c.ld
        if c32:
            a.C32, a.ldc32 = self.c32.ptr, self.c32.ld
        if cs:
            a.colsum_ws = self.cs.ptr
        self.args = a

    def outs(self):
        return [o for o in (self.c, self.c32, self.cs) if o is not None]

    def untouched(self):
        return all(o.untouched() for o in self.outs())

    def verify(self, name):
        P, kind = self.P, self.P.kind.upper()
        got32 = got8 = None
        if self.c32 is not None:
            assert self.c32.outside_intact(), (name, "fp32 guards")
            got32 = self.c32.values()
            _within(kind, name + " fp32", got32, P.ref, P.e)
        if self.c is not None:
            assert self.c.outside_intact(), (name, "S8 guards")
            w = self.c.view().cpu()
            hi, lo = C.unpack_rows(w, C.rup(P.N, 8))
            assert (hi[:, P.N:] == 0).all() and (lo[:, P.N:] == 0).all(), (name, "pads of the last group")
            got8 = self.c.values()
            _within(kind, name + " S8", got8, P.ref, P.e + C.s8_extra(P.ref))
            if self.c32 is not None:
                assert torch.equal(w, C.pack_rows(self.c32.view().cpu())), (name, "S8 != split(fp32)")
        if self.cs is not None:
            assert self.cs.outside_intact(), (name, "column-sum guards")
            src = got32 if got32 is not None else got8
            if src is not None:
                sums, asum = C.colsums(src)
                _within(kind, name + " colsum", self.cs.values(), sums, C.colsum_tol(asum, got32 is None))


def _same(a, b):
    """Two jobs' outputs, guards included, bit for bit."""
    return all(torch.equal(x.flat, y.flat) for x, y in zip(a.outs(), b.outs()))


OUTS = ((True, False), (False, True), (True, True))  # (C, C32)


# ------------------------------------------------------------------ (a) single problems
@pytest.mark.parametrize("pads", C.PADS, ids=["A0", "B0"])
@pytest.mark.parametrize("M,N,K", C.SHAPES)
def test_fwd_single(S, M, N, K, pads):
    for bias, elu in ((False, False), (True, False), (True, True)):
        P = C.Gemm("fwd", M, N, K, pads=pads, bias=bias, elu=elu)
        if K == 0:  # epilogue(0)
            z = torch.zeros(M, N, dtype=torch.float64) + (P.bias.double() if bias else 0.0)
            assert torch.equal(P.ref, torch.nn.functional.elu(z) if elu else z)
        for c, c32 in OUTS:
            for cs in (False, True):
                J = Job(S, P, c, c32, cs)
                S.gemm_group([J.args], S.FWD)
                torch.cuda.synchronize()
                J.verify(f"{M}x{N}x{K} bias{int(bias)} elu{int(elu)} C{int(c)} C32{int(c32)} cs{int(cs)}")


@pytest.mark.parametrize("pads", C.PADS, ids=["A0", "B0"])
@pytest.mark.parametrize("M,N,K", C.SHAPES)
def test_dx_single(S, M, N, K, pads):
    for use_delu, add_cols in ((False, 0), (True, 0), (True, 1), (True, 17), (False, N), (True, N)):
        P = C.Gemm("dx", M, N, K, pads=pads, use_delu=use_delu, add_cols=add_cols)
        for c, c32 in OUTS:
            for cs in (False, True):
                J = Job(S, P, c, c32, cs)
                S.gemm_group([J.args], S.DX)
                torch.cuda.synchronize()
                J.verify(f"{M}x{N}x{K} delu{int(use_delu)} add{P.add_cols} C{int(c)} C32{int(c32)} cs{int(cs)}")


# ------------------------------------------------------------------ (b) operands as column spans
@pytest.mark.parametrize("pads", C.PADS, ids=["A0", "B0"])
@pytest.mark.parametrize("c0", [8, 64])
@pytest.mark.parametrize("M,N,K", C.SPAN_SHAPES)
def test_column_span_operands(S, M, N, K, c0, pads):
    """FWD's X, DX's W (TR) and both DW operands as column spans of wider, NaN-filled rows."""
    P = C.Gemm("fwd", M, N, K, pads=pads, c0=(c0, 0), extra=(8, 0), bias=True, elu=True)
    J = Job(S, P)
    S.gemm_group([J.args], S.FWD)
    P2 = C.Gemm("dx", M, N, K, pads=pads, c0=(0, c0), extra=(0, 8), use_delu=True, add_cols=17)
    J2 = Job(S, P2)
    S.gemm_group([J2.args], S.DX)
    P3 = C.Gemm("dw", N, M, K, pads=pads, c0=(c0, c0), extra=(8, 0))
    o3, a3, k3 = _dw_args(S, P3, 1)
    S.gemm_group([a3], S.DW)
    torch.cuda.synchronize()
    J.verify(f"span {M}x{N}x{K} c0 {c0}")
    J2.verify(f"span {M}x{N}x{K} c0 {c0}")
    _dw_verify(P3, o3, 1, f"span {N}x{M}x{K} c0 {c0}")


# ------------------------------------------------------------------ (c) tile counts against the 8 XCD slots
@pytest.mark.parametrize("kind", ["fwd", "dx"])
@pytest.mark.parametrize("M,N,K", C.XCD_SHAPES)
def test_tile_counts(S, M, N, K, kind):
    P = C.Gemm(kind, M, N, K, pads=C.PADS[M % 2], bias=True, elu=True, use_delu=True, add_cols=N)
    J = Job(S, P)
    S.gemm_group([J.args], S.FWD if kind == "fwd" else S.DX)
    torch.cuda.synchronize()
    J.verify(f"tiles {M}x{N}x{K}")


# ------------------------------------------------------------------ (d) groups
def _group_vs_single(S, kind, probs, name, chunked=False):
    code = S.FWD if kind == "fwd" else S.DX
    grouped = [Job(S, P) for P in probs]
    single = [Job(S, P) for P in probs]
    S.gemm_group([J.args for J in grouped], code)
    for J in single:
        S.gemm_group([J.args], code)
    torch.cuda.synchronize()
    for i, (g, s) in enumerate(zip(grouped, single)):
        if g.P.M == 0:
            assert g.untouched(), (name, i, "a skipped problem's output was touched")
            continue
        assert _same(g, s), (name, i, "grouped != single")
        g.verify(f"{name}[{i}] {g.P.M}x{g.P.N}x{g.P.K}")


def _gemm(kind, M, N, K, i=0):
    return C.Gemm(kind, M, N, K, pads=C.PADS[i % 2], bias=True, elu=i % 3 != 0, use_delu=i % 3 != 1,
                  add_cols=(0, 1, N)[i % 3], seed=i)


@pytest.mark.parametrize("kind", ["fwd", "dx"])
def test_group_of_five_reordered(S, kind):
    """K = (0, 33, 160, 32, 96) with 1, 2, 4, 9, 3 tiles in that order: launch_fwd sorts them by K and
    cuts the tile list into 8 XCD ranges; DX deals each problem's tiles over start[] / per_xcd."""
    _group_vs_single(S, kind, [_gemm(kind, M, N, K, i) for i, (M, N, K) in enumerate(C.GROUP_SHAPES)], f"group5 {kind}")


@pytest.mark.parametrize("kind", ["fwd", "dx"])
@pytest.mark.parametrize("n", [20, 21])
def test_group_of_one_tile_problems(S, kind, n):
    """LGX_S8_GROUP_MAX problems in one launch, and one more through the wrapper's chunking."""
    probs = [_gemm(kind, M, N, K, i) for i, (M, N, K) in enumerate(C.one_tile_group(n))]
    _group_vs_single(S, kind, probs, f"group{n} {kind}")


@pytest.mark.parametrize("kind", ["fwd", "dx"])
def test_group_skips_an_empty_problem(S, kind):
    _group_vs_single(S, kind, [_gemm(kind, M, N, K, i) for i, (M, N, K) in enumerate(C.GROUP_EMPTY)],
                     f"group-empty {kind}")


# ------------------------------------------------------------------ (e) DW
def _dw_args(S, P, split, accum=False, epi=None):
    """(outputs, lgx_s8_gemm_args, keep) of a DW problem: split 1 into a guarded C32 of pitch N + 5
    (0.5 everywhere under EPI_ACCUM), split > 1 into a NaN-filled dense [split][M][N] workspace."""
    ta, pa = _up(P.A)
    tb, pb = _up(P.B)
    M, N = P.M, P.N
    if split == 1:
        o = C.Out("f32", M, N, ld=N + 5, off=3, device=dev, init=torch.full((M, N), 0.5) if accum else None)
    else:
        o = C.Out("f32", split * M, N, ld=N, off=4, device=dev, init=torch.full((split * M, N), NAN))
    a = S.GemmArgs(A=pa, lda=P.A.ld, B=pb, ldb=P.B.ld, M=M, N=N, K=P.K, C32=o.ptr, ldc32=o.ld, split=split,
                   epilogue=(S.EPI_ACCUM if accum else 0) if epi is None else epi)
    return o, a, (ta, tb)


def _dw_verify(P, o, split, name, accum=False):
    assert o.outside_intact(), (name, "guards")
    got = o.values()
    if split == 1:
        ref, e = C.dw_ref(P.A.value, P.B.value, torch.full((P.M, P.N), 0.5) if accum else None)
        _within("DW", name, got, ref, e)
        return
    assert not torch.isnan(got).any(), (name, "a requested slab was not written")
    _within("DW", name + " slabs", got.reshape(split, P.M, P.N).sum(0), P.ref, P.e)


def _dw_reduce(S, P, o, split, name):
    """lgx_s8_reduce of the `split` requested slabs onto 0.25."""
    out = C.Out("f32", 1, P.M * P.N, off=4, device=dev, init=torch.full((1, P.M * P.N), 0.25))
    S.reduce([S.flat_reduce(o.ptr, P.M * P.N, out.ptr, P.M * P.N, split, accumulate=1)])
    torch.cuda.synchronize()
    assert out.outside_intact()
    _within("DW", name + " reduced", out.values().view(P.M, P.N) - 0.25, P.ref, P.e + 1e-6)


@pytest.mark.parametrize("pads", C.PADS, ids=["A0", "B0"])
@pytest.mark.parametrize("M,N,K,split", C.DW_SHAPES)
def test_dw_single(S, M, N, K, split, pads):
    P = C.Gemm("dw", M, N, K, pads=pads)
    for accum in (False, True):
        o, a, _k = _dw_args(S, P, 1, accum)
        S.gemm_group([a], S.DW)
        torch.cuda.synchronize()
        _dw_verify(P, o, 1, f"{M}x{N}x{K} accum{int(accum)}", accum)
    if split > 1:
        o, a, _k = _dw_args(S, P, split)
        S.gemm_group([a], S.DW)
        torch.cuda.synchronize()
        _dw_verify(P, o, split, f"{M}x{N}x{K} split {split}")
        _dw_reduce(S, P, o, split, f"{M}x{N}x{K} split {split}")


@pytest.mark.parametrize("shapes", [C.DW_GROUP, C.DW_FALLBACK], ids=["units", "fallback"])
def test_dw_group_equals_single(S, shapes):
    """deal_units (<= 256 units: one K-chunk slice of a problem per XCD slot) and its fallback to the
    per-problem deal above 256 units: every output bit-equal to the single launch, within bound."""
    probs = [C.Gemm("dw", M, N, K, pads=C.PADS[i % 2], seed=i) for i, (M, N, K, _s) in enumerate(shapes)]
    grouped = [_dw_args(S, P, s[3]) for P, s in zip(probs, shapes)]
    single = [_dw_args(S, P, s[3]) for P, s in zip(probs, shapes)]
    S.gemm_group([g[1] for g in grouped], S.DW)
    for g in single:
        S.gemm_group([g[1]], S.DW)
    torch.cuda.synchronize()
    for i, (P, s, g, q) in enumerate(zip(probs, shapes, grouped, single)):
        assert torch.equal(g[0].flat, q[0].flat), (i, "grouped != single")
        _dw_verify(P, g[0], s[3], f"group[{i}] {s}")


# ------------------------------------------------------------------ (f) the split contract
@pytest.mark.parametrize("accum", [False, True])
@pytest.mark.parametrize("M,N,K,split", C.SPLIT_CONTRACT)
def test_dw_split_contract(S, M, N, K, split, accum):
    """A request of split > 1 is a partial workspace [split][M][N] with ALL slabs written (zeros where
    the slab's K range is empty) and EPI_ACCUM ignored, also where whole 32-deep steps leave fewer
    chunks than slabs (K = 160 / 4, 20 / 4, 64 / 5, 0 / 2). K = 0 with split 1: zero, or unchanged
    under EPI_ACCUM."""
    P = C.Gemm("dw", M, N, K)
    o, a, _k = _dw_args(S, P, split, accum)
    S.gemm_group([a], S.DW)
    torch.cuda.synchronize()
    name = f"contract {M}x{N}x{K} split {split} accum{int(accum)}"
    _dw_verify(P, o, split, name, accum)
    if split > 1:
        kchunk = C.rup(C.cdiv(K, split), 32) if K else 32
        slabs = o.values().reshape(split, M, N)
        for z in range(split):
            if z * kchunk >= K:
                assert (slabs[z] == 0).all(), (name, z, "an empty slab is not zero")
        _dw_reduce(S, P, o, split, name)
    elif K == 0:
        assert (o.values() == (0.5 if accum else 0.0)).all()


# ------------------------------------------------------------------ (g) lgx_s8_split
def _split_src(rows, cols, g, src_rows=None):
    x = torch.randn(src_rows or rows, cols, generator=g) * torch.logspace(-6, 3, cols)
    return x, _nanpad(x)[:, :cols]


@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("rows,cols", C.SPLIT_SHAPES)
def test_split_rows(S, rows, cols, gather):
    g = torch.Generator().manual_seed(rows + cols)
    x, xd = _split_src(rows, cols, g, rows + 5 if gather else None)
    idx = torch.randint(0, rows + 5, (rows,), generator=g) if gather else None  # a draw with repeats
    idxd = idx.to(dev) if gather else None
    dst = C.Out("s8", rows, cols, ld=C.rup(cols, 8) + 8, off=4, device=dev)
    cs = C.Out("f32", C.cdiv(rows, C.SPLIT_ROWS), cols, ld=cols, off=3, device=dev) if cols <= 64 else None
    j = S.split_job(xd, dst.ptr, dst.ld, idx=idxd, rows=rows)
    if cs is not None:
        j.colsum_ws = cs.ptr
    S.split([j])
    torch.cuda.synchronize()
    src = x[idx] if gather else x
    assert dst.outside_intact(), "S8 guards"
    assert torch.equal(dst.view().cpu(), C.pack_rows(src)), "not the split of the source rows"
    if cs is not None:
        assert cs.outside_intact()
        sums, asum = C.colsums(src.double(), C.SPLIT_ROWS)
        _within("SPLIT", f"{rows}x{cols} colsum", cs.values(), sums, C.colsum_tol(asum, False))


@pytest.mark.parametrize("transpose", [False, True])
def test_split_packed(S, transpose):
    """Packed and packed-transposed jobs against pack_frag; the destination is zeroed (the format's
    own pads are never written), with a 2 KB sentinel guard behind."""
    g = torch.Generator().manual_seed(5)
    jobs, checks = [], []
    for N, K in C.PACK_SHAPES:
        W = torch.randn(K, N, generator=g) if transpose else torch.randn(N, K, generator=g)
        Wd = _nanpad(W)[:, :W.shape[1]]
        n = C.cdiv(N, 16) * C.cdiv(K, 32) * 512
        dst = torch.full((n + 512,), C.SENT_I, dtype=torch.int32, device=dev)
        dst[:n] = 0
        jobs.append(S.split_packed_job(Wd, dst, transpose=transpose))
        checks.append((W, Wd, dst, n))
    S.split(jobs)
    torch.cuda.synchronize()
    for W, _wd, dst, n in checks:
        assert (dst[n:] == C.SENT_I).all(), "guard behind the packed buffer"
        assert torch.equal(dst[:n].cpu(), C.pack_frag(W, transpose=transpose)), tuple(W.shape)


def test_split_49_jobs(S):
    """More than LGX_S8_BATCH_MAX jobs through the wrapper."""
    g = torch.Generator().manual_seed(49)
    jobs, checks = [], []
    for i in range(49):
        rows, cols = 1 + (37 * i) % 300, 1 + (11 * i) % 70
        x, xd = _split_src(rows, cols, g)
        dst = C.Out("s8", rows, cols, ld=C.rup(cols, 8) + 8, off=4, device=dev)
        jobs.append(S.split_job(xd, dst.ptr, dst.ld))
        checks.append((x, xd, dst))
    S.split(jobs)
    torch.cuda.synchronize()
    for x, _xd, dst in checks:
        assert dst.outside_intact() and torch.equal(dst.view().cpu(), C.pack_rows(x)), tuple(x.shape)


# ------------------------------------------------------------------ (h) lgx_s8_reduce
def test_reduce_paths(S):
    """The wave path (nsplit >= 64, rows * cols <= 4096) with rows > 1 and both pitches > cols, the
    vector path (flat, 16-B aligned) next to a job that is not aligned, the scalar path; nsplit 0 ..
    17; accumulate on every path; guards around every output; fp64 sums; a second launch bit-equal."""
    g = torch.Generator().manual_seed(9)
    specs = []  # (rows, cols, nsplit, ld_ws, ld_out, off)
    for acc in (0, 1):
        specs += [(3, 20, 65, 24, 23, 3, acc), (3, 20, 300, 24, 23, 0, acc), (1, 64, 64, 64, 64, 4, acc),
                  (1, 1000, 3, 1000, 1000, 4, acc), (1, 1000, 3, 1000, 1000, 1, acc), (2, 4096, 70, 4100, 4099, 4, acc)]
        for ns in (0, 1, 7, 8, 9, 16, 17):
            specs += [(1, 64, ns, 64, 64, 4, acc), (2, 9, ns, 11, 13, 3, acc)]
    jobs, checks = [], []
    for rows, cols, ns, ld_ws, ld_out, off, acc in specs:
        ws = torch.full((max(ns, 1), rows, ld_ws), NAN)
        ws[:, :, :cols] = torch.randn(max(ns, 1), rows, cols, generator=g)
        wsd = ws.to(dev)
        init = torch.randn(rows, cols, generator=g)
        out = C.Out("f32", rows, cols, ld=ld_out, off=off, device=dev, init=init if acc else None)
        jobs.append(S.ReduceArgs(ws=wsd.data_ptr(), stride=rows * ld_ws, ld_ws=ld_ws, out=out.ptr, ld_out=ld_out,
                                 rows=rows, cols=cols, nsplit=ns, accumulate=acc))
        ref = ws[:ns, :, :cols].double().sum(0) + (init.double() if acc else 0.0)
        checks.append((wsd, out, ref, init if acc else None, (rows, cols, ns, acc)))
    S.reduce(jobs)
    torch.cuda.synchronize()
    first = []
    for _ws, out, ref, init, what in checks:
        assert out.outside_intact(), what
        _within("REDUCE", str(what), out.values(), ref, 1e-5 * ref.abs() + 1e-5)
        first.append(out.flat.clone())
        if init is not None:
            out.view().copy_(init.to(dev))
    S.reduce(jobs)
    torch.cuda.synchronize()
    for f, (_ws, out, _ref, _init, what) in zip(first, checks):
        assert torch.equal(f, out.flat), (what, "a second launch differs")


# ------------------------------------------------------------------ (k) loud paths
def test_loud_paths(S):
    """Rejected before any launch: a negative return, the message named, the outputs untouched."""
    L = S.lib()
    P = C.Gemm("fwd", 20, 12, 40, bias=True)
    D = C.Gemm("dx", 20, 12, 40, use_delu=True)
    W = C.Gemm("dw", 20, 12, 40)
    outs = []

    def rejected(a, n, kind, msg):
        rc = L.lgx_s8_gemm_group(a, n, kind, None)
        assert rc < 0 and msg in L.lgx_s8_last_error(), (msg, rc, L.lgx_s8_last_error())

    J = Job(S, P)
    outs.append(J)
    J.args.lda = 56  # < round_up(40, 32)
    rejected(Ct.byref(J.args), 1, S.FWD, b"ROW operand A pitch")
    J = Job(S, P)
    outs.append(J)
    J.args.A += 4
    rejected(Ct.byref(J.args), 1, S.FWD, b"16-B aligned")
    J = Job(S, P)
    outs.append(J)
    J.args.ldc32 = 11
    rejected(Ct.byref(J.args), 1, S.FWD, b"ldc32 < N")
    J = Job(S, P)
    outs.append(J)
    J.args.epilogue |= S.EPI_HEAD_ACTOR
    rejected(Ct.byref(J.args), 1, S.FWD, b"lgx_s8_heads_fwd")
    J = Job(S, D)
    outs.append(J)
    J.args.act = None
    rejected(Ct.byref(J.args), 1, S.DX, b"ELU' epilogue")
    o, a, _keep = _dw_args(S, W, 1)
    a.C32 = None
    rejected(Ct.byref(a), 1, S.DW, b"DW needs C32")
    o2, a2, _keep2 = _dw_args(S, W, 1)
    a2.split = 1 << 30  # K offsets of the slabs would leave 32 bits
    rejected(Ct.byref(a2), 1, S.DW, b"split too large")
    jobs = [Job(S, P) for _ in range(21)]
    outs += jobs
    arr = (S.GemmArgs * 21)(*[j.args for j in jobs])
    rejected(arr, 21, S.FWD, b"LGX_S8_GROUP_MAX")
    torch.cuda.synchronize()
    assert all(j.untouched() for j in outs) and o.untouched() and o2.untouched()
    # lgx_s8_split
    x = torch.randn(4, 65).to(dev)
    dst = C.Out("s8", 4, 65, ld=80, off=4, device=dev)
    cs = C.Out("f32", 1, 65, device=dev)
    j = S.split_job(x, dst.ptr, dst.ld)
    j.colsum_ws = cs.ptr
    assert L.lgx_s8_split(Ct.byref(j), 1, None) < 0 and b"<= 64 columns" in L.lgx_s8_last_error()
    pk = torch.full((4 * 512,), C.SENT_I, dtype=torch.int32, device=dev)
    j = S.split_packed_job(x, pk)
    j.packed_steps = 2  # < ceil(65 / 32)
    assert L.lgx_s8_split(Ct.byref(j), 1, None) < 0 and b"packed_steps" in L.lgx_s8_last_error()
    torch.cuda.synchronize()
    assert dst.untouched() and cs.untouched() and (pk == C.SENT_I).all()


# ------------------------------------------------------------------ (i) lgx_s8_chain
# per chain: (widths, hidden layers' (C, C32), last layer's (C, C32), input as a column span, last C
# into a column span of a wider buffer)
FWD_CHAINS = (((256, 250, 70), (True, False), (True, True), False, False),
              ((29, 64, 20), (True, False), (True, True), True, True),
              ((20, 16), (False, False), (False, True), False, False),
              ((132, 128, 64, 32), (True, True), (True, False), True, False))
DX_CHAINS = (((32, 64, 128), (True, False), (True, True), True, False),
             ((20, 64), (True, False), (True, False), False, True))


def _chain_setup(S, spec, rows, packed, elu2, ci):
    """One chain on the device: its lgx_s8_chain_args, and per layer the chain's guarded outputs next
    to the same layer run as one grouped launch (on zero-padded hip_s8 buffers) and the fp64 chain."""
    widths, hid, lastm, span_in, span_out = spec
    g = C._gen(rows, ci, packed, elu2, len(widths))
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    # fragment-packed weights have zero pads by their format: the input's pads are the finite ones
    pad_in, pad_w = ("finite", "zero") if packed or (rows + ci) % 2 else ("zero", "finite")
    x = r(rows, widths[0])
    xin = C.Operand(x, "row", pad_in, extra=8 if span_in else 0, c0=8 if span_in else 0)
    tx, px = _up(xin)
    keep = [tx]
    n_l = len(widths) - 1
    c = S.ChainArgs(A=px, lda=xin.ld, rows=rows, nlayers=n_l)
    a_ref = S.to_s8_torch(x.to(dev))
    ref_layers, layers = [], []
    for l, (k, n) in enumerate(zip(widths[:-1], widths[1:])):
        last = l == n_l - 1
        W = r(n, k) * C.wscale(k)
        b = None if elu2 else r(n)
        elu = 2 if elu2 else int(not last)
        y = torch.nn.functional.elu(r(rows, n)) if elu2 else None
        wop = C.Operand(W, "row", pad_w)
        L = c.layers[l]
        L.K, L.N, L.elu = k, n, elu
        if packed:
            wp = C.pack_frag(W).to(dev)
            keep.append(wp)
            L.W, L.packed = wp.data_ptr(), 1
        else:
            tw, pw = _up(wop)
            keep.append(tw)
            L.W, L.ldw = pw, wop.ld
        bd = None
        if b is not None:
            bd = torch.cat([torch.full((3,), NAN), b, torch.full((3,), NAN)]).to(dev)
            keep.append(bd)
            L.bias = bd.data_ptr() + 12
        yop = None
        if elu2:
            yop = C.Operand(y, "act", "zero")
            ty, py = _up(yop)
            keep.append(ty)
            L.act, L.ld_act = py, yop.ld
        want_c, want_c32 = lastm if last else hid
        oc = oc32 = ocs = None
        if want_c:
            co = 40 if last and span_out else 0
            oc = C.Out("s8", rows, n, ld=co + C.rup(n, 8) + 8, off=4 + co, device=dev)
            L.C, L.ldc = oc.ptr, oc.ld
        if want_c32:
            oc32 = C.Out("f32", rows, n, ld=n + 3, off=3, device=dev)
            L.C32, L.ldc32 = oc32.ptr, oc32.ld
        if elu2:
            ocs = C.Out("f32", C.cdiv(rows, C.CHAIN_ROWS), n, ld=n, off=5, device=dev)
            L.colsum_ws = ocs.ptr
        # the same layer as one grouped launch
        rc, r32 = S.empty(rows, n, dev), torch.zeros(rows, n, device=dev)
        if elu2:
            wt = S.to_s8_torch(W.t().contiguous().to(dev))
            ya = S.to_s8_torch(y.to(dev))
            keep += [wt, ya]
            S.gemm_group([S.GemmArgs(A=a_ref.data_ptr(), lda=a_ref.shape[1], B=wt.data_ptr(), ldb=wt.shape[1], M=rows,
                                     N=n, K=k, epilogue=S.EPI_DELU, C=rc.data_ptr(), ldc=rc.shape[1], C32=r32.data_ptr(),
                                     ldc32=n, act=ya.data_ptr(), ld_act=ya.shape[1])], S.DX)
        else:
            wr = S.to_s8_torch(W.to(dev))
            keep.append(wr)
            S.gemm_group([S.GemmArgs(A=a_ref.data_ptr(), lda=a_ref.shape[1], B=wr.data_ptr(), ldb=wr.shape[1], M=rows,
                                     N=n, K=k, epilogue=S.EPI_BIAS | (S.EPI_ELU if elu else 0), C=rc.data_ptr(),
                                     ldc=rc.shape[1], C32=r32.data_ptr(), ldc32=n, bias=bd.data_ptr() + 12)], S.FWD)
        keep.append(a_ref)
        a_ref = rc
        ref_layers.append((wop.value, b, elu, None if yop is None else yop.value))
        layers.append((n, oc, oc32, ocs, rc, r32))
    return c, keep, layers, C.chain_ref(xin.value, ref_layers)


def _chain_verify(rows, layers, refs, name):
    for l, ((n, oc, oc32, ocs, rc, r32), (ref, e)) in enumerate(zip(layers, refs)):
        what = f"{name} layer {l}"
        if oc32 is not None:
            assert oc32.outside_intact(), (what, "fp32 guards")
            _within("CHAIN", what + " fp32", oc32.values(), ref, e)
            assert torch.equal(oc32.view(), r32), (what, "fp32 != grouped launch")
        if oc is not None:
            assert oc.outside_intact(), (what, "S8 guards")
            _within("CHAIN", what + " S8", oc.values(), ref, e + C.s8_extra(ref))
            assert torch.equal(oc.view(), rc[:rows, :C.rup(n, 8)]), (what, "S8 != grouped launch")
            if ocs is not None:
                assert ocs.outside_intact(), (what, "column-sum guards")
                sums, asum = C.colsums(oc.values(), C.CHAIN_ROWS)
                _within("CHAIN", what + " colsum", ocs.values(), sums, C.colsum_tol(asum, True))


@pytest.mark.parametrize("packed", [0, 1])
@pytest.mark.parametrize("rows", C.CHAIN_ROWS_CASES)
@pytest.mark.parametrize("which", ["all", 0, 1, 2, 3])
def test_chain_forward(S, which, rows, packed):
    """Forward chains against the fp64 chain at the per-layer bounds carried forward, and bit for bit
    against one grouped launch per layer: LGX_S8_CHAIN_MAX chains of all width classes in one launch,
    and each alone (its own width class); packed and row-layout weights; C only / C32 only / both;
    the input and the last output as column spans."""
    assert [s[0] for s in FWD_CHAINS] == list(C.CHAINS_FWD)
    specs = list(enumerate(FWD_CHAINS)) if which == "all" else [(which, FWD_CHAINS[which])]
    sets = [_chain_setup(S, spec, rows, packed, False, ci) for ci, spec in specs]
    S.chain([s[0] for s in sets])
    torch.cuda.synchronize()
    for (ci, spec), (_c, _keep, layers, refs) in zip(specs, sets):
        _chain_verify(rows, layers, refs, f"fwd {spec[0]} rows {rows} packed {packed}")


@pytest.mark.parametrize("packed", [0, 1])
def test_chain_input_gradients(S, packed):
    """Input-gradient chains (elu = 2) at rows 33: S8 outputs, and the 32-row column sums against fp64."""
    assert [s[0] for s in DX_CHAINS] == list(C.CHAINS_DX)
    sets = [_chain_setup(S, spec, 33, packed, True, ci) for ci, spec in enumerate(DX_CHAINS)]
    S.chain([s[0] for s in sets])
    torch.cuda.synchronize()
    for spec, (_c, _keep, layers, refs) in zip(DX_CHAINS, sets):
        _chain_verify(33, layers, refs, f"dx {spec[0]} packed {packed}")


# ------------------------------------------------------------------ (j) lgx_s8_dx_group_aux
@pytest.mark.parametrize("n", [0, 2])
def test_dx_group_aux(S, n):
    """The aux head in front of n DX problems: out, dp, de, de_s8, de_cs bit-equal to
    lgx_loss_heads_fused on the same arguments (B = 300: two aux blocks, the last partial), the GEMM
    outputs bit-equal to lgx_s8_gemm_group(DX) and within bound, guards intact."""
    from legged_gym_custom_amd.rsl_rl.modules import hip_mlp as H
    g = torch.Generator(device=dev).manual_seed(43)
    B, A, Ll, E = 300, 12, 20, 3
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    mu, value, std = r(B, A), r(B, 1), r(A).abs() + 0.5
    actions, old_logp, adv, tv, ret = r(B, A), r(B, 1), r(B, 1), r(B, 1), r(B, 1)
    old_mu, old_sigma = r(B, A), r(B, A).abs() + 0.5
    p_lat, a_lat, pred, t_est = r(B, Ll), r(B, Ll), r(B, E), r(B, E)
    seeds = torch.tensor([1.0, 1.3, -0.01, 0.05, 1.0], device=dev)
    nblk = (B + 255) // 256

    def bufs():
        z = lambda *s: torch.full(s, NAN, device=dev)  # noqa: E731
        f = lambda rows, cols, off: C.Out("f32", rows, cols, ld=cols, off=off, device=dev)  # noqa: E731
        return dict(ws=torch.zeros(19 * nblk, device=dev), wsa=torch.zeros(2 * nblk, device=dev), out=z(8),
                    dmu=z(B, A), dvalue=z(B), dstd=z(A), cnt=torch.zeros(1, dtype=torch.int32, device=dev),
                    cnta=torch.zeros(1, dtype=torch.int32, device=dev), out_aux=f(1, 2, 3), dp=f(B, Ll, 4),
                    de=f(B, E, 5), cs_e=f(nblk, E, 3), de8=C.Out("s8", B, E, ld=16, off=4, device=dev))

    def aux_args(o):
        x = H.AuxArgs(p=p_lat.data_ptr(), a=a_lat.data_ptr(), L=Ll, e=pred.data_ptr(), t=t_est.data_ptr(), E=E, B=B,
                      out=o["out_aux"].ptr, g=seeds.data_ptr() + 12, dp=o["dp"].ptr, de=o["de"].ptr,
                      ws=o["wsa"].data_ptr(), counter=o["cnta"].data_ptr(), ld_p=Ll)
        s8 = H.HeadsS8Args(de_s8=o["de8"].ptr, ld_de=o["de8"].ld, de_cs=o["cs_e"].ptr)
        return x, s8

    ref = bufs()
    x, s8 = aux_args(ref)
    dmu8, dv8 = S.empty(B, A, dev), S.empty(B, 1, dev)
    cs_mu, cs_v = torch.zeros(nblk, A, device=dev), torch.zeros(nblk, 1, device=dev)
    s8.dmu_s8, s8.ld_dmu, s8.dmu_cs = dmu8.data_ptr(), dmu8.shape[1], cs_mu.data_ptr()
    s8.dvalue_s8, s8.ld_dvalue, s8.dvalue_cs = dv8.data_ptr(), dv8.shape[1], cs_v.data_ptr()
    h = H.HeadArgs(mu=mu.data_ptr(), value=value.data_ptr(), std=std.data_ptr(), actions=actions.data_ptr(),
                   old_logp=old_logp.data_ptr(), adv=adv.data_ptr(), target_values=tv.data_ptr(),
                   returns=ret.data_ptr(), old_mu=old_mu.data_ptr(), old_sigma=old_sigma.data_ptr(), B=B, A=A,
                   clip=0.2, clipped_value=1, out=ref["out"].data_ptr(), g=seeds.data_ptr(),
                   dmu=ref["dmu"].data_ptr(), dvalue=ref["dvalue"].data_ptr(), dstd=ref["dstd"].data_ptr(),
                   ws=ref["ws"].data_ptr(), counter=ref["cnt"].data_ptr(), accumulate_dstd=0)
    H._check(H.lib().lgx_loss_heads_fused(H.C.byref(h), H.C.byref(x), H.C.byref(s8), H._stream()), "fused")
    got = bufs()
    x2, s82 = aux_args(got)
    probs = [C.Gemm("dx", M, N, K, pads=C.PADS[i], use_delu=True, add_cols=17)
             for i, (M, N, K) in enumerate(((129, 120, 65), (257, 136, 160))[:n])]
    jobs, single = [Job(S, P) for P in probs], [Job(S, P) for P in probs]
    S.dx_group_aux([J.args for J in jobs], x2, s82)
    if single:
        S.gemm_group([J.args for J in single], S.DX)
    torch.cuda.synchronize()
    for k in ("out_aux", "dp", "de", "de8", "cs_e"):
        assert got[k].outside_intact(), (k, "guards")
        assert not torch.isnan(got[k].values()).any(), k
        assert torch.equal(got[k].flat, ref[k].flat), (k, "!= lgx_loss_heads_fused")
    for i, (J, Js) in enumerate(zip(jobs, single)):
        assert _same(J, Js), (i, "!= lgx_s8_gemm_group(DX)")
        J.verify(f"aux[{i}] {J.P.M}x{J.P.N}x{J.P.K}")
