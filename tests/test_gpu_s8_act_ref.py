"""The fused rollout act kernel through its raw ABI (include/lgx_s8.h: lgx_s8_act, lgx_s8_act_pack;
hip_s8.ActArgs / ActLayer / ActPackArgs) against tests/act_case.py's fp64 reference, at the shapes
where the kernel's design can break: partial row blocks, an incomplete last group of four row
blocks, nets = 1 / 2, the in-kernel encoder chains, every layer-width class with a full and a
partial last tile, K no multiple of 8 and fewer K steps than the weight pipeline is deep.

Harness: every input is a strided view (ld > n, a first-row offset) into a NaN-filled buffer with
NaN rows behind row B - 1; every output is a view into a sentinel-filled buffer with guard columns
and guard rows. After each launch every guard element is still the sentinel and no output is NaN.
The forward comparisons first run one launch on NaN inputs, which leaves NaN in the LDS images of
the CUs the next launch most likely lands on: a layer that let image columns past its K, or rows
the block did not fill, reach a stored result would then return NaN and not a plausible number
(the pad columns of the packed weights are zero, and zero times a finite leftover hides it).

The bounds are act_case's (stated there, not tuned); every comparison prints max |err| / bound.
Which comparisons can see a subtle defect is stated there too: the four-layer wide chains end to end
cannot (their bound exceeds the input-dependent part of the output), so the wide layers are also
compared layer by layer, as two-layer probes, and through a selecting actor, where the signal is
10 to 4000 times the bound (asserted in tests/test_act_case_host.py)."""
import functools

import pytest
import torch

import act_case as A

pytestmark = pytest.mark.gpu
dev = "cuda:0"
SENT = -12345.0
NAN = float("nan")
ST_ROWS = {"obs_st": "obs", "priv_st": "priv_obs", "scan_st": "scan_obs", "critic_st": "critic_obs",
           "est_st": "est_obs"}
HEAD_OUT = ("actions", "mu_st", "sigma_st", "logp_st", "actions_copy")
SEED, ENV_OFFSET, STEP = 0x9E3779B97F4A7C15, 5, 7


@pytest.fixture(scope="module")
def S():
    from legged_gym_custom_amd.rsl_rl.modules import hip_s8
    hip_s8.lib()
    return hip_s8


class Buf:
    """A [rows, n] fp32 view (row pitch ld, first element at `off`) inside a flat buffer filled with
    `fill`, with guard columns (ld > n), guard rows behind it and `off` guard elements in front."""

    def __init__(self, rows, n, ld=None, off=0, fill=SENT, x=None):
        self.ld = n if ld is None else ld
        self.flat = torch.full((off + (rows + 2) * self.ld + 8,), fill, device=dev)
        self.geom = ((rows, n), (self.ld, 1), off)
        self.v = self.flat.as_strided(*self.geom)
        if x is not None:
            self.v.copy_(x)

    @property
    def ptr(self):
        return self.v.data_ptr()

    def guards_intact(self):
        g = torch.ones_like(self.flat, dtype=torch.bool)
        g.as_strided(*self.geom).fill_(False)
        return bool((self.flat[g] == SENT).all())

    def untouched(self):
        return bool((self.flat == SENT).all())


def _pack_job(S, Wd, dst, N, steps, spans):
    j = S.ActPackArgs(W=Wd.data_ptr(), ld=Wd.stride(0), dst=dst.data_ptr(), N=N, steps=steps, nspans=len(spans))
    for q, (c0, p0, w) in enumerate(spans):
        j.span_c0[q], j.span_p0[q], j.span_w[q] = c0, p0, w
    return j


def _act_layer(S, L):
    return S.ActLayer(W=L["Wp"].data_ptr(), ldw=L["steps"], b=L["b"].data_ptr(), K=L["K"], N=L["N"], elu=L["elu"])


def _padded(W):
    """W on the device with a row pitch > K and NaN in the pad columns."""
    Wd = torch.full((W.shape[0], W.shape[1] + 3), NAN, device=dev)
    Wd[:, :W.shape[1]] = W.to(dev)
    return Wd[:, :W.shape[1]]


def _device(S, case):
    """The case's weights on the device, act-packed by lgx_s8_act_pack (kept in the case)."""
    if "_dev" in case:
        return case["_dev"]
    lay = A.layout(case["spec"])
    dv, jobs = {"keep": []}, []
    for net in A.NETS:
        dv[net] = []
        layers = case["W"][net]
        for i, (W, b) in enumerate(layers):
            N, K = W.shape
            first = net == "actor" and i == 0
            spans = lay["spans"] if first else [(0, 0, K)]
            Kp = lay["width"] if first else K
            steps = (Kp + 31) // 32
            Wd = _padded(W)
            Wp = torch.full(((N + 15) // 16 * steps * 512,), -1, dtype=torch.int32, device=dev)
            jobs.append(_pack_job(S, Wd, Wp, N, steps, spans))
            dv["keep"].append(Wd)
            elu = i < len(layers) - 1 or (net == "actor" and case["spec"].get("actor_last_elu", False))
            dv[net].append(dict(Wp=Wp, b=b.to(dev), K=Kp, N=N, steps=steps, elu=int(elu)))
    S.act_pack(jobs)
    torch.cuda.synchronize()
    case["_dev"] = dv
    return dv


def run(S, case, enc=False, nets=0, head=None, tweak=None, raises=False, check=True):
    """One lgx_s8_act launch on the case. head: None, "eps" (the case's eps) or "philox". tweak(a):
    edits the argument block before the launch. raises: the launch must raise S8LibError and write
    nothing (returns the message). Returns {output name: CPU copy} and, under "_buf", the buffers."""
    s = case["spec"]
    lay, dv, B, nA = A.layout(s), _device(S, case), s["B"], s["A"]
    pads = dict(obs=(3, 1), priv_obs=(1, 3), scan_obs=(5, 2), critic_obs=(4, 4), est_obs=(2, 1))  # (ld - n, offset)
    ins = {k: Buf(B, case[k].shape[1], ld=case[k].shape[1] + p, off=o, fill=NAN, x=case[k])
           for k, (p, o) in pads.items()}
    parts = [Buf(B, p.shape[1], ld=p.shape[1] + 3, off=1 + q, fill=NAN, x=p) for q, p in enumerate(case["parts"])]
    outs = dict(mu=Buf(B, nA, ld=nA + 3, off=1), value=Buf(B, 1, off=3))
    for k, src in ST_ROWS.items():
        outs[k] = Buf(B, case[src].shape[1], off=2)
    for k in HEAD_OUT:
        outs[k] = Buf(B, 1 if k == "logp_st" else nA, off=2)
    keep = [ins, parts, outs]

    a = S.ActArgs()
    a.B, a.width, a.est_c0, a.nets = B, lay["width"], s["est_c0"], nets
    for i in range(4):
        a.seg[i] = lay["seg"][i]
    a.obs, a.ld_obs, a.n_obs = ins["obs"].ptr, ins["obs"].ld, s["n_obs"]
    a.priv_obs, a.ld_priv, a.n_priv_in = ins["priv_obs"].ptr, ins["priv_obs"].ld, s["n_priv_in"]
    a.scan_obs, a.ld_scan, a.n_scan_in = ins["scan_obs"].ptr, ins["scan_obs"].ld, s["n_scan_in"]
    a.critic_obs, a.ld_critic, a.n_critic_in = ins["critic_obs"].ptr, ins["critic_obs"].ld, s["n_critic_in"]
    a.est_obs, a.ld_est, a.n_est_obs = ins["est_obs"].ptr, ins["est_obs"].ld, s["nest"]

    def fill(dst, layers):
        for i, L in enumerate(layers):
            dst[i] = _act_layer(S, L)
        return len(layers)
    a.n_actor, a.n_critic = fill(a.actor, dv["actor"]), fill(a.critic, dv["critic"])
    if enc:
        a.n_est, a.n_scan, a.n_priv = fill(a.est, dv["est"]), fill(a.scan, dv["scan"]), fill(a.priv, dv["priv"])
    else:
        for q, p in enumerate(parts):
            a.part_src[q], a.part_ld[q], a.part_w[q] = p.ptr, p.ld, p.v.shape[1]
    a.mu, a.ld_mu, a.value = outs["mu"].ptr, outs["mu"].ld, outs["value"].ptr
    for k in ST_ROWS:
        setattr(a, k, outs[k].ptr)
    if head is not None:
        std = case["std"].to(dev)
        keep.append(std)
        a.std = std.data_ptr()
        for k in HEAD_OUT:
            setattr(a, k, outs[k].ptr)
        if head == "eps":
            eps = Buf(B, nA, off=1, fill=NAN, x=case["eps"])
            keep.append(eps)
            a.eps = eps.ptr
        else:
            step = torch.tensor([STEP], dtype=torch.int64, device=dev)
            keep.append(step)
            a.step_dev, a.seed, a.env_offset = step.data_ptr(), SEED, ENV_OFFSET
    if tweak is not None:
        tweak(a)
    if raises:
        with pytest.raises(S.S8LibError) as e:
            S.act(a)
        torch.cuda.synchronize()
        for k, b in outs.items():
            assert b.untouched(), f"{k} written by a rejected launch"
        return str(e.value)
    S.act(a)
    torch.cuda.synchronize()
    if check:
        for k, b in outs.items():
            assert b.guards_intact(), f"{k}: a guard element was written"
            assert not torch.isnan(b.flat).any(), f"{k}: NaN"
    res = {k: b.v.cpu() for k, b in outs.items()}
    res["_buf"] = outs
    return res


@functools.lru_cache(maxsize=None)
def _case(kind, *args):
    """(case, fp64 reference), computed once and shared by the tests. The tensors are never modified;
    _device() adds the "_dev" key (the packed weights on the device), which take_rows shares and
    select_actor / cut_actor drop."""
    case = getattr(A, kind + "_case")(*args)
    return case, A.forward_ref(case, enc=kind in ("enc", "sel"))


def _poison_lds(S):
    """One launch of the widest spec on NaN inputs (see the module docstring)."""
    case, _ = _case("fwd", "wide", 129)
    c = dict(case, parts=[torch.full_like(p, NAN) for p in case["parts"]])
    for k in A.ROW_KEYS:
        c[k] = torch.full_like(case[k], NAN)
    run(S, c, check=False)


def _ratio(label, got, ref, bound):
    r = float(((got.double() - ref).abs() / bound).max())
    print(f"{label}: max |err| / bound = {r:.3f}")
    return r


def _storage_rows_equal_inputs(out, case, names=tuple(ST_ROWS)):
    for k in names:
        assert torch.equal(out[k], case[ST_ROWS[k]]), k


# ---------------------------------------------------------------- 1. the packed weights
PACK_SHAPES = [(1, 1), (12, 128), (17, 33), (130, 20), (260, 100), (512, 640)]


def test_act_pack_bit_for_bit(S):
    g = torch.Generator().manual_seed(11)
    items = [(N, K, (K + 31) // 32, [(0, 0, K)]) for N, K in PACK_SHAPES]
    for base in ("wide", "narrow"):  # the first actor layer's four spans
        s = A.spec(base, 1)
        lay = A.layout(s)
        items.append((s["actor"][0], A.dims(s)["actor"][0], lay["width"] // 32, lay["spans"]))
    items += [(1 + i % 19, 1 + (7 * i) % 70, (1 + (7 * i) % 70 + 31) // 32, None) for i in range(S.BATCH_MAX)]
    assert len(items) > S.BATCH_MAX  # the wrapper sends more than one chunk
    jobs, todo = [], []
    for N, K, steps, spans in items:
        spans = [(0, 0, K)] if spans is None else spans
        W = torch.randn(N, K, generator=g) * 10.0 ** (torch.rand(K, generator=g) * 4 - 3)
        Wd = _padded(W)
        size = (N + 15) // 16 * steps * 512
        dst = torch.full((size + 512,), -1, dtype=torch.int32, device=dev)  # 0xFF bytes; 2 KB behind as a guard
        jobs.append(_pack_job(S, Wd, dst, N, steps, spans))
        todo.append((W, Wd, dst, N, steps, spans, size))
    S.act_pack(jobs)
    torch.cuda.synchronize()
    for W, _, dst, N, steps, spans, size in todo:
        got = dst.cpu()
        assert torch.equal(got[:size], A.pack_ref(W, N, steps, spans)), (N, W.shape[1], steps)
        assert (got[size:] == -1).all(), (N, W.shape[1])


# ---------------------------------------------------------------- 2. part-source mode
@pytest.mark.parametrize("B", A.FWD_B)
@pytest.mark.parametrize("base", list(A.BASES))
def test_forward_part_sources_against_fp64(S, base, B):
    case, ref = _case("fwd", base, B)
    _poison_lds(S)
    out = run(S, case)
    r = [_ratio(f"fwd {base} B={B} {k}", out[k].reshape(ref[k].shape), ref[k], ref["e_" + k]) for k in ("mu", "value")]
    _storage_rows_equal_inputs(out, case)
    for k in HEAD_OUT:
        assert out["_buf"][k].untouched(), k
    assert max(r) <= 1.0, r


# ---------------------------------------------------------------- 3. the in-kernel encoders
@pytest.mark.parametrize("c0", (False, True))
@pytest.mark.parametrize("lens", A.ENC_LENS, ids=lambda t: "est%d-scan%d-priv%d" % t)
@pytest.mark.parametrize("B", A.ENC_B)
@pytest.mark.parametrize("base", ("wide", "narrow"))
def test_in_kernel_encoders_against_fp64(S, base, B, lens, c0):
    case, ref = _case("enc", base, B, lens, c0)
    assert (case["spec"]["est_c0"] > 0) == c0
    _poison_lds(S)
    out = run(S, case, enc=True)
    tag = f"enc {base} B={B} {lens} c0={case['spec']['est_c0']}"
    r = [_ratio(f"{tag} {k}", out[k].reshape(ref[k].shape), ref[k], ref["e_" + k]) for k in ("mu", "value")]
    _storage_rows_equal_inputs(out, case)
    # the encoder outputs never leave LDS: a one-layer actor that selects the latent columns, on a
    # draw of the same spec whose encoder weights keep the signal (act_case.SEL_WSCALE)
    sel, rs = _case("sel", base, B, lens, c0)
    assert torch.equal(rs["mu"], torch.cat([rs["lat"], rs["scan"], rs["est"]], dim=1))
    _poison_lds(S)
    so = run(S, sel, enc=True)
    r.append(_ratio(f"{tag} encoder outputs", so["mu"], rs["mu"], rs["e_mu"]))
    assert max(r) <= 1.0, r


# ------------------------------------------------- 2b / 3b. where the wide layers' signal survives
def _layer_by_layer(S, case, x, tag, enc=False):
    """The actor cut after 1, 2, ... layers (the cut layer keeps its ELU and writes mu): layer n at its
    one-layer bound on x, the kernel's own output of the chain cut after n - 1 (first: the inputs)."""
    layers = case["W"]["actor"]
    r = []
    for n, (W, b) in enumerate(layers, 1):
        cut = A.cut_actor(case, n)
        assert cut["spec"]["actor_last_elu"] == (n < len(layers))
        _poison_lds(S)
        got = run(S, cut, enc=enc)["mu"]
        y, e = A.layer_ref(x, W, b, n < len(layers))
        r.append(_ratio(f"{tag} layer {n} ({W.shape[1]} -> {W.shape[0]})", got, y, e))
        x = got
    return r, got


@pytest.mark.parametrize("B", A.ENC_B)
@pytest.mark.parametrize("base", list(A.BASES))
def test_actor_layer_by_layer_on_unshrunk_weights(S, base, B):
    case = A.unshrunk_case(base, B)
    r, mu = _layer_by_layer(S, case, A.forward_ref(case)["cat"], f"layers {base} B={B}")
    assert torch.equal(mu, run(S, case)["mu"])  # the last cut is the whole chain
    assert max(r) <= 1.0, r


@pytest.mark.parametrize("lens", A.ENC_LENS, ids=lambda t: "est%d-scan%d-priv%d" % t)
@pytest.mark.parametrize("base", ("wide", "narrow"))
def test_actor_layer_by_layer_behind_the_in_kernel_encoders(S, base, lens):
    """The same with n_est > 0: the first layer's input is [obs | the kernel's own encoder outputs]."""
    case = A.enc_case(base, 33, lens, True, wscale=1.0)
    latents = run(S, A.select_actor(case), enc=True)["mu"]
    x = torch.cat([case["obs"].double(), latents.double()], dim=1)
    r, _ = _layer_by_layer(S, case, x, f"layers behind encoders {base} {lens}", enc=True)
    assert max(r) <= 1.0, r


@pytest.mark.parametrize("B", A.ENC_B)
@pytest.mark.parametrize("h", A.PROBE_H)
def test_two_layer_wide_probes_against_fp64(S, h, B):
    case, ref = _case("probe", h, B)
    _poison_lds(S)
    out = run(S, case)
    r = [_ratio(f"probe h={h} B={B} {k}", out[k].reshape(ref[k].shape), ref[k], ref["e_" + k]) for k in ("mu", "value")]
    assert max(r) <= 1.0, r


# ---------------------------------------------------------------- 4. nets
@pytest.mark.parametrize("B", (33, 129))
@pytest.mark.parametrize("base", ("wide", "narrow"))
def test_nets_1_and_2_are_the_two_halves_of_nets_0(S, base, B):
    case, _ = _case("fwd", base, B)
    both, actor, critic = (run(S, case, nets=n) for n in (0, 1, 2))
    assert actor["_buf"]["value"].untouched() and actor["_buf"]["critic_st"].untouched()
    assert critic["_buf"]["mu"].untouched()
    for k in ("obs_st", "priv_st", "scan_st", "est_st"):
        assert critic["_buf"][k].untouched(), k
    assert torch.equal(actor["mu"], both["mu"]) and torch.equal(critic["value"], both["value"])
    _storage_rows_equal_inputs(actor, case, ("obs_st", "priv_st", "scan_st", "est_st"))
    _storage_rows_equal_inputs(critic, case, ("critic_st",))


# ---------------------------------------------------------------- 5. the act head
@pytest.mark.parametrize("base,nA", A.HEAD_CASES)
def test_act_head_against_fp64(S, base, nA):
    """"Within 2 ulp of mu_st + std * eps" is read at the larger of |mu_st + std * eps| and |std * eps|:
    the fp32 product and the add round once each, half an ulp of each. Where mu_st and std * eps cancel,
    the product's half ulp is many ulp of the small sum (up to 200 in these cases, printed below), so
    the ulp of the sum alone would fail a correct kernel."""
    case, ref = _case("head", base, nA)
    B = case["spec"]["B"]
    plain = run(S, case)
    out = run(S, case, head="eps")
    assert out["_buf"]["mu"].untouched()  # with the head, mu is not written
    assert torch.equal(out["value"], plain["value"])
    assert torch.equal(out["mu_st"], plain["mu"])
    assert torch.equal(out["sigma_st"], case["std"].expand(B, nA))
    assert torch.equal(out["actions"], out["actions_copy"])
    mu, std, eps = out["mu_st"].double(), case["std"].double(), case["eps"].double()
    exact = mu + std * eps
    err = (out["actions"].double() - exact).abs()
    ulp = A.ulp32(torch.maximum(exact.abs(), (std * eps).abs()))
    print(f"head {base} A={nA} actions: max |err| / ulp = {float((err / ulp).max()):.3f}"
          f" (in ulp of the sum itself: {float((err / A.ulp32(exact)).max()):.3f})")
    r = _ratio(f"head {base} A={nA} actions vs the reference's", out["actions"], ref["actions"], ref["e_actions"])
    assert (err <= 2 * ulp).all()
    assert r <= 1.0
    lp = out["logp_st"][:, 0].double()
    torch.testing.assert_close(lp, A.logp_ref(out["actions"], out["mu_st"], case["std"]), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lp, ref["logp"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("base,nA", A.HEAD_CASES)
def test_act_head_philox_draw_matches_act_head_kernel(S, base, nA):
    from legged_gym_custom_amd.rsl_rl.modules import hip_mlp as H
    case, _ = _case("head", base, nA)
    B = case["spec"]["B"]
    plain = run(S, case)
    out = run(S, case, head="philox")
    want = {k: torch.full((B, 1 if k == "logp_st" else nA), SENT, device=dev) for k in HEAD_OUT}
    step = torch.tensor([STEP], dtype=torch.int64, device=dev)
    H.act_head(plain["mu"].to(dev), case["std"].to(dev), None, want["actions"], want["mu_st"], want["sigma_st"],
               want["logp_st"], actions_copy=want["actions_copy"], noise=(SEED, step, ENV_OFFSET))
    torch.cuda.synchronize()
    for k in HEAD_OUT:
        assert torch.equal(out[k], want[k].cpu()), k
    assert (out["actions"] != out["mu_st"]).any()


# ---------------------------------------------------------------- 6. rows and repeats
@pytest.mark.parametrize("base", ("wide", "narrow"))
def test_rows_are_independent_and_launches_repeat(S, base):
    case, _ = _case("fwd", base, 129)
    full, again = run(S, case), run(S, case)
    for k in ("mu", "value") + tuple(ST_ROWS):
        assert torch.equal(full[k], again[k]), k
    for i in (0, 31, 32, 128):
        one = run(S, A.take_rows(case, [i]))
        assert torch.equal(one["mu"][0], full["mu"][i]) and torch.equal(one["value"][0], full["value"][i]), i


# ---------------------------------------------------------------- 7. loud paths
def _fresh(base, B=33, c0=False, enc_len=None, **kw):
    return A.build(A.spec(base, B, c0=c0, enc_len=enc_len, **kw), torch.Generator().manual_seed(77))


def test_a_layer_wider_than_512_columns_is_rejected(S):
    # a last actor layer, no head, ld_mu >= N: columns 512.. would never be written
    msg = run(S, _fresh("narrow", A=600), raises=True)
    assert "512" in msg, msg
    # an encoder's last layer into a part wider than 512 (actor input: 8 + 520 + 8 + 8 = 544 columns)
    wide_part = dict(A.NARROW, n_obs=8, est_K=8, nlat=520, nscan=8, nest=8)
    assert A.layout(A.spec(wide_part, 1))["width"] == 544
    msg = run(S, _fresh(wide_part, enc_len=(1, 1, 1)), enc=True, raises=True)
    assert "512" in msg, msg
    # and a hidden layer (the old check)
    assert "actor chain" in run(S, _fresh("narrow", actor=[20, 520]), raises=True)


def test_bad_arguments_are_rejected_and_nothing_is_written(S):
    case = _fresh("narrow")
    run(S, case)  # the case itself is fine
    assert "multiple of 32" in run(S, _fresh("narrow", n_critic_in=40), raises=True)  # the critic's width

    def misaligned(a):
        a.critic_obs += 4
    assert "aligned" in run(S, case, tweak=misaligned, raises=True)
    assert "nets" in run(S, case, nets=3, raises=True)
    assert "act head" in run(S, _fresh("narrow", A=17), head="eps", raises=True)
    run(S, _fresh("narrow", A=17))  # fine without the head

    def chains_without_estimator(a):
        a.scan[0] = _act_layer(S, case["_dev"]["scan"][0])
        a.n_scan = 1
    assert "encoders" in run(S, case, tweak=chains_without_estimator, raises=True)

    def part_too_wide(a):
        a.part_w[0] = A.layout(case["spec"])["part_w"][0] + 4
        a.part_ld[0] = a.part_w[0] + 4
    assert "part sources" in run(S, case, tweak=part_too_wide, raises=True)
