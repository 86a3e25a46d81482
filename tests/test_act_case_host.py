"""tests/act_case.py checked on the CPU before a kernel is compared with it: the segmented layout
and the span-packed first actor weight compute what the concatenated input and the plain weight do,
pack_ref round-trips, and every case of tests/test_gpu_s8_act_ref.py has a reference bound far
below its outputs."""
import pytest
import torch

import act_case as A


def _dequant_packed(W, N, steps, spans):
    hi, lo = A.unpack(A.pack_ref(W, N, steps, spans), N, steps)
    return hi, lo


@pytest.mark.parametrize("base", list(A.BASES))
def test_segmented_image_times_span_packed_weight_is_the_concatenated_product(base):
    case = A.fwd_case(base, 33)
    lay = A.layout(case["spec"])
    ref = A.forward_ref(case)
    W = case["W"]["actor"][0][0]
    N = W.shape[0]
    assert lay["width"] % 32 == 0 and all(p % 8 == 0 for p in lay["seg"])
    hi, lo = _dequant_packed(W, N, lay["width"] // 32, lay["spans"])
    Wp = (hi.double() + lo.double())[:N]
    assert Wp.shape[1] == ref["image"].shape[1] == lay["width"]
    assert ref["cat"].shape[1] == W.shape[1] < lay["width"]  # the gaps exist
    # rtol 1e-12 of each dot product's sum of magnitudes (the two sum in different orders, and an
    # output that cancels to 1e-6 has no 12 digits relative to itself)
    Wd = A.dequant(W)
    err = (ref["image"] @ Wp.t() - ref["cat"] @ Wd.t()).abs()
    assert (err <= 1e-12 * (ref["cat"].abs() @ Wd.abs().t())).all(), float(err.max())


@pytest.mark.parametrize("N,K", [(1, 1), (12, 128), (17, 33), (130, 20), (260, 100)])
def test_pack_ref_round_trips(N, K):
    g = torch.Generator().manual_seed(N * 1000 + K)
    W = torch.randn(N, K + 3, generator=g)  # row pitch > K
    steps = (K + 31) // 32
    hi, lo = _dequant_packed(W, N, steps, [(0, 0, K)])
    rh, rl = A.split_ref(W[:, :K])
    assert torch.equal(hi[:N, :K], rh.float()) and torch.equal(lo[:N, :K], rl.float())
    real = torch.zeros_like(hi, dtype=torch.bool)
    real[:N, :K] = True
    assert not hi[~real].any() and not lo[~real].any()
    assert A.pack_ref(W, N, steps, [(0, 0, K)]).numel() == (N + 15) // 16 * steps * 512


def test_pack_ref_spans_place_columns_and_leave_gaps_zero():
    s = A.spec("narrow", 1)
    lay = A.layout(s)
    W = torch.randn(20, A.dims(s)["actor"][0], generator=torch.Generator().manual_seed(5))
    hi, lo = _dequant_packed(W, 20, lay["width"] // 32, lay["spans"])
    rh, rl = A.split_ref(W)
    real = torch.zeros_like(hi, dtype=torch.bool)
    for c0, p0, w in lay["spans"]:
        assert torch.equal(hi[:20, p0:p0 + w], rh[:, c0:c0 + w].float())
        assert torch.equal(lo[:20, p0:p0 + w], rl[:, c0:c0 + w].float())
        real[:20, p0:p0 + w] = True
    assert (~real[:20]).any()  # non-empty gaps
    assert not hi[~real].any() and not lo[~real].any()


def _signal_ratio(x, e):
    """The smallest, over the columns, of the std over the rows divided by the column's largest bound."""
    e = e.max(dim=0).values
    return float((A.signal(x) / e).min())


def test_every_gpu_case_has_a_bound_far_below_its_outputs_and_a_signal_above_it():
    """Conditions on the drawn inputs, not measurements. For mu and value of every end-to-end case:
    bound < 1e-3 of the output's largest magnitude (a case that misses it gets a smaller wscale).
    That alone is met by the biases, so for every case marked `signal` also: the part of the output
    that depends on the inputs is at least A.SIGNAL times the bound. The cases not marked are the
    four-layer wide chains (act_case's docstring: compared layer by layer instead) and the encoder
    cases' own mu and value (the encoders are judged through their sel- case)."""
    n = 0
    for name, case, enc, signal in A.all_gpu_cases():
        r = A.forward_ref(case, enc)
        for out in ("mu", "value"):
            if name.startswith("sel-") and out == "value":
                continue  # the select launches judge mu (the encoder outputs) only
            scale = float(r[out].abs().max())
            bound = float(r["e_" + out].max())
            assert bound < 1e-3 * scale, (name, out, bound, scale)
            assert torch.isfinite(r[out]).all()
            if signal:
                ratio = _signal_ratio(r[out], r["e_" + out])
                assert ratio >= A.SIGNAL, (name, out, ratio)
        n += 1
    n_enc = 2 * len(A.ENC_B) * len(A.ENC_LENS) * 2
    assert n == 3 * len(A.FWD_B) + 2 * n_enc + len(A.HEAD_CASES) + len(A.PROBE_H) * len(A.ENC_B)


@pytest.mark.parametrize("base", list(A.BASES))
def test_layer_by_layer_cases_have_a_signal_far_above_the_one_layer_bound(base):
    for B in A.ENC_B:
        case = A.unshrunk_case(base, B)
        layers = case["W"]["actor"]
        x = A.forward_ref(case)["cat"]
        for n, (W, b) in enumerate(layers, 1):
            y, e = A.layer_ref(x, W, b, n < len(layers))
            assert torch.equal(y, A.forward_ref(A.cut_actor(case, n))["mu"])  # cut_actor is that chain
            assert float(e.max()) < 1e-3 * float(y.abs().max()), (base, B, n)
            assert _signal_ratio(y, e) >= 10 * A.SIGNAL, (base, B, n, _signal_ratio(y, e))
            x = y


def test_layouts_of_the_specs_are_what_the_gpu_file_relies_on():
    w = A.layout(A.spec("wide", 1))
    assert w["width"] == 640 and A.spec("wide", 1, c0=True)["est_c0"] % 4 == 0
    n = A.layout(A.spec("narrow", 1))
    assert n["width"] == 64 and n["seg"] == [0, 16, 24, 40] and A.spec("narrow", 1, c0=True)["est_c0"] == 8
    assert A.layout(A.spec("mid", 1))["width"] == 96
    for base in A.BASES:  # part sources narrower than their parts
        s = A.spec(base, 1)
        assert all(a < b for a, b in zip((s["nlat"], s["nscan"], s["nest"]), A.layout(s)["part_w"]))
