"""Shared by tests/test_act_case_host.py and tests/test_gpu_s8_act_ref.py: the rollout's act networks
(include/lgx_s8.h lgx_s8_act / lgx_s8_act_pack) restated in plain torch on the CPU, in fp64, with no
GPU and no PPO. A spec is a dict of sizes; build() draws a case from a seeded CPU generator;
forward_ref() is the mathematics the kernel is compared with, pack_ref() the packed weight format.

Spec fields: B, n_obs, est_c0, est_K (the estimator reads obs columns [est_c0, est_c0 + est_K)),
n_priv_in, n_scan_in, n_critic_in, the hidden lists actor / critic / est / scan / priv, the latent
widths nlat / nscan / nest, A, and wscale (a factor on every weight matrix, not on the biases).

Bounds (stated, not measured). A layer y = act(x W^T + b) on the kernel's 3 x bf16 products with
fp32 accumulation is off by at most 1.5 * (2e-5 * |x| |W|^T + 1e-6) + 1e-6 per element: the
tolerance tests/test_gpu_s8.py states for the same product (_bound, with its ELU factor). An input
error e passes a layer as e |W|^T, and through ELU unchanged (ELU' <= 1). forward_ref carries that
bound next to every activation.

What the bound can see. With weights U(+-1/sqrt(fan_in)) the worst-case term e |W|^T grows by about
sqrt(fan_in) / 2 per layer, the part of an output that depends on the inputs by about 0.6 at best:
each layer of depth costs the comparison a factor of about sqrt(fan_in). The issue's condition
"bound < 1e-3 of the output's largest magnitude" (tests/test_act_case_host.py) is met by shrinking
the deep specs' weight matrices (wscale); the biases, of magnitude 0.25 to 0.5, then carry the
outputs, and in the four-layer "wide" chains the input-dependent part of mu and value falls BELOW
the bound: those end-to-end comparisons see NaN, guards, rows and the last layer, not a subtle
defect in a first layer. So every wide layer is also compared where its signal is at least 10 times
its bound, and the host file asserts that ratio (SIGNAL):
* the actor layer by layer on unshrunk weights (unshrunk_case, cut_actor): the chain cut after l
  layers keeps its ELU and writes mu, and layer l is judged at its one-layer bound on the kernel's
  own output of the chain cut after l - 1 (signal 500 to 4000 times the bound);
* the critic, and the actor's first layer from every hidden width, as two-layer chains 736 -> h -> 1
  and 640 -> h -> 12, h = 512, 260, 130, at wscale 0.25 (probe_case; 55 to 130 times);
* the encoders through select_actor on encoder weights at wscale 0.5 (15 to 50 times).
The narrow and mid cases keep 10 times the bound end to end (asserted as well)."""
import math

import torch
import torch.nn.functional as F

NETS = ("est", "scan", "priv", "actor", "critic")
LOG_SQRT_2PI = 0.91893853320467274178

# "wide": the actor input fills LGX_S8_ACT_MAXIN (640); 512 is a full last tile of the 4-tile width
# class, 260 a partial one, 130 a partial one of the 2-tile class; K steps 20, 16, 9, 5 and 23.
WIDE = dict(n_obs=530, est_K=50, n_priv_in=37, n_scan_in=132, n_critic_in=736, actor=[512, 260, 130],
            critic=[512, 260, 130], est=[], scan=[], priv=[], nlat=29, nscan=33, nest=9, A=12, wscale=0.125)
# "narrow": one-tile-class layers with partial tiles, K = 20 and 17 (no multiple of 8), K steps 2, 1, 4;
# n_obs is no multiple of 8, so the gaps between the parts are not empty.
NARROW = dict(n_obs=13, est_K=5, n_priv_in=20, n_scan_in=132, n_critic_in=32, actor=[20, 100], critic=[17],
              est=[], scan=[], priv=[], nlat=5, nscan=9, nest=3, A=5, wscale=0.5)
# "mid": what the two above leave out: full last tiles in the 1- and 2-tile classes (32, 256), 3 K steps.
MID = dict(NARROW, n_obs=45, est_K=9, actor=[32, 256], critic=[64], n_critic_in=64, wscale=0.25)
BASES = {"wide": WIDE, "narrow": NARROW, "mid": MID}
# encoder hidden lists by chain length: 256 = LGX_S8_ACT_MAXENC (full last tile, 2-tile class), 250 a
# partial one and no multiple of 8 as the next K, 70 = 3 K steps
ENC_HIDDEN = {1: [], 2: [256], 3: [250, 70]}


def spec(base, B, c0=False, enc_len=None, **kw):
    """A spec from a base: c0 -> est_c0 = n_obs - est_K (else 0); enc_len = chain lengths of
    (est, scan, priv)."""
    s = dict(BASES[base] if isinstance(base, str) else base, B=B)
    s.update(kw)
    s["est_c0"] = s["n_obs"] - s["est_K"] if c0 else 0
    if enc_len is not None:
        for net, n in zip(("est", "scan", "priv"), enc_len):
            s[net] = list(ENC_HIDDEN[n])
        s["wscale"] = 0.125  # up to three more layers in front of the actor
    return s


def _r8(x):
    return (x + 7) // 8 * 8


def layout(s):
    """The actor input's segmented layout as rsl_rl/algorithms/s8_act.py builds it: parts at _r8
    boundaries, the width rounded up to 32; spans = (logical column, packed column, width)."""
    nobs, nlat, nscan, nest = s["n_obs"], s["nlat"], s["nscan"], s["nest"]
    P0 = _r8(nobs)
    P1 = P0 + _r8(nlat)
    P2 = P1 + _r8(nscan)
    width = (P2 + _r8(nest) + 31) // 32 * 32
    spans = [(0, 0, nobs), (nobs, P0, nlat), (nobs + nlat, P1, nscan), (nobs + nlat + nscan, P2, nest)]
    return dict(seg=[0, P0, P1, P2], width=width, spans=spans, part_w=[P1 - P0, P2 - P1, width - P2])


def dims(s):
    """{net: [input width, hidden..., output width]}."""
    return {"est": [s["est_K"]] + s["est"] + [s["nest"]],
            "scan": [s["n_scan_in"]] + s["scan"] + [s["nscan"]],
            "priv": [s["n_priv_in"]] + s["priv"] + [s["nlat"]],
            "actor": [s["n_obs"] + s["nlat"] + s["nscan"] + s["nest"]] + s["actor"] + [s["A"]],
            "critic": [s["n_critic_in"]] + s["critic"] + [1]}


def build(s, gen):
    """A case: fp32 weights U(+-1/sqrt(fan_in)) * wscale, biases of either sign with magnitude in
    (0.25, 0.5) (no output is near zero by the luck of one draw), standard normal inputs, part
    sources (the encoder outputs of the part-source mode) and eps, std in (0.7, 1.3)."""
    def u(*shape, bound):
        return (torch.rand(*shape, generator=gen) * 2 - 1) * bound

    def n(*shape):
        return torch.randn(*shape, generator=gen)
    W = {}
    for net in NETS:
        d = dims(s)[net]
        W[net] = []
        for i in range(len(d) - 1):
            bias = u(d[i + 1], bound=1.0).sign() * (u(d[i + 1], bound=0.125) + 0.375)
            W[net].append((u(d[i + 1], d[i], bound=s["wscale"] / math.sqrt(d[i])), bias))
    B = s["B"]
    return dict(spec=s, W=W, obs=n(B, s["n_obs"]), priv_obs=n(B, s["n_priv_in"]), scan_obs=n(B, s["n_scan_in"]),
                critic_obs=n(B, s["n_critic_in"]), est_obs=n(B, s["nest"]),
                parts=[n(B, s["nlat"]), n(B, s["nscan"]), n(B, s["nest"])],
                std=torch.rand(s["A"], generator=gen) * 0.6 + 0.7, eps=n(B, s["A"]))


ROW_KEYS = ("obs", "priv_obs", "scan_obs", "critic_obs", "est_obs", "eps")


def take_rows(case, idx):
    """The case of rows idx alone (same weights; a shallow copy, so caches kept in the case stay shared)."""
    c = dict(case, spec=dict(case["spec"], B=len(idx)))
    for k in ROW_KEYS:
        c[k] = case[k][idx].clone()
    c["parts"] = [p[idx].clone() for p in case["parts"]]
    return c


def _with_actor(case, layers, hidden, last_elu=False):
    """The same case with another actor chain (std and eps redrawn for its width)."""
    nA = layers[-1][0].shape[0]
    c = {k: v for k, v in case.items() if not k.startswith("_")}
    c["spec"] = dict(case["spec"], actor=list(hidden), A=nA, actor_last_elu=last_elu)
    c["W"] = dict(case["W"], actor=list(layers))
    g = torch.Generator().manual_seed(nA)
    c["std"] = torch.rand(nA, generator=g) * 0.6 + 0.7
    c["eps"] = torch.randn(case["spec"]["B"], nA, generator=g)
    return c


def select_actor(case):
    """The same case with a one-layer actor whose weight is a 0/1 selection of the latent columns
    [priv latent | scan latent | est] and whose bias is zero: mu is then the encoder outputs."""
    s = case["spec"]
    nl = s["nlat"] + s["nscan"] + s["nest"]
    Wsel = torch.zeros(nl, s["n_obs"] + nl)
    Wsel[torch.arange(nl), s["n_obs"] + torch.arange(nl)] = 1.0
    return _with_actor(case, [(Wsel, torch.zeros(nl))], [])


def cut_actor(case, n):
    """The same case with the actor cut after its first n layers. A cut inside the chain keeps the
    layer's ELU (spec actor_last_elu; the ABI's per-layer flag), so mu is the activation that the
    full chain holds in LDS after layer n."""
    layers = case["W"]["actor"]
    return _with_actor(case, layers[:n], case["spec"]["actor"][:n - 1], last_elu=n < len(layers))


def layer_ref(x, W, b, elu):
    """One layer in fp64 on the given input (taken as exact) and its one-layer bound."""
    y, e = _chain(x.double(), None, [(W, b)])
    return (F.elu(y) if elu else y), e


def split_ref(x):
    """hi = bf16(x), lo = bf16(x - hi), torch's (round-to-nearest-even) bf16: hip_s8.to_s8_torch's."""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi, lo


def dequant(W):
    hi, lo = split_ref(W)
    return hi.double() + lo.double()


def pack_ref(W, N, steps, spans):
    """The act-packed buffer (int32, ceil(N / 16) * steps * 512 words) of fp32 W [N, >= K]: tile t,
    step s at byte (t * steps + s) * 2048, 1 KB of hi then 1 KB of lo, lane l = row 16 t + (l & 15),
    columns 32 s + 8 (l >> 4) .. + 7; zero where the row >= N or the column lies in no span."""
    T = (N + 15) // 16
    P = torch.zeros(16 * T, 32 * steps, dtype=torch.float32)
    for c0, p0, w in spans:
        P[:N, p0:p0 + w] = W[:N, c0:c0 + w]
    planes = []
    for x in split_ref(P):
        x = x.view(T, 16, steps, 4, 8).permute(0, 2, 3, 1, 4)  # [t, s, g, c, e]: lane = 16 g + c
        planes.append(x.reshape(T, steps, 64, 8))
    return torch.stack(planes, dim=2).contiguous().view(torch.int32).reshape(-1)


def unpack(buf, N, steps):
    """(hi, lo) fp32 [16 ceil(N / 16), 32 steps] of an act-packed buffer: pack_ref's inverse."""
    T = (N + 15) // 16
    b = buf.reshape(-1).view(torch.bfloat16).view(T, steps, 2, 4, 16, 8).float()
    b = b.permute(2, 0, 4, 1, 3, 5).reshape(2, 16 * T, 32 * steps)
    return b[0], b[1]


def _chain(x, e, layers):
    """fp64 [Linear, ELU]* Linear on the dequantised weights, with the elementwise bound (e: the
    input's; None = exact)."""
    e = torch.zeros_like(x) if e is None else e
    for i, (W, b) in enumerate(layers):
        Wd = dequant(W)
        Wa = Wd.abs().t()
        e = e @ Wa + 1.5 * (2e-5 * (x.abs() @ Wa) + 1e-6) + 1e-6
        x = x @ Wd.t() + b.double()
        if i < len(layers) - 1:
            x = F.elu(x)
    return x, e


def forward_ref(case, enc=False):
    """The act networks in fp64. enc: the encoders run (the kernel's n_est > 0 mode); else the actor's
    parts 1..3 are case["parts"] (exact inputs). Returns mu, value, lat / scan / est (the encoder
    outputs), actions (= mu + std * eps), each with its bound e_<name>, logp, cat (the actor input as
    the concatenation, which the actor is run on) and image (the same in the segmented layout)."""
    s, W = case["spec"], case["W"]
    lay = layout(s)
    obs = case["obs"].double()
    if enc:
        c0 = s["est_c0"]
        est, e_est = _chain(obs[:, c0:c0 + s["est_K"]], None, W["est"])
        scan, e_scan = _chain(case["scan_obs"].double(), None, W["scan"])
        lat, e_lat = _chain(case["priv_obs"].double(), None, W["priv"])
    else:
        lat, scan, est = (p.double() for p in case["parts"])
        e_lat, e_scan, e_est = (torch.zeros_like(p) for p in (lat, scan, est))
    parts = [obs, lat, scan, est]
    cat = torch.cat(parts, dim=1)
    e_cat = torch.cat([torch.zeros_like(obs), e_lat, e_scan, e_est], dim=1)
    image = torch.zeros(s["B"], lay["width"], dtype=torch.float64)
    for p, (_, p0, w) in zip(parts, lay["spans"]):
        image[:, p0:p0 + w] = p
    mu, e_mu = _chain(cat, e_cat, W["actor"])
    if s.get("actor_last_elu"):
        mu = F.elu(mu)
    value, e_value = _chain(case["critic_obs"].double(), None, W["critic"])
    std, eps = case["std"].double(), case["eps"].double()
    actions = mu + std * eps
    # the fp32 product and the add round once each
    e_actions = e_mu + 2.0 ** -23 * (mu.abs() + (std * eps).abs())
    logp = (-0.5 * eps * eps - std.log() - LOG_SQRT_2PI).sum(dim=1)
    return dict(mu=mu, e_mu=e_mu, value=value[:, 0], e_value=e_value[:, 0], lat=lat, e_lat=e_lat, scan=scan,
                e_scan=e_scan, est=est, e_est=e_est, actions=actions, e_actions=e_actions, logp=logp, cat=cat,
                image=image)


def logp_ref(actions, mu, std):
    """fp64 Normal(mu, std) log-prob of the given actions, summed over the action dimension."""
    a, m, sd = actions.double(), mu.double(), std.double()
    return (-((a - m) ** 2) / (2 * sd * sd) - sd.log() - LOG_SQRT_2PI).sum(dim=1)


def ulp32(x):
    """The fp32 spacing at |x| (fp64 tensor; normal range)."""
    _, ex = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), ex - 24)


# ---- the cases of tests/test_gpu_s8_act_ref.py (tests/test_act_case_host.py checks each one's bound)
FWD_B = (1, 31, 32, 33, 129)
ENC_B = (33, 129)
ENC_LENS = ((1, 2, 3), (2, 3, 1), (3, 1, 2))  # chain lengths of (est, scan, priv)
HEAD_CASES = (("narrow", 1), ("narrow", 5), ("wide", 12), ("narrow", 16))


def fwd_case(base, B):
    return build(spec(base, B), torch.Generator().manual_seed(1000 + B))


SEL_WSCALE = 0.5


def enc_case(base, B, lens, c0, wscale=None):
    """wscale None: the spec's shrunk weights; SEL_WSCALE: the draw that select_actor is run on."""
    s = spec(base, B, c0=c0, enc_len=lens)
    if wscale is not None:
        s["wscale"] = wscale
    return build(s, torch.Generator().manual_seed(2000 + B + 7 * lens[0] + c0))


def unshrunk_case(base, B):
    """The spec at wscale = 1: for the layer-by-layer comparison (cut_actor)."""
    return build(spec(base, B, wscale=1.0), torch.Generator().manual_seed(4000 + B))


PROBE_H = (512, 260, 130)


def probe_case(h, B):
    """The wide inputs with the two-layer critic 736 -> h -> 1 and actor 640 -> h -> 12."""
    return build(spec("wide", B, actor=[h], critic=[h], wscale=0.25), torch.Generator().manual_seed(5000 + h + B))


def sel_case(base, B, lens, c0):
    return select_actor(enc_case(base, B, lens, c0, wscale=SEL_WSCALE))


SIGNAL = 10.0


def signal(x):
    """The input-dependent part of an output: its standard deviation over the rows, per column."""
    return x.std(dim=0)


def head_case(base, A, B=33):
    return build(spec(base, B, A=A), torch.Generator().manual_seed(3000 + A))


def all_gpu_cases():
    """(name, case, enc, signal) of every end-to-end comparison the GPU file makes; signal: the
    input-dependent part of mu and value is at least SIGNAL times the bound (module docstring)."""
    for base in BASES:
        for B in FWD_B:
            yield f"fwd-{base}-{B}", fwd_case(base, B), False, base != "wide" and B > 1
    for base in ("wide", "narrow"):
        for B in ENC_B:
            for lens in ENC_LENS:
                for c0 in (False, True):
                    yield f"enc-{base}-{B}-{lens}-{int(c0)}", enc_case(base, B, lens, c0), True, False
                    yield f"sel-{base}-{B}-{lens}-{int(c0)}", sel_case(base, B, lens, c0), True, True
    for base, A in HEAD_CASES:
        yield f"head-{base}-{A}", head_case(base, A), False, base != "wide"
    for h in PROBE_H:
        for B in ENC_B:
            yield f"probe-{h}-{B}", probe_case(h, B), False, True
