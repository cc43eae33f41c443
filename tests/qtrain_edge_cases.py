"""Seeded inputs of tests/test_gpu_qtrain_edges.py, their float64 reference and the conditions they must meet, CPU only (no library
load).  The GPU tests call `ph_qtrain_forward` / `ph_qtrain_backward` on these; tests/test_qtrain_oracle_host.py asserts every
condition without a GPU, so that a seed change which breaks one fails there.  Everything comes from seeded CPU generators; nothing
is stored.

`query_side` is the part of `oracle/poly_oracle.update_stage` between the pooling and the dynamic convolutions, from the oracle's
own bricks, with feat_transform folded the way `train._Stage` folds it: it takes the pooled sums of the UNtransformed maps and the
pixel counts, and returns the dynamic kernels already multiplied into feat_transform."""
import contextlib
import functools

import torch
import torch.nn.functional as F

import helpers as Hh
from oracle import poly_oracle as O
from polyphonicformer_amd import train as TR
from polyphonicformer_amd.registry import HEADS
import polyphonicformer_amd.kernel_update_head  # noqa: F401
import polyphonicformer_amd.kernel_updator  # noqa: F401
from track_edge_cases import row_err  # noqa: F401  -- the per-row measure, shared with the other edge files

MARGIN = 5e-5                    # a ReLU pre-activation this close to 0 is a coin flip between device and float64
NUDGE, ROUNDS = 2e-3, 20
C = 256
NAMES = TR.QT_MASK_NAMES + TR.QT_DEPTH_NAMES            # the 83 parameters in the order of the pointer table
OUTPUTS = ("cls", "kern", "kbias", "obj")
INPUT_GRADS = ("g_pooled", "g_k", "g_q")

# per branch: feat_transform, the suffix of the updator / attention / FFN names
BRANCH = (("feat_transform.conv", ""), ("feat_depth_transform.conv", "_depth"))
# the six ReLUs in the order `query_side` evaluates them, and the bias that shifts each one's input
RELU_BIAS = ["kernel_update_conv.fc_norm.bias", "ffn.layers.0.0.bias", "cls_fcs.1.bias", "mask_fcs.1.bias",
             "kernel_update_conv_depth.fc_norm.bias", "ffn_depth.layers.0.0.bias"]
# the biases the `offset` fixture raises and the LayerNorms behind them, per branch suffix.  300 puts the rows of the first three
# at |mean| / spread >= 200; the rows that feed the gates' LayerNorms (input_gate(i_in * p_in): a product of two projections) spread
# up to 7 (mask branch) and 12 (depth branch, k + q), where 300 measured a ratio of 41 -- the gates' biases are raised by 1200 so that
# every row is past 100 there as well
OFFSET_BIAS = ["kernel_update_conv{s}.fc_layer.bias", "attention{s}.attn.out_proj.bias", "ffn{s}.layers.1.bias",
               "kernel_update_conv{s}.input_gate.bias", "kernel_update_conv{s}.update_gate.bias"]
OFFSET_BY = [300.0, 300.0, 300.0, 1200.0, 1200.0]
OFFSET_NORMS = ["kernel_update_conv{s}.fc_norm", "attention_norm{s}", "ffn_norm{s}", "kernel_update_conv{s}.input_norm_in",
                "kernel_update_conv{s}.norm_in"]
GATE_NORMS = ["kernel_update_conv{s}.input_norm_in", "kernel_update_conv{s}.norm_in"]

# name -> (B, N, L, F)
SIZE_CASES = {
    "S1": (1, 1, 19, 2048),      # R = 1: softmax over one key, one row under 16 colsum row lanes, K = 1 in every dY^T X
    "S2": (1, 2, 1, 4),          # L = 1 (Lp = 4, ldc = 1); F = 4: one K step, mostly padding, seven empty splits
    "S3": (1, 65, 3, 36),        # R = N = 65: one past the GEMM tile and the attention lane stride; F = 36: a second K step of 4
    "S4": (3, 21, 19, 256),      # R = 63, one short of the tile
    "S5": (2, 64, 4, 288),       # N = 64; Lp = L; 9 K steps: splits of 2, 2, 2, 2, 1, 0, 0, 0; M = 288: four and a half row tiles
    "S6": (1, 280, 133, 256),    # the largest N: 156 800 B of LDS in the attention backward
}
VALUE_SHAPE = (2, 37, 19, 256)
VALUE_CASES = ("norms", "sharp", "gates", "offset", "counts")
CASES = tuple(SIZE_CASES) + VALUE_CASES
COUNT_VALUES = (0.0, 1.0, 37.0, 32768.0)
SHARP_FACTORS = (12.0, 14.0, 16.0, 20.0, 24.0)           # tried in order; the first that gives scores beyond +-100 in both branches
SEED = {n: 8100 + 10 * i for i, n in enumerate(CASES)}


def gen(seed):
    return torch.Generator().manual_seed(seed)


# =================================================================================================================================
# the reference
# =================================================================================================================================
def query_side(sd, pooled, cnt, k, q, heads=8):
    """pooled [2, B, N, 256] (sums of x / depth_feats over each hard mask), cnt [B, N] (pixels per mask), k, q [B, N, 256]
    -> cls [B, N, L], kern [2, B, N, 256], kbias [2, B, N], obj [2, B, N, 256]: the outputs of `ph_qtrain_forward`"""
    kin = (k, q + k.detach())                                                 # update_stage :250
    obj, kern, kbias, cls = [], [], [], None
    for br, (ft, s) in enumerate(BRANCH):
        Wt, bt = sd[ft + ".weight"].flatten(1), sd[ft + ".bias"]
        u = pooled[br] @ Wt.t() + cnt[..., None] * bt                         # pooling is linear in feat_transform
        o = O.kernel_updator(sd, "kernel_update_conv" + s, u, kin[br])
        o = O._ln(sd, "attention_norm" + s, O.mha_self(sd, "attention" + s, o, heads))
        o = O._ln(sd, "ffn_norm" + s, O.ffn(sd, "ffn" + s, o))
        if br == 0:
            cls_feat = F.relu(O._ln(sd, "cls_fcs.1", O._lin(sd, "cls_fcs.0", o, bias=False)))
            feat = F.relu(O._ln(sd, "mask_fcs.1", O._lin(sd, "mask_fcs.0", o, bias=False)))
            cls = O._lin(sd, "fc_cls", cls_feat)
            kraw = O._lin(sd, "fc_mask", feat)
        else:
            kraw = O._lin(sd, "fc_depth", O._ln(sd, "depth_regs.1", O._lin(sd, "depth_regs.0", o, bias=False)))    # no activation
        obj.append(o)
        kern.append(kraw @ Wt)                                                # conv(W_t x + b_t, kraw) = (kraw W_t) x + kraw . b_t
        kbias.append(kraw @ bt)
    return cls, torch.stack(kern), torch.stack(kbias), torch.stack(obj)


@contextlib.contextmanager
def tap():
    """records, while the block runs, the input of every F.relu and torch.softmax and (weight, input, output) of every
    F.layer_norm the oracle's bricks call -> dict(relu=[...], softmax=[...], ln=[...])"""
    seen = dict(relu=[], softmax=[], ln=[])
    relu, ln, sm = F.relu, F.layer_norm, torch.softmax

    def ln_(x, shape, w, b, eps):
        y = ln(x, shape, w, b, eps)
        seen["ln"].append((w, x.detach(), y.detach()))
        return y

    F.relu = lambda t, *a, **kw: (seen["relu"].append(t.detach()), relu(t, *a, **kw))[1]
    F.layer_norm = ln_
    torch.softmax = lambda t, *a, **kw: (seen["softmax"].append(t.detach()), sm(t, *a, **kw))[1]
    try:
        yield seen
    finally:
        F.relu, F.layer_norm, torch.softmax = relu, ln, sm


def trace(sd, inp, dtype=torch.float64):
    """the forward alone in `dtype` -> dict(relu: the six ReLU inputs in RELU_BIAS order, scores: the pre-softmax scores per
    branch, ln_in / ln_out: {LayerNorm name: input / output})"""
    w = {n: v.to(dtype) for n, v in sd.items()}
    with torch.no_grad(), tap() as seen:
        query_side(w, *(inp[n].to(dtype) for n in ("pooled", "cnt", "k", "q")))
    assert len(seen["relu"]) == len(RELU_BIAS) and len(seen["softmax"]) == 2
    name_of = {id(v): n[:-len(".weight")] for n, v in w.items() if n.endswith(".weight")}
    return dict(relu=seen["relu"], scores=seen["softmax"], ln_in={name_of[id(g)]: x for g, x, _ in seen["ln"]},
                ln_out={name_of[id(g)]: y for g, _, y in seen["ln"]})


def run(sd, inp, cot, dtype):
    """`query_side` under autograd in `dtype` with the cotangents `cot` -> the 90 tensors {name: tensor}: the 4 outputs, g_pooled,
    g_k, g_q and the gradient of each of the 83 parameters under its state-dict name"""
    with torch.enable_grad():
        w = {n: sd[n].detach().clone().to(dtype).requires_grad_(True) for n in NAMES}
        x = {n: inp[n].detach().clone().to(dtype).requires_grad_(n != "cnt") for n in ("pooled", "cnt", "k", "q")}
        outs = query_side(w, x["pooled"], x["cnt"], x["k"], x["q"])
        total = sum((o * cot[n].to(dtype)).sum() for n, o in zip(OUTPUTS, outs))
        leaves = [x["pooled"], x["k"], x["q"]] + [w[n] for n in NAMES]
        grads = torch.autograd.grad(total, leaves)
    res = {n: o.detach() for n, o in zip(OUTPUTS, outs)}
    res.update(zip(INPUT_GRADS + tuple(NAMES), grads))
    return res


# =================================================================================================================================
# parameters and inputs
# =================================================================================================================================
@functools.lru_cache(maxsize=None)
def _shipped_shapes():
    head = HEADS.build(Hh.stage_cfg(C, 256, 8, 19, 8, 11))
    shapes = {n: tuple(v.shape) for n, v in head.state_dict().items()}
    assert set(NAMES) <= set(shapes) and len(NAMES) == 83
    return {n: shapes[n] for n in NAMES}


def state(L, Fd, seed):
    """the 83 parameters of one stage with `L` classes and an FFN of width `Fd` (the Python head refuses Fd % 256 != 0: the
    shapes are a shipped head's with Fd and L substituted), filled by `helpers.seeded_fill`"""
    shapes = dict(_shipped_shapes())
    for s in ("", "_depth"):
        shapes[f"ffn{s}.layers.0.0.weight"], shapes[f"ffn{s}.layers.0.0.bias"], shapes[f"ffn{s}.layers.1.weight"] = (Fd, C), (Fd,), (C, Fd)
    shapes["fc_cls.weight"], shapes["fc_cls.bias"] = (L, C), (L,)
    return Hh.seeded_fill(shapes, seed)


def inputs(B, N, L, seed, counts=None):
    """-> (inp, cot): cnt integers in [1, 60) (or drawn from `counts`), pooled = sqrt(cnt) N(0, 1), k, q ~ N(0, 1); cotangents
    N(0, 1), 0.1 N(0, 1) for kern / kbias"""
    g = gen(seed)
    if counts is None:
        cnt = torch.randint(1, 60, (B, N), generator=g).float()
    else:
        cnt = torch.tensor(counts)[torch.randint(0, len(counts), (B, N), generator=g)]
    pooled = cnt.sqrt()[None, :, :, None] * torch.randn(2, B, N, C, generator=g)
    inp = dict(pooled=pooled.contiguous(), cnt=cnt, k=torch.randn(B, N, C, generator=g), q=torch.randn(B, N, C, generator=g))
    cot = dict(cls=torch.randn(B, N, L, generator=g), kern=0.1 * torch.randn(2, B, N, C, generator=g),
               kbias=0.1 * torch.randn(2, B, N, generator=g), obj=torch.randn(2, B, N, C, generator=g))
    return inp, cot


def ln_gains(sd):
    return [n for n, v in sd.items() if v.dim() == 1 and n.endswith(".weight")]


def _norms(sd, g):
    """every LayerNorm gain +-2^|N(0, 1)|, capped at 4, about 5 % exactly 0; every 1-D bias N(0, 1)"""
    for n in sorted(sd):
        v = sd[n]
        if v.dim() != 1:
            continue
        if n.endswith(".weight"):
            mag = (2.0 ** torch.randn(v.shape, generator=g).abs()).clamp_max(4.0)
            sign = torch.where(torch.rand(v.shape, generator=g) < 0.5, -1.0, 1.0)
            sd[n] = (mag * sign * (torch.rand(v.shape, generator=g) >= 0.05)).float()
        else:
            sd[n] = torch.randn(v.shape, generator=g)


def score_range(sd, inp):
    """per branch (largest, smallest) pre-softmax score of the float64 forward"""
    return [(float(s.max()), float(s.min())) for s in trace(sd, inp)["scores"]]


def _sharp(sd, inp):
    """rows 0 .. 511 (q and k) of both in_proj_weights times the first of SHARP_FACTORS that puts scores beyond +-100 in both
    branches: a softmax that does not subtract the row maximum overflows in float32"""
    base = {s: sd[f"attention{s}.attn.in_proj_weight"].clone() for s in ("", "_depth")}
    for f in SHARP_FACTORS:
        for s, w in base.items():
            w = w.clone()
            w[:2 * C] *= f
            sd[f"attention{s}.attn.in_proj_weight"] = w
        if all(hi > 100.0 and lo < -100.0 for hi, lo in score_range(sd, inp)):
            return f
    raise AssertionError(("no factor gives scores beyond +-100", score_range(sd, inp)))


def condition_relus(sd, inp):
    """`test_gpu_qtrain.condition_relus` for `query_side`: nudge the bias of every channel whose ReLU input lies within MARGIN of 0
    on some row of the float64 forward by NUDGE, until none does -> rounds used"""
    for it in range(ROUNDS + 1):
        dirty = False
        for t, name in zip(trace(sd, inp)["relu"], RELU_BIAS):
            close = (t.abs() < MARGIN).reshape(-1, t.shape[-1]).any(0)
            if close.any():
                assert it < ROUNDS, f"{name}: {int(close.sum())} channels within {MARGIN} of 0 after {ROUNDS} rounds"
                sd[name] = sd[name] + NUDGE * close.float()
                dirty = True
        if not dirty:
            return it


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(shape (B, N, L, F), sd, inp, cot) of a size case or a value fixture, ReLUs conditioned; shared, never modified"""
    B, N, L, Fd = SIZE_CASES.get(name, VALUE_SHAPE)
    seed = SEED[name]
    sd = state(L, Fd, seed)
    inp, cot = inputs(B, N, L, seed + 1, COUNT_VALUES if name == "counts" else None)
    extra = {}
    if name == "norms":
        _norms(sd, gen(seed + 2))
    elif name == "sharp":
        extra["factor"] = _sharp(sd, inp)
    elif name == "gates":
        for s in ("", "_depth"):
            for n in GATE_NORMS:
                sd[n.format(s=s) + ".weight"] = sd[n.format(s=s) + ".weight"] * 40.0
    elif name == "offset":
        for s in ("", "_depth"):
            for n, by in zip(OFFSET_BIAS, OFFSET_BY):
                sd[n.format(s=s)] = sd[n.format(s=s)] + by
    extra["rounds"] = condition_relus(sd, inp)
    return dict(shape=(B, N, L, Fd), sd=sd, inp=inp, cot=cot, **extra)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 run, float32 run) of a case -- computed once, shared, never modified"""
    c = case(name)
    return run(c["sd"], c["inp"], c["cot"], torch.float64), run(c["sd"], c["inp"], c["cot"], torch.float32)
