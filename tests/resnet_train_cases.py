"""The recipe of the backbone's training golden (tools/gen_golden_resnet_train.py writes tests/golden/resnet_train.npz from the reference's
class; tests/test_resnet_train_host.py and tests/test_gpu_resnet_train.py run this package's class on the same values): weights and
image by tests/resnet_cases.py, upstream gradients randn (fp32) from ONE generator with seed 11 in stage order (all four stages drawn, stages 1..3 applied), the
sample positions of a conv weight from a generator seeded by the tensor's position in the state_dict; and the float64 restatement of
the fold backward that both test files check (the kernel's formulas, include/polyhead.h)."""
import json
import os

import torch
import torch.nn.functional as F

import helpers
import resnet_cases

GSEED, SAMPLES = 11, 2048


def stage_shapes(shape):
    """[(C, h, w)] of the four stages of an image of `shape`"""
    B, _, H, W = shape
    half = lambda n: (n - 1) // 2 + 1
    h, w = half(half(H)), half(half(W))
    out = []
    for i in range(4):
        if i:
            h, w = half(h), half(w)
        out.append((256 << i, h, w))
    return out


def upstream(shape):
    """{stage: fp32 gradient [B, C, h, w]} for stages 1..3: randn for all four stages in stage order, stage 0's (frozen) not applied"""
    g = torch.Generator().manual_seed(GSEED)
    ups = [torch.randn((shape[0],) + s, generator=g) for s in stage_shapes(shape)]
    return {i: ups[i] for i in (1, 2, 3)}


def sample_index(position, numel):
    """the flat positions of the golden's samples of the conv weight that is entry `position` of the state_dict"""
    g = torch.Generator().manual_seed(1000 + position)
    return torch.randint(0, numel, (SAMPLES,), generator=g)


def build_module(**cfg_changes):
    from polyphonicformer_amd import registry
    import polyphonicformer_amd.resnet  # noqa: F401
    with open(os.path.join(helpers.GOLDEN, "resnet_cfg.json")) as f:
        cfg = json.load(f)
    cfg.update(cfg_changes)
    m = registry.build_backbone(cfg)
    m.load_state_dict(resnet_cases.fill(m.state_dict()))
    return m


def gradients_of(m, x, ups):
    """float64 autograd of module `m` (this package's or the reference's, in train mode) -> ({parameter name: gradient}, stages)"""
    m.double().train()
    with torch.enable_grad():
        outs = m(x.double())
        torch.autograd.backward([outs[i] for i in ups], [ups[i].double() for i in ups])
    return {n: p.grad.detach() for n, p in m.named_parameters() if p.grad is not None}, [o.detach() for o in outs]


def torch_reference(shape, frames=None):
    """`_forward_torch` of this package's class on the CPU in float64 with the golden's inputs at `shape`, on the batch entries `frames`"""
    x, ups = resnet_cases.inputs(1, shape)[0], upstream(shape)
    if frames is not None:
        idx = list(frames)
        x, ups = x[idx], {i: u[idx] for i, u in ups.items()}
    m = build_module()
    return gradients_of(m, x, ups)


# ---- the fold backward ---------------------------------------------------------------------------------------------------------
def fold_bwd_formulas(dwp, db, w, gamma, mean, var, eps):
    """(dW' [cout, taps * cin] with k = tap * cin + c, db) -> (dw [cout, cin, kh, kw], dgamma, dbeta) in the dtype of the inputs"""
    cout, cin, kh, kw = w.shape
    rstd = 1.0 / torch.sqrt(var + eps)
    s = gamma * rstd
    d = dwp.reshape(cout, kh, kw, cin).permute(0, 3, 1, 2)
    return d * s[:, None, None, None], ((d * w).sum((1, 2, 3)) - mean * db) * rstd, db.clone()


def fold_case(k, cin, cout, seed):
    """fp32 operands of one fold backward: gamma of both signs, variances from 1e-6 to 1e4 (log-uniform), means of both signs"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    var = 10.0 ** (torch.rand(cout, generator=g) * 10.0 - 6.0)
    var[0], var[1] = 1e-6, 1e4
    gamma = r(cout)
    gamma[2] = -abs(float(gamma[2])) - 0.1
    return dict(dwp=r(cout, k * k * cin) * 3, db=r(cout) * 5, w=r(cout, cin, k, k) * (2.0 / (cin * k * k)) ** 0.5, gamma=gamma,
                mean=r(cout) * 2, var=var)


# ---- the device's forward and backward restated in float64, with or without its rounding points -----------------------------------
def bf16(t):
    return t.float().bfloat16().double()


def exact(t):
    return t.double()


def fold(sd, conv, bn, eps, rnd):
    """(W' rounded by `rnd`, b' in fp32, s, 1 / sqrt(var + eps)) of a convolution and its norm, float64"""
    rstd = 1.0 / torch.sqrt(sd[bn + ".running_var"].double() + eps)
    s = sd[bn + ".weight"].double() * rstd
    return rnd(sd[conv + ".weight"].double() * s[:, None, None, None]), \
        (sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * s).float().double(), s, rstd


def forward_blocks(sd, x, rnd=bf16, eps=1e-5):
    """the device's forward in float64 (tools/gen_golden_resnet.py emulate) -> per block dict(p, stride, stage, first, x, a1, a2, y and the
    folds c1, c2, c3, sc)"""
    w, b, _, _ = fold(sd, "conv1", "bn1", eps, rnd)
    y = rnd(F.max_pool2d(F.conv2d(rnd(x.double()), w, b, stride=2, padding=3).relu(), 3, 2, 1))
    blocks = []
    for i in range(1, 5):
        j = 0
        while f"layer{i}.{j}.conv1.weight" in sd:
            p = f"layer{i}.{j}."
            stride = 2 if (i > 1 and j == 0) else 1
            blk = dict(p=p, stride=stride, x=y, stage=i - 1, first=j == 0)
            blk["c1"] = fold(sd, p + "conv1", p + "bn1", eps, rnd)
            blk["a1"] = rnd(F.conv2d(y, blk["c1"][0], blk["c1"][1]).relu())
            blk["c2"] = fold(sd, p + "conv2", p + "bn2", eps, rnd)
            blk["a2"] = rnd(F.conv2d(blk["a1"], blk["c2"][0], blk["c2"][1], stride=stride, padding=1).relu())
            idn = y
            if p + "downsample.0.weight" in sd:
                blk["sc"] = fold(sd, p + "downsample.0", p + "downsample.1", eps, rnd)
                idn = rnd(F.conv2d(y, blk["sc"][0], blk["sc"][1], stride=stride))
            blk["c3"] = fold(sd, p + "conv3", p + "bn3", eps, rnd)
            y = blk["y"] = rnd((F.conv2d(blk["a2"], blk["c3"][0], blk["c3"][1]) + idn).relu())
            blocks.append(blk)
            j += 1
    return blocks


def backward_blocks(sd, blocks, ups, rnd=bf16, first_trained=1):
    """the device's backward in float64 on the activations of `blocks` (the trained stages' suffice) -> {parameter name: gradient}.
    rnd=bf16: its rounding points -- every gradient plane where the device writes it, the double rounding at a stage boundary, dW'
    and db in fp32; rnd=exact: none, the plain chain rule through the same masks"""
    f32 = (lambda t: t.float().double()) if rnd is bf16 else exact
    grads = {}

    def params(conv, bn, fold_, dz, xin, stride, pad):
        wq, _, s, rstd = fold_
        dwp = f32(torch.nn.grad.conv2d_weight(xin, wq.shape, dz, stride=stride, padding=pad))
        db = f32(dz.sum((0, 2, 3)))
        grads[conv + ".weight"] = dwp * s[:, None, None, None]
        grads[bn + ".weight"] = ((dwp * sd[conv + ".weight"].double()).sum((1, 2, 3)) - sd[bn + ".running_mean"].double() * db) * rstd
        grads[bn + ".bias"] = db

    dinput = lambda shape, fold_, dz, stride, pad: torch.nn.grad.conv2d_input(shape, fold_[0], dz, stride=stride, padding=pad)
    top = blocks[-1]
    up = ups.get(top["stage"])
    g = rnd(up.double() if up is not None else torch.zeros_like(top["y"])) * (top["y"] > 0)
    for n in range(len(blocks) - 1, -1, -1):
        blk = blocks[n]
        if blk["stage"] < first_trained:
            break
        p, s_, xin = blk["p"], blk["stride"], blk["x"]
        need_dx = not (blk["stage"] == first_trained and blk["first"])
        da2 = rnd(dinput(blk["a2"].shape, blk["c3"], g, 1, 0) * (blk["a2"] > 0))
        params(p + "conv3", p + "bn3", blk["c3"], g, blk["a2"], 1, 0)
        if "sc" in blk:
            params(p + "downsample.0", p + "downsample.1", blk["sc"], g, xin, s_, 0)
        da1 = rnd(dinput(blk["a1"].shape, blk["c2"], da2, s_, 1) * (blk["a1"] > 0))
        params(p + "conv2", p + "bn2", blk["c2"], da2, blk["a1"], s_, 1)
        params(p + "conv1", p + "bn1", blk["c1"], da1, xin, 1, 0)
        if not need_dx:
            continue
        dx1 = dinput(xin.shape, blk["c1"], da1, 1, 0)
        if "sc" in blk:
            low = rnd(torch.nn.grad.conv2d_input(g.shape[:1] + xin.shape[1:2] + g.shape[2:], blk["sc"][0], g))     # on the sampled pixels
            spread = torch.zeros_like(xin)
            spread[:, :, ::s_, ::s_] = low
            up = ups.get(blk["stage"] - 1)
            g = rnd(rnd(dx1 + spread) + (up.double() if up is not None else 0)) * (xin > 0)
        else:
            g = rnd(dx1 + g) * (xin > 0)
    return grads
