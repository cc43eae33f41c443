"""CPU: the arithmetic the backbone's training kernels implement (csrc/ph_resnet_train.hip) restated in float64 against torch autograd
-- the fold backward, the parity rule of the data gradient --, `_forward_torch`'s float64 autograd against the reference class's
gradients (tests/golden/resnet_train.npz: this pins the CPU reference of tests/test_gpu_resnet_train.py to the reference), the sizing
arithmetic of engine.ResNetTrainPlan, and the refusals of the device training path."""
import json

import pytest
import torch
import torch.nn.functional as F

import helpers as Hh
import resnet_cases
import resnet_train_cases as TC
from polyphonicformer_amd import _lib, engine as E, train as T


@pytest.mark.parametrize("eps", [1e-5, 1e-3])
@pytest.mark.parametrize("k,s,H,W", [(3, 1, 5, 9), (3, 2, 6, 8), (3, 2, 5, 9), (1, 1, 4, 7), (1, 2, 4, 7), (1, 2, 6, 8)])
def test_fold_backward_formulas_against_autograd(eps, k, s, H, W):
    """z = conv(x, rnd-free w s) + beta - mu s; dW' and db are autograd's of the folded form, (dw, dgamma, dbeta) by the formulas must
    be autograd's of the unfolded one.  gamma of both signs, variances 1e-6 .. 1e4"""
    cin, cout, B = 6, 5, 2
    p = {n: t.double() for n, t in TC.fold_case(k, cin, cout, seed=10 * k + s + H).items()}
    g = torch.Generator().manual_seed(H * W + k)
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64)
    beta = torch.randn(cout, generator=g, dtype=torch.float64)
    w, gamma, beta = p["w"].requires_grad_(), p["gamma"].requires_grad_(), beta.requires_grad_()
    with torch.enable_grad():
        z = F.batch_norm(F.conv2d(x, w, stride=s, padding=k // 2), p["mean"], p["var"], gamma, beta, False, 0.0, eps)
        dz = torch.randn(z.shape, generator=g, dtype=torch.float64)
        z.backward(dz)
    dwp = torch.nn.grad.conv2d_weight(x, w.shape, dz, stride=s, padding=k // 2).permute(0, 2, 3, 1).reshape(cout, -1)    # k = tap cin + c
    dw, dg, db = TC.fold_bwd_formulas(dwp, dz.sum((0, 2, 3)), w.detach(), gamma.detach(), p["mean"], p["var"], eps)
    for name, got, want in (("dw", dw, w.grad), ("dgamma", dg, gamma.grad), ("dbeta", db, beta.grad)):
        assert Hh.rel_err(got, want) < 1e-12, (name, Hh.rel_err(got, want))
    assert float(gamma.detach().min()) < 0 < float(gamma.detach().max()) and float(p["var"].min()) <= 1e-6 and float(p["var"].max()) >= 1e4


def _data_gradient_by_the_rule(dz, w, s, H, W):
    """dX[q][c] = sum_{tap, n} dZ[(q + pad - tap) / stride][n] W[n][tap][c] over the taps where the quotient is whole and inside"""
    B, cout, Ho, Wo = dz.shape
    cin, k = w.shape[1], w.shape[2]
    pad = k // 2
    dx = torch.zeros(B, cin, H, W, dtype=torch.float64)
    for qy in range(H):
        for qx in range(W):
            for ky in range(k):
                for kx in range(k):
                    ty, tx = qy + pad - ky, qx + pad - kx
                    if ty % s or tx % s or not (0 <= ty // s < Ho and 0 <= tx // s < Wo):
                        continue
                    dx[:, :, qy, qx] += dz[:, :, ty // s, tx // s] @ w[:, :, ky, kx]
    return dx


@pytest.mark.parametrize("k,s", [(3, 1), (3, 2), (1, 1), (1, 2)])
@pytest.mark.parametrize("H,W", [(5, 9), (6, 8), (4, 7)])
def test_data_gradient_parity_rule_against_autograd(k, s, H, W):
    g = torch.Generator().manual_seed(H + W + k + s)
    x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(4, 3, k, k, generator=g, dtype=torch.float64)
    with torch.enable_grad():
        z = F.conv2d(x, w, stride=s, padding=k // 2)
        assert tuple(z.shape[2:]) == (E.conv_out_size(H, k, s), E.conv_out_size(W, k, s))
        dz = torch.randn(z.shape, generator=g, dtype=torch.float64)
        z.backward(dz)
    assert Hh.rel_err(_data_gradient_by_the_rule(dz, w, s, H, W), x.grad) < 1e-13


def test_forward_torch_autograd_against_the_reference_golden():
    golden = Hh.load_golden("resnet_train.npz")
    names = json.loads(bytes(golden["names_json"]).decode())
    ref, _ = TC.torch_reference(resnet_cases.SHAPE)
    keys = list(TC.build_module().state_dict().keys())
    assert len(names) == 126 and set(names) == set(ref)
    for i, n in enumerate(names):
        g = ref[n]
        got = g.reshape(-1)[TC.sample_index(keys.index(n), g.numel())] if g.dim() == 4 else g
        want, peak = torch.from_numpy(golden[f"g{i}"]), float(golden[f"gmax{i}"])
        assert tuple(got.shape) == tuple(want.shape)
        assert float((got - want).abs().max()) <= 1e-10 * peak, (n, float((got - want).abs().max()), peak)
        assert abs(float(g.abs().max()) - peak) <= 1e-10 * peak
        assert 1.0 <= peak <= 1e3


def test_float64_restatement_without_rounding_is_autograd():
    """tests/resnet_train_cases.forward_blocks + backward_blocks with no rounding point: the chain rule the plan implements, against
    float64 autograd of `_forward_torch` -- the structure (masks, stage boundaries, the downsample spread) is right before any kernel runs"""
    m = TC.build_module()
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    x, ups = resnet_cases.inputs(1)[0], TC.upstream(resnet_cases.SHAPE)
    ref, _ = TC.torch_reference(resnet_cases.SHAPE)
    got = TC.backward_blocks(sd, TC.forward_blocks(sd, x, TC.exact), ups, TC.exact)
    assert set(got) == set(ref)
    assert max(Hh.rel_err(got[n], ref[n]) for n in ref) < 1e-6           # b' is kept in fp32 by the restatement as by the device


def test_train_plan_sizes():
    m = TC.build_module()
    blocks = m.block_table()
    B, H, W = 2, 40, 72
    z = E.resnet_train_sizes(B, H, W, blocks, 1)
    (c0, h0, w0), (c1, h1, w1), (c2, h2, w2), (c3, h3, w3) = TC.stage_shapes((B, 3, H, W))
    assert (h0, w0, h3, w3) == (10, 18, 2, 3)
    assert z["stem"] == B * h0 * w0 * 64 and z["frozen_io"] == B * h0 * w0 * 256 == z["frozen_down"] and z["frozen_inner"] == B * h0 * w0 * 64
    kept = 0
    for (c, h, w), (cp, hp, wp), nb in (((c1, h1, w1), (c0, h0, w0), 4), ((c2, h2, w2), (c1, h1, w1), 6), ((c3, h3, w3), (c2, h2, w2), 3)):
        planes = c // 4
        kept += B * (hp * wp * planes + h * w * planes + 2 * h * w * c)            # the first block: a1 at the input size, y and downsample
        kept += (nb - 1) * B * h * w * (2 * planes + c)
    assert z["kept"] == kept
    assert z["grad_io"] == B * h1 * w1 * c1 and z["grad_inner"] == B * h0 * w0 * 128 and z["grad_down"] == B * h2 * w2 * c1
    assert z["wmax"] == 512 * 9 * 512 and len(z["layers"]) == 42
    assert [l[:3] for l in z["layers"][:4]] == [(1, 0, "conv1"), (1, 0, "conv2"), (1, 0, "conv3"), (1, 0, "downsample")]
    z2 = E.resnet_train_sizes(B, H, W, blocks, 2)                                   # layer2 frozen as well
    assert len(z2["layers"]) == 42 - 13 and z2["frozen_io"] == z["frozen_io"] and z2["kept"] < z["kept"]
    index = E.resnet_conv_index(blocks)
    assert index[(0, 0, "conv1")] == 1 and index[(0, 0, "downsample")] == 4 and index[(3, 2, "conv3")] == 52 and len(index) == 52
    lib = _lib.load()
    for (si, j, name, k, s, ci, co, hh, ww) in z["layers"]:
        n = lib.ph_conv_cl_bwd_weight_nsplit(k, s, ci, co, hh, ww, B)
        chunks = B * ((E.conv_out_size(hh, k, s) * E.conv_out_size(ww, k, s) + 63) // 64)
        assert 1 <= n <= chunks
        assert lib.ph_conv_cl_bwd_weight_partial_floats(k, s, ci, co, hh, ww, B, 0) == (0 if n == 1 else n * (co * k * k * ci + co))
        assert lib.ph_conv_cl_bwd_weight_partial_floats(k, s, ci, co, hh, ww, B, chunks + 1) == _lib.PH_EINVAL


def test_nsplit_rule_at_the_full_size():
    """layer2's conv1 has 16 tiles and 128 x 256 x B pixels: many ranges; layer4's conv2 has 576 tiles and 2048 B pixels: few"""
    lib = _lib.load()
    early, late = lib.ph_conv_cl_bwd_weight_nsplit(1, 1, 512, 128, 128, 256, 2), lib.ph_conv_cl_bwd_weight_nsplit(3, 1, 512, 512, 32, 64, 2)
    assert early * 16 >= 1024 and late * 576 <= 2 * 1024 and 1 <= late < early <= 64


@torch.enable_grad()
def test_refusals_need_no_device():
    x = resnet_cases.inputs(1)[0]
    for changes, arg in ((dict(frozen_stages=0), "frozen_stages"), (dict(frozen_stages=-1), "frozen_stages"), (dict(norm_eval=False), "norm_eval")):
        m = TC.build_module(**changes).train().train_on_device()
        with pytest.raises(NotImplementedError, match=arg):
            m(x)
    with pytest.raises(NotImplementedError, match="precision"):
        TC.build_module().train().set_precision("fp16").train_on_device()(x)
    with pytest.raises(NotImplementedError, match="img"):
        TC.build_module().train().train_on_device()(x.clone().requires_grad_(True))
    m = TC.build_module().train()
    assert m.device_training is False and m.train_on_device().device_training is True and m.train_on_device(False).device_training is False
    outs = m(x)                                                            # the default stays torch
    assert outs[1].requires_grad and T.resnet_forward_train is not None
    with pytest.raises(_lib.PolyheadError):
        TC.build_module().train().train_on_device()(x)                     # in scope, but not on the GPU: an error, not torch
