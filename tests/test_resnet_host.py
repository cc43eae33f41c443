"""CPU: the backbone module (polyphonicformer_amd/resnet.py) without the device -- the reference's key set, `_forward_torch` against
the reference's golden outputs (tools/gen_golden_resnet.py), the float64 BatchNorm fold, train() / frozen_stages, the unsupported
arguments and the registry."""
import json

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import helpers as Hh
import resnet_cases
from polyphonicformer_amd import registry
import polyphonicformer_amd.resnet as RN


def _golden():
    g = Hh.load_golden("resnet.npz")
    return g, json.loads(bytes(g["keys_json"]).decode())


def _cfg():
    with open(Hh.GOLDEN + "/resnet_cfg.json") as f:
        return json.load(f)


def _module():
    m = registry.MODELS.build(_cfg())
    m.load_state_dict(resnet_cases.fill(m.state_dict()))
    return m.eval()


def test_state_dict_keys_and_shapes_are_the_reference_s():
    _, keys = _golden()
    m = registry.build_backbone(_cfg())
    assert isinstance(m, RN.ResNet)
    sd = m.state_dict()
    assert len(keys) == 318 and list(sd) == list(keys)
    assert {k: list(v.shape) for k, v in sd.items()} == keys
    assert sd["bn1.num_batches_tracked"].dtype == torch.int64


def test_forward_torch_against_reference_golden():
    g, _ = _golden()
    m = _module()
    with torch.no_grad():
        outs = m(resnet_cases.inputs(1)[0])                     # a CPU tensor: forward takes the torch path
    assert len(outs) == 4
    bound = 4 * float(g["f32_err"])
    for i, o in enumerate(outs):
        ref = torch.from_numpy(g[f"out{i}"])
        assert o.shape == ref.shape
        err = Hh.rel_err(o, ref)
        print(f"stage {i}: {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (i, err, bound)


@pytest.mark.parametrize("cin,cout,k,stride", [(3, 64, 7, 2), (64, 64, 3, 1), (128, 128, 3, 2), (256, 512, 1, 2)])
def test_fold_bn_against_float64_batch_norm(cin, cout, k, stride):
    g = torch.Generator().manual_seed(cin + cout + k)
    conv = nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=False)
    bn = nn.BatchNorm2d(cout).eval()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.1)
        bn.weight.copy_(1 + 0.3 * torch.randn(cout, generator=g)); bn.bias.copy_(torch.randn(cout, generator=g))
        bn.running_mean.copy_(torch.randn(cout, generator=g)); bn.running_var.copy_(0.2 + torch.rand(cout, generator=g))
    x = torch.randn(2, cin, 9, 11, generator=g).double()
    w, b = RN.fold_bn(conv.weight, bn)
    assert w.dtype == b.dtype == torch.float64
    with torch.no_grad():
        ref = F.batch_norm(F.conv2d(x, conv.weight.double(), stride=stride, padding=k // 2), bn.running_mean.double(),
                           bn.running_var.double(), bn.weight.double(), bn.bias.double(), False, 0.0, bn.eps)
        got = F.conv2d(x, w, b, stride=stride, padding=k // 2)
    assert Hh.rel_err(got, ref) < 1e-13


def test_stem_matrix_is_the_kernel_s_k_order():
    w = torch.randn(64, 3, 7, 7, dtype=torch.float64)
    m = RN.stem_matrix(w)
    assert m.shape == (64, RN.STEM_K)
    for kh, kw, c in ((0, 0, 0), (3, 6, 2), (6, 2, 1)):
        assert torch.equal(m[:, 24 * kh + 3 * kw + c], w[:, c, kh, kw])
    assert float(m.reshape(64, -1)[:, 168:].abs().max()) == 0 and float(m[:, :168].reshape(64, 7, 24)[:, :, 21:].abs().max()) == 0


def test_train_keeps_norms_in_eval_and_frozen_stages_without_grad():
    m = registry.MODELS.build(_cfg())
    m.train()
    assert m.training
    assert all(not b.training for b in m.modules() if isinstance(b, nn.BatchNorm2d))
    frozen = list(m.conv1.parameters()) + list(m.bn1.parameters()) + list(m.layer1.parameters())
    assert frozen and all(not p.requires_grad for p in frozen)
    assert not m.layer1.training and m.layer2.training
    assert all(p.requires_grad for p in m.layer2.parameters())
    # norm_eval=False: only the frozen part stays in eval mode
    m2 = RN.ResNet(50, frozen_stages=1, norm_eval=False).train()
    assert not m2.bn1.training and not m2.layer1[0].bn1.training and m2.layer2[0].bn1.training
    # the torch path is differentiable where training asks for it
    x = torch.randn(1, 3, 32, 32)
    with torch.enable_grad():                      # whatever an earlier test left the global switch at
        outs = m(x)
        sum(o.sum() for o in outs).backward()
    assert m.layer2[0].conv1.weight.grad is not None and m.conv1.weight.grad is None


@pytest.mark.parametrize("kw,name", [(dict(dcn=dict(type="DCN")), "dcn"), (dict(plugins=[dict(cfg=dict(type="X"), position="after_conv1")]), "plugins"),
                                     (dict(deep_stem=True), "deep_stem"), (dict(avg_down=True), "avg_down"), (dict(style="caffe"), "style"),
                                     (dict(depth=18), "depth"), (dict(depth=34), "depth"), (dict(dilations=(1, 1, 2, 4)), "dilations"),
                                     (dict(strides=(1, 2, 2, 1)), "strides")])
def test_unsupported_arguments_raise_naming_them(kw, name):
    args = dict(depth=50)
    args.update(kw)
    with pytest.raises(NotImplementedError, match=rf"ResNet: {name}:"):
        RN.ResNet(**args)


@pytest.mark.parametrize("depth,n", [(50, 318), (101, 318 + 17 * 18), (152, 318 + 34 * 18)])
def test_depths_and_out_indices(depth, n):
    m = RN.ResNet(depth, out_indices=(1, 3)).eval()
    assert len(m.state_dict()) == n
    if depth == 50:
        with torch.no_grad():
            outs = m(torch.randn(1, 3, 33, 47))
        assert [tuple(o.shape) for o in outs] == [(1, 512, 5, 6), (1, 2048, 2, 2)]


def test_wrap_fp16_model_switches_this_backbone():
    m = registry.MODELS.build(_cfg())
    assert m.precision == "bf16"
    assert registry.wrap_fp16_model(m) == [m] and m.precision == "fp16"
    with pytest.raises(ValueError):
        m.set_precision("fp32")
