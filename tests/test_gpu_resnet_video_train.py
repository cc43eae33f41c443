"""`VideoTrainStep(fpn=..., backbone=...)` on tests/test_gpu_video_train.py's fixture at the size tests/test_gpu_fpn_train.py uses for
`fpn=`: the step from the images gives, bit for bit, the losses and every parameter gradient of the step run on the backbone's stages
with the stage gradients then pushed through the backbone's backward by hand."""
import pytest
import torch

import resnet_cases
import resnet_train_cases as TC
from test_gpu_video_train import video_parts  # noqa: F401  (the module fixture of the video step's parts)
from test_gpu_fpn_train import B, _fpn

pytestmark = pytest.mark.gpu


def test_video_train_step_from_the_images(gpu, video_parts):  # noqa: F811
    from polyphonicformer_amd import train as TR
    neck, rpn, roi, th, tcfg, _, _, img_gt, vid = video_parts
    fpn = _fpn(gpu)
    bb = TC.build_module().to(gpu).train().train_on_device()
    mods = (bb, fpn, neck, rpn, roi, th)
    img, img_ref = (t.to(gpu) for t in resnet_cases.inputs(2, (B, 3, 64, 128)))          # stages 16x32, 8x16, 4x8, 2x4

    def clear():
        for top in mods:
            for p in top.parameters():
                p.grad = None

    def grads():
        return {(i, n): p.grad.clone() for i, top in enumerate(mods) for n, p in top.named_parameters() if p.grad is not None}

    with pytest.raises(ValueError, match="backbone needs fpn"):
        TR.VideoTrainStep(neck, rpn, roi, th, tcfg, backbone=bb)
    with torch.enable_grad():
        st = [t.detach().clone() for t in TR.resnet_forward_train(bb, img)]
    with torch.no_grad():
        st_ref = [t.clone() for t in bb.eval()(img_ref)]
    bb.train()
    assert [tuple(t.shape[2:]) for t in st] == [(16, 32), (8, 16), (4, 8), (2, 4)]
    clear()
    with TR.VideoTrainStep(neck, rpn, roi, th, tcfg, fpn=fpn) as step:
        want_losses, want_total, g_st = step.forward_backward(st, st_ref, *img_gt, *vid)
    with torch.enable_grad():
        torch.autograd.backward(TR.resnet_forward_train(bb, img), g_st)                   # the backbone's backward by hand
    want = grads()
    clear()
    flags = [m.training for top in mods for m in top.modules()]
    with TR.VideoTrainStep(neck, rpn, roi, th, tcfg, fpn=fpn, backbone=bb) as step:
        ps = step.parameters()
        trained = [p for p in bb.parameters() if p.requires_grad]
        assert len(trained) == 126 and len(ps) == len({id(p) for p in ps}) and all(a is b for a, b in zip(ps, trained))
        assert all(a is b for a, b in zip(ps[126:], fpn.parameters()))
        losses, total, g_in = step.forward_backward(img, img_ref, *img_gt, *vid)
    assert [m.training for top in mods for m in top.modules()] == flags
    assert g_in == [] and set(losses) == set(want_losses) and len(losses) == 26
    for k, v in want_losses.items():
        assert torch.equal(losses[k], v), (k, float(losses[k]), float(v))
    assert torch.equal(total, want_total)
    got = grads()
    assert set(got) == set(want) and sum(1 for (i, _) in got if i == 0) == 126
    for key, g in want.items():
        assert torch.equal(got[key], g), key
        assert bool(torch.isfinite(g).all())
    assert any(float(g.abs().max()) > 0 for (i, n), g in got.items() if i == 0 and n.startswith("layer2."))
