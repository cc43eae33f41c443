"""`mixed16` (PH_PREC_BF16_KF16) conv kernels: the bf16 feature tile reaches LDS as fp16 through a producer wave's registers
(ph_conv_inl.h conv_stage_*).  Pinned to the fp16 grade's kernels, which run the same MFMA sequence on an fp16 plane through the
LDS-DMA ring: on a bf16 plane whose every value converts to fp16 exactly, both grades must give the same bits."""
import pytest
import torch

from polyphonicformer_amd import _lib, engine as E

pytestmark = pytest.mark.gpu


def _exact_planes(B, H, W, gen, gpu):
    """the same feature values as a bf16 plane and as an fp16 plane ([1, B, 256, HWp] int16, zero padding): randn rounded to bf16, magnitudes
    below 2^-10 set to zero -- what is left lies in fp16's normal range with 8 significand bits, so bf16 -> fp16 loses nothing"""
    HW, HWp = H * W, E.hw_padded(H * W)
    xb = torch.randn(B, 256, HW, generator=gen).bfloat16()
    xb = torch.where(xb.float().abs() < 2.0 ** -10, torch.zeros_like(xb), xb)
    xh = xb.to(torch.float16)
    assert torch.equal(xh.float(), xb.float())                      # the conversion is exact (on the CPU, before anything runs)
    assert float(xb.float().abs().max()) > 1.0 and float((xb == 0).float().mean()) < 0.01
    pb = torch.zeros(1, B, 256, HWp, dtype=torch.bfloat16)
    ph = torch.zeros(1, B, 256, HWp, dtype=torch.float16)
    pb[0, :, :, :HW], ph[0, :, :, :HW] = xb, xh
    return pb.view(torch.int16).to(gpu), ph.view(torch.int16).to(gpu)


def _kernels(B, Npad, gen, gpu):
    kern = (torch.randn(2, B, Npad, 256, generator=gen) * 0.1).to(torch.float16).view(torch.int16)[None].contiguous().to(gpu)
    kbias = (torch.randn(2, B, Npad, generator=gen) * 0.1).to(gpu)
    return kern, kbias


@pytest.mark.parametrize("N,H,W,B,ns", [(153, 2, 64, 1, 1),        # one range of two tiles: shorter than the register pipeline
                                        (153, 4, 64, 2, 2),
                                        (40, 7, 64, 1, 2),         # NRT = 2
                                        (111, 16, 24, 3, 3),
                                        (160, 9, 31, 2, 4),        # ragged H * W, pixel padding, uneven and empty ranges
                                        (192, 6, 20, 2, 1)])       # NRT = 6: keeps the in-place conversion
def test_poolx_staged_equals_fp16_grade(gpu, N, H, W, B, ns):
    """ph_dynconv_poolx: mask bits and the x columns of the partial sums, bit for bit at the same nsplit"""
    lib = _lib.load()
    assert lib.ph_dynconv_poolx_supported(N, _lib.PH_PREC_BF16_KF16) == 1 and lib.ph_dynconv_poolx_supported(N, _lib.PH_PREC_F16) == 1
    g = torch.Generator().manual_seed(900 + N + H)
    HW, Npad = H * W, E.n_padded(N)
    pb, ph = _exact_planes(B, H, W, g, gpu)
    kern, kbias = _kernels(B, Npad, g, gpu)
    out = {}
    for prec, planes in ((_lib.PH_PREC_F16, ph), (_lib.PH_PREC_BF16_KF16, pb)):
        bits = torch.full((B, Npad, E.hw_padded(HW) // 32), -1, dtype=torch.int32, device=gpu)
        part = torch.full((B, ns, Npad, 512), float("nan"), dtype=torch.float32, device=gpu)
        E.dynconv_poolx(planes, kern, kbias, N, HW, prec, bits, part)
        out[prec] = (bits, part[..., :256])
    torch.cuda.synchronize()
    ref_bits, ref_part = out[_lib.PH_PREC_F16]
    bits, part = out[_lib.PH_PREC_BF16_KF16]
    assert not torch.isnan(ref_part).any() and bool((ref_bits[:, :N] != 0).any()) and bool((ref_part != 0).any())
    assert torch.equal(bits, ref_bits)
    assert torch.equal(part, ref_part)


@pytest.mark.parametrize("N,H,B,wgs", [(153, 2, 1, 0),
                                       # ranges that start inside a frame: silent halo row first.  The issue lists this case with N = 33,
                                       # which ph_dynconv_up2 does not exist for in any grade (65 <= N <= 224, ph_dynconv_up2_supported);
                                       # 65 is the kernel's nearest N with the same shape: one live query row in the last 32-row block
                                       (65, 3, 2, 5),
                                       (153, 5, 2, 7),
                                       (153, 3, 2, 6)])            # one-row ranges
def test_up2_staged_equals_fp16_grade(gpu, N, H, B, wgs):
    """ph_dynconv_up2 at W = 256, both branches, with and without the low-resolution output: `low` and `up` bit for bit"""
    W = 256
    lib = _lib.load()
    assert lib.ph_dynconv_up2_supported(N, H, W, _lib.PH_PREC_BF16_KF16, _lib.PH_OUT_F16) == 1
    g = torch.Generator().manual_seed(700 + N + H)
    Npad = E.n_padded(N)
    pb, ph = _exact_planes(B, H, W, g, gpu)
    kern, kbias = _kernels(B, Npad, g, gpu)
    with _lib.switches(up2_wgs=wgs):
        for br in (0, 1):
            out = {}
            for prec, planes in ((_lib.PH_PREC_F16, ph), (_lib.PH_PREC_BF16_KF16, pb)):
                low = torch.full((B, N, H, W), float("nan"), device=gpu, dtype=torch.float16)
                up = torch.full((B, N, 2 * H, 2 * W), float("nan"), device=gpu, dtype=torch.float16)
                upn = torch.full_like(up, float("nan"))
                E.dynconv_up2(planes, kern, kbias, br, N, H, W, prec, up, logits_out=low, out_dtype=_lib.PH_OUT_F16)
                E.dynconv_up2(planes, kern, kbias, br, N, H, W, prec, upn, logits_out=None, out_dtype=_lib.PH_OUT_F16)
                out[prec] = (low, up, upn)
            torch.cuda.synchronize()
            rlow, rup, rupn = out[_lib.PH_PREC_F16]
            low, up, upn = out[_lib.PH_PREC_BF16_KF16]
            assert not torch.isnan(rlow.float()).any() and not torch.isnan(rup.float()).any() and torch.equal(rupn, rup)
            assert torch.equal(low.view(torch.int16), rlow.view(torch.int16)), br
            assert torch.equal(up.view(torch.int16), rup.view(torch.int16)), br
            assert torch.equal(upn.view(torch.int16), rup.view(torch.int16)), br
