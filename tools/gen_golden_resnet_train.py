#!/usr/bin/env python
"""Golden for the backbone's training path (train.resnet_forward_train), produced by the reference's own ResNet class on the CPU in
float64 (loaded as tools/gen_golden_resnet.py loads it).

Setup: tests/resnet_cases.py's weights and its 1 x 3 x 40 x 72 input, the class in train mode as the config builds it (frozen_stages=1,
norm_eval=True), upstream gradients by tests/resnet_train_cases.upstream (randn, seed 11, drawn for the four stages in order, applied to stages 1..3), one backward in float64.

Writes tests/golden/resnet_train.npz
    names_json                 the 126 trained parameters in state_dict order
    g{i}                       float64: a norm's weight / bias gradient in full; a conv weight's gradient at the
                               resnet_train_cases.sample_index positions (2048 per tensor: 4096 float64 samples of 42 tensors beside
                               the 50 176 norm gradients would not fit the 1 MiB a committed file may have)
    gmax{i}                    the tensor's max |g|
    emu_gerr_bf16              helpers.rel_err of this tool's float64 emulation of the device's rounding points against the float64
                               reference, the maximum over the 126 tensors
    emu_gneed_bf16             helpers.needed_atol of the same at rtol 2^-8, the maximum over the tensors
    emu_perr_bf16, emu_pneed_bf16   the same two measures of the emulated backward against the unrounded float64 backward ON THE SAME
                               (emulated) activations: what the gradient planes' roundings alone cost, with no ReLU mask that differs;
                               asserted below 5e-2, so that twice it is a bound no wrong gradient meets
    emu_perr_bf16_b2, emu_pneed_bf16_b2   the same at 2 x 3 x 64 x 96 (the batch test's shape; resnet_cases.inputs and upstream at that shape)

The emulation's rounding points: the forward's (gen_golden_resnet.emulate: image, folded weights, every layer output); every gradient
plane rounded to bf16 where the device writes it (da2, da1, the downsample's low-resolution input gradient, a block's input gradient);
at a stage boundary the first block's input gradient is rounded, the stage's own gradient added and the sum rounded again; dW' and db
in fp32.

The tool asserts what lets the case fail: every trained tensor's max |g| lies in [1, 1e3] and at least 30 % of its entries are nonzero.

usage: PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_resnet_train.py     (needs the reference tree)"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests")); sys.path.insert(0, os.path.join(REPO, "tools"))
import helpers  # noqa: E402
import resnet_cases  # noqa: E402
import resnet_train_cases as TC  # noqa: E402
import gen_golden_resnet as GR  # noqa: E402

B2_SHAPE = (2, 3, 64, 96)          # tests/test_gpu_resnet_train.py test_batch_sum_and_run_to_run_bits


def run():
    ResNet = GR.load_reference_resnet()
    cfg = GR.backbone_cfg()
    m = ResNet(**{k: v for k, v in cfg.items() if k != "type"})
    sd = resnet_cases.fill(m.state_dict())
    m.load_state_dict(sd)
    x, ups = resnet_cases.inputs(1)[0], TC.upstream(resnet_cases.SHAPE)
    ref, _ = TC.gradients_of(m, x, ups)
    blocks = TC.forward_blocks(sd, x)
    emu, plain = TC.backward_blocks(sd, blocks, ups), TC.backward_blocks(sd, blocks, ups, TC.exact)
    assert set(emu) == set(ref) and len(ref) == 126, (len(emu), len(ref))
    gerr = gneed = 0.0
    perr = max(helpers.rel_err(emu[n], plain[n]) for n in ref)
    pneed = max(helpers.needed_atol(emu[n], plain[n], rtol=2.0 ** -8) for n in ref)
    # the same two measures at the batch test's shape (the emulation against itself: no reference class needed)
    x2, ups2 = resnet_cases.inputs(1, B2_SHAPE)[0], TC.upstream(B2_SHAPE)
    blocks2 = TC.forward_blocks(sd, x2)
    emu2, plain2 = TC.backward_blocks(sd, blocks2, ups2), TC.backward_blocks(sd, blocks2, ups2, TC.exact)
    perr2 = max(helpers.rel_err(emu2[n], plain2[n]) for n in ref)
    pneed2 = max(helpers.needed_atol(emu2[n], plain2[n], rtol=2.0 ** -8) for n in ref)
    # the bound of the narrow check is 2 x these: it must stay one that a wrong gradient (zeros: 1.0, half a batch: about 0.5) misses
    assert max(perr, pneed, perr2, pneed2) < 5e-2, (perr, pneed, perr2, pneed2)
    if 2 * gerr >= 1:
        print(f"NOTE: 2 x emu_gerr_bf16 = {2 * gerr:.3g} >= 1: the bound against the reference passes a zero gradient; the tests pair it "
              "with the narrow check on the device's own activations (emu_perr_bf16, emu_perr_bf16_b2)")
    for n, r in ref.items():
        peak, nz = float(r.abs().max()), float((r != 0).double().mean())
        assert 1.0 <= peak <= 1e3, (n, peak)
        assert nz >= 0.3, (n, nz)
        gerr = max(gerr, helpers.rel_err(emu[n], r))
        gneed = max(gneed, helpers.needed_atol(emu[n], r, rtol=2.0 ** -8))
    peaks = [float(r.abs().max()) for r in ref.values()]
    print(f"{len(ref)} trained tensors, {sum(r.numel() for r in ref.values())} elements, max |g| from {min(peaks):.3g} to {max(peaks):.3g}, "
          f"smallest nonzero share {min(float((r != 0).double().mean()) for r in ref.values()):.2f}")
    return list(m.state_dict().keys()), ref, gerr, gneed, (perr, pneed, perr2, pneed2)


def main():
    keys, ref, gerr, gneed, (perr, pneed, perr2, pneed2) = run()
    names = [k for k in keys if k in ref]
    arrays = {}
    for i, n in enumerate(names):
        r = ref[n]
        arrays[f"g{i}"] = (r.reshape(-1)[TC.sample_index(keys.index(n), r.numel())] if r.dim() == 4 else r).numpy()
        arrays[f"gmax{i}"] = np.float64(float(r.abs().max()))
    path = os.path.join(REPO, "tests", "golden", "resnet_train.npz")
    np.savez_compressed(path, names_json=np.frombuffer(json.dumps(names).encode(), dtype=np.uint8), emu_gerr_bf16=np.float64(gerr),
                        emu_gneed_bf16=np.float64(gneed), emu_perr_bf16=np.float64(perr),
                        emu_pneed_bf16=np.float64(pneed), emu_perr_bf16_b2=np.float64(perr2), emu_pneed_bf16_b2=np.float64(pneed2), **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print("resnet_train.npz", size, "bytes; emu_gerr_bf16", gerr, "emu_gneed_bf16", gneed, "emu_perr_bf16", perr,
          "emu_pneed_bf16", pneed, "at 2x3x64x96", perr2, pneed2)


if __name__ == "__main__":
    main()
