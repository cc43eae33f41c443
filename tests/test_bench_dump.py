"""bench.py --dump-outputs (CPU): float32 .npy files of the five caller-visible outputs, at most 64 MB in all, the larger arrays as
a fixed sample that is the same for the same shape in every run."""
import os

import numpy as np
import torch

import bench


def _outs(seed):
    g = torch.Generator().manual_seed(seed)
    B, N, H, W, L = 2, 153, 64, 128, 133
    return dict(obj=torch.randn(B, N, 256, generator=g), cls=torch.rand(B, N, L, generator=g),
                mask=torch.randn(B, N, H, W, generator=g).half(), mask_up=torch.randn(B, N, 2 * H, 2 * W, generator=g).half(),
                depth_up=torch.randn(B, N, 2 * H, 2 * W, generator=g).bfloat16(), dobj=torch.zeros(1), depth=None)


def test_dump_outputs_files_budget_and_fixed_sample(tmp_path):
    outs = _outs(0)
    info = bench.dump_outputs(outs, str(tmp_path / "a"))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(n + ".npy" for n in bench.DUMP_NAMES)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_BYTES == 64 * 10 ** 6
    for name in bench.DUMP_NAMES:
        a = np.load(tmp_path / "a" / (name + ".npy"))
        assert a.dtype == np.float32 and np.isfinite(a).all()
        assert info["arrays"][name]["shape"] == list(outs[name].shape) and info["arrays"][name]["elements_written"] == a.size
    # small arrays whole, in their own shape and values
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "obj.npy"), outs["obj"].numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "mask.npy"), outs["mask"].float().numpy())
    # the large ones sampled: values taken from the array, at the same indices in a second dump of other values of that shape
    up = np.load(tmp_path / "a" / "mask_up.npy")
    assert up.ndim == 1 and up.size < outs["mask_up"].numel()
    assert np.isin(up, outs["mask_up"].float().numpy().ravel()).all()
    outs2 = dict(outs, mask_up=outs["mask_up"] + 1)
    bench.dump_outputs(outs2, str(tmp_path / "b"))
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "mask_up.npy"), (outs["mask_up"] + 1).float().numpy().ravel()[
        np.sort(np.random.default_rng(0).choice(outs["mask_up"].numel(), up.size, replace=False))])
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "depth_up.npy"), np.load(tmp_path / "a" / "depth_up.npy"))
