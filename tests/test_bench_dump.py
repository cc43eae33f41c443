"""bench.py --dump-outputs (CPU): float32 .npy files of the five caller-visible outputs, at most 64 MB in all, the larger arrays as
a fixed sample that is the same for the same shape in every run; and (GPU) what a plain run's line carries."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
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


@pytest.mark.gpu
def test_plain_run_line_is_the_headline_and_the_dump(gpu, tmp_path):
    """a plain run (no --full) times the headline and writes the dump; the legs that need runs of their own stay out of its line"""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None), env.pop("RANK", None), env.pop("LOCAL_RANK", None)
    r = subprocess.run([sys.executable, bench.__file__, "--gpus", "1", "--workload", "tiny", "--frames", "8", "--steps", "3", "--warmup", "1",
                        "--streams", "2", "--dump-outputs", str(tmp_path / "d")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["unit"] == "frames/s" and res["higher_is_better"] is True and res["steps"] == 3 and res["warmup"] == 1
    assert abs(res["value"] - 8 * 1e3 / res["ms_per_step"]) / res["value"] < 1e-3
    assert res["dtype"].startswith("bf16") and res["metric"].startswith("frames/sec")
    for leg in ("roofline", "kernels_ms", "algorithmic", "precision_modes", "cfg5_fp16", "sparse_masks", "with_kernel_head",
                "track_allgather", "cpu_baseline"):
        assert leg not in res, leg
    assert "--full" in res["legs_not_run"]
    assert sorted(os.listdir(tmp_path / "d")) == sorted(n + ".npy" for n in bench.DUMP_NAMES)
    assert sorted(res["dump_outputs"]["arrays"]) == sorted(bench.DUMP_NAMES)
