"""CPU: the video training step's host side -- the C ABI declarations of `ph_gtmask_boxes`, its workspace formula and the argument
checks that need no device, `train.gt_match_indices` against the reference's list logic, and the fixture generator's integer arrays
(tools/gen_golden_video_train.py `box_cases`, torch only) against the committed tests/golden/video_train.npz."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import torch

import helpers as Hh
from polyphonicformer_amd import _lib

sys.path.insert(0, os.path.join(Hh.REPO, "tools"))
import gen_golden_video_train as GV  # noqa: E402


def _i32(a):
    return (C.c_int32 * len(a))(*[int(v) for v in a])


def test_header_and_binding_declare_the_entry_points():
    hdr = open(os.path.join(Hh.REPO, "include", "polyhead.h")).read()
    for name in ("ph_gtmask_boxes", "ph_gtmask_boxes_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in _lib.SIGNATURES, name
    assert re.search(r"#define\s+PH_GTBOX_MAX_FRAMES\s+64\b", hdr) and _lib.PH_GTBOX_MAX_FRAMES == 64
    assert len(_lib.SIGNATURES["ph_gtmask_boxes"][1]) == 19
    from polyphonicformer_amd import track_head, train
    for fn in (track_head.gt_mask_rois, train.gt_match_indices, train.track_sample, train.video_track_branch, train.VideoTrainStep):
        assert callable(fn)


def test_workspace_bytes_match_the_documented_formula():
    lib = _lib.load()
    al = lambda b: (b + 255) // 256 * 256
    for G, H, W in (([5], 64, 128), ([3, 0, 9], 25, 49), ([40] * 4, 1024, 2048), ([0], 7, 7), ([1], 65, 1), ([256], 1, 65536)):
        S = sum(G)
        assert lib.ph_gtmask_boxes_workspace_bytes(len(G), _i32(G), H, W) == al(S * H * 4) + al(S * ((H + 63) // 64) * W * 2), (G, H, W)
    for G, H, W in (([257], 8, 8), ([-1], 8, 8), ([1], 0, 8), ([1], 8, 65537), ([1] * 65, 8, 8)):
        assert lib.ph_gtmask_boxes_workspace_bytes(len(G), _i32(G), H, W) == 0
        assert Hh.last_error().startswith("ph_gtmask_boxes_workspace_bytes")


def test_argument_checks_without_a_device():
    """every refusal comes before the first launch, so none of these calls touches a device: the pointers are never read"""
    lib = _lib.load()
    fake = C.c_void_p(4096)

    def call(G=(6,), n=(6,), Np=8, h=4, w=4, H=16, W=16, mode=0, ws=1 << 20, frames=None, stride=16):
        F_ = len(G) if frames is None else frames
        ptrs = (C.c_void_p * max(len(G), 1))(*[4096] * len(G))
        return lib.ph_gtmask_boxes(ptrs, _i32(G), _i32(n), _i32([0] * len(G)), fake, stride, Np, F_, h, w, H, W, mode, fake, fake, fake, fake, ws, None)

    assert call(G=(130,), n=(129,), Np=129) == _lib.PH_EINVAL and "128" in Hh.last_error()
    assert call(n=(5,)) == _lib.PH_EINVAL and "min(G, Np)" in Hh.last_error()
    assert call(G=(9,), n=(9,), Np=8) == _lib.PH_EINVAL
    assert call(G=(257,), n=(8,)) == _lib.PH_EINVAL
    assert call(ws=512) == _lib.PH_EWORKSPACE
    assert call(H=3) == _lib.PH_EUNSUPPORTED and call(W=3) == _lib.PH_EUNSUPPORTED
    assert call(mode=_lib.PH_GTBOX_NEAREST) == _lib.PH_EUNSUPPORTED and "nearest" in Hh.last_error()
    assert call(frames=0) == _lib.PH_EINVAL and call(G=(1,) * 65, n=(1,) * 65) == _lib.PH_EINVAL
    assert call(G=(6, 20), n=(6, 8), stride=16) == _lib.PH_EINVAL and "match_stride" in Hh.last_error()
    assert Hh.last_error().startswith("ph_gtmask_boxes")
    assert call(G=(0,), n=(0,)) == 0                       # nothing to do is not an error, and launches nothing


def test_gt_match_indices_is_the_reference_list_logic():
    from polyphonicformer_amd.train import gt_match_indices
    g = torch.Generator().manual_seed(1)
    cases = [([3, 7, 7, 1], [7, 3, 7, 9, 3]), ([5, 6], []), ([], [1, 2]), ([4, 4, 4], [4]), ([1, 2, 3], [9, 8]),
             (torch.randint(0, 6, (40,), generator=g).tolist(), torch.randint(0, 6, (25,), generator=g).tolist())]
    for gt_ids, ref_ids in cases:
        want = [ref_ids.index(i) if i in ref_ids else -1 for i in gt_ids]                  # polyphonic_former_video.py:248-250
        got = gt_match_indices(torch.tensor(gt_ids, dtype=torch.int64), torch.tensor(ref_ids, dtype=torch.int32))
        assert got.dtype == torch.int64 and got.tolist() == want, (gt_ids, ref_ids)


def test_generator_reproduces_the_committed_integer_arrays():
    z = Hh.load_golden("video_train.npz")
    meta = json.loads(bytes(z["meta_json"]).decode())
    assert meta["shapes"] == {k: list(v) for k, v in GV.SHAPES.items()} and meta["ref_gap"] * 4 <= 1e-4
    fresh = GV.box_cases()
    ints = [k for k, v in fresh.items() if v.dtype.kind == "i"]
    assert len(ints) == 4 * (1 + 3 * 3)
    for k in ints:
        assert np.array_equal(fresh[k], z[k]), k
    for name in GV.SHAPES:
        assert np.array_equal(fresh[f"a.{name}.masks"], z[f"a.{name}.masks"]) and np.allclose(fresh[f"a.{name}.exact"], z[f"a.{name}.exact"], rtol=0, atol=1e-9)
        G = fresh[f"a.{name}.masks"].shape[0]
        for sel in meta["selections"]:
            m, pg = z[f"a.{name}.{sel}.match"], z[f"a.{name}.{sel}.pos_gt"]
            assert len(pg) == min(G, int(z[f"a.{name}.{sel}.Np"])) == int((m >= 0).sum())
            assert z[f"a.{name}.{sel}.ref_rois"].shape == (len(pg), 5)
            assert list(m[pg]) == sorted(m[m >= 0])          # ascending prediction row
    assert not np.array_equal(z["a.s4.perm.pos_gt"], np.sort(z["a.s4.perm.pos_gt"]))       # the permutation is not monotone in g
    for tag in ("g5", "g10"):
        s = meta["sampling"][tag]
        assert s["margin"] >= 1e-2 and len(z[f"b.{tag}.pos_gt"]) == min(s["G"], s["Np"])
