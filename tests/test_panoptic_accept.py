"""CPU: the host side of the launch-only panoptic merge (include/polyhead.h ph_panoptic_accept / ph_panoptic_merge).
  * `panoptic.segments_from_records` rebuilds `accept_loop`'s segments_info from a record row, `==` on the list of dicts;
  * where `torch.argsort(-scores, stable=True)` puts NaN and signed zeros is pinned (the device ranks the same way);
  * the size query refuses a bad size and `ph_panoptic_merge` a small workspace, before
    anything is launched (in a child process that sees no GPU, on fake addresses).
`accept_cases` are also the inputs of the device accept step's test (tests/test_gpu_batch_merge.py)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import torch

import helpers as Hh
from polyphonicformer_amd import _lib, panoptic as Pn
from polyphonicformer_amd import build as BLD

NT = 8                       # thing classes of the shipped config
SCORE_THR, OVERLAP_THR = 0.3, 0.6


def _rows(*rows):
    """(score, label, area, orig) rows -> a case"""
    sc, lab, area, orig = zip(*rows)
    return dict(scores=torch.tensor(sc, dtype=torch.float32), labels=torch.tensor(lab, dtype=torch.int64),
                area=np.array(area, dtype=np.int32), orig=np.array(orig, dtype=np.int32), score_thr=SCORE_THR, overlap_thr=OVERLAP_THR)


def accept_cases(K=111, n_random=300, seed=5):
    """name -> dict(scores fp32 [K], labels int64 [K], area / orig int32 [K], score_thr, overlap_thr): `n_random` random draws
    (scores around the threshold, area / orig ratios around 0.6 with exact 3 : 5 pairs, zeros in both counts, repeated scores)
    plus crafted rows, every case padded to the same K so that cases batch."""
    g = torch.Generator().manual_seed(seed)
    f32 = np.float32
    thr32 = f32(SCORE_THR)
    cases = {}
    for i in range(n_random):
        sc = torch.rand(K, generator=g)
        sc[torch.rand(K, generator=g) < 0.2] = float(thr32)                      # exactly the fp32 threshold
        dup = torch.randint(0, K, (K // 4,), generator=g)
        sc[dup] = sc[dup.flip(0)]                                                # exact ties
        lab = torch.randint(0, NT + 11, (K,), generator=g)
        orig = torch.randint(0, 5000, (K,), generator=g)
        area = (orig.double() * (0.2 + 0.8 * torch.rand(K, generator=g).double())).long()
        m = torch.rand(K, generator=g) < 0.25
        orig[m] = orig[m] // 5 * 5
        area[m] = orig[m] // 5 * 3                                               # area / orig == 3 / 5 exactly
        area[torch.rand(K, generator=g) < 0.05] = 0
        orig[torch.rand(K, generator=g) < 0.05] = 0
        cases[f"random{i}"] = dict(scores=sc, labels=lab, area=area.numpy().astype(np.int32), orig=orig.numpy().astype(np.int32),
                                   score_thr=SCORE_THR, overlap_thr=OVERLAP_THR)
    below, above = float(np.nextafter(thr32, f32(0))), float(np.nextafter(thr32, f32(1)))
    # a thing scoring exactly float32(0.3) is NOT below 0.3 (the test is in fp32), one fp32 ulp below it is; stuff has no score test
    cases["score_at_thr"] = _rows((float(thr32), 2, 50, 60), (below, 3, 50, 60), (above, 4, 50, 60), (below, NT + 1, 50, 60),
                                  (0.9, 0, 40, 41))
    # area / orig exactly 0.6 (3 / 5 is the double nearest 0.6): kept at overlap_thr 0.6 and one ulp below, rejected one ulp above
    # -- two int32 counts cannot give a quotient within 1e-10 of 0.6 without being 3 : 5, so the ulp is put on the threshold,
    # which the ABI takes as a double for exactly this reason
    ratio = [(0.9, 1, 3, 5), (0.8, NT + 2, 600, 1000), (0.7, 2, 599, 1000), (0.6, NT, 601, 1000), (0.5, 3, 3 << 20, 5 << 20)]
    for name, thr in (("ratio_at_thr", 0.6), ("ratio_thr_ulp_up", math.nextafter(0.6, 1.0)), ("ratio_thr_ulp_down", math.nextafter(0.6, 0.0))):
        cases[name] = dict(_rows(*ratio), overlap_thr=thr)
    cases["zero_counts"] = _rows((0.9, 1, 10, 0), (0.8, 2, 0, 10), (0.7, NT + 1, 0, 0), (0.6, NT + 2, 7, 7), (0.5, 0, 1, 1))
    cases["equal_scores"] = _rows((0.5, 1, 9, 9), (0.75, NT + 1, 9, 9), (0.5, NT + 2, 9, 9), (0.75, 2, 9, 9), (0.5, 3, 9, 9), (0.75, 4, 1, 9),
                                  (0.0, NT + 3, 5, 5), (-0.0, NT + 4, 5, 5), (0.0, NT + 5, 5, 5))
    cases["all_rejected"] = _rows((0.1, 1, 9, 9), (0.9, NT, 1, 9), (0.2, 2, 9, 9))
    for name, c in cases.items():                   # pad with rejected rows: one K for all
        n = len(c["scores"])
        if n < K:
            c["scores"] = torch.cat([c["scores"], torch.zeros(K - n)])
            c["labels"] = torch.cat([c["labels"], torch.zeros(K - n, dtype=torch.int64)])
            c["area"] = np.concatenate([c["area"], np.zeros(K - n, np.int32)])
            c["orig"] = np.concatenate([c["orig"], np.zeros(K - n, np.int32)])
    return cases


def host_accept(c):
    return Pn.accept_loop(c["scores"], c["labels"], c["area"], c["orig"], NT, c["score_thr"], c["overlap_thr"])


def record_row(c, newid, info):
    """the record row ph_panoptic_merge writes for a frame, built by hand from accept_loop's own output: nseg | seg[K][4] =
    {new id, k, label, area} in id order, unused rows zero | scores as fp32 bits"""
    K = len(newid)
    row = np.zeros(1 + 5 * K, dtype=np.int32)
    row[0] = len(info)
    seg = row[1:1 + 4 * K].reshape(K, 4)
    for s in info:
        k = int(np.flatnonzero(newid == s["id"])[0])
        seg[s["id"] - 1] = (s["id"], k, int(c["labels"][k]), int(c["area"][k]))
    row[1 + 4 * K:] = c["scores"].numpy().view(np.int32)
    return row


def test_segments_from_records_reproduces_accept_loop():
    cases = accept_cases()
    assert sum(n.startswith("random") for n in cases) >= 300
    kept = 0
    for name, c in cases.items():
        newid, info = host_accept(c)
        got = Pn.segments_from_records(record_row(c, newid, info), len(newid), NT)
        assert got == info, name
        for a, b in zip(got, info):                # the same Python types, not merely equal values
            assert [(k, type(v)) for k, v in a.items()] == [(k, type(v)) for k, v in b.items()], name
        kept += len(info)
    assert kept > 1000                              # the draws keep and reject in quantity


def test_crafted_rows_decide_as_documented():
    cases = accept_cases()
    nid = lambda name, n: host_accept(cases[name])[0][:n].tolist()
    assert nid("score_at_thr", 5) == [3, 0, 2, 4, 1]          # fp32(0.3) kept, one ulp below rejected for a thing, kept for stuff
    assert nid("ratio_at_thr", 5) == [1, 2, 0, 3, 4]
    assert nid("ratio_thr_ulp_down", 5) == [1, 2, 0, 3, 4]
    assert nid("ratio_thr_ulp_up", 5) == [0, 0, 0, 1, 0]      # exactly 0.6 is below nextafter(0.6, 1)
    assert nid("zero_counts", 5) == [0, 0, 0, 1, 2]
    assert nid("equal_scores", 9) == [3, 1, 4, 2, 5, 0, 6, 7, 8]   # ties (and +0 / -0) by ascending index
    assert nid("all_rejected", 3) == [0, 0, 0]


def test_nan_and_signed_zero_order_of_the_stable_descending_sort():
    """what k_pan_accept ranks by: torch.argsort(-scores, stable=True) puts NaN LAST (after -inf) and treats +0 / -0 as a tie"""
    s = torch.tensor([0.5, float("nan"), 0.7, 0.0, -0.0, 0.7, float("inf"), -float("inf"), float("nan")])
    assert torch.argsort(-s, stable=True).tolist() == [6, 2, 5, 0, 3, 4, 7, 1, 8]
    c = _rows(*[(float(v), NT + 1, 5, 5) for v in s])
    newid, info = host_accept(c)
    assert newid.tolist() == [4, 8, 2, 5, 6, 3, 1, 7, 9]       # a NaN-scored stuff segment is kept, numbered last
    got = Pn.segments_from_records(record_row(c, newid, info), len(newid), NT)
    assert got == info


def test_workspace_query():
    lib = _lib.load()
    geom = (C.c_int32 * 8)(256, 512, 1024, 2048, 1024, 2048, 1024, 2048)
    al = lambda n: (n + 255) // 256 * 256
    B, K, hw, npx = 4, 111, 256 * 512, 1024 * 2048
    want = al(B * 5 * K * 4) + 2 * al(B * K * hw * 4) + al(B * hw * 4) + al(B * npx * 4) + al(B * K * 4)
    assert lib.ph_panoptic_merge_workspace_bytes(B, K, 256, 512, geom) == want
    assert lib.ph_panoptic_merge_workspace_bytes(0, K, 256, 512, geom) == 0 and "bad size" in Hh.last_error()
    assert lib.ph_panoptic_merge_workspace_bytes(B, K, 0, 512, geom) == 0 and "bad size" in Hh.last_error()
    assert lib.ph_panoptic_merge_workspace_bytes(B, K, 128, 512, geom) == 0 and "bad geometry" in Hh.last_error()      # geom[0] != h2
    assert lib.ph_panoptic_merge_workspace_bytes(B, 5000, 256, 512, geom) == 0 and "4096 candidates" in Hh.last_error()
    assert lib.ph_panoptic_merge_workspace_bytes(B, K, 256, 512, None) == 0 and "geom" in Hh.last_error()
    bad = (C.c_int32 * 8)(256, 512, 1024, 2048, 1025, 2048, 1024, 2048)                                         # img_shape > batch shape
    assert lib.ph_panoptic_merge_workspace_bytes(B, K, 256, 512, bad) == 0 and "bad geometry" in Hh.last_error()


_MERGE_ARG_CHECKS = r"""
import ctypes as C, sys
sys.path.insert(0, ".")
import torch
from polyphonicformer_amd import _lib
assert torch.cuda.device_count() == 0, "the argument checks need a process without a visible GPU"
lib = _lib.load()
FAKE = C.c_void_p(1 << 40)
msg = lambda: lib.ph_last_error_string().decode()
geom = (C.c_int32 * 8)(64, 128, 256, 512, 256, 512, 256, 512)
K = 100 + 11
need = lib.ph_panoptic_merge_workspace_bytes(2, K, 64, 128, geom)
assert need > 0
def call(**kw):
    a = dict(cls=FAKE, dtype=_lib.PH_OUT_F32, B=2, N=111, L=19, P=100, T=8, M=100, h2=64, w2=128, geom=geom, mode=0, ws=FAKE,
             nbytes=need, pan=FAKE)
    a.update(kw)
    return lib.ph_panoptic_merge(a["cls"], FAKE, FAKE, a["dtype"], FAKE, a["B"], a["N"], a["L"], a["P"], a["T"], a["M"], a["h2"], a["w2"],
                                 a["geom"], a["mode"], 0.3, 0.6, a["ws"], a["nbytes"], a["pan"], FAKE, FAKE, FAKE, None)
assert call(nbytes=need - 1) == -4 and "workspace too small" in msg(), msg()
assert call(nbytes=0) == -4 and "workspace too small" in msg(), msg()
assert call(cls=None) == -1 and "null pointer" in msg(), msg()
assert call(pan=None) == -1 and "null pointer" in msg(), msg()
assert call(B=0) == -1, msg()
assert call(P=200) == -1 and "head geometry" in msg(), msg()
assert call(M=900) == -1 and "max_per_img" in msg(), msg()
assert call(dtype=7) == -1 and "dtype" in msg(), msg()
assert call(mode=2) == -1 and "depth mode" in msg(), msg()
assert call(h2=32) == -1 and "bad geometry" in msg(), msg()
assert call(N=5000, L=5000, P=2, T=2, M=4) == -2 and "4096 candidates" in msg(), msg()
assert call(ws=C.c_void_p((1 << 40) + 8)) == -1 and "256-byte aligned" in msg(), msg()
# the single kernels' new entry points check before they launch, too
assert lib.ph_panoptic_accept(FAKE, FAKE, FAKE, 5 * K, 2, 5000, 8, 0.3, 0.6, FAKE, K, FAKE, FAKE, 1 + 5 * K, None) == -1 and "K" in msg()
assert lib.ph_panoptic_accept(FAKE, FAKE, FAKE, 5 * K, 2, K, 8, 0.3, 0.6, FAKE, K, FAKE, FAKE, K, None) == -1 and "stride" in msg()
assert lib.ph_panoptic_accept(FAKE, FAKE, None, 5 * K, 2, K, 8, 0.3, 0.6, FAKE, K, FAKE, FAKE, 1 + 5 * K, None) == -1
assert lib.ph_panoptic_activate_batch(FAKE, FAKE, 0, FAKE, FAKE, 3, 2, 111, K, 64, 128, 0, FAKE, FAKE, FAKE, None) == -1 and "stride" in msg()
assert lib.ph_panoptic_argmax_batch(FAKE, FAKE, 5 * K, 2, K, geom, 0, 0, FAKE, FAKE, K, None) == -1 and "stride" in msg()
assert lib.ph_panoptic_paste_batch(FAKE, FAKE, 1, FAKE, FAKE, 2, K, geom, 0, FAKE, FAKE, FAKE, None) == -1 and "stride" in msg()
print("merge checks ok")
"""


def test_merge_refuses_bad_arguments_before_anything_is_launched():
    """a too small workspace is PH_EWORKSPACE, bad sizes PH_EINVAL / PH_EUNSUPPORTED, with a message -- returned before the first
    launch: the pointers are fake, and the child process sees no GPU, so a check that came too late would fail on the host"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _MERGE_ARG_CHECKS], cwd=os.path.dirname(BLD.HERE), env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "merge checks ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
