"""GPU: the launch-only panoptic merge (ph_panoptic_accept, the batched kernels, ph_panoptic_merge, panoptic.BatchMerge,
panoptic.get_panoptic_batch, KernelUpdateIterHead.use_device_merge).  Everything is compared BIT-EXACT, no tolerances:
the accept kernel against panoptic.accept_loop, the batched kernels at B = 1 against the single-frame calls, the batched
merge against DeviceMerge / get_panoptic / the oracle / the reference's golden id maps."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import helpers as Hh
from oracle import poly_oracle as O
from polyphonicformer_amd import _lib, panoptic as Pn
from test_gpu_panoptic import CFG, _Head, _case, _golden
from test_panoptic_accept import NT, accept_cases, host_accept

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
NQ, K = CFG["Nq"], CFG["Nq"] + CFG["n_stuff"]
CASES = ["a", "b", "c", "d", "e"]


def _i32(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


# ---- 3. the accept step --------------------------------------------------------------------------------------------------
def test_accept_kernel_equals_accept_loop(gpu):
    """ph_panoptic_accept against panoptic.accept_loop on the CPU test's inputs, three different frames per launch, laid out as
    select / argmax leave them (pack row: q | labels | scores | counts [2][K]) and written as ph_panoptic_merge's records"""
    lib = _lib.load()
    cases = accept_cases()
    names = sorted(cases)
    names += names[: (-len(names)) % 3]
    Kc = len(cases[names[0]]["scores"])
    groups = {}
    for n in names:                                     # the thresholds are per call: batch cases that share them
        groups.setdefault((cases[n]["score_thr"], cases[n]["overlap_thr"]), []).append(n)
    done = 0
    for (sthr, othr), members in groups.items():
        members += members[: (-len(members)) % 3]
        for i in range(0, len(members), 3):
            trio = [cases[n] for n in members[i:i + 3]]
            pack = torch.zeros((3, 5 * Kc), dtype=torch.int32)
            for b, c in enumerate(trio):
                pack[b, Kc:2 * Kc] = c["labels"].int()
                pack[b, 2 * Kc:3 * Kc] = c["scores"].view(torch.int32)
                pack[b, 3 * Kc:4 * Kc] = torch.from_numpy(c["area"])
                pack[b, 4 * Kc:] = torch.from_numpy(c["orig"])
            pd = pack.to(gpu)
            newid = torch.full((3, Kc), -9, dtype=torch.int32, device=gpu)
            rec = torch.full((3, 1 + 5 * Kc), -9, dtype=torch.int32, device=gpu)
            _lib.check(lib.ph_panoptic_accept(_i32(pd, Kc), _i32(pd, 2 * Kc), _i32(pd, 3 * Kc), 5 * Kc, 3, Kc, NT, sthr, othr, _i32(newid), Kc,
                                              _i32(rec), _i32(rec, 1), 1 + 5 * Kc, _lib.stream_ptr()), "ph_panoptic_accept")
            nh, rh = newid.cpu(), rec.cpu()
            for b, c in enumerate(trio):
                want_id, want_info = host_accept(c)
                assert torch.equal(nh[b], torch.from_numpy(want_id)), members[i + b]
                assert int(rh[b, 0]) == len(want_info), members[i + b]
                row = rh[b].numpy().copy()
                assert (row[1 + 4 * Kc:] == -9).all()                       # the public call leaves the score slots alone
                row[1 + 4 * Kc:] = c["scores"].numpy().view(np.int32)
                assert Pn.segments_from_records(row, Kc, NT) == want_info, members[i + b]
                seg = row[1:1 + 4 * Kc].reshape(Kc, 4)
                assert not seg[len(want_info):].any(), members[i + b]       # unused rows are zero
                done += 1
    assert done >= len(cases)


def test_accept_kernel_ranks_nan_last(gpu):
    """NaN scores rank where torch.argsort(-scores, stable=True) puts them: last, after -inf; +0 and -0 tie"""
    lib = _lib.load()
    s = torch.tensor([0.5, float("nan"), 0.7, 0.0, -0.0, 0.7, float("inf"), -float("inf"), float("nan")])
    n = len(s)
    pack = torch.zeros((1, 5 * n), dtype=torch.int32)
    pack[0, n:2 * n] = NT + 1
    pack[0, 2 * n:3 * n] = s.view(torch.int32)
    pack[0, 3 * n:] = 5
    pd = pack.to(gpu)
    newid = torch.empty((1, n), dtype=torch.int32, device=gpu)
    rec = torch.empty((1, 1 + 5 * n), dtype=torch.int32, device=gpu)
    _lib.check(lib.ph_panoptic_accept(_i32(pd, n), _i32(pd, 2 * n), _i32(pd, 3 * n), 5 * n, 1, n, NT, 0.3, 0.6, _i32(newid), n, _i32(rec),
                                      _i32(rec, 1), 1 + 5 * n, _lib.stream_ptr()), "ph_panoptic_accept")
    want, _ = Pn.accept_loop(s, torch.full((n,), NT + 1), np.full(n, 5), np.full(n, 5), NT, 0.3, 0.6)
    assert want.tolist() == [4, 8, 2, 5, 6, 3, 1, 7, 9]
    assert newid.cpu()[0].tolist() == want.tolist() and int(rec.cpu()[0, 0]) == n


# ---- 4. / 5. / 10. the batched merge on the fixtures -------------------------------------------------------------------------
def _two_frames(case, dtype, gpu, ramp):
    """a batch of two different frames from a fixture, as test_device_select_and_device_merge_equal_the_host_form builds it;
    ramp: that test's tie-breaking ramp on the class scores"""
    z = _golden(case)
    cls, m_up, d_up, d0_up, meta = _case(z, case)
    if ramp:
        cls = (cls.double() * 0.98 + 1e-6 * torch.arange(cls.numel(), dtype=torch.float64).reshape(cls.shape)).float()
    cls2 = torch.stack([cls, cls.flip(0).roll(3, 1) * 0.5 + 0.25 * cls])
    mm, dd, d0 = (torch.stack([t, t.flip(-1)]) for t in (m_up, d_up, d0_up))
    mm, dd = mm.to(dtype), dd.to(dtype)
    return cls2, mm, dd, d0, meta, (cls2.to(gpu).contiguous(), mm.to(gpu), dd.to(gpu), d0.to(gpu))


def _device_merge_results(c, mm, dd, d0, meta):
    dm = Pn.DeviceMerge(_Head, c, mm, dd, d0, meta)
    dm.begin(c, mm, dd, d0)
    dm.download()
    torch.cuda.synchronize()
    return [dm.finish(b) for b in range(c.shape[0])]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CASES)
def test_batch_merge_equals_device_merge(gpu, case, dtype):
    """BatchMerge (one native call, accept on the device) = DeviceMerge (accept loop on the host) on the fixtures as they are,
    exact score ties included: both paths share ph_panoptic_select"""
    _, _, _, _, meta, (c, mm, dd, d0) = _two_frames(case, dtype, gpu, ramp=False)
    bm = Pn.BatchMerge(_Head, 2, c.shape[1], c.shape[2], mm.shape[2], mm.shape[3], dtype, meta, gpu)
    bm.run(c, mm, dd, d0)
    bm.download()
    torch.cuda.synchronize()
    got, want = bm.results_device(), _device_merge_results(c, mm, dd, d0, meta)
    nseg = 0
    for b in range(2):
        pan, info, d_basic, d_final = got[b]
        pan2, info2, d_basic2, d_final2 = want[b]
        assert torch.equal(pan, pan2) and torch.equal(d_basic, d_basic2) and torch.equal(d_final, d_final2), (case, b)
        assert info == info2, (case, b)
        nseg += len(info)
    assert nseg > 0
    # results(): the same on the host, in the reference's tuple
    for b, r in enumerate(bm.results()):
        assert r[0] is None and r[1] is None and r[2][0].dtype == np.int32
        assert np.array_equal(r[2][0], want[b][0].cpu().numpy()) and r[2][1] == want[b][1]
        assert np.array_equal(r[3], want[b][2].cpu().numpy()) and np.array_equal(r[4], want[b][3].cpu().numpy())


@pytest.mark.parametrize("case", CASES)
def test_get_panoptic_batch_vs_oracle_and_per_frame(gpu, case):
    """ramped class scores (no exact ties, so that the host's topk order is defined): get_panoptic_batch against the oracle on
    the same inputs (id maps, segment lists, stuff areas) and against get_panoptic per frame (everything, bit for bit)"""
    cls2, mm, dd, d0, meta, (c, gm, gd, g0) = _two_frames(case, torch.float32, gpu, ramp=True)
    res = Pn.get_panoptic_batch(_Head, c, gm, gd, g0, [meta, meta])
    assert len(res) == 2
    key = lambda s: (s["id"], s["isthing"], s["category_id"], s.get("instance_id"))
    for b in range(2):
        assert res[b][0] is None and res[b][1] is None
        pan, info = res[b][2]
        pan_ref, info_ref, _, _ = O.get_panoptic(cls2[b], mm[b], dd[b], d0[b], meta, NQ, CFG["n_thing"], NQ)
        bad = int((pan != pan_ref).sum())
        print(f"batched merge case {case} frame {b}: {bad} of {pan.size} pixels differ from the oracle's id map")
        assert pan.dtype == np.int32 and np.array_equal(pan, pan_ref)
        assert [key(s) for s in info] == [key(s) for s in info_ref]
        for x, y in zip(info, info_ref):
            if not x["isthing"]:
                assert x["area"] == y["area"]
        one = Pn.get_panoptic(_Head, c[b], gm[b], gd[b], g0[b], meta)
        assert np.array_equal(pan, one[2][0]) and info == one[2][1]
        assert np.array_equal(res[b][3], one[3]) and np.array_equal(res[b][4], one[4])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CASES)
def test_raw_c_abi_merge(gpu, case, dtype):
    """ph_panoptic_merge through ctypes with no head object: plain device tensors, a workspace of exactly
    ph_panoptic_merge_workspace_bytes with a guard region behind it; result = DeviceMerge's, guard untouched"""
    lib = _lib.load()
    _, _, _, _, meta, (c, mm, dd, d0) = _two_frames(case, dtype, gpu, ramp=False)
    B, N, L = c.shape
    h2, w2 = mm.shape[-2:]
    geom, (Ho, Wo) = Pn._geom((h2, w2), meta)
    need = lib.ph_panoptic_merge_workspace_bytes(B, K, h2, w2, geom)
    assert need > 0 and need % 256 == 0
    guard = 4096
    buf = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=gpu)
    assert buf.data_ptr() % 256 == 0
    pan = torch.full((B, Ho, Wo), -3, dtype=torch.int32, device=gpu)
    d_basic, d_final = torch.zeros((B, Ho, Wo), device=gpu), torch.zeros((B, Ho, Wo), device=gpu)
    rec = torch.full((B, 1 + 5 * K), -3, dtype=torch.int32, device=gpu)
    d0c = d0.reshape(B, h2, w2).contiguous()
    code = {torch.float32: _lib.PH_OUT_F32, torch.bfloat16: _lib.PH_OUT_BF16}[dtype]
    rc = lib.ph_panoptic_merge(_lib.ptr(c), _lib.ptr(mm), _lib.ptr(dd), code, _lib.ptr(d0c), B, N, L, NQ, CFG["n_thing"], NQ, h2, w2, geom, 0,
                               0.3, 0.6, _lib.ptr(buf), need, _lib.ptr(pan), _lib.ptr(d_basic), _lib.ptr(d_final), _lib.ptr(rec),
                               _lib.stream_ptr())
    assert rc == 0, lib.ph_last_error_string()
    torch.cuda.synchronize()
    assert bool((buf[need:] == 0xA5).all()), "the merge wrote behind its workspace"
    want = _device_merge_results(c, mm, dd, d0, meta)
    rh = rec.cpu().numpy()
    for b in range(B):
        assert torch.equal(pan[b], want[b][0]) and torch.equal(d_basic[b], want[b][2]) and torch.equal(d_final[b], want[b][3])
        assert Pn.segments_from_records(rh[b], K, CFG["n_thing"]) == want[b][1]


# ---- 6. the batched kernels at B = 1 (and B = 2) against the single-frame calls ----------------------------------------------
def _geoms(sh, sw, cut_h, cut_w):
    """the x4 geometry of test_argmax_x4_form_equals_the_generic_kernel and a generic one on the same source map (padded batch
    shape, crop, a second resize with non-integer factors)"""
    Ho, Wo = 4 * sh - cut_h, 4 * sw - cut_w
    x4 = ((C.c_int32 * 8)(sh, sw, 4 * sh, 4 * sw, Ho, Wo, Ho, Wo), (Ho, Wo))
    Hb, Wb = 4 * sh + 3, 4 * sw + 5
    h, w = max(Hb - 2 - cut_h, 1), max(Wb - 3 - cut_w, 1)
    oh, ow = (3 * h + 1) // 2, (3 * w + 1) // 2
    return {"x4": x4, "generic": ((C.c_int32 * 8)(sh, sw, Hb, Wb, h, w, oh, ow), (oh, ow))}


@pytest.mark.parametrize("form", ["x4", "generic"])
@pytest.mark.parametrize("shape", [(24, 40, 0, 0), (17, 23, 3, 2), (8, 16, 1, 3), (1, 1, 0, 0), (64, 128, 0, 0)])
def test_batched_kernels_equal_the_single_frame_calls(gpu, shape, form):
    lib, s = _lib.load(), _lib.stream_ptr
    sh, sw, cut_h, cut_w = shape
    geom, (Ho, Wo) = _geoms(sh, sw, cut_h, cut_w)[form]
    Kk, N, B = 70, 83, 2
    g = torch.Generator().manual_seed(sh * 131 + sw)
    e = lambda shp, dt, fill=None: (torch.empty(shp, dtype=dt, device=gpu) if fill is None else torch.full(shp, fill, dtype=dt, device=gpu))
    for dtype, code in ((torch.float32, _lib.PH_OUT_F32), (torch.bfloat16, _lib.PH_OUT_BF16)):
        m_up = (torch.randn(B, N, sh, sw, generator=g) * 3).to(dtype).to(gpu)
        d_up = torch.randn(B, N, sh, sw, generator=g).to(dtype).to(gpu)
        d0 = torch.randn(B, sh, sw, generator=g).to(gpu)
        q = torch.stack([torch.randperm(N, generator=g)[:Kk] for _ in range(B)]).int().to(gpu)
        # activate
        one = [[e((Kk, sh, sw), torch.float32), e((Kk, sh, sw), torch.float32), e((sh, sw), torch.float32)] for _ in range(B)]
        for b in range(B):
            _lib.check(lib.ph_panoptic_activate(_lib.ptr(m_up[b]), _lib.ptr(d_up[b]), code, _lib.ptr(d0[b]), _lib.ptr(q[b]), Kk, sh, sw, 0,
                                                _lib.ptr(one[b][0]), _lib.ptr(one[b][1]), _lib.ptr(one[b][2]), s()), "activate")
        for nb in (1, 2):
            am, ad, a0 = e((nb, Kk, sh, sw), torch.float32), e((nb, Kk, sh, sw), torch.float32), e((nb, sh, sw), torch.float32)
            _lib.check(lib.ph_panoptic_activate_batch(_lib.ptr(m_up), _lib.ptr(d_up), code, _lib.ptr(d0), _lib.ptr(q), Kk, nb, N, Kk, sh, sw, 0,
                                                      _lib.ptr(am), _lib.ptr(ad), _lib.ptr(a0), s()), "activate_batch")
            for b in range(nb):
                assert torch.equal(am[b], one[b][0]) and torch.equal(ad[b], one[b][1]) and torch.equal(a0[b], one[b][2]), (dtype, nb, b)
    # argmax: maps with exact ties, exact 0.5s and a NaN, as the x4 test has them
    act = torch.rand(B, Kk, sh, sw, generator=g)
    act[:, :, : sh // 2] = (act[:, :, : sh // 2] * 8).round() / 8
    act[0, 3, 0, 0] = float("nan")
    sc = torch.rand(B, Kk, generator=g)
    sc[:, 5] = sc[:, 4]
    a, scd = act.to(gpu).contiguous(), sc.to(gpu)
    dep, dep0 = (torch.rand(B, Kk, sh, sw, generator=g) * 80).to(gpu), (torch.rand(B, sh, sw, generator=g) * 80).to(gpu)
    newid = torch.randint(0, 3, (B, Kk), generator=g).int()
    newid = (newid * torch.arange(1, Kk + 1).int()).to(gpu)            # a third of the candidates rejected
    for generic_only in ((0, 1) if form == "x4" else (0,)):
        ref = []
        for b in range(B):
            ids, cnt = e((Ho, Wo), torch.int32, -7), e((2, Kk), torch.int32, -7)
            with _lib.switches(pan_generic=generic_only):              # the single-frame call's switch; the batched call has a flag
                _lib.check(lib.ph_panoptic_argmax(_lib.ptr(a[b]), _lib.ptr(scd[b]), Kk, geom, 0, _lib.ptr(ids), _lib.ptr(cnt), s()), "argmax")
            pan, db, df = e((Ho, Wo), torch.int32, -7), e((Ho, Wo), torch.float32, -7), e((Ho, Wo), torch.float32, -7)
            _lib.check(lib.ph_panoptic_paste(_lib.ptr(ids), _lib.ptr(newid[b]), _lib.ptr(dep[b]), _lib.ptr(dep0[b]), geom, 0, _lib.ptr(pan),
                                             _lib.ptr(db), _lib.ptr(df), s()), "paste")
            ref.append((ids, cnt, pan, db, df))
            assert int(cnt[0].sum()) == Ho * Wo and int(ids.min()) >= 0 and int(ids.max()) < Kk
        for nb in (1, 2):
            ids, cnt = e((nb, Ho, Wo), torch.int32, -7), e((nb, 2, Kk), torch.int32, -7)
            _lib.check(lib.ph_panoptic_argmax_batch(_lib.ptr(a), _lib.ptr(scd), Kk, nb, Kk, geom, 0, generic_only, _lib.ptr(ids), _lib.ptr(cnt),
                                                    2 * Kk, s()), "argmax_batch")
            pan, db, df = e((nb, Ho, Wo), torch.int32, -7), e((nb, Ho, Wo), torch.float32, -7), e((nb, Ho, Wo), torch.float32, -7)
            _lib.check(lib.ph_panoptic_paste_batch(_lib.ptr(ids), _lib.ptr(newid), Kk, _lib.ptr(dep), _lib.ptr(dep0), nb, Kk, geom, 0,
                                                   _lib.ptr(pan), _lib.ptr(db), _lib.ptr(df), s()), "paste_batch")
            for b in range(nb):
                for got, want, what in zip((ids[b], cnt[b], pan[b], db[b], df[b]), ref[b], ("ids", "counts", "pan", "depth_basic", "depth_final")):
                    assert torch.equal(got, want), (what, generic_only, nb, b)


# ---- 7. mixed geometries -------------------------------------------------------------------------------------------------
def test_get_panoptic_batch_groups_frames_by_geometry(gpu):
    """frames of three geometries interleaved (fixtures a, b and d share the 24 x 48 logit maps): results come back in frame order
    and equal per-frame get_panoptic"""
    za, zd = _golden("a"), _golden("d")
    parts = [_case(za, "a"), _case(za, "b"), _case(zd, "d")]
    ramp = lambda cls, k: (cls.double() * (0.98 - 0.01 * k) + 1e-6 * torch.arange(cls.numel(), dtype=torch.float64).reshape(cls.shape)).float()
    order = [0, 1, 0, 2, 1, 0]
    cls = torch.stack([ramp(parts[p][0], i) for i, p in enumerate(order)]).to(gpu)
    mm = torch.stack([parts[p][1] if i % 2 == 0 else parts[p][1].flip(-1) for i, p in enumerate(order)]).to(gpu)
    dd = torch.stack([parts[p][2] if i % 2 == 0 else parts[p][2].flip(-1) for i, p in enumerate(order)]).to(gpu)
    d0 = torch.stack([parts[p][3] for p in order]).to(gpu)
    metas = [parts[p][4] for p in order]
    assert len({Pn._geom_key(m) for m in metas}) == 3
    res = Pn.get_panoptic_batch(_Head, cls, mm, dd, d0, metas)
    assert len(res) == len(order)
    shapes = set()
    for b, meta in enumerate(metas):
        one = Pn.get_panoptic(_Head, cls[b], mm[b], dd[b], d0[b], meta)
        assert res[b][2][0].shape == tuple(meta["ori_shape"][:2])
        assert np.array_equal(res[b][2][0], one[2][0]) and res[b][2][1] == one[2][1], b
        assert np.array_equal(res[b][3], one[3]) and np.array_equal(res[b][4], one[4]), b
        assert len(one[2][1]) > 0
        shapes.add(res[b][2][0].shape)
    assert len(shapes) == 3


# ---- 8. graph capture ----------------------------------------------------------------------------------------------------
def test_batch_merge_is_capturable(gpu):
    """BatchMerge.run captured with torch.cuda.graph on a side stream (a call that synchronised or allocated would fail the
    capture); the static inputs are overwritten with a second batch and the replay equals an eager run on that batch"""
    _, _, _, _, meta, first = _two_frames("a", torch.float32, gpu, ramp=False)
    _, _, _, _, meta_b, second = _two_frames("b", torch.float32, gpu, ramp=True)
    second = tuple(t.flip(0).contiguous() for t in second)                  # another batch on the same logit size
    c, mm, dd, d0 = (t.clone() for t in first)                              # the static inputs
    mk = lambda: Pn.BatchMerge(_Head, 2, c.shape[1], c.shape[2], mm.shape[2], mm.shape[3], torch.float32, meta, gpu)
    bm = mk()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bm.run(c, mm, dd, d0)                                               # warm-up outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        bm.run(c, mm, dd, d0)
    for dst, src in zip((c, mm, dd, d0), second):
        dst.copy_(src)
    for t in (bm.pan, bm.d_basic, bm.d_final, bm.records):
        t.fill_(-1)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    eager = mk()
    eager.run(*second)
    torch.cuda.synchronize()
    assert torch.equal(bm.pan, eager.pan) and torch.equal(bm.d_basic, eager.d_basic) and torch.equal(bm.d_final, eager.d_final)
    assert torch.equal(bm.records, eager.records)
    assert int(eager.records[:, 0].min()) > 0                               # segments were found
    first_run = mk()
    first_run.run(*first)
    torch.cuda.synchronize()
    assert not torch.equal(first_run.pan, eager.pan)                        # and the two batches do differ


# ---- 9. the module switch -------------------------------------------------------------------------------------------------
def test_simple_test_with_device_merge_whole_path_golden(gpu, monkeypatch):
    """test_simple_test_whole_path_golden's fixture with use_device_merge(True): the reference's golden id maps, exactly;
    with the switch off the head does not go near get_panoptic_batch"""
    from test_gpu_parity import _full_weights, _iter_head, _kernel_head
    z = Hh.load_golden("full_panoptic.npz")
    m = json.loads(bytes(z["meta_json"]).decode())
    B, H, W = m["B"], m["H"], m["W"]
    weights = _full_weights()
    kh, ih = _kernel_head(weights, "fp32"), _iter_head(weights, m["cfg"]["S"], precision="fp32")
    assert ih.device_merge is False                                         # the default
    assert ih.use_device_merge(True) is ih and ih.device_merge is True
    feats = [f.to(gpu) for f in Hh.neck_inputs(m["nseed"], B, 256, H, W)]
    metas = [Hh.img_meta(H * 8, W * 8) for _ in range(B)]
    calls = []
    real = Pn.get_panoptic_batch
    monkeypatch.setattr(Pn, "get_panoptic_batch", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    (pf, xf, mp, cs, seg, df, dp, dpr, aspp) = kh.simple_test_rpn(feats, metas)
    res = ih.simple_test(xf, pf, mp, cs, metas, depth_preds=dpr, depth_feats=df, depth_proposal=dp, imgs_whwh=None,
                         aspp_semantic=aspp, rescale=True)
    assert len(res) == B and calls == [1]
    for b in range(B):
        assert res[b][0] is None and res[b][1] is None
        pan, info = res[b][2]
        assert pan.dtype == np.int32 and np.array_equal(pan, z[f"pan{b}"])
        ref_info = json.loads(bytes(z[f"info{b}"]).decode())
        assert [(s["id"], s["category_id"]) for s in info] == [(s["id"], s["category_id"]) for s in ref_info]
    h, w, bh, bw, oh, ow = [int(v) for v in z["geo2_meta"]]
    meta2 = Hh.img_meta(h, w, pad_to=(bh, bw), ori=(oh, ow))
    (pf, xf, mp, cs, seg, df, dp, dpr, aspp) = kh.simple_test_rpn([f[:1] for f in feats], [meta2])
    res2 = ih.simple_test(xf, pf, mp, cs, [meta2], depth_preds=dpr, depth_feats=df, depth_proposal=dp)
    assert np.array_equal(res2[0][2][0], z["pan_geo2"]) and calls == [1, 1]
    # switch off: the old per-image path

    def refuse(*a, **k):
        raise AssertionError("get_panoptic_batch called with the switch off")
    monkeypatch.setattr(Pn, "get_panoptic_batch", refuse)
    ih.use_device_merge(False)
    res3 = ih.simple_test(xf, pf, mp, cs, [meta2], depth_preds=dpr, depth_feats=df, depth_proposal=dp)
    assert np.array_equal(res3[0][2][0], z["pan_geo2"])
    assert res3[0][2][1] == res2[0][2][1] and np.array_equal(res3[0][3], res2[0][3]) and np.array_equal(res3[0][4], res2[0][4])
