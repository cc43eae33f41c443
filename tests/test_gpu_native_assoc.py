"""GPU: the native association plan (csrc/ph_assocplan.hip: ph_track_pack, ph_assoc_plan_run, ph_assoc_plan_match) against the Python
chain it replaces (video.VideoAssociator, track_head.QuasiDenseMaskEmbedHeadGTMask), the single-frame kernels, the oracle
(oracle/video_oracle.py) and the reference's goldens (tests/golden/video.npz).

Shapes: id maps of 64 x 128 (W % 8 == 0: the box kernels' 8-pixel path) and 37 x 50 (the scalar path), FPN levels at strides 4, 8,
16, 32 of the map, K = 24 record rows, the shipped track head (4 convs, 1024, 256) with seeded weights whose GroupNorm gains and
biases are not 1 / 0 (helpers.seeded_fill)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import helpers as Hh
from oracle import video_oracle as VO
from polyphonicformer_amd import _lib, engine as E, track_head as T, video as V
from polyphonicformer_amd.panoptic import segments_from_records
from polyphonicformer_amd.registry import HEADS

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

K, N_THING, N_STUFF = 24, 8, 11
SHAPES = [(64, 128), (37, 50)]
TRACKER_CFG = dict(init_score_thr=0.35, obj_score_thr=0.3, match_score_thr=0.5, memo_tracklet_frames=5, memo_backdrop_frames=1,
                   memo_momentum=0.8, nms_conf_thr=0.5, nms_backdrop_iou_thr=0.3, nms_class_iou_thr=0.7, with_cats=True,
                   match_metric="bisoftmax")
SENTINEL = -123.25


@functools.lru_cache(maxsize=None)
def _head(precision, num_convs=4, fc_out=1024, embed=256):
    shapes = {k: v for k, v in Hh.TRACK_HEAD_SHAPES.items() if not k.startswith("track_head.convs.") or int(k.split(".")[2]) < num_convs}
    shapes.update({"track_head.fcs.0.weight": (fc_out, 12544), "track_head.fcs.0.bias": (fc_out,),
                   "track_head.fc_embed.weight": (embed, fc_out), "track_head.fc_embed.bias": (embed,)})
    sd = Hh.seeded_fill(shapes, 4321)
    head = HEADS.build(dict(type="QuasiDenseMaskEmbedHeadGTMask", num_convs=num_convs, num_fcs=1, fc_out_channels=fc_out,
                            embed_channels=embed, norm_cfg=dict(type="GN", num_groups=32)))
    head.load_state_dict({k[len("track_head."):]: v for k, v in sd.items()})
    head.to("cuda:0").eval()
    head.precision = precision
    return head


@functools.lru_cache(maxsize=None)
def _pack(precision):
    head = _head(precision)
    return E.native_track_pack(head, E.native_track_cfg(head), torch.device("cuda:0"))


def _plan(precision, B, hw, cap, levels):
    cfg = E.native_assoc_cfg(B, hw, K, cap, N_THING, N_STUFF, [tuple(f.shape[-2:]) for f in levels], _pack(precision).cfg)
    return E.NativeAssocPlan(_pack(precision), cfg, torch.device("cuda:0"))


def _records(segs, seed=0):
    """one ph_panoptic_merge record row (int32 [1 + 5 K]) from [(label, score)] in id order: ids 1 .. n, candidate indices a seeded
    permutation of 0 .. K - 1, areas arbitrary; the score of a thing sits at scores[candidate index]"""
    rng = np.random.default_rng(seed)
    row = np.zeros(1 + 5 * K, dtype=np.int32)
    cand = rng.permutation(K)
    scores = rng.uniform(0.05, 0.25, K).astype(np.float32)
    row[0] = len(segs)
    for i, (label, score) in enumerate(segs):
        row[1 + 4 * i:5 + 4 * i] = (i + 1, cand[i], label, 10 + i)
        scores[cand[i]] = np.float32(score)
    row[1 + 4 * K:] = scores.view(np.int32)
    return row


def _frame(hw, labels, seed):
    """a crafted frame: an id map with len(labels) blobs (ids 1 .. n, consecutive), its record row, its four FPN levels"""
    H, W = hw
    pan, info, feats, _ = Hh.video_case(seed=seed, H=H, W=W, nseg=len(labels) + 3)
    ids = [i for i in np.unique(pan) if i > 0][:len(labels)]
    assert len(ids) == len(labels), "the crafted map lost segments: choose another seed"
    out = np.zeros_like(pan)
    for new, old in enumerate(ids):
        out[pan == old] = new + 1
    g = torch.Generator().manual_seed(seed)
    scores = (0.4 + 0.6 * torch.rand(len(labels), generator=g)).tolist()
    return out, _records(list(zip(labels, scores)), seed), feats


def _batch(frames, gpu):
    pan = torch.from_numpy(np.stack([f[0] for f in frames])).to(gpu)
    rec = torch.from_numpy(np.stack([f[1] for f in frames])).to(gpu)
    levels = [torch.cat([f[2][l] for f in frames], 0).to(gpu).contiguous() for l in range(4)]
    return pan, rec, levels


def _python_record(precision, frame, gpu):
    """VideoAssociator.record on one frame: (seg_ids, (bboxes, labels, embeds) or None)"""
    pan, row, feats = frame
    assoc = V.VideoAssociator(_head(precision), TRACKER_CFG, N_THING, N_STUFF)
    info = segments_from_records(row, K, N_THING)
    return assoc.record([f.to(gpu) for f in feats], None, info, torch.from_numpy(pan).to(gpu))


def _table(things, b, cap):
    t = things[b].cpu().numpy()
    n = int(t[0])
    return n, t[1:1 + cap], t[1 + cap:1 + 2 * cap], t[1 + 2 * cap:1 + 7 * cap].view(np.float32).reshape(cap, 5), int(t[-1])


# ---- 1. packing
def _pack_into_poison(head, gpu):
    """ph_track_pack into a buffer filled with 0xA5 (stale bytes cannot pass for padding) -> NativeTrackPack"""
    lib, cfg = _lib.load(), E.native_track_cfg(head)
    params, ptrs = E._gather_params(head, gpu, 3 * cfg.num_convs + 4, lambda i: lib.ph_track_param_name(C.byref(cfg), i),
                                    lambda i: lib.ph_track_param_numel(C.byref(cfg), i))
    blob = torch.full((lib.ph_track_pack_bytes(C.byref(cfg)),), 0xA5, dtype=torch.uint8, device=gpu)
    _lib.check(lib.ph_track_pack(C.byref(cfg), ptrs, _lib.ptr(blob), _lib.stream_ptr()), "ph_track_pack")
    torch.cuda.synchronize()
    return E.NativeTrackPack(blob, cfg)


def _assert_pack_is_get_pack(head, pack, gpu):
    """piece by piece against `_get_pack`; the pieces of the absent convs are empty and every byte outside the pieces is zero"""
    ref, pk, n = head._get_pack(gpu), pack.pk, head.num_convs
    assert pk["P"] == ref["P"] and pk["prec"] == ref["prec"] and len(pk["convs"]) == len(pk["gn"]) == n
    for i in range(n):
        assert pk["convs"][i].shape == ref["convs"][i].shape and torch.equal(pk["convs"][i], ref["convs"][i]), i
        assert torch.equal(pk["gn"][i][0], ref["gn"][i][0]) and torch.equal(pk["gn"][i][1], ref["gn"][i][1]), i
    for k in ("fc", "emb", "fc_b", "emb_b"):
        assert pk[k].shape == ref[k].shape and torch.equal(pk[k], ref[k]), k
    lay = pack.layout
    for i in range(n, _lib.PH_TRACK_MAX_CONVS):
        assert lay.bytes[i] == lay.bytes[_lib.PH_TRACK_MAX_CONVS + i] == lay.bytes[2 * _lib.PH_TRACK_MAX_CONVS + i] == 0, i
    covered = torch.zeros_like(pack.blob, dtype=torch.bool)
    for i in range(_lib.PH_TPACK_COUNT):
        covered[lay.offset[i]:lay.offset[i] + lay.bytes[i]] = True
    assert int(pack.blob[~covered].ne(0).sum()) == 0


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_track_pack_is_get_packs_bytes(gpu, precision):
    head = _head(precision)
    pack = _pack_into_poison(head, gpu)
    _assert_pack_is_get_pack(head, pack, gpu)
    # padding is zero, so a packing into other stale bytes is byte-equal
    assert torch.equal(pack.blob, _pack(precision).blob)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_track_pack_of_a_small_head_is_get_packs_bytes(gpu, precision):
    """2 convs, fc_out_channels 64, embed_channels 32: fc_embed's plain-K fragments with K = 64 (two k-steps) and the 49-tap
    permutation of fcs.0 with sizes other than the default's -- a wrong K / 32 or tap stride cancels nowhere at this size"""
    head = _head(precision, 2, 64, 32)
    _assert_pack_is_get_pack(head, _pack_into_poison(head, gpu), gpu)


# ---- 2. things table
def test_things_table_equals_the_host_walk(gpu):
    """the table depends on the records only (the id maps here are empty); integer for integer and score bit for score bit"""
    cap = 5
    th, st = lambda i: (i % N_THING, 0.3 + 0.05 * i), lambda i: (N_THING + i % N_STUFF, 0.0)
    cases = [[], [st(0), st(1), st(2)], [th(0), th(1), th(2), th(3)], [st(0), th(1), th(2), st(3), st(4), th(5), st(6)],
             [th(0), st(1), th(2), th(3), st(4), th(5), th(6)], [th(0), th(1), st(2), th(3), th(4), th(5), st(6), th(7)]]
    rows = np.stack([_records(c, i) for i, c in enumerate(cases)])
    B, hw = len(cases), (64, 128)
    levels = [torch.zeros(B, 256, 64 // s, 128 // s, device=gpu) for s in (4, 8, 16, 32)]
    plan = _plan("fp32", B, hw, cap, levels)
    plan.things.fill_(-7)
    _, things, _ = plan.run(torch.zeros(B, *hw, dtype=torch.int32, device=gpu), torch.from_numpy(rows).to(gpu), levels)
    for b, c in enumerate(cases):
        info = segments_from_records(rows[b], K, N_THING)
        seg_ids, idxs, labels, score = V.things_for_tracking(None, info)
        n, ids, lab, box, over = _table(things, b, cap)
        want = min(len(seg_ids), cap)
        assert n == want and over == int(len(seg_ids) > cap), (b, n, over)
        assert ids[:n].tolist() == seg_ids[:cap] and lab[:n].tolist() == labels[:cap]
        assert box[:n, 4].view(np.int32).tolist() == np.asarray(score[:cap], dtype=np.float32).view(np.int32).tolist()
        assert not ids[n:].any() and not lab[n:].any() and not box[n:].view(np.int32).any()
        # the semantic table through the painted map of an all-void frame
        assert int(plan.sem[b].min()) == int(plan.sem[b].max()) == N_THING + N_STUFF
    assert [len(V.things_for_tracking(None, segments_from_records(r, K, N_THING))[0]) for r in rows] == [0, 0, 4, 3, 5, 6]


# ---- 3. boxes
@pytest.mark.parametrize("hw", SHAPES)
def test_batched_boxes_equal_the_single_frame_call(gpu, hw):
    frames = [_frame(hw, [0, 9, 3, 3, 12, 7], 5), _frame(hw, [], 6), _frame(hw, [2, 1, 15, 4, 4, 10, 6, 0, 18], 7)]
    frames[1] = (np.zeros(hw, dtype=np.int32), frames[1][1], frames[1][2])
    pan, rec, levels = _batch(frames, gpu)
    plan = _plan("fp32", 3, hw, 12, levels)
    _, things, _ = plan.run(pan, rec, levels)
    assert plan.geometry.vec8 == int(hw[1] % 8 == 0)
    rois_all = plan.rois().cpu()
    for b, (p, row, _) in enumerate(frames):
        nseg = int(row[0])
        n, ids, lab, box, over = _table(things, b, 12)
        if nseg == 0:
            assert n == 0 and rois_all[b].abs().sum() == 0
            continue
        rois1, ext1 = T.segment_boxes(torch.from_numpy(p).to(gpu), nseg)
        assert torch.allclose(rois_all[b, :nseg], rois1.cpu(), atol=2e-3)
        assert torch.equal(torch.from_numpy(box[:n, :4].copy()), ext1.cpu()[ids[:n].astype(np.int64) - 1])
        masks = torch.stack([torch.from_numpy(p == s) for s in range(1, nseg + 1)])
        assert torch.allclose(rois_all[b, :nseg, 1:], VO.mask_stat_boxes(masks).clamp(min=0).float(), atol=2e-3)
        assert torch.equal(torch.from_numpy(box[:n, :4].copy()), VO.mask_extent_boxes(masks).float()[ids[:n].astype(np.int64) - 1])
        # ids above nseg do not occur: the reference's empty-mask conventions, never selected by the table
        assert rois_all[b, nseg:].abs().sum() == 0


# ---- 4. embeddings, same split
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 3, 11])
def test_embeddings_with_cap_equal_n_are_forward_planes_bits(gpu, n, precision):
    labels = []
    for i in range(n):                                           # n things, a stuff segment after every second one
        labels.append((i * 3) % N_THING)
        if i % 2 == 1:
            labels.append(N_THING + i % N_STUFF)
    frame = _frame((64, 128), labels, 30 + n)
    seg_ids, rec = _python_record(precision, frame, gpu)
    pan, rows, levels = _batch([frame], gpu)
    plan = _plan(precision, 1, (64, 128), n, levels)
    _, things_t, emb = plan.run(pan, rows, levels)
    nn, ids, lab, box, over = _table(things_t, 0, n)
    assert nn == n and ids.tolist() == seg_ids and not over
    assert torch.equal(emb[0], rec[2])
    assert torch.equal(torch.from_numpy(box.copy()), rec[0]) and lab.tolist() == rec[1].tolist()


# ---- 5. count and batch invariance
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_embeddings_do_not_depend_on_the_batch_or_the_neighbours(gpu, precision):
    cap, hw = 12, (37, 50)
    A = _frame(hw, [1, 9, 0, 5, 12, 7, 2], 41)                     # 5 things
    N0 = _frame(hw, [10, 11], 42)
    N1 = _frame(hw, [13, 4, 9], 43)
    N12 = _frame(hw, [i % N_THING for i in range(12)], 44)
    alone = None
    for frames, at in (([A], 0), ([A, N0, N12], 0), ([N1, A, N0], 1), ([N12, N1, A], 2)):
        pan, rec, levels = _batch(frames, gpu)
        plan = _plan(precision, len(frames), hw, cap, levels)
        plan.embeds.fill_(SENTINEL)
        _, things, emb = plan.run(pan, rec, levels)
        counts = things[:, 0].tolist()
        assert counts == [sum(int(l) < N_THING for l in f[1][3:3 + 4 * int(f[1][0]):4]) for f in frames]
        for b, nb in enumerate(counts):
            assert bool((emb[b, nb:] == SENTINEL).all()), "rows at or beyond nthing were written"
            assert bool((emb[b, :nb] != SENTINEL).any()) or nb == 0
        if alone is None:
            alone = emb[0, :5].clone()
            assert counts == [5]
        assert torch.equal(emb[at, :5], alone), (len(frames), at)
    assert 12 in counts and 1 in counts


# ---- 6. embeddings against the reference's golden
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_embeddings_against_the_golden(gpu, precision):
    z = Hh.load_golden("video.npz")
    _, _, _, roi_feats = Hh.video_case()
    cap, n, hw = 12, 5, (64, 128)
    frame = _frame(hw, [0, 1, 2, 3, 4], 50)
    pan, rec, levels = _batch([frame], gpu)
    plan = _plan(precision, 1, hw, cap, levels)
    P = plan.geometry.P
    xc = roi_feats[:n].to(gpu).permute(0, 2, 3, 1).reshape(n, 49, 256)
    hi = xc.to(torch.bfloat16)
    pl = [hi.view(torch.int16)] + ([(xc - hi.float()).to(torch.bfloat16).view(torch.int16)] if P == 2 else [])
    planes = torch.full((P, 1, cap, 49, 256), 0x7fc0, dtype=torch.int16, device=gpu)       # NaN beyond the count: never read
    planes[:, 0, :n] = torch.stack(pl, 0)
    _, things, emb = plan.run(pan, rec, levels, roi_planes=planes.contiguous())
    assert int(things[0, 0]) == n
    e = Hh.rel_err(emb[0, :n].cpu(), z["embeds"][:n])
    print("native track embed rel err", precision, e)
    assert e < (1e-3 if precision == "fp32" else 3e-2)


# ---- 7. RoI levels
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_roi_features_on_all_four_levels_vs_oracle(gpu, precision):
    hw = (512, 512)
    pan = np.zeros(hw, dtype=np.int32)
    pan[4:508, 4:508] = 1
    pan[20:320, 20:320] = 2
    pan[340:490, 340:490] = 3
    pan[330:370, 30:70] = 4
    g = torch.Generator().manual_seed(3)
    feats = [torch.randn(1, 256, 512 // s, 512 // s, generator=g) for s in (4, 8, 16, 32)]
    row = _records([(0, 0.9), (1, 0.8), (2, 0.7), (3, 0.6)], 1)
    masks = torch.stack([torch.from_numpy(pan == s) for s in range(1, 5)])
    rois_ref = torch.cat([torch.zeros(4, 1), VO.mask_stat_boxes(masks)], 1).clamp(min=0)
    assert set(VO.map_roi_levels(rois_ref).tolist()) == {0, 1, 2, 3}
    ref = VO.roi_extract(feats, rois_ref)
    p, r, levels = _batch([(pan, row, feats)], gpu)
    plan = _plan(precision, 1, hw, 4, levels)
    plan.run(p, r, levels)
    assert plan.things[0, 0] == 4
    planes = plan.roi_planes()[:, 0]                                                        # [P, 4, 49, 256]
    rec = sum(planes[q].view(torch.bfloat16).float() for q in range(planes.shape[0])).cpu()
    tol = 2e-4 if precision == "fp32" else 5e-3
    assert Hh.rel_err(rec.permute(0, 2, 1).reshape(-1, 256, 7, 7), ref) < tol


# ---- 8, 9, 12. the whole step
def _clip(hw=(64, 128)):
    f0 = _frame(hw, [1, 9, 0, 5, 12, 7, 2, 3], 21)
    empty = (np.zeros(hw, dtype=np.int32), _records([], 1), f0[2])
    f2 = (np.roll(f0[0], (2, 3), axis=(0, 1)), f0[1], [torch.roll(f, (1, 1), dims=(2, 3)) if i == 0 else f for i, f in enumerate(f0[2])])
    return [f0, empty, f2]


@functools.lru_cache(maxsize=None)
def _whole_step():
    gpu = torch.device("cuda:0")
    frames = _clip()
    # the Python chain: three step_device calls on a fresh tracker
    assoc = V.VideoAssociator(_head("fp32"), TRACKER_CFG, N_THING, N_STUFF)
    ref = []
    for pan, row, feats in frames:
        sem, trk = assoc.step_device([f.to(gpu) for f in feats], torch.from_numpy(pan).to(gpu), segments_from_records(row, K, N_THING))
        ref.append((sem.cpu(), trk.cpu()))
    pan, rec, levels = _batch(frames, gpu)
    plan = _plan("fp32", 3, (64, 128), 12, levels)
    plan.run(pan, rec, levels)
    tr = V.QuasiDenseEmbedTracker(**TRACKER_CFG)
    trk, ids, matched = plan.match(tr.native_tracker(gpu), pan, 1)
    torch.cuda.synchronize()
    return dict(frames=frames, ref=ref, sem=plan.sem.cpu(), trk=trk.cpu(), ids=ids.clone(), matched=matched, things=plan.things.cpu(),
                embeds=plan.embeds.cpu(), cnt=assoc.cnt, batch=(pan, rec, levels))


def test_whole_step_equals_three_step_device_calls(gpu):
    w = _whole_step()
    assert w["matched"] == 2 and w["cnt"] == 3
    for b in range(3):
        assert w["sem"].dtype == torch.uint8 and w["trk"].dtype == torch.float64
        assert torch.equal(w["sem"][b], w["ref"][b][0]), b
        assert torch.equal(w["trk"][b], w["ref"][b][1]), b
    assert float(w["trk"][1].abs().sum()) == 0 and float(w["trk"][0].max()) > 0


def test_whole_step_track_ids_equal_the_oracle_tracker(gpu):
    """the oracle's restatement of the reference tracker on the plan's own records (boxes, labels, embeddings)"""
    w = _whole_step()
    ref_tr = VO.TrackerOracle(**TRACKER_CFG)
    cnt = 1
    for b in range(3):
        n, ids, lab, box, over = _table(w["things"], b, 12)
        if n == 0:
            assert not w["ids"][b].any()
            continue
        got = ref_tr.match(torch.from_numpy(box[:n].copy()), torch.from_numpy(lab[:n].astype(np.int64)), w["embeds"][b, :n], cnt)[2] + 1
        cnt += 1
        got[got == -1] = 0
        k = len(got)
        assert w["ids"][b, :k].tolist() == got.tolist() and not w["ids"][b, k:].any()
        want = V.track_id_map(w["frames"][b][0], ids[:n].tolist(), got.tolist())
        assert np.array_equal(w["trk"][b].numpy(), want)


def test_module_switch(gpu):
    w = _whole_step()
    pan, rec, levels = w["batch"]
    assoc = V.VideoAssociator(_head("fp32"), TRACKER_CFG, N_THING, N_STUFF)
    assert assoc.native_plan is False
    assoc.use_native_plan(True, max_things=12)
    sem, trk = assoc.step_records(levels, pan, rec)
    assert torch.equal(sem.cpu(), w["sem"]) and torch.equal(trk.cpu(), w["trk"]) and assoc.cnt == 3
    # a second clip continues the stream: the frame counter and the tracker's memory carry over
    sem2, trk2 = assoc.step_records(levels, pan, rec)
    assert assoc.cnt == 5 and torch.equal(sem2.cpu(), w["sem"])
    # a frame with more things than max_things is an error, not a truncation
    assoc.use_native_plan(True, max_things=3)
    with pytest.raises(_lib.PolyheadError, match="max_things"):
        assoc.step_records(levels, pan, rec)
    # off: the Python chain as before
    assoc.use_native_plan(False)
    assoc.init_tracker()
    f = w["frames"][0]
    s1, t1 = assoc.step_device([x.to(gpu) for x in f[2]], torch.from_numpy(f[0]).to(gpu), segments_from_records(f[1], K, N_THING))
    assert torch.equal(s1.cpu(), w["ref"][0][0]) and torch.equal(t1.cpu(), w["ref"][0][1])


# ---- 10. graph
def test_run_is_capturable_and_replays_on_new_inputs(gpu):
    hw = (37, 50)
    first = [_frame(hw, [1, 9, 0, 5], 61), _frame(hw, [10, 2, 3, 11, 4, 6], 62)]
    second = [_frame(hw, [12, 7, 7], 63), _frame(hw, [0, 1, 2, 3, 4, 5, 6], 64)]
    pan, rec, levels = _batch(first, gpu)
    plan = _plan("bf16", 2, hw, 8, levels)
    plan.run(pan, rec, levels)                                  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                  # one stream, no parallel branches
        plan.run(pan, rec, levels)
    torch.cuda.synchronize()
    p2, r2, l2 = _batch(second, gpu)
    eager = _plan("bf16", 2, hw, 8, l2)
    eager.embeds.fill_(SENTINEL)
    eager.run(p2, r2, l2)
    pan.copy_(p2), rec.copy_(r2)
    for a, b in zip(levels, l2):
        a.copy_(b)
    plan.embeds.fill_(SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    assert plan.things[:, 0].tolist() == [2, 7] and torch.equal(plan.things, eager.things)
    assert torch.equal(plan.sem, eager.sem) and torch.equal(plan.embeds, eager.embeds)


# ---- 11. environment
def test_environment_does_not_reach_the_plan(gpu, monkeypatch):
    """the library's switches (set by call) and the variables the Python plans read change nothing in the plan"""
    frames = [_frame((64, 128), [1, 9, 0, 5, 12], 71), _frame((64, 128), [3, 3], 72)]
    pan, rec, levels = _batch(frames, gpu)
    plan = _plan("bf16", 2, (64, 128), 6, levels)
    plan.embeds.fill_(SENTINEL)
    plan.run(pan, rec, levels)
    valid = lambda p: [p.roi_planes()[:, b, :n].clone() for b, n in enumerate(p.things[:, 0].tolist())]     # rows < nthing are written
    ref = [t.clone() for t in (plan.sem, plan.things, plan.embeds)] + valid(plan)
    assert plan.things[:, 0].tolist() == [3, 2]
    for k, v in dict(PH_GNSUM_TPW="2", PH_NECK_STATS3="0", PH_NECK_APPLY3="0", PH_KHEAD1_PAIR="1", PH_POOL_NSPLIT="3").items():
        monkeypatch.setenv(k, v)
    with _lib.switches(conv_wgs=7, up2_wgs=5, query_nrt=1, conv_tile_rows=4, gnsum_wgs=3, cplanes_tpw=2):
        again = _plan("bf16", 2, (64, 128), 6, levels)
        again.embeds.fill_(SENTINEL)
        again.run(pan, rec, levels)
    for a, b in zip(ref, [again.sem, again.things, again.embeds] + valid(again)):
        assert torch.equal(a, b)
    g0, g1 = plan.geometry, again.geometry
    assert bytes(g0)[:40] == bytes(g1)[:40]
