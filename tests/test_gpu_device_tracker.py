"""GPU: the device tracker (csrc/ph_dtracker.hip: ph_dtracker_*, ph_assoc_plan_track) against the host-side native tracker
(csrc/ph_tracker.hip through ph_tracker_match / ph_assoc_plan_match), the CPU form's tables (tracker._TrackTable) and the reference's
goldens (tests/golden/tracker.npz) -- never against itself.  Everything is integer or bit equality: there is no tolerance here."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import helpers as Hh
import test_gpu_native_assoc as NA
from polyphonicformer_amd import _lib, tracker as TR, video as V

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _gold_cfg(**kw):
    cfg = json.loads(bytes(Hh.load_golden("tracker.npz")["cfg_json"]).decode())
    cfg.update(kw)
    return cfg


def _host_tracker(cfg, capacity=4096):
    class Sized(V.QuasiDenseEmbedTracker):
        NATIVE_CAPACITY = capacity
    return Sized(**cfg)


def _host_match(tr, bb, lab, emb_dev, frame_id):
    """ph_tracker_match itself: (k or a negative code, kept [k], ids [k])"""
    lib = _lib.load()
    box, lb = np.ascontiguousarray(bb.numpy(), dtype=np.float32), np.ascontiguousarray(lab.numpy(), dtype=np.int64)
    n = box.shape[0]
    kept, ids = np.empty((max(n, 1),), dtype=np.int32), np.empty((max(n, 1),), dtype=np.int64)
    k = lib.ph_tracker_match(tr.native_tracker(emb_dev.device).handle, box.ctypes.data_as(C.c_void_p), lb.ctypes.data_as(C.c_void_p), _lib.ptr(emb_dev), n,
                             int(frame_id), kept.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), _lib.stream_ptr())
    return k, kept[:max(k, 0)].tolist(), ids[:max(k, 0)].tolist()


def _host_stream(cfg, recs, gpu, capacity=4096, cpu_form=False):
    """the host native tracker over the non-empty frames of `recs` with frame ids 1, 2, ..: per frame (kept, ids), the tracker, and
    (cpu_form) the array form on the CPU fed the same frames plus the largest m and n it saw"""
    tr, cpu = _host_tracker(cfg, capacity), (V.QuasiDenseEmbedTracker(**cfg) if cpu_form else None)
    out, cnt, max_m, max_n = [], 1, 0, 0
    for _, bb, lab, emb in recs:
        if bb.shape[0] == 0:
            out.append(([], []))
            continue
        k, kept, ids = _host_match(tr, bb, lab, emb.to(gpu).contiguous(), cnt)
        assert k >= 0, _lib.load().ph_last_error_string()
        if cpu is not None:
            max_m = max(max_m, len(cpu.table) + sum(b[0].shape[0] for b in cpu.table.backdrops))
            max_n = max(max_n, bb.shape[0])
            assert cpu.match(bboxes=bb, labels=lab, track_feats=emb, frame_id=cnt)[2].tolist() == ids
        out.append((kept, ids))
        cnt += 1
    return out, tr, cpu, max_m, max_n


def _tables(recs, gpu, width=None, refuse=None):
    """the frames as ph_dtracker_io tables: boxes [F, w, 5], labels [F, w], counts [F], embeds [F, w, 256], refuse [F] or None"""
    F = len(recs)
    w = width or max(1, max(r[1].shape[0] for r in recs))
    boxes, labels, embeds = torch.zeros(F, w, 5), torch.zeros(F, w, dtype=torch.int32), torch.zeros(F, w, 256)
    counts = torch.tensor([r[1].shape[0] for r in recs], dtype=torch.int32)
    for i, (_, bb, lab, emb) in enumerate(recs):
        n = min(bb.shape[0], w)
        boxes[i, :n], labels[i, :n], embeds[i, :n] = bb[:n], lab[:n].int(), emb[:n]
    ref = None if refuse is None else torch.tensor(refuse, dtype=torch.int32).to(gpu)
    return boxes.to(gpu), labels.to(gpu), counts.to(gpu), embeds.to(gpu), ref


def _device_stream(dt, tabs, per_call=1):
    """the frames through NativeDeviceTracker.run, `per_call` frames per call -> per frame (kept, ids)"""
    boxes, labels, counts, embeds, refuse = tabs
    out = []
    for a in range(0, counts.shape[0], per_call):
        b = a + per_call
        kept, ids, kc = dt.run(boxes[a:b], labels[a:b], counts[a:b], embeds[a:b], None if refuse is None else refuse[a:b])
        kept, ids, kc = kept.cpu(), ids.cpu(), kc.cpu().tolist()
        out += [(kept[i, :k].tolist(), ids[i, :k].tolist()) for i, k in enumerate(kc)]
    return out


def _dtracker(cfg, gpu, capacity=512, max_dets=128):
    return TR.NativeDeviceTracker(TR.native_tracker_cfg(**cfg), gpu, capacity, max_dets)


def _painted(ids):
    r = np.asarray(ids, dtype=np.int64) + 1
    r[r == -1] = 0
    return r


# ---- 1. the reference's ids
@pytest.mark.parametrize("metric", ["bisoftmax", "softmax", "cosine"])
def test_reference_ids(gpu, metric):
    z = Hh.load_golden("tracker.npz")
    cfg = _gold_cfg(match_metric=metric)
    dt = _dtracker(cfg, gpu, capacity=64, max_dets=16)
    for seed in (1, 2, 3):
        recs = Hh.tracker_records(seed)
        host, tr, _, _, _ = _host_stream(cfg, recs, gpu)
        dt.reset(1)
        got = _device_stream(dt, _tables(recs, gpu))
        assert got == host, seed
        # the branches: ids matched to an existing tracklet, unmatched (-1) and suppressed (-2) detections, from the host's output
        born, matched, flat = 0, 0, [i for _, ids in host for i in ids]
        for _, ids in host:
            matched += sum(1 for i in ids if 0 <= i < born)
            born = max([born] + [i + 1 for i in ids])
        assert matched > 0 and -1 in flat and -2 in flat, (seed, matched)
        st = dt.status()
        assert (st["matched"], st["num_tracklets"], st["rows"], st["error"], st["refused_frame"], st["frame_id"]) == \
            (len(recs), tr.num_tracklets, _lib.load().ph_tracker_rows(tr._native.handle), 0, -1, len(recs) + 1)
        if metric == "bisoftmax":
            for (f, _, _, _), (_, ids) in zip(recs, got):
                assert np.array_equal(_painted(ids), z[f"s{seed}_f{f}_ids"]), (seed, f)


# ---- 2. many columns, many detections, slot recycling
@functools.lru_cache(maxsize=None)
def _long_stream():
    gpu = torch.device("cuda:0")
    recs = [r for s in range(8) for r in Hh.tracker_records(200 + s, nframes=2, nobj=120)]
    host, tr, cpu, max_m, max_n = _host_stream(_gold_cfg(), recs, gpu, capacity=512, cpu_form=True)
    torch.cuda.synchronize()
    pool = tr._native.mem[:512 * 1024].view(torch.float32).reshape(512, 256).cpu()
    return dict(recs=recs, host=host, num=tr.num_tracklets, rows=_lib.load().ph_tracker_rows(tr._native.handle), table=cpu.table, pool=pool,
                max_m=max_m, max_n=max_n, tabs=_tables(recs, gpu, 128))


@pytest.mark.parametrize("per_call", [1, 4])
def test_long_stream_equals_the_host_tracker(gpu, per_call):
    """16 frames of ~100 detections: more than 256 memory columns (past k_aff_dot's 64-column tile and k_aff_rows' stride), more
    than 64 detections, 762 tracklets born and slots recycled; as 16 one-frame calls and as 4 calls of 4 frames.  The host tracker
    exposes no slot table: both take and return slots in the same order, so a tracklet's pool row is compared at the device's slot."""
    w = _long_stream()
    assert w["max_m"] > 256 and w["max_n"] > 64 and w["num"] == 762
    dt = _dtracker(_gold_cfg(), gpu, capacity=512, max_dets=128)
    got = _device_stream(dt, w["tabs"], per_call)
    for f, (g, h) in enumerate(zip(got, w["host"])):
        assert g == h, f
    st, tb, ref = dt.status(), dt.tables(), w["table"]
    assert (st["num_tracklets"], st["rows"], st["matched"], st["error"]) == (w["num"], w["rows"], 16, 0) and st["rows"] == len(ref)
    assert st["free"] == 512 - st["rows"] - sum(len(b["slots"]) for b in tb["backdrops"])
    assert tb["ids"].tolist() == ref.ids.tolist() and tb["labels"].tolist() == ref.lab.tolist() and tb["seen"].tolist() == ref.seen.tolist()
    assert torch.equal(tb["boxes"], torch.from_numpy(ref.box))
    slots = tb["slots"].long()
    assert len(set(slots.tolist())) == len(slots)
    assert torch.equal(tb["pool"], w["pool"][slots])


# ---- 3. small edges
def _edge(n, seed, scores=None, spread=60.0):
    g = torch.Generator().manual_seed(seed)
    xy = torch.arange(n, dtype=torch.float32)[:, None] * spread + torch.rand(n, 2, generator=g)
    sc = torch.rand(n, 1, generator=g) * 0.6 + 0.4 if scores is None else torch.tensor(scores, dtype=torch.float32).reshape(n, 1)
    return (0, torch.cat([xy, xy + 40, sc], 1), torch.randint(0, 3, (n,), generator=g), torch.randn(n, 256, generator=g) * 0.5)


def _same(cfg, recs, gpu, **kw):
    host, tr, _, _, _ = _host_stream(cfg, recs, gpu)
    dt = _dtracker(cfg, gpu, **kw)
    got = _device_stream(dt, _tables(recs, gpu))
    assert got == host
    st = dt.status()
    assert (st["num_tracklets"], st["rows"], st["error"]) == (tr.num_tracklets, _lib.load().ph_tracker_rows(tr._native.handle), 0)
    return host, dt


def test_small_edges(gpu):
    cfg = _gold_cfg()
    # one detection; the first frame meets an empty memory (no affinity launch takes effect), the second a memory of one column
    one = _edge(1, 1, [0.9])
    host, _ = _same(cfg, [one, one], gpu, capacity=16, max_dets=1)
    assert host == [([0], [0]), ([0], [0])]
    # n = max_dets = 128, twice: 128 new tracklets, then 128 columns to match
    full = _edge(128, 2)
    host, dt = _same(cfg, [full, full], gpu, capacity=512, max_dets=128)
    assert len(host[0][0]) == 128 and dt.status()["rows"] > 100 and set(host[1][1]) & set(host[0][1])
    # all scores equal: the order is ascending index
    host, _ = _same(cfg, [_edge(9, 3, [0.7] * 9)], gpu, capacity=16, max_dets=16)
    assert host[0][0] == list(range(9))
    # two identical boxes: the second is de-duplicated, whatever follows it in score
    f = _edge(5, 4, [0.9, 0.8, 0.8, 0.6, 0.5])
    f[1][2] = f[1][1]
    host, _ = _same(cfg, [(0, *f[1:])], gpu, capacity=16, max_dets=16)
    assert host[0][0] == [0, 1, 3, 4]
    # a detection whose best column is a backdrop: frame 0 leaves tracklet 0 (score 0.9) and a backdrop (score 0.32: unmatched, below
    # init_score_thr); frame 1's second detection carries the backdrop's embedding -- its best column has id -1, so it starts track 1
    e = torch.zeros(2, 256)
    e[0, 0], e[1, 1] = 8.0, 8.0
    lab = torch.zeros(2, dtype=torch.long)
    f0 = (0, torch.tensor([[0., 0., 40., 40., 0.9], [100., 0., 140., 40., 0.32]]), lab, e)
    f1 = (1, torch.tensor([[2., 0., 42., 40., 0.9], [102., 0., 142., 40., 0.8]]), lab, e)
    host, dt = _same(cfg, [f0, f1], gpu, capacity=16, max_dets=4)
    assert host == [([0, 1], [0, -1]), ([0, 1], [0, 1])]
    assert [len(b["slots"]) for b in dt.tables()["backdrops"]] == [0]


# ---- 4. empty frames
def test_empty_frames_do_not_advance_the_counter(gpu):
    cfg = _gold_cfg(memo_tracklet_frames=2)
    r = Hh.tracker_records(5, nframes=3)
    empty = (1, torch.zeros(0, 5), torch.zeros(0, dtype=torch.long), torch.zeros(0, 256))
    host, tr, cpu, _, _ = _host_stream(cfg, [r[0], r[2]], gpu, cpu_form=True)
    dt = _dtracker(cfg, gpu, capacity=64, max_dets=16)
    got = _device_stream(dt, _tables([r[0], empty, r[2]], gpu), per_call=3)
    assert got == [host[0], ([], []), host[1]]
    st, tb = dt.status(), dt.tables()
    assert (st["matched"], st["frame_id"], st["frames_seen"], st["error"]) == (2, 3, 3, 0)
    assert tb["ids"].tolist() == cpu.table.ids.tolist() and tb["seen"].tolist() == cpu.table.seen.tolist() and st["rows"] == len(cpu.table)
    assert 1 in tb["seen"].tolist() and 2 in tb["seen"].tolist()      # with the empty frame counted, frame 0's rows would have expired


# ---- 5. refusal
def _state(dt):
    tb = dt.tables()
    flat = [tb[k] for k in ("ids", "labels", "seen", "boxes", "slots", "pool")] + [b[k] for b in tb["backdrops"] for k in ("labels", "slots", "boxes")]
    return flat, {k: v for k, v in dt.status().items() if k not in ("error", "refused_frame", "frames_seen")}


def _assert_refused(dt, tabs, at, code, gpu):
    """frames 0 .. at - 1 run, frame `at` is refused with `code`, the state is what frame at - 1 left, the rest is skipped"""
    boxes, labels, counts, embeds, refuse = tabs
    sl = lambda a, b: (boxes[a:b], labels[a:b], counts[a:b], embeds[a:b], None if refuse is None else refuse[a:b])
    before_out = _device_stream(dt, sl(0, at))
    before = _state(dt)
    assert dt.status()["error"] == 0 and before[1]["matched"] == at
    out = _device_stream(dt, sl(at, at + 1))
    st = dt.status()
    assert out == [([], [])] and (st["error"], st["refused_frame"], st["frames_seen"]) == (code, at, at + 1)
    after = _state(dt)
    assert after[1] == before[1] and all(torch.equal(a, b) for a, b in zip(before[0], after[0]))
    rest = _device_stream(dt, sl(at + 1, None), per_call=2)
    st = dt.status()
    assert all(o == ([], []) for o in rest) and (st["error"], st["refused_frame"], st["matched"]) == (code, at, at)
    assert st["frames_seen"] == counts.shape[0]
    after = _state(dt)
    assert after[1] == before[1] and all(torch.equal(a, b) for a, b in zip(before[0], after[0]))
    return before_out


def _assert_golden_after_reset(dt, gpu):
    z = Hh.load_golden("tracker.npz")
    dt.reset(1)
    recs = Hh.tracker_records(1)
    got = _device_stream(dt, _tables(recs, gpu, 16))
    st = dt.status()
    assert (st["error"], st["refused_frame"], st["matched"]) == (0, -1, len(recs))
    for (f, _, _, _), (_, ids) in zip(recs, got):
        assert np.array_equal(_painted(ids), z[f"s1_f{f}_ids"]), f


def test_pool_exhaustion_is_a_status_word_and_leaves_the_state(gpu):
    """capacity 16.  The golden clip tracker_records(1) (14 objects) never needs more than 16 slots, so the refused stream is the same
    generator with 16 objects, whose second frame needs 3 slots with 2 free; the frame is taken from the host tracker's own
    pool-exhaustion error.  After the reset the golden clip runs from the start with the reference's ids."""
    cfg = _gold_cfg()
    recs = Hh.tracker_records(1, nobj=16)
    tr, at, host = _host_tracker(cfg, 16), None, []
    for i, (_, bb, lab, emb) in enumerate(recs):
        k, kept, ids = _host_match(tr, bb, lab, emb.to(gpu).contiguous(), i + 1)
        if k < 0:
            assert k == -4 and b"pool exhausted" in _lib.load().ph_last_error_string()
            at = i
            break
        host.append((kept, ids))
    assert at is not None and at >= 1
    dt = _dtracker(cfg, gpu, capacity=16, max_dets=16)
    assert _assert_refused(dt, _tables(recs, gpu, 16), at, _lib.PH_DTRK_EPOOL, gpu) == host
    _assert_golden_after_reset(dt, gpu)


def test_refuse_word_and_count_above_max_dets_are_status_words(gpu):
    cfg = _gold_cfg()
    recs = Hh.tracker_records(1)
    dt = _dtracker(cfg, gpu, capacity=64, max_dets=16)
    flags = [0] * len(recs)
    flags[3] = 7
    _assert_refused(dt, _tables(recs, gpu, 16, refuse=flags), 3, _lib.PH_DTRK_EREFUSED, gpu)
    _assert_golden_after_reset(dt, gpu)
    tabs = _tables(recs, gpu, 16)
    tabs[2][2] = 17                                       # a count above max_dets = 16 (the rows are not read)
    dt.reset(1)
    _assert_refused(dt, tabs, 2, _lib.PH_DTRK_ECOUNT, gpu)
    _assert_golden_after_reset(dt, gpu)


# ---- 6. the whole step
def _tcfg():
    return TR.native_tracker_cfg(**NA.TRACKER_CFG)


def test_whole_step_equals_the_host_path(gpu):
    w = NA._whole_step()
    pan, rec, levels = w["batch"]
    host_plan, host_tr = NA._plan("fp32", 3, (64, 128), 12, levels), V.QuasiDenseEmbedTracker(**NA.TRACKER_CFG)
    plan, dt = NA._plan("fp32", 3, (64, 128), 12, levels), TR.NativeDeviceTracker(_tcfg(), gpu, 512, 12)
    first = 1
    for call in range(2):                                # the second call continues the stream
        host_plan.run(pan, rec, levels)
        trk_h, ids_h, matched = host_plan.match(host_tr.native_tracker(gpu), pan, first)
        first += matched
        plan.run(pan, rec, levels)
        trk, ids = plan.track(dt, pan)
        assert torch.equal(trk, trk_h) and torch.equal(ids.cpu(), ids_h), call
        assert dt.status()["matched"] == first - 1 == 2 * (call + 1)
        if call == 0:
            assert torch.equal(trk.cpu(), w["trk"]) and torch.equal(ids.cpu(), w["ids"]) and float(trk[1].abs().sum()) == 0
    assert dt.status()["error"] == 0


# ---- 7. capture
def test_run_and_track_in_one_graph_carry_the_state_across_replays(gpu):
    hw = (37, 50)
    pairs = [[NA._frame(hw, [1, 9, 0, 5], 61), NA._frame(hw, [10, 2, 3, 11, 4, 6], 62)],
             [NA._frame(hw, [1, 7, 0, 5, 2], 61), NA._frame(hw, [0, 1, 2, 3, 4, 5, 6], 64)]]
    batches = [NA._batch(p, gpu) for p in pairs]
    # eager host path on the four frames
    host_plan, host_tr, first, want = NA._plan("bf16", 2, hw, 8, batches[0][2]), V.QuasiDenseEmbedTracker(**NA.TRACKER_CFG), 1, []
    for pan, rec, levels in batches:
        host_plan.run(pan, rec, levels)
        trk, ids, matched = host_plan.match(host_tr.native_tracker(gpu), pan, first)
        first += matched
        want.append((trk.clone(), ids.clone(), host_plan.sem.clone()))
    assert first == 5 and any(int(i.max()) > 0 for _, i, _ in want)
    pan, rec, levels = (batches[0][0].clone(), batches[0][1].clone(), [l.clone() for l in batches[0][2]])
    plan, dt = NA._plan("bf16", 2, hw, 8, levels), TR.NativeDeviceTracker(_tcfg(), gpu, 256, 8)
    plan.run(pan, rec, levels)                           # warm-up outside the capture
    plan.track(dt, pan)
    dt.reset(1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                            # one stream, no parallel branches
        plan.run(pan, rec, levels)
        plan.track(dt, pan)
    torch.cuda.synchronize()
    assert dt.status()["frames_seen"] == 0               # the capture ran nothing
    for i, (p2, r2, l2) in enumerate(batches):
        pan.copy_(p2), rec.copy_(r2)
        for a, b in zip(levels, l2):
            a.copy_(b)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(plan.track_map, want[i][0]) and torch.equal(plan.ids_dev.cpu(), want[i][1]) and torch.equal(plan.sem, want[i][2]), i
    assert dt.status()["matched"] == 4


# ---- 8. the module switch
def test_module_switch(gpu):
    w = NA._whole_step()
    pan, rec, levels = w["batch"]
    host = V.VideoAssociator(NA._head("fp32"), NA.TRACKER_CFG, NA.N_THING, NA.N_STUFF).use_native_plan(True, max_things=12)
    host.step_records(levels, pan, rec)
    trk2_h = host.step_records(levels, pan, rec)[1].clone()
    assert host.cnt == 5 and host.frames_matched() == 4  # device_tracker=False: the old call path, assoc.cnt advances
    assoc = V.VideoAssociator(NA._head("fp32"), NA.TRACKER_CFG, NA.N_THING, NA.N_STUFF)
    assoc.use_native_plan(True, max_things=12, device_tracker=True)
    sem, trk = assoc.step_records(levels, pan, rec)
    assert torch.equal(sem.cpu(), w["sem"]) and torch.equal(trk.cpu(), w["trk"])
    assert assoc.frames_matched() == 2 and assoc.cnt == 1 and assoc.tracker._native is None
    sem2, trk2 = assoc.step_records(levels, pan, rec)
    assert assoc.frames_matched() == 4 and torch.equal(trk2, trk2_h) and torch.equal(sem2.cpu(), w["sem"])
    assoc.init_tracker()
    assert assoc.frames_matched() == 0
    assert torch.equal(assoc.step_records(levels, pan, rec)[1].cpu(), w["trk"]) and assoc.frames_matched() == 2
