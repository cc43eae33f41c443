"""GPU: the tracker bank (csrc/ph_dtracker.hip: ph_dtracker_bank_*, ph_dtracker_step, ph_dtracker_reset_streams,
ph_assoc_plan_track_streams) -- S independent device trackers advanced by one frame each in one launch sequence -- against the host
native tracker (ph_tracker_match), the reference's goldens (tests/golden/tracker.npz) and SINGLE device trackers fed the same frames
(`NativeDeviceTracker`, itself pinned to the host tracker by tests/test_gpu_device_tracker.py); never the bank against itself.
Everything is integer or bit equality: there is no tolerance here."""
import numpy as np
import pytest
import torch

import helpers as Hh
import test_gpu_device_tracker as DT
import test_gpu_native_assoc as NA
from polyphonicformer_amd import _lib, tracker as TR, video as V

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EMPTY = (0, torch.zeros(0, 5), torch.zeros(0, dtype=torch.long), torch.zeros(0, 256))


def _bank(cfg, gpu, streams, capacity, max_dets):
    return TR.NativeDeviceTrackerBank(TR.native_tracker_cfg(**cfg), gpu, streams, capacity, max_dets)


# a schedule is a list of steps; a step has one entry per stream: None (idle), a record (bboxes, labels, embeds as
# helpers.tracker_records gives them; EMPTY: count 0), or a dict(rec=record, reset=True, refuse=word, count=n) for a frame in front of
# which the stream is reset, whose refuse word is non-zero or whose count word is overwritten
def _entry(e):
    e = dict(rec=e) if not isinstance(e, dict) else e
    return e["rec"], bool(e.get("reset")), int(e.get("refuse", 0)), e.get("count")


def _frame_tables(entries, width, gpu):
    recs = [EMPTY if e is None else _entry(e)[0] for e in entries]
    boxes, labels, counts, embeds, refuse = DT._tables(recs, gpu, width, refuse=[0 if e is None else _entry(e)[2] for e in entries])
    for s, e in enumerate(entries):
        if e is not None and _entry(e)[3] is not None:
            counts[s] = _entry(e)[3]
    return boxes, labels, counts, embeds, refuse


def _run_bank(bank, schedule, width, gpu, check_idle=False):
    """the schedule through `bank.step` -> per stream the (kept, ids) of its frames in order.  check_idle: an idle stream's whole block
    is compared before and after the step, and its kept_counts entry is 0"""
    S = bank.streams
    out = [[] for _ in range(S)]
    for entries in schedule:
        assert len(entries) == S
        resets = [s for s, e in enumerate(entries) if e is not None and _entry(e)[1]]
        if resets:
            bank.reset(resets, 1)
        idle = [s for s, e in enumerate(entries) if e is None]
        before = {s: bank.block(s).clone() for s in idle} if check_idle else {}
        boxes, labels, counts, embeds, refuse = _frame_tables(entries, width, gpu)
        active = None if not idle else torch.tensor([0 if e is None else 1 for e in entries], dtype=torch.int32, device=gpu)
        kept, ids, kc = bank.step(boxes, labels, counts, embeds, refuse, active)
        kept, ids, kc = kept.cpu(), ids.cpu(), kc.cpu().tolist()
        for s, e in enumerate(entries):
            if e is None:
                assert kc[s] == 0
                if check_idle:
                    assert torch.equal(bank.block(s), before[s]), s
            else:
                out[s].append((kept[s, :kc[s]].tolist(), ids[s, :kc[s]].tolist()))
    return out


def _run_solo(cfg, events, width, gpu, capacity, max_dets):
    """one stream's entries (the non-idle ones of its column of a schedule) through a single NativeDeviceTracker, one frame per call"""
    dt = DT._dtracker(cfg, gpu, capacity=capacity, max_dets=max_dets)
    out = []
    for e in events:
        if _entry(e)[1]:
            dt.reset(1)
        boxes, labels, counts, embeds, refuse = _frame_tables([e], width, gpu)
        kept, ids, kc = dt.run(boxes, labels, counts, embeds, refuse)
        k = int(kc.cpu()[0])
        out.append((kept.cpu()[0, :k].tolist(), ids.cpu()[0, :k].tolist()))
    return out, dt


def _column(schedule, s):
    return [entries[s] for entries in schedule if entries[s] is not None]


def _assert_tables_equal(a, b, what):
    for k in ("ids", "labels", "seen", "boxes", "slots", "pool"):
        assert torch.equal(a[k], b[k]), (what, k)
    assert len(a["backdrops"]) == len(b["backdrops"]), what
    for g, (x, y) in enumerate(zip(a["backdrops"], b["backdrops"])):
        for k in ("labels", "slots", "boxes"):
            assert torch.equal(x[k], y[k]), (what, "backdrop", g, k)


def _assert_stream_is_solo(bank, s, got, solo_out, solo, what=None):
    what = s if what is None else what
    assert got == solo_out, what
    assert bank.status(s) == solo.status(), what
    _assert_tables_equal(bank.tables(s), solo.tables(), what)


def _side_by_side(clips):
    """clips of different lengths as a schedule: stream s idle once its clip has ended"""
    return [[c[f] if f < len(c) else None for c in clips] for f in range(max(len(c) for c in clips))]


# ---- 1. the reference's ids, side by side
@pytest.mark.parametrize("metric", ["bisoftmax", "softmax", "cosine"])
def test_reference_ids_side_by_side(gpu, metric):
    z = Hh.load_golden("tracker.npz")
    cfg = DT._gold_cfg(match_metric=metric)
    clips = [Hh.tracker_records(seed) for seed in (1, 2, 3)]
    bank = _bank(cfg, gpu, 3, 64, 16)
    got = _run_bank(bank, _side_by_side(clips), 16, gpu)
    for s, (seed, recs) in enumerate(zip((1, 2, 3), clips)):
        host, _, _, _, _ = DT._host_stream(cfg, recs, gpu)
        assert got[s] == host, seed
        if metric == "bisoftmax":
            for (f, _, _, _), (_, ids) in zip(recs, got[s]):
                assert np.array_equal(DT._painted(ids), z[f"s{seed}_f{f}_ids"]), (seed, f)
        solo_out, solo = _run_solo(cfg, recs, 16, gpu, 64, 16)
        assert solo_out == host and bank.status(s) == solo.status(), seed
        assert bank.status(s)["matched"] == len(recs) and bank.status(s)["error"] == 0


# ---- 2. phase, idle steps, empty frames and a reset in the middle
def test_phase_idle_steps_empty_frames_and_a_reset_in_the_middle(gpu):
    cfg = DT._gold_cfg()
    a, b, c, d = (Hh.tracker_records(5, nframes=6), Hh.tracker_records(6, nframes=4), Hh.tracker_records(7, nframes=5),
                  Hh.tracker_records(8, nframes=3))
    schedule = [
        [a[0], None, c[0]],
        [a[1], b[0], c[1]],
        [None, b[1], c[2]],
        [a[2], EMPTY, c[3]],
        [a[3], b[2], dict(rec=d[0], reset=True)],            # stream 2's camera starts a new sequence; 0 and 1 go on
        [EMPTY, None, d[1]],
        [a[4], b[3], None],
        [a[5], None, d[2]],
        [None, None, c[4]],
    ]
    bank = _bank(cfg, gpu, 3, 64, 16)
    got = _run_bank(bank, schedule, 16, gpu, check_idle=True)
    for s in range(3):
        solo_out, solo = _run_solo(cfg, _column(schedule, s), 16, gpu, 64, 16)
        _assert_stream_is_solo(bank, s, got[s], solo_out, solo)
    assert [bank.status(s)["frames_seen"] for s in range(3)] == [7, 5, 4]       # idle steps are not frames; stream 2 counts from its reset
    assert [bank.status(s)["matched"] for s in range(3)] == [6, 4, 4]            # empty frames do not advance the counter


# ---- 3. wide state away from stream 0
def test_wide_state_in_the_last_stream(gpu):
    """stream 3 of 4 gets test_gpu_device_tracker's long clip (more than 256 memory columns, more than 64 detections, slot recycling),
    streams 0 .. 2 small clips: a wrong stride or a stream-0 pointer shows here.  The long clip's ids are the host tracker's too."""
    w = DT._long_stream()
    cfg = DT._gold_cfg()
    clips = [Hh.tracker_records(40 + s, nframes=10 + 2 * s) for s in range(3)] + [w["recs"]]
    schedule = _side_by_side(clips)
    bank = _bank(cfg, gpu, 4, 512, 128)
    got = _run_bank(bank, schedule, 128, gpu)
    assert got[3] == w["host"] and bank.status(3)["num_tracklets"] == w["num"]
    for s in range(4):
        solo_out, solo = _run_solo(cfg, clips[s], 128, gpu, 512, 128)
        _assert_stream_is_solo(bank, s, got[s], solo_out, solo)


# ---- 4. errors stay in their stream
def test_errors_stay_in_their_stream(gpu):
    """capacity 16: stream 0 runs out of pool slots (tracker_records(1, nobj=16), test_gpu_device_tracker's refused clip), stream 1 gets
    a count above max_dets in frame 2, stream 2 a refuse word in frame 3, stream 3 the golden clip, which fits.  Each refused stream is
    sticky with the state its previous frame left -- a solo tracker fed the frames in front of the refusal -- and every stream equals
    the solo tracker fed the same words."""
    cfg = DT._gold_cfg()
    gold = Hh.tracker_records(1)
    clips = [Hh.tracker_records(1, nobj=16), list(gold), list(gold), list(gold)]
    clips[1][2] = dict(rec=gold[2], count=17)
    clips[2][3] = dict(rec=gold[3], refuse=7)
    bank = _bank(cfg, gpu, 4, 16, 16)
    got = _run_bank(bank, _side_by_side(clips), 16, gpu)
    sts = [bank.status(s) for s in range(4)]
    at = sts[0]["refused_frame"]
    assert at >= 1 and (sts[0]["error"], sts[0]["matched"]) == (_lib.PH_DTRK_EPOOL, at)
    assert (sts[1]["error"], sts[1]["refused_frame"], sts[1]["matched"]) == (_lib.PH_DTRK_ECOUNT, 2, 2)
    assert (sts[2]["error"], sts[2]["refused_frame"], sts[2]["matched"]) == (_lib.PH_DTRK_EREFUSED, 3, 3)
    assert (sts[3]["error"], sts[3]["refused_frame"], sts[3]["matched"]) == (0, -1, 12)
    assert all(st["frames_seen"] == 12 for st in sts)
    for s, cut in ((0, at), (1, 2), (2, 3), (3, 12)):
        assert all(o == ([], []) for o in got[s][cut:]), s                      # refused, then sticky
        solo_out, solo = _run_solo(cfg, clips[s], 16, gpu, 16, 16)
        _assert_stream_is_solo(bank, s, got[s], solo_out, solo)
        before_out, before = _run_solo(cfg, clips[s][:cut], 16, gpu, 16, 16)   # the state as the previous frame left it
        assert got[s][:cut] == before_out
        _assert_tables_equal(bank.tables(s), before.tables(), (s, "before the refusal"))
    z = Hh.load_golden("tracker.npz")
    for (f, _, _, _), (_, ids) in zip(gold, got[3]):
        assert np.array_equal(DT._painted(ids), z[f"s1_f{f}_ids"]), f
    # a reset of the refused streams only: they start again, stream 3 goes on
    bank.reset([0, 1, 2], 1)
    assert [bank.status(s)["error"] for s in range(4)] == [0, 0, 0, 0] and bank.status(3)["matched"] == 12 and bank.status(1)["frames_seen"] == 0


# ---- 5. bounds
def test_sixty_four_streams(gpu):
    cfg = DT._gold_cfg()
    clips = [Hh.tracker_records(300 + s, nframes=4, nobj=4) for s in range(64)]
    bank = _bank(cfg, gpu, 64, 16, 4)
    got = _run_bank(bank, _side_by_side(clips), 4, gpu)
    for s in (0, 31, 63):
        solo_out, solo = _run_solo(cfg, clips[s], 4, gpu, 16, 4)
        _assert_stream_is_solo(bank, s, got[s], solo_out, solo)
        assert any(len(k) for k, _ in got[s])
    bank.reset([63], 1)
    assert bank.status(63)["frames_seen"] == 0 and bank.status(62)["frames_seen"] == 4 and bank.status(0)["frames_seen"] == 4


def test_bad_stream_counts_and_run_on_a_bank_fail_with_a_message(gpu):
    cfg = DT._gold_cfg()
    for streams in (0, 65):
        with pytest.raises(_lib.PolyheadError, match="streams"):
            _bank(cfg, gpu, streams, 16, 4)
    bank = _bank(cfg, gpu, 2, 16, 4)
    mem = bank.mem.clone()
    boxes, labels, counts, embeds, refuse = _frame_tables([EMPTY, EMPTY], 4, gpu)
    out = (torch.zeros(2, 4, dtype=torch.int32, device=gpu), torch.zeros(2, 4, dtype=torch.int64, device=gpu),
           torch.full((2,), -5, dtype=torch.int32, device=gpu))
    with pytest.raises(_lib.PolyheadError, match="step"):
        bank.run(boxes, labels, counts, embeds)
    io = _lib.DtrackerIO()
    io.boxes, io.labels, io.counts, io.embeds = boxes.data_ptr(), labels.data_ptr(), counts.data_ptr(), embeds.data_ptr()
    io.kept_out, io.ids_out, io.kept_counts = (o.data_ptr() for o in out)
    import ctypes as C
    assert _lib.load().ph_dtracker_run(bank._h, C.byref(io), 1, _lib.stream_ptr()) == -1 and "ph_dtracker_step" in Hh.last_error()
    torch.cuda.synchronize()
    assert torch.equal(bank.mem, mem) and out[2].tolist() == [-5, -5]           # no launch
    with pytest.raises(_lib.PolyheadError):
        bank.reset([2])


# ---- 6. capture
def test_one_step_in_a_graph_replays_over_the_clips(gpu):
    cfg = DT._gold_cfg()
    clips = [Hh.tracker_records(seed, nframes=6) for seed in (11, 12, 13)]
    schedule = _side_by_side(clips)
    schedule[2][1] = None                                    # an idle word inside the replayed tables
    want = _run_bank(_bank(cfg, gpu, 3, 64, 16), schedule, 16, gpu)
    for s in range(3):
        assert want[s] == _run_solo(cfg, _column(schedule, s), 16, gpu, 64, 16)[0]
    bank = _bank(cfg, gpu, 3, 64, 16)
    static = [t.clone() for t in _frame_tables(schedule[0], 16, gpu)]
    active = torch.ones(3, dtype=torch.int32, device=gpu)
    out = (torch.zeros(3, 16, dtype=torch.int32, device=gpu), torch.zeros(3, 16, dtype=torch.int64, device=gpu),
           torch.zeros(3, dtype=torch.int32, device=gpu))
    bank.step(*static, active, out)                          # warm-up outside the capture
    bank.reset(None, 1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bank.step(*static, active, out)
    torch.cuda.synchronize()
    assert all(bank.status(s)["frames_seen"] == 0 for s in range(3))           # the capture ran nothing
    got = [[] for _ in range(3)]
    for entries in schedule:
        for dst, src in zip(static, _frame_tables(entries, 16, gpu)):
            dst.copy_(src)
        active.copy_(torch.tensor([0 if e is None else 1 for e in entries], dtype=torch.int32))
        g.replay()
        torch.cuda.synchronize()
        kc = out[2].tolist()
        for s, e in enumerate(entries):
            if e is not None:
                got[s].append((out[0][s, :kc[s]].tolist(), out[1][s, :kc[s]].tolist()))
    assert got == want


def test_the_captured_step_is_seven_launches_in_a_line(gpu):
    """the step of three streams is the seven launches of one frame with a stream dimension, and the captured graph is linear: one
    root, six edges, no node with two dependents -- no side streams inside the capture, no memset or copy node"""
    import ctypes as C
    bank = _bank(DT._gold_cfg(match_metric="bisoftmax"), gpu, 3, 64, 16)
    tabs = _frame_tables([Hh.tracker_records(s, nframes=1)[0] for s in (1, 2, 3)], 16, gpu)
    run = lambda: bank.step(*tabs)
    assert Hh.graph_kernel_nodes(run) == sorted([[3, 1, 1, 256, 0], [16 + 64, 3, 1, 256, 0], [1, 4, 3, 256, 0], [1, 3, 1, 256, 0],
                                                 [16, 3, 1, 256, 0], [3, 1, 1, 256, 0], [16, 3, 1, 256, 0]])
    hip = C.CDLL(next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64.so" in l))
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        run()
    graph = C.c_void_p(g.raw_cuda_graph())
    n, e, r = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and hip.hipGraphGetEdges(graph, None, None, C.byref(e)) == 0
    assert hip.hipGraphGetRootNodes(graph, None, C.byref(r)) == 0
    assert (n.value, e.value, r.value) == (7, 6, 1)
    arr = (C.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(graph, arr, C.byref(n)) == 0
    for node in arr:
        d = C.c_size_t(0)
        assert hip.hipGraphNodeGetDependentNodes(C.c_void_p(node), None, C.byref(d)) == 0 and d.value <= 1


# ---- 7. association
def _assoc_frames(hw, gpu):
    """four steps of three streams' crafted frames (different seeds per stream), at most 12 things"""
    labels = [[[1, 9, 0, 5], [10, 2, 3, 11, 4, 6], [0, 1, 2]],
              [[1, 7, 0, 5, 2], [10, 2, 3, 4, 6], [0, 1, 2, 3]],
              [[1, 9, 0], [2, 3, 11, 4, 6], [0, 1, 2, 3, 4, 5, 6]],
              [[1, 9, 0, 5], [10, 2, 3, 11], [0, 2, 1]]]
    seeds = [[61, 62, 64], [61, 62, 64], [61, 62, 64], [61, 62, 64]]
    return [[NA._frame(hw, labels[t][s], seeds[t][s]) for s in range(3)] for t in range(4)]


def test_association_of_three_streams_equals_three_single_stream_associators(gpu):
    hw = (96, 160)
    steps = _assoc_frames(hw, gpu)
    idle = (2, 1)                                            # step 2: stream 1 has no frame
    multi = V.VideoAssociator(NA._head("fp32"), NA.TRACKER_CFG, NA.N_THING, NA.N_STUFF)
    multi.use_native_plan(True, max_things=12, device_tracker=True, streams=3)
    solos = [V.VideoAssociator(NA._head("fp32"), NA.TRACKER_CFG, NA.N_THING, NA.N_STUFF).use_native_plan(True, max_things=12, device_tracker=True)
             for _ in range(3)]
    for t, frames in enumerate(steps):
        pan, rec, levels = NA._batch(frames, gpu)
        active = [0 if (t, s) == idle else 1 for s in range(3)] if t == idle[0] else None
        if active is not None:
            before = (multi.device_status(idle[1]), multi._dtracker.tables(idle[1]))
        sem, trk = multi.step_records(levels, pan, rec, active=active)
        sem, trk = sem.clone(), trk.clone()
        for s in range(3):
            if (t, s) == idle:
                assert float(trk[s].abs().sum()) == 0
                assert multi.device_status(s) == before[0]
                _assert_tables_equal(multi._dtracker.tables(s), before[1], "idle")
                continue
            p1, r1, l1 = NA._batch(frames[s:s + 1], gpu)
            sem1, trk1 = solos[s].step_records(l1, p1, r1)
            assert torch.equal(sem[s], sem1[0]) and torch.equal(trk[s], trk1[0]), (t, s)
            assert float(trk1[0].abs().sum()) > 0
    for s in range(3):
        assert multi.frames_matched(s) == solos[s].frames_matched() == (3 if s == idle[1] else 4)
        assert multi.device_status(s) == solos[s].device_status()
    # a new video on stream 2 only
    multi.init_tracker(streams=[2])
    assert [multi.frames_matched(s) for s in range(3)] == [4, 3, 0]
