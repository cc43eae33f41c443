"""Host-side checks of the tracker bank's C ABI (include/polyhead.h ph_dtracker_bank_* .. ph_dtracker_step, ph_assoc_plan_track_streams)
and of `VideoAssociator.use_native_plan(streams=...)`: the size and argument rules that touch no device memory.  No GPU: nothing here
launches a kernel (tests/test_gpu_tracker_streams.py does)."""
import ctypes as C

import pytest

import helpers as Hh
from polyphonicformer_amd import _lib, engine as E, tracker as TR, video as V

FAKE_PTR = 1 << 40          # a 256-byte aligned address create() stores and never dereferences
LEVELS = ((16, 32), (8, 16), (4, 8), (2, 4))
NAMES = ("boxes", "labels", "counts", "embeds", "kept_out", "ids_out", "kept_counts")


def _cfg(**kw):
    return TR.native_tracker_cfg(**kw)


def _io(**kw):
    o = _lib.DtrackerIO()
    for k in NAMES:
        setattr(o, k, kw.get(k, FAKE_PTR))
    return o


def _bank(streams, capacity=64, max_dets=16):
    lib, cfg, h = _lib.load(), _cfg(), C.c_void_p()
    need = lib.ph_dtracker_bank_bytes(C.byref(cfg), capacity, max_dets, streams)
    assert lib.ph_dtracker_bank_create(C.byref(cfg), C.c_void_p(FAKE_PTR), need, capacity, max_dets, streams, C.byref(h)) == 0, Hh.last_error()
    return h


def test_bank_bytes_is_streams_times_the_single_tracker_and_bounded():
    lib, cfg = _lib.load(), _cfg()
    one = lib.ph_dtracker_device_bytes(C.byref(cfg), 512, 128)
    for s in (1, 2, 7, 64):
        assert lib.ph_dtracker_bank_bytes(C.byref(cfg), 512, 128, s) == s * one
    for s in (0, -1, 65):
        assert lib.ph_dtracker_bank_bytes(C.byref(cfg), 512, 128, s) == 0 and "streams" in Hh.last_error(), s
        h = C.c_void_p()
        assert lib.ph_dtracker_bank_create(C.byref(cfg), C.c_void_p(FAKE_PTR), 1 << 40, 512, 128, s, C.byref(h)) == -1 and not h.value
        assert "streams" in Hh.last_error()
    # the single tracker's rules hold for a bank
    for cap, nd, word in ((15, 128, "capacity"), (4097, 128, "capacity"), (512, 0, "max_dets"), (512, 129, "max_dets")):
        assert lib.ph_dtracker_bank_bytes(C.byref(cfg), cap, nd, 4) == 0 and word in Hh.last_error()
    assert lib.ph_dtracker_bank_bytes(None, 512, 128, 4) == 0 and "cfg" in Hh.last_error()


def test_bank_create_checks_the_whole_buffer_and_reports_streams_and_stride():
    lib, cfg, h = _lib.load(), _cfg(), C.c_void_p()
    one = lib.ph_dtracker_device_bytes(C.byref(cfg), 64, 16)
    need = lib.ph_dtracker_bank_bytes(C.byref(cfg), 64, 16, 3)
    assert lib.ph_dtracker_bank_create(C.byref(cfg), C.c_void_p(FAKE_PTR), need - 256, 64, 16, 3, C.byref(h)) == -4 and "too small" in Hh.last_error()
    assert lib.ph_dtracker_bank_create(C.byref(cfg), C.c_void_p(FAKE_PTR), 2 * one, 64, 16, 3, C.byref(h)) == -4 and not h.value
    assert lib.ph_dtracker_bank_create(C.byref(cfg), C.c_void_p(FAKE_PTR + 16), need, 64, 16, 3, C.byref(h)) == -1 and "aligned" in Hh.last_error()
    assert lib.ph_dtracker_bank_create(C.byref(cfg), C.c_void_p(FAKE_PTR), need, 64, 16, 3, None) == -1
    assert lib.ph_dtracker_bank_create(C.byref(cfg), C.c_void_p(FAKE_PTR), need, 64, 16, 3, C.byref(h)) == 0 and h.value
    n, stride, lay = C.c_int(), C.c_uint64(), _lib.DtrackerLayout()
    assert lib.ph_dtracker_get_streams(h, C.byref(n), C.byref(stride)) == 0 and (n.value, stride.value) == (3, one)
    assert lib.ph_dtracker_get_layout(h, C.byref(lay)) == 0 and lay.total_bytes == one and lay.pool == 0       # stream 0's block
    assert lib.ph_dtracker_get_streams(h, None, C.byref(stride)) == -1 and lib.ph_dtracker_get_streams(None, C.byref(n), C.byref(stride)) == -1
    lib.ph_dtracker_destroy(h)
    # the single tracker is the bank of one
    assert lib.ph_dtracker_create(C.byref(cfg), C.c_void_p(FAKE_PTR), one, 64, 16, C.byref(h)) == 0
    assert lib.ph_dtracker_get_streams(h, C.byref(n), C.byref(stride)) == 0 and (n.value, stride.value) == (1, one)
    lib.ph_dtracker_destroy(h)


def test_step_run_and_reset_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    h = _bank(2)
    # a launch on the fake addresses would fault: every one of these comes back first
    assert lib.ph_dtracker_run(h, C.byref(_io()), 1, None) == -1 and "ph_dtracker_step" in Hh.last_error()
    for k in NAMES:
        assert lib.ph_dtracker_step(h, C.byref(_io(**{k: None})), None, None) == -1 and k in Hh.last_error(), k
    assert lib.ph_dtracker_step(h, None, None, None) == -1 and lib.ph_dtracker_step(None, C.byref(_io()), None, None) == -1
    assert lib.ph_dtracker_reset_streams(None, 1, 1, None) == -1
    for mask in (4, -(1 << 63), 7, -1):
        assert lib.ph_dtracker_reset_streams(h, mask, 1, None) == -1 and "mask" in Hh.last_error(), mask
    lib.ph_dtracker_destroy(h)


def test_plan_track_streams_needs_one_frame_per_stream_and_room_for_the_things():
    lib = _lib.load()
    track = _lib.TrackCfg(num_convs=4, fc_out_channels=1024, embed_channels=256, groups=32, prec=_lib.PH_PREC_SPLIT)
    acfg = E.native_assoc_cfg(3, (64, 128), 24, 12, 8, 11, LEVELS, track)
    plan = C.c_void_p()
    assert lib.ph_assoc_plan_create(C.byref(acfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), 1 << 62, C.byref(plan)) == 0, Hh.last_error()
    two, small, good = _bank(2, 64, 12), _bank(3, 64, 11), _bank(3, 64, 12)
    P = C.c_void_p(FAKE_PTR)
    assert lib.ph_assoc_plan_track_streams(plan, two, P, P, P, None, P, None, None) == -1 and "streams" in Hh.last_error()
    assert lib.ph_assoc_plan_track_streams(plan, small, P, P, P, None, P, None, None) == -1 and "max_dets" in Hh.last_error()
    for args in ((None, good, P, P, P, None, P), (plan, None, P, P, P, None, P), (plan, good, None, P, P, None, P),
                 (plan, good, P, None, P, None, P), (plan, good, P, P, None, None, P), (plan, good, P, P, P, None, None)):
        assert lib.ph_assoc_plan_track_streams(*args, None, None) == -1 and "null" in Hh.last_error()
    for h in (two, small, good):
        lib.ph_dtracker_destroy(h)
    lib.ph_assoc_plan_destroy(plan)


def test_module_switch_streams_bookkeeping():
    a = V.VideoAssociator.__new__(V.VideoAssociator)
    assert a.streams is None
    a.use_native_plan(True, max_things=12, device_tracker=True)
    assert a.streams is None                                  # without `streams` nothing changes
    a.cnt = 1
    assert a.frames_matched() == 0 and a.device_status() is None
    with pytest.raises(_lib.PolyheadError):
        a.frames_matched(1)
    with pytest.raises(_lib.PolyheadError):
        a.init_tracker(streams=[0])
    a.use_native_plan(True, max_things=12, device_tracker=True, streams=3)
    assert (a.streams, a.device_tracker, a.native_plan, a._dtracker) == (3, True, True, None)
    assert a.frames_matched(2) == 0 and a.device_status(0) is None        # no bank yet: nothing to read
    a.init_tracker()                                          # nothing to reset yet either
    a.init_tracker(streams=[1])
    for bad in (None, 3, -1):
        with pytest.raises(_lib.PolyheadError):
            a.frames_matched(bad)
    with pytest.raises(_lib.PolyheadError):
        a.init_tracker(streams=[3])
    for kw in (dict(device_tracker=False, streams=2), dict(device_tracker=True, streams=0), dict(device_tracker=True, streams=65)):
        with pytest.raises(_lib.PolyheadError):
            a.use_native_plan(True, **kw)
    with pytest.raises(_lib.PolyheadError):
        a.use_native_plan(False, device_tracker=True, streams=2)
    assert a.use_native_plan(True, max_things=12, device_tracker=True).streams is None
