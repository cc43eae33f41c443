"""Host-side checks of the device tracker's C ABI (include/polyhead.h ph_dtracker_* and ph_assoc_plan_track): the size query, the state
layout, and argument validation.  No GPU: nothing here launches a
kernel or touches device memory (tests/test_gpu_device_tracker.py does)."""
import ctypes as C

import helpers as Hh
from polyphonicformer_amd import _lib, engine as E, tracker as TR

FAKE_PTR = 1 << 40          # a 256-byte aligned address create() stores and never dereferences
LEVELS = ((16, 32), (8, 16), (4, 8), (2, 4))


def _cfg(**kw):
    return TR.native_tracker_cfg(**kw)


def al256(n):
    return (n + 255) // 256 * 256


def test_device_bytes_refuses_bad_configurations_with_a_message():
    lib = _lib.load()
    good = lib.ph_dtracker_device_bytes(C.byref(_cfg()), 512, 128)
    assert good > 512 * 256 * 4 and good % 256 == 0
    bad = [(_cfg(), 15, 128, "capacity"), (_cfg(), 4097, 128, "capacity"), (_cfg(), 512, 0, "max_dets"), (_cfg(), 512, 129, "max_dets")]
    for metric in (-1, 3):
        c = _cfg()
        c.metric = metric
        bad.append((c, 512, 128, "metric"))
    c = _cfg(memo_backdrop_frames=17)
    bad.append((c, 512, 128, "memo_backdrop_frames"))
    for cfg, cap, nd, word in bad:
        assert lib.ph_dtracker_device_bytes(C.byref(cfg), cap, nd) == 0 and word in Hh.last_error(), (cap, nd, word, Hh.last_error())
        h = C.c_void_p()
        assert lib.ph_dtracker_create(C.byref(cfg), C.c_void_p(FAKE_PTR), 1 << 40, cap, nd, C.byref(h)) == -1 and not h.value and word in Hh.last_error()
    assert lib.ph_dtracker_device_bytes(None, 512, 128) == 0 and "cfg" in Hh.last_error()
    # the edges are good, and the size grows with every argument
    for cap, nd in ((16, 1), (4096, 128)):
        assert lib.ph_dtracker_device_bytes(C.byref(_cfg()), cap, nd) > 0
    assert lib.ph_dtracker_device_bytes(C.byref(_cfg(memo_backdrop_frames=2)), 512, 128) > good
    assert lib.ph_dtracker_device_bytes(C.byref(_cfg(memo_backdrop_frames=0)), 512, 128) < good


def test_layout_is_aligned_ordered_and_inside_the_buffer():
    lib = _lib.load()
    for cap, nd, G in ((512, 128, 1), (16, 1, 0), (4096, 77, 3)):
        cfg, h, lay = _cfg(memo_backdrop_frames=G), C.c_void_p(), _lib.DtrackerLayout()
        need = lib.ph_dtracker_device_bytes(C.byref(cfg), cap, nd)
        assert lib.ph_dtracker_create(C.byref(cfg), C.c_void_p(FAKE_PTR), need, cap, nd, C.byref(h)) == 0, Hh.last_error()
        assert lib.ph_dtracker_get_layout(h, C.byref(lay)) == 0
        lib.ph_dtracker_destroy(h)
        assert (lay.capacity, lay.max_dets, lay.generations, lay.total_bytes) == (cap, nd, G, need)
        sizes = [("pool", cap * 1024), ("trk_id", cap * 8), ("trk_seen", cap * 8), ("trk_label", cap * 4), ("trk_slot", cap * 4),
                 ("trk_box", cap * 20), ("bd_count", G * 4), ("bd_label", G * nd * 4), ("bd_slot", G * nd * 4), ("bd_box", G * nd * 20),
                 ("free_stack", cap * 4), ("status", 8 * _lib.PH_DTRK_ST_WORDS)]
        end = 0
        for name, nbytes in sizes:
            assert getattr(lay, name) == end and end % 256 == 0, name
            end += al256(nbytes)
        assert lay.workspace == end and lay.workspace < need


def test_create_and_run_refuse_bad_arguments_before_any_device_call():
    lib = _lib.load()
    cfg, h = _cfg(), C.c_void_p()
    need = lib.ph_dtracker_device_bytes(C.byref(cfg), 64, 16)
    assert lib.ph_dtracker_create(C.byref(cfg), C.c_void_p(FAKE_PTR), need - 256, 64, 16, C.byref(h)) == -4 and "too small" in Hh.last_error() and not h.value
    assert lib.ph_dtracker_create(C.byref(cfg), C.c_void_p(FAKE_PTR + 16), need, 64, 16, C.byref(h)) == -1 and "aligned" in Hh.last_error() and not h.value
    assert lib.ph_dtracker_create(C.byref(cfg), None, need, 64, 16, C.byref(h)) == -1 and not h.value
    assert lib.ph_dtracker_create(C.byref(cfg), C.c_void_p(FAKE_PTR), need, 64, 16, None) == -1
    assert lib.ph_dtracker_create(C.byref(cfg), C.c_void_p(FAKE_PTR), need, 64, 16, C.byref(h)) == 0 and h.value
    # run-time argument checks come back before any launch (a launch on the fake addresses would fault)
    names = ("boxes", "labels", "counts", "embeds", "kept_out", "ids_out", "kept_counts")

    def io(**kw):
        o = _lib.DtrackerIO()
        for k in names:
            setattr(o, k, kw.get(k, FAKE_PTR))
        return o
    for k in names:
        assert lib.ph_dtracker_run(h, C.byref(io(**{k: None})), 1, None) == -1 and k in Hh.last_error(), k
    assert lib.ph_dtracker_run(h, C.byref(io()), 0, None) == -1 and "B must be" in Hh.last_error()
    assert lib.ph_dtracker_run(h, None, 1, None) == -1 and lib.ph_dtracker_run(None, C.byref(io()), 1, None) == -1
    assert lib.ph_dtracker_reset(None, 1, None) == -1 and lib.ph_dtracker_get_layout(h, None) == -1
    lib.ph_dtracker_destroy(h)
    lib.ph_dtracker_destroy(None)


def test_plan_track_refuses_more_things_than_the_tracker_takes():
    lib = _lib.load()
    track = _lib.TrackCfg(num_convs=4, fc_out_channels=1024, embed_channels=256, groups=32, prec=_lib.PH_PREC_SPLIT)
    acfg = E.native_assoc_cfg(2, (64, 128), 24, 12, 8, 11, LEVELS, track)
    plan, trk, small = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.ph_assoc_plan_create(C.byref(acfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), 1 << 62, C.byref(plan)) == 0, Hh.last_error()
    cfg = _cfg()
    assert lib.ph_dtracker_create(C.byref(cfg), C.c_void_p(FAKE_PTR), 1 << 40, 64, 11, C.byref(small)) == 0
    assert lib.ph_dtracker_create(C.byref(cfg), C.c_void_p(FAKE_PTR), 1 << 40, 64, 12, C.byref(trk)) == 0
    P = C.c_void_p(FAKE_PTR)
    assert lib.ph_assoc_plan_track(plan, small, P, P, P, P, None, None) == -1 and "max_dets" in Hh.last_error() and "max_things" in Hh.last_error()
    for args in ((None, trk, P, P, P, P), (plan, None, P, P, P, P), (plan, trk, None, P, P, P), (plan, trk, P, None, P, P),
                 (plan, trk, P, P, None, P), (plan, trk, P, P, P, None)):
        assert lib.ph_assoc_plan_track(*args, None, None) == -1 and "null" in Hh.last_error()
    for h in (small, trk):
        lib.ph_dtracker_destroy(h)
    lib.ph_assoc_plan_destroy(plan)


def test_module_switch_defaults_to_the_host_tracker():
    from polyphonicformer_amd import video as V
    a = V.VideoAssociator.__new__(V.VideoAssociator)
    assert a.device_tracker is False
    assert a.use_native_plan(True, max_things=12).device_tracker is False
    assert a.use_native_plan(True, max_things=12, device_tracker=True).device_tracker is True and a.native_plan is True
    a.cnt = 1
    assert a.frames_matched() == 0 and a.device_status() is None          # no device tracker yet: nothing to read
    assert a.use_native_plan(False, device_tracker=True).device_tracker is False
