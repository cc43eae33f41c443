"""The library's switch table (include/polyhead.h PH_SWITCH_*, ph_set_switch / ph_get_switch) and its binding _lib.switches: set and
get by call, refusals that change nothing, the one read of the environment at first use -- host only, nothing here touches a GPU --
and, on the GPU, that a captured graph keeps the value it was captured with."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

import helpers as Hh
from polyphonicformer_amd import _lib, engine as E

ENV_NAMES = ("PH_CONV_WGS", "PH_UP2_WGS", "PH_QUERY_NRT", "PH_QUERY_TIMELINE", "PH_CONV_TH", "PH_CONV_TH_NOW", "PH_GNSUM_WGS",
             "PH_CPLANES_TPW", "PH_PAN_GENERIC")
# a value every switch takes, and one it refuses (beside any negative one)
GOOD = dict(conv_wgs=5, up2_wgs=7, query_nrt=2, query_timeline=1, conv_tile_rows=4, gnsum_wgs=3, cplanes_tpw=2, pan_generic=1)
BAD = dict(conv_wgs=-1, up2_wgs=-2, query_nrt=-1, query_timeline=2, conv_tile_rows=3, gnsum_wgs=-1, cplanes_tpw=-1, pan_generic=2)


def _get(i):
    v = C.c_int(-99)
    assert _lib.load().ph_get_switch(i, C.byref(v)) == 0
    return v.value


def _all():
    return [_get(i) for i in range(len(_lib.SWITCHES))]


def test_set_then_get_round_trips_for_every_id():
    lib = _lib.load()
    assert set(GOOD) == set(BAD) == set(_lib.SWITCHES)
    before = _all()
    try:
        for i, name in enumerate(_lib.SWITCHES):
            want = _all()
            for v in (GOOD[name], 0):
                want[i] = v
                assert lib.ph_set_switch(i, v) == 0, (name, v)
                assert _all() == want, (name, v)                  # this one changed, no other did
    finally:
        for i, v in enumerate(before):
            assert lib.ph_set_switch(i, v) == 0
    assert _all() == before


def test_bad_id_and_bad_values_are_refused_and_change_nothing():
    lib = _lib.load()
    with _lib.switches(**GOOD):
        want = [GOOD[n] for n in _lib.SWITCHES]
        for bad_id in (-1, len(_lib.SWITCHES), 1 << 20):
            v = C.c_int(-99)
            assert lib.ph_set_switch(bad_id, 0) == _lib.PH_EINVAL and b"ph_set_switch" in lib.ph_last_error_string()
            assert lib.ph_get_switch(bad_id, C.byref(v)) == _lib.PH_EINVAL and v.value == -99
            assert b"ph_get_switch" in lib.ph_last_error_string()
        assert lib.ph_get_switch(0, None) == _lib.PH_EINVAL
        for i, name in enumerate(_lib.SWITCHES):
            for bad in (BAD[name], -1, -(1 << 31)):
                assert lib.ph_set_switch(i, bad) == _lib.PH_EINVAL, (name, bad)
                assert b"ph_set_switch" in lib.ph_last_error_string()
        for bad in (1, 3, 5, 8):
            assert lib.ph_set_switch(_lib.SWITCHES.index("conv_tile_rows"), bad) == _lib.PH_EINVAL
        assert _all() == want


def test_switches_restores_on_exit_and_on_an_exception():
    before = _all()
    i, j = _lib.SWITCHES.index("up2_wgs"), _lib.SWITCHES.index("conv_tile_rows")
    with _lib.switches(up2_wgs=7):
        assert _get(i) == 7
        with _lib.switches(up2_wgs=3, conv_tile_rows=2):           # nested: back to the outer value
            assert (_get(i), _get(j)) == (3, 2)
        assert (_get(i), _get(j)) == (7, before[j])
    assert _all() == before
    with pytest.raises(ZeroDivisionError):
        with _lib.switches(up2_wgs=5, pan_generic=1):
            assert _get(i) == 5
            1 / 0
    assert _all() == before
    with pytest.raises(_lib.PolyheadError):                       # a refused value: what was set before it is put back, the block not entered
        with _lib.switches(up2_wgs=5, conv_tile_rows=3):
            raise AssertionError("entered")
    assert _all() == before
    with pytest.raises(ValueError):
        with _lib.switches(no_such_switch=1):
            raise AssertionError("entered")
    assert _all() == before


_REPORT = """
import ctypes as C, json
from polyphonicformer_amd import _lib
lib = _lib.load()
out = {}
for i, name in enumerate(_lib.SWITCHES):
    v = C.c_int(-99)
    assert lib.ph_get_switch(i, C.byref(v)) == 0
    out[name] = v.value
import torch
assert not torch.cuda.is_initialized()
print(json.dumps(out))
"""


def _report(env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ENV_NAMES}
    r = subprocess.run([sys.executable, "-c", _REPORT], cwd=Hh.REPO, env=dict(env, **env_extra), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_environment_is_read_at_first_use():
    """every documented spelling, and the precedence of the retired one: PH_CONV_TH_NOW wins over PH_CONV_TH, as it did when the
    library read it on every call"""
    got = _report(dict(PH_CONV_WGS="5", PH_UP2_WGS="7", PH_PAN_GENERIC="1", PH_CONV_TH="4", PH_CONV_TH_NOW="2"))
    assert got == dict(conv_wgs=5, up2_wgs=7, query_nrt=0, query_timeline=0, conv_tile_rows=2, gnsum_wgs=0, cplanes_tpw=0, pan_generic=1)
    # the other four spellings; values ph_set_switch would refuse are ignored (PH_CONV_TH=3, a negative count)
    got = _report(dict(PH_QUERY_NRT="2", PH_QUERY_TIMELINE="1", PH_GNSUM_WGS="3", PH_CPLANES_TPW="2", PH_CONV_TH="3", PH_UP2_WGS="-4"))
    assert got == dict(conv_wgs=0, up2_wgs=0, query_nrt=2, query_timeline=1, conv_tile_rows=0, gnsum_wgs=3, cplanes_tpw=2, pan_generic=0)


def test_no_variable_set_means_all_zeros():
    assert _report({}) == {n: 0 for n in _lib.SWITCHES}


@pytest.mark.gpu
def test_a_captured_graph_keeps_the_value_it_was_captured_with(gpu):
    """ph_dynconv_up2_wgs captured with the up2 switch at 0, replayed with it at 5: the replay writes the captured run's bits and the
    graph's kernel node keeps the capture's grid, while a fresh launch takes 5 workgroups.  (145, 2, 3): the smallest shape of
    tests/test_gpu_kernels.py's sweep with more than 5 image rows -- the count is capped at B * H, so on fewer rows 5 changes nothing"""
    N, H, B, W = 145, 2, 3, 256
    prec, dt, oc = _lib.PH_PREC_F16, torch.float16, _lib.PH_OUT_F16
    assert _lib.load().ph_dynconv_up2_supported(N, H, W, prec, oc) == 1
    g = torch.Generator().manual_seed(43 + N + H)
    Npad = E.n_padded(N)
    x = torch.randn(B, 256, H, W, generator=g)
    kern = (torch.randn(2, B, Npad, 256, generator=g) * 0.1).to(dt).view(torch.int16)[None].contiguous().to(gpu)
    kbias = (torch.randn(2, B, Npad, generator=g) * 0.1).to(gpu)
    xp = E.ingest(x.to(gpu), prec)
    up = torch.full((B, N, 2 * H, 2 * W), float("nan"), device=gpu, dtype=dt)
    run = lambda: E.dynconv_up2(xp, kern, kbias, 0, N, H, W, prec, up, logits_out=None, out_dtype=oc)
    with _lib.switches(up2_wgs=0):
        run()                                                     # outside the capture: the module load
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph):
            run()
        nodes0 = Hh.graph_kernel_nodes(None, graph=graph)
        graph.replay()
        torch.cuda.synchronize()
        want = up.clone()
    assert not torch.isnan(want.float()).any()
    assert len(nodes0) == 1 and nodes0[0][:3] == [B * H, 1, 1]    # one workgroup per image row (fewer rows than CUs)
    with _lib.switches(up2_wgs=5):
        up.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(up, want)
        assert Hh.graph_kernel_nodes(None, graph=graph) == nodes0
        fresh = Hh.graph_kernel_nodes(run)                        # the public entry point does listen
        assert len(fresh) == 1 and fresh[0][:3] == [5, 1, 1] and fresh[0][3:] == nodes0[0][3:]
        assert torch.equal(up, want)                              # same values whatever the count
