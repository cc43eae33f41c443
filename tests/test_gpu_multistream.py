"""GPU: `video.MultiStreamRunner` -- S live streams per launch over one tracker bank -- against the parent's way of serving S cameras:
one `VideoStreamRunner(pipe, meta, graph=False).run_one` loop per stream.  Bit equality of all three maps: both sides run the
frame-invariant heads and `ph_panoptic_select`'s candidate order."""
import numpy as np
import pytest
import torch

import test_gpu_video as GV
from polyphonicformer_amd import video as V

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

STEPS, STREAMS = 4, 3
IDLE = (1, 2)                  # step 1: stream 2 has no frame
RESET = (2, 1)                 # in front of step 2: stream 1's camera starts a new video


def _streams(gpu):
    """the fp16 cfg3 pipeline of test_gpu_video._small_stream and three streams of 256 x 512 frames by its recipe (a seeded base
    frame, rolled from frame to frame), a different seed per stream"""
    pipe, frames0, meta = GV._small_stream(gpu, STEPS, 71)
    streams = [frames0]
    for seed in (72, 73):
        g = torch.Generator().manual_seed(seed)
        base = [torch.randn(1, 256, 256 // s, 512 // s, generator=g).to(gpu) for s in (4, 8, 16, 32)]
        streams.append([tuple(torch.roll(t, (f, 2 * f), dims=(2, 3)) for t in base) for f in range(STEPS)])
    return pipe, streams, meta[0]


def test_three_streams_equal_three_single_stream_loops(gpu):
    pipe, streams, meta = _streams(gpu)
    # the single-stream loops, one stream after the other through the pipeline's own associator
    want = [[None] * STREAMS for _ in range(STEPS)]
    for s in range(STREAMS):
        pipe.init_tracker()
        runner = V.VideoStreamRunner(pipe, meta, graph=False)
        for t in range(STEPS):
            if (t, s) == IDLE:
                continue
            if (t, s) == RESET:
                pipe.init_tracker()
            want[t][s] = runner.run_one(streams[s][t])[0]
    pipe.init_tracker()
    multi = V.MultiStreamRunner(pipe, meta, STREAMS)
    ids_seen = [[set() for _ in range(STREAMS)] for _ in range(STEPS)]
    for t in range(STEPS):
        if t == RESET[0]:
            multi.init_tracker(stream=RESET[1])
        x = tuple(torch.cat([streams[s][t][l] for s in range(STREAMS)], 0) for l in range(4))
        active = [0 if (t, s) == IDLE else 1 for s in range(STREAMS)] if t == IDLE[0] else None
        got = multi.step(x, active)
        assert len(got) == STREAMS
        for s in range(STREAMS):
            if (t, s) == IDLE:
                assert got[s] is None
                continue
            g, w = got[s][0], want[t][s]
            assert g["sem"].dtype == np.uint8 and g["track"].dtype == np.float64 and g["depth"].dtype == np.float32
            assert np.array_equal(g["sem"], w["sem"]), (t, s)
            assert np.array_equal(g["track"], w["track"]), (t, s)
            assert np.array_equal(g["depth"], w["depth"]), (t, s)
            ids_seen[t][s] = set(np.unique(g["track"]).astype(np.int64).tolist()) - {0}
    # the comparison is about something: track ids in every stream's every frame; the reset restarted stream 1's frame count only
    assert all(ids_seen[t][s] for t in range(STEPS) for s in range(STREAMS) if (t, s) != IDLE)
    assert [multi.frames_matched(s) for s in range(STREAMS)] == [STEPS, STEPS - RESET[0], STEPS - 1]
    assert all(multi.device_status(s)["error"] == 0 for s in range(STREAMS))
