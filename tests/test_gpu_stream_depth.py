"""Stream batching of large frames when the pipeline is shallow (csrc/tpt_stream_batch.h): a streaming caller of 1280x720x4 frames gets
several frames per launch when only two launches can be in flight, one per launch with the full pipeline, and the same tile and ray total
as without batching either way."""
import json
import os
import subprocess
import sys

import pytest

from oracle_lib import FLAG_PROGRESSIVE

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, SPP, FRAMES = 1280, 720, 4, 24


@pytest.mark.gpu
def test_streaming_1280x720_batched_equals_unbatched_in_this_process(tpt_defaults):
    """in this process, with whatever queues it was given: batching on and off give the same tile and ray total, and a pipeline of at
    most two launches traces the frames in fewer launches than frames"""
    import torch
    tpt = tpt_defaults
    depth = tpt.pipeline_info()["overlap_effective"]
    got = {}
    try:
        for batching in (True, False):
            tpt.set_stream_batching(batching)
            tile = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            r0 = tpt.ray_counter_read()
            tpt.kernel_timing_begin(FRAMES)
            for f in range(FRAMES):
                tpt.UpdateTest(0.0, f, W, H, FLAG_PROGRESSIVE)
                tpt.draw_device(0.0, f, W, H, tile.data_ptr(), FLAG_PROGRESSIVE)
            tpt.synchronize()
            _, launches = tpt.kernel_timing_end()
            got[batching] = (launches, tpt.ray_counter_read() - r0, tile.cpu().numpy().tobytes())
    finally:
        tpt.set_stream_batching(True)
    assert got[True][1] == got[False][1] and got[True][2] == got[False][2], (depth, got[True][:2], got[False][:2])
    assert got[False][0] == FRAMES
    if depth <= 2:
        assert got[True][0] < FRAMES, (depth, got[True][0])


def _child(queues):
    env = dict(os.environ, TPT_HW_QUEUES=str(queues))
    out = subprocess.run([sys.executable, os.path.join(HERE, "stream_depth_child.py"), str(W), str(H), str(SPP), str(FRAMES)], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    return json.loads(out.stdout.decode().strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("queues,depth", [(2, 2), (16, 16)])
def test_streaming_1280x720_at_a_pinned_depth(queues, depth):
    """a child process with the queue probe overridden (TPT_HW_QUEUES): two launches in flight -> 2, 4, 8, 8, ... frames per launch
    (24 frames: two plain launches, then batches of 2 + 4 + 8 + 8 frames, the last 6 beyond the stream dropped at the synchronise);
    sixteen -> one frame per launch as before.  Same tile and ray total as without batching."""
    r = _child(queues)
    assert r["pipeline"]["overlap_effective"] == depth, r
    assert r["on"]["rays"] == r["off"]["rays"] and r["on"]["fnv"] == r["off"]["fnv"], r
    assert r["off"]["launches"] == FRAMES
    assert r["on"]["launches"] == (6 if depth == 2 else FRAMES), r
