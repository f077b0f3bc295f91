"""Child process of tests/test_gpu_stream_depth.py: streams frames 0 .. n-1 of w x h x spp into a device tile (enqueue, enqueue, ...,
one synchronise), once with stream batching on and once off, in a process whose pipeline depth the parent pins with TPT_HW_QUEUES.
Prints one JSON line: the depth, and per pass the trace launches, the ray total and the tile's hash.
    TPT_HW_QUEUES=<q> python tests/stream_depth_child.py <w> <h> <spp> <frames>"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from oracle_lib import FLAG_PROGRESSIVE, fnv1a  # noqa: E402
from toypathtracer_amd import api as tpt  # noqa: E402

w, h, spp, frames = (int(v) for v in sys.argv[1:5])
tpt.InitializeTest()
tpt.set_samples_per_pixel(spp)
out = dict(pipeline=tpt.pipeline_info())
for batching in (True, False):
    tpt.set_stream_batching(batching)
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r0 = tpt.ray_counter_read()
    tpt.kernel_timing_begin(frames)
    for f in range(frames):
        tpt.UpdateTest(0.0, f, w, h, FLAG_PROGRESSIVE)
        tpt.draw_device(0.0, f, w, h, tile.data_ptr(), FLAG_PROGRESSIVE)
    tpt.synchronize()
    _, launches = tpt.kernel_timing_end()
    out["on" if batching else "off"] = dict(launches=launches, rays=tpt.ray_counter_read() - r0, fnv="%08x" % fnv1a(tile.cpu().numpy()))
tpt.ShutdownTest()
print(json.dumps(out))
