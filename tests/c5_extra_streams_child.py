"""Child process of tests/test_gpu_parity.py::test_grouped_kernel_is_exact_beside_16_extra_streams: opens 16 extra streams beside the
library's own, on the hardware queues the process was started with, and renders frames 0-2 of the 4096-sphere scene `sets` times,
three in flight.  Prints one JSON line: how many sets differ from the committed oracle hashes.
    python tests/c5_extra_streams_child.py <sets> <hit-spheres variant>"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if len(sys.argv) > 2 and sys.argv[2] == "4":  # the groups' bounds on the matrix cores: in the hooks build of the library only
    os.environ["TPT_LIB"] = os.path.join(ROOT, "toypathtracer_amd", "lib", "libtoypathtracer_hip_hooks.so")
import torch  # noqa: E402

torch.cuda.init()
torch.zeros(1, device="cuda")
from common import oracle_goldens  # noqa: E402
from oracle_lib import fnv1a  # noqa: E402
from toypathtracer_amd import api as tpt  # noqa: E402
from toypathtracer_amd.scenes import STRESS_CAMERA, stress_scene  # noqa: E402

sets, variant = int(sys.argv[1]), int(sys.argv[2])
streams = []
for _ in range(16):
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        torch.zeros(16, device="cuda").add_(1.0)
    streams.append(st)
torch.cuda.synchronize()
want = sorted(oracle_goldens(), key=lambda c: c["frame"])
tpt.InitializeTest()
s, m = stress_scene(4096, 64)
tpt.set_scene(s, m)
tpt.set_camera(**STRESS_CAMERA)
tpt.set_samples_per_pixel(8)
tpt.set_kernel_variant(variant, 3, -1)
info = tpt.scene_info()
W, H = 1920, 1080
bad, seen = 0, {}
for r in range(sets):
    tiles = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
    r0 = tpt.ray_counter_read()
    for f in range(3):
        tpt.UpdateTest(0.0, f, W, H, 2)
        tpt.draw_device(0.0, f, W, H, tiles[f].data_ptr(), 2)
    tpt.synchronize()
    rays = tpt.ray_counter_read() - r0
    key = (rays,) + tuple("%08x" % fnv1a(t.cpu().numpy()) for t in tiles)
    seen[key] = seen.get(key, 0) + 1
    if key != (sum(c["rays"] for c in want),) + tuple(c["fnv"] for c in want):
        bad += 1
pipe = tpt.pipeline_info() if hasattr(tpt, "pipeline_info") else None
tpt.ShutdownTest()
print(json.dumps(dict(sets=sets, renders=3 * sets, sets_differing_from_the_oracle=bad, distinct_results=len(seen), scene_info=info, pipeline=pipe)))
