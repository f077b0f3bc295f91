"""The rate of tptTraceRaysDevice against the draws that trace the same paths.  The rays are those a 1280x720 frame's first samples
start with (tests/rays_checker.c's camera_rays: the pixel's seed, two jitter draws, Camera::GetRay, the state left behind as the seed
word), so the ray call, `tptDrawDevice` at 1 spp under tptSetKernelVariant(1, 1, -1) and (0, 1, -1) -- the lane-refill kernel the ray
call runs, with the simple and the two-phase HitSpheres -- and `tptDrawDevice` on the default path-queue kernel all trace the very same
920 k paths.  Every variant once per round, the order rotating, `--reps` rounds of `--calls` calls each between two tptSynchronize;
the lane-refill draw and the ray call also with a tptSynchronize after every call; prints one JSON line: Mray/s of each (median,
range), the ratios, and whether the radiance equals the draw's colour bytes.
    python3 tools/rays_rate.py [--calls N] [--reps R] [--size WxH]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from rays_lib import RaysChecker  # noqa: E402
from toypathtracer_amd import api  # noqa: E402

VARIANTS = {"draw_queue": (0, 3, -1), "draw_refill_two_phase": (0, 1, -1), "draw_refill_simple": (1, 1, -1),
            "rays_two_phase": (0, 1, -1), "rays_simple": (1, 1, -1), "rays_two_phase_hits_only": (0, 1, -1),
            # ... and with a tptSynchronize after every call: one launch at a time, as the ray calls run anyway (they share the context
            # stream, the draws' launches run side by side on the trace streams)
            "draw_refill_two_phase_sync": (0, 1, -1), "rays_two_phase_sync": (0, 1, -1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", default="1280x720")
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    n = w * h
    api.InitializeTest()
    try:
        api.set_samples_per_pixel(1)
        api.UpdateTest(0.0, 0, w, h, 0)
        cam = api.GetSceneDesc()[2]
        rays = torch.from_numpy(RaysChecker(tempfile.mkdtemp(prefix="rays_rate_")).camera_rays(cam, w, h, 0)).cuda()
        rad = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        hits = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
        tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def bracket(name, calls):
            """`calls` calls of one variant between two synchronisations -> (rays traced, seconds)"""
            api.set_kernel_variant(*VARIANTS[name])
            api.UpdateTest(0.0, 0, w, h, 0)
            cnt.zero_()
            torch.cuda.synchronize()
            api.synchronize()
            r0 = api.ray_counter_read()
            t0 = time.perf_counter()
            for _ in range(calls):
                if name.startswith("draw"):
                    api.draw_device(0.0, 0, w, h, tile.data_ptr(), 0)
                elif name.endswith("hits_only"):
                    api.trace_rays_device(n, rays.data_ptr(), None, hits.data_ptr(), cnt.data_ptr())
                else:
                    api.trace_rays_device(n, rays.data_ptr(), rad.data_ptr(), None, cnt.data_ptr())
                if name.endswith("_sync"):
                    api.synchronize()
            api.synchronize()
            dt = time.perf_counter() - t0
            return (api.ray_counter_read() - r0) + int(cnt.item()), dt

        names = list(VARIANTS)
        for name in names:  # warm-up: buffers, code objects
            bracket(name, 2)
        same = bool(torch.equal(rad.view(h, w, 4)[..., :3].view(torch.int32), tile[..., :3].view(torch.int32)))
        rate = {k: [] for k in names}
        traced = {}
        for rep in range(args.reps):
            for name in names[rep % len(names):] + names[:rep % len(names)]:
                r, dt = bracket(name, args.calls)
                traced[name] = r // args.calls
                rate[name].append(r / dt / 1e6)
        out = dict(size=args.size, rays_per_call=n, calls=args.calls, reps=args.reps, device=api.device_name(), radiance_equals_draw=same,
                   hitworld_calls_per_call=traced)
        for k in names:
            out[k + "_mray_s"] = round(statistics.median(rate[k]), 1)
            out[k + "_range"] = [round(min(rate[k]), 1), round(max(rate[k]), 1)]
        med = {k: statistics.median(rate[k]) for k in names}
        out["rays_over_refill_two_phase"] = round(med["rays_two_phase"] / med["draw_refill_two_phase"], 3)
        out["rays_over_refill_simple"] = round(med["rays_simple"] / med["draw_refill_simple"], 3)
        out["rays_over_refill_two_phase_sync"] = round(med["rays_two_phase_sync"] / med["draw_refill_two_phase_sync"], 3)
        out["rays_over_queue"] = round(med["rays_two_phase"] / med["draw_queue"], 3)
        print(json.dumps(out), flush=True)
    finally:
        api.ShutdownTest()


if __name__ == "__main__":
    main()
