"""The cost of the first-hit planes: tptDrawDeviceAov against tptDrawDevice on the same frames, for a caller that waits for every frame
(sync) and for one that streams frames and waits once (stream).  Three interleaved repetitions per configuration; prints one JSON line
per configuration: Gray/s of both (median, min, max), AOV / plain, the kernel time of one frame each, and whether both left the same
bytes in the tile.
    python3 tools/aov_rate.py [--frames N] [--reps R] [--only 640x360|1280x720|stress]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from toypathtracer_amd import api  # noqa: E402
from toypathtracer_amd.scenes import stress_scene  # noqa: E402

FLAGS = 2  # kFlagProgressive


def draw(kind, w, h, f, tile, alb, nd):
    if kind == "aov":
        api.draw_device_aov(0.0, f, w, h, tile.data_ptr(), FLAGS, albedo_ptr=alb.data_ptr(), normal_depth_ptr=nd.data_ptr())
    else:
        api.draw_device(0.0, f, w, h, tile.data_ptr(), FLAGS)


def run(kind, sync, w, h, frames, tile, alb, nd):
    """frames 0..frames-1 on a zeroed tile -> (rays, seconds)"""
    tile.zero_()
    torch.cuda.synchronize()
    api.UpdateTest(0.0, 0, w, h, FLAGS)
    api.synchronize()
    r0 = api.ray_counter_read()
    t0 = time.perf_counter()
    for f in range(frames):
        draw(kind, w, h, f, tile, alb, nd)
        if sync:
            api.synchronize()
    api.synchronize()
    dt = time.perf_counter() - t0
    return api.ray_counter_read() - r0, dt


def kernel_ms(kind, w, h, tile, alb, nd):
    api.UpdateTest(0.0, 0, w, h, FLAGS)
    api.synchronize()
    api.kernel_timing_begin(8)
    draw(kind, w, h, 0, tile, alb, nd)
    api.synchronize()
    ms, n = api.kernel_timing_end()
    return round(ms / max(n, 1), 3)


def config(name, w, h, spp, frames, reps, scene=None):
    api.set_samples_per_pixel(spp)
    if scene:
        api.set_scene(*scene)
        api.set_camera((0.0, 6.0, 20.0), (0.0, 0.0, 0.0), 60.0, 0.02, 20.0)
    else:
        api.set_scene(None)
        api.set_camera(None)
    tiles = {k: torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for k in ("plain", "aov")}
    alb = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    nd = torch.zeros_like(alb)
    out = dict(config=name, w=w, h=h, spp=spp, frames=frames, reps=reps)
    for k in ("plain", "aov"):  # warm-up: buffers, code objects
        run(k, False, w, h, 2, tiles[k], alb, nd)
    rays = {}
    for mode in ("sync", "stream"):
        rate = {"plain": [], "aov": []}
        for _ in range(reps):  # interleaved: plain, aov, plain, aov, ...
            for k in ("plain", "aov"):
                r, dt = run(k, mode == "sync", w, h, frames, tiles[k], alb, nd)
                rays.setdefault((mode, k), r)
                rate[k].append(r / dt / 1e9)
        for k in ("plain", "aov"):
            out["%s_%s_gray_s" % (mode, k)] = round(statistics.median(rate[k]), 3)
            out["%s_%s_range" % (mode, k)] = [round(min(rate[k]), 3), round(max(rate[k]), 3)]
        out["%s_ratio" % mode] = round(statistics.median(rate["aov"]) / statistics.median(rate["plain"]), 3)
    out["rays_equal"] = rays[("sync", "plain")] == rays[("sync", "aov")] == rays[("stream", "aov")]
    out["tiles_equal"] = bool(torch.equal(tiles["plain"].view(torch.int32), tiles["aov"].view(torch.int32)))
    out["plain_kernel_ms"] = kernel_ms("plain", w, h, tiles["plain"], alb, nd)
    out["aov_kernel_ms"] = kernel_ms("aov", w, h, tiles["aov"], alb, nd)
    out["launch_info_aov"] = api.launch_info()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=0, help="frames per timed run (0: 60 / 30 / 6)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    api.InitializeTest()
    try:
        if args.only in ("", "640x360"):
            config("640x360x4", 640, 360, 4, args.frames or 60, args.reps)
        if args.only in ("", "1280x720"):
            config("1280x720x4", 1280, 720, 4, args.frames or 30, args.reps)
        if args.only in ("", "stress"):
            s, m = stress_scene(4096, 64)
            config("stress4096 960x540x8", 960, 540, 8, args.frames or 6, args.reps, scene=(s, m))
    finally:
        api.ShutdownTest()


if __name__ == "__main__":
    main()
