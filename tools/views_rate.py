"""K views of one scene per frame: one tptDrawDeviceViews call against K set-camera / update / tptDrawDevice sequences (same cameras,
same frames).  Prints one JSON line per configuration: Gray/s of both, the views launch's tptGetLaunchInfo, and whether both ways left
the same bytes in every view's tile.
    python3 tools/views_rate.py [--frames N] [--warmup W] [--only 640x360|1280x720|stress]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from toypathtracer_amd import api  # noqa: E402
from toypathtracer_amd.scenes import stress_scene  # noqa: E402

FLAGS = 2  # kFlagProgressive


def ring(k, radius, height, look_at, vfov, aperture, focus):
    out = []
    for i in range(k):
        a = 2.0 * math.pi * i / k
        out.append([radius * math.sin(a), height, radius * math.cos(a)] + list(look_at) + [vfov, aperture, focus])
    return out


def run_views(w, h, views, frames, tiles):
    for f in frames:
        api.UpdateTest(0.0, f, w, h, FLAGS)
        api.draw_device_views(0.0, f, w, h, views, tiles.data_ptr(), FLAGS)


def run_sequential(w, h, views, frames, tiles):
    for f in frames:
        for v, p in enumerate(views):
            api.set_camera(p[0:3], p[3:6], p[6], p[7], p[8])
            api.UpdateTest(0.0, f, w, h, FLAGS)
            api.draw_device(0.0, f, w, h, tiles[v].data_ptr(), FLAGS)
    api.set_camera(None)


def measure(fn, w, h, views, warmup, frames, tiles):
    tiles.zero_()
    torch.cuda.synchronize()
    fn(w, h, views, range(warmup), tiles)
    api.synchronize()
    r0 = api.ray_counter_read()
    t0 = time.perf_counter()
    fn(w, h, views, range(warmup, warmup + frames), tiles)
    api.synchronize()
    dt = time.perf_counter() - t0
    rays = api.ray_counter_read() - r0
    return rays, dt


def config(name, w, h, spp, views, warmup, frames, scene=None):
    api.set_samples_per_pixel(spp)
    if scene:
        api.set_scene(*scene)
    else:
        api.set_scene(None)
    k = len(views)
    a = torch.zeros((k, h, w, 4), dtype=torch.float32, device="cuda")
    b = torch.zeros_like(a)
    rv, tv = measure(run_views, w, h, views, warmup, frames, a)
    info = api.launch_info()
    rs, ts = measure(run_sequential, w, h, views, warmup, frames, b)
    # kernel time of one call: the views launch against the K launches of the sequence
    api.UpdateTest(0.0, 0, w, h, FLAGS)
    api.kernel_timing_begin(64)
    run_views(w, h, views, [warmup + frames], a)
    kv = api.kernel_timing_end()
    api.kernel_timing_begin(64)
    run_sequential(w, h, views, [warmup + frames], b)
    ks = api.kernel_timing_end()
    same = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
    out = dict(config=name, w=w, h=h, spp=spp, views=k, frames=frames, rays_equal=rv == rs, tiles_equal=same,
               views_gray_s=round(rv / tv / 1e9, 3), sequential_gray_s=round(rs / ts / 1e9, 3), speedup=round((rv / tv) / (rs / ts), 3),
               views_ms_per_frame=round(tv / frames * 1e3, 3), sequential_ms_per_frame=round(ts / frames * 1e3, 3),
               views_kernel_ms=round(kv[0], 3), views_launches=kv[1], sequential_kernel_ms=round(ks[0], 3), sequential_launches=ks[1],
               launch_info=info)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=0, help="timed frames per configuration (0: 30 / 20 / 8)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    api.InitializeTest()
    try:
        cam = ring(8, 3.0, 2.0, (0.0, 0.0, 0.0), 60.0, 0.02, 3.0)
        if args.only in ("", "640x360"):
            config("640x360x4 K=8", 640, 360, 4, cam, args.warmup, args.frames or 30)
        if args.only in ("", "1280x720"):
            config("1280x720x4 K=4", 1280, 720, 4, cam[::2], args.warmup, args.frames or 20)
        if args.only in ("", "stress"):
            s, m = stress_scene(4096, 64)
            config("stress4096 960x540x8 K=4", 960, 540, 8, ring(4, 20.0, 6.0, (0.0, 0.0, 0.0), 60.0, 0.02, 20.0), args.warmup,
                   args.frames or 8, scene=(s, m))
    finally:
        api.ShutdownTest()


if __name__ == "__main__":
    main()
