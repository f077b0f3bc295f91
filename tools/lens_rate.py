"""The rate of tptDrawDeviceLens against the route it replaces and against its ceiling: an equirectangular image (2048x1024 by default)
at 4 and at 32 samples per pixel, three ways --
  lens       one tptDrawDeviceLens call: the rays made on the device, all samples of a pixel in one launch
  rays       what a caller did before: the directions made with numpy on the host, a 32-byte record per ray uploaded, and per sample
             one seed pass with torch, one tptTraceRaysDevice call and one torch accumulation (the former examples/panorama.py)
  draw       tptDrawDevice through the thin-lens camera on the lane-refill kernel (tptSetKernelVariant(0, 1, -1)) at the same size and
             sample count: the kernel the lens draw runs, fed by the camera -- the ceiling
Every way once per round, the order rotating, `--reps` rounds, each image between two synchronisations; `rays` is timed with and
without its host part (directions and upload, which a caller pays once per image size).  The three trace different paths (other
directions, other seeds): the rates are HitWorld calls per second of each.  Prints one JSON line per sample count.
    python3 tools/lens_rate.py [--size WxH] [--spp 4,32] [--reps R]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from toypathtracer_amd import api  # noqa: E402

EYE = (0.0, 1.0, 0.0)


def host_rays(w, h):
    """the caller's own panorama camera: [h * w, 8] float32 records, pixel centres, unit directions"""
    lon = (np.arange(w, dtype=np.float64) + 0.5) / w * 2.0 * np.pi - np.pi
    lat = (np.arange(h, dtype=np.float64) + 0.5) / h * np.pi - np.pi / 2
    lon, lat = np.meshgrid(lon, lat)
    d = np.stack([np.cos(lat) * np.sin(lon), np.sin(lat), -np.cos(lat) * np.cos(lon)], axis=-1).reshape(-1, 3)
    d32 = d.astype(np.float32)
    rays = np.zeros((w * h, 8), np.float32)
    rays[:, 0:3] = EYE
    rays[:, 4:7] = d32 / np.sqrt((d32.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(np.float32)
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="2048x1024")
    ap.add_argument("--spp", default="4,32")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    n = w * h
    api.InitializeTest()
    try:
        api.set_seed_mode(api.SEED_PER_PIXEL)  # (the lens draw's seeds, for the camera's draw too)
        api.UpdateTest(0.0, 0, w, h, 0)
        lens = api.lens_equirect(origin=EYE)
        tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        radiance = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        total = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        index = torch.arange(n, dtype=torch.int64, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def image(way, spp):
            """one image -> (HitWorld calls, seconds, seconds of the host part)"""
            api.set_samples_per_pixel(spp)
            api.set_kernel_variant(0, 1, -1)
            api.UpdateTest(0.0, 0, w, h, 0)
            cnt.zero_()
            torch.cuda.synchronize()
            api.synchronize()
            r0 = api.ray_counter_read()
            host = 0.0
            t0 = time.perf_counter()
            if way == "lens":
                api.draw_device_lens(0, w, h, tile.data_ptr(), lens, 0, cnt.data_ptr())
            elif way == "draw":
                api.draw_device(0.0, 0, w, h, tile.data_ptr(), 0)
            else:
                rays = torch.from_numpy(host_rays(w, h)).cuda()
                torch.cuda.synchronize()
                host = time.perf_counter() - t0
                seeds = rays[:, 3].view(torch.int32)
                total.zero_()
                for p in range(spp):
                    s = ((index * 1973 + p * 26699 + 9277) * 2654435761) & 0x7FFFFFFF
                    seeds.copy_((s | 1).to(torch.int32))
                    torch.cuda.synchronize()  # (torch's stream and the library's are not the same one)
                    api.trace_rays_device(n, rays.data_ptr(), radiance.data_ptr(), None, cnt.data_ptr())
                    api.synchronize()
                    total.add_(radiance)
                tile.copy_((total / spp).view(h, w, 4))
                torch.cuda.synchronize()
            api.synchronize()
            dt = time.perf_counter() - t0
            return (api.ray_counter_read() - r0) + int(cnt.item()), dt, host

        ways = ["lens", "rays", "draw"]
        for spp in (int(v) for v in args.spp.split(",")):
            for way in ways:  # warm-up: buffers, code objects
                image(way, spp)
            ms, ms_dev, rate, traced = {k: [] for k in ways}, [], {k: [] for k in ways}, {}
            for rep in range(args.reps):
                for way in ways[rep % 3:] + ways[:rep % 3]:
                    r, dt, host = image(way, spp)
                    traced[way] = r
                    ms[way].append(dt * 1e3)
                    rate[way].append(r / dt / 1e6)
                    if way == "rays":
                        ms_dev.append((dt - host) * 1e3)
            med = {k: statistics.median(ms[k]) for k in ways}
            out = dict(size=args.size, spp=spp, reps=args.reps, device=api.device_name(), hitworld_calls=traced)
            for k in ways:
                out[k + "_ms"] = round(med[k], 2)
                out[k + "_ms_range"] = [round(min(ms[k]), 2), round(max(ms[k]), 2)]
                out[k + "_mray_s"] = round(statistics.median(rate[k]), 1)
            out["rays_ms_without_host_part"] = round(statistics.median(ms_dev), 2)
            out["lens_time_over_rays"] = round(med["lens"] / med["rays"], 3)
            out["lens_time_over_rays_without_host_part"] = round(med["lens"] / statistics.median(ms_dev), 3)
            out["lens_rate_over_draw"] = round(statistics.median(rate["lens"]) / statistics.median(rate["draw"]), 3)
            print(json.dumps(out), flush=True)
    finally:
        api.ShutdownTest()


if __name__ == "__main__":
    main()
