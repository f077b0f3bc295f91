"""The cost and the use of tptDenoiseDevice.  (1) Kernel time per call and per iteration at 1280x720 and 3840x2160 for 1..8 iterations,
with both guides and demodulation: tptTimerBegin / tptTimerEnd around --calls calls on the context stream, the median of --reps such
brackets.  (2) The quality figure of tests/test_gpu_denoise.py: at 640x360 on the default scene, the mean squared error of the denoised
4-spp frame against a 1024-spp render of the same frame, over the raw 4-spp frame's, for the api defaults and for a small grid of
sigmas around them.  One JSON line per measurement.
    python3 tools/denoise_rate.py [--calls N] [--reps R] [--no-sweep]"""
import argparse
import itertools
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from toypathtracer_amd import api  # noqa: E402

FLAGS = 2  # kFlagProgressive
D = api.DENOISE_DEFAULTS


def planes(w, h):
    g = torch.Generator(device="cuda").manual_seed(w * 31 + h)
    colour = torch.rand((h, w, 4), device="cuda", generator=g) ** 3 * 4
    albedo = torch.rand((h, w, 4), device="cuda", generator=g)
    n = torch.nn.functional.normalize(torch.randn((h, w, 3), device="cuda", generator=g), dim=-1)
    nd = torch.cat([n, torch.rand((h, w, 1), device="cuda", generator=g) * 20], dim=-1).contiguous()
    return colour.contiguous(), albedo.contiguous(), nd, torch.empty_like(colour)


def timing(w, h, calls, reps):
    colour, albedo, nd, out = planes(w, h)
    torch.cuda.synchronize()
    for it in range(1, 9):
        args = (w, h, colour.data_ptr(), out.data_ptr())
        kw = dict(albedo_ptr=albedo.data_ptr(), normal_depth_ptr=nd.data_ptr(), iterations=it)
        api.denoise_device(*args, **kw)  # (warm-up; makes the scratch plane)
        api.synchronize()
        ms = []
        for _ in range(reps):
            api.timer_begin()
            for _ in range(calls):
                api.denoise_device(*args, **kw)
            ms.append(api.timer_end() / calls)
        m = statistics.median(ms)
        print(json.dumps(dict(size="%dx%d" % (w, h), iterations=it, us_per_call=round(m * 1000, 1),
                              us_per_iteration=round(m * 1000 / it, 1), min_us=round(min(ms) * 1000, 1), max_us=round(max(ms) * 1000, 1))),
              flush=True)


def quality(sweep):
    w, h = 640, 360
    api.set_samples_per_pixel(1024)
    ref = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    api.UpdateTest(0.0, 0, w, h, FLAGS)
    api.draw_device(0.0, 0, w, h, ref.data_ptr(), FLAGS)
    api.synchronize()
    api.set_samples_per_pixel(4)
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    alb = torch.zeros_like(tile)
    nd = torch.zeros_like(tile)
    out = torch.zeros_like(tile)
    torch.cuda.synchronize()
    api.UpdateTest(0.0, 0, w, h, FLAGS)
    api.draw_device_aov(0.0, 0, w, h, tile.data_ptr(), FLAGS, albedo_ptr=alb.data_ptr(), normal_depth_ptr=nd.data_ptr())
    api.synchronize()
    r = ref[..., :3].double()
    raw = float(((tile[..., :3].double() - r) ** 2).mean())

    def ratio(**kw):
        api.denoise_device(w, h, tile.data_ptr(), out.data_ptr(), albedo_ptr=alb.data_ptr(), normal_depth_ptr=nd.data_ptr(), **kw)
        api.synchronize()
        return float(((out[..., :3].double() - r) ** 2).mean()) / raw

    print(json.dumps(dict(quality="defaults", mse_raw=raw, ratio=round(ratio(), 4), **D)), flush=True)
    if not sweep:
        return
    print(json.dumps(dict(quality="blur", ratio=round(ratio(sigma_colour=0.0, sigma_normal=0.0, sigma_depth=0.0), 4))), flush=True)
    for it, sc, sn, sd in itertools.product((4, 5), (1.0, 4.0, 16.0, 32.0, 64.0), (0.03, 0.1, 0.3), (0.5, 2.0)):
        print(json.dumps(dict(quality="sweep", iterations=it, sigma_colour=sc, sigma_normal=sn, sigma_depth=sd,
                              ratio=round(ratio(iterations=it, sigma_colour=sc, sigma_normal=sn, sigma_depth=sd), 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-sweep", action="store_true")
    a = ap.parse_args()
    api.InitializeTest()
    try:
        print(json.dumps(dict(device=api.device_name(), defaults=D)), flush=True)
        for w, h in ((1280, 720), (3840, 2160)):
            timing(w, h, a.calls, a.reps)
        quality(not a.no_sweep)
    finally:
        api.ShutdownTest()


if __name__ == "__main__":
    main()
