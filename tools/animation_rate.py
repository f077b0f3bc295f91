"""Frames of the animated scene (kFlagAnimate): (a) tptUpdate + tptDrawDevice per frame, (b) tptDrawDeviceAnimation with 32 frames per
call, (c) tptDrawDeviceBatch on the same frames with the scene static (the ceiling: one launch per 32 frames, nothing moves).  The modes
run interleaved, --runs times each, in one process.  Prints one JSON line per (size, mode, run) -- ms per frame, Gray/s -- and one summary
line per size with the medians, the ratio (b) / (c) and whether (a) and (b) left the same bytes in the tile.
    python3 tools/animation_rate.py [--frames N] [--warmup W] [--runs R] [--only 640x360|1280x720]"""
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

PROGRESSIVE, ANIMATED = 2, 3  # kFlagProgressive, | kFlagAnimate
PER_CALL = 32


def times_of(frames):
    return [f / 60.0 for f in frames]  # a clip at 60 frames per second


def run_sequence(w, h, frames, tile):
    for f, t in zip(frames, times_of(frames)):
        api.UpdateTest(t, f, w, h, ANIMATED)
        api.draw_device(t, f, w, h, tile.data_ptr(), ANIMATED)


def run_animation(w, h, frames, tile):
    frames = list(frames)
    api.UpdateTest(times_of(frames[:1])[0], frames[0], w, h, ANIMATED)
    for k in range(0, len(frames), PER_CALL):
        part = frames[k:k + PER_CALL]
        api.draw_device_animation(times_of(part), part[0], w, h, tile.data_ptr(), ANIMATED)


def run_static_batch(w, h, frames, tile):
    frames = list(frames)
    api.UpdateTest(0.0, frames[0], w, h, PROGRESSIVE)
    for k in range(0, len(frames), PER_CALL):
        part = frames[k:k + PER_CALL]
        api.draw_device_batch(0.0, part[0], len(part), w, h, tile.data_ptr(), PROGRESSIVE)


MODES = {"a_update_draw": run_sequence, "b_animation": run_animation, "c_static_batch": run_static_batch}


def measure(fn, w, h, warmup, frames, tile):
    tile.zero_()
    torch.cuda.synchronize()
    fn(w, h, range(warmup), tile)
    api.synchronize()
    r0 = api.ray_counter_read()
    t0 = time.perf_counter()
    fn(w, h, range(warmup, warmup + frames), tile)
    api.synchronize()
    dt = time.perf_counter() - t0
    return api.ray_counter_read() - r0, dt


def size(name, w, h, spp, warmup, frames, runs):
    api.set_samples_per_pixel(spp)
    api.set_scene(None)
    tiles = {m: torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for m in MODES}
    rates = {m: [] for m in MODES}
    rays = {}
    for r in range(runs):
        for m, fn in MODES.items():
            n, dt = measure(fn, w, h, warmup, frames, tiles[m])
            rays[m] = n
            rates[m].append(n / dt / 1e9)
            print(json.dumps(dict(config=name, mode=m, run=r, frames=frames, ms_per_frame=round(dt / frames * 1e3, 4),
                                  gray_s=round(n / dt / 1e9, 3))), flush=True)
    same = bool(torch.equal(tiles["a_update_draw"].view(torch.int32), tiles["b_animation"].view(torch.int32)))
    med = {m: statistics.median(v) for m, v in rates.items()}
    # trace launches of one call of 32 frames against 32 frames drawn one by one
    api.kernel_timing_begin(64)
    run_animation(w, h, range(warmup, warmup + PER_CALL), tiles["b_animation"])
    kb = api.kernel_timing_end()
    api.kernel_timing_begin(64)
    run_static_batch(w, h, range(warmup, warmup + PER_CALL), tiles["c_static_batch"])
    kc = api.kernel_timing_end()
    out = dict(config=name, w=w, h=h, spp=spp, frames=frames, runs=runs, median_gray_s={m: round(v, 3) for m, v in med.items()},
               all_gray_s={m: [round(x, 3) for x in v] for m, v in rates.items()},
               b_over_a=round(med["b_animation"] / med["a_update_draw"], 3), b_over_c=round(med["b_animation"] / med["c_static_batch"], 3),
               a_b_tiles_equal=same, a_b_rays_equal=rays["a_update_draw"] == rays["b_animation"],
               kernel_ms_per_32={"b_animation": round(kb[0], 3), "c_static_batch": round(kc[0], 3)},
               launches_per_32={"b_animation": kb[1], "c_static_batch": kc[1]}, pipeline=api.pipeline_info())
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=0, help="timed frames per measurement (0: 256 / 128)")
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    api.InitializeTest()
    try:
        if args.only in ("", "640x360"):
            size("640x360x4", 640, 360, 4, args.warmup, args.frames or 256, args.runs)
        if args.only in ("", "1280x720"):
            size("1280x720x4", 1280, 720, 4, args.warmup, args.frames or 128, args.runs)
    finally:
        api.ShutdownTest()


if __name__ == "__main__":
    main()
