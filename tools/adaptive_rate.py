"""The cost and the use of tptDrawDeviceAdaptive and tptAdaptiveSamplesDevice, each interleaved with the call it is compared with.
(1) constant: synchronous draws at 1280x720 (the caller waits for every frame), a plane of constant counts 4 against
tptDrawDeviceMoments at 4 spp, --frames frames per run, --reps alternating runs, Gray/s median and range, and whether both left the same
tile bytes.  With --moments-only the moments runs alone (the same caller on another build of the library, TPT_LIB).
(2) skewed: one launch on a planned plane of the default scene (base pass at 4 spp, then tptAdaptiveSamplesDevice) and on a synthetic
plane (10 % of the pixels at 64, the rest at 1), against a uniform tptDrawDeviceMoments launch of the same total samples (rounded to whole
spp), Gray/s each; and the launch time against a launch whose only work is one 64-sample pixel: the sequential floor.
(3) quality at 640x360 on the default scene, at equal samples: k frames of 4 spp against a base pass of 4 spp plus one planned pass whose
targetError is bisected until tptAdaptiveSamplesDevice's total matches (k - 1) * 4 samples per pixel within 2 %; mean squared error
against a 4096-sample render, raw and through tptDenoiseDeviceVariance (guides averaged over the samples in both arms).
(4) helpers: tptAdaptiveSamplesDevice at 1280x720 between timer brackets, with and without its optional outputs; the weighted blend's
time comes from a kernel trace of this part (rocprofv3 --kernel-trace --stats -- python3 tools/adaptive_rate.py --only helpers).
One JSON line per measurement.
    python3 tools/adaptive_rate.py [--frames F] [--reps R] [--calls N] [--k K] [--only constant|skewed|quality|helpers] [--moments-only]"""
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

FLAGS = 2  # kFlagProgressive


def zeros(h, w):
    return torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")


def rng_ms(v):
    return [round(min(v), 3), round(max(v), 3)]


class Caller:
    """one tile, moments plane and pair of guide planes; each run is `frames` synchronous draws from zeroed planes"""

    def __init__(self, w, h):
        self.w, self.h = w, h
        self.tile, self.mo, self.alb, self.nd = (zeros(h, w) for _ in range(4))

    def run(self, frames, counts=None, spp=4, frame0=0, keep=False):
        """-> (Gray/s, seconds per frame, rays, tile bytes)"""
        w, h = self.w, self.h
        if not keep:
            self.tile.zero_()
            self.mo.zero_()
        if counts is None:
            api.set_samples_per_pixel(spp)
        torch.cuda.synchronize()
        api.UpdateTest(0.0, frame0, w, h, FLAGS)
        api.synchronize()
        r0 = api.ray_counter_read()
        t0 = time.perf_counter()
        for f in range(frame0, frame0 + frames):
            if counts is None:
                api.draw_device_moments(0.0, f, w, h, self.tile.data_ptr(), self.mo.data_ptr(), FLAGS, albedo_ptr=self.alb.data_ptr(),
                                        normal_depth_ptr=self.nd.data_ptr())
            else:
                api.draw_device_adaptive(0.0, f, w, h, self.tile.data_ptr(), self.mo.data_ptr(), counts.data_ptr(), FLAGS,
                                         albedo_ptr=self.alb.data_ptr(), normal_depth_ptr=self.nd.data_ptr())
            api.synchronize()
        dt = time.perf_counter() - t0
        rays = api.ray_counter_read() - r0
        api.set_samples_per_pixel(4)
        return rays / dt / 1e9, dt / frames, rays, self.tile.cpu().numpy().tobytes()


def constant(frames, reps, moments_only):
    w, h = 1280, 720
    c = Caller(w, h)
    counts = torch.full((h, w), 4, dtype=torch.int32, device="cuda")
    kinds = ["moments"] if moments_only else ["moments", "adaptive"]
    run = {"moments": lambda: c.run(frames), "adaptive": lambda: c.run(frames, counts)}
    for k in kinds:
        run[k]()  # (warm-up)
    g = {k: [] for k in kinds}
    tiles = {}
    for _ in range(reps):
        for k in kinds:
            r = run[k]()
            g[k].append(r[0])
            tiles[k] = r[3]
    out = dict(measure="sync_draws_1280x720_counts4", frames=frames, library=os.environ.get("TPT_LIB", "built"))
    for k in kinds:
        out["gray_s_" + k] = round(statistics.median(g[k]), 3)
        out["range_" + k] = rng_ms(g[k])
    if not moments_only:
        out["ratio"] = round(out["gray_s_adaptive"] / out["gray_s_moments"], 4)
        out["same_tile"] = tiles["adaptive"] == tiles["moments"]
    print(json.dumps(out), flush=True)


def planned_counts(c, te, lo, hi):
    """a base pass at 4 spp (frame 0) into c's planes, then the plan -> (counts, total)"""
    w, h = c.w, c.h
    base = torch.full((h, w), 4, dtype=torch.int32, device="cuda")
    counts = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    c.run(1, base)
    api.adaptive_samples_device(w, h, c.mo.data_ptr(), te, counts.data_ptr(), min_samples=lo, max_samples=hi, total_ptr=total.data_ptr())
    api.synchronize()
    return counts, int(total.cpu()[0])


def skewed(reps):
    w, h = 1280, 720
    c = Caller(w, h)
    planes = {}
    planes["planned"], _ = planned_counts(c, 0.05, 0, 64)
    g = torch.Generator(device="cuda").manual_seed(64)
    planes["synthetic"] = torch.where(torch.rand((h, w), device="cuda", generator=g) < 0.1, 64, 1).to(torch.int32).contiguous()
    one = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    one[h // 2, w // 2] = 64
    for name, counts in planes.items():
        total = int(counts.clamp(0, 2047).sum().cpu())
        spp = max(1, round(total / (w * h)))
        c.run(1, counts, frame0=1)
        c.run(1, spp=spp, frame0=1)
        c.run(1, one, frame0=1)  # (warm-up)
        a, u, f = [], [], []
        for _ in range(reps):
            a.append(c.run(1, counts, frame0=1))
            u.append(c.run(1, spp=spp, frame0=1))
            f.append(c.run(1, one, frame0=1))
        hist = {int(v): int(n) for v, n in zip(*[t.cpu().tolist() for t in torch.unique(counts, return_counts=True)])}
        print(json.dumps(dict(measure="skewed_1280x720_" + name, total_samples=total, mean_samples=round(total / (w * h), 3),
                              zero_pixels=hist.get(0, 0), max_count_pixels=hist.get(64, 0), uniform_spp=spp,
                              gray_s_adaptive=round(statistics.median(r[0] for r in a), 3), range_adaptive=rng_ms([r[0] for r in a]),
                              gray_s_uniform=round(statistics.median(r[0] for r in u), 3), range_uniform=rng_ms([r[0] for r in u]),
                              rays_adaptive=a[0][2], rays_uniform=u[0][2],
                              ms_adaptive=round(statistics.median(r[1] for r in a) * 1e3, 3),
                              ms_uniform=round(statistics.median(r[1] for r in u) * 1e3, 3),
                              ms_one_64_sample_pixel=round(statistics.median(r[1] for r in f) * 1e3, 3))), flush=True)


def quality(k):
    w, h = 640, 360
    api.set_samples_per_pixel(1024)
    ref = zeros(h, w)
    torch.cuda.synchronize()
    for f in range(4):
        api.UpdateTest(0.0, f, w, h, FLAGS)
        api.draw_device(0.0, f, w, h, ref.data_ptr(), FLAGS)  # (frames 0..3 blended: the mean of 4096 samples)
    api.synchronize()
    api.set_samples_per_pixel(4)
    r = ref[..., :3].double()
    out = zeros(h, w)

    def mse(img):
        api.synchronize()
        return float(((img[..., :3].double() - r) ** 2).mean())

    # ---- uniform: k frames of 4 spp, the guides averaged over the frames like the tile
    c = Caller(w, h)
    alb_avg, nd_avg = zeros(h, w), zeros(h, w)
    c.tile.zero_()
    c.mo.zero_()
    torch.cuda.synchronize()
    r0 = api.ray_counter_read()
    for f in range(k):
        api.UpdateTest(0.0, f, w, h, FLAGS)
        api.draw_device_moments(0.0, f, w, h, c.tile.data_ptr(), c.mo.data_ptr(), FLAGS, albedo_ptr=c.alb.data_ptr(), normal_depth_ptr=c.nd.data_ptr())
        lerp = f / (f + 1.0)
        for avg, p in ((alb_avg, c.alb), (nd_avg, c.nd)):
            avg.mul_(lerp).add_(p * (1.0 - lerp))
    api.synchronize()
    rays_u = api.ray_counter_read() - r0
    raw_u = mse(c.tile)
    api.denoise_device_variance(w, h, c.tile.data_ptr(), c.mo.data_ptr(), api.moment_samples(4, k - 1, FLAGS), out.data_ptr(),
                                albedo_ptr=alb_avg.data_ptr(), normal_depth_ptr=nd_avg.data_ptr())
    den_u = mse(out)
    # ---- adaptive: a base pass of 4 spp, then one planned pass of the same budget (targetError bisected on the plan's total)
    budget = (k - 1) * 4 * w * h
    hi_count = 64
    lo_te, hi_te = 1e-3, 10.0
    r0 = api.ray_counter_read()
    counts, total = planned_counts(c, hi_te, 0, hi_count)
    alb0, nd0 = c.alb.clone(), c.nd.clone()
    te = hi_te
    tot = torch.zeros(1, dtype=torch.int64, device="cuda")
    for _ in range(40):
        te = (lo_te * hi_te) ** 0.5
        api.adaptive_samples_device(w, h, c.mo.data_ptr(), te, counts.data_ptr(), min_samples=0, max_samples=hi_count, total_ptr=tot.data_ptr())
        api.synchronize()
        total = int(tot.cpu()[0])
        if abs(total - budget) <= 0.02 * budget:
            break
        if total > budget:
            lo_te = te
        else:
            hi_te = te
    c.run(1, counts, frame0=1, keep=True)
    rays_a = api.ray_counter_read() - r0
    n = counts.clamp(0, 2047).float()[..., None]
    alb_a = torch.where(n > 0, (alb0 * 4 + c.alb * n) / (4 + n), alb0).contiguous()
    nd_a = torch.where(n > 0, (nd0 * 4 + c.nd * n) / (4 + n), nd0).contiguous()
    raw_a = mse(c.tile)
    var = zeros(h, w)
    scratch = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    api.adaptive_samples_device(w, h, c.mo.data_ptr(), te, scratch.data_ptr(), min_samples=0, max_samples=hi_count, out_variance_ptr=var.data_ptr())
    api.denoise_device_variance(w, h, c.tile.data_ptr(), var.data_ptr(), 1.0, out.data_ptr(), albedo_ptr=alb_a.data_ptr(),
                                normal_depth_ptr=nd_a.data_ptr())
    den_a = mse(out)
    hist = torch.bincount(counts.flatten().clamp(0, hi_count), minlength=hi_count + 1).cpu().tolist()
    print(json.dumps(dict(quality="equal_samples_640x360", k=k, samples_uniform=4 * k * w * h, samples_adaptive=4 * w * h + total,
                          budget_match=round(total / budget, 4), target_error=te, max_samples=hi_count, rays_uniform=rays_u,
                          rays_adaptive=rays_a, zero_pixels=hist[0], capped_pixels=hist[hi_count], mse_raw_uniform=raw_u,
                          mse_raw_adaptive=raw_a, raw_ratio=round(raw_a / raw_u, 4), mse_denoised_uniform=den_u,
                          mse_denoised_adaptive=den_a, denoised_ratio=round(den_a / den_u, 4))), flush=True)


def helpers(calls, reps):
    w, h = 1280, 720
    c = Caller(w, h)
    counts, _ = planned_counts(c, 0.05, 0, 64)
    var = zeros(h, w)
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    forms = {
        "counts_only": lambda: api.adaptive_samples_device(w, h, c.mo.data_ptr(), 0.05, counts.data_ptr()),
        "all_outputs": lambda: api.adaptive_samples_device(w, h, c.mo.data_ptr(), 0.05, counts.data_ptr(), out_variance_ptr=var.data_ptr(),
                                                           total_ptr=total.data_ptr()),
    }
    for f in forms.values():
        f()
    api.synchronize()
    us = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            api.timer_begin()
            for _ in range(calls):
                f()
            us[k].append(api.timer_end() / calls * 1000)
    px = w * h
    print(json.dumps(dict(measure="plan_1280x720", us_counts_only=round(statistics.median(us["counts_only"]), 2),
                          us_all_outputs=round(statistics.median(us["all_outputs"]), 2), range_counts_only=rng_ms(us["counts_only"]),
                          range_all_outputs=rng_ms(us["all_outputs"]), bytes_counts_only=20 * px, bytes_all_outputs=36 * px,
                          gb_s_counts_only=round(20 * px / statistics.median(us["counts_only"]) / 1e3, 1),
                          gb_s_all_outputs=round(36 * px / statistics.median(us["all_outputs"]) / 1e3, 1))), flush=True)
    # a few adaptive draws at constant counts for a kernel trace of the weighted blend (100 B per traced pixel)
    four = torch.full((h, w), 4, dtype=torch.int32, device="cuda")
    c.run(8, four)
    print(json.dumps(dict(measure="resolve_1280x720", note="kernel time of tptAdaptiveResolveKernel from the kernel trace of this run",
                          bytes=100 * px)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--only", choices=["constant", "skewed", "quality", "helpers"])
    ap.add_argument("--moments-only", action="store_true")
    a = ap.parse_args()
    api.InitializeTest()
    try:
        print(json.dumps(dict(device=api.device_name())), flush=True)
        if a.only in (None, "constant"):
            constant(a.frames, a.reps, a.moments_only)
        if a.moments_only:
            return
        if a.only in (None, "skewed"):
            skewed(a.reps)
        if a.only in (None, "quality"):
            quality(a.k)
        if a.only in (None, "helpers"):
            helpers(a.calls, a.reps)
    finally:
        api.ShutdownTest()


if __name__ == "__main__":
    main()
