"""A progressive still, denoised: the frames are accumulated 32 per launch with the planes the variance-guided filter reads
(tptDrawDeviceBatchMoments: the tile, the luminance moments, and the albedo and normal / depth planes averaged over the frames as the
tile is), then filtered once (tptDenoiseDeviceVariance).  The still is built in a few calls that continue one another, as a viewer that
shows a preview between them would.

    python examples/progressive_denoise.py [width height frames [calls [out_dir]]]

Writes progressive_raw.tga and progressive_denoised.tga into out_dir and prints the rate of the accumulation.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from toypathtracer_amd import api  # noqa: E402

SPP = 4
PROGRESSIVE = api.kFlagProgressive


def write(path, plane):
    rgba = plane.cpu().numpy().copy()
    rgba[..., :3] = np.clip(rgba[..., :3], 0.0, 1.0) ** (1.0 / 2.2)
    rgba[..., 3] = 1.0
    # (row 0 of a plane is the bottom row; write_tga takes the top row first)
    api.write_tga(path, (rgba[::-1] * 255.0 + 0.5).astype(np.uint8))


def main():
    args = sys.argv[1:]
    w = int(args[0]) if len(args) > 0 else 1280
    h = int(args[1]) if len(args) > 1 else 720
    frames = int(args[2]) if len(args) > 2 else 64
    calls = int(args[3]) if len(args) > 3 else 2
    out_dir = args[4] if len(args) > 4 else "."
    api.InitializeTest()
    api.set_samples_per_pixel(SPP)
    # the four running means, zeroed once, and the filter's output
    tile, moments, albedo, normal_depth, out = (torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(5))
    torch.cuda.synchronize()
    api.UpdateTest(0.0, 0, w, h, PROGRESSIVE)
    rays0 = api.ray_counter_read()
    t0 = time.perf_counter()
    first = 0
    for c in range(calls):
        n = (frames - first + (calls - c) - 1) // (calls - c)
        if n < 1:
            continue
        api.draw_device_batch_moments(0.0, first, n, w, h, tile.data_ptr(), moments.data_ptr(), PROGRESSIVE, albedo_ptr=albedo.data_ptr(),
                                      normal_depth_ptr=normal_depth.data_ptr())
        first += n
    api.synchronize()
    dt = time.perf_counter() - t0
    rays = api.ray_counter_read() - rays0
    # the colour and the moments average spp * frames samples; so do the guides
    samples = api.moment_samples(SPP, frames - 1, PROGRESSIVE)
    api.denoise_device_variance(w, h, tile.data_ptr(), moments.data_ptr(), samples, out.data_ptr(), albedo_ptr=albedo.data_ptr(),
                                normal_depth_ptr=normal_depth.data_ptr())
    api.synchronize()
    write(os.path.join(out_dir, "progressive_raw.tga"), tile)
    write(os.path.join(out_dir, "progressive_denoised.tga"), out)
    print("%dx%d, %d frames at %d spp in %d calls: %.1f ms, %.1f Gray/s; %g samples per pixel behind the filter -> progressive_raw.tga, "
          "progressive_denoised.tga in %s" % (w, h, frames, SPP, calls, dt * 1e3, rays / dt / 1e9, samples, out_dir))
    api.ShutdownTest()


if __name__ == "__main__":
    main()
