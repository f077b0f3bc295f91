"""A 360-degree equirectangular image of the built-in scene: a camera the library does not have, through tptTraceRaysDevice.

    python examples/panorama.py [width height passes [out_dir]]

Every pixel is a direction -- longitude along x, latitude along y, row 0 at the bottom like the tile -- from one point above the
scene; the directions are made once with numpy, every pass gives each ray a seed of its own, the passes' radiance is accumulated with
torch on the device, and the mean goes through tptDisplayRGBA8 into panorama.tga.  There is no lens and no jitter here: a pixel's
passes differ by their random bounces only (add a sub-pixel offset to lon / lat per pass for anti-aliasing).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from toypathtracer_amd import api  # noqa: E402

EYE = (0.0, 1.0, 0.0)


def directions(w, h):
    """[h * w, 3] float32 unit vectors: pixel (x, y) looks at longitude 2 pi (x + 0.5) / w - pi, latitude pi (y + 0.5) / h - pi / 2"""
    lon = (np.arange(w, dtype=np.float64) + 0.5) / w * 2.0 * np.pi - np.pi
    lat = (np.arange(h, dtype=np.float64) + 0.5) / h * np.pi - np.pi / 2
    lon, lat = np.meshgrid(lon, lat)
    d = np.stack([np.cos(lat) * np.sin(lon), np.sin(lat), -np.cos(lat) * np.cos(lon)], axis=-1).reshape(-1, 3)
    d32 = d.astype(np.float32)
    # (float32 unit length to the last bit or two, as the tracer's own normalised rays are)
    return d32 / np.sqrt((d32.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(np.float32)


def main():
    args = sys.argv[1:]
    w = int(args[0]) if len(args) > 0 else 2048
    h = int(args[1]) if len(args) > 1 else 1024
    passes = int(args[2]) if len(args) > 2 else 32
    out_dir = args[3] if len(args) > 3 else "."
    n = w * h
    api.InitializeTest()
    try:
        api.UpdateTest(0.0, 0, w, h, 0)  # stages the scene (the camera it also builds plays no part)
        rays = np.zeros((n, 8), np.float32)
        rays[:, 0:3] = EYE
        rays[:, 4:7] = directions(w, h)
        d_rays = torch.from_numpy(rays).cuda()
        seeds = d_rays[:, 3].view(torch.int32)
        index = torch.arange(n, dtype=torch.int64, device="cuda")
        radiance = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        total = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        for p in range(passes):
            # one seed per ray and pass: a hash of (ray, pass), never 0
            s = ((index * 1973 + p * 26699 + 9277) * 2654435761) & 0x7FFFFFFF
            seeds.copy_((s | 1).to(torch.int32))
            torch.cuda.synchronize()  # (torch's stream and the library's are not the same one)
            api.trace_rays_device(n, d_rays.data_ptr(), radiance.data_ptr(), None, count.data_ptr())
            api.synchronize()
            total += radiance
        tile = (total / passes).view(h, w, 4).contiguous()
        rgba = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        api.display_rgba8(tile.data_ptr(), w, h, rgba.data_ptr())
        api.synchronize()
        api.write_tga(os.path.join(out_dir, "panorama.tga"), rgba.cpu().numpy())
        print("%dx%d equirectangular, %d passes, %d rays (%.2f per path) -> panorama.tga"
              % (w, h, passes, int(count.item()), float(total[:, 3].sum().item()) / (n * passes)))
    finally:
        api.ShutdownTest()


if __name__ == "__main__":
    main()
