"""A 360-degree equirectangular image of the built-in scene through tptDrawDeviceLens.

    python examples/panorama.py [width height samples [frames [out_dir]]]

Longitude runs along x, latitude along y, row 0 at the bottom like the tile, from one point above the scene.  The lens is a record of
64 bytes (api.lens_equirect); the library makes the rays on the device, jitters every sample inside its pixel from the pixel's own
random stream -- so edges are anti-aliased -- traces all `samples` of a pixel in one launch and blends the frames progressively into
the tile, exactly as draw_device does for the camera.  The mean goes through tptDisplayRGBA8 into panorama.tga.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from toypathtracer_amd import api  # noqa: E402

EYE = (0.0, 1.0, 0.0)


def main():
    args = sys.argv[1:]
    w = int(args[0]) if len(args) > 0 else 2048
    h = int(args[1]) if len(args) > 1 else 1024
    samples = int(args[2]) if len(args) > 2 else 8
    frames = int(args[3]) if len(args) > 3 else 4
    out_dir = args[4] if len(args) > 4 else "."
    api.InitializeTest()
    try:
        api.set_samples_per_pixel(samples)
        api.UpdateTest(0.0, 0, w, h, 0)  # stages the scene (the camera it also builds plays no part)
        lens = api.lens_equirect(origin=EYE, forward=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0))
        tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        rgba = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # (torch's stream and the library's are not the same one)
        for f in range(frames):
            api.draw_device_lens(f, w, h, tile.data_ptr(), lens, api.FLAG_PROGRESSIVE, count.data_ptr())
        api.display_rgba8(tile.data_ptr(), w, h, rgba.data_ptr())
        api.synchronize()
        api.write_tga(os.path.join(out_dir, "panorama.tga"), rgba.cpu().numpy())
        rays = int(count.item())
        print("%dx%d equirectangular, %d frames of %d samples, %d rays (%.2f per path) -> panorama.tga"
              % (w, h, frames, samples, rays, rays / (w * h * samples * frames)))
    finally:
        api.ShutdownTest()


if __name__ == "__main__":
    main()
