"""A 180-degree equidistant fisheye image of the built-in scene through tptDrawDeviceLens.

    python examples/fisheye.py [size samples [max_angle_degrees [out_dir]]]

The angle from the viewing direction grows linearly with the distance from the image centre and reaches max_angle where the image
circle touches the edges of the square image (api.lens_fisheye: sx = sy = 2); the corners look further out.  One call traces all
samples of every pixel; the image goes through tptDisplayRGBA8 into fisheye.tga.
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from toypathtracer_amd import api  # noqa: E402


def main():
    args = sys.argv[1:]
    size = int(args[0]) if len(args) > 0 else 1024
    samples = int(args[1]) if len(args) > 1 else 16
    max_angle = math.radians(float(args[2])) if len(args) > 2 else math.pi / 2
    out_dir = args[3] if len(args) > 3 else "."
    api.InitializeTest()
    try:
        api.set_samples_per_pixel(samples)
        api.UpdateTest(0.0, 0, size, size, 0)  # stages the scene
        lens = api.lens_fisheye(origin=(0.0, 2.0, 3.0), forward=(0.0, -0.4, -1.0), up=(0.0, 1.0, 0.0), max_angle=max_angle)
        tile = torch.zeros((size, size, 4), dtype=torch.float32, device="cuda")
        rgba = torch.zeros((size, size, 4), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # (torch's stream and the library's are not the same one)
        api.draw_device_lens(0, size, size, tile.data_ptr(), lens)
        api.display_rgba8(tile.data_ptr(), size, size, rgba.data_ptr())
        api.synchronize()
        api.write_tga(os.path.join(out_dir, "fisheye.tga"), rgba.cpu().numpy())
        print("%dx%d fisheye, %.0f degrees at the circle, %d samples -> fisheye.tga" % (size, size, math.degrees(max_angle), samples))
    finally:
        api.ShutdownTest()


if __name__ == "__main__":
    main()
