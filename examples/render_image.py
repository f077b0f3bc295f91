"""Render the built-in scene on the GPU and write it as TGA (the reference's Cs/Program.cs:33-59 format) and PNG.

    python examples/render_image.py [--aov] [--denoise] [width height frames [out_dir]]

--aov: the last frame is drawn with tptDrawDeviceAov, and its first-hit planes are written too: albedo.png (the albedo) and
normal.png (0.5 + 0.5 n) -- the guide images a denoiser takes beside the colour.
--denoise: implies --aov, and also writes denoised.png: the final tile through tptDenoiseDevice, guided by those planes (api defaults).
"""
import os
import struct
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from toypathtracer_amd import api  # noqa: E402


def write_png(path, rgba):
    h, w = rgba.shape[:2]
    raw = b"".join(b"\x00" + rgba[y].tobytes() for y in range(h))

    def chunk(tag, data):
        c = struct.pack(">I", len(data)) + tag + data
        return c + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def to_rgba8(rgb):
    """[h, w, 3] floats in [0, 1] -> [h, w, 4] uint8, opaque"""
    h, w = rgb.shape[:2]
    out = np.full((h, w, 4), 255, np.uint8)
    out[..., :3] = np.clip(rgb * 255.0 + 0.5, 0, 255).astype(np.uint8)
    return out


def main():
    denoise = "--denoise" in sys.argv[1:]
    aov = denoise or "--aov" in sys.argv[1:]
    args = [a for a in sys.argv[1:] if a not in ("--aov", "--denoise")]
    w = int(args[0]) if len(args) > 0 else 1280
    h = int(args[1]) if len(args) > 1 else 720
    frames = int(args[2]) if len(args) > 2 else 64
    out_dir = args[3] if len(args) > 3 else "."
    api.InitializeTest()
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    rgba = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    albedo = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") if aov else None
    normal_depth = torch.zeros_like(albedo) if aov else None
    r0 = api.ray_counter_read()
    for f in range(frames):
        api.UpdateTest(0.0, f, w, h, api.kFlagProgressive)
        if aov and f == frames - 1:
            api.draw_device_aov(0.0, f, w, h, tile.data_ptr(), api.kFlagProgressive, albedo_ptr=albedo.data_ptr(),
                                normal_depth_ptr=normal_depth.data_ptr())
        else:
            api.draw_device(0.0, f, w, h, tile.data_ptr(), api.kFlagProgressive)
    api.display_rgba8(tile.data_ptr(), w, h, rgba.data_ptr())
    rays = api.ray_counter_read() - r0
    img = rgba.cpu().numpy()
    api.write_tga(os.path.join(out_dir, "output.tga"), img)
    write_png(os.path.join(out_dir, "output.png"), img)
    print("%dx%d, %d frames x 4 spp, %d rays -> output.tga / output.png" % (w, h, frames, rays))
    if aov:
        # (the planes of the last frame: means over its samples; a pixel no sample hit is 0 in both)
        write_png(os.path.join(out_dir, "albedo.png"), to_rgba8(albedo.cpu().numpy()[..., :3]))
        write_png(os.path.join(out_dir, "normal.png"), to_rgba8(0.5 + 0.5 * normal_depth.cpu().numpy()[..., :3]))
        print("first-hit planes of frame %d -> albedo.png / normal.png" % (frames - 1))
    if denoise:
        out = torch.empty_like(tile)
        api.denoise_device(w, h, tile.data_ptr(), out.data_ptr(), albedo_ptr=albedo.data_ptr(), normal_depth_ptr=normal_depth.data_ptr())
        api.display_rgba8(out.data_ptr(), w, h, rgba.data_ptr())
        write_png(os.path.join(out_dir, "denoised.png"), rgba.cpu().numpy())
        print("the tile through tptDenoiseDevice (%s) -> denoised.png" % ", ".join("%s %g" % kv for kv in api.DENOISE_DEFAULTS.items()))
    api.ShutdownTest()


if __name__ == "__main__":
    main()
