"""The per-frame denoising chain with history rectification, on a short animated clip: every frame is traced with its planes
(tptDrawDeviceMoments), blended with its reprojected history (tptTemporalAccumulateDevice), rectified in place against this frame's
neighbourhood (tptRectifyHistoryDevice: the colour and moments outputs are the pass's own planes) and filtered
(tptDenoiseDeviceVariance).  The rectified colour and moments are the next frame's history.

    python examples/rectified_chain.py [width height frames [max_history [out_dir]]]

Writes rectified_0000.tga ... into out_dir and prints, per frame, how many pixels the clamp touched and the mean history length
before and after.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from toypathtracer_amd import api  # noqa: E402

SPP = 4
ANIMATE = 1


def main():
    args = sys.argv[1:]
    w = int(args[0]) if len(args) > 0 else 640
    h = int(args[1]) if len(args) > 1 else 360
    n = int(args[2]) if len(args) > 2 else 12
    max_history = float(args[3]) if len(args) > 3 else 16.0
    out_dir = args[4] if len(args) > 4 else "."
    api.InitializeTest()
    api.set_samples_per_pixel(SPP)
    plane = lambda: torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")  # noqa: E731
    # two sets of the planes a frame hands to the next one; everything else is reused
    sets = [dict(colour=plane(), albedo=plane(), moments=plane(), normal_depth=plane()) for _ in range(2)]
    tile, traced_albedo, traced_moments, variance, before, out = plane(), plane(), plane(), plane(), plane(), plane()
    prev = None
    for j in range(n):
        time = 0.05 * j
        cur = sets[j % 2]
        api.UpdateTest(time, j, w, h, ANIMATE)
        cam = api.GetSceneDesc()[2].copy()
        tile.zero_()
        traced_moments.zero_()
        torch.cuda.synchronize()
        api.draw_device_moments(time, j, w, h, tile.data_ptr(), traced_moments.data_ptr(), ANIMATE, albedo_ptr=traced_albedo.data_ptr(),
                                normal_depth_ptr=cur["normal_depth"].data_ptr())
        api.temporal_accumulate_device(w, h, cam, tile.data_ptr(), traced_albedo.data_ptr(), cur["normal_depth"].data_ptr(),
                                       traced_moments.data_ptr(), cur["colour"].data_ptr(), cur["albedo"].data_ptr(),
                                       cur["moments"].data_ptr(), variance.data_ptr(), prev=prev, max_history=max_history)
        api.synchronize()
        before.copy_(cur["moments"])  # (for the printed figures only)
        untouched = cur["colour"].clone()
        torch.cuda.synchronize()
        # in place: colour and moments are rectified where they lie, the variance plane is rewritten
        api.rectify_history_device(w, h, tile.data_ptr(), traced_moments.data_ptr(), cur["colour"].data_ptr(), cur["moments"].data_ptr(),
                                   cur["colour"].data_ptr(), cur["moments"].data_ptr(), variance.data_ptr())
        api.denoise_device_variance(w, h, cur["colour"].data_ptr(), variance.data_ptr(), float(SPP), out.data_ptr(),
                                    albedo_ptr=cur["albedo"].data_ptr(), normal_depth_ptr=cur["normal_depth"].data_ptr())
        api.synchronize()
        clamped = float((untouched != cur["colour"]).any(dim=-1).float().mean())
        print("frame %2d: %5.1f%% of the pixels clamped, mean history %.2f -> %.2f"
              % (j, 100.0 * clamped, float(before[..., 3].mean()), float(cur["moments"][..., 3].mean())))
        rgba = out.cpu().numpy().copy()
        rgba[..., :3] = np.clip(rgba[..., :3], 0.0, 1.0) ** (1.0 / 2.2)
        rgba[..., 3] = 1.0
        # (row 0 of a plane is the bottom row; write_tga takes the top row first)
        api.write_tga(os.path.join(out_dir, "rectified_%04d.tga" % j), (rgba[::-1] * 255.0 + 0.5).astype(np.uint8))
        prev = (cam, cur["colour"].data_ptr(), cur["albedo"].data_ptr(), cur["normal_depth"].data_ptr(), cur["moments"].data_ptr())
    print("%dx%d, %d frames at %d spp, max_history %g, rectified at %r -> rectified_0000.tga .. in %s"
          % (w, h, n, SPP, max_history, api.RECTIFY_DEFAULTS, out_dir))
    api.ShutdownTest()


if __name__ == "__main__":
    main()
