"""TEST INFRASTRUCTURE: what the host's plan does with the light list, on the host-emulation build (tests/test_lights_plan.py runs this
in a child process with TPT_LIB=tests/_build/libtpt_hostemu.so, as tests/hostemu_driver.py is run).  One section per call
(`counts`, `kinds`, `plan`, `fallbacks`); the last line printed is a JSON object of what was seen -- every image is held against the oracle here,
the numbers of the plan are asserted by the test."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from common import oracle_frames  # noqa: E402
from oracle_lib import FLAG_PROGRESSIVE, SEED_PER_PIXEL, Oracle  # noqa: E402
import lights_lib  # noqa: E402

assert "hostemu" in os.environ.get("TPT_LIB", ""), "this driver is for the host-emulation build only"
from toypathtracer_amd import api as tpt  # noqa: E402
from toypathtracer_amd.scenes import STRESS_CAMERA  # noqa: E402

o = Oracle.get()


def draw(s, m, w, h, spp, frames, variant=(0, 3, -1), camera=None):
    """-> dict: refused (the message) or rays per frame, whether image and rays equal the oracle's, whether the oracle's image is finite,
    and launch_info() of the last launch"""
    tpt.set_kernel_variant(*variant)
    tpt.set_samples_per_pixel(spp)
    tpt.set_scene(s, m)
    cam = None
    if camera:
        tpt.set_camera(**camera)
        cam = o.camera(camera["look_from"], camera["look_at"], (0, 1, 0), camera["vfov"], w / h, camera["aperture"], camera["focus_dist"])
    bb = np.zeros((h, w, 4), np.float32)
    per = []
    try:
        for f in range(frames):
            tpt.UpdateTest(0.0, f, w, h, FLAG_PROGRESSIVE)
            per.append(tpt.DrawTest(0.0, f, w, h, bb, FLAG_PROGRESSIVE))
    except tpt.TptError as e:
        return dict(refused=str(e), untouched=not bb.any())
    finally:
        if camera:
            tpt.set_camera()
    info = tpt.launch_info()
    _, want, per_o = oracle_frames(o, w, h, spp, frames, spheres=s, mats=m, cam=cam, seed_mode=SEED_PER_PIXEL)
    return dict(refused=None, rays=per, rays_equal=per == per_o, image_equal=bb.tobytes() == want.tobytes(), finite=bool(np.isfinite(want).all()),
                lit=bool(want[..., :3].any()), **info)


def main(section):
    tpt.InitializeTest()
    tpt.set_seed_mode(SEED_PER_PIXEL)
    out = {}
    if section == "counts":
        for k in (0, 1, 15, 16, 46):
            s, m = lights_lib.default_with_lights(k, seed=k + 1)
            out["%d" % k] = draw(s, m, 64, 32, 2, 2)
            if k in (15, 16):
                out["%d lane-refill" % k] = draw(s, m, 64, 32, 2, 2, (0, 1, -1))
        # the scene forced into LDS beside 16 lights, right after launches 32 bytes smaller: one workgroup per CU, not the neighbour's two
        out["16 lds_scene 1"] = draw(*lights_lib.default_with_lights(16, seed=17), 64, 32, 2, 2, (0, 3, 1))
    elif section == "kinds":
        for name in lights_lib.LIGHT_KINDS:
            s, m = lights_lib.light_kind(name)
            for key, variant in (("", (0, 3, -1)), (" lane-refill", (0, 1, -1))):
                out[name + key] = dict(draw(s, m, 64, 32, 2, 2, variant), div_safe=lights_lib.r2_div_safe(s, m))
    elif section == "plan":
        for k in (2864, 2865, 3072, 3073):
            s, m = lights_lib.stress_with_lights(4096, 64, k)
            out["%d" % k] = draw(s, m, 16, 8, 1, 1, camera=STRESS_CAMERA)
            out["%d lds_scene 0" % k] = dict(refused=draw(s, m, 16, 8, 1, 1, (0, 3, 0), camera=STRESS_CAMERA)["refused"]) if k in (2865, 3073) else None
        # the draw after a refusal: the built-in scene again, as if nothing had happened
        tpt.set_scene()
        s, m = o.default_scene()
        out["after"] = draw(s, m, 16, 8, 1, 1)
    elif section == "fallbacks":
        # 3072 lights: more than the path-queue kernel's LDS holds beside this scene.  The entry points with a frame-by-frame way take
        # it (a stream of tptDrawDevice calls, which would otherwise be batched from the third frame on; tptDrawDeviceAnimation); the one
        # without refuses with the count and its own limit.
        s, m = lights_lib.stress_with_lights(4096, 64, 3072)
        w, h, frames = 8, 8, 4
        cam = o.camera(STRESS_CAMERA["look_from"], STRESS_CAMERA["look_at"], (0, 1, 0), STRESS_CAMERA["vfov"], w / h, STRESS_CAMERA["aperture"], STRESS_CAMERA["focus_dist"])
        total, want, per_o = oracle_frames(o, w, h, 1, frames, spheres=s, mats=m, cam=cam, seed_mode=SEED_PER_PIXEL)
        tpt.set_kernel_variant(0, 3, -1)
        tpt.set_samples_per_pixel(1)
        tpt.set_scene(s, m)
        tpt.set_camera(**STRESS_CAMERA)
        tpt.set_stream_batching(1)
        tile = np.zeros((h, w, 4), np.float32)
        r0 = tpt.ray_counter_read()
        for f in range(frames):
            tpt.UpdateTest(0.0, f, w, h, FLAG_PROGRESSIVE)
            tpt.draw_device(0.0, f, w, h, tile.ctypes.data, FLAG_PROGRESSIVE)
        tpt.synchronize()
        out["stream"] = dict(image_equal=tile.tobytes() == want.tobytes(), rays_equal=tpt.ray_counter_read() - r0 == total, **tpt.launch_info())
        tile2, rays = np.zeros((h, w, 4), np.float32), np.zeros(frames, np.int64)
        tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
        tpt.draw_device_animation(np.zeros(frames, np.float32), 0, w, h, tile2.ctypes.data, FLAG_PROGRESSIVE, frame_rays_ptr=rays.ctypes.data)
        tpt.synchronize()
        out["animation"] = dict(image_equal=tile2.tobytes() == want.tobytes(), rays_equal=rays.tolist() == per_o, **tpt.launch_info())
        tile3 = np.zeros((h, w, 4), np.float32)
        try:
            tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
            tpt.draw_device_batch(0.0, 0, 2, w, h, tile3.ctypes.data, FLAG_PROGRESSIVE)
            tpt.synchronize()
            out["batch"] = dict(refused=None)
        except tpt.TptError as e:
            out["batch"] = dict(refused=str(e), untouched=not tile3.any())
        tpt.set_camera()
    else:
        raise KeyError(section)
    tpt.ShutdownTest()
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1])
