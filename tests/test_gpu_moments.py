"""tptDrawDeviceMoments on the GPU: the tile and ray count of tptDrawDevice, the planes of tptDrawDeviceAov, and the luminance moments
of the samples held byte for byte against the CPU reference (tests/moments_checker.c) -- a single frame, a progressive sequence (the
blend), an animated frame, a scene of 4096 spheres -- and a streaming caller that mixes it with plain draws and variance denoises."""
import ctypes as C

import numpy as np
import pytest

from moments_lib import MomentsChecker, VarianceChecker
from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return MomentsChecker(tmp_path_factory.mktemp("moments_checker"))


def plane(h, w, fill=0.0):
    import torch
    return torch.full((h, w, 4), fill, dtype=torch.float32, device="cuda")


def draw_moments(tpt, w, h, frames, flags=FLAG_PROGRESSIVE, time=0.0, albedo=True, normal_depth=True):
    """frames drawn through tptDrawDeviceMoments on one tile and one moments plane (both zeroed first) -> (tile, moments, albedo or None,
    normalDepth or None, per-frame rays); the planes are the last frame's"""
    import torch
    tile, mo = plane(h, w), plane(h, w)
    alb, nd = plane(h, w, float("nan")), plane(h, w, float("nan"))
    torch.cuda.synchronize()
    per = []
    for f in frames:
        tpt.UpdateTest(time, f, w, h, flags)
        r0 = tpt.ray_counter_read()
        tpt.draw_device_moments(time, f, w, h, tile.data_ptr(), mo.data_ptr(), flags, albedo_ptr=alb.data_ptr() if albedo else None,
                                normal_depth_ptr=nd.data_ptr() if normal_depth else None)
        per.append(tpt.ray_counter_read() - r0)
    tpt.synchronize()
    return (tile.cpu().numpy(), mo.cpu().numpy(), alb.cpu().numpy() if albedo else None, nd.cpu().numpy() if normal_depth else None, per)


def draw_plain(tpt, w, h, frames, flags=FLAG_PROGRESSIVE, time=0.0):
    import torch
    tile = plane(h, w)
    torch.cuda.synchronize()
    per = []
    for f in frames:
        tpt.UpdateTest(time, f, w, h, flags)
        r0 = tpt.ray_counter_read()
        tpt.draw_device(time, f, w, h, tile.data_ptr(), flags)
        per.append(tpt.ray_counter_read() - r0)
    tpt.synchronize()
    return tile.cpu().numpy(), per


def draw_aov(tpt, w, h, f, flags=FLAG_PROGRESSIVE, time=0.0):
    import torch
    tile, alb, nd = plane(h, w), plane(h, w, float("nan")), plane(h, w, float("nan"))
    torch.cuda.synchronize()
    tpt.UpdateTest(time, f, w, h, flags)
    tpt.draw_device_aov(time, f, w, h, tile.data_ptr(), flags, albedo_ptr=alb.data_ptr(), normal_depth_ptr=nd.data_ptr())
    tpt.synchronize()
    return alb.cpu().numpy(), nd.cpu().numpy()


def check(checker, oracle, got, w, h, spp, nframes, **kw):
    tile, mo, alb, nd, per = got
    pero, bo, mo_want, ao, no = checker.frames(oracle, w, h, spp, nframes, **kw)
    assert per == pero
    assert tile.tobytes() == bo.tobytes(), "the tile differs from the checker"
    assert mo.tobytes() == mo_want.tobytes(), "the moments differ from the checker"
    if alb is not None:
        assert alb.tobytes() == ao.tobytes(), "the albedo plane differs from the checker"
    if nd is not None:
        assert nd.tobytes() == no.tobytes(), "the normal / depth plane differs from the checker"
    return mo_want


def test_single_frame_640x360_equals_the_checker(tpt_defaults, checker, oracle):
    tpt = tpt_defaults
    w, h = 640, 360
    mo = check(checker, oracle, draw_moments(tpt, w, h, [0]), w, h, 4, 1)
    assert (mo[..., 1] > mo[..., 0] * mo[..., 0]).any() and (mo[..., 2] == 0).all() and (mo[..., 3] == 0).all()
    assert tpt.launch_info()["blocks_per_cu"] == 2  # (the moments kernel has its single-frame twin's LDS)


@pytest.mark.parametrize("frames", [3, 5])
def test_progressive_sequence_blends_like_the_tile(tpt_defaults, checker, oracle, frames):
    tpt = tpt_defaults
    w, h = 200, 120
    check(checker, oracle, draw_moments(tpt, w, h, list(range(frames))), w, h, 4, frames)


def test_animated_frame(tpt_defaults, checker, oracle):
    tpt = tpt_defaults
    w, h = 160, 96
    flags = FLAG_PROGRESSIVE | FLAG_ANIMATE
    check(checker, oracle, draw_moments(tpt, w, h, [0, 1, 2], flags=flags, time=1.7), w, h, 4, 3, flags=flags, time=1.7)


@pytest.mark.parametrize("albedo,normal_depth", [(False, False), (True, False), (False, True)], ids=["none", "albedo", "normal_depth"])
def test_optional_planes(tpt_defaults, checker, oracle, albedo, normal_depth):
    tpt = tpt_defaults
    w, h = 96, 64
    tpt.set_samples_per_pixel(7)
    check(checker, oracle, draw_moments(tpt, w, h, [0, 1], albedo=albedo, normal_depth=normal_depth), w, h, 7, 2)


SCENES = ["default", "stress", "cloud"]


def set_scene(tpt, oracle, scene, w, h):
    """-> (spheres, mats, oracle camera) or (None, None, None) for the default scene"""
    from toypathtracer_amd.scenes import CLOUD_CAMERA_OUTSIDE, cloud_scene, stress_scene
    if scene == "default":
        return None, None, None
    if scene == "stress":
        s, m = stress_scene(4096, 64)
        cam = dict(look_from=(0.0, 6.0, 20.0), look_at=(0.0, 0.0, 0.0), vfov=60.0, aperture=0.02, focus_dist=20.0)
    else:
        s, m = cloud_scene(300, 12.0, 7)
        cam = CLOUD_CAMERA_OUTSIDE
    tpt.set_scene(s, m)
    tpt.set_camera(**cam)
    ocam = oracle.camera(cam["look_from"], cam["look_at"], (0, 1, 0), cam["vfov"], w / h, cam["aperture"], cam["focus_dist"])
    return s, m, ocam


@pytest.mark.parametrize("scene", SCENES)
def test_tile_and_planes_are_the_existing_calls(tpt_defaults, checker, oracle, scene):
    """tile and rays byte-identical to tptDrawDevice's, planes to tptDrawDeviceAov's, moments to the checker's; frames 0-1"""
    tpt = tpt_defaults
    w, h = 128, 72
    s, m, cam = set_scene(tpt, oracle, scene, w, h)
    got = draw_moments(tpt, w, h, [0, 1])
    tile, per = draw_plain(tpt, w, h, [0, 1])
    alb, nd = draw_aov(tpt, w, h, 1)
    assert got[0].tobytes() == tile.tobytes() and got[4] == per
    assert got[2].tobytes() == alb.tobytes() and got[3].tobytes() == nd.tobytes()
    if scene == "stress":
        assert tpt.scene_info()["groups"] > 0  # (the grouped instantiation, tptTraceMomentsKernel<false>)
    kw = {} if s is None else dict(spheres=s, mats=m, cam=cam)
    check(checker, oracle, got, w, h, 4, 2, **kw)


def test_refusals_write_nothing(tpt_defaults):
    import torch
    tpt = tpt_defaults
    lib = tpt.load_library()
    w, h = 32, 16
    tile, mo, alb, nd = plane(h, w, 7.25), plane(h, w, -1.5), plane(h, w, 3.0), plane(h, w, 11.0)
    tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
    torch.cuda.synchronize()
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def refused(what, t=tile, a=alb, n=nd, m=mo, ww=w):
        rc = lib.tptDrawDeviceMoments(C.c_float(0.0), 0, ww, h, P(t), P(a), P(n), m if isinstance(m, C.c_void_p) else P(m), 2)
        msg = lib.tptGetLastError().decode()
        assert rc != 0 and "tptDrawDeviceMoments" in msg, (what, rc, msg)

    refused("moments NULL", m=None)
    refused("tile NULL", t=None)
    refused("moments is the tile", m=tile)
    refused("moments overlaps the albedo", m=C.c_void_p(alb.data_ptr() + 16 * 7))
    refused("moments is the normal / depth plane", m=nd)
    refused("no tptUpdate at this size", ww=w + 1)
    tpt.set_seed_mode(0)
    refused("row-serial seeds")
    tpt.set_seed_mode(1)
    tpt.synchronize()
    torch.cuda.synchronize()
    assert bool((tile == 7.25).all() and (mo == -1.5).all() and (alb == 3.0).all() and (nd == 11.0).all()), "a refused call wrote"


def test_streaming_caller_loses_nothing(tpt_defaults, checker, oracle, tmp_path):
    """12 frames at 320x180x4 on one stream: plain tptDrawDevice frames interleaved with moments draws and variance denoises of the
    tile after each moments draw.  The tile and the rays are those of 12 plain frames; each moments draw's moments, and each denoised
    output, are the checkers' for the tile and moments as they stood"""
    import torch
    from toypathtracer_amd.api import DENOISE_VARIANCE_DEFAULTS as D
    tpt = tpt_defaults
    w, h, n = 320, 180, 12
    kinds = ["plain", "moments", "moments", "plain", "moments", "plain", "plain", "moments", "moments", "moments", "plain", "moments"]
    stream = torch.cuda.Stream()

    def run(mixed):
        tile, mo = plane(h, w), plane(h, w)
        alb, nd = plane(h, w), plane(h, w)
        outs, snaps = [], []
        stream.wait_stream(torch.cuda.current_stream())
        torch.cuda.synchronize()
        tpt.set_stream(stream.cuda_stream)
        tiles = []
        try:
            r0 = tpt.ray_counter_read()
            tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
            with torch.cuda.stream(stream):
                for f in range(n):
                    if mixed and kinds[f] == "moments":
                        tpt.draw_device_moments(0.0, f, w, h, tile.data_ptr(), mo.data_ptr(), FLAG_PROGRESSIVE, albedo_ptr=alb.data_ptr(),
                                                normal_depth_ptr=nd.data_ptr())
                        out = plane(h, w, float("nan"))
                        # (samples = 4 whatever the frame: this test holds the bytes against the checker, which takes the same value,
                        #  not the quality; a progressive caller would pass moment_samples and average its guides)
                        tpt.denoise_device_variance(w, h, tile.data_ptr(), mo.data_ptr(), 4.0, out.data_ptr(), albedo_ptr=alb.data_ptr(),
                                                    normal_depth_ptr=nd.data_ptr(), iterations=3)
                        outs.append(out)
                        snaps.append((tile.clone(), mo.clone(), alb.clone(), nd.clone()))
                    else:
                        tpt.draw_device(0.0, f, w, h, tile.data_ptr(), FLAG_PROGRESSIVE)
                    tiles.append(tile.clone())
            stream.synchronize()
            rays = tpt.ray_counter_read() - r0
        finally:
            tpt.set_stream(None)
        return [t.cpu().numpy() for t in tiles], rays, [o.cpu().numpy() for o in outs], [[x.cpu().numpy() for x in s] for s in snaps]

    plain = run(False)
    mixed = run(True)
    assert [t.tobytes() for t in mixed[0]] == [t.tobytes() for t in plain[0]], "a tile changed"
    assert mixed[1] == plain[1]
    vc = VarianceChecker(tmp_path)
    s, m = oracle.default_scene()
    cam = oracle.default_camera(w, h)
    for k, f in enumerate([f for f in range(n) if kinds[f] == "moments"]):
        t, mo, alb, nd = mixed[3][k]
        # the moments of frame f blended into the moments plane as it stood after the previous moments draw (the plain draws do not
        # touch it): the checker's blend of frame f alone into that plane
        prev = mixed[3][k - 1][1].copy() if k else np.zeros((h, w, 4), np.float32)
        _, _, want_mo, want_a, want_n = checker.render(s, m, cam, w, h, 4, f, FLAG_PROGRESSIVE, backbuffer=np.zeros((h, w, 4), np.float32),
                                                       moments=prev)
        assert mo.tobytes() == want_mo.tobytes() and alb.tobytes() == want_a.tobytes() and nd.tobytes() == want_n.tobytes(), f
        want = vc.run(t, alb, nd, mo, 4.0, iterations=3, sigma_luminance=D["sigma_luminance"], sigma_normal=D["sigma_normal"],
                      sigma_depth=D["sigma_depth"], flags=1)
        assert mixed[2][k].tobytes() == want.tobytes(), f
