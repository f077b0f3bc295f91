"""tptDenoiseDevice on the GPU: the a-trous filter held byte for byte against its CPU statement (tests/denoise_checker.c) on real
tptDrawDeviceAov planes and on synthetic ones; its inputs left alone; refusals that write nothing; a streaming caller that denoises every
frame losing nothing; and a denoised 4-spp frame closer to a converged render than the raw one."""
import ctypes as C

import numpy as np
import pytest

from denoise_lib import DEMODULATE, DenoiseChecker, random_planes
from oracle_lib import FLAG_PROGRESSIVE

pytestmark = pytest.mark.gpu

# MSE(denoised 4 spp) / MSE(raw 4 spp) against 1024 spp at 640x360, default scene, api defaults: measured 0.5076 on one MI355X (DESIGN.md
# 3.6; the trace and the filter are bit-exact, so the figure is deterministic)
QUALITY_BOUND = 0.55


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return DenoiseChecker(tmp_path_factory.mktemp("denoise_checker"))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan_plane(h, w):
    import torch
    return torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda")


def aov_frame(tpt, w, h):
    """frame 0 through tptDrawDeviceAov -> (tile, albedo, normalDepth) as host arrays"""
    import torch
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    alb, nd = nan_plane(h, w), nan_plane(h, w)
    torch.cuda.synchronize()
    tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
    tpt.draw_device_aov(0.0, 0, w, h, tile.data_ptr(), FLAG_PROGRESSIVE, albedo_ptr=alb.data_ptr(), normal_depth_ptr=nd.data_ptr())
    tpt.synchronize()
    return tile.cpu().numpy(), alb.cpu().numpy(), nd.cpu().numpy()


def denoise_gpu(tpt, colour, albedo, nd, iterations, sc, sn, sd, demod):
    """tptDenoiseDevice on copies of the host planes -> (out, the inputs as they are after the call)"""
    h, w = colour.shape[:2]
    dc = dev(colour)
    da = None if albedo is None else dev(albedo)
    dn = None if nd is None else dev(nd)
    out = nan_plane(h, w)
    import torch
    torch.cuda.synchronize()
    tpt.denoise_device(w, h, dc.data_ptr(), out.data_ptr(), albedo_ptr=None if da is None else da.data_ptr(),
                       normal_depth_ptr=None if dn is None else dn.data_ptr(), iterations=iterations, sigma_colour=sc, sigma_normal=sn,
                       sigma_depth=sd, demodulate=demod)
    tpt.synchronize()
    return out.cpu().numpy(), [None if t is None else t.cpu().numpy() for t in (dc, da, dn)]


def same_bytes(got, want):
    return got.tobytes() == want.tobytes()


def check_all_modes(tpt, checker, colour, albedo, nd, iterations, same=same_bytes, sigmas=None):
    """every mode of the call against the checker, compared with `same` (byte equality unless the caller's reference holds NaNs, whose
    payload is not part of the contract); sigmas: (colour, normal, depth), None for the api's defaults"""
    from toypathtracer_amd.api import DENOISE_DEFAULTS as D
    sc, sn, sd = (D["sigma_colour"], D["sigma_normal"], D["sigma_depth"]) if sigmas is None else sigmas
    for use_alb, use_nd, demod in ((True, True, True), (True, True, False), (False, True, False), (True, False, True), (False, False, False)):
        a = albedo if use_alb else None
        n = nd if use_nd else None
        for it in iterations:
            got, ins = denoise_gpu(tpt, colour, a, n, it, sc, sn if use_nd else 0.0, sd if use_nd else 0.0, demod)
            want = checker.run(colour, a, n, it, sc, sn if use_nd else 0.0, sd if use_nd else 0.0, DEMODULATE if demod else 0)
            assert same(got, want), (use_alb, use_nd, demod, it)
            for x, y in zip(ins, (colour, a, n)):
                assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), "an input was written"


def test_real_planes_1280x720x4(tpt_defaults, checker):
    tpt = tpt_defaults
    colour, albedo, nd = aov_frame(tpt, 1280, 720)
    check_all_modes(tpt, checker, colour, albedo, nd, range(1, 6))


@pytest.mark.parametrize("scene", ["stress", "cloud"])
def test_real_planes_480x270_other_scenes(tpt_defaults, checker, scene):
    from toypathtracer_amd.scenes import CLOUD_CAMERA_OUTSIDE, cloud_scene, stress_scene
    tpt = tpt_defaults
    if scene == "stress":
        s, m = stress_scene(4096, 64)
        cam = dict(look_from=(0.0, 6.0, 20.0), look_at=(0.0, 0.0, 0.0), vfov=60.0, aperture=0.02, focus_dist=20.0)
    else:
        s, m = cloud_scene(3000, 12.0, 7)
        cam = CLOUD_CAMERA_OUTSIDE
    tpt.set_scene(s, m)
    tpt.set_camera(**cam)
    colour, albedo, nd = aov_frame(tpt, 480, 270)
    assert (albedo[..., 3] > 0).any()
    check_all_modes(tpt, checker, colour, albedo, nd, range(1, 6))


@pytest.mark.parametrize("size,iterations", [((1, 1), 3), ((1, 17), 3), ((33, 7), 4), ((257, 129), 5), ((8192, 2), 3), ((20, 20), 8)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_synthetic_planes(tpt_defaults, checker, size, iterations):
    tpt = tpt_defaults
    w, h = size
    colour, albedo, nd = random_planes(np.random.default_rng(w * 7919 + h), h, w)
    check_all_modes(tpt, checker, colour, albedo, nd, [iterations])


def test_refusals_leave_out_untouched(tpt_defaults):
    import torch
    tpt = tpt_defaults
    lib = tpt.load_library()
    w, h = 64, 40
    colour, albedo, nd = (dev(x) for x in random_planes(np.random.default_rng(2), h, w))
    out = nan_plane(h, w)
    torch.cuda.synchronize()
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def refused(what, ww=w, hh=h, c=colour, a=albedo, n=nd, o=out, it=3, sc=1.0, sn=0.2, sd=0.5, fl=1):
        rc = lib.tptDenoiseDevice(ww, hh, P(c), P(a), P(n), o if isinstance(o, C.c_void_p) else P(o), it, sc, sn, sd, fl)
        msg = lib.tptGetLastError().decode()
        assert rc != 0 and "tptDenoiseDevice" in msg, (what, msg)

    refused("w 0", ww=0)
    refused("h 8193", hh=8193)
    refused("colour NULL", c=None)
    refused("out NULL", o=None)
    refused("out is the albedo", o=albedo)
    refused("out overlaps the colour", o=C.c_void_p(colour.data_ptr() + 16 * 5))
    refused("iterations 9", it=9)
    refused("sigma NaN", sc=float("nan"))
    refused("sigma tiny", sn=1e-7)
    refused("sigma huge", sd=2e6)
    refused("sigmaNormal without the plane", n=None, sd=0.0)
    refused("demodulate without albedo", a=None)
    refused("unknown flag", fl=2)
    tpt.synchronize()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote deviceOut"


def test_streamed_frames_lose_nothing(tpt_defaults, checker):
    """12 streamed tptDrawDevice frames at 640x360x4, each tile denoised into its own output straight after its call: the tiles, the
    rays of the 12 frames, the look-ahead hits and the trace launches are those of the same stream without the denoiser,
    and each output is the checker's filter of its frame's tile"""
    import torch
    tpt = tpt_defaults
    w, h, n = 640, 360, 12
    stream = torch.cuda.Stream()

    def run(denoise):
        tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        outs = [nan_plane(h, w) for _ in range(n)] if denoise else []
        stream.wait_stream(torch.cuda.current_stream())
        torch.cuda.synchronize()
        tpt.set_stream(stream.cuda_stream)
        tiles = []
        try:
            r0 = tpt.ray_counter_read()
            hits0 = tpt.lookahead_hits()
            tpt.kernel_timing_begin(64)
            tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
            with torch.cuda.stream(stream):
                for f in range(n):
                    tpt.draw_device(0.0, f, w, h, tile.data_ptr(), FLAG_PROGRESSIVE)
                    if denoise:
                        tpt.denoise_device(w, h, tile.data_ptr(), outs[f].data_ptr(), iterations=3)
                    tiles.append(tile.clone())  # (stream-ordered behind the frame's blend)
            _, launches = tpt.kernel_timing_end()
            hits = tpt.lookahead_hits() - hits0
            rays = tpt.ray_counter_read() - r0
            stream.synchronize()
        finally:
            tpt.set_stream(None)
        return ([t.cpu().numpy() for t in tiles], rays, hits, launches, [o.cpu().numpy() for o in outs])

    plain = run(False)
    den = run(True)
    assert [t.tobytes() for t in den[0]] == [t.tobytes() for t in plain[0]], "a tile changed"
    assert den[1] == plain[1], (den[1], plain[1])
    assert den[2] == plain[2] and den[3] == plain[3], (den[2:4], plain[2:4])
    from toypathtracer_amd.api import DENOISE_DEFAULTS
    sc = DENOISE_DEFAULTS["sigma_colour"]
    for f in range(n):
        want = checker.run(den[0][f], iterations=3, sigma_colour=sc)
        assert den[4][f].tobytes() == want.tobytes(), f


def test_denoised_4spp_is_closer_to_the_converged_frame(tpt_defaults):
    """640x360, default scene: MSE against a 1024-spp render of the same frame drops to at most QUALITY_BOUND of the raw 4-spp MSE"""
    import torch
    tpt = tpt_defaults
    w, h = 640, 360
    tpt.set_samples_per_pixel(1024)
    ref = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
    tpt.draw_device(0.0, 0, w, h, ref.data_ptr(), FLAG_PROGRESSIVE)
    tpt.synchronize()
    tpt.set_samples_per_pixel(4)
    colour, albedo, nd = aov_frame(tpt, w, h)
    dc, da, dn = dev(colour), dev(albedo), dev(nd)
    out = nan_plane(h, w)
    torch.cuda.synchronize()
    tpt.denoise_device(w, h, dc.data_ptr(), out.data_ptr(), albedo_ptr=da.data_ptr(), normal_depth_ptr=dn.data_ptr())
    tpt.synchronize()
    r = ref.cpu().numpy()[..., :3].astype(np.float64)
    raw = np.mean((colour[..., :3] - r) ** 2)
    den = np.mean((out.cpu().numpy()[..., :3] - r) ** 2)
    print("denoise quality: MSE raw %.6g, denoised %.6g, ratio %.4f" % (raw, den, den / raw))
    assert np.isfinite(den) and den / raw <= QUALITY_BOUND, (raw, den, den / raw)
