"""tptDenoiseDeviceVariance on the GPU: the variance-guided a-trous filter held byte for byte against its C and numpy statements
(tests/variance_checker.c, moments_lib.variance_numpy) on real tptDrawDeviceMoments planes in every mode and on synthetic ones; its
inputs left alone; refusals that write nothing; and the two quality figures -- a single 4-spp frame (Q1) and 64 accumulated frames
(Q2) against converged renders, beside tptDenoiseDevice's fixed-sigma figures for the same images."""
import ctypes as C

import numpy as np
import pytest

from moments_lib import DEMODULATE, VarianceChecker, random_moments, random_planes, variance_numpy
from oracle_lib import FLAG_PROGRESSIVE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return VarianceChecker(tmp_path_factory.mktemp("variance_checker"))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan_plane(h, w):
    import torch
    return torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda")


def moments_frames(tpt, w, h, frames, average_guides=False):
    """frames 0..frames-1 through tptDrawDeviceMoments -> (tile, albedo, normalDepth, moments) as host arrays.  The guide planes are
    the last frame's, or with average_guides their running mean over the frames, blended like the tile (what a progressive caller
    that denoises the accumulated tile does: include/tpt_hip.h)"""
    import torch
    tile, mo, alb_avg, nd_avg = (torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(4))
    alb, nd = nan_plane(h, w), nan_plane(h, w)
    torch.cuda.synchronize()
    for f in range(frames):
        tpt.UpdateTest(0.0, f, w, h, FLAG_PROGRESSIVE)
        tpt.draw_device_moments(0.0, f, w, h, tile.data_ptr(), mo.data_ptr(), FLAG_PROGRESSIVE, albedo_ptr=alb.data_ptr(),
                                normal_depth_ptr=nd.data_ptr())
        if average_guides:
            lerp = float(np.float32(f) / np.float32(f + 1))
            for avg, plane in ((alb_avg, alb), (nd_avg, nd)):
                avg.mul_(lerp).add_(plane * (1.0 - lerp))
    tpt.synchronize()
    if average_guides:
        alb, nd = alb_avg, nd_avg
    return tile.cpu().numpy(), alb.cpu().numpy(), nd.cpu().numpy(), mo.cpu().numpy()


def denoise_gpu(tpt, colour, albedo, nd, moments, samples, iterations, sl, sn, sd, demod):
    """tptDenoiseDeviceVariance on copies of the host planes -> (out, the inputs as they are after the call)"""
    import torch
    h, w = colour.shape[:2]
    dc, dm = dev(colour), dev(moments)
    da = None if albedo is None else dev(albedo)
    dn = None if nd is None else dev(nd)
    out = nan_plane(h, w)
    torch.cuda.synchronize()
    tpt.denoise_device_variance(w, h, dc.data_ptr(), dm.data_ptr(), samples, out.data_ptr(), albedo_ptr=None if da is None else da.data_ptr(),
                                normal_depth_ptr=None if dn is None else dn.data_ptr(), iterations=iterations, sigma_luminance=sl,
                                sigma_normal=sn, sigma_depth=sd, demodulate=demod)
    tpt.synchronize()
    return out.cpu().numpy(), [None if t is None else t.cpu().numpy() for t in (dc, da, dn, dm)]


MODES = ((True, True, True), (True, True, False), (False, True, False), (True, False, True), (True, False, False), (False, False, False))


def same_bytes(got, want):
    return got.tobytes() == want.tobytes()


def check_all_modes(tpt, checker, colour, albedo, nd, moments, samples, iterations, sl=None, numpy_too=False, same=same_bytes, guides=None):
    """every mode of the call against the checker, compared with `same` (byte equality unless the caller's reference holds NaNs, whose
    payload is not part of the contract); guides: (sigma_normal, sigma_depth), None for the api's defaults"""
    from toypathtracer_amd.api import DENOISE_VARIANCE_DEFAULTS as D
    sl = D["sigma_luminance"] if sl is None else sl
    guides = (D["sigma_normal"], D["sigma_depth"]) if guides is None else guides
    for use_alb, use_nd, demod in MODES:
        a = albedo if use_alb else None
        n = nd if use_nd else None
        sn, sd = guides if use_nd else (0.0, 0.0)
        for it in iterations:
            got, ins = denoise_gpu(tpt, colour, a, n, moments, samples, it, sl, sn, sd, demod)
            kw = dict(iterations=it, sigma_luminance=sl, sigma_normal=sn, sigma_depth=sd, flags=DEMODULATE if demod else 0)
            want = checker.run(colour, a, n, moments, samples, **kw)
            assert same(got, want), (use_alb, use_nd, demod, it)
            if numpy_too:
                assert same(got, variance_numpy(colour, a, n, moments, samples, **kw)), (use_alb, use_nd, demod, it)
            for x, y in zip(ins, (colour, a, n, moments)):
                assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), "an input was written"


def test_real_planes_single_frame_640x360(tpt_defaults, checker):
    tpt = tpt_defaults
    colour, albedo, nd, mo = moments_frames(tpt, 640, 360, 1)
    check_all_modes(tpt, checker, colour, albedo, nd, mo, tpt.moment_samples(4), range(1, 6))


def test_real_planes_progressive_256x144(tpt_defaults, checker):
    tpt = tpt_defaults
    colour, albedo, nd, mo = moments_frames(tpt, 256, 144, 6)
    check_all_modes(tpt, checker, colour, albedo, nd, mo, tpt.moment_samples(4, 5, FLAG_PROGRESSIVE), [1, 5, 8], numpy_too=True)


@pytest.mark.parametrize("size,iterations,spread", [((1, 1), 3, 1.0), ((1, 17), 3, 1.0), ((33, 7), 4, 0.0), ((130, 67), 5, 1e30),
                                                    ((8192, 2), 3, 1.0), ((20, 20), 8, 1e-3)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_synthetic_planes(tpt_defaults, checker, size, iterations, spread):
    """zero variance (spread 0), a very large one (1e30) and image edges"""
    tpt = tpt_defaults
    w, h = size
    rng = np.random.default_rng(w * 7919 + h)
    colour, albedo, nd = random_planes(rng, h, w)
    mo = random_moments(rng, colour, spread)
    check_all_modes(tpt, checker, colour, albedo, nd, mo, 3.0, [iterations], sl=2.0)


def test_refusals_leave_out_untouched(tpt_defaults):
    import torch
    tpt = tpt_defaults
    lib = tpt.load_library()
    w, h = 64, 40
    rng = np.random.default_rng(2)
    c0, a0, n0 = random_planes(rng, h, w)
    colour, albedo, nd, mo = dev(c0), dev(a0), dev(n0), dev(random_moments(rng, c0))
    out = nan_plane(h, w)
    torch.cuda.synchronize()
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    count = [0]

    def refused(what, ww=w, hh=h, c=colour, a=albedo, n=nd, m=mo, s=4.0, o=out, it=3, sl=4.0, sn=0.2, sd=0.5, fl=1):
        rc = lib.tptDenoiseDeviceVariance(ww, hh, P(c), P(a), P(n), m if isinstance(m, C.c_void_p) else P(m), C.c_float(s),
                                          o if isinstance(o, C.c_void_p) else P(o), it, C.c_float(sl), C.c_float(sn), C.c_float(sd), fl)
        msg = lib.tptGetLastError().decode()
        assert rc != 0 and "tptDenoiseDeviceVariance" in msg, (what, msg)
        tpt.synchronize()
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), "a refused call wrote deviceOut: " + what
        count[0] += 1

    refused("w 0", ww=0)
    refused("h 8193", hh=8193)
    refused("colour NULL", c=None)
    refused("out NULL", o=None)
    refused("moments NULL", m=None)
    refused("out is the moments", o=mo)
    refused("out overlaps the moments", m=C.c_void_p(out.data_ptr() + 16 * 9))
    refused("out is the albedo", o=albedo)
    refused("iterations 0", it=0)
    refused("iterations 9", it=9)
    for s in (0.0, 0.5, float("nan"), float("inf"), -3.0):
        refused("samples %r" % s, s=s)
    for sl in (0.0, -1.0, 2e6, float("nan"), float("inf")):
        refused("sigmaLuminance %r" % sl, sl=sl)
    refused("sigmaNormal tiny", sn=1e-7)
    refused("sigmaNormal without the plane", n=None, sd=0.0)
    refused("demodulate without albedo", a=None)
    refused("unknown flag", fl=2)
    assert count[0] == 24


def mse(a, ref):
    return float(np.mean((a[..., :3].astype(np.float64) - ref) ** 2))


def reference(tpt, w, h, spp, frames):
    """frames 0..frames-1 at spp accumulated by tptDrawDevice -> float64 rgb"""
    import torch
    tpt.set_samples_per_pixel(spp)
    ref = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for f in range(frames):
        tpt.UpdateTest(0.0, f, w, h, FLAG_PROGRESSIVE)
        tpt.draw_device(0.0, f, w, h, ref.data_ptr(), FLAG_PROGRESSIVE)
    tpt.synchronize()
    tpt.set_samples_per_pixel(4)
    return ref.cpu().numpy()[..., :3].astype(np.float64)


def both_filters(tpt, colour, albedo, nd, mo, samples):
    """-> (variance-guided output at DENOISE_VARIANCE_DEFAULTS, fixed-sigma output at DENOISE_DEFAULTS), both guides, demodulated"""
    import torch
    h, w = colour.shape[:2]
    dc, da, dn, dm = dev(colour), dev(albedo), dev(nd), dev(mo)
    var, fix = nan_plane(h, w), nan_plane(h, w)
    torch.cuda.synchronize()
    tpt.denoise_device_variance(w, h, dc.data_ptr(), dm.data_ptr(), samples, var.data_ptr(), albedo_ptr=da.data_ptr(),
                                normal_depth_ptr=dn.data_ptr())
    tpt.denoise_device(w, h, dc.data_ptr(), fix.data_ptr(), albedo_ptr=da.data_ptr(), normal_depth_ptr=dn.data_ptr())
    tpt.synchronize()
    return var.cpu().numpy(), fix.cpu().numpy()


def test_q1_single_4spp_frame(tpt_defaults):
    """640x360 default scene, one 4-spp frame against 1024 spp: the variance-guided MSE ratio is at most tptDenoiseDevice's"""
    tpt = tpt_defaults
    w, h = 640, 360
    ref = reference(tpt, w, h, 1024, 1)
    colour, albedo, nd, mo = moments_frames(tpt, w, h, 1)
    var, fix = both_filters(tpt, colour, albedo, nd, mo, tpt.moment_samples(4))
    raw = mse(colour, ref)
    rv, rf = mse(var, ref) / raw, mse(fix, ref) / raw
    print("Q1: MSE raw %.6g; variance-guided / raw %.4f; fixed-sigma / raw %.4f" % (raw, rv, rf))
    assert np.isfinite(rv) and rv <= rf, (rv, rf)


def test_q2_64_progressive_frames(tpt_defaults):
    """640x360 default scene, 64 accumulated 4-spp frames (256 samples) against 4 accumulated 1024-spp frames (4096 samples), the guide
    planes averaged over the frames like the tile: the variance-guided output is no further from the reference than the raw
    accumulated image; the fixed-sigma figure for the same image is printed beside it"""
    tpt = tpt_defaults
    w, h = 640, 360
    ref = reference(tpt, w, h, 1024, 4)
    colour, albedo, nd, mo = moments_frames(tpt, w, h, 64, average_guides=True)
    var, fix = both_filters(tpt, colour, albedo, nd, mo, tpt.moment_samples(4, 63, FLAG_PROGRESSIVE))
    raw = mse(colour, ref)
    rv, rf = mse(var, ref) / raw, mse(fix, ref) / raw
    print("Q2: MSE raw %.6g; variance-guided / raw %.4f; fixed-sigma / raw %.4f" % (raw, rv, rf))
    assert np.isfinite(rv) and rv <= 1.0, (rv, rf)
