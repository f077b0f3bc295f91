"""tptSpatialVarianceDevice on the GPU: the call held byte for byte against its C statement (tests/spatial_variance_checker.c) on the
synthetic planes of tests/test_spatial_variance_checker.py, on the moments of a real 1-spp chain through tptTemporalAccumulateDevice and
on a stack of views from tptDrawDeviceCameraClip; its inputs left alone; refusals that write nothing; and, at 1 spp, the filter on the
estimate against the filter on the traced moments."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle_lib import FLAG_ANIMATE
from spatial_variance_lib import KINDS, RADII, SIZES, SpatialVarianceChecker, estimated, own_variance, synthetic_case
from test_gpu_temporal import accumulate, dev, figures, host, plane, spatial, trace_frame

pytestmark = pytest.mark.gpu
GUIDE = dict(sigma_normal=0.03, sigma_depth=0.5)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return SpatialVarianceChecker(tmp_path_factory.mktemp("spatial_variance_checker"))


def stack(frames, h, w, fill=0.0):
    import torch
    return torch.full((frames, h, w, 4), fill, dtype=torch.float32, device="cuda")


def estimate(tpt, w, h, moments, nd=None, frames=1, **kw):
    """the call on device planes -> its output on the device, in the shape of `moments`"""
    import torch
    out = torch.full_like(moments, float("nan"))
    torch.cuda.synchronize()
    tpt.spatial_variance_device(w, h, moments.data_ptr(), out.data_ptr(), None if nd is None else nd.data_ptr(), frames=frames, **kw)
    return out


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_synthetic_planes(tpt_defaults, checker, size):
    tpt = tpt_defaults
    w, h = size
    for kind in KINDS:
        for frames in (1, 3):
            moments, nd = synthetic_case(w, h, frames, kind)
            dm, dn = dev(moments), dev(nd)
            for radius in RADII:
                for guide, dg in ((None, None), (nd, dn)):
                    kw = dict(radius=radius, **(GUIDE if guide is not None else dict(sigma_normal=0.0, sigma_depth=0.0)))
                    for more in (dict(), dict(samples_per_frame=2.0, min_samples=4.0), dict(min_samples=float("inf"))):
                        if more and (kind != "mixed" or radius != 2):
                            continue
                        want = checker.run(moments, guide, **kw, **more)
                        got = estimate(tpt, w, h, dm, dg, frames, **kw, **more)
                        tpt.synchronize()
                        assert got.cpu().numpy().tobytes() == want.tobytes(), (kind, frames, radius, guide is not None, more)
            assert dm.cpu().numpy().tobytes() == moments.tobytes() and dn.cpu().numpy().tobytes() == nd.tobytes(), "an input was written"


def test_behind_the_temporal_pass(tpt_defaults, checker):
    """96x54, 1 spp, 6 animated frames through tptTemporalAccumulateDevice at maxHistory 4, the new call on its deviceOutMoments: equal
    to the checker on the GPU's own inputs frame by frame, and the pass's own variance bytes wherever N >= 2"""
    tpt = tpt_defaults
    w, h, frames = 96, 54, 6
    tpt.set_samples_per_pixel(1)
    try:
        prev = None
        for j in range(frames):
            cam, cur = trace_frame(tpt, w, h, j, FLAG_ANIMATE, 0.05 * j)
            acc = accumulate(tpt, w, h, cam, cur, prev, max_history=4.0)
            tpt.synchronize()
            om, ov, nd = host([acc[2], acc[3], cur[2]])
            for radius in RADII:
                out = estimate(tpt, w, h, acc[2], cur[2], radius=radius, **GUIDE)
                tpt.synchronize()
                got = out.cpu().numpy()
                assert got.tobytes() == checker.run(om, nd, radius=radius, **GUIDE).tobytes(), "frame %d, radius %d" % (j, radius)
                keep = om[..., 3] >= 2
                assert got[keep].tobytes() == ov[keep].tobytes(), "frame %d: a pixel with N >= 2 lost the pass's variance" % j
            assert all(a.tobytes() == b.tobytes() for a, b in zip((om, ov, nd), host([acc[2], acc[3], cur[2]]))), "an input was written"
            share = float((~keep).mean())
            assert share == 1.0 if j == 0 else 0.0 < share < 0.2, (j, share)
            prev = (cam, acc[0], acc[1], cur[2], acc[2])
    finally:
        tpt.set_samples_per_pixel(4)


def test_a_stack_of_views_is_its_frames_one_by_one(tpt_defaults, checker):
    """three 1-spp views from tptDrawDeviceCameraClip through one call: plane j equals the per-frame call's, and the checker's"""
    tpt = tpt_defaults
    w, h, n = 96, 54, 3
    views = np.array([[3.0 * math.sin(a), 2.0, 3.0 * math.cos(a), 0, 0, 0, 60.0, 0.02, 3.0] for a in (0.0, 0.7, 1.4)], np.float32)
    times = [0.0] * n
    tpt.set_samples_per_pixel(1)
    try:
        import torch
        tile, mo = plane(h, w), plane(h, w)
        fmo, nd = stack(n, h, w, float("nan")), stack(n, h, w, float("nan"))
        torch.cuda.synchronize()
        tpt.UpdateTest(0.0, 0, w, h, 0)
        tpt.draw_device_camera_clip(times, views, 0, w, h, tile.data_ptr(), mo.data_ptr(), 0, normal_depth_ptr=nd.data_ptr(),
                                    frame_moments_ptr=fmo.data_ptr(), cameras=False)
        tpt.synchronize()
        for radius in RADII:
            whole = estimate(tpt, w, h, fmo, nd, n, radius=radius, **GUIDE)
            tpt.synchronize()
            got = whole.cpu().numpy()
            assert got.tobytes() == checker.run(fmo.cpu().numpy(), nd.cpu().numpy(), radius=radius, **GUIDE).tobytes()
            for j in range(n):
                one = estimate(tpt, w, h, fmo[j], nd[j], radius=radius, **GUIDE)
                tpt.synchronize()
                assert one.cpu().numpy().tobytes() == got[j].tobytes(), "view %d, radius %d" % (j, radius)
            assert (got[..., 3] == 1).all() and (got[..., 1] > 0).mean() > 0.5
        assert not (got[0] == got[1]).all()
    finally:
        tpt.set_samples_per_pixel(4)
        tpt.set_camera(None)


def test_refusals_leave_out_untouched(tpt_defaults):
    import torch
    tpt = tpt_defaults
    lib = tpt.load_library()
    w, h, n = 64, 20, 2
    moments, guide = (dev(a) for a in synthetic_case(w, h, n))
    out = stack(n, h, w, float("nan"))
    big = stack(2 * n, h, w, float("nan"))
    planes = 16 * w * h * n
    torch.cuda.synchronize()
    count = [0]

    def refused(what, ww=w, hh=h, frames=n, m=moments.data_ptr(), g=guide.data_ptr(), o=out.data_ptr(), spp=1.0, ms=2.0, radius=2,
                sn=0.03, sd=0.5):
        rc = lib.tptSpatialVarianceDevice(ww, hh, frames, *[C.c_void_p(p) if p else None for p in (m, g, o)], C.c_float(spp), C.c_float(ms),
                                          radius, C.c_float(sn), C.c_float(sd))
        msg = lib.tptGetLastError().decode()
        assert rc != 0 and "tptSpatialVarianceDevice" in msg, (what, msg)
        tpt.synchronize()
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(big).all()), "a refused call wrote an output: " + what
        count[0] += 1

    refused("w 0", ww=0)
    refused("h 8193", hh=8193)
    refused("nFrames 0", frames=0)
    refused("nFrames 4097", frames=4097)
    refused("moments NULL", m=0)
    refused("output NULL", o=0)
    for r in (0, 4, -2):
        refused("radius %d" % r, radius=r)
    for s in (0.5, float("nan"), float("inf")):
        refused("samplesPerFrame %r" % s, spp=s)
    for s in (0.5, float("nan")):
        refused("minSamples %r" % s, ms=s)
    refused("sigmaNormal negative", sn=-1.0)
    refused("sigmaDepth NaN", sd=float("nan"))
    refused("a sigma without the plane", g=0)
    refused("the output is the moments", o=moments.data_ptr())
    refused("the output is the guide", o=guide.data_ptr())
    refused("the output starts in the moments' last pixel", m=big.data_ptr(), o=big.data_ptr() + planes - 16)
    refused("the guide starts in the output's last pixel", g=big.data_ptr() + planes - 16, o=big.data_ptr())
    assert count[0] == 6 + 3 + 3 + 2 + 3 + 4


def test_quality_at_one_and_four_samples_per_pixel(tpt_defaults):
    """96x54, frame 0, reference 1024 spp, squared error over the raw frame's (linear, relative).  At 1 spp the filter
    (DENOISE_VARIANCE_DEFAULTS, demodulated) on the traced moments leaves the frame as it found it: 0.99974, 0.99544.  On the window
    estimate (SPATIAL_VARIANCE_DEFAULTS' sigmas and threshold) it gives 0.8933, 0.1959 at radius 1; 0.8921, 0.2039 at radius 2; 0.8943,
    0.2350 at radius 3 -- the figures of the CPU statements (tests/test_spatial_variance_checker.py), with which trace, estimate and
    filter are bit-exact.  At 4 spp the default threshold passes every pixel through."""
    tpt = tpt_defaults
    w, h = 96, 54
    try:
        tpt.set_samples_per_pixel(1024)
        _, ref = trace_frame(tpt, w, h, 0, 0, 0.0)
        tpt.synchronize()
        ref = ref[0].cpu().numpy()[..., :3].astype(np.float64)
        tpt.set_samples_per_pixel(1)
        _, cur = trace_frame(tpt, w, h, 0, 0, 0.0)
        tpt.synchronize()
        raw = figures(cur[0].cpu().numpy(), ref)
        over = lambda x: [a / b for a, b in zip(figures(x, ref), raw)]  # noqa: E731
        own = over(spatial(tpt, w, h, cur[0], cur[1], cur[2], cur[3], 1))
        for radius in RADII:
            est = estimate(tpt, w, h, cur[3], cur[2], samples_per_frame=1.0, **dict(tpt.SPATIAL_VARIANCE_DEFAULTS, radius=radius))
            new = over(spatial(tpt, w, h, cur[0], cur[1], cur[2], est, 1))
            print("1 spp, radius %d: traced moments %.5f %.5f, estimate %.5f %.5f" % (radius, own[0], own[1], new[0], new[1]))
            assert new[0] < own[0] and new[1] < own[1], (radius, own, new)
            assert new[1] < 0.5 * own[1], (radius, own, new)
        tpt.set_samples_per_pixel(4)
        _, cur = trace_frame(tpt, w, h, 0, 0, 0.0)
        est = estimate(tpt, w, h, cur[3], cur[2], samples_per_frame=4.0, **tpt.SPATIAL_VARIANCE_DEFAULTS)
        tpt.synchronize()
        moments = cur[3].cpu().numpy()
        assert not estimated(moments, 4.0, tpt.SPATIAL_VARIANCE_DEFAULTS["min_samples"]).any()
        assert est.cpu().numpy().tobytes() == own_variance(moments)[0].tobytes()
    finally:
        tpt.set_samples_per_pixel(4)
