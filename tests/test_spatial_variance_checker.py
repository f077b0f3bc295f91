"""tptSpatialVarianceDevice without a GPU: its two CPU statements -- tests/spatial_variance_checker.c and
spatial_variance_lib.spatial_variance_numpy -- agree byte for byte on seeded planes, a stack of frames is its frames one by one, and the
statement has the properties include/tpt_hip.h promises: pixels with enough samples keep the temporal pass's variance bytes, a raw plane
that passes through filters to the very bytes of the raw plane, a flat window estimates exactly 0, and at 1 spp the filter on the
estimate does what the filter on the traced moments cannot."""
import numpy as np
import pytest

from spatial_variance_lib import (KINDS, RADII, SIZES, SpatialVarianceChecker, estimated, own_variance, spatial_variance_numpy,
                                  synthetic_case)

f32 = np.float32
GUIDE = dict(sigma_normal=0.03, sigma_depth=0.5)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return SpatialVarianceChecker(tmp_path_factory.mktemp("spatial_variance_checker"))


def finite(v):
    with np.errstate(all="ignore"):
        return np.abs(v) <= f32(3.40282347e38)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_checker_and_numpy_agree(checker, size, radius):
    w, h = size
    for kind in KINDS:
        for frames in (1, 3):
            moments, nd = synthetic_case(w, h, frames, kind)
            for guide in (None, nd):
                for kw in (dict(), dict(samples_per_frame=2.0, min_samples=4.0), dict(min_samples=float("inf"))):
                    if guide is not None:
                        kw = dict(kw, **GUIDE)
                    got = checker.run(moments, guide, radius=radius, **kw)
                    want = spatial_variance_numpy(moments, guide, radius=radius, **kw)
                    assert got.tobytes() == want.tobytes(), (kind, frames, guide is not None, kw)
                    # a stack is its frames one by one: a window that read across a frame seam would show here
                    for j in range(frames if frames > 1 else 0):
                        one = checker.run(np.ascontiguousarray(moments[j]), None if guide is None else np.ascontiguousarray(guide[j]),
                                          radius=radius, **kw)
                        assert one.tobytes() == got[j].tobytes(), (kind, j, guide is not None, kw)
                    # the form {0, v/N, 0, N}, N >= 1 and finite; pass-through pixels carry step 0's bytes
                    Vt, N = own_variance(moments)
                    est = estimated(moments, kw.get("samples_per_frame", 1.0), kw.get("min_samples", 2.0))
                    assert (got[..., 0] == 0).all() and (got[..., 2] == 0).all() and got[..., 3].tobytes() == N.tobytes()
                    assert finite(N).all() and (N >= 1).all()
                    assert got[~est].tobytes() == Vt[~est].tobytes()
                    assert not np.isnan(got[..., 1]).any() and (got[..., 1] >= 0).all()
                    if "min_samples" not in kw:
                        share = est.mean()
                        if kind == "all":
                            assert share == 1
                        elif kind == "none":
                            assert share == 0 and got.tobytes() == Vt.tobytes()
                        elif kind == "checker" and w * h > 1:
                            assert 0.3 < share < 0.7
                        elif kind == "corner":
                            assert est.sum() == frames and est[:, min(3, h - 1), min(63, w - 1)].all()
                        elif size == (130, 67):
                            assert 0.3 < share < 0.8 and (est & (got != Vt).any(axis=-1)).mean() > 0.2


def test_history_lengths_that_are_no_history(checker):
    """N of 0, below 1, negative, NaN and infinite count as 1 (and so are estimated at 1 spp); a fractional N >= 1 stays"""
    values = np.array([0.0, 0.5, -2.0, np.nan, np.inf, -np.inf, 1.0, 1.5, 1.99, 2.0, 7.25, 3.0e38], f32)
    moments = np.zeros((1, len(values), 4), f32)
    moments[..., 0] = np.linspace(0.5, 1.5, len(values), dtype=f32)
    moments[..., 1] = moments[..., 0] * moments[..., 0] + f32(0.125)
    moments[..., 3] = values
    out = checker.run(moments, radius=1)
    want_N = np.array([1, 1, 1, 1, 1, 1, 1, 1.5, 1.99, 2, 7.25, 3.0e38], f32)
    assert out[0, :, 3].tobytes() == want_N.tobytes()
    est = estimated(moments)[0]
    assert est.tolist() == [True] * 9 + [False] * 3
    Vt, _ = own_variance(moments)
    assert out[0, 9:].tobytes() == Vt[0, 9:].tobytes()
    assert (out[0, :9, 1] != Vt[0, :9, 1]).all()  # (the neighbours' means differ: the window's spread is not the pixel's own)
    assert out.tobytes() == spatial_variance_numpy(moments, radius=1).tobytes()


@pytest.mark.parametrize("radius", RADII)
def test_flat_window_overflow_and_windows_without_a_tap(checker, radius):
    w, h = 70, 12
    moments = np.zeros((h, w, 4), f32)
    moments[..., 0], moments[..., 1], moments[..., 3] = 0.625, 0.390625, 1.0
    nd = np.zeros((h, w, 4), f32)
    nd[..., 2], nd[..., 3] = 1.0, 4.0
    for guide in (None, nd):
        kw = GUIDE if guide is not None else {}
        out = checker.run(moments, guide, radius=radius, **kw)
        assert (out[..., 1] == 0).all() and (out[..., 3] == 1).all()  # (every weight is 1: the sums are exact, e2 == e1*e1)
    # moments whose e1*e1 overflows: e2 - inf is -inf (or NaN for an infinite e2), and the estimate is 0
    big = moments.copy()
    big[..., 0], big[..., 1] = 1e20, 3e38
    out = checker.run(big, radius=radius)
    assert (out[..., 1] == 0).all()
    assert out.tobytes() == spatial_variance_numpy(big, radius=radius).tobytes()
    # no tap counts (every moment in reach is non-finite, the pixel's own included): the pixel's own variance
    rng = np.random.default_rng(11)
    noisy = moments.copy()
    noisy[..., 0] = rng.random((h, w), dtype=f32)
    noisy[..., 1] = noisy[..., 0] * noisy[..., 0] + f32(0.25)
    hole = noisy.copy()
    hole[0:2 * radius + 1, 0:2 * radius + 1, 0] = np.nan
    out = checker.run(hole, radius=radius)
    Vt, _ = own_variance(hole)
    assert out[radius, radius].tobytes() == Vt[radius, radius].tobytes() and out[radius, radius, 1] == 0  # (NaN > 0 is false)
    # ... and with the guide: a non-finite guide pixel at p makes every den NaN
    g = nd.copy()
    g[5, 33, 1] = np.inf
    out = checker.run(noisy, g, radius=radius, **GUIDE)
    Vt, _ = own_variance(noisy)
    assert out[5, 33].tobytes() == Vt[5, 33].tobytes()
    assert out[5, 34].tobytes() != Vt[5, 34].tobytes()  # (its neighbour only loses that tap)
    assert out.tobytes() == spatial_variance_numpy(noisy, g, radius=radius, **GUIDE).tobytes()


def test_checker_refuses_what_the_product_refuses(checker):
    moments, nd = synthetic_case(8, 4)
    assert checker.run(moments, nd, rc=True, **GUIDE) == 0
    assert checker.run(moments, None, rc=True, min_samples=float("inf")) == 0
    for kw in (dict(radius=0), dict(radius=4), dict(samples_per_frame=0.5), dict(samples_per_frame=float("inf")),
               dict(samples_per_frame=float("nan")), dict(min_samples=0.5), dict(min_samples=float("nan")), dict(sigma_normal=-1.0),
               dict(sigma_depth=1e7), dict(sigma_normal=float("nan"))):
        assert checker.run(moments, nd, rc=True, **kw) == -1, kw
    assert checker.run(moments, None, rc=True, sigma_normal=0.03) == -1
    assert checker.run(moments, None, rc=True, sigma_depth=0.5) == -1


# ---------------------------------------------------------------- the chain's other CPU statements
@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """96x54, default scene and camera, frame 0: the traced planes at 1 and 4 spp, and the 1024-spp reference"""
    from moments_lib import MomentsChecker, VarianceChecker
    from oracle_lib import Oracle
    from temporal_lib import TemporalChecker
    d = tmp_path_factory.mktemp("spatial_variance_chain")
    mc, vc, tc = MomentsChecker(d), VarianceChecker(d), TemporalChecker(d)
    o = Oracle.get()
    w, h = 96, 54
    spheres, mats = o.default_scene()
    cam = o.default_camera(w, h)
    traced = {spp: mc.render(spheres, mats, cam, w, h, spp, 0, flags=0)[1:] for spp in (1, 4)}  # colour, moments, albedo, nd
    ref = mc.render(spheres, mats, cam, w, h, 1024, 0, flags=0)[1][..., :3].astype(np.float64)
    return dict(vc=vc, tc=tc, cam=cam, traced=traced, ref=ref, o=o, mc=mc, spheres=spheres, mats=mats, size=(w, h))


def figures(x, ref):
    dd = (x[..., :3].astype(np.float64) - ref) ** 2
    return float(dd.mean()), float((dd / (ref ** 2 + 0.01)).mean())


def test_a_raw_plane_that_passes_through_filters_to_the_raw_plane_s_bytes(checker, chain):
    from moments_lib import DEMODULATE
    from toypathtracer_amd import api
    colour, moments, albedo, nd = chain["traced"][4]
    est = checker.run(moments, nd, samples_per_frame=4.0, **api.SPATIAL_VARIANCE_DEFAULTS)
    Vt, N = own_variance(moments)
    assert est.tobytes() == Vt.tobytes() and (N == 1).all()  # (the draw leaves 0 in .w)
    dd = moments[..., 1] - moments[..., 0] * moments[..., 0]
    assert est[..., 1].tobytes() == np.where(dd > 0, dd, f32(0)).astype(f32).tobytes()
    vc = chain["vc"]
    a = vc.run(colour, albedo, nd, moments, 4.0, flags=DEMODULATE, **api.DENOISE_VARIANCE_DEFAULTS)
    b = vc.run(colour, albedo, nd, est, 4.0, flags=DEMODULATE, **api.DENOISE_VARIANCE_DEFAULTS)
    assert a.tobytes() == b.tobytes()


def test_behind_a_temporal_pass_pixels_with_enough_samples_keep_its_variance(checker, chain):
    """1 spp, animated, max_history 4: frame 0 is estimated everywhere; later frames only where the history was cut"""
    mc, tc, o, cam = chain["mc"], chain["tc"], chain["o"], chain["cam"]
    w, h = chain["size"]
    prev = None
    for j in range(4):
        sp = chain["spheres"].copy()
        o.animate(sp, 0.05 * j)
        _, bb, mo, alb, nd = mc.render(sp, chain["mats"], cam, w, h, 1, j, flags=0)
        oc, oa, om, ov = tc.run(cam, (bb, alb, nd, mo), prev, max_history=4.0)
        prev = (cam, oc, oa, nd, om)
        out = checker.run(om, nd, radius=1, **GUIDE)
        N = om[..., 3]
        keep = N >= 2
        assert out[keep].tobytes() == ov[keep].tobytes()
        assert out[..., 3].tobytes() == ov[..., 3].tobytes()
        assert out.tobytes() == spatial_variance_numpy(om, nd, radius=1, **GUIDE).tobytes()
        if j == 0:
            assert not keep.any() and (ov[..., 1] == 0).all() and (out[..., 1] > 0).mean() > 0.9
        else:
            assert 0.005 < (~keep).mean() < 0.2, (j, (~keep).mean())


@pytest.mark.parametrize("radius", RADII)
def test_quality_at_one_sample_per_pixel(checker, chain, radius):
    """The filter on the window estimate against the filter on the traced moments, 1 spp, frame 0, reference 1024 spp, squared error
    over the raw frame's (linear, relative).  Measured through these statements (bit-exact with the GPU's):
        traced moments            0.99974  0.99544
        estimate, radius 1, 2, 3  0.8933 0.1959,  0.8921 0.2039,  0.8943 0.2350"""
    from moments_lib import DEMODULATE
    from toypathtracer_amd import api
    colour, moments, albedo, nd = chain["traced"][1]
    assert (moments[..., 1] - moments[..., 0] * moments[..., 0] == 0).mean() > 0.99  # ({l, l*l}: no variance of its own)
    kw = dict(api.SPATIAL_VARIANCE_DEFAULTS, radius=radius)
    est = checker.run(moments, nd, samples_per_frame=1.0, **kw)
    vc, ref = chain["vc"], chain["ref"]
    raw = figures(colour, ref)
    own = [a / b for a, b in zip(figures(vc.run(colour, albedo, nd, moments, 1.0, flags=DEMODULATE, **api.DENOISE_VARIANCE_DEFAULTS), ref), raw)]
    new = [a / b for a, b in zip(figures(vc.run(colour, albedo, nd, est, 1.0, flags=DEMODULATE, **api.DENOISE_VARIANCE_DEFAULTS), ref), raw)]
    print("radius %d: traced moments %.5f %.5f, estimate %.5f %.5f" % (radius, own[0], own[1], new[0], new[1]))
    assert new[0] < own[0] and new[1] < own[1]
    assert new[1] < 0.5 * own[1]


def test_four_samples_per_pixel_pass_through_with_the_default_threshold(checker, chain):
    from toypathtracer_amd import api
    _, moments, _, nd = chain["traced"][4]
    assert not estimated(moments, 4.0, api.SPATIAL_VARIANCE_DEFAULTS["min_samples"]).any()
    assert checker.run(moments, nd, samples_per_frame=4.0, **api.SPATIAL_VARIANCE_DEFAULTS).tobytes() == own_variance(moments)[0].tobytes()
