"""The CPU references of the moments feature against what they are built from.  tests/moments_checker.c: its tile and ray count are
tpto_render's and its planes tests/aov_checker.c's, byte for byte; its moments are what the header defines.  tests/variance_checker.c
against moments_lib.variance_numpy, a second statement of the filter, byte for byte: every iteration count from 1 to 8, with and
without each guide, zero and very large variance, image edges; and what the filter must do."""
import numpy as np
import pytest

from aov_lib import AovChecker
from moments_lib import DEMODULATE, MomentsChecker, VarianceChecker, lum, random_moments, random_planes, variance_numpy
from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE, SEED_PER_PIXEL


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return MomentsChecker(tmp_path_factory.mktemp("moments_checker"))


@pytest.fixture(scope="module")
def vchecker(tmp_path_factory):
    return VarianceChecker(tmp_path_factory.mktemp("variance_checker"))


@pytest.mark.parametrize("spp,kw", [(1, {}), (4, {}), (2, dict(light_sampling=False)), (4, dict(mitsuba_compare=True))],
                         ids=["spp1", "spp4", "no_light_sampling", "mitsuba"])
def test_tile_rays_and_planes_are_the_oracles(checker, oracle, tmp_path, spp, kw):
    w, h = 61, 37
    s, m = oracle.default_scene()
    cam = (oracle.camera((0, 2, 3), (0, 0, 0), (0, 1, 0), 60.0, w / h, 0.0, 3.0) if kw.get("mitsuba_compare")
           else oracle.default_camera(w, h))
    rays, bb, mo, alb, nd = checker.render(s, m, cam, w, h, spp, 0, FLAG_PROGRESSIVE, **kw)
    ro, bo = oracle.render(s, m, cam, w, h, spp, 0, FLAG_PROGRESSIVE, seed_mode=SEED_PER_PIXEL, **kw)
    assert rays == ro and bb.tobytes() == bo.tobytes()
    _, _, ao, no = AovChecker(tmp_path).render(s, m, cam, w, h, spp, 0, FLAG_PROGRESSIVE, **kw)
    assert alb.tobytes() == ao.tobytes() and nd.tobytes() == no.tobytes()
    # {mean l, mean l^2, 0}, .w untouched (0 on the zeroed plane); Jensen: mean l^2 >= (mean l)^2 up to rounding
    assert (mo[..., 2] == 0).all() and (mo[..., 3] == 0).all()
    assert (mo[..., 1] >= mo[..., 0] * mo[..., 0] * np.float32(1 - 1e-5)).all()
    if spp == 1:  # one sample: the second moment is the square of the first, exactly
        assert (mo[..., 1] == mo[..., 0] * mo[..., 0]).all()


def test_progressive_frames_blend_the_moments(checker, oracle):
    """frames 0-3: the tile and rays stay tpto_render's; the moments plane is the blend of each frame's own moments"""
    w, h, spp = 48, 30, 2
    s, m = oracle.default_scene()
    cam = oracle.default_camera(w, h)
    bb, mo, bo = (np.zeros((h, w, 4), np.float32) for _ in range(3))
    mo[..., 3] = 5.0  # (.w is the caller's: kept)
    want = mo.copy()
    for f in range(4):
        rays, _, _, _, _ = checker.render(s, m, cam, w, h, spp, f, FLAG_PROGRESSIVE, backbuffer=bb, moments=mo)
        ro, _ = oracle.render(s, m, cam, w, h, spp, f, FLAG_PROGRESSIVE, backbuffer=bo, seed_mode=SEED_PER_PIXEL)
        assert rays == ro and bb.tobytes() == bo.tobytes(), f
        # frame f's own moments: the same frame without the progressive flag (lerp 0) on a zeroed plane
        _, _, frame_only, _, _ = checker.render(s, m, cam, w, h, spp, f, 0)
        lerp = np.float32(f) / np.float32(f + 1)
        frame_moments = frame_only[..., :3]
        want[..., :3] = want[..., :3] * lerp + frame_moments * (np.float32(1) - lerp)
        assert mo.tobytes() == want.tobytes(), f
    assert (mo[..., 3] == 5.0).all()


def test_animated_time(checker, oracle):
    from common import oracle_frames
    w, h, spp, t = 50, 32, 2, 1.7
    flags = FLAG_PROGRESSIVE | FLAG_ANIMATE
    per, bb, mo, _, _ = checker.frames(oracle, w, h, spp, 2, flags=flags, time=t)
    ro, bo, pero = oracle_frames(oracle, w, h, spp, 2, flags=flags, time=t, seed_mode=SEED_PER_PIXEL)
    assert per == pero and bb.tobytes() == bo.tobytes()
    _, _, mo0, _, _ = checker.frames(oracle, w, h, spp, 2)
    assert mo.tobytes() != mo0.tobytes()


# (albedo plane, normal / depth plane, demodulate): every combination the product accepts
MODES = {"both": (True, True, False), "both-demod": (True, True, True), "albedo": (True, False, False), "albedo-demod": (True, False, True),
         "normal_depth": (False, True, False), "none": (False, False, False)}


@pytest.mark.parametrize("size", [(1, 1), (1, 17), (33, 7), (40, 29)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("spread", [0.0, 1.0, 1e30], ids=["zero", "unit", "huge"])
@pytest.mark.parametrize("mode", list(MODES))
def test_checker_equals_the_numpy_statement(vchecker, size, spread, mode):
    w, h = size
    use_alb, use_nd, demod = MODES[mode]
    rng = np.random.default_rng(w * 1000 + h)
    colour, albedo, nd = random_planes(rng, h, w)
    mo = random_moments(rng, colour, spread)
    albedo = albedo if use_alb else None
    nd = nd if use_nd else None
    for it in range(1, 9):
        kw = dict(iterations=it, sigma_luminance=1.5, sigma_normal=0.3 if use_nd else 0.0, sigma_depth=0.9 if use_nd else 0.0,
                  flags=DEMODULATE if demod else 0)
        got = vchecker.run(colour, albedo, nd, mo, 3.0, **kw)
        want = variance_numpy(colour, albedo, nd, mo, 3.0, **kw)
        assert got.tobytes() == want.tobytes(), "iterations %d" % it
        assert np.isfinite(got).all()


def test_checker_refuses_what_the_product_refuses(vchecker):
    rng = np.random.default_rng(1)
    colour, albedo, nd = random_planes(rng, 4, 4)
    mo = random_moments(rng, colour)
    for kw in (dict(iterations=0), dict(iterations=9), dict(samples=0.5), dict(samples=float("nan")), dict(samples=float("inf")),
               dict(sigma_luminance=0.0), dict(sigma_luminance=-1.0), dict(sigma_luminance=2e6), dict(sigma_luminance=float("nan")),
               dict(sigma_normal=1e-7), dict(flags=2), dict(sigma_normal=0.5, nd=None), dict(flags=DEMODULATE, albedo=None),
               dict(mo=None)):
        a = dict(albedo=albedo, nd=nd, mo=mo, samples=4.0, sigma_normal=0.2, flags=DEMODULATE)
        a.update(kw)
        alb, n, m, s = a.pop("albedo"), a.pop("nd"), a.pop("mo"), a.pop("samples")
        with pytest.raises(AssertionError):
            vchecker.run(colour, alb, n, m, s, **a)


def test_zero_variance_keeps_luminance_edges_large_variance_blurs(vchecker):
    """a flat-guided image of two luminance levels: with zero variance (a converged image) the filter keeps the step to within 1 %;
    with a variance far above the step it blurs across it like the plain spline"""
    w, h, edge = 48, 24, 24
    colour = np.zeros((h, w, 4), np.float32)
    colour[:, :edge, :3] = 0.2
    colour[:, edge:, :3] = 2.0
    mo = np.zeros((h, w, 4), np.float32)
    mo[..., 0] = lum(colour[..., 0], colour[..., 1], colour[..., 2])
    mo[..., 1] = mo[..., 0] * mo[..., 0]
    sharp = vchecker.run(colour, None, None, mo, 4.0, iterations=5, sigma_luminance=4.0)
    assert (np.abs(sharp[:, : edge - 1, :3] / np.float32(0.2) - 1) < 0.01).all()
    assert (np.abs(sharp[:, edge + 1:, :3] / np.float32(2.0) - 1) < 0.01).all()
    noisy = mo.copy()
    noisy[..., 1] += 1e4
    blur = vchecker.run(colour, None, None, noisy, 4.0, iterations=5, sigma_luminance=4.0)
    assert (np.abs(blur[:, edge - 2, :3] / np.float32(0.2) - 1) > 0.5).all()


def test_constant_image_stays_constant(vchecker):
    w, h = 40, 30
    rng = np.random.default_rng(5)
    _, albedo, nd = random_planes(rng, h, w)
    colour = np.empty((h, w, 4), np.float32)
    colour[...] = (0.25, 2.0, 0.5, 1.0)
    mo = random_moments(rng, colour)
    for it in (1, 3, 8):
        out = vchecker.run(colour, None, nd, mo, 4.0, iterations=it, sigma_luminance=2.0, sigma_normal=0.2, sigma_depth=1.0)
        assert out.tobytes() == colour.tobytes(), it  # (powers of two: every product with a weight exact)
