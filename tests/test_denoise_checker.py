"""The CPU statement of tptDenoiseDevice's filter (tests/denoise_checker.c) against a second, vectorised numpy float32 statement of the
same formula, byte for byte, and against what the filter must do: keep a constant image, be the plain B3-spline a-trous blur when every
sigma is 0, and keep a hard edge between two normals."""
import numpy as np
import pytest

from denoise_lib import DEMODULATE, HK, DenoiseChecker, denoise_numpy, random_planes


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return DenoiseChecker(tmp_path_factory.mktemp("denoise_checker"))


# (albedo plane, normal / depth plane, demodulate): every combination the product accepts
MODES = {"both": (True, True, False), "both-demod": (True, True, True), "albedo": (True, False, False), "albedo-demod": (True, False, True),
         "normal_depth": (False, True, False), "none": (False, False, False)}


@pytest.mark.parametrize("size", [(1, 1), (1, 17), (33, 7), (64, 48)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mode", list(MODES))
def test_checker_equals_the_numpy_statement(checker, size, mode):
    w, h = size
    use_alb, use_nd, demod = MODES[mode]
    rng = np.random.default_rng(w * 1000 + h)
    colour, albedo, nd = random_planes(rng, h, w)
    albedo = albedo if use_alb else None
    nd = nd if use_nd else None
    for it in range(1, 9):
        kw = dict(iterations=it, sigma_colour=0.7, sigma_normal=0.3 if use_nd else 0.0, sigma_depth=0.9 if use_nd else 0.0,
                  flags=DEMODULATE if demod else 0)
        got = checker.run(colour, albedo, nd, **kw)
        want = denoise_numpy(colour, albedo, nd, **kw)
        assert got.tobytes() == want.tobytes(), "iterations %d" % it
        assert np.isfinite(got).all()


def test_checker_refuses_what_the_product_refuses(checker):
    colour, albedo, nd = random_planes(np.random.default_rng(1), 4, 4)
    for kw in (dict(iterations=0), dict(iterations=9), dict(sigma_colour=-1.0), dict(sigma_colour=float("nan")),
               dict(sigma_colour=float("inf")), dict(sigma_colour=1e-7), dict(sigma_colour=2e6), dict(flags=2),
               dict(sigma_normal=0.5, nd=None), dict(sigma_depth=0.5, nd=None), dict(flags=DEMODULATE, albedo=None)):
        a = dict(albedo=albedo, nd=nd)
        a.update(kw)
        alb, n = a.pop("albedo"), a.pop("nd")
        with pytest.raises(AssertionError):
            checker.run(colour, alb, n, **a)


@pytest.mark.parametrize("demod", [False, True], ids=["plain", "demod"])
def test_constant_image_stays_constant(checker, demod):
    """the weights of a constant image are the guides' alone, and the quotient of the two 25-term sums is the constant up to their
    roundings: a few ulp per iteration, not compounding (measured: at most 12 ulp after 8 iterations); exact for powers of two, whose
    products with the weights are exact, as long as nothing is demodulated"""
    w, h = 40, 30
    albedo = np.full((h, w, 4), 0.6, np.float32)
    _, _, nd = random_planes(np.random.default_rng(5), h, w)
    for value, exact in (((0.3, 1.7, 0.05, 1.0), False), ((0.25, 2.0, 0.5, 1.0), not demod)):
        colour = np.empty((h, w, 4), np.float32)
        colour[...] = value
        for it in (1, 3, 8):
            out = checker.run(colour, albedo, nd, iterations=it, sigma_colour=0.5, sigma_normal=0.2, sigma_depth=1.0,
                              flags=DEMODULATE if demod else 0)
            err = np.abs(out[..., :3] - colour[..., :3]) / np.spacing(colour[..., :3])
            assert err.max() <= (0 if exact else 16), (value, it, err.max())
            assert (out[..., 3] == colour[..., 3]).all()


def b3_blur(img, iterations):
    """the plain B3-spline a-trous blur with skipped off-image taps, in float64"""
    h, w = img.shape[:2]
    cur = img[..., :3].astype(np.float64)
    k = HK.astype(np.float64)
    for i in range(iterations):
        s = 1 << i
        num = np.zeros_like(cur)
        den = np.zeros((h, w))
        for ky in range(5):
            for kx in range(5):
                oy, ox = (ky - 2) * s, (kx - 2) * s
                ys, xs = np.arange(h) + oy, np.arange(w) + ox
                valid = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
                q = cur[np.clip(ys, 0, h - 1)][:, np.clip(xs, 0, w - 1)]
                wt = k[ky] * k[kx] * valid
                num += wt[..., None] * q
                den += wt
        cur = num / den[..., None]
    return cur


def test_zero_sigmas_are_the_b3_spline_blur(checker):
    w, h = 50, 37
    colour, albedo, nd = random_planes(np.random.default_rng(9), h, w)
    for it in (1, 2, 5):
        out = checker.run(colour, albedo, nd, iterations=it)  # every sigma 0: the weights are the spline's alone
        want = b3_blur(colour, it)
        np.testing.assert_allclose(out[..., :3], want, rtol=2e-6, atol=1e-6)
        # ... whatever the guides are
        assert out.tobytes() == checker.run(colour, None, None, iterations=it).tobytes()


def test_hard_normal_edge_survives_a_small_sigma_normal(checker):
    """left half faces +x, right half +y, each side a noisy but otherwise flat colour: pixels two or more columns from the edge stay
    within 1 % of their side's value"""
    w, h, edge = 64, 32, 32
    rng = np.random.default_rng(3)
    colour = np.zeros((h, w, 4), np.float32)
    colour[:, :edge, :3] = 0.2
    colour[:, edge:, :3] = 2.0
    colour[..., :3] *= (1 + np.float32(0.002) * rng.standard_normal((h, w, 1))).astype(np.float32)
    nd = np.zeros((h, w, 4), np.float32)
    nd[:, :edge, 0] = 1
    nd[:, edge:, 1] = 1
    nd[..., 3] = 5
    out = checker.run(colour, None, nd, iterations=5, sigma_colour=0.0, sigma_normal=0.01)
    cols = np.arange(w)
    left, right = cols <= edge - 2, cols >= edge + 1
    assert (np.abs(out[:, left, :3] / np.float32(0.2) - 1) < 0.01).all()
    assert (np.abs(out[:, right, :3] / np.float32(2.0) - 1) < 0.01).all()
    # ... and without the normal guide the edge is blurred well beyond that
    blur = checker.run(colour, None, None, iterations=5)
    assert (np.abs(blur[:, edge - 3, :3] / np.float32(0.2) - 1) > 0.05).all()
