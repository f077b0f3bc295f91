"""tptRectifyHistoryDevice without a GPU: its two CPU statements -- tests/rectify_checker.c and rectify_lib.rectify_numpy -- agree byte
for byte on seeded planes, and the statement has the properties include/tpt_hip.h promises: a history inside every bound comes back
as it went in, a switched light pulls the history to this frame and shortens it to under two frames, the result lies between the
accumulated and this frame's value, and the history never grows."""
import numpy as np
import pytest

from rectify_lib import NAMES, SIZES, RectifyChecker, luminance_moments, rectify_numpy, synthetic_case

f32 = np.float32
EPS = f32(2.0 ** -23)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return RectifyChecker(tmp_path_factory.mktemp("rectify_checker"))


def finite(v):
    return np.abs(v) <= f32(3.40282347e38)


def passed_through(planes):
    colour, _, acc, am = planes
    N = am[..., 3]
    with np.errstate(all="ignore"):
        return ~(finite(N) & (N > 1)) | ~finite(colour[..., :3]).all(axis=-1) | ~finite(acc[..., :3]).all(axis=-1)


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_checker_and_numpy_agree(checker, size, radius):
    w, h = size
    planes = synthetic_case(w, h)
    through = passed_through(planes)
    colour, _, acc, am = planes
    N = am[..., 3]
    for gamma in (0.0, 0.75, 3.0):
        got = checker.run(*planes, radius=radius, gamma=gamma)
        want, d = rectify_numpy(*planes, radius=radius, gamma=gamma, details=True)
        for name, g, n in zip(NAMES, got, want):
            assert g.tobytes() == n.tobytes(), (name, gamma)
        in_place = checker.run(*planes, radius=radius, gamma=gamma, in_place=True)
        for name, g, n in zip(NAMES, got, in_place):
            assert g.tobytes() == n.tobytes(), ("in place", name, gamma)
        assert (d["through"] == through).all()
        # pass-through and unclipped pixels: the accumulated planes' bytes
        keep = d["keep"]
        assert got[0][keep].tobytes() == acc[keep].tobytes() and got[1][keep].tobytes() == am[keep].tobytes()
        assert got[2][..., 3].tobytes() == got[1][..., 3].tobytes() and (got[2][..., 0] == 0).all() and (got[2][..., 2] == 0).all()
        # (d) the history never grows, and never falls under one frame
        N1 = got[1][..., 3]
        assert (N1[~through] >= 1).all() and (N1[~through] <= N[~through]).all()
        assert (got[0][..., 3].tobytes() == acc[..., 3].tobytes())  # (the colour's alpha)
        # (c) between the accumulated and this frame's value: L and U are blends of values on either side of cur with cur, each a
        #     product pair and a sum of binary32 -- three roundings of magnitudes up to |lo| + |cur|
        o, a3, c3 = got[0][~through, :3], acc[~through, :3], colour[~through, :3]
        slack = f32(4) * EPS * (np.abs(a3) + np.abs(c3) + np.abs(o))
        assert (o >= np.minimum(a3, c3) - slack).all() and (o <= np.maximum(a3, c3) + slack).all()
        if size == (130, 67):
            clipped = ~keep
            assert clipped.mean() > 0.1 and (keep & ~through).mean() > (0.02 if gamma else 0.0), (gamma, clipped.mean(), (keep & ~through).mean())
            assert through.mean() > 0.1  # (the planted cases are there)


def test_flat_window_and_gamma_0_clamp_to_this_frame(checker):
    """sd == 0 (a window of one colour) and gamma == 0 both give lo <= cur <= hi with lo = min(mean, cur), hi = max(mean, cur): where the
    window is flat, the clamped value is this frame's own but for the rounding of cur*lerp + cur*one, and the history falls to
    (nearly) one frame"""
    w, h = 40, 12
    rng = np.random.default_rng(3)
    colour = np.zeros((h, w, 4), f32)
    colour[..., :3] = (0.25, 0.5, 0.75)
    acc = colour.copy()
    acc[..., :3] = (2.0, 0.125, 0.75)
    moments, am = luminance_moments(rng, colour, 0.0), luminance_moments(rng, acc, 8.0)
    for gamma in (0.0, 1.0, 100.0):
        oc, om, ov = checker.run(colour, moments, acc, am, radius=2, gamma=gamma)
        assert np.abs(oc[..., :3] - colour[..., :3]).max() <= 2 * EPS
        assert (om[..., 3] >= 1).all() and (om[..., 3] < 1.0001).all()
        assert np.abs(om[..., :2] - moments[..., :2]).max() < 1e-3


def test_a_history_inside_every_bound_comes_back_untouched(checker):
    """(a): an accumulated colour between this frame's value and the window's mean lies inside [L, U] whatever gamma is"""
    w, h = 70, 11
    rng = np.random.default_rng(5)
    colour = (rng.random((h, w, 4), dtype=f32) * f32(2)).astype(f32)
    for radius in (1, 2, 3):
        _, d = rectify_numpy(colour, colour, colour, luminance_moments(rng, colour, 2.0), radius=radius, gamma=0.0, details=True)
        acc = colour.copy()
        acc[..., :3] = (d["L"] + (d["U"] - d["L"]) * rng.random((h, w, 3), dtype=f32)).astype(f32)
        acc[..., :3] = np.clip(acc[..., :3], d["L"], d["U"])  # (inside [L, U] of gamma 0 at N = 2: inside every wider gamma's too)
        am = luminance_moments(rng, acc, 2.0)
        for gamma in (0.0, 1.0):
            oc, om, ov = checker.run(colour, colour, acc, am, radius=radius, gamma=gamma)
            assert oc.tobytes() == acc.tobytes() and om.tobytes() == am.tobytes()
            dd = am[..., 1] - am[..., 0] * am[..., 0]
            assert ov[..., 1].tobytes() == (np.where(dd > 0, dd, f32(0)) / f32(2)).astype(f32).tobytes()


def light_switch(w, h, A, B, N=16.0, seed=9):
    """this frame: the constant B plus a small deterministic pattern; the history: the constant A, blended in at history length N"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    pattern = (((xx * 7 + yy * 13) % 16).astype(f32) / f32(16) - f32(0.5)) * f32(0.02)
    colour = np.zeros((h, w, 4), f32)
    colour[..., :3] = f32(B) + pattern[..., None]
    lerp = (f32(N) - f32(1)) / f32(N)
    acc = colour.copy()
    acc[..., :3] = f32(A) * lerp + colour[..., :3] * (f32(1) - lerp)
    return colour, luminance_moments(rng, colour, 0.0), acc, luminance_moments(rng, acc, N)


@pytest.mark.parametrize("levels", [(0.1, 3.0), (3.0, 0.1)], ids=["on", "off"])
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_light_switch_pulls_the_history_to_this_frame(checker, levels, radius):
    """(b)"""
    w, h = 66, 9
    A, B = levels
    planes = light_switch(w, h, A, B)
    colour, moments, acc, am = planes
    (oc, om, ov), d = rectify_numpy(*planes, radius=radius, gamma=1.0, details=True)
    got = checker.run(*planes, radius=radius, gamma=1.0)
    assert all(g.tobytes() == n.tobytes() for g, n in zip(got, (oc, om, ov)))
    assert (oc[..., :3] >= d["L"]).all() and (oc[..., :3] <= d["U"]).all()
    assert (d["a"] > 0.97).all() and (d["a"] <= 1).all()
    assert (om[..., 3] >= 1).all() and (om[..., 3] < 2).all()
    assert np.abs(oc[..., :3] - f32(B)).max() < 0.05  # (the pattern's range and gamma standard deviations of it)
    assert np.abs(om[..., :2] - moments[..., :2]).max() < 0.05 * max(A, B) ** 2


def test_checker_refuses_what_the_product_refuses(checker):
    planes = synthetic_case(8, 4)
    assert checker.run(*planes, rc=True) == 0
    for kw in (dict(radius=0), dict(radius=4), dict(radius=-1), dict(gamma=-0.5), dict(gamma=float("nan")), dict(gamma=float("inf"))):
        assert checker.run(*planes, rc=True, **kw) == -1, kw
