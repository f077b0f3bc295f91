"""tptTemporalAccumulateDevice without a GPU: its two CPU statements -- tests/temporal_checker.c and temporal_lib.temporal_numpy -- agree
byte for byte on seeded planes and cameras, and the statement has the properties include/tpt_hip.h promises: an unmoved camera with
agreeing guides reproduces the progressive tile, a camera shifted by whole pixels fetches whole pixels, a step in depth, normal or
coverage cuts the history, and the variance plane is what tptDenoiseDeviceVariance expects."""
import numpy as np
import pytest

from oracle_lib import FLAG_PROGRESSIVE
from temporal_lib import KINDS, TemporalChecker, axis_camera, plane_frame, random_frame, synthetic_case, temporal_numpy

f32 = np.float32
NAMES = ("colour", "albedo", "moments", "variance")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return TemporalChecker(tmp_path_factory.mktemp("temporal_checker"))


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("size", [(1, 1), (17, 1), (1, 17), (8192, 2), (130, 67)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_checker_and_numpy_agree(checker, kind, size):
    w, h = size
    cam, cur, prev = synthetic_case(kind, w, h)
    for kw in (dict(max_history=8.0), dict(max_history=2.5, depth_tolerance=0.5, normal_tolerance=1.0, coverage_tolerance=0.25)):
        got, want = checker.run(cam, cur, prev, **kw), temporal_numpy(cam, cur, prev, **kw)
        for name, g, n in zip(NAMES, got, want):
            assert g.tobytes() == n.tobytes(), (name, kw)
        N = got[2][..., 3]
        assert (N >= 1).all() and (N <= kw["max_history"]).all()
        assert (got[3][..., 0] == 0).all() and (got[3][..., 1] >= 0).all() and (got[3][..., 3] == N).all()
        assert (got[0][..., 3] == cur[0][..., 3]).all()  # (the colour's alpha)
        if kind in ("first", "behind"):
            assert (N == 1).all()
        elif size == (130, 67) and kind != "outside":
            assert (N > 1).mean() > 0.4  # (the planted history is found ...)
        if kind == "same" and size == (130, 67):
            bad = ~(prev[4][..., 3] >= 1) | ~np.isfinite(prev[4][..., 3]) | ~np.isfinite(prev[1][..., :3]).all(axis=-1)
            assert bad.any() and (N[bad] == 1).all()  # (... and what was planted in it is not)
            assert (N[~bad] > 1).all()


def unhistoried(cur):
    """the outputs of a pixel without history: this frame's values, N = 1"""
    colour, albedo, _, mo = cur
    one, zero = np.ones(mo.shape[:2], f32), np.zeros(mo.shape[:2], f32)
    dd = mo[..., 1] - mo[..., 0] * mo[..., 0]
    return (colour, albedo, np.stack([mo[..., 0], mo[..., 1], zero, one], axis=-1),
            np.stack([zero, np.where(dd > 0, dd, f32(0)), zero, one], axis=-1))


def test_first_frame_and_max_history_1_return_this_frame(checker):
    w, h = 40, 24
    cam, cur, prev = synthetic_case("same", w, h)
    want = unhistoried(cur)
    assert same(checker.run(cam, cur, None), want)
    finite = tuple(np.nan_to_num(p, nan=1.0, posinf=2.0, neginf=3.0) for p in prev[1:])  # (inf * 0 would be NaN: garbage in)
    assert same(checker.run(cam, cur, (prev[0],) + finite, max_history=1.0), want)


def test_unmoved_camera_is_the_progressive_tile(checker, oracle):
    """identical cameras, agreeing guides: N = N' + 1 exactly, and the colour is the oracle's progressive blend of the same two
    planes (tpto_render's lerp: frame N' of a progressive sequence)"""
    w, h = 48, 32
    rng = np.random.default_rng(5)
    cam = oracle.default_camera(w, h)
    spheres, mats = oracle.default_scene()
    frames = []
    for f in range(3):
        r, bb = oracle.render(spheres, mats, cam, w, h, 4, f, flags=0)
        frames.append(bb)
    guides = random_frame(rng, h, w)
    prev = None
    tile = np.zeros((h, w, 4), f32)
    for f in range(3):
        oracle.render(spheres, mats, cam, w, h, 4, f, flags=FLAG_PROGRESSIVE, backbuffer=tile)
        cur = (frames[f], guides[1], guides[2], guides[3])
        out = checker.run(cam, cur, prev, max_history=64.0)
        assert (out[2][..., 3] == f + 1).all()
        assert out[0][..., :3].tobytes() == tile[..., :3].tobytes(), "frame %d" % f
        assert same(out, temporal_numpy(cam, cur, prev, max_history=64.0))
        prev = (cam, out[0], out[1], guides[2], out[2])


@pytest.mark.parametrize("k", [1, 3, -2])
def test_whole_pixel_shift_fetches_one_tap(checker, k):
    """a camera translated parallel to a fronto-parallel plane by exactly k pixel widths (of the plane's depth) fetches the pixel k
    columns away with its whole weight"""
    w, h, depth = 32, 16, 4.0
    rng = np.random.default_rng(7)
    pixel = 1.0 / 64  # at distance 1: a pixel of the plane at depth 4 is 1/16 wide
    prev_cam, cam = axis_camera(w, h, 0.0, pixel), axis_camera(w, h, k * pixel * depth, pixel)
    cur = plane_frame(rng, h, w, cam, depth)
    pcol, palb, pnd, pmo = plane_frame(rng, h, w, prev_cam, depth, history=2)
    out = checker.run(cam, cur, (prev_cam, pcol, palb, pnd, pmo), max_history=64.0, depth_tolerance=0.01, normal_tolerance=0.01)
    assert same(out, temporal_numpy(cam, cur, (prev_cam, pcol, palb, pnd, pmo), max_history=64.0, depth_tolerance=0.01, normal_tolerance=0.01))
    N = out[2][..., 3]
    xs = np.arange(w) + k  # pixel x of this frame shows what pixel x + k of the previous frame showed
    inside = (xs >= 0) & (xs < w)
    assert (N[:, inside] == 3).all() and (N[:, ~inside] == 1).all()
    lerp = f32(2) / f32(3)
    want = pcol[:, xs[inside], :3] * lerp + cur[0][:, inside, :3] * (f32(1) - lerp)
    assert out[0][:, inside, :3].tobytes() == np.ascontiguousarray(want.astype(f32)).tobytes()


@pytest.mark.parametrize("what", ["depth", "normal", "coverage", "sky-to-surface"])
def test_a_step_in_the_guides_cuts_the_history(checker, what):
    w, h, depth = 32, 16, 4.0
    rng = np.random.default_rng(11)
    cam = axis_camera(w, h)
    cur = plane_frame(rng, h, w, cam, depth)
    pcol, palb, pnd, pmo = plane_frame(rng, h, w, cam, depth, history=5)
    cut = np.zeros((h, w), bool)
    cut[3:9, 5:20] = True
    if what == "depth":
        pnd[cut, 3] *= f32(1.25)
    elif what == "normal":
        pnd[cut, 0:3] = (0.0, 1.0, 0.0)
    elif what == "coverage":
        for p in (palb, pnd):
            p[cut] *= f32(0.75)  # (the same surface, three samples of four on it)
    else:
        palb[cut] = 0
        pnd[cut] = 0
    out = checker.run(cam, cur, (cam, pcol, palb, pnd, pmo), max_history=64.0)
    assert same(out, temporal_numpy(cam, cur, (cam, pcol, palb, pnd, pmo), max_history=64.0))
    N = out[2][..., 3]
    assert (N[cut] == 1).all() and (N[~cut] == 6).all()
    for got, want in zip(out, unhistoried(cur)):
        assert got[cut].tobytes() == want[cut].tobytes()
    if what == "coverage":  # within the tolerance the history is kept
        loose = checker.run(cam, cur, (cam, pcol, palb, pnd, pmo), max_history=64.0, coverage_tolerance=0.25)
        assert (loose[2][..., 3] == 6).all()


def test_checker_refuses_what_the_product_refuses(checker):
    w, h = 8, 4
    cam, cur, prev = synthetic_case("same", w, h)
    assert checker.run(cam, cur, prev, rc=True) == 0
    for kw in (dict(max_history=0.5), dict(max_history=65537.0), dict(max_history=float("nan")), dict(depth_tolerance=-1.0),
               dict(normal_tolerance=float("inf")), dict(coverage_tolerance=float("nan"))):
        assert checker.run(cam, cur, prev, rc=True, **kw) == -1, kw
    for k, v in ((0, np.nan), (7, np.inf), (21, np.nan)):
        bad = cam.copy()
        bad[k] = v
        assert checker.run(bad, cur, prev, rc=True) == -1 and checker.run(cam, cur, (bad,) + prev[1:], rc=True) == -1
    flat, behind = cam.copy(), cam.copy()
    flat[6:9] = 0  # dot(H, H) == 0
    behind[18:21] = -behind[18:21]  # the frame behind the origin: f <= 0
    for bad in (flat, behind):
        assert checker.run(bad, cur, None, rc=True) == -1 and checker.run(cam, cur, (bad,) + prev[1:], rc=True) == -1
