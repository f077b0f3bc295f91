"""tests/lens_checker.c, the CPU reference of tptDrawDeviceLens, held against what it is made of: its rays against the projections'
formulas in float64, the exact cases (the image centre, r == 0, parallel orthographic rays), and its render at 1 spp against
tests/rays_checker.c on the rays it says the first samples start with.  No GPU."""
import numpy as np
import pytest

from lens_lib import EQUIRECT, FISHEYE, FOLD_FORWARD, FOLD_RECURSIVE, KINDS, ORTHO, PI, TWO_PI, LensChecker, default_scene, make_lens
from rays_lib import RaysChecker

ULP1 = 2.0 ** -23  # a binary32 ulp of 1


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return LensChecker(tmp_path_factory.mktemp("lens_checker"))


@pytest.fixture(scope="module")
def rays_checker(tmp_path_factory):
    return RaysChecker(tmp_path_factory.mktemp("lens_rays_checker"))


def uv_grid(n=41):
    t = np.concatenate([np.linspace(0.0, 1.0, n, dtype=np.float32)[:-1], np.float32([np.nextafter(np.float32(1), np.float32(0)), 0.5])])
    return np.stack(np.meshgrid(t, t), -1).reshape(-1, 2)


def formula64(lens, uv):
    """the three projections in float64.  a, b and the arguments of sin / cos are the CONTRACT's binary32 values -- the statement defines
    them as such, so their rounding is not an error of the ray -- and everything behind them is float64: what is left to differ is the
    checker's sin / cos (under an ulp each), its products and sums of terms no larger than 1, and normalize."""
    u, v = uv[:, 0].astype(np.float32), uv[:, 1].astype(np.float32)
    a32, b32 = (u - np.float32(0.5)) * np.float32(lens.sx), (v - np.float32(0.5)) * np.float32(lens.sy)
    a, b = a32.astype(np.float64), b32.astype(np.float64)
    o, r, up, f = (np.array(x[:], np.float64) for x in (lens.origin, lens.right, lens.up, lens.forward))
    orig = np.broadcast_to(o, (len(uv), 3)).copy()
    if lens.kind == EQUIRECT:
        q = r * (np.cos(b) * np.sin(a))[:, None] + up * np.sin(b)[:, None] + f * (np.cos(b) * np.cos(a))[:, None]
    elif lens.kind == FISHEYE:
        r32 = np.sqrt(a32 * a32 + b32 * b32)
        th = (r32 * np.float32(lens.maxAngle)).astype(np.float64)
        rr = np.hypot(a, b)
        k = np.divide(np.sin(th), rr, out=np.zeros_like(rr), where=rr > 0)
        q = r * (a * k)[:, None] + up * (b * k)[:, None] + f * np.cos(th)[:, None]
    else:
        q = np.broadcast_to(f, (len(uv), 3)).copy()
        orig = o + r * a[:, None] + up * b[:, None]
    return orig, q / np.linalg.norm(q, axis=1, keepdims=True)


LENSES = {
    "equirect-full": dict(kind=EQUIRECT),
    "equirect-tilted": dict(kind=EQUIRECT, forward=(0.3, -0.5, -0.8), up=(0.1, 1.0, 0.2), sx=2.0, sy=1.0),
    "equirect-tiny": dict(kind=EQUIRECT, sx=1e-3, sy=1e-3),
    "fisheye-180": dict(kind=FISHEYE),
    "fisheye-largest": dict(kind=FISHEYE, sx=4.0, sy=4.0, max_angle=PI, forward=(0.3, -0.5, -0.8)),
    "fisheye-tiny": dict(kind=FISHEYE, sx=1e-3, sy=1e-3, max_angle=0.01),
    "ortho": dict(kind=ORTHO, forward=(0.3, -0.5, -0.8)),
}


@pytest.mark.parametrize("name", sorted(LENSES))
def test_rays_are_the_formulas(checker, name):
    lens = make_lens(**LENSES[name])
    uv = uv_grid()
    got = checker.ray_grid(lens, uv)
    orig, d = formula64(lens, uv)
    assert np.isfinite(got).all()
    err = np.abs(got[:, 3:6].astype(np.float64) - d).max()
    print("%s: largest direction error %.3g ulps of 1" % (name, err / ULP1))
    assert err <= 4 * ULP1
    # the origin: exact for the lenses that look from a point, two roundings of terms up to sx / 2, sy / 2 for the window
    if lens.kind == ORTHO:
        assert np.abs(got[:, 0:3].astype(np.float64) - orig).max() <= 4 * ULP1 * max(lens.sx, lens.sy)
    else:
        assert (got[:, 0:3] == np.float32(lens.origin[:])).all()
    # unit length to the rounding of normalize
    assert np.abs(np.linalg.norm(got[:, 3:6].astype(np.float64), axis=1) - 1).max() <= 4 * ULP1


AXES = [((0, 0, -1), (0, 1, 0)), ((1, 0, 0), (0, 0, 1)), ((0, -1, 0), (1, 0, 0)), ((0, 0, 1), (0, -1, 0))]


@pytest.mark.parametrize("forward,up", AXES)
def test_the_image_centre_of_an_equirect_is_forward_exactly(checker, forward, up):
    for sx, sy in ((TWO_PI, PI), (1.0, 0.5), (1e-3, 1e-3)):
        lens = make_lens(EQUIRECT, forward=forward, up=up, sx=sx, sy=sy)
        got = checker.ray(lens, 0.5, 0.5)
        assert got[3:6].tobytes() == np.float32(forward).tobytes() and got[0:3].tobytes() == np.float32(lens.origin[:]).tobytes()


def normalised32(v):
    """the oracle's normalize of a binary32 vector: v * (1.0f / sqrtf(dot(v, v))), sums left to right"""
    v = np.float32(v)
    dd = np.float32(np.float32(np.float32(v[0] * v[0]) + np.float32(v[1] * v[1])) + np.float32(v[2] * v[2]))
    return v * (np.float32(1) / np.sqrt(dd))


def test_a_fisheye_at_r_0_is_forward_and_no_nan(checker):
    for forward, up in AXES + [((0.3, -0.5, -0.8), (0.1, 1.0, 0.2))]:
        for max_angle in (PI, 1.0, 1e-3):
            lens = make_lens(FISHEYE, forward=forward, up=up, max_angle=max_angle)
            got = checker.ray(lens, 0.5, 0.5)
            assert np.isfinite(got).all()
            # (k = 0 at r == 0: q = right * 0 + up * 0 + forward * cos(0) = forward, then the reference's normalize)
            assert got[3:6].tobytes() == normalised32(lens.forward[:]).tobytes(), (forward, max_angle, got)
    lens = make_lens(FISHEYE, forward=(0, 0, -1), up=(0, 1, 0))
    assert checker.ray(lens, 0.5, 0.5)[3:6].tobytes() == np.float32([0, 0, -1]).tobytes()


def test_ortho_directions_are_all_equal(checker):
    lens = make_lens(ORTHO, forward=(0.3, -0.5, -0.8), up=(0.1, 1.0, 0.2))
    uv = np.unique(uv_grid(17), axis=0)
    got = checker.ray_grid(lens, uv)
    assert (got[:, 3:6] == got[0, 3:6]).all() and got[0, 3:6].tobytes() == normalised32(lens.forward[:]).tobytes()
    assert len(np.unique(got[:, 0:3], axis=0)) == len(uv)  # ... and every origin its own


@pytest.mark.parametrize("fold", [FOLD_RECURSIVE, FOLD_FORWARD], ids=["recursive", "forward"])
@pytest.mark.parametrize("frame", [0, 3])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_one_sample_is_the_ray_checker_on_the_lens_rays(checker, rays_checker, kind, frame, fold):
    W, H = 37, 19
    s, m = default_scene()
    lens = make_lens(KINDS[kind])
    rays = checker.rays(lens, W, H, frame)
    assert np.isfinite(rays[:, [0, 1, 2, 4, 5, 6]]).all() and (rays[:, 3].view(np.uint32) != 0).all() and (rays[:, 7] == 0).all()
    total, rad, _ = rays_checker.trace(s, m, rays, hits=False, fold=fold)
    want_rays, bb = checker.render(s, m, lens, W, H, 1, frame, fold=fold)
    # (a zeroed buffer and lerp 0: the pixel is prev * 0 + col * 1, the bytes of 0.0f + col)
    assert rad.reshape(H, W, 4)[..., :3].tobytes() == bb[..., :3].tobytes() and (bb[..., 3] == 0).all()
    assert total == want_rays and int(rad[:, 3].astype(np.int64).sum()) == want_rays
    assert (bb[..., :3] > 0).any()


def test_samples_come_in_sequence_from_one_stream_and_are_blended(checker):
    """spp samples are not spp one-sample frames: the stream runs on; and the progressive blend reads the tile"""
    W, H = 24, 16
    s, m = default_scene()
    lens = make_lens(FISHEYE)
    r1, one = checker.render(s, m, lens, W, H, 1, 2)
    r3, three = checker.render(s, m, lens, W, H, 3, 2)
    assert r3 > 2 * r1 and one.tobytes() != three.tobytes()
    tile = np.full((H, W, 4), 0.5, np.float32)
    _, blended = checker.render(s, m, lens, W, H, 3, 2, flags=2, backbuffer=tile.copy())
    lerp = np.float32(2) / np.float32(3)
    want = tile[..., :3] * lerp + three[..., :3] * (np.float32(1) - lerp)
    assert blended[..., :3].tobytes() == want.astype(np.float32).tobytes() and (blended[..., 3] == 0.5).all()
