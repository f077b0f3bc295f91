"""The CPU reference of tptDrawDeviceAov's planes (tests/aov_checker.c) against the oracle it is built from: its colour and ray count
are tpto_render's, byte for byte, in every configuration the GPU tests use; its planes have the shape the definition gives them."""
import numpy as np
import pytest

from aov_lib import AovChecker
from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE, SEED_PER_PIXEL, SEED_ROW_SERIAL


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return AovChecker(tmp_path_factory.mktemp("aov_checker"))


def mitsuba_cam(oracle, w, h):
    return oracle.camera((0, 2, 3), (0, 0, 0), (0, 1, 0), 60.0, w / h, 0.0, 3.0)  # (aperture 0, Test.cpp:312-313)


CASES = {
    "spp1": dict(spp=1),
    "spp4": dict(spp=4),
    "mitsuba": dict(spp=4, mitsuba_compare=True),
    "no_light_sampling": dict(spp=2, light_sampling=False),
    "row_serial": dict(spp=2, seed_mode=SEED_ROW_SERIAL),
}


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_colour_and_rays_are_the_oracles(checker, oracle, case):
    kw = dict(CASES[case])
    spp = kw.pop("spp")
    w, h = 61, 37
    s, m = oracle.default_scene()
    cam = mitsuba_cam(oracle, w, h) if kw.get("mitsuba_compare") else oracle.default_camera(w, h)
    kw.setdefault("seed_mode", SEED_PER_PIXEL)
    rays, bb, alb, nd = checker.render(s, m, cam, w, h, spp, 0, FLAG_PROGRESSIVE, **kw)
    ro, bo = oracle.render(s, m, cam, w, h, spp, 0, FLAG_PROGRESSIVE, **kw)
    assert rays == ro
    assert bb.tobytes() == bo.tobytes()
    assert np.isfinite(alb).all() and np.isfinite(nd).all()


def test_progressive_frames_zero_to_three(checker, oracle):
    w, h, spp = 48, 30, 2
    s, m = oracle.default_scene()
    cam = oracle.default_camera(w, h)
    bb = np.zeros((h, w, 4), np.float32)
    bo = np.zeros((h, w, 4), np.float32)
    for f in range(4):
        rays, _, alb, nd = checker.render(s, m, cam, w, h, spp, f, FLAG_PROGRESSIVE, backbuffer=bb)
        ro, _ = oracle.render(s, m, cam, w, h, spp, f, FLAG_PROGRESSIVE, backbuffer=bo, seed_mode=SEED_PER_PIXEL)
        assert rays == ro, f
        assert bb.tobytes() == bo.tobytes(), f
    # the planes are overwritten, not blended: frame 3's planes are frame 3's alone
    _, _, alb3, nd3 = checker.render(s, m, cam, w, h, spp, 3, FLAG_PROGRESSIVE)
    assert alb.tobytes() == alb3.tobytes() and nd.tobytes() == nd3.tobytes()


def test_animated_time(checker, oracle):
    w, h, spp, t = 50, 32, 2, 1.7
    flags = FLAG_PROGRESSIVE | FLAG_ANIMATE
    per, bb, _, nd = checker.frames(oracle, w, h, spp, 2, flags=flags, time=t)
    from common import oracle_frames
    ro, bo, pero = oracle_frames(oracle, w, h, spp, 2, flags=flags, time=t, seed_mode=SEED_PER_PIXEL)
    assert per == pero and bb.tobytes() == bo.tobytes()
    # ... and the planes see the moved spheres: differ from the static scene's somewhere
    _, _, _, nd0 = checker.frames(oracle, w, h, spp, 1)
    assert nd.tobytes() != nd0.tobytes()


@pytest.mark.parametrize("spp", [1, 3, 4, 7])
def test_coverage_is_a_multiple_of_one_over_spp(checker, oracle, spp):
    w, h = 64, 40
    s, m = oracle.default_scene()
    # looking up at the sky from the ground's edge: a frame with misses, hits and pixels with both
    cam = oracle.camera((0, 1.0, 3), (0, 2.5, 0), (0, 1, 0), 90.0, w / h, 0.1, 3.0)
    _, _, alb, nd = checker.render(s, m, cam, w, h, spp, 0)
    cov = alb[..., 3]
    inv = np.float32(1.0) / np.float32(spp)
    allowed = np.array([np.float32(k) * inv for k in range(spp + 1)], np.float32)
    assert np.isin(cov, allowed).all()
    assert (cov == 0).any() and (cov == allowed[-1]).any()
    # a pixel no sample hit has all-zero planes
    none = cov == 0
    assert (alb[none] == 0).all() and (nd[none] == 0).all()
    assert (nd[..., 3][~none] > 0).all()


def test_unit_normals_at_one_sample(checker, oracle):
    w, h = 80, 45
    s, m = oracle.default_scene()
    cam = oracle.camera((0, 1.0, 3), (0, 2.5, 0), (0, 1, 0), 90.0, w / h, 0.1, 3.0)
    _, _, alb, nd = checker.render(s, m, cam, w, h, 1, 0)
    hit = alb[..., 3] == 1.0
    assert hit.any() and (~hit).any()
    # (pos - centre) * invRadius in float: the hit position carries the rounding of t (nb - sqrt(nb^2 - c), which cancels), so a
    # third to a half of the default scene's hits are off unit length by more than 1e-6 -- up to 6e-5, in the reference's own arithmetic
    n = nd[..., :3][hit].astype(np.float64)
    err = np.abs(np.linalg.norm(n, axis=1) - 1.0)
    assert err.max() <= 1e-4, err.max()
    assert (err <= 1e-6).mean() >= 0.25, (err <= 1e-6).mean()
    # ... and the albedo is a material's albedo as the scene holds it
    albedos = {tuple(a) for a in m["albedo"].astype(np.float32).tolist()}
    assert {tuple(a) for a in alb[..., :3][hit].tolist()} <= albedos
