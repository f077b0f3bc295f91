"""The CPU references of adaptive sampling against what they are built from.  tests/adaptive_checker.c with constant counts n is
tests/moments_checker.c at n spp, byte for byte: tile, moments.xyz, planes and rays, over progressive frames (the sample-weighted lerp
S / (S + n) then rounds to frame / (frame + 1)).  Its plan function against adaptive_lib.plan_numpy, a second statement, on seeded
moments, and on hand-made planes that take each branch."""
import numpy as np
import pytest

from adaptive_lib import LUM_FLOOR, AdaptiveChecker, plan_numpy
from moments_lib import MomentsChecker, random_moments, random_planes
from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return AdaptiveChecker(tmp_path_factory.mktemp("adaptive_checker"))


@pytest.fixture(scope="module")
def mchecker(tmp_path_factory):
    return MomentsChecker(tmp_path_factory.mktemp("moments_checker"))


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("n", [1, 4, 7])
def test_constant_counts_are_the_moments_checker(checker, mchecker, oracle, n, frames):
    w, h = 45, 28
    per, bb, mo, alb, nd = checker.frames(oracle, w, h, np.full((h, w), n, np.int32), frames)
    perm, bbm, mom, albm, ndm = mchecker.frames(oracle, w, h, n, frames)
    assert per == perm
    assert bb.tobytes() == bbm.tobytes()
    assert mo[..., :3].tobytes() == mom[..., :3].tobytes()
    assert (mo[..., 3] == frames * n).all()
    assert alb.tobytes() == albm.tobytes() and nd.tobytes() == ndm.tobytes()


def test_animated_blend_leaves_the_smoothing_out(checker, mchecker, oracle):
    """kFlagAnimate moves the spheres; the sample-weighted lerp does not take the 0.9: frame 0 equals the moments checker's (lerp 0
    both), frame 1 is blended with 4 / 8 exactly"""
    w, h, n, t = 40, 24, 4, 1.7
    flags = FLAG_PROGRESSIVE | FLAG_ANIMATE
    counts = np.full((h, w), n, np.int32)
    _, bb0, mo0, _, _ = checker.frames(oracle, w, h, counts, 1, flags=flags, time=t)
    _, bbm, mom, _, _ = mchecker.frames(oracle, w, h, n, 1, flags=flags, time=t)
    assert bb0.tobytes() == bbm.tobytes() and mo0[..., :3].tobytes() == mom[..., :3].tobytes()
    _, bb1, _, _, _ = checker.frames(oracle, w, h, counts, 2, flags=flags, time=t)
    s, m = oracle.default_scene()
    s = s.copy()
    oracle.animate(s, t)
    _, own, _, _, _ = checker.render(s, m, oracle.default_camera(w, h), w, h, counts, 1, 0)
    half = np.float32(0.5)
    assert bb1[..., :3].tobytes() == (bb0[..., :3] * half + own[..., :3] * (np.float32(1) - half)).tobytes()


def test_zero_counts_leave_the_pixel_alone_and_the_clamp_holds(checker, oracle):
    w, h = 33, 20
    rng = np.random.default_rng(11)
    counts = rng.choice(np.int32([0, 0, 1, 2, 5]), size=(h, w)).astype(np.int32)
    counts[3, 4], counts[7, 9] = -3, 5000
    s, m = oracle.default_scene()
    cam = oracle.default_camera(w, h)
    bb, mo, alb, nd = (np.full((h, w, 4), v, np.float32) for v in (7.25, -1.5, 3.0, 11.0))
    mo[..., 3] = 2.0
    rays, _, _, _, _ = checker.render(s, m, cam, w, h, counts, 2, FLAG_PROGRESSIVE, backbuffer=bb, moments=mo, albedo=alb, normal_depth=nd)
    zero = counts <= 0
    assert zero.sum() > 100
    assert (bb[zero] == 7.25).all() and (alb[zero] == 3.0).all() and (nd[zero] == 11.0).all()
    assert (mo[zero][:, :3] == -1.5).all() and (mo[zero][:, 3] == 2.0).all()
    assert (bb[~zero][:, 3] == 7.25).all() and not (bb[~zero][:, :3] == 7.25).all(axis=1).any()
    assert mo[7, 9, 3] == 2.0 + 2047 and (mo[~zero][:, 3] == 2.0 + np.clip(counts[~zero], 0, 2047)).all()
    # the rays are those of the traced pixels alone: the same plane with the zeros turned into ones traces more
    more, _, _, _, _ = checker.render(s, m, cam, w, h, np.where(zero, 1, counts), 2, FLAG_PROGRESSIVE)
    assert 0 < rays < more
    # without the progressive flag the count starts over: S = 0 whatever .w held
    mo2 = np.full((h, w, 4), 9.0, np.float32)
    checker.render(s, m, cam, w, h, counts, 2, 0, moments=mo2)
    assert (mo2[~zero][:, 3] == np.clip(counts[~zero], 0, 2047)).all()


def seeded_moments(rng, h, w, kind):
    colour, _, _ = random_planes(rng, h, w)
    mo = random_moments(rng, colour, 1.0)
    if kind == "valid":
        mo[..., 3] = rng.integers(1, 200, (h, w)).astype(np.float32)
    elif kind == "invalid":
        mo[..., 3] = rng.choice(np.float32([0.0, 0.5, -4.0, np.nan, np.inf, -np.inf]), size=(h, w))
    else:
        mo[..., 3] = rng.choice(np.float32([0.0, 0.999, 1.0, 4.0, 8.0, 64.0, 3e38, np.nan, np.inf]), size=(h, w))
    return np.ascontiguousarray(mo)


@pytest.mark.parametrize("size", [(1, 1), (1, 17), (37, 21), (64, 40)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", ["valid", "invalid", "mixed"])
@pytest.mark.parametrize("te,lo,hi", [(0.05, 0, 64), (0.2, 1, 16), (0.01, 4, 2047), (1e-30, 0, 9), (1e6, 3, 3)])
def test_plan_c_and_numpy_agree(checker, size, kind, te, lo, hi):
    w, h = size
    mo = seeded_moments(np.random.default_rng(w * 100 + h + len(kind)), h, w, kind)
    counts, var, total = checker.plan(mo, te, lo, hi)
    nc, nv, nt = plan_numpy(mo, te, lo, hi)
    assert counts.tobytes() == nc.tobytes()
    assert var.tobytes() == nv.tobytes()
    assert total == nt == int(counts.astype(np.int64).sum())
    assert counts.min() >= min(lo, 1) and counts.max() <= max(hi, 1)
    if kind == "invalid":
        assert (counts == max(lo, 1)).all() and (var == 0).all()


def flat(h, w, mean, second, S):
    mo = np.zeros((h, w, 4), np.float32)
    mo[...] = (mean, second, 0.0, S)
    return mo


def test_plan_branches_by_hand(checker):
    f32 = np.float32
    h, w = 5, 6
    te = 0.125  # te^2 = 1/64, exact
    # a flat valid plane: R = r exactly (the weights are dyadic and sum exactly), need = r * 64, extra = need - S
    mean, var, S = f32(0.99), f32(0.5), f32(4.0)
    second = f32(mean * mean + var)
    mo = flat(h, w, mean, second, S)
    d = f32(second - mean * mean)
    b = f32(mean + LUM_FLOOR)
    r = f32(d / f32(b * b))
    extra = f32(f32(r * f32(64.0)) - S)
    assert 9 < extra < 60
    counts, out, total = checker.plan(mo, te, 1, 2047)
    assert (counts == int(np.ceil(extra))).all() and total == h * w * int(np.ceil(extra))
    assert (out[..., 1] == f32(d / S)).all() and (out[..., 3] == S).all() and (out[..., 0] == 0).all() and (out[..., 2] == 0).all()
    # extra >= max: max; extra <= min: min (also min = 0)
    assert (checker.plan(mo, te, 1, 9)[0] == 9).all()
    assert (checker.plan(mo, te, 60, 100)[0] == 60).all()
    assert (checker.plan(flat(h, w, mean, second, f32(1000.0)), te, 0, 64)[0] == 0).all()
    # an invalid pixel among valid ones: max(min, 1) there and {0, 0, 0, 0}; its neighbours skip it and keep R = r
    mo2 = mo.copy()
    mo2[2, 3, 3] = 0.0
    c2, o2, _ = checker.plan(mo2, te, 0, 2047)
    assert c2[2, 3] == 1 and (o2[2, 3] == 0).all()
    assert (np.delete(c2.ravel(), 2 * w + 3) == int(np.ceil(extra))).all()
    assert checker.plan(mo2, te, 5, 2047)[0][2, 3] == 5
    # no valid pixel anywhere
    c3, o3, t3 = checker.plan(flat(h, w, mean, second, f32(0.5)), te, 0, 64)
    assert (c3 == 1).all() and (o3 == 0).all() and t3 == h * w
    # NaN moments under a valid count: NaN lands on min, at the pixel and at the neighbours whose R it poisons
    mo4 = mo.copy()
    mo4[2, 3, 0] = np.nan
    c4, o4, _ = checker.plan(mo4, te, 2, 2047)
    assert (c4[1:4, 2:5] == 2).all() and c4[0, 0] == int(np.ceil(extra)) and o4[2, 3, 3] == S
    # a neighbourhood guards the pixel whose samples happened to agree: variance 0 at one pixel, its count still well above min
    mo5 = mo.copy()
    mo5[2, 3, 1] = mean * mean
    c5, o5, _ = checker.plan(mo5, te, 1, 2047)
    assert o5[2, 3, 1] == 0 and c5[2, 3] > 1
    n5, v5, _ = plan_numpy(mo5, te, 1, 2047)
    assert c5.tobytes() == n5.tobytes() and o5.tobytes() == v5.tobytes()


def test_plan_checker_refuses_what_the_product_refuses(checker):
    mo = flat(3, 3, 0.5, 0.5, 4.0)
    for te, lo, hi in ((0.0, 0, 4), (-1.0, 0, 4), (float("nan"), 0, 4), (float("inf"), 0, 4), (2e6, 0, 4), (0.1, -1, 4), (0.1, 0, 2048),
                       (0.1, 5, 4)):
        with pytest.raises(AssertionError):
            checker.plan(mo, te, lo, hi)
