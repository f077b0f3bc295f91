"""tptMotionVectorsDevice without a GPU: its CPU statements -- tests/flow_checker.c and flow_lib's numpy twin -- agree byte for byte on
seeded clips that reach every branch, and the statement has the properties include/tpt_hip.h promises: a camera and a scene that stand
still give mv = {0, 0} and W = 1 exactly, a whole-pixel shift gives that integer, a pixel that does not project gives four zeros, a
step in depth gives W = 0 with mv still reported, and W stays within [0, 1]."""
import numpy as np
import pytest

from flow_lib import FORMS, KINDS, N_IDS, TOLERANCES, FlowChecker, flow_numpy, synthetic_clip
from temporal_lib import axis_camera, look_at_camera, plane_frame, random_frame

f32 = np.float32
SIZES = [(1, 1), (17, 1), (1, 17), (65, 5), (130, 67)]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return FlowChecker(tmp_path_factory.mktemp("flow_checker"))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_checker_and_numpy_agree(checker, kind, size):
    w, h = size
    clip = synthetic_clip(kind, w, h)
    assert clip["objects"].max() == N_IDS - 1 or w * h < 40  # (ids outside the table's 0 .. N_IDS - 3)
    for tol in (TOLERANCES, dict(depth_tolerance=0.0, normal_tolerance=0.0, coverage_tolerance=0.0),
                dict(depth_tolerance=0.5, normal_tolerance=1.0, coverage_tolerance=0.5)):
        for form in FORMS:
            for prev in (True, False):
                got = checker.run(clip, prev=prev, **form, **tol)
                want = flow_numpy(clip, prev=prev, **form, **tol)
                for j in range(3):
                    assert got[j].tobytes() == want[j].tobytes(), (j, form, prev, tol)
                W = got[..., 3]
                assert ((W >= 0) & (W <= 1)).all(), "W outside [0, 1] (or no number)"
                assert not np.isnan(got[..., :2]).any()
                if not prev:
                    assert not got[0].any() and got[0].tobytes() == bytes(got[0].nbytes), "a frame without a predecessor is not +0"
                # a pixel that does not project is four zeros: e > 0 wherever anything is reported
                silent = got[..., 2] == 0
                assert not got[silent].any()


def test_every_branch_is_reached(checker):
    """the synthetic clips are worth their name: at 130 x 67 they hold pixels that project and pixels that do not, taps that count and
    taps refused by each test, snapped and fractional positions, and points outside the previous image"""
    w, h = 130, 67
    out = {k: checker.run(synthetic_clip(k, w, h), **FORMS[2], **TOLERANCES) for k in KINDS}
    plain = {k: checker.run(synthetic_clip(k, w, h), **FORMS[0], **TOLERANCES) for k in KINDS}
    # (the plain form: a table moves the few points that an infinite coverage puts into the lens itself)
    assert not plain["away"][0].any(), "a previous camera that looks the other way: nothing projects"
    turned = out["away"][1]  # a previous camera at a right angle: some points behind it, most of the others outside its image
    px = turned[..., 0] + np.arange(w, dtype=f32)[None, :]
    outside = (turned[..., 2] > 0) & ((px < -1) | (px >= w))
    assert (turned[..., 2] == 0).any() and outside.any() and not turned[..., 3][outside].any()
    same = plain["same"][1:]  # (no table: nothing moves)
    assert ((same[..., 3] == 1).mean() > 0.2) and (same[..., 3] == 0).any() and (same[..., :2] == 0).all()
    moved = out["moved"]
    frac = moved[..., 3]
    assert ((frac > 0) & (frac < 1)).any() and (moved[..., 0] != np.round(moved[..., 0])).any()
    for k in KINDS:  # the id test and the table change bytes
        assert out[k].tobytes() != plain[k].tobytes(), k
        assert checker.run(synthetic_clip(k, w, h), **FORMS[1], **TOLERANCES).tobytes() != out[k].tobytes(), k
    # the pixel clip: frame 0 is 2 pixels from its predecessor, frame 1 a 256th of a pixel from frame 0 (snapped), frame 2 1.25 pixels
    # less a 256th from frame 1 (not snapped) -- wherever no step in depth is planted, which moves the point along its ray
    pix = plain["pixel"]
    assert (pix[0][..., 0] == 2).mean() > 0.5 and (pix[1][..., 0] == 0).mean() > 0.5 and (pix[..., 1] == 0).mean() > 0.5
    assert abs(np.median(pix[2][..., 0]) - (1.25 - 1.0 / 256)) < 1e-4
    # each tolerance decides somewhere: tightening one of them alone changes W
    clip = synthetic_clip("same", w, h)
    base = checker.run(clip, **FORMS[0], **TOLERANCES)
    for name in TOLERANCES:
        tight = checker.run(clip, **FORMS[0], **dict(TOLERANCES, **{name: TOLERANCES[name] * 0.5}))
        assert (tight[..., 3] < base[..., 3]).any() and (tight[..., 3] <= base[..., 3]).all(), name
        assert tight[..., :3].tobytes() == base[..., :3].tobytes(), name


def clean_clip(w, h, cams, frames, prev=None):
    n = len(cams)
    return dict(cameras=np.ascontiguousarray(np.stack(cams).astype(f32)), albedo=np.ascontiguousarray(np.stack([f[1] for f in frames])),
                nd=np.ascontiguousarray(np.stack([f[2] for f in frames])), objects=np.zeros((n, h, w), np.int32),
                motion=np.zeros((n, 1, 4), f32), prev=prev)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_nothing_moves_gives_zero_motion_and_full_weight(checker, size):
    w, h = size
    cam = look_at_camera([0.0, 2.0, 3.0], [0.0, 0.0, 0.0], w, h)
    frame = random_frame(np.random.default_rng([3, w, h]), h, w)
    clip = clean_clip(w, h, [cam, cam], [frame, frame])
    for form in FORMS:
        out = checker.run(clip, prev=False, **form)
        assert not out[0].any()
        assert (out[1][..., :2] == 0).all() and (out[1][..., 3] == 1).all(), form
        assert (out[1][..., 2] > 0).all()


@pytest.mark.parametrize("shift", [1, 2, -3])
def test_a_whole_pixel_shift_gives_that_integer(checker, shift):
    w, h = 65, 5
    rng = np.random.default_rng([4, shift + 8])
    cams = [axis_camera(w, h, 0.0), axis_camera(w, h, shift / 64.0)]
    clip = clean_clip(w, h, cams, [plane_frame(rng, h, w, c, depth_z=1.0) for c in cams])
    out = checker.run(clip, prev=False, **FORMS[0])[1]
    assert (out[..., 0] == shift).all() and (out[..., 1] == 0).all()
    x = np.arange(w)[None, :] + shift
    inside = np.broadcast_to((x >= 0) & (x < w), (h, w))
    assert (out[..., 3][inside] == 1).all() and (out[..., 3][~inside] == 0).all()
    assert (out[..., 2] >= 1).all()


def test_a_pixel_that_does_not_project_gives_four_zeros(checker):
    w, h = 65, 5
    cam = look_at_camera([0.0, 2.0, 3.0], [0.0, 0.0, 0.0], w, h)
    away = look_at_camera([0.0, 2.0, 3.0], [0.0, 4.0, 6.0], w, h)
    frame = random_frame(np.random.default_rng(5), h, w)
    out = checker.run(clean_clip(w, h, [away, cam], [frame, frame]), prev=False, **FORMS[0])
    assert out[1].tobytes() == bytes(out[1].nbytes)


def test_a_depth_step_gives_no_weight_with_the_motion_still_reported(checker):
    w, h = 65, 5
    cam = look_at_camera([0.0, 2.0, 3.0], [0.0, 0.0, 0.0], w, h)
    colour, albedo, nd, mo = random_frame(np.random.default_rng(6), h, w)
    far = nd.copy()
    far[..., 3] *= f32(1.5)
    out = checker.run(clean_clip(w, h, [cam, cam], [(colour, albedo, nd, mo), (colour, albedo, far, mo)]), prev=False, **FORMS[0])[1]
    hit = albedo[..., 3] > 0
    assert hit.any() and (~hit).any()
    assert (out[..., 3][hit] == 0).all() and (out[..., 3][~hit] == 1).all()
    assert (out[..., :2] == 0).all() and (out[..., 2] > 0).all()


def test_refused_arguments(checker):
    w, h = 17, 1
    clip = synthetic_clip("same", w, h)
    assert checker.run(clip, rc=True) == 0
    for name in ("depth_tolerance", "normal_tolerance", "coverage_tolerance"):
        for v in (-1e-6, float("nan"), float("inf")):
            assert checker.run(clip, rc=True, **{name: v}) == -1, (name, v)
    bad = dict(clip, cameras=clip["cameras"].copy())
    bad["cameras"][2, 5] = np.inf
    assert checker.run(bad, rc=True) == -1
    flat = clip["prev"][0].copy()
    flat[6:9] = 0
    assert checker.run(dict(clip, prev=(flat,) + clip["prev"][1:]), rc=True) == -1
    assert checker.run(dict(clip, prev=(flat,) + clip["prev"][1:]), prev=False, rc=True) == 0  # (a prev set that is not given is not read)
