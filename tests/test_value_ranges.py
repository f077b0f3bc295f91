"""The catalogue of tests/value_ranges_lib.py without a GPU: every case is what its name says, proven from the C checkers and the numpy
statements alone.  These are the conditions that keep tests/test_gpu_value_ranges.py from passing vacuously:

  - the C checker and the numpy statement agree (same_bits) on every case, so the reference itself is not in doubt out there;
  - the cases named "straddles" put at least 1 % of the first-iteration tap denominators of tptDenoiseDevice above 2^60 (the arm of
    tdivSafeNum that takes `a / b`) and at least 1 % at or below it; the cases named "inside" put none above;
  - at least half of the rgb values of every reference output are numbers (all but `overflow_2^126`, whose demodulated colour
    overflows): a case that drowned in NaN would hold the device to nothing but the positions of its NaNs;
  - a planted non-finite, huge, subnormal or negative value stays inside the footprint of R = 2 (2^iterations - 1) pixels, changes
    something inside it, and a NaN in the colour fills it;
  - the temporal, object, flow and rectify statements are invariant under a power-of-two scale of the geometry / the colour for
    k in {-50, -12, 16, 50} (the rectify statement also at -60), with history, weight and clipping on a stated share of the pixels;
    at k = -12 and 16 the argument of the guarded square root lies inside [2^-96, 2^96] for every pixel, and outside it for at least half of the pixels that reach it at
    k = +-50 (and -60) for the rectify case and at k = 50 for every geometry case.  At k = -50 the geometry cases are asserted at
    0.25 only (the "pixel" clip, a plane at depth 1, measures 0.97).  The others cannot have half: their depths are 1 .. 9, |rel|^2 2^-100 is below 2^-96 only for a depth below 4, which is 3/8 of the covered
    6/7 of the pixels (asserted: at least 0.25; measured 0.29 .. 0.33).  So the geometry cases also run at k = -54, where every
    covered pixel is outside (asserted: at least half; measured 0.82 .. 0.97) and the statements are invariant as well;
  - the deep cases (rectify at k = -60, the flow, temporal and object cases at k = -62) put at least half of the square roots'
    arguments below 2^-118, where the fast forms without their guards round wrong, and their two statements still agree.

Every share is printed (pytest -s) at the committed seeds.  Left out on purpose: NaN payloads and signs, and k beyond -54 / +50, where
the statements themselves stop being scale-invariant (squares of lengths and colours leave the normal range).  The object statement
holds at all five k, so none is dropped for it."""
import numpy as np
import pytest

import value_ranges_lib as lib
from denoise_lib import DEMODULATE, DenoiseChecker, denoise_numpy
from flow_lib import FORMS, TOLERANCES, FlowChecker, flow_numpy
from moments_lib import VarianceChecker, variance_numpy
from object_lib import ObjectChecker, object_numpy
from rectify_lib import RectifyChecker, rectify_numpy
from temporal_lib import TemporalChecker, temporal_numpy
from value_ranges_lib import same_bits

f32 = np.float32
MODES = ((True, True, True), (False, False, False))  # (albedo, normal / depth, demodulate): everything, and the colour alone


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    built = {}

    def get(cls):
        if cls not in built:
            built[cls] = cls(tmp_path_factory.mktemp(cls.__name__))
        return built[cls]
    return get


def non_nan_share(out):
    return float((~np.isnan(out[..., :3])).mean())


def fixed(checker, p, iterations, sigmas, mode=(True, True, True), numpy_too=True):
    """tptDenoiseDevice's statement on a case's planes -> the checker's output (held against the numpy statement)"""
    use_alb, use_nd, demod = mode
    kw = dict(iterations=iterations, sigma_colour=sigmas[0], sigma_normal=sigmas[1] if use_nd else 0.0, sigma_depth=sigmas[2] if use_nd else 0.0,
              flags=DEMODULATE if demod else 0)
    args = (p["colour"], p["albedo"] if use_alb else None, p["nd"] if use_nd else None)
    want = checker.run(*args, **kw)
    if numpy_too:
        assert same_bits(denoise_numpy(*args, **kw), want), ("tptDenoiseDevice's two statements differ", mode, iterations)
    return want


def variance(checker, p, iterations, sigmas, mode=(True, True, True), numpy_too=True):
    """tptDenoiseDeviceVariance's statement on a case's planes -> the checker's output (held against the numpy statement)"""
    use_alb, use_nd, demod = mode
    kw = dict(iterations=iterations, sigma_luminance=sigmas[0], sigma_normal=sigmas[1] if use_nd else 0.0,
              sigma_depth=sigmas[2] if use_nd else 0.0, flags=DEMODULATE if demod else 0)
    args = (p["colour"], p["albedo"] if use_alb else None, p["nd"] if use_nd else None, p["moments"], lib.SAMPLES)
    want = checker.run(*args, **kw)
    if numpy_too:
        assert same_bits(variance_numpy(*args, **kw), want), ("tptDenoiseDeviceVariance's two statements differ", mode, iterations)
    return want


# ---------------------------------------------------------------- 1. magnitudes, depths and signs through both filters
@pytest.mark.parametrize("name", ["clean"] + list(lib.ATROUS_CASES))
def test_atrous_cases(checkers, name):
    p = lib.atrous_case(name)
    for mode in MODES:
        for what, run, sigmas in (("fixed", fixed, lib.default_sigmas()), ("variance", variance, lib.variance_sigmas())):
            out = run(checkers(DenoiseChecker if run is fixed else VarianceChecker), p, lib.ITERATIONS, sigmas, mode)
            share = non_nan_share(out)
            print("%s %s %r: non-NaN share of the rgb values %.4f" % (name, what, mode, share))
            assert out[..., 3].tobytes() == p["colour"][..., 3].tobytes()
            if name not in lib.MAY_BE_MOSTLY_NAN:
                assert share >= 0.5, (name, what, mode, share)
            if name == "clean" or name.startswith(("colour_2^", "depth_2^")):
                assert share == 1.0, (name, what, mode, share)  # (measured: no NaN in any magnitude case below the overflow)


def test_the_signs_cases_are_what_they_say():
    clean = lib.clean_planes()
    c = lib.atrous_case("negated_colour")["colour"]
    neg = (c[..., :3] < 0).any(axis=-1).mean()
    assert 0.25 < neg < 0.4 and np.array_equal(np.abs(c), np.abs(clean["colour"]))
    a = lib.atrous_case("odd_albedo")["albedo"]
    tiny = f32(2.0 ** -126)
    assert (a == -1).sum() > 100 and ((a == 0) & np.signbit(a)).sum() > 100 and ((a > 0) & (a < tiny)).sum() > 200
    m = lib.atrous_case("low_moments")["moments"]
    assert (m[..., 1] < m[..., 0] * m[..., 0]).all()


# ---------------------------------------------------------------- 2. the sigma ends and the guard of the weights' division
@pytest.mark.parametrize("name", lib.SIGMA_CASE_NAMES)
def test_sigma_cases_lie_where_their_names_say(checkers, name):
    planes, sigmas, mode = lib.sigma_cases()[name]
    p = lib.atrous_case(planes)
    den = lib.first_iteration_denominators(p["colour"], p["albedo"], p["nd"] if mode[1] else None, sigmas, demodulate=mode[2])
    above, inside, infinite = lib.division_shares(den)
    print("%s: first-iteration taps %d, above 2^60 %.4f (of those infinite %.4f), at or below %.4f" % (name, den.size, above, infinite, inside))
    if name.startswith("straddles"):
        assert above >= 0.01 and inside >= 0.01, (name, above, inside)
    else:
        assert name.startswith("inside") and above == 0 and inside == 1.0, (name, above, inside)
    for it in lib.SIGMA_ITERATIONS:
        out = fixed(checkers(DenoiseChecker), p, it, sigmas, mode)
        share = non_nan_share(out)
        print("%s, %d iterations: non-NaN share %.4f" % (name, it, share))
        assert share == 1.0, (name, it, share)  # (measured: no NaN in any sigma case)


@pytest.mark.parametrize("name", list(lib.VARIANCE_SIGMA_CASES))
def test_variance_sigma_cases(checkers, name):
    sigmas = lib.VARIANCE_SIGMA_CASES[name]
    p = lib.clean_planes()
    den = lib.first_iteration_denominators(p["colour"], p["albedo"], p["nd"], sigmas, moments=p["moments"])
    above, inside, infinite = lib.division_shares(den)
    print("%s: first-iteration taps %d, above 2^60 %.4f (of those infinite %.4f), at or below %.4f" % (name, den.size, above, infinite, inside))
    if sigmas[1] == 1e-6:  # the guides' inverse squared sigma of 1e12 alone carries most taps past 2^60
        assert above >= 0.01 and inside >= 0.01, (name, above, inside)
    for it in lib.SIGMA_ITERATIONS:
        out = variance(checkers(VarianceChecker), p, it, sigmas)
        share = non_nan_share(out)
        print("%s, %d iterations: non-NaN share %.4f" % (name, it, share))
        assert share == 1.0, (name, it, share)


def test_the_variance_filter_straddles_on_the_scaled_colour():
    """colour times 2^40 at the default sigmas: the luminance term alone is past 2^60 for most taps"""
    p = lib.atrous_case("colour_2^40")
    den = lib.first_iteration_denominators(p["colour"], p["albedo"], p["nd"], lib.variance_sigmas(), moments=p["moments"])
    above, inside, _ = lib.division_shares(den)
    print("variance filter, colour_2^40: above 2^60 %.4f, at or below %.4f" % (above, inside))
    assert above >= 0.01 and inside >= 0.01


# ---------------------------------------------------------------- 3. the footprint of a planted value
@pytest.fixture(scope="module")
def clean(checkers):
    """both filters' outputs for the clean footprint planes"""
    p = lib.footprint_planes()
    return dict(fixed=fixed(checkers(DenoiseChecker), p, lib.FOOTPRINT_ITERATIONS, lib.default_sigmas()),
                variance=variance(checkers(VarianceChecker), p, lib.FOOTPRINT_ITERATIONS, lib.variance_sigmas()))


def test_the_footprint_is_29_pixels_wide_inside_the_image():
    w, h = lib.FOOTPRINT_SIZE
    y0, x0 = lib.FOOTPRINT_AT
    r = lib.footprint_radius(lib.FOOTPRINT_ITERATIONS)
    outside = lib.footprint_mask(h, w, y0, x0, lib.FOOTPRINT_ITERATIONS)
    assert r == 14 and y0 - r >= 0 and y0 + r < h and x0 - r >= 0 and x0 + r < w
    assert (~outside).sum() == 29 * 29 and abs(outside.mean() - 0.79) < 0.005


@pytest.mark.parametrize("plane,value", lib.FOOTPRINT_CASES, ids=lambda v: v)
def test_a_planted_value_stays_inside_its_footprint(checkers, clean, plane, value):
    w, h = lib.FOOTPRINT_SIZE
    outside = lib.footprint_mask(h, w, *lib.FOOTPRINT_AT, lib.FOOTPRINT_ITERATIONS)
    p = lib.footprint_planes(plane, value)
    outs = dict(fixed=fixed(checkers(DenoiseChecker), p, lib.FOOTPRINT_ITERATIONS, lib.default_sigmas()),
                variance=variance(checkers(VarianceChecker), p, lib.FOOTPRINT_ITERATIONS, lib.variance_sigmas()))
    for what, out in outs.items():
        assert out[outside].tobytes() == clean[what][outside].tobytes(), "%s: the planted value left its footprint" % what
        changed = int((out.view(np.uint32) != clean[what].view(np.uint32)).any(axis=-1).sum())
        share = non_nan_share(out)
        print("%s = %s, %s: %d pixels changed, non-NaN share %.4f" % (plane, value, what, changed, share))
        assert share >= 0.5
        if what == "fixed" and plane == "moments.y":
            assert changed == 0  # (the fixed-sigma filter does not read the moments)
        else:
            assert changed >= 1, "%s: the planted value changed nothing" % what
        if plane == "colour.g" and value == "nan":
            assert int(np.isnan(out[..., :3]).all(axis=-1).sum()) == 29 * 29 and np.isnan(out[~outside][..., :3]).all()


# ---------------------------------------------------------------- 4. power-of-two invariance of the other statements
def guard_shares(name, k, args, geometry=True):
    share, count = lib.outside_sqrt_guard(args)
    print("%s, k = %d: %d positive square-root arguments, outside [2^-96, 2^96] %.4f" % (name, k, count, share))
    assert count > 0
    if k in lib.MOST_OUTSIDE_THE_SQRT_GUARD or (abs(k) >= 50 and not geometry):
        assert share >= 0.5, (name, k, share)
    elif k == -50:  # (the geometry cases: depths of 1 .. 9, of which those below 4 square to less than 2^-96 -- see GEOMETRY_SCALES)
        assert share >= 0.25, (name, k, share)
    else:
        assert share == 0.0, (name, k, share)


@pytest.mark.parametrize("kind", lib.TEMPORAL_KINDS)
def test_temporal_statement_is_scale_invariant(checkers, kind):
    checker = checkers(TemporalChecker)
    base = checker.run(*lib.temporal_case(kind), **lib.TEMPORAL_KW)
    assert all(same_bits(a, b) for a, b in zip(base, temporal_numpy(*lib.temporal_case(kind), **lib.TEMPORAL_KW)))
    history = float((base[2][..., 3] > 1).mean())
    print("temporal %s: history (N > 1) on %.4f of the pixels" % (kind, history))
    assert history >= 0.5
    for k in lib.GEOMETRY_SCALES:
        cam, cur, prev = lib.temporal_case(kind, k)
        got = checker.run(cam, cur, prev, **lib.TEMPORAL_KW)
        assert all(same_bits(a, b) for a, b in zip(got, temporal_numpy(cam, cur, prev, **lib.TEMPORAL_KW))), (kind, k)
        for name, a, b in zip(("colour", "albedo", "moments", "variance"), got, base):
            assert same_bits(a, b), "temporal %s, k = %d: out %s is not the k = 0 output" % (kind, k, name)
        guard_shares("temporal " + kind, k, lib.rel_squared(cam, cur[1], cur[2], prev[0]))


def test_object_statement_is_scale_invariant(checkers):
    checker = checkers(ObjectChecker)
    cam, cur, obj, prev, motion = lib.object_case()
    for table in (True, False):
        base = checker.run(cam, cur, obj, prev, motion if table else None, **lib.TEMPORAL_KW)
        history = float((base[2][..., 3] > 1).mean())
        print("object pass, table %s: history (N > 1) on %.4f of the pixels" % (table, history))
        assert history >= 0.2
        for k in lib.OBJECT_SCALES:
            c, cu, ob, pv, mo = lib.object_case(k)
            got = checker.run(c, cu, ob, pv, mo if table else None, **lib.TEMPORAL_KW)
            assert all(same_bits(a, b) for a, b in zip(got, object_numpy(c, cu, ob, pv, mo if table else None, **lib.TEMPORAL_KW))), k
            for name, a, b in zip(("colour", "albedo", "moments", "variance"), got, base):
                assert same_bits(a, b), "object pass, table %s, k = %d: out %s is not the k = 0 output" % (table, k, name)
            if table:
                guard_shares("object pass", k, lib.rel_squared(c, cu[1], cu[2], pv[0], ob, mo))


@pytest.mark.parametrize("kind", lib.FLOW_KINDS)
def test_flow_statement_scales_its_distance_alone(checkers, kind):
    checker = checkers(FlowChecker)
    clip0 = lib.flow_case(kind)
    for form in FORMS:
        base = checker.run(clip0, **form, **TOLERANCES)
        assert same_bits(base, flow_numpy(clip0, **form, **TOLERANCES))
        weight = float((base[..., 3] > 0).mean())
        print("flow %s %r: weight > 0 on %.4f of the pixels" % (kind, form, weight))
        assert weight >= 0.2
        for k in lib.GEOMETRY_SCALES:
            clip = lib.flow_case(kind, k)
            got = checker.run(clip, **form, **TOLERANCES)
            assert same_bits(got, flow_numpy(clip, **form, **TOLERANCES)), (kind, form, k)
            assert same_bits(got, lib.flow_expected(base, clip, k)), "flow %s %r, k = %d: not the k = 0 output with .z scaled" % (kind, form, k)
    for k in lib.GEOMETRY_SCALES:
        clip = lib.flow_case(kind, k)
        args = [lib.rel_squared(clip["cameras"][j], clip["albedo"][j], clip["nd"][j], clip["cameras"][j - 1] if j else clip["prev"][0],
                                clip["objects"][j], clip["motion"][j]) for j in range(3)]
        guard_shares("flow " + kind, k, np.stack(args))


def test_the_deep_cases_reach_where_the_unguarded_square_root_goes_wrong(checkers):
    """value_ranges_lib.RECTIFY_SCALES, FLOW_DEEP_SCALE: at least half of the square roots' arguments lie below 2^-118"""
    var = lib.window_variance(lib.rectify_case(lib.RECTIFY_SCALES[0]), lib.RECTIFY_KW["radius"])
    var = var[var > 0]
    clip = lib.flow_case("pixel", lib.FLOW_DEEP_SCALE)
    rel2 = np.stack([lib.rel_squared(clip["cameras"][j], clip["albedo"][j], clip["nd"][j], clip["cameras"][j - 1] if j else clip["prev"][0],
                                     clip["objects"][j], clip["motion"][j]) for j in range(3)])
    rel2 = rel2[(rel2 > 0) & np.isfinite(rel2)]
    shares = float((var < lib.DEEP).mean()), float((rel2 < lib.DEEP).mean())
    print("below 2^-118: %.4f of the window variances at k = %d, %.4f of |rel|^2 at k = %d" % (shares[0], lib.RECTIFY_SCALES[0], shares[1], lib.FLOW_DEEP_SCALE))
    assert min(shares) >= 0.5
    for form in FORMS:
        got = checkers(FlowChecker).run(clip, **form, **TOLERANCES)
        assert same_bits(got, flow_numpy(clip, **form, **TOLERANCES)), form
        assert (got[..., 3] > 0).mean() >= 0.2 and non_nan_share(got) >= 0.5
    k = lib.TEMPORAL_DEEP_SCALE
    for kind in lib.TEMPORAL_KINDS:
        cam, cur, prev = lib.temporal_case(kind, k)
        got = checkers(TemporalChecker).run(cam, cur, prev, **lib.TEMPORAL_KW)
        assert all(same_bits(a, b) for a, b in zip(got, temporal_numpy(cam, cur, prev, **lib.TEMPORAL_KW))), kind
        rel2 = lib.rel_squared(cam, cur[1], cur[2], prev[0])
        covered, ray2 = cur[1][..., 3] > 0, lib.ray_squared(cam, lib.W, lib.H)
        history = float((got[2][..., 3] > 1).mean())
        print("temporal %s at k = %d: below 2^-118 %.4f of the covered pixels' |rel|^2, %.4f of |v|^2; history on %.4f"
              % (kind, k, (rel2[covered] < lib.DEEP).mean(), (ray2 < lib.DEEP).mean(), history))
        assert (rel2[covered] < lib.DEEP).mean() >= 0.5 and (ray2 < lib.DEEP).mean() >= 0.5 and history >= 0.5
    cam, cur, obj, prev, motion = lib.object_case(k)
    for table in (motion, None):
        got = checkers(ObjectChecker).run(cam, cur, obj, prev, table, **lib.TEMPORAL_KW)
        assert all(same_bits(a, b) for a, b in zip(got, object_numpy(cam, cur, obj, prev, table, **lib.TEMPORAL_KW))), table is None
        assert (got[2][..., 3] > 1).mean() >= 0.2


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_rectify_statement_scales_with_its_colours(checkers, radius):
    checker = checkers(RectifyChecker)
    kw = dict(lib.RECTIFY_KW, radius=radius)
    base = checker.run(*lib.rectify_case(), **kw)
    assert all(same_bits(a, b) for a, b in zip(base, rectify_numpy(*lib.rectify_case(), **kw)))
    acc = lib.rectify_case()[2]
    clipped = float((base[0].view(np.uint32) != acc.view(np.uint32)).any(axis=-1).mean())
    print("rectify, radius %d: %.4f of the pixels clipped" % (radius, clipped))
    assert clipped >= 0.2
    for k in lib.RECTIFY_SCALES:
        planes = lib.rectify_case(k)
        got = checker.run(*planes, **kw)
        assert all(same_bits(a, b) for a, b in zip(got, rectify_numpy(*planes, **kw))), k
        if k not in lib.SCALES and radius != lib.RECTIFY_KW["radius"]:
            continue  # (k = -60: the relation holds at radius 2; the windows of 1 and 3 round otherwise down there)
        colour, N = lib.rectify_expected(base, k)
        assert same_bits(got[0], colour), "rectify, k = %d: the colour is not 2^k times the k = 0 colour" % k
        assert same_bits(got[1][..., 3], N) and same_bits(got[2][..., 3], base[2][..., 3]), "rectify, k = %d: the history lengths differ" % k
        if radius == lib.RECTIFY_KW["radius"]:
            guard_shares("rectify", k, lib.window_variance(planes, radius), geometry=False)
