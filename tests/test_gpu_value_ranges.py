"""The post-process kernels across MAGNITUDES, SIGMA ENDS, SIGNS and NON-FINITE PIXELS (tests/value_ranges_lib.py): tptDenoiseKernel,
tptVarianceAtrousKernel, tptFramesAtrousKernel, tptTemporalKernel, tptReprojectObjectsKernel, tptFlowKernel and tptRectifyKernel.  The
rest of the suite holds them byte for byte to their C statements, but on planes from one narrow range -- colours of rand^3 * 4, depths
of 1 .. 20, cameras three units from the origin, the default sigmas --, and parts of them exist on the device only and depend on
magnitude.  Held here:

  - the fallback arm of tdivSafeNum in both a-trous filters (a weight's denominator outside [2^-60, 2^60], up to infinity): colours
    times 2^-140 ... 2^126, depths times 2^-60 ... 2^62, every sigma at the accepted ends 1e-6 and 1e6, at 1, 5 and 8 iterations;
  - the compiler's expansions behind the guards of tsqrt and trsqrt2 (an argument outside [2^-96, 2^96]) in the temporal, object and
    flow kernels, with the geometry times 2^-54 ... 2^50, and in the rectify kernel, with the colours times 2^-60 ... 2^50 -- against
    the checker on the scaled inputs AND against the device's own unscaled output, through the power-of-two relations that
    tests/test_value_ranges.py proves for the statements.  The fast forms without their guards still round right on those arguments
    (the guards are conservative); they go wrong below about 2^-108, so the rectify case at 2^-60 and the temporal, object and flow
    cases at 2^-62 (against the checker alone: the statements are not scale-invariant down there) are the ones a build without the
    guards fails;
  - NaN, infinities, 3e38, a subnormal and -1 planted in the colour, the albedo, the depth and the second moment: where the NaNs are
    (the statement fixes it: "in the order written, IEEE division"), and that nothing leaves the footprint -- the second against the
    device's own output for the clean planes, without any checker;
  - negative colours, albedo channels of -1, -0 and subnormals, second moments below the squared first (the `x > 0 ? x : 0` ternaries);
  - the clip form on three frames of 2^-100, 1 and 2^62 with a NaN in the middle one, which stays in its frame;
  - the whole chain -- two traced frames, temporal, rectify, variance filter, motion vectors -- on the extreme scenes of
    tests/scene_kinds_lib.py, stage by stage against the checkers on the device's own inputs.

The comparison is value_ranges_lib.same_bits wherever a reference may hold a NaN: the NaN positions equal, every other element
byte-equal; the chain is finite throughout and compared with tobytes().  Left out on purpose: a NaN's sign and payload, and scales
further out than those, where the statements themselves stop being scale-invariant.  tests/test_value_ranges.py proves on the CPU that
every case is what its name says."""
import numpy as np
import pytest

import scene_kinds_lib as scenes
import test_gpu_denoise as fixed_filter
import test_gpu_denoise_variance as variance_filter
import test_gpu_objects as objects_pass
import value_ranges_lib as lib
from clip_denoise_lib import filter_kwargs, stacks_of
from denoise_lib import DEMODULATE, DenoiseChecker
from flow_lib import FORMS, TOLERANCES, FlowChecker
from moments_lib import VarianceChecker
from object_lib import ObjectChecker
from rectify_lib import RectifyChecker
from temporal_lib import TemporalChecker, camera_floats
from test_gpu_clip_denoise import clip as denoise_clip
from test_gpu_flow import motion_vectors, upload
from test_gpu_lights import restore
from test_gpu_rectify import rectify
from test_gpu_temporal import accumulate, dev, host, plane, trace_frame
from value_ranges_lib import same_bits

pytestmark = pytest.mark.gpu

NAMES = ("colour", "albedo", "moments", "variance")


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    built = {}

    def get(cls):
        if cls not in built:
            built[cls] = cls(tmp_path_factory.mktemp(cls.__name__))
        return built[cls]
    return get


def record(cam):
    from toypathtracer_amd.api import CAMERA_DT
    return np.frombuffer(np.ascontiguousarray(cam, np.float32).tobytes(), CAMERA_DT)


def both_filters_all_modes(tpt, checkers, p, iterations):
    fixed_filter.check_all_modes(tpt, checkers(DenoiseChecker), p["colour"], p["albedo"], p["nd"], iterations, same=same_bits)
    variance_filter.check_all_modes(tpt, checkers(VarianceChecker), p["colour"], p["albedo"], p["nd"], p["moments"], lib.SAMPLES, iterations,
                                    same=same_bits)


# ---------------------------------------------------------------- 1. magnitudes, signs and small albedo through both a-trous filters
@pytest.mark.parametrize("name", list(lib.ATROUS_FAMILIES["magnitude"]) + list(lib.ATROUS_FAMILIES["depth"]))
def test_magnitudes_through_both_filters(tpt_defaults, checkers, name):
    both_filters_all_modes(tpt_defaults, checkers, lib.atrous_case(name), [lib.ITERATIONS])


@pytest.mark.parametrize("name", list(lib.ATROUS_FAMILIES["signs"]))
def test_signs_and_small_albedo(tpt_defaults, checkers, name):
    both_filters_all_modes(tpt_defaults, checkers, lib.atrous_case(name), [lib.ITERATIONS])


# ---------------------------------------------------------------- 2. the sigma ends
@pytest.mark.parametrize("name", lib.SIGMA_CASE_NAMES)
def test_sigma_ends_of_the_fixed_filter(tpt_defaults, checkers, name):
    tpt = tpt_defaults
    planes, sigmas, mode = lib.sigma_cases()[name]
    p = lib.atrous_case(planes)
    if mode == lib.EVERYTHING:
        fixed_filter.check_all_modes(tpt, checkers(DenoiseChecker), p["colour"], p["albedo"], p["nd"], lib.SIGMA_ITERATIONS, same=same_bits,
                                     sigmas=sigmas)
        return
    for it in lib.SIGMA_ITERATIONS:  # the colour term alone: no guide plane, no demodulation
        got, ins = fixed_filter.denoise_gpu(tpt, p["colour"], None, None, it, sigmas[0], 0.0, 0.0, False)
        assert same_bits(got, checkers(DenoiseChecker).run(p["colour"], None, None, it, sigmas[0], 0.0, 0.0, 0)), (name, it)
        assert ins[0].tobytes() == p["colour"].tobytes(), "an input was written"


@pytest.mark.parametrize("name", list(lib.VARIANCE_SIGMA_CASES))
def test_sigma_ends_of_the_variance_filter(tpt_defaults, checkers, name):
    sl, sn, sd = lib.VARIANCE_SIGMA_CASES[name]
    p = lib.clean_planes()
    variance_filter.check_all_modes(tpt_defaults, checkers(VarianceChecker), p["colour"], p["albedo"], p["nd"], p["moments"], lib.SAMPLES,
                                    lib.SIGMA_ITERATIONS, sl=sl, guides=(sn, sd), same=same_bits)


# ---------------------------------------------------------------- 3. planted non-finite pixels
def footprint_outputs(tpt, p):
    """both filters on the device, everything given, demodulated, FOOTPRINT_ITERATIONS iterations -> dict(fixed, variance)"""
    it = lib.FOOTPRINT_ITERATIONS
    sc, sn, sd = lib.default_sigmas()
    sl, vn, vd = lib.variance_sigmas()
    fixed, ins = fixed_filter.denoise_gpu(tpt, p["colour"], p["albedo"], p["nd"], it, sc, sn, sd, True)
    var, vins = variance_filter.denoise_gpu(tpt, p["colour"], p["albedo"], p["nd"], p["moments"], lib.SAMPLES, it, sl, vn, vd, True)
    for x, y in list(zip(ins, (p["colour"], p["albedo"], p["nd"]))) + list(zip(vins, (p["colour"], p["albedo"], p["nd"], p["moments"]))):
        assert same_bits(x, y), "an input was written"
    return dict(fixed=fixed, variance=var)


@pytest.fixture(scope="module")
def clean(tpt):
    """the device's own outputs for the clean footprint planes"""
    return footprint_outputs(tpt, lib.footprint_planes())


@pytest.mark.parametrize("plane_name,value", lib.FOOTPRINT_CASES, ids=lambda v: v)
def test_a_planted_value_stays_inside_its_footprint(tpt_defaults, checkers, clean, plane_name, value):
    tpt = tpt_defaults
    w, h = lib.FOOTPRINT_SIZE
    it = lib.FOOTPRINT_ITERATIONS
    p = lib.footprint_planes(plane_name, value)
    got = footprint_outputs(tpt, p)
    sc, sn, sd = lib.default_sigmas()
    sl, vn, vd = lib.variance_sigmas()
    want = dict(fixed=checkers(DenoiseChecker).run(p["colour"], p["albedo"], p["nd"], it, sc, sn, sd, DEMODULATE),
                variance=checkers(VarianceChecker).run(p["colour"], p["albedo"], p["nd"], p["moments"], lib.SAMPLES, iterations=it,
                                                       sigma_luminance=sl, sigma_normal=vn, sigma_depth=vd, flags=DEMODULATE))
    outside = lib.footprint_mask(h, w, *lib.FOOTPRINT_AT, it)
    for what in ("fixed", "variance"):
        assert same_bits(got[what], want[what]), "%s filter: differs from the checker" % what
        assert got[what][outside].tobytes() == clean[what][outside].tobytes(), "%s filter: the planted value left its footprint" % what


# ---------------------------------------------------------------- 4. the clip form
def test_the_clip_form_keeps_a_nan_in_its_frame(tpt_defaults, checkers):
    """three frames of 130x67 in one tptDenoiseClipDevice call, spatial only: colour times 2^-100, times 1 with a NaN pixel, times 2^62;
    every frame is the variance checker's filter of that frame alone"""
    tpt = tpt_defaults
    w, h = lib.W, lib.H
    middle = lib.planted(lib.clean_planes(), ("colour", h // 2, w // 2, 1), np.nan)
    frames = [tuple(p[k] for k in lib.PLANES) for p in (lib.atrous_case("colour_2^-100"), middle, lib.atrous_case("colour_2^62"))]
    got = denoise_clip(tpt, w, h, stacks_of(frames), lib.SAMPLES, spatial_only=True, iterations=lib.ITERATIONS, demodulate=True).cpu().numpy()
    kw = filter_kwargs(tpt, True, True, lib.ITERATIONS)
    for j, (colour, albedo, nd, moments) in enumerate(frames):
        want = checkers(VarianceChecker).run(colour, albedo, nd, moments, lib.SAMPLES, **kw)
        assert same_bits(got[j], want), "frame %d differs from the filter of that frame alone" % j
    assert not np.isnan(got[0]).any() and not np.isnan(got[2]).any() and np.isnan(got[1]).any()


# ---------------------------------------------------------------- 5. the geometry's scale
def temporal_gpu(tpt, case):
    cam, cur, prev = case
    w, h = lib.W, lib.H
    dcur, dprev = [dev(a) for a in cur], [dev(a) for a in prev[1:]]
    outs = accumulate(tpt, w, h, record(cam), dcur, (record(prev[0]),) + tuple(dprev), **lib.TEMPORAL_KW)
    tpt.synchronize()
    for a, d in zip(list(cur) + list(prev[1:]), dcur + dprev):
        assert same_bits(a, d.cpu().numpy()), "an input was written"
    return host(outs)


@pytest.mark.parametrize("kind", lib.TEMPORAL_KINDS)
def test_temporal_pass_across_the_geometry_s_scale(tpt_defaults, checkers, kind):
    tpt = tpt_defaults
    base = temporal_gpu(tpt, lib.temporal_case(kind))
    for k in (0,) + lib.GEOMETRY_SCALES:
        case = lib.temporal_case(kind, k)
        got = temporal_gpu(tpt, case)
        want = checkers(TemporalChecker).run(*case, **lib.TEMPORAL_KW)
        for name, g, wnt, b in zip(NAMES, got, want, base):
            assert same_bits(g, wnt), "k = %d: out %s differs from the checker" % (k, name)
            assert same_bits(g, b), "k = %d: out %s differs from the device's own k = 0 output" % (k, name)


def objects_gpu(tpt, case, table):
    cam, cur, obj, prev, motion = case
    w, h = lib.W, lib.H
    dcur, dobj, dmotion = [dev(a) for a in cur], dev(obj), dev(motion)
    dprev = (record(prev[0]),) + tuple(dev(a) for a in prev[1:])
    outs = objects_pass.accumulate(tpt, w, h, record(cam), dcur, dobj, dprev, dmotion if table else None, **lib.TEMPORAL_KW)
    tpt.synchronize()
    for a, d in zip(list(cur) + [obj, motion] + list(prev[1:]), dcur + [dobj, dmotion] + list(dprev[1:])):
        assert same_bits(a, d.cpu().numpy()), "an input was written"
    return host(outs)


@pytest.mark.parametrize("table", [True, False], ids=["table", "no_table"])
def test_object_pass_across_the_geometry_s_scale(tpt_defaults, checkers, table):
    tpt = tpt_defaults
    base = objects_gpu(tpt, lib.object_case(), table)
    for k in (0,) + lib.OBJECT_SCALES:
        case = lib.object_case(k)
        got = objects_gpu(tpt, case, table)
        cam, cur, obj, prev, motion = case
        want = checkers(ObjectChecker).run(cam, cur, obj, prev, motion if table else None, **lib.TEMPORAL_KW)
        for name, g, wnt, b in zip(NAMES, got, want, base):
            assert same_bits(g, wnt), "k = %d: out %s differs from the checker" % (k, name)
            assert same_bits(g, b), "k = %d: out %s differs from the device's own k = 0 output" % (k, name)


@pytest.mark.parametrize("kind", lib.FLOW_KINDS)
def test_motion_vectors_across_the_geometry_s_scale(tpt_defaults, checkers, kind):
    tpt = tpt_defaults
    clip0 = lib.flow_case(kind)
    dev0 = upload(clip0)
    for form in FORMS:
        base = motion_vectors(tpt, dev0, **form, **TOLERANCES)
        for k in (0,) + lib.GEOMETRY_SCALES:
            clip = lib.flow_case(kind, k)
            got = motion_vectors(tpt, upload(clip), **form, **TOLERANCES)
            assert same_bits(got, checkers(FlowChecker).run(clip, **form, **TOLERANCES)), "%r, k = %d: differs from the checker" % (form, k)
            assert same_bits(got, lib.flow_expected(base, clip, k)), \
                "%r, k = %d: not the device's own k = 0 output with e times 2^k on the covered pixels" % (form, k)


def test_motion_vectors_below_the_scale_invariant_range(tpt_defaults, checkers):
    """the "pixel" clip at 2^-62: |rel|^2 is 2^-138 .. 2^-124, where the five-instruction square root without its guard misrounds (and
    the statement's own products are subnormal, so there is no relation to the k = 0 output: the checker alone)"""
    tpt = tpt_defaults
    clip = lib.flow_case("pixel", lib.FLOW_DEEP_SCALE)
    d = upload(clip)
    for form in FORMS:
        got = motion_vectors(tpt, d, **form, **TOLERANCES)
        assert same_bits(got, checkers(FlowChecker).run(clip, **form, **TOLERANCES)), "%r: differs from the checker" % (form,)


@pytest.mark.parametrize("kind", lib.TEMPORAL_KINDS)
def test_temporal_pass_below_the_scale_invariant_range(tpt_defaults, checkers, kind):
    """geometry times 2^-62: |rel|^2 and the squared length of every pixel's ray are 2^-124 .. 2^-118, where tsqrt and trsqrt2 without
    their guards round wrong; the checker alone"""
    case = lib.temporal_case(kind, lib.TEMPORAL_DEEP_SCALE)
    got = temporal_gpu(tpt_defaults, case)
    for name, g, wnt in zip(NAMES, got, checkers(TemporalChecker).run(*case, **lib.TEMPORAL_KW)):
        assert same_bits(g, wnt), "out %s differs from the checker" % name


@pytest.mark.parametrize("table", [True, False], ids=["table", "no_table"])
def test_object_pass_below_the_scale_invariant_range(tpt_defaults, checkers, table):
    case = lib.object_case(lib.TEMPORAL_DEEP_SCALE)
    got = objects_gpu(tpt_defaults, case, table)
    cam, cur, obj, prev, motion = case
    for name, g, wnt in zip(NAMES, got, checkers(ObjectChecker).run(cam, cur, obj, prev, motion if table else None, **lib.TEMPORAL_KW)):
        assert same_bits(g, wnt), "out %s differs from the checker" % name


# ---------------------------------------------------------------- 6. the colour's scale
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_rectify_across_the_colour_s_scale(tpt_defaults, checkers, radius):
    tpt = tpt_defaults
    w, h = lib.W, lib.H
    kw = dict(radius=radius, gamma=lib.RECTIFY_KW["gamma"])

    def run(planes, in_place):
        d = [dev(a) for a in planes]
        outs = rectify(tpt, w, h, *d, in_place=in_place, **kw)
        tpt.synchronize()
        got = host(outs)
        for a, t in list(zip(planes, d))[:2 if in_place else 4]:
            assert same_bits(a, t.cpu().numpy()), "an input was written"
        return got

    base = run(lib.rectify_case(), False)
    for k in (0,) + lib.RECTIFY_SCALES:
        planes = lib.rectify_case(k)
        want = checkers(RectifyChecker).run(*planes, **kw)
        colour, N = lib.rectify_expected(base, k)
        for in_place in (False, True):
            got = run(planes, in_place)
            for name, g, wnt in zip(("colour", "moments", "variance"), got, want):
                assert same_bits(g, wnt), "k = %d, in place %s: out %s differs from the checker" % (k, in_place, name)
            if k not in lib.SCALES and k != 0 and radius != lib.RECTIFY_KW["radius"]:
                continue  # (k = -60: the statement's relation to k = 0 holds at radius 2 only; the checker alone)
            assert same_bits(got[0], colour), "k = %d, in place %s: not 2^k times the device's own k = 0 colour" % (k, in_place)
            assert same_bits(got[1][..., 3], N) and same_bits(got[2][..., 3], base[2][..., 3]), "k = %d: the history lengths differ" % k


# ---------------------------------------------------------------- 7. the chain on the extreme scenes
CHAIN_SCENES = ("albedo_2", "albedo_-0.5", "scale_2^16", "scale_2^-12", "far_camera_2000", "offset_100000")


@pytest.mark.parametrize("name", CHAIN_SCENES)
def test_the_chain_on_an_extreme_scene(tpt_defaults, checkers, name):
    """96x54 at 2 spp: two frames through tptDrawDeviceMoments, then the temporal pass, the rectification (radius 2, gamma 1) and the
    variance filter (3 iterations, demodulated, both guides), and tptMotionVectorsDevice between the two frames; every stage equals its
    checker on the device's own inputs byte for byte -- every plane of the chain is finite"""
    tpt = tpt_defaults
    w, h, spp = 96, 54, 2
    s, m, camera = scenes.scene(name)
    temporal_kw, rectify_kw, iterations = dict(max_history=8.0), dict(radius=2, gamma=1.0), 3
    try:
        tpt.set_scene(s, m)
        if camera is not None:
            tpt.set_camera(**camera)
        tpt.set_samples_per_pixel(spp)
        (cam0, cur0), (cam1, cur1) = [trace_frame(tpt, w, h, j, 0, 0.0) for j in range(2)]
        acc0 = accumulate(tpt, w, h, cam0, cur0, None, **temporal_kw)
        acc1 = accumulate(tpt, w, h, cam1, cur1, (cam0, acc0[0], acc0[1], cur0[2], acc0[2]), **temporal_kw)
        rect = rectify(tpt, w, h, cur1[0], cur1[3], acc1[0], acc1[2], **rectify_kw)
        out = plane(h, w, float("nan"))
        tpt.denoise_device_variance(w, h, rect[0].data_ptr(), rect[2].data_ptr(), tpt.moment_samples(spp), out.data_ptr(),
                                    albedo_ptr=acc1[1].data_ptr(), normal_depth_ptr=cur1[2].data_ptr(), iterations=iterations)
        tpt.synchronize()
        hcur0, hcur1, hacc0, hacc1, hrect, hout = host(cur0), host(cur1), host(acc0), host(acc1), host(rect), out.cpu().numpy()
        clip = dict(cameras=np.ascontiguousarray(np.stack([camera_floats(cam0), camera_floats(cam1)])),
                    albedo=np.ascontiguousarray(np.stack([hcur0[1], hcur1[1]])), nd=np.ascontiguousarray(np.stack([hcur0[2], hcur1[2]])),
                    objects=np.zeros((2, h, w), np.int32), motion=np.zeros((2, 1, 4), np.float32), prev=None)
        flow_kw = {k: v for k, v in tpt.TEMPORAL_DEFAULTS.items() if k != "max_history"}
        flow = motion_vectors(tpt, upload(clip), objects=False, table=False, prev=False, **flow_kw)
    finally:
        restore(tpt)
    everything = hcur0 + hcur1 + hacc0 + hacc1 + hrect + [hout, flow]
    assert all(np.isfinite(a).all() for a in everything), "a plane of the chain is not finite"
    want0 = checkers(TemporalChecker).run(cam0, tuple(hcur0), None, **temporal_kw)
    want1 = checkers(TemporalChecker).run(cam1, tuple(hcur1), (cam0, hacc0[0], hacc0[1], hcur0[2], hacc0[2]), **temporal_kw)
    for j, (got, want) in enumerate(((hacc0, want0), (hacc1, want1))):
        for pname, g, wnt in zip(NAMES, got, want):
            assert g.tobytes() == wnt.tobytes(), "temporal pass, frame %d: out %s differs from the checker" % (j, pname)
    want = checkers(RectifyChecker).run(hcur1[0], hcur1[3], hacc1[0], hacc1[2], **rectify_kw)
    for pname, g, wnt in zip(("colour", "moments", "variance"), hrect, want):
        assert g.tobytes() == wnt.tobytes(), "rectification: out %s differs from the checker" % pname
    want = checkers(VarianceChecker).run(hrect[0], hacc1[1], hcur1[2], hrect[2], float(tpt.moment_samples(spp)),
                                         **filter_kwargs(tpt, True, True, iterations))
    assert hout.tobytes() == want.tobytes(), "the variance filter differs from the checker"
    want = checkers(FlowChecker).run(clip, objects=False, table=False, prev=False, **flow_kw)
    assert flow.tobytes() == want.tobytes(), "the motion vectors differ from the checker"
    history = float((hacc1[2][..., 3] > 1).mean())
    clipped = float((hrect[0].view(np.uint32) != hacc1[0].view(np.uint32)).any(axis=-1).mean())
    print("%s: colours %.3g .. %.3g, depths up to %.3g, history on %.4f of the pixels, %.4f clipped"
          % (name, hcur1[0][..., :3].min(), hcur1[0][..., :3].max(), hcur1[2][..., 3].max(), history, clipped))
    assert history >= 0.5 and clipped > 0 and not flow[0].any() and (flow[1][..., 3] > 0).mean() >= 0.5
