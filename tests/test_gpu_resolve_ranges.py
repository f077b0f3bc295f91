"""The kernels between the tracer and the screen across MAGNITUDES, SIGNS and NON-FINITE VALUES (tests/resolve_ranges_lib.py):
tptDisplayKernel, the blends (tptResolveKernel, tptResolveMirrorKernel, tptResolveBatchKernel, tptFoldBatchKernel,
tptAdaptiveResolveKernel), tptAdaptivePlanKernel and tptSpreadKernel.  The rest of the suite feeds them rendered tiles, zeroed planes
and moments of rand^3 * 4.  Held here:

  - the display conversion at every one of its 255 steps from both sides, at both ends of tsqrt's guard, for zeros, subnormals,
    infinities, negatives and NaNs of both kinds and signs, with garbage in alpha, at sizes that are no whole number of workgroups,
    with a sentinel behind the image: NaN and negative channels are 0 (include/tpt_hip.h), the rows are flipped, nothing else is
    written;
  - blendPixel's contract in every kernel that blends into a caller's plane: the previous value is READ also where the lerp
    factor is 0, so a planted NaN or infinity comes out NaN at frame 0 while every other pixel is the frame's colour byte for
    byte; a previous 3e38, -0 or subnormal goes through the statement's arithmetic; .w of the tile and of the moments comes back bit
    for bit (a signalling NaN's pattern included, compared as int32); a guide plane of the fold is blended in all four channels;
    the mirror receives the blended pixel with that alpha;
  - the adaptive blend with the running sample count S at 0, below 1, 1, 2^24, FLT_MAX, infinities, NaN, negative and subnormal,
    under counts of 0, 1, 7, 2047, beyond the clamp on both sides: against the C checker started from the planted planes and
    against the numpy statement over the device's own frame colours;
  - the plan kernel where m.x*m.x underflows or overflows, where b is 0, negative or its square subnormal, where the variance is
    inf - inf, where te*te is subnormal or 0, and with `extra` exactly on minSamples, maxSamples and an integer and one ulp beside them;
  - the spread kernel where e1*e1 and w*m underflow or overflow, at the sigmas' accepted ends with guides whose squared differences
    overflow, and at the ends of samplesPerFrame and minSamples; what the call refuses beyond them writes nothing.

Byte for byte everywhere; value_ranges_lib.same_bits (NaN positions equal, every other element byte-equal) only where the reference
holds a NaN.  tests/test_resolve_ranges.py proves on the CPU that every case lies where it says."""
import ctypes as C

import numpy as np
import pytest

import resolve_ranges_lib as lib
from adaptive_lib import AdaptiveChecker, plan_numpy
from batch_moments_lib import blend, fold_frames, lerp_factor
from oracle_lib import FLAG_PROGRESSIVE
from resolve_ranges_lib import u32
from spatial_variance_lib import RADII, SpatialVarianceChecker, spatial_variance_numpy
from test_gpu_adaptive import dev_counts, run_plan
from test_gpu_spatial_variance import estimate
from test_gpu_temporal import dev, plane
from value_ranges_lib import same_bits

pytestmark = pytest.mark.gpu
W, H = lib.RESOLVE_SIZE
FLAGS = [FLAG_PROGRESSIVE, 0]
FLAG_IDS = ["progressive", "each-frame-its-own"]


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    built = {}

    def get(cls):
        if cls not in built:
            built[cls] = cls(tmp_path_factory.mktemp(cls.__name__))
        return built[cls]
    return get


def same(got, want):
    """byte for byte; same_bits where the reference holds a NaN"""
    return same_bits(got, want) if np.isnan(want).any() else got.tobytes() == want.tobytes()


def bits_of(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---------------------------------------------------------------- 1. the display conversion
@pytest.mark.parametrize("size", lib.DISPLAY_SIZES, ids=lambda s: "%dx%d" % s)
def test_display_conversion(tpt_defaults, size):
    import torch
    tpt = tpt_defaults
    w, h = size
    tile = lib.display_plane(w, h)
    d_tile = dev(tile)
    out = torch.full((w * h * 4 + lib.DISPLAY_TAIL,), lib.DISPLAY_SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    tpt.display_rgba8(d_tile.data_ptr(), w, h, out.data_ptr())
    tpt.synchronize()
    got = out.cpu().numpy()
    assert (got[w * h * 4:] == lib.DISPLAY_SENTINEL).all(), "written behind the image"
    assert bits_of(d_tile.cpu().numpy()).tobytes() == bits_of(tile).tobytes(), "the input was written"
    image, want = got[:w * h * 4].reshape(h, w, 4), lib.display_numpy(tile)
    assert (image[..., 3] == 255).all(), "alpha"
    wrong = image[..., :3] != want[..., :3]
    if wrong.any():
        src = tile[::-1, :, :3]
        seen = sorted({(hex(int(b)), int(g), int(e)) for b, g, e in zip(src[wrong].view(u32), image[..., :3][wrong], want[..., :3][wrong])})
        raise AssertionError("%d channels differ from the statement; (the input's bits, got, want): %r" % (wrong.sum(), seen[:12]))


# ---------------------------------------------------------------- 2. the blends
_traced = {}


def traced(tpt):
    """frames 0 .. 9 of the default scene at 37 x 21, RESOLVE_SPP samples: what a draw without the progressive flag leaves in zeroed
    planes (lerp 0: 0*0 + c*1 == c) -> {frame: (colour, moments, albedo, normal / depth)}, traced once and shared"""
    if not _traced:
        tpt.set_samples_per_pixel(lib.RESOLVE_SPP)
        try:
            for f in range(10):
                t = [plane(H, W), plane(H, W), plane(H, W, float("nan")), plane(H, W, float("nan"))]
                tpt.UpdateTest(0.0, f, W, H, 0)
                tpt.draw_device_moments(0.0, f, W, H, t[0].data_ptr(), t[1].data_ptr(), 0, albedo_ptr=t[2].data_ptr(), normal_depth_ptr=t[3].data_ptr())
                tpt.synchronize()
                _traced[f] = tuple(x.cpu().numpy() for x in t)
                assert all(np.isfinite(x).all() for x in _traced[f]) and (_traced[f][0][..., :3].view(u32) != lib.SIGN).all()
        finally:
            tpt.set_samples_per_pixel(4)
        assert _traced[0][0][..., :3].max() > 0.5 and not np.array_equal(_traced[0][0], _traced[1][0])
    return _traced


def check_kept_w(got, start, what):
    assert bits_of(got[..., 3]).tobytes() == bits_of(start[..., 3]).tobytes(), "%s: .w was rewritten" % what


def check_only_the_poison_shows(got, where, colour, what):
    """the lerp factor was 0: NaN exactly where the previous value was NaN or infinite, the frame's colour byte for byte elsewhere"""
    poison = lib.poisoned(where)
    assert np.array_equal(np.isnan(got[..., :3]), poison), "%s: a non-finite previous value did not propagate at a lerp factor of 0" % what
    assert got[..., :3][~poison].tobytes() == colour[..., :3][~poison].tobytes(), "%s: a finite previous value changed the frame" % what


@pytest.mark.parametrize("mirror", [False, True], ids=["plain", "mirror"])
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("frame", lib.RESOLVE_FRAMES)
def test_draw_device_reads_the_tile_it_blends_into(tpt_defaults, frame, flags, mirror):
    import torch
    tpt = tpt_defaults
    colour = traced(tpt)[frame][0]
    start, where = lib.planted_plane(1)
    want = blend(start.copy(), colour, lerp_factor(frame, flags), 3)
    tile = dev(start)
    mbuf = torch.full((H + 1, W, 4), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tpt.set_samples_per_pixel(lib.RESOLVE_SPP)
    try:
        if mirror:
            tpt.set_tile_mirror(mbuf.data_ptr(), mbuf[H].data_ptr())
        tpt.UpdateTest(0.0, frame, W, H, flags)
        tpt.draw_device(0.0, frame, W, H, tile.data_ptr(), flags)
        tpt.synchronize()
    finally:
        tpt.set_tile_mirror(None)
        tpt.set_samples_per_pixel(4)
    got = tile.cpu().numpy()
    assert same(got[..., :3], want[..., :3]), "the tile differs from the statement"
    check_kept_w(got, start, "tile")
    if lerp_factor(frame, flags) == 0:
        check_only_the_poison_shows(got, where, colour, "frame %d" % frame)
    if mirror:
        assert bits_of(mbuf[:H].cpu().numpy()).tobytes() == bits_of(got).tobytes(), "the mirror is not the blended tile, alpha included"
    else:
        assert bool((mbuf == -1.0).all())


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("first", [0, 5])
def test_draw_device_batch_reads_the_tile_it_blends_into(tpt_defaults, first, flags):
    import torch
    tpt = tpt_defaults
    frames = traced(tpt)
    start, where = lib.planted_plane(1)
    want, clean = start.copy(), np.zeros_like(start)
    for f in range(first, first + 3):
        blend(want, frames[f][0], lerp_factor(f, flags), 3)
        blend(clean, frames[f][0], lerp_factor(f, flags), 3)
    tile = dev(start)
    torch.cuda.synchronize()
    tpt.set_samples_per_pixel(lib.RESOLVE_SPP)
    try:
        tpt.UpdateTest(0.0, first, W, H, flags)
        tpt.draw_device_batch(0.0, first, 3, W, H, tile.data_ptr(), flags)
        tpt.synchronize()
    finally:
        tpt.set_samples_per_pixel(4)
    got = tile.cpu().numpy()
    assert same(got[..., :3], want[..., :3]), "the tile differs from the statement"
    check_kept_w(got, start, "tile")
    if first == 0 or not flags:  # a lerp factor of 0 in the batch: the poison shows, every other pixel is the clean batch's
        check_only_the_poison_shows(got, where, clean, "3 frames from %d" % first)


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("n", [3, 5])
def test_draw_device_batch_moments_reads_the_planes_it_folds_into(tpt_defaults, n, first, flags):
    """3 frames: the remainder of the loop unrolled by four alone; 5: one pass of it and one frame of the remainder"""
    import torch
    tpt = tpt_defaults
    frames = traced(tpt)
    planted = [lib.planted_plane(1), lib.planted_plane(2), lib.planted_plane(3, 4), lib.planted_plane(4, 4)]
    start = [p for p, _ in planted]
    want = fold_frames(*[p.copy() for p in start], [frames[f] for f in range(first, first + n)], first, flags)
    planes = [dev(p) for p in start]
    torch.cuda.synchronize()
    tpt.set_samples_per_pixel(lib.RESOLVE_SPP)
    try:
        tpt.UpdateTest(0.0, first, W, H, flags)
        tpt.draw_device_batch_moments(0.0, first, n, W, H, planes[0].data_ptr(), planes[1].data_ptr(), flags, albedo_ptr=planes[2].data_ptr(),
                                      normal_depth_ptr=planes[3].data_ptr())
        tpt.synchronize()
    finally:
        tpt.set_samples_per_pixel(4)
    got = [p.cpu().numpy() for p in planes]
    for k, name in enumerate(("tile", "moments")):
        assert same(got[k][..., :3], want[k][..., :3]), "%s differs from the statement" % name
        check_kept_w(got[k], start[k], name)
    for k, name in ((2, "albedo"), (3, "normal / depth")):
        assert same(got[k], want[k]), "%s differs from the statement (all four channels are blended)" % name
    if first == 0 or not flags:
        for k in range(4):
            ch = 3 if k < 2 else 4
            assert np.array_equal(np.isnan(got[k][..., :ch]), lib.poisoned(planted[k][1], ch)), "plane %d: the poison at a lerp factor of 0" % k


def adaptive_draw(tpt, frame, flags, tile, moments, counts):
    import torch
    t, m, c = dev(tile), dev(moments), dev_counts(counts)
    torch.cuda.synchronize()
    tpt.UpdateTest(0.0, frame, W, H, flags)
    tpt.draw_device_adaptive(0.0, frame, W, H, t.data_ptr(), m.data_ptr(), c.data_ptr(), flags)
    tpt.synchronize()
    assert c.cpu().numpy().tobytes() == counts.tobytes(), "the counts were written"
    return t.cpu().numpy(), m.cpu().numpy()


@pytest.mark.parametrize("frame,progressive", lib.ADAPTIVE_DRAWS, ids=["frame0-progressive", "frame1-progressive", "frame5-alone"])
def test_draw_device_adaptive_across_the_running_sample_counts(tpt_defaults, checkers, oracle, frame, progressive):
    tpt = tpt_defaults
    tile, moments, counts = lib.adaptive_case()
    flags = FLAG_PROGRESSIVE if progressive else 0
    got = adaptive_draw(tpt, frame, flags, tile, moments, counts)
    # the C checker, started from the planted planes
    spheres, mats = oracle.default_scene()
    _, bb, mo, _, _ = checkers(AdaptiveChecker).render(spheres, mats, oracle.default_camera(W, H), W, H, counts, frame, flags,
                                                       backbuffer=tile.copy(), moments=moments.copy())
    assert same(got[0], bb) and same(got[1], mo), "differs from the checker"
    check_kept_w(got[0], tile, "tile")
    # the numpy statement over the device's own frame: what the draw leaves in zeroed planes without the flag
    colour, staged = adaptive_draw(tpt, frame, 0, np.zeros_like(tile), np.zeros_like(moments), counts)
    want = lib.adaptive_blend_numpy(tile, moments, colour, staged, counts, progressive)
    assert same(got[0], want[0]) and same(got[1], want[1]), "differs from the numpy statement"
    untraced = lib.clamped(counts) == 0
    assert bits_of(got[0][untraced]).tobytes() == bits_of(tile[untraced]).tobytes(), "a pixel with a count of 0 was written"
    assert bits_of(got[1][untraced]).tobytes() == bits_of(moments[untraced]).tobytes(), "a pixel with a count of 0 was written"


# ---------------------------------------------------------------- 3. the plan kernel
def check_plan(tpt, checker, mo, arguments, what):
    for te, lo, hi in arguments:
        counts, var, total = run_plan(tpt, mo, te, lo, hi)
        for name, (wc, wv, wt) in (("checker", checker.plan(mo, te, lo, hi)), ("numpy statement", plan_numpy(mo, te, lo, hi))):
            where = "%s, targetError %g, %d..%d: differs from the %s" % (what, te, lo, hi, name)
            assert counts.tobytes() == wc.tobytes(), where + " (%d counts)" % (counts != wc).sum()
            assert same(var, wv) and total == wt, where
    return counts


@pytest.mark.parametrize("k", lib.PLAN_SCALES)
def test_plan_on_scaled_moments(tpt_defaults, checkers, k):
    for kind in ("valid", "mixed"):
        for w, h in lib.PLAN_SIZES:
            check_plan(tpt_defaults, checkers(AdaptiveChecker), lib.plan_scaled_case(kind, w, h, k), lib.PLAN_ARGUMENTS, "%s %dx%d" % (kind, w, h))


@pytest.mark.parametrize("size", lib.PLAN_SIZES, ids=lambda s: "%dx%d" % s)
def test_plan_on_planted_pixels(tpt_defaults, checkers, size):
    w, h = size
    case = lib.plan_flat_case(w, h)
    planes = {name: mo for name, (mo, _) in case.items()} if size == (1, 1) else {"flat": case[0]}
    for name, mo in planes.items():
        check_plan(tpt_defaults, checkers(AdaptiveChecker), mo, lib.PLAN_ARGUMENTS + [(0.05, 1, 2047)], name)


def test_plan_on_the_boundaries_of_the_count(tpt_defaults, checkers):
    lo, mid, hi, seconds = lib.plan_boundary_cases()
    want = dict(zip(lib.BOUNDARY_NAMES, (lo, lo + 1, mid, mid + 1, hi, hi)))
    for w, h in lib.PLAN_SIZES[1:]:
        for name in lib.BOUNDARY_NAMES:
            mo = lib.flat(h, w, lib.BOUNDARY_MEAN, seconds[name], lib.BOUNDARY_S)
            counts = check_plan(tpt_defaults, checkers(AdaptiveChecker), mo, [(lib.BOUNDARY_TE, lo, hi)], name)
            assert (counts[1:-1, 1:-1] == want[name]).all(), name


# ---------------------------------------------------------------- 4. the spread kernel
def check_spread(tpt, checker, m, nd, what, **kw):
    w, h = m.shape[1], m.shape[0]
    dm, dn = dev(m), None if nd is None else dev(nd)
    got = estimate(tpt, w, h, dm, dn, **kw)
    tpt.synchronize()
    got = got.cpu().numpy()
    for name, want in (("checker", checker.run(m, nd, **kw)), ("numpy statement", spatial_variance_numpy(m, nd, **kw))):
        assert same(got, want), "%s, %r: differs from the %s" % (what, kw, name)
    assert bits_of(dm.cpu().numpy()).tobytes() == bits_of(m).tobytes() and (nd is None or bits_of(dn.cpu().numpy()).tobytes() == bits_of(nd).tobytes()), \
        "an input was written"


@pytest.mark.parametrize("k", lib.SPREAD_SCALES)
def test_spread_on_scaled_moments(tpt_defaults, checkers, k):
    for kind in lib.SPREAD_KINDS:
        for w, h in lib.SPREAD_SIZES:
            m, nd = lib.spread_scaled_case(kind, w, h, k)
            for radius in RADII:
                check_spread(tpt_defaults, checkers(SpatialVarianceChecker), m, None, "%s %dx%d" % (kind, w, h), radius=radius)
                check_spread(tpt_defaults, checkers(SpatialVarianceChecker), m, nd, "%s %dx%d" % (kind, w, h), radius=radius, **lib.SPREAD_GUIDE)


@pytest.mark.parametrize("sigmas", lib.SPREAD_SIGMA_CASES, ids=lambda s: "%g_%g" % s)
def test_spread_at_the_sigma_ends_with_an_extreme_guide(tpt_defaults, checkers, sigmas):
    for w, h in lib.SPREAD_SIZES:
        m, nd = lib.spread_guide_case(w, h)
        for radius in RADII:
            check_spread(tpt_defaults, checkers(SpatialVarianceChecker), m, nd, "%dx%d" % (w, h), radius=radius, sigma_normal=sigmas[0],
                         sigma_depth=sigmas[1], min_samples=float("inf"))


def test_spread_at_the_ends_of_its_counts(tpt_defaults, checkers):
    for w, h in lib.SPREAD_SIZES:
        m, nd = lib.spread_guide_case(w, h)
        for kw in lib.SPREAD_COUNT_ENDS:
            check_spread(tpt_defaults, checkers(SpatialVarianceChecker), m, nd, "%dx%d" % (w, h), radius=2, **lib.SPREAD_GUIDE, **kw)


def test_spread_refuses_the_ends_beyond_its_contract(tpt_defaults):
    """sigmas of 1e-20 .. 1e20, a subnormal minSamples, samplesPerFrame below 1: refused before a kernel runs, nothing written"""
    import torch
    tpt = tpt_defaults
    w, h = 65, 9
    m, nd = (dev(a) for a in lib.spread_guide_case(w, h))
    out = plane(h, w, float("nan"))
    torch.cuda.synchronize()
    call = tpt.load_library().tptSpatialVarianceDevice
    refused = []
    for s in lib.SPREAD_REFUSED_SIGMAS:
        refused += [dict(sigma_normal=s), dict(sigma_depth=s), dict(sigma_normal=s, sigma_depth=s)]
    for kw in refused + list(lib.SPREAD_REFUSED_COUNTS):
        a = dict(dict(samples_per_frame=1.0, min_samples=2.0, sigma_normal=0.03, sigma_depth=0.5), **kw)
        rc = call(w, h, 1, C.c_void_p(m.data_ptr()), C.c_void_p(nd.data_ptr()), C.c_void_p(out.data_ptr()), C.c_float(a["samples_per_frame"]),
                  C.c_float(a["min_samples"]), 2, C.c_float(a["sigma_normal"]), C.c_float(a["sigma_depth"]))
        assert rc != 0 and "tptSpatialVarianceDevice" in tpt.load_library().tptGetLastError().decode(), kw
    tpt.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote its output"
