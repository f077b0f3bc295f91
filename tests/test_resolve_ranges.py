"""The catalogue of tests/resolve_ranges_lib.py without a GPU: every case lies where its name says, proven from the numpy statements
first and the C checkers second.  These are the conditions that keep tests/test_gpu_resolve_ranges.py from passing vacuously:

  - display: each of the 255 steps of the conversion is straddled by its two planted values; the specials convert as the contract of
    include/tpt_hip.h says (NaN, negatives and both zeros 0, +inf 255); the statement equals the reference formula's where that one
    is defined; the plane is not symmetric top to bottom, holds every value and garbage in alpha;
  - the blends: every planted value sits in at least a dozen pixels, some in the last partial workgroup; 0*0 + c*1 == c on float32 for
    every c but -0; at a lerp factor of 0 exactly the pixels whose previous value was NaN or an infinity come out NaN and every other
    one is the frame's colour byte for byte; .w comes back as bits; the adaptive blend's numpy statement equals the C checker on the
    planted planes (same_bits) and the stated ends of S are where they are said to be;
  - the plan function: per scale, the share of pixels whose m.x*m.x, b*b underflow or overflow; every planted pixel of the flat
    plane on its side of its branch; the six boundary values of `extra` exactly, and the counts they give; where te*te lies;
  - the spread function: the shares of underflowing and overflowing e1*e1 / S2, the windows without a counting tap per sigma
    case, and what the statement refuses;
  - the C checker and the numpy statement agree on every case.

Every share is printed (pytest -s) at the committed seeds."""
import numpy as np
import pytest

import resolve_ranges_lib as lib
from adaptive_lib import LUM_FLOOR, AdaptiveChecker, plan_numpy
from batch_moments_lib import blend, fold_frames, lerp_factor
from oracle_lib import FLAG_PROGRESSIVE
from resolve_ranges_lib import bits, f32, u32
from spatial_variance_lib import RADII, SpatialVarianceChecker, spatial_variance_numpy
from value_ranges_lib import same_bits

TINY = np.finfo(np.float32).tiny  # the smallest normal


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return AdaptiveChecker(tmp_path_factory.mktemp("adaptive_checker"))


@pytest.fixture(scope="module")
def spread_checker(tmp_path_factory):
    return SpatialVarianceChecker(tmp_path_factory.mktemp("spatial_variance_checker"))


def subnormal_or_zero(x):
    with np.errstate(all="ignore"):
        return np.abs(x) < TINY


# ---------------------------------------------------------------- 1. display
def test_every_step_of_the_conversion_is_straddled():
    steps = lib.display_steps()
    below = np.nextafter(steps, f32(0))
    k = np.arange(1, 256)
    assert (lib.display_level(steps) == k).all() and (lib.display_level(below) == k - 1).all()
    assert (np.diff(steps) > 0).all() and steps[0] > 0 and steps[-1] == f32(1)
    with np.errstate(all="ignore"):  # said once more without the statement: the truncated product on both sides
        assert (np.trunc(np.sqrt(steps) * f32(255)) >= k).all() and (np.trunc(np.sqrt(below) * f32(255)) == k - 1).all()
    values = lib.display_values()
    assert len(values) == len(lib.display_specials()) + 510 and values.dtype == np.float32


def test_the_specials_convert_as_the_contract_says():
    want = {"nan": 0, "-nan": 0, "nan payload": 0, "snan": 0, "-snan": 0, "-1": 0, "-1e-45": 0, "-3e38": 0, "-inf": 0, "+0": 0, "-0": 0,
            "1e-45": 0, "2^-127": 0, "below 2^-96": 0, "2^-96": 0, "above 2^-96": 0, "below 1": 254, "1": 255, "above 1": 255, "4": 255,
            "below 2^96": 255, "2^96": 255, "above 2^96": 255, "3e38": 255, "+inf": 255}
    specials = lib.display_specials()
    assert set(want) == set(specials)
    for name, v in specials.items():
        assert int(lib.display_level(v)) == want[name], name
    for name, pattern in (("nan", lib.QUIET_NAN), ("snan", lib.SIGNALLING_NAN), ("-snan", lib.SIGN | lib.SIGNALLING_NAN), ("-0", lib.SIGN)):
        assert specials[name].view(u32) == pattern, name
    assert subnormal_or_zero(specials["1e-45"]) and subnormal_or_zero(specials["2^-127"]) and specials["2^-127"] > 0


def test_the_statement_is_the_reference_formula_where_that_is_defined():
    rng = np.random.default_rng(3)
    tile = (rng.random((19, 23, 4), dtype=f32) ** f32(3) * f32(4)).astype(f32)
    tile[rng.random((19, 23)) < 0.2, :3] = 0
    old = np.empty(tile.shape, np.uint8)
    old[..., :3] = np.minimum(np.sqrt(tile[::-1, :, :3]) * f32(255), f32(255.0)).astype(np.uint8)
    old[..., 3] = 255
    assert np.array_equal(lib.display_numpy(tile), old)


@pytest.mark.parametrize("size", lib.DISPLAY_SIZES, ids=lambda s: "%dx%d" % s)
def test_display_planes(size):
    w, h = size
    plane = lib.display_plane(w, h)
    assert (w * h) % 256 != 0, "a whole number of workgroups: the bounds test would decide nothing"
    values = lib.display_values()
    held = plane[..., :3].reshape(-1).view(u32)
    assert np.array_equal(held[:len(values)], values.view(u32)[:held.size])
    if 3 * w * h >= len(values):
        assert set(held.tolist()) == set(values.view(u32).tolist())
    alpha = plane[..., 3].reshape(-1)
    assert np.isnan(alpha[0]) and (w * h < 3 or (alpha[1] == -1 and alpha[2] == f32(1e30)))
    out = lib.display_numpy(plane)
    assert (out[..., 3] == 255).all()
    if h > 1:
        assert not np.array_equal(out, lib.display_numpy(plane[::-1])), "symmetric top to bottom: a missing row flip would pass"
    if (w, h) == (130, 67):
        assert (w * h) // 256 == 34 and (w * h) % 256 == 6
        assert set(out[..., :3].reshape(-1).tolist()) == set(range(256))


# ---------------------------------------------------------------- 2. the blends
def colour_plane(seed):
    """a stand-in for a frame's colour: rand^3 * 4 with a fifth of the pixels black (what the tracer gives: no negative zero)"""
    w, h = lib.RESOLVE_SIZE
    rng = np.random.default_rng([seed, 5])
    c = (rng.random((h, w, 4), dtype=f32) ** f32(3) * f32(4)).astype(f32)
    c[rng.random((h, w)) < 0.2] = 0
    return c


@pytest.mark.parametrize("channels", [3, 4])
def test_planted_planes_hold_what_they_say(channels):
    w, h = lib.RESOLVE_SIZE
    assert w * h == 777 and lib.LAST_WORKGROUP == 3 * 256
    plane, where = lib.planted_plane(7, channels)
    flat = plane.reshape(-1, 4).view(u32)
    for name, value in lib.PLANTED.items():
        px, ch = where[name]
        assert len(set(px.tolist())) == len(px) >= lib.PER_VALUE + 1 and (px >= lib.LAST_WORKGROUP).sum() >= 1, name
        assert (flat[px, ch] == value.view(u32)).all() and (ch < channels).all() and len(set(ch.tolist())) == channels, name
    if channels == 3:
        for pattern in lib.ALPHA_BITS:
            px, _ = where["alpha %08x" % pattern]
            assert len(px) >= lib.PER_VALUE + 1 and (px >= lib.LAST_WORKGROUP).sum() >= 1 and (flat[px, 3] == pattern).all()
    everything = np.concatenate([p for p, _ in where.values()])
    assert channels == 3 or len(set(everything.tolist())) == len(everything), "two values in one pixel"
    assert lib.poisoned(where, channels).sum() == sum(len(where[n][0]) for n in lib.POISON)
    assert bits(lib.PAYLOAD_NAN) != bits(lib.PAYLOAD_NAN) and bits(lib.SIGNALLING_NAN) != bits(lib.SIGNALLING_NAN)  # (NaNs both)


def test_a_frame_s_colour_is_what_a_draw_into_zeros_leaves():
    """0*0 + c*1 == c, bit for bit, for every float32 c but -0 (and a NaN's payload): how the GPU tests take a frame's colour plane"""
    rng = np.random.default_rng(11)
    c = np.concatenate([rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(u32).view(f32),
                        np.array([0.0, 1e-45, 2.0 ** -127, 3e38, np.inf, -np.inf, -1e-45], f32)])
    c = c[~np.isnan(c) & (c.view(u32) != lib.SIGN)]
    with np.errstate(all="ignore"):
        got = f32(0) * f32(0) + c * (f32(1) - f32(0))
    assert got.tobytes() == c.tobytes()
    assert (f32(0) * f32(0) + f32(-0.0) * f32(1)).view(u32) == 0  # -0 comes back +0: the tracer's colours hold none
    assert lerp_factor(0, FLAG_PROGRESSIVE) == 0 and all(lerp_factor(f, 0) == 0 for f in lib.RESOLVE_FRAMES)
    assert lerp_factor(1, FLAG_PROGRESSIVE) == f32(0.5) and lerp_factor(5, FLAG_PROGRESSIVE) == f32(5) / f32(6)


def test_at_a_lerp_factor_of_0_only_the_poison_shows():
    """the assertion that carries blendPixel's contract: prev is read also when lerpFac == 0"""
    tile, where = lib.planted_plane(1)
    colour = colour_plane(1)
    got = blend(tile.copy(), colour, lerp_factor(0, FLAG_PROGRESSIVE), 3)
    poison = lib.poisoned(where)
    assert np.array_equal(np.isnan(got[..., :3]), poison) and poison.sum() >= 3 * (lib.PER_VALUE + 1)
    assert got[..., :3][~poison].tobytes() == colour[..., :3][~poison].tobytes()
    assert got[..., 3].view(np.int32).tobytes() == tile[..., 3].view(np.int32).tobytes(), "alpha was touched"
    # later frames: a huge value stays finite, a subnormal and -0 vanish into the colour's rounding, the poison stays
    for f in (1, 5):
        got = blend(tile.copy(), colour, lerp_factor(f, FLAG_PROGRESSIVE), 3)
        assert np.array_equal(~np.isfinite(got[..., :3]), poison)
    # a kernel that skipped the read would give the colour everywhere:
    assert not same_bits(blend(tile.copy(), colour, 0.0, 3)[..., :3], colour[..., :3])


def test_the_fold_poisons_every_channel_of_a_guide_and_keeps_w_of_the_tile_and_the_moments():
    planes = [lib.planted_plane(1)[0], lib.planted_plane(2)[0], lib.planted_plane(3, 4)[0], lib.planted_plane(4, 4)[0]]
    wheres = [lib.planted_plane(1)[1], lib.planted_plane(2)[1], lib.planted_plane(3, 4)[1], lib.planted_plane(4, 4)[1]]
    for n in (3, 5):
        frames = [tuple(colour_plane(10 * j + k) for k in range(4)) for j in range(n)]
        got = fold_frames(*[p.copy() for p in planes], frames, 0, FLAG_PROGRESSIVE)
        for k in (0, 1):
            assert got[k][..., 3].view(np.int32).tobytes() == planes[k][..., 3].view(np.int32).tobytes()
            assert np.array_equal(np.isnan(got[k][..., :3]), lib.poisoned(wheres[k]))
        for k in (2, 3):
            assert np.array_equal(np.isnan(got[k]), lib.poisoned(wheres[k], 4)) and np.isnan(got[k][..., 3]).sum() >= lib.PER_VALUE // 4
    assert n % 4 == 1 and 3 < 4, "5 frames: the loop unrolled by four and one frame of its remainder; 3: the remainder alone"


def test_adaptive_case_and_the_ends_of_S(checker, oracle):
    w, h = lib.RESOLVE_SIZE
    tile, moments, counts = lib.adaptive_case()
    n = lib.clamped(counts)
    per_draw = int(n.sum())
    total = per_draw * len(lib.ADAPTIVE_DRAWS)
    print("adaptive case: %d samples a draw, %d in the %d draws" % (per_draw, total, len(lib.ADAPTIVE_DRAWS)))
    assert per_draw == 13515 and total == 40545 <= lib.ADAPTIVE_MOST_SAMPLES
    flat_counts, S = counts.reshape(-1), moments[..., 3].reshape(-1)
    for c in lib.ADAPTIVE_COUNTS_COMMON + lib.ADAPTIVE_COUNTS_FEW:
        assert (flat_counts == c).sum() >= 2 and (flat_counts[lib.LAST_WORKGROUP:] == c).any(), c
    for s in lib.ADAPTIVE_S:  # every S under a traced and under an untraced pixel
        at = np.isnan(S) if s != s else S == f32(s)
        assert (n.reshape(-1)[at] > 0).any() and (n.reshape(-1)[at] == 0).any(), s
    assert len({float(S[i]) for i in np.flatnonzero(n.reshape(-1) == 2047)}) >= 5
    # the ends, on float32
    assert f32(2.0 ** 24) + f32(1) == f32(2.0 ** 24) and f32(2.0 ** 24) + f32(7) > f32(2.0 ** 24)
    big = f32(3.4028235e38)
    assert big == lib.FLT_MAX and np.isfinite(big + f32(2047)) and big / (big + f32(2047)) == f32(1)
    assert f32(0.999) < 1 and 0 < f32(1e-40) < TINY
    # the numpy statement against the C checker, from the planted planes: the frame's colour and staged moments are what the checker
    # leaves in zeroed planes without the progressive flag (lerp = 0 / n)
    spheres, mats = oracle.default_scene()
    cam = oracle.default_camera(w, h)
    for frame, progressive in lib.ADAPTIVE_DRAWS:
        flags = FLAG_PROGRESSIVE if progressive else 0
        _, colour, staged, _, _ = checker.render(spheres, mats, cam, w, h, counts, frame, 0)
        assert (staged[..., 3] == n).all() and np.isfinite(colour).all() and (colour.view(u32) != lib.SIGN).all()
        _, bb, mo, _, _ = checker.render(spheres, mats, cam, w, h, counts, frame, flags, backbuffer=tile.copy(), moments=moments.copy())
        want = lib.adaptive_blend_numpy(tile, moments, colour, staged, counts, progressive)
        assert same_bits(bb, want[0]) and same_bits(mo, want[1]), (frame, progressive)
        assert bb[..., 3].view(np.int32).tobytes() == tile[..., 3].view(np.int32).tobytes(), "alpha was touched"
        untraced = n == 0
        assert bb[untraced].tobytes() == tile[untraced].tobytes() and mo[untraced].tobytes() == moments[untraced].tobytes()
        Sv = moments[..., 3]
        valid = progressive & (Sv >= 1) & (Sv <= lib.FLT_MAX)
        assert (mo[..., 3][~untraced & ~valid] == n[~untraced & ~valid]).all()
        if progressive:  # S = FLT_MAX: lerp is 1 and the tile keeps its values, infinities included (inf * 1 + c * 0); a -0 comes back +0
            kept = ~untraced & (Sv == big)
            assert kept.sum() >= 10 and np.array_equal(bb[kept][:, :3], tile[kept][:, :3], equal_nan=True)


# ---------------------------------------------------------------- 3. the plan function
@pytest.mark.parametrize("k", lib.PLAN_SCALES)
def test_plan_scaled_planes_lie_where_their_scale_says(checker, k):
    for kind in ("valid", "mixed"):
        for w, h in lib.PLAN_SIZES:
            mo = lib.plan_scaled_case(kind, w, h, k)
            with np.errstate(all="ignore"):
                mm = mo[..., 0] * mo[..., 0]
                b = mo[..., 0] + LUM_FLOOR
                bb = b * b
            shares = dict(mm_tiny=float(subnormal_or_zero(mm).mean()), mm_inf=float(np.isinf(mm).mean()), bb_tiny=float(subnormal_or_zero(bb).mean()),
                          bb_inf=float(np.isinf(bb).mean()))
            if (w, h) == (37, 21):
                print("plan, %s, k = %d: m.x*m.x subnormal or zero %.3f, infinite %.3f; b*b subnormal %.3f, infinite %.3f"
                      % (kind, k, shares["mm_tiny"], shares["mm_inf"], shares["bb_tiny"], shares["bb_inf"]))
                if k == -70:
                    assert shares["mm_tiny"] > 0.5 and shares["mm_inf"] == 0
                elif k == -50:
                    assert shares["mm_tiny"] < 0.5 and shares["mm_inf"] == 0
                elif k == 63:
                    assert 0.1 < shares["mm_inf"] < 1 and shares["bb_inf"] == shares["mm_inf"]
                else:
                    assert shares["mm_inf"] == 0 and (k != 50 or np.isinf(mo[..., 1]).mean() < 0.5)
                assert shares["bb_tiny"] == 0  # the luminance floor does not scale: b*b >= 1e-4 while m.x >= 0 (PLAN_PLANTED goes below)
            for te, lo, hi in lib.PLAN_ARGUMENTS:
                c, v, t = checker.plan(mo, te, lo, hi)
                nc, nv, nt = plan_numpy(mo, te, lo, hi)
                assert c.tobytes() == nc.tobytes() and same_bits(v, nv) and t == nt, (kind, w, h, te, lo, hi)


def test_where_the_squared_target_errors_lie():
    te2 = {te: f32(te) * f32(te) for te in lib.PLAN_TARGETS}
    assert te2[1e6] == f32(1e12) and te2[2e-19] >= TINY
    assert 0 < te2[1e-19] < TINY, "1e-19 squared is 1e-38, below the smallest normal 1.1755e-38"
    assert 0 < te2[1e-22] < TINY and te2[1e-22].view(u32) == 7
    assert te2[1e-23] == 0


@pytest.mark.parametrize("size", lib.PLAN_SIZES, ids=lambda s: "%dx%d" % s)
def test_plan_planted_pixels_lie_on_their_side(checker, size):
    w, h = size
    case = lib.plan_flat_case(w, h)
    cases = case if (w, h) == (1, 1) else {name: (case[0], at) for name, at in case[1].items()}
    te, lo, hi = 0.05, 1, 2047
    for name, (mo, (y, x)) in cases.items():
        counts, _, _, d = plan_numpy(mo, te, lo, hi, details=True)
        mx, my = mo[y, x, 0], mo[y, x, 1]
        with np.errstate(all="ignore"):
            b = mx + LUM_FLOOR
            r = d["r"][y, x]
            if name == "b == 0, var > 0":
                assert b == 0 and my - mx * mx > 0 and r == np.inf and counts[y, x] == hi
            elif name == "b == 0, var == 0":
                assert b == 0 and my - mx * mx == 0 and np.isnan(r) and counts[y, x] == lo
                ys, xs = slice(max(y - 1, 0), y + 2), slice(max(x - 1, 0), x + 2)
                assert np.isnan(d["R"][ys, xs]).all() and (counts[ys, xs] == lo).all(), "the 0/0 poisons its neighbours' R"
            elif name == "mean below the floor":
                assert b < 0 and r > 0 and np.isfinite(r)
            elif name == "second below the squared mean":
                assert my < mx * mx and r == 0
            elif name == "inf - inf":
                assert np.isinf(mx * mx) and np.isnan(my - mx * mx) and r == 0, "a NaN difference is not > 0: the variance is 0"
            elif name == "mean NaN":
                assert np.isnan(r) and d["counted"][y, x] and counts[y, x] == lo
            else:
                assert subnormal_or_zero(mx) and subnormal_or_zero(my) and mx > 0 and my > 0 and mx * mx == 0 and r > 0
        if (w, h) != (1, 1):
            clean = plan_numpy(lib.flat(h, w, **lib.FLAT), te, lo, hi)[0]
            assert lo < clean[h - 1, w - 1] < hi and (counts != clean).any(), "the flat plane itself is on neither bound"
        for args in lib.PLAN_ARGUMENTS + [(te, lo, hi)]:
            c, v, t = checker.plan(mo, *args)
            nc, nv, nt = plan_numpy(mo, *args)
            assert c.tobytes() == nc.tobytes() and same_bits(v, nv) and t == nt, (name, args)


def test_plan_boundaries(checker):
    """the six values of `extra` exactly, from the numpy statement alone, then the counts that `!(extra > lo)`, `extra >= hi` and ceilf give"""
    lo, mid, hi, seconds = lib.plan_boundary_cases()
    assert lo < mid < mid + 1 < hi and f32(lib.BOUNDARY_MEAN) + LUM_FLOOR == lib.BOUNDARY_MEAN, "the floor is absorbed: b*b == m.x*m.x"
    want_extra = dict(zip(lib.BOUNDARY_NAMES, (f32(lo), lib.after(lo), f32(mid), lib.after(mid), lib.after(hi, 0), f32(hi))))
    want_count = dict(zip(lib.BOUNDARY_NAMES, (lo, lo + 1, mid, mid + 1, hi, hi)))
    print("plan boundaries: minSamples %d, %d between, maxSamples %d" % (lo, mid, hi))
    for w, h in lib.PLAN_SIZES[1:]:
        for name in lib.BOUNDARY_NAMES:
            mo = lib.flat(h, w, lib.BOUNDARY_MEAN, seconds[name], lib.BOUNDARY_S)
            counts, _, _, d = plan_numpy(mo, lib.BOUNDARY_TE, lo, hi, details=True)
            inner = d["extra"][1:-1, 1:-1]
            assert inner.size > 0 and (inner.view(u32) == want_extra[name].view(u32)).all(), name
            e = want_extra[name]
            by_hand = lo if not e > f32(lo) else hi if e >= f32(hi) else int(np.ceil(e))
            assert by_hand == want_count[name] and (counts[1:-1, 1:-1] == by_hand).all(), name
            c, v, t = checker.plan(mo, lib.BOUNDARY_TE, lo, hi)
            assert c.tobytes() == counts.tobytes() and t == int(counts.sum()), name


# ---------------------------------------------------------------- 4. the spread function
def both_statements(spread_checker, m, nd, **kw):
    want, d = spatial_variance_numpy(m, nd, details=True, **kw)
    assert same_bits(spread_checker.run(m, nd, **kw), want), kw
    return want, d


@pytest.mark.parametrize("k", lib.SPREAD_SCALES)
def test_spread_scaled_planes_lie_where_their_scale_says(spread_checker, k):
    for kind in lib.SPREAD_KINDS:
        for w, h in lib.SPREAD_SIZES:
            m, nd = lib.spread_scaled_case(kind, w, h, k)
            for radius in RADII:
                for guide in (None, nd):
                    kw = dict(radius=radius, **(lib.SPREAD_GUIDE if guide is not None else {}))
                    _, d = both_statements(spread_checker, m, guide, **kw)
                    if (w, h) != (130, 67) or guide is None:
                        continue
                    est = d["est"] & d["any"]
                    with np.errstate(all="ignore"):
                        ee = d["e1"] * d["e1"]
                    tiny, huge = float(subnormal_or_zero(ee)[est].mean()), float((np.isinf(ee) | np.isinf(d["S2"]))[est].mean())
                    print("spread, %s, k = %d, radius %d: %d estimated pixels, e1*e1 subnormal or zero in %.3f, e1*e1 or S2 infinite in %.3f"
                          % (kind, k, radius, est.sum(), tiny, huge))
                    assert est.sum() > 1000
                    if k == -70:
                        assert tiny > 0.5
                    elif k == 63:
                        assert 0.1 < huge < 1 and tiny == 0
                    else:  # (-50: squares of 2^-100, still normal; 50: squares of 2^100, and the block near 1e20 has an infinite second
                        assert tiny < 0.01 and huge == 0  # moment, which does not count: the overflow begins further out, at 63)


@pytest.mark.parametrize("sigmas", lib.SPREAD_SIGMA_CASES, ids=lambda s: "%g_%g" % s)
def test_spread_sigma_ends_and_the_extreme_guide(spread_checker, sigmas):
    sn, sd = sigmas
    for w, h in lib.SPREAD_SIZES:
        m, nd = lib.spread_guide_case(w, h)
        for radius in RADII:
            _, d = both_statements(spread_checker, m, nd, radius=radius, sigma_normal=sn, sigma_depth=sd, min_samples=float("inf"))
            if (w, h) != (130, 67):
                continue
            none = int((d["est"] & ~d["any"]).sum())
            print("spread, sigmas %g / %g, radius %d: %d of %d estimated pixels have no counting tap" % (sn, sd, radius, none, d["est"].sum()))
            # a window without a counting tap: the pixel's own moments or guide are not finite (planted by synthetic_case), or -- at a
            # sigma of 0 -- its own normal is 3e38, whose squared difference to ITSELF is 0 but to every neighbour infinite ...
            assert d["est"].all() and 0 < none < 0.1 * d["est"].sum()
    m, nd = lib.spread_guide_case(130, 67)
    with np.errstate(all="ignore"):
        dw = nd[:, 1:43, 3] - nd[:, 0:42, 3]
        assert np.isinf(dw * dw).all() and np.isinf(f32(3e38) * f32(3e38))
        assert np.isnan(f32(np.inf) * f32(0)), "an infinite squared difference times a sigma of 0 (inv2 == 0) is NaN: the tap does not count"
    assert (m[..., 3] == f32(3e38)).sum() >= 800


def test_spread_count_ends(spread_checker):
    w, h = 130, 67
    m, nd = lib.spread_guide_case(w, h)
    huge = m[..., 3] == f32(3e38)
    for kw in lib.SPREAD_COUNT_ENDS:
        want, d = both_statements(spread_checker, m, nd, radius=2, **lib.SPREAD_GUIDE, **kw)
        spf, ms = kw["samples_per_frame"], kw["min_samples"]
        if spf == 2.0:
            assert not d["est"][huge].any(), "2 * 3e38 is infinite: never below minSamples, not even an infinite one"
            assert d["est"][~huge].all() == (ms > 2)
        elif ms == 1.0:
            assert not d["est"].any()
        else:  # FLT_MAX * 1 is finite and below infinity, FLT_MAX * 3e38 is not
            assert d["est"][~huge].all() and not d["est"][huge].any()


def test_spread_refuses_the_ends_beyond_its_contract(spread_checker):
    """a sigma outside {0} and [1e-6, 1e6], a subnormal minSamples and samplesPerFrame below 1 never reach a kernel: the C statement
    refuses them as the call does; the numpy statement takes them and says what they would be"""
    m, nd = lib.spread_guide_case(65, 9)
    for s in lib.SPREAD_REFUSED_SIGMAS:
        for kw in (dict(sigma_normal=s), dict(sigma_depth=s), dict(sigma_normal=s, sigma_depth=s)):
            assert spread_checker.run(m, nd, rc=True, **kw) == -1, kw
    for kw in lib.SPREAD_REFUSED_COUNTS:
        assert spread_checker.run(m, nd, rc=True, **kw) == -1, kw
    for s in lib.SPREAD_SIGMAS:
        assert spread_checker.run(m, nd, rc=True, sigma_normal=s, sigma_depth=s) == 0
    from spatial_variance_lib import inv2
    with np.errstate(all="ignore"):
        assert inv2(1e-20) == np.inf and np.isfinite(inv2(1e-19)) and inv2(1e-19) > f32(1e37) and inv2(1e19) > 0 and inv2(1e20) == 0
    clean_m, clean_nd = lib.spread_scaled_case("all", 65, 9, -12)
    flat_nd = np.ascontiguousarray(np.broadcast_to(f32(1), clean_nd.shape))
    _, at_end = spatial_variance_numpy(clean_m, flat_nd, sigma_normal=1e-20, sigma_depth=1e-20, details=True)
    _, inside = spatial_variance_numpy(clean_m, flat_nd, sigma_normal=1e19, sigma_depth=1e19, details=True)
    # identical guides at inv2 == inf: the centre tap's 0 * inf is NaN, no tap counts, step 0's value passes through
    assert (at_end["est"] & ~at_end["any"]).sum() == at_end["est"].sum() > 0 and (inside["est"] & ~inside["any"]).sum() == 0
