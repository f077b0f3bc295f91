"""TEST INFRASTRUCTURE: planes whose MAGNITUDE, SIGN and NON-FINITE VALUES are the subject, for the kernels between the tracer and the
screen that tests/value_ranges_lib.py does not reach: tptDisplayKernel, the blends (tptResolveKernel, tptResolveMirrorKernel,
tptResolveBatchKernel, tptFoldBatchKernel, tptAdaptiveResolveKernel), tptAdaptivePlanKernel and tptSpreadKernel.  Used by
tests/test_resolve_ranges.py (the statements, on the CPU) and tests/test_gpu_resolve_ranges.py (the kernels).  Nothing under
toypathtracer_amd/ imports this module.

  display_numpy      the display conversion of include/tpt_hip.h with explicit branches, float32 throughout;
  display_values, display_plane   every step of the conversion from both sides, the ends of tsqrt's guard, zeros, subnormals,
                     infinities, negatives and NaNs, packed one value per channel slot;
  planted_plane, PLANTED, ALPHA_BITS   the previous contents of a tile, a moments plane or a guide plane with non-finite, huge, tiny
                     and negative-zero values scattered over it, and bit patterns in .w that nobody may rewrite;
  adaptive_case      the running sample counts S (moments.w) and the counts plane of the adaptive blend;
  scaled_moments, plan_flat_case, plan_boundary_cases, PLAN_*   the plan kernel's planes;
  spread_*           the spread kernel's.

Every case is built once from seeded builders and shared; no test writes to a case's arrays."""
import numpy as np

from adaptive_lib import LUM_FLOOR, MAX_COUNT
from spatial_variance_lib import synthetic_case
from value_ranges_lib import pow2

f32 = np.float32
u32 = np.uint32
FLT_MAX = f32(3.40282347e38)
_built = {}


def _once(key, make):
    if key not in _built:
        _built[key] = make()
    return _built[key]


def bits(pattern):
    """the float32 with this bit pattern"""
    return np.array([pattern], u32).view(f32)[0]


def after(x, towards=np.inf):
    return np.nextafter(f32(x), f32(towards))


# ---------------------------------------------------------------- 1. the display conversion
DISPLAY_SIZES = [(1, 1), (1, 17), (17, 1), (255, 1), (257, 1), (130, 67)]  # (w, h); 130 x 67 is 34 workgroups of 256 and 6 lanes
DISPLAY_TAIL = 256 * 4       # bytes behind the image that a lane past the last pixel would write
DISPLAY_SENTINEL = 0xA5
QUIET_NAN, PAYLOAD_NAN, SIGNALLING_NAN = 0x7FC00000, 0x7FC01234, 0x7F800001
SIGN = 0x80000000


def display_numpy(tile):
    """tptDisplayRGBA8 as include/tpt_hip.h states it: [h, w, 4] float32 -> [h, w, 4] uint8, rows flipped.  Per colour channel
    s = sqrt(c) * 255 in float32; NaN, or not > 0: 0; otherwise trunc(min(s, 255)).  Alpha is 255 whatever the input's holds."""
    tile = np.asarray(tile)
    assert tile.dtype == np.float32 and tile.ndim == 3 and tile.shape[2] == 4
    out = np.empty(tile.shape, np.uint8)
    with np.errstate(all="ignore"):
        c = tile[::-1, :, :3]
        s = (np.sqrt(c) * f32(255)).astype(f32)
        lit = s > f32(0)                                        # (false for a NaN: sqrt of a NaN or of a negative)
        capped = np.where(s < f32(255), s, f32(255))            # min(s, 255) where lit
        out[..., :3] = np.where(lit, np.trunc(np.where(lit, capped, f32(0))), f32(0)).astype(np.uint8)
    out[..., 3] = 255
    return out


def display_level(c):
    """one channel of display_numpy on an array of any shape -> uint8"""
    c = np.asarray(c, f32)
    return display_numpy(np.stack([c.reshape(-1)] * 3 + [np.zeros(c.size, f32)], axis=-1)[None])[0, :, 0].reshape(c.shape)


def display_steps():
    """for every k in 1..255 the smallest float32 c with display_level(c) == k, by bisection over the bit patterns of the positive
    floats (the level is monotone in c) -> float32 [255]; its predecessors are nextafter(., 0)"""
    def make():
        k = np.arange(1, 256)
        lo, hi = np.zeros(255, np.int64), np.full(255, 0x7F800000, np.int64)  # level(lo) < k <= level(hi): +0 gives 0, +inf 255
        while (hi - lo > 1).any():
            mid = (lo + hi) // 2
            up = display_level(mid.astype(u32).view(f32)).astype(np.int64) >= k
            hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
        return hi.astype(u32).view(f32)
    return _once("display steps", make)


def display_specials():
    """name -> float32: the values beside the 510 of the steps"""
    lo, hi = pow2(-96), pow2(96)  # tpt_math.h: TPT_SQRT_LO, TPT_SQRT_HI, the guard of tsqrt's fast arm
    v = {"nan": bits(QUIET_NAN), "-1": f32(-1), "+inf": f32(np.inf), "+0": f32(0), "-0": f32(-0.0), "1e-45": bits(1), "2^-127": pow2(-127),
         "below 2^-96": after(lo, 0), "2^-96": lo, "above 2^-96": after(lo), "below 1": after(1, 0), "1": f32(1), "above 1": after(1, 2),
         "4": f32(4), "below 2^96": after(hi, 0), "2^96": hi, "above 2^96": after(hi), "3e38": f32(3e38), "-1e-45": bits(SIGN | 1),
         "-3e38": f32(-3e38), "-inf": f32(-np.inf), "-nan": bits(SIGN | QUIET_NAN), "nan payload": bits(PAYLOAD_NAN),
         "snan": bits(SIGNALLING_NAN), "-snan": bits(SIGN | SIGNALLING_NAN)}
    return v


def display_values():
    """the specials, then for k = 1..255 the value below the step and the step -> float32 [25 + 510]"""
    def make():
        steps = display_steps()
        pairs = np.stack([np.nextafter(steps, f32(0)), steps], axis=1).reshape(-1)
        return np.concatenate([np.array(list(display_specials().values()), f32), pairs]).astype(f32)
    return _once("display values", make)


def display_plane(w, h):
    """[h, w, 4]: display_values() one after the other through the 3 * w * h colour slots, as often as they fit (a plane of fewer
    slots holds the first of them); alpha NaN, -1 and 1e30 in turn"""
    def make():
        values = display_values()
        t = np.empty((h, w, 4), f32)
        t[..., :3] = values[np.arange(3 * w * h) % len(values)].reshape(h, w, 3)
        t[..., 3] = np.array([np.nan, -1.0, 1e30], f32)[np.arange(w * h) % 3].reshape(h, w)
        return np.ascontiguousarray(t)
    return _once(("display plane", w, h), make)


# ---------------------------------------------------------------- 2. the blends
RESOLVE_SIZE = (37, 21)   # (w, h): 777 pixels, three workgroups of 256 and 9 lanes
RESOLVE_SPP = 2
RESOLVE_FRAMES = (0, 1, 5)
LAST_WORKGROUP = 768      # the first pixel of the last, partial workgroup
# what is planted in the colour channels (one channel of a pixel each) ...
PLANTED = {"nan": bits(PAYLOAD_NAN), "+inf": f32(np.inf), "-inf": f32(-np.inf), "3e38": f32(3e38), "-3e38": f32(-3e38), "-0": f32(-0.0),
           "1e-45": bits(1), "2^-127": pow2(-127)}
POISON = ("nan", "+inf", "-inf")   # times a lerp factor of 0 these are NaN; every other value times 0 is a zero
# ... and the bit patterns of .w where .w is kept: they come back bit for bit
ALPHA_BITS = (PAYLOAD_NAN, SIGNALLING_NAN, SIGN)
PER_VALUE = 12


def planted_plane(seed, channels=3):
    """-> (plane [h, w, 4] float32, {name: (pixel indices, channel indices)}): finite seeded contents (rand * 3 - 0.75 plus the seed,
    .w included) with every value of PLANTED in PER_VALUE pixels outside the last workgroup and in one or two inside it, in one of
    the first `channels` channels each.  channels == 3: .w is kept by the blend, and holds ALPHA_BITS in PER_VALUE pixels each
    (and in every pixel of the last workgroup)"""
    def make():
        w, h = RESOLVE_SIZE
        n = w * h
        rng = np.random.default_rng([seed, 77])
        a = (rng.random((n, 4), dtype=f32) * f32(3) - f32(0.75) + f32(seed)).astype(f32)
        head, tail = rng.permutation(LAST_WORKGROUP), np.arange(LAST_WORKGROUP, n)
        where = {}
        for i, (name, value) in enumerate(PLANTED.items()):
            px = np.concatenate([head[i * PER_VALUE:(i + 1) * PER_VALUE], tail[i::len(PLANTED)]])
            ch = (np.arange(len(px)) + i) % channels
            a[px, ch] = value
            where[name] = (px, ch)
        if channels == 3:
            rest = head[len(PLANTED) * PER_VALUE:]
            alpha = a[:, 3].view(u32)
            for i, pattern in enumerate(ALPHA_BITS):
                px = np.concatenate([rest[i * PER_VALUE:(i + 1) * PER_VALUE], tail[i::len(ALPHA_BITS)]])
                alpha[px] = pattern
                where["alpha %08x" % pattern] = (px, np.full(len(px), 3))
        return np.ascontiguousarray(a.reshape(h, w, 4)), where
    return _once(("planted", seed, channels), make)


def poisoned(where, channels=3):
    """[h, w, channels] bool: the values of a planted plane that a lerp factor of 0 turns into NaN"""
    w, h = RESOLVE_SIZE
    m = np.zeros((w * h, channels), bool)
    for name in POISON:
        px, ch = where[name]
        m[px, ch] = True
    return m.reshape(h, w, channels)


# the adaptive blend: S = moments.w, lerp = S / (S + n) with S taken as 0 unless it is finite and >= 1
ADAPTIVE_S = (0.0, 0.999, 1.0, 4.0, 2.0 ** 24, 3.4028235e38, np.inf, -np.inf, np.nan, -4.0, 1e-40)
ADAPTIVE_COUNTS_COMMON = (0, 1, 7, -1, -2 ** 31)            # over the plane, in turn with the 11 values of S (5 and 11 are coprime)
ADAPTIVE_COUNTS_FEW = (2047, 2048, 2 ** 31 - 1)            # two pixels each: these are 2047 samples a pixel
ADAPTIVE_DRAWS = ((0, True), (1, True), (5, False))        # (frame, progressive), each from the planted planes
ADAPTIVE_MOST_SAMPLES = 50000                              # of the three draws together (tests/test_resolve_ranges.py states the sum)


def adaptive_case():
    """-> (tile, moments, counts): the planted tile, planted moments whose .w goes through ADAPTIVE_S pixel after pixel, and a counts
    plane of ADAPTIVE_COUNTS_COMMON in turn with ADAPTIVE_COUNTS_FEW at six pixels, each beside another S -- three of them in the
    last workgroup"""
    def make():
        w, h = RESOLVE_SIZE
        n = w * h
        tile = planted_plane(1)[0]
        mo = planted_plane(2)[0].copy().reshape(n, 4)
        mo[:, 3] = np.array(ADAPTIVE_S, f32)[np.arange(n) % len(ADAPTIVE_S)]
        counts = np.array(ADAPTIVE_COUNTS_COMMON, np.int64)[np.arange(n) % len(ADAPTIVE_COUNTS_COMMON)]
        for i, c in enumerate(ADAPTIVE_COUNTS_FEW):
            for px in (100 + 41 * i, LAST_WORKGROUP + (1, 5, 7)[i]):  # (every common count is left standing in the last workgroup)
                counts[px] = c
        return tile, np.ascontiguousarray(mo.reshape(h, w, 4)), np.ascontiguousarray(counts.astype(np.int32).reshape(h, w))
    return _once("adaptive", make)


def clamped(counts):
    return np.clip(counts.astype(np.int64), 0, MAX_COUNT)


def adaptive_blend_numpy(tile, moments, colour, staged, counts, progressive):
    """tptDrawDeviceAdaptive's blend as include/tpt_hip.h states it, on whole planes: n the clamped count; a pixel with n == 0 is left
    alone; S = moments.w where `progressive` and it is finite and >= 1, else 0; lerp = S / (S + n), an IEEE quotient; tile.rgb and
    moments.xyz through batch_moments_lib.blend's arithmetic with colour.rgb and staged.xyz; moments.w = S + n; the tile's alpha kept
    -> (tile, moments), copies"""
    n = clamped(counts).astype(f32)
    traced = (n > 0)[..., None]
    with np.errstate(all="ignore"):
        S = moments[..., 3]
        S = np.where(bool(progressive) & (S >= f32(1)) & (S <= FLT_MAX), S, f32(0)).astype(f32)
        S1 = (S + n).astype(f32)
        lerp = (S / S1).astype(f32)[..., None]
        one = f32(1) - lerp
        t, m = tile.copy(), moments.copy()
        t[..., :3] = np.where(traced, tile[..., :3] * lerp + colour[..., :3] * one, tile[..., :3])
        m[..., :3] = np.where(traced, moments[..., :3] * lerp + staged[..., :3] * one, moments[..., :3])
        m[..., 3] = np.where(traced[..., 0], S1, moments[..., 3])
    return t, m


# ---------------------------------------------------------------- 3. the plan kernel
PLAN_SIZES = [(1, 1), (65, 5), (37, 21)]
PLAN_SCALES = (-70, -50, -12, 16, 50, 63)
# targetError: 1e6, the largest the call takes; 2e-19, whose square 4e-38 is normal; 1e-19, whose square 1e-38 is already below the
# smallest normal 1.18e-38; 1e-22, whose square is 7 subnormal steps; 1e-23, whose square is 0 (R / 0 is inf, or NaN where R == 0)
PLAN_TARGETS = (1e6, 2e-19, 1e-19, 1e-22, 1e-23)
PLAN_BOUNDS = ((0, 0), (0, 2047), (2047, 2047))
PLAN_ARGUMENTS = [(te, lo, hi) for te in PLAN_TARGETS for lo, hi in PLAN_BOUNDS] + [(0.05, 1, 64)]


def scaled_moments(moments, k):
    """.x times 2^k, .y times 2^k twice (one product 2^2k would leave the format at |k| = 64 already); .z and .w as they are"""
    s = pow2(k)
    with np.errstate(all="ignore"):
        m = moments.copy()
        m[..., 0] *= s
        m[..., 1] *= s
        m[..., 1] *= s
    return np.ascontiguousarray(m)


def plan_scaled_case(kind, w, h, k):
    def make():
        from test_adaptive_checker import seeded_moments
        return scaled_moments(seeded_moments(np.random.default_rng([w, h, len(kind)]), h, w, kind), k)
    return _once(("plan scaled", kind, w, h, k), make)


def flat(h, w, mean, second, S):
    from test_adaptive_checker import flat as flat_plane
    return flat_plane(h, w, mean, second, S)


FLAT = dict(mean=f32(0.5), second=f32(0.75), S=f32(4.0))  # var 0.5, b = 0.51: r = 1.92
# name -> (m.x, m.y) of a pixel planted in the flat plane, under the plane's valid S
PLAN_PLANTED = {
    "b == 0, var > 0": (-LUM_FLOOR, f32(1)),                        # var / 0 = inf
    "b == 0, var == 0": (-LUM_FLOOR, f32(LUM_FLOOR * LUM_FLOOR)),   # 0 / 0 = NaN: minSamples here and in the eight neighbours
    "mean below the floor": (f32(-3), f32(16)),
    "second below the squared mean": (f32(2), f32(3)),
    "inf - inf": (f32(3e20), f32(np.inf)),
    "mean NaN": (f32(np.nan), f32(1)),
    "subnormal moments": (f32(1e-40), f32(1e-42)),
}


def plan_flat_case(w, h):
    """-> (moments, {name: (y, x)}): the flat plane with PLAN_PLANTED's pixels -- at 1 x 1 one plane per name instead, a dict name ->
    (moments, (0, 0)) --, four columns apart on the middle row and the next one, so that no two share a 3 x 3 window"""
    def make():
        if (w, h) == (1, 1):
            out = {}
            for name, (mx, my) in PLAN_PLANTED.items():
                mo = flat(1, 1, **FLAT)
                mo[0, 0, :2] = (mx, my)
                out[name] = (mo, (0, 0))
            return out
        mo = flat(h, w, **FLAT)
        at = {}
        for i, (name, (mx, my)) in enumerate(PLAN_PLANTED.items()):
            y, x = (h // 2 if i % 2 == 0 else 0), 2 + 4 * i
            mo[y, x, :2] = (mx, my)
            at[name] = (y, x)
        return np.ascontiguousarray(mo), at
    return _once(("plan flat", w, h), make)


# The boundaries of the count.  A flat plane with m.x = 2^18: the luminance floor is absorbed, b*b = 2^36 = m.x*m.x, and r = d / 2^36
# is d = m.y - 2^36 with another exponent.  Where m.y is in d's binade (d >= 4 * 2^36) the second moment's own last bit is d's, so it
# moves r by one unit in the last place.  targetError 1: need = R; S = 1: extra = need - 1, exact and in need's binade for extra >= 4
# (and >= 8, where the bounds below lie).
# Away from the border every pixel has the same nine taps and the same R, which is r up to the roundings of the nine partial sums;
# so the second moment is SEARCHED, bit pattern by bit pattern around its estimate, until the statement's own `extra` of the interior
# pixels is the wanted float32 exactly.
BOUNDARY_TE, BOUNDARY_S, BOUNDARY_MEAN = 1.0, f32(1.0), pow2(18)
BOUNDARY_NAMES = ("minSamples", "one ulp above minSamples", "an integer between", "that integer plus one ulp", "one ulp below maxSamples",
                  "maxSamples")


def interior_extra(second, lo=0, hi=MAX_COUNT, size=(5, 5)):
    """`extra` of the numpy statement at the middle of a flat plane of BOUNDARY_MEAN, `second`, BOUNDARY_S"""
    from adaptive_lib import plan_numpy
    w, h = size
    return plan_numpy(flat(h, w, BOUNDARY_MEAN, f32(second), BOUNDARY_S), BOUNDARY_TE, lo, hi, details=True)[3]["extra"][h // 2, w // 2]


def second_for(extra):
    """the second moment with which the interior pixels' `extra` is this float32 exactly; None when no second moment gives it.  The
    candidates go through the statement's nine taps all at once; the one found is confirmed by the statement itself"""
    from moments_lib import GK
    mm = float(BOUNDARY_MEAN) ** 2
    guess = f32(mm + (float(extra) + float(BOUNDARY_S)) * mm)
    cand = (guess.view(u32).astype(np.int64) + np.arange(-64, 65)).astype(u32).view(f32)
    d = cand - BOUNDARY_MEAN * BOUNDARY_MEAN
    b = BOUNDARY_MEAN + LUM_FLOOR
    r = np.where(d > 0, d, f32(0)) / (b * b)
    gv, gw = np.zeros_like(r), f32(0)
    for jy in range(3):
        for jx in range(3):
            k = GK[jy] * GK[jx]
            gv, gw = gv + k * r, gw + k
    got = (gv / gw) / (f32(BOUNDARY_TE) * f32(BOUNDARY_TE)) - BOUNDARY_S
    hit = np.flatnonzero(got.view(u32) == f32(extra).view(u32))
    if not len(hit):
        return None
    assert interior_extra(cand[hit[0]]).tobytes() == f32(extra).tobytes()
    return cand[hit[0]]


def plan_boundary_cases():
    """-> (lo, mid, hi, {name: second moment}): the first (minSamples, an integer between, maxSamples) for which all six values of
    `extra` can be had exactly"""
    def make():
        for lo, mid, hi in ((8, 10, 13), (9, 11, 14), (8, 9, 12), (10, 12, 14)):
            targets = (f32(lo), after(lo), f32(mid), after(mid), after(hi, 0), f32(hi))
            seconds = [second_for(t) for t in targets]
            if all(s is not None for s in seconds):
                return lo, mid, hi, dict(zip(BOUNDARY_NAMES, seconds))
        raise AssertionError("no set of bounds whose six boundary values are all reachable")
    return _once("plan boundaries", make)


# ---------------------------------------------------------------- 4. the spread kernel
SPREAD_SIZES = [(3, 2), (65, 9), (130, 67)]
SPREAD_SCALES = (-70, -50, -12, 50, 63)   # (63: e1*e1 does not overflow before)
SPREAD_KINDS = ("all", "mixed")
SPREAD_GUIDE = dict(sigma_normal=0.03, sigma_depth=0.5)
# The call (include/tpt_hip.h), the host and the C statement take a guide's sigma of 0 or in [1e-6, 1e6], samplesPerFrame >= 1 and
# minSamples >= 1 and refuse everything else before a kernel runs.  So the ends the kernel can meet are 0 (inv2 = 0), 1e-6 (1e12)
# and 1e6 (1e-12); a sigma of 1e-20 .. 1e20, a subnormal minSamples and samplesPerFrame below 1 are held as REFUSALS, and the numpy
# statement, which takes them, says what they would be.
SPREAD_SIGMAS = (0.0, 1e-6, 1e6)
SPREAD_SIGMA_CASES = [(sn, sd) for sn in SPREAD_SIGMAS for sd in SPREAD_SIGMAS]
SPREAD_REFUSED_SIGMAS = (1e-20, 1e-19, 1e19, 1e20)
SPREAD_REFUSED_COUNTS = (dict(min_samples=1e-40), dict(samples_per_frame=1.1754944e-38), dict(samples_per_frame=0.999))
SPREAD_COUNT_ENDS = (dict(samples_per_frame=2.0, min_samples=float("inf")), dict(samples_per_frame=2.0, min_samples=3.0),
                     dict(samples_per_frame=3.4028235e38, min_samples=float("inf")), dict(samples_per_frame=1.0, min_samples=1.0))


def spread_scaled_case(kind, w, h, k):
    """spatial_variance_lib.synthetic_case with its moments scaled -> (moments, normal_depth), [h, w, 4]"""
    def make():
        m, nd = synthetic_case(w, h, 1, kind)
        return scaled_moments(m[0], k), np.ascontiguousarray(nd[0])
    return _once(("spread scaled", kind, w, h, k), make)


def spread_guide_case(w, h):
    """the "all" case (every pixel estimated) with a guide of extremes: depths of 1e20 and -1e20 in alternating columns on the left
    third (dw*dw is infinite between neighbours, 0 within a column), normals of 3e38 in every third pixel of the middle third (their
    squared difference to a neighbour is infinite; times a sigma of 0 that is NaN), the seeded guide on the right, and N = 3e38 in
    one pixel of ten: samplesPerFrame * N is infinite there at samplesPerFrame = 2 and never below minSamples
    -> (moments, normal_depth), [h, w, 4]"""
    def make():
        m, nd = synthetic_case(w, h, 1, "all")
        m, nd = m[0].copy(), nd[0].copy()
        xs = np.arange(w)
        left, middle = xs < w // 3, (xs >= w // 3) & (xs < 2 * w // 3)
        nd[:, left, 3] = np.where(xs[left] % 2 == 0, f32(1e20), f32(-1e20))[None, :]
        third = ((np.arange(h)[:, None] * w + xs[None, :]) % 3 == 0) & middle[None, :]
        nd[third, :3] = f32(3e38)
        m.reshape(-1, 4)[::10, 3] = f32(3e38)
        return np.ascontiguousarray(m), np.ascontiguousarray(nd)
    return _once(("spread guide", w, h), make)
