"""TEST INFRASTRUCTURE: planes whose MAGNITUDE, SIGN and NON-FINITE PIXELS are the subject, for tests/test_value_ranges.py (the C
checkers and the numpy statements, on the CPU) and tests/test_gpu_value_ranges.py (the post-process kernels on the GPU).  The rest of
the suite feeds those kernels colours of rand^3 * 4, depths of 1 .. 20, cameras three units from the origin and the default sigmas; the
guarded fast forms of the a-trous weights' division (tdivSafeNum: denominator in [2^-60, 2^60]) and of the square roots (tsqrt, trsqrt2:
argument in [2^-96, 2^96]) never leave their fast arm there.  Nothing under toypathtracer_amd/ imports this module.

  same_bits          the one relaxation of byte equality: NaN positions equal, every other element byte-equal.  A NaN's sign and
                     payload are not part of the contract (tests/scene_kinds_lib.py says the same); a reference without a NaN is
                     compared with tobytes() as everywhere else;
  scaled_geometry    cameras, normal / depth planes and motion tables with every length times 2^k;
  scaled_colour      colours times 2^k, first moments times 2^k, second moments times 2^k twice;
  planted, footprint_mask   one value planted in one plane, and the pixels no a-trous filter of `iterations` iterations can carry it to;
  first_iteration_denominators   a numpy restatement of the tap denominators of iteration 0 of both a-trous filters, used only to prove
                     which side of 2^60 a case lies on;
  rel_squared, window_variance   the arguments of the guarded square roots of the temporal / object / flow kernels and of the
                     rectify kernel, restated, used only to prove which side of [2^-96, 2^96] a case lies on;
  ATROUS_CASES       the named planes of both a-trous filters (families magnitude, depth, signs), SIGMA_CASES / VARIANCE_SIGMA_CASES the
                     sigma ends, FOOTPRINT_* the planted pixels; temporal_case, object_case, flow_case, rectify_case the scaled cases of
                     the other kernels.  Each is built once from the existing seeded builders and shared: no test writes
                     to a case's arrays (they stay writable, since the GPU helpers hand them to torch.from_numpy).

LEFT OUT ON PURPOSE: NaN payloads and signs (same_bits).  Beyond 2^-54 and 2^50 for the geometry and 2^-60 and 2^50 for the colour the
temporal, object, flow and rectify statements stop being scale-invariant -- their own intermediates (squares of lengths, of colours)
leave the normal range --, so the cases further out (2^-62) are held to the checker alone, not to the unscaled output."""
import numpy as np

import flow_lib
import object_lib
import rectify_lib
import temporal_lib
from denoise_lib import inv2
from moments_lib import EPS, GK, lum, random_moments, random_planes

f32 = np.float32
DIV_LO, DIV_HI = f32(2.0 ** -60), f32(2.0 ** 60)      # tpt_math.h: TPT_DIV_LO, TPT_DIV_HI
SQRT_LO, SQRT_HI = f32(2.0 ** -96), f32(2.0 ** 96)    # tpt_math.h: TPT_SQRT_LO, TPT_SQRT_HI
W, H, SEED, ITERATIONS = 130, 67, 5, 5                # the a-trous cases: two blocks in x, seventeen in y, neither a multiple of the tile
SCALES = (-50, -12, 16, 50)                           # 2^k of the colour cases; +-50 squares to beyond 2^+-96
# ... and of the geometry cases.  The synthetic depths are 1 .. 9, so at k = -50 only a point nearer than 4 has |rel|^2 below 2^-96
# (3/8 of the covered 6/7 of the pixels); at k = -54 every covered pixel has, and the statements are as invariant there as at -50
GEOMETRY_SCALES = (-54,) + SCALES
MOST_OUTSIDE_THE_SQRT_GUARD = (-54, 50)               # (tests/test_value_ranges.py: at least half of the pixels, for every geometry case)
# The guards are conservative: emulated on these cases' own arguments, the unguarded five-instruction square root still rounds right
# at every k above (0 of 18237 window variances, 0 of 8710 |rel|^2), and goes wrong only once its residual x - s0^2 is subnormal, near
# 2^-108 and below.  Two cases reach that: the rectify statement is invariant down to k = -60 (variances of 2^-131 .. 2^-118: the
# unguarded form misrounds 0.15 of them), and the "pixel" clip at k = -62 (|rel|^2 of 2^-138 .. 2^-124: 0.04), where the flow
# statement is no longer invariant -- its products leave the normal range -- and only the checker is left to compare with.  The
# temporal and object cases run at k = -62 too (|rel|^2 of 2^-124 .. 2^-118, and |v|^2 of the pixel's ray, which normalize() hands
# to trsqrt2, of 2^-121 .. 2^-119), against their checkers alone.  tests/test_value_ranges.py proves on the CPU where these
# arguments lie; the build without the guards fails on them (the pull request's summary says which tests).
RECTIFY_SCALES = (-60,) + SCALES
FLOW_DEEP_SCALE = -62
TEMPORAL_DEEP_SCALE = -62
DEEP = f32(2.0 ** -118)
OBJECT_SCALES = GEOMETRY_SCALES                       # (tests/test_value_ranges.py: the object statement is invariant at all of them)
SAMPLES = 3.0


def same_bits(got, want):
    """the NaN positions are equal and every other element is byte-equal"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn)) and got[~gn].tobytes() == want[~wn].tobytes()


def pow2(k):
    return f32(2.0 ** k)


# ---------------------------------------------------------------- scale
def scaled_geometry(cameras, nds, motion, k):
    """every length times 2^k: floats 0 .. 11 (origin, lower left corner, horizontal, vertical) and 21 (lens radius) of each camera
    record (float32 [22] or [n, 22]), .w of every normal / depth plane (an array or a sequence of arrays), .xyz of a motion table
    (None, [n, 4] or [f, n, 4]).  The callers pass the current and the previous frame's alike; everything else stays as it is
    -> (cameras, nds, motion), copies"""
    s = pow2(k)
    c = np.array(cameras, f32, copy=True)
    c[..., 0:12] *= s
    c[..., 21] *= s

    def nd_scaled(a):
        a = a.copy()
        a[..., 3] *= s
        return np.ascontiguousarray(a)

    with np.errstate(all="ignore"):
        n = nd_scaled(nds) if isinstance(nds, np.ndarray) else tuple(nd_scaled(a) for a in nds)
        m = None
        if motion is not None:
            m = motion.copy()
            m[..., 0:3] *= s
    return np.ascontiguousarray(c), n, m


def scaled_colour(colour, acc, moments, acc_moments, k):
    """rgb of both colour planes times 2^k, .x of both moments planes times 2^k, .y times 2^k twice (one product 2^2k would leave the
    format at |k| = 64 already); every .w, and the moments' .z, stay as they are -> the four planes, copies"""
    s = pow2(k)
    with np.errstate(all="ignore"):
        def col(a):
            a = a.copy()
            a[..., :3] *= s
            return np.ascontiguousarray(a)

        def mom(a):
            a = a.copy()
            a[..., 0] *= s
            a[..., 1] *= s
            a[..., 1] *= s
            return np.ascontiguousarray(a)
        return col(colour), col(acc), mom(moments), mom(acc_moments)


# ---------------------------------------------------------------- planted pixels
PLANES = ("colour", "albedo", "nd", "moments")


def planted(planes, where, value):
    """planes: dict of colour, albedo, nd, moments; where: (plane, y, x, component) -> a dict with that one element replaced (the other
    planes are shared, not copied)"""
    name, y, x, comp = where
    out = dict(planes)
    a = planes[name].copy()
    a[y, x, comp] = f32(value)
    out[name] = np.ascontiguousarray(a)
    return out


def footprint_radius(iterations):
    """how far both a-trous filters carry a pixel: 2 * 2^i per iteration i (the variance filter's 3x3 blur of v stays inside it)"""
    return 2 * ((1 << iterations) - 1)


def footprint_mask(h, w, y0, x0, iterations):
    """True for the pixels farther than the footprint radius from (y0, x0) in x or in y: no filter output there depends on (y0, x0)"""
    r = footprint_radius(iterations)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    return (np.abs(ys - y0) > r) | (np.abs(xs - x0) > r)


FOOTPRINT_SIZE = (97, 41)          # (w, h)
FOOTPRINT_AT = (20, 48)            # (y, x): the whole footprint lies inside the image
FOOTPRINT_ITERATIONS = 3           # R = 14: 29 x 29 pixels, 0.79 of the image outside
FOOTPRINT_VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "3e38": 3e38, "1e-42": 1e-42, "-1": -1.0}
FOOTPRINT_PLANES = {"colour.g": ("colour", 1), "albedo.g": ("albedo", 1), "normalDepth.w": ("nd", 3), "moments.y": ("moments", 1)}
FOOTPRINT_CASES = [(p, v) for p in FOOTPRINT_PLANES for v in FOOTPRINT_VALUES]

_built = {}


def _once(key, make):
    if key not in _built:
        _built[key] = make()
    return _built[key]


def clean_planes(w=W, h=H, seed=SEED):
    """random_planes and random_moments of one seeded generator -> dict(colour, albedo, nd, moments), built once and shared"""
    def make():
        rng = np.random.default_rng(seed)
        colour, albedo, nd = random_planes(rng, h, w)
        return dict(zip(PLANES, (colour, albedo, nd, random_moments(rng, colour))))
    return _once(("clean", w, h, seed), make)


def footprint_planes(plane=None, value=None):
    """the clean planes at FOOTPRINT_SIZE, or those with FOOTPRINT_VALUES[value] planted at FOOTPRINT_AT of FOOTPRINT_PLANES[plane]"""
    w, h = FOOTPRINT_SIZE

    def make_clean():
        p = dict(clean_planes(w, h))
        m = p["moments"].copy()  # a variance of 0.5 at the planted pixel (one pixel in six has none, and a second moment that clamps to
        m[FOOTPRINT_AT + (1,)] = m[FOOTPRINT_AT + (0,)] * m[FOOTPRINT_AT + (0,)] + f32(0.5)  # the same +0 would change nothing)
        p["moments"] = np.ascontiguousarray(m)
        return p
    clean = _once(("footprint clean",), make_clean)
    if plane is None:
        return clean
    name, comp = FOOTPRINT_PLANES[plane]
    return _once(("planted", plane, value), lambda: planted(clean, (name,) + FOOTPRINT_AT + (comp,), FOOTPRINT_VALUES[value]))


# ---------------------------------------------------------------- the a-trous cases
COLOUR_SCALES = (-140, -100, -40, 20, 30, 40, 62, 100, 126)
DEPTH_SCALES = (-60, 40, 62)


def _colour_case(k):
    def make():
        p = dict(clean_planes())
        c = p["colour"].copy()
        with np.errstate(all="ignore"):
            c[..., :3] *= pow2(k)
        p["colour"] = np.ascontiguousarray(c)
        return p
    return make


def _depth_case(k):
    def make():
        p = dict(clean_planes())
        p["nd"] = scaled_geometry(np.zeros(22, f32), p["nd"], None, k)[1]
        return p
    return make


def _negated_colour():
    p = dict(clean_planes())
    rng = np.random.default_rng([SEED, 1])
    c = p["colour"].copy()
    c[rng.random((H, W)) < 1.0 / 3.0, :3] *= f32(-1)
    p["colour"] = np.ascontiguousarray(c)
    return p


def _odd_albedo():
    """-1, -0 and subnormal channels: `a > 0` is false for the first two (the channel passes through), true for a subnormal: the
    demodulated colour is up to 1e38, its squared difference to any neighbour infinite, and it comes back through the same product.
    The subnormals stand where the colour's channel is below 1 (1e-38) or zero (1e-42), so that no quotient overflows: one infinity
    is a NaN in every pixel of its footprint, which after five iterations is the whole image (that is `overflow_2^126`'s subject)"""
    p = dict(clean_planes())
    rng = np.random.default_rng([SEED, 2])
    a = p["albedo"].copy()
    for value in (-1.0, -0.0):
        a[rng.random((H, W, 4)) < 0.03] = f32(value)
    rgb, c = a[..., :3], p["colour"][..., :3]
    for value, where in ((1e-38, (c > 0) & (c < 1)), (1e-42, c == 0)):
        at = np.argwhere(where)
        at = at[rng.choice(len(at), 150, replace=False)]
        rgb[at[:, 0], at[:, 1], at[:, 2]] = f32(value)
    p["albedo"] = np.ascontiguousarray(a)
    return p


def _low_moments():
    """m.y < m.x^2 everywhere: the variance clamps to +0 in every pixel"""
    p = dict(clean_planes())
    m = p["moments"].copy()
    m[..., 1] = m[..., 0] * m[..., 0] * f32(0.5) - f32(0.125)
    p["moments"] = np.ascontiguousarray(m)
    return p


def colour_name(k):
    return "overflow_2^126" if k == 126 else "colour_2^%d" % k


ATROUS_FAMILIES = {
    "magnitude": {colour_name(k): _colour_case(k) for k in COLOUR_SCALES},
    "depth": {"depth_2^%d" % k: _depth_case(k) for k in DEPTH_SCALES},
    "signs": {"negated_colour": _negated_colour, "odd_albedo": _odd_albedo, "low_moments": _low_moments},
}
ATROUS_CASES = {name: fn for fam in ATROUS_FAMILIES.values() for name, fn in fam.items()}
MAY_BE_MOSTLY_NAN = ("overflow_2^126",)


def atrous_case(name):
    """the planes of this name (or "clean"), built once and shared"""
    if name == "clean":
        return clean_planes()

    return _once(("atrous", name), ATROUS_CASES[name])


def default_sigmas():
    from toypathtracer_amd.api import DENOISE_DEFAULTS as D
    return D["sigma_colour"], D["sigma_normal"], D["sigma_depth"]


def variance_sigmas():
    from toypathtracer_amd.api import DENOISE_VARIANCE_DEFAULTS as D
    return D["sigma_luminance"], D["sigma_normal"], D["sigma_depth"]


EVERYTHING, COLOUR_ALONE = (True, True, True), (False, False, False)  # (albedo, normal / depth, demodulate)


# tptDenoiseDevice's sigma ends: name -> (planes, (sigma_colour, sigma_normal, sigma_depth), mode).  "straddles": the first-iteration
# tap denominators lie on both sides of 2^60; "inside": none lies above it (tests/test_value_ranges.py proves both).  sigma_colour
# 1e-6 ALONE is the colour term by itself, 1 + dc * 1e12 <= 2^46: a guide's factor or a demodulated colour carries it past 2^60, which
# is the case with the default guides beside it, in every mode
def sigma_cases():
    d = default_sigmas()
    return {
        "straddles_sigmas_1e-3": ("clean", (1e-3, 1e-3, 1e-3), EVERYTHING),
        "straddles_sigmas_1e-6": ("clean", (1e-6, 1e-6, 1e-6), EVERYTHING),
        "straddles_colour_2^40": ("colour_2^40", d, EVERYTHING),
        "inside_default_sigmas": ("clean", d, EVERYTHING),
        "inside_sigmas_1e6": ("clean", (1e6, 1e6, 1e6), EVERYTHING),
        "inside_sigma_colour_1e-6": ("clean", (1e-6, 0.0, 0.0), COLOUR_ALONE),
        "straddles_sigma_colour_1e-6_default_guides": ("clean", (1e-6, d[1], d[2]), EVERYTHING),  # (0.72 of its taps pass 2^60)
    }


SIGMA_CASE_NAMES = ("straddles_sigmas_1e-3", "straddles_sigmas_1e-6", "straddles_colour_2^40", "inside_default_sigmas", "inside_sigmas_1e6",
                    "inside_sigma_colour_1e-6", "straddles_sigma_colour_1e-6_default_guides")
SIGMA_ITERATIONS = (1, 5, 8)  # (the inverse squared colour sigma is multiplied by 4^i)
# tptDenoiseDeviceVariance's: sigma_luminance at both ends, the guides' sigmas at both ends -> (sl, sn, sd)
VARIANCE_SIGMA_CASES = {"sl_%g_guides_%g" % (sl, g): (sl, g, g) for sl in (1e-6, 1e6) for g in (1e-6, 1e6)}


def _shifted(arr, oy, ox):
    h, w = arr.shape
    ys, xs = np.arange(h) + oy, np.arange(w) + ox
    valid = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
    return arr[np.clip(ys, 0, h - 1)][:, np.clip(xs, 0, w - 1)], valid


def first_iteration_denominators(colour, albedo, nd, sigmas, demodulate=True, moments=None, samples=SAMPLES):  # (nd None: no guide)
    """The weight denominators of every tap inside the image in iteration 0 (step 1), in the order and roundings of the statements:
    tptDenoiseDevice's with sigmas = (sigma_colour, sigma_normal, sigma_depth), tptDenoiseDeviceVariance's when `moments` is given, with
    sigmas = (sigma_luminance, sigma_normal, sigma_depth) -> a flat float32 array"""
    h, w = colour.shape[:2]
    out = []
    with np.errstate(all="ignore"):
        c = [colour[..., k].astype(f32) for k in range(3)]
        if demodulate:
            for k in range(3):
                a = albedo[..., k]
                c[k] = np.where(a > 0, c[k] / np.where(a > 0, a, f32(1)), c[k])
        inn, idd = inv2(sigmas[1]), inv2(sigmas[2])
        if moments is None:
            ic = inv2(sigmas[0])
        else:
            d = moments[..., 1] - moments[..., 0] * moments[..., 0]
            v = np.where(d > 0, d, f32(0)) / f32(samples)
            if demodulate:
                la = lum(albedo[..., 0], albedo[..., 1], albedo[..., 2])
                la2 = la * la
                v = np.where(la2 > 0, v / np.where(la2 > 0, la2, f32(1)), v)
            v = v.astype(f32)
            gv, gw = np.zeros((h, w), f32), np.zeros((h, w), f32)
            for jy in range(3):
                for jx in range(3):
                    vq, valid = _shifted(v, jy - 1, jx - 1)
                    k = GK[jy] * GK[jx]
                    gv = np.where(valid, gv + k * vq, gv)
                    gw = np.where(valid, gw + k, gw)
            il = f32(1) / ((f32(sigmas[0]) * f32(sigmas[0])) * (gv / gw) + EPS)
            lp = lum(c[0], c[1], c[2])
        for ky in range(5):
            for kx in range(5):
                cq = []
                for ck in c:
                    q, valid = _shifted(ck, ky - 2, kx - 2)
                    cq.append(q)
                if moments is None:
                    dd = [cq[k] - c[k] for k in range(3)]
                    den = f32(1) + ((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]) * ic
                else:
                    dl = lum(cq[0], cq[1], cq[2]) - lp
                    den = f32(1) + (dl * dl) * il
                if nd is not None:
                    nq = [_shifted(nd[..., k], ky - 2, kx - 2)[0] for k in range(4)]
                    dn = [nq[k] - nd[..., k] for k in range(3)]
                    den = den * (f32(1) + ((dn[0] * dn[0] + dn[1] * dn[1]) + dn[2] * dn[2]) * inn)
                    dz = nq[3] - nd[..., 3]
                    den = den * (f32(1) + (dz * dz) * idd)
                out.append(den[valid].astype(f32))
    return np.concatenate(out)


def division_shares(den):
    """-> (share of the taps whose denominator is above 2^60 -- the kernel's `a / b` arm --, share at or below it, share of the first
    that is infinite); a NaN denominator is in neither of the first two"""
    above = den > DIV_HI
    inside = (den >= DIV_LO) & (den <= DIV_HI)
    n = float(den.size)
    return above.sum() / n, inside.sum() / n, (np.isinf(den) & above).sum() / max(1.0, float(above.sum()))


def outside_sqrt_guard(x):
    """per element of the positive finite values of x: the kernel's guard sends it to the compiler's expansion (not in [2^-96, 2^96]).
    A zero, a negative, an infinity or a NaN (the planted ones) takes the expansion at every scale and says nothing about one: they
    are left out -> (share outside, count)"""
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        pos = (x > 0) & (x <= f32(3.40282347e38))
        out = pos & ~((x >= SQRT_LO) & (x <= SQRT_HI))
    return out.sum() / max(1.0, float(pos.sum())), int(pos.sum())


# ---------------------------------------------------------------- the scaled cases of the other kernels
TEMPORAL_KW = dict(max_history=8.0, depth_tolerance=0.1, normal_tolerance=0.25, coverage_tolerance=0.0)
RECTIFY_KW = dict(radius=2, gamma=0.75)
TEMPORAL_KINDS = ("same", "moved")
FLOW_KINDS = ("moved", "pixel")
FLOW_SIZE = (65, 5)


def temporal_case(kind, k=0):
    """temporal_lib.synthetic_case(kind, 130, 67) with its geometry times 2^k -> (camera, cur, prev)"""
    def make():
        cam, cur, prev = temporal_lib.synthetic_case(kind, W, H)
        cams, nds, _ = scaled_geometry(np.stack([cam, prev[0]]), (cur[2], prev[3]), None, k)
        cur2 = (cur[0], cur[1], nds[0], cur[3])
        prev2 = (cams[1].copy(), prev[1], prev[2], nds[1], prev[4])
        return cams[0].copy(), cur2, prev2
    return _once(("temporal", kind, k), make)


def object_case(k=0):
    """object_lib.synthetic_objects("moved", 130, 67) with its geometry and its table's displacements times 2^k
    -> (camera, cur, object plane, prev with its object plane, motion table)"""
    def make():
        cam, cur, obj, prev, motion = object_lib.synthetic_objects("moved", W, H)
        cams, nds, m = scaled_geometry(np.stack([cam, prev[0]]), (cur[2], prev[3]), motion, k)
        cur2 = (cur[0], cur[1], nds[0], cur[3])
        prev2 = (cams[1].copy(), prev[1], prev[2], nds[1], prev[4], prev[5])
        return cams[0].copy(), cur2, obj, prev2, m
    return _once(("object", k), make)


def flow_case(kind, k=0):
    """flow_lib.synthetic_clip(kind, 65, 5) with its geometry and its tables' displacements times 2^k -> the clip's dict"""
    def make():
        w, h = FLOW_SIZE
        clip = flow_lib.synthetic_clip(kind, w, h)
        pv = clip["prev"]
        cams, nds, m = scaled_geometry(np.concatenate([clip["cameras"], pv[0][None]]), (clip["nd"], pv[2]), clip["motion"], k)
        return dict(clip, cameras=np.ascontiguousarray(cams[:-1]), nd=nds[0], motion=m, prev=(cams[-1].copy(), pv[1], nds[1], pv[3]))
    return _once(("flow", kind, k), make)


def flow_expected(out0, clip, k):
    """what scaling the geometry by 2^k does to the k = 0 output: e (.z) times 2^k where the frame's pixel is a hit (albedo.w > 0); a
    sky pixel's `rel` is its unit ray, which does not scale"""
    want = out0.copy()
    with np.errstate(all="ignore"):
        hit = clip["albedo"][..., 3] > 0
        want[..., 2] = np.where(hit, out0[..., 2] * pow2(k), out0[..., 2])
    return want


def rectify_case(k=0):
    """rectify_lib.synthetic_case(130, 67) with its colours times 2^k -> (colour, moments, acc_colour, acc_moments)"""
    def make():
        colour, moments, acc, acc_moments = rectify_lib.synthetic_case(W, H)
        c, a, m, am = scaled_colour(colour, acc, moments, acc_moments, k)
        return c, m, a, am
    return _once(("rectify", k), make)


def rectify_expected(out0, k):
    """out0: the k = 0 outputs (colour, moments, variance) -> (the colour with rgb times 2^k, the history lengths)"""
    want = out0[0].copy()
    with np.errstate(all="ignore"):
        want[..., :3] *= pow2(k)
    return want, out0[1][..., 3]


def rel_squared(cam, albedo, nd, pcam, obj=None, motion=None):
    """dot(rel, rel) of the temporal, object and flow statements for every pixel of a frame: the argument of the kernels' tsqrt
    (obj and motion: the table's displacement is added where the statements read it) -> float32 [h, w]"""
    h, w = albedo.shape[:2]
    o, d3 = object_lib.centre_rays(cam, w, h)
    po = temporal_lib.camera_floats(pcam)[0:3]
    with np.errstate(all="ignore"):
        cov = albedo[..., 3]
        hit = cov > 0
        d = nd[..., 3] / np.where(hit, cov, f32(1))
        at = [o[i] + d3[i] * d for i in range(3)]
        if obj is not None and motion is not None:
            read = hit & (obj >= 0) & (obj < motion.shape[0])
            entry = motion[np.where(read, obj, 0)]
            at = [np.where(read, at[i] + entry[..., i], at[i]) for i in range(3)]
        rel = [np.where(hit, at[i] - po[i], d3[i]).astype(f32) for i in range(3)]
        return ((rel[0] * rel[0] + rel[1] * rel[1]) + rel[2] * rel[2]).astype(f32)


def ray_squared(cam, w, h):
    """dot(v, v) of the ray through every pixel's centre before it is normalised: the argument of the kernels' trsqrt2 -> float32 [h, w]"""
    c = temporal_lib.camera_floats(cam)
    o, ll, H, V = (c[i:i + 3] for i in (0, 3, 6, 9))
    s = ((np.arange(w, dtype=f32) + f32(0.5)) / f32(w))[None, :]
    t = ((np.arange(h, dtype=f32) + f32(0.5)) / f32(h))[:, None]
    with np.errstate(all="ignore"):
        v = [((ll[i] + s * H[i]) + t * V[i]) - o[i] for i in range(3)]
        return ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]).astype(f32)


def window_variance(planes, radius):
    """the per-channel window variance the rectify statement takes the square root of, for the pixels it clamps (not passed through)
    -> a flat float32 array"""
    _, d = rectify_lib.rectify_numpy(*planes, radius=radius, gamma=1.0, details=True)
    return d["var"][~d["through"]].astype(f32).reshape(-1)
