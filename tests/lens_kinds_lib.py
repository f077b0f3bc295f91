"""TEST INFRASTRUCTURE for tptDrawDeviceLens across BASES, SPANS, ORIGINS, SIZES, FRAMES, SAMPLE COUNTS and SCENES: the cases of
tests/test_lens_kinds.py (the checker and the host emulation of the draw, on the CPU) and tests/test_gpu_lens_kinds.py (the lane-refill
kernel's lens mode on the GPU).  Nothing under toypathtracer_amd/ imports this module.  Run as a program (python tests/lens_kinds_lib.py
ROOT [SECTION ...], with TPT_LIB naming the host-emulation build of tests/test_lens_abi.py) it is the child process of
tests/test_lens_kinds.py: the sections' cases (all of them when none is named; `own` stands for tests/test_gpu_lens.py's own lenses)
drawn through the product's own mapItem, laneLens, hitSpheres and lanePost and held byte for byte, counter included, against the checker.

A CASE is a name, a lens, a size, a sample count, a frame and a scene, and how it is drawn: the flags, what the tile holds before
(`start`: None for zeros, "noise" for lens_lib.noise_tile), the fold and the LDS switch of tptSetKernelVariant.  Every comparison is of
bytes and of the ray count; tests/test_lens_kinds.py proves on the checker that each case is what its name says.

SECTIONS
  bases     per kind at 37 x 19, 4 spp: a basis with squared lengths 0.9901, 1.0099, 0.9901 and the three dot products +0.0099
            (`skew+`) or -0.0099 (`skew-`), made from lens_lib.make_lens's basis by the Cholesky factor of that Gram matrix in float64
            and rounded to binary32; make_lens's basis with `right` negated (`left-handed`); one rotated onto no axis (`rotated`)
  spans     FISHEYE and EQUIRECT with sx = sy = 2^-e, e in SCALES (EQUIRECT also EQUIRECT_TINY, where its arguments are subnormal);
            FISHEYE at GROUND_SCALES over a ground of radius 2^60, the one scene whose image shows a direction 2^-64 off forward's;
            FISHEYE with maxAngle 2^-126 and 2^-149 at sx = sy = 2; EQUIRECT one binary32 step below 2 pi x pi at 1 spp; ORTHO windows of 2^-126, 2^-149, 2^20, 2^64, FLT_MAX, and the window whose ray
            origins overflow on one side of the image (origin.x = 3e38, sx = 3.4e38)
  origins   origin.z = 2^e in front of the built-in scene, looking back at it: ORIGIN_NEAR for all kinds, ORIGIN_FAR for ORTHO with
            the 6 x 4 window; an origin on the surface of the glass sphere (every kind) and at its centre (the angular kinds)
  sizes     8192 x 8 and 8 x 8192 at 4 spp (the seam between 8 x 8 tiles and 256-pixel chunks depends on the device: seam_sizes)
  frames    FRAMES drawn progressively onto noise (EQUIRECT) and plainly onto zeros (FISHEYE)
  samples   SAMPLES on 8 x 8, the largest also on 1 x 1
  scenes    inside the closed glass and the inward mirror shell of tests/scene_kinds_lib.py, 0 / 15 / 16 / 17 lights of
            tests/lights_lib.py with the LDS scene chosen, forced in and forced out, the grouped scene with 300 lights, and the forward
            fold on the shell and on 17 lights"""
import collections
import ctypes as C
import os
import sys

import numpy as np

from lens_lib import EQUIRECT, FISHEYE, FLAG_PROGRESSIVE, FOLD_FORWARD, FOLD_RECURSIVE, KINDS, ORTHO, PI, TWO_PI, Lens, make_lens, noise_tile

f32 = np.float32
W, H, SPP = 37, 19, 4
Case = collections.namedtuple("Case", "name lens w h spp frame scene flags start fold lds")


def case(name, lens, w=W, h=H, spp=SPP, frame=0, scene="default", flags=0, start=None, fold=FOLD_RECURSIVE, lds=-1):
    return Case(name, lens, w, h, spp, frame, scene, flags, start, fold, lds)


def copy_lens(lens, **fields):
    out = Lens()
    C.memmove(C.byref(out), C.byref(lens), C.sizeof(Lens))
    for k, v in fields.items():
        if isinstance(v, (tuple, list, np.ndarray)):
            getattr(out, k)[:] = [float(f32(x)) for x in v]
        else:
            setattr(out, k, v)
    return out


def below(x):
    return float(np.nextafter(f32(x), f32(-np.inf)))


# ---------------------------------------------------------------- what a pixel's first sample is, restated in numpy
def first_uv(w, h, frame=0):
    """-> (u, v) [h, w] float32 of every pixel's first sample: the seed of ComputeShader.hlsl:380, two xorshift32 draws"""
    x, y = np.meshgrid(np.arange(w, dtype=np.uint32), np.arange(h, dtype=np.uint32))
    state = (x * np.uint32(1973) + y * np.uint32(9277) + np.uint32((frame * 26699) & 0xFFFFFFFF)) | np.uint32(1)
    out = []
    for _ in range(2):
        state = state ^ (state << np.uint32(13))
        state = state ^ (state >> np.uint32(17))
        state = state ^ (state << np.uint32(15))
        out.append((state & np.uint32(0xFFFFFF)).astype(f32) / f32(16777216))
    return (x.astype(f32) + out[0]) * (f32(1) / f32(w)), (y.astype(f32) + out[1]) * (f32(1) / f32(h))


def plane_coords(lens, w, h, frame=0):
    """-> (a, b) [h, w] float32: (u - 0.5f) * sx, (v - 0.5f) * sy of the first samples"""
    u, v = first_uv(w, h, frame)
    return (u - f32(0.5)) * f32(lens.sx), (v - f32(0.5)) * f32(lens.sy)


TINY = f32(2.0 ** -126)


def regimes(x):
    """which of normal / subnormal / zero the non-negative float32 values of x are -> a set"""
    x = np.asarray(x, f32)
    out = set()
    if (x >= TINY).any():
        out.add("normal")
    if ((x > 0) & (x < TINY)).any():
        out.add("subnormal")
    if (x == 0).any():
        out.add("zero")
    return out


# ---------------------------------------------------------------- 1. bases
SKEW_LEN2, SKEW_DOT = (0.9901, 1.0099, 0.9901), 0.0099
LEN2_BOUNDS, DOT_BOUNDS = (0.99, 1.01), (-0.01, 0.01)  # csrc/tpt_host_draw.cpp: lensFault, in double
CLEAR = 1e-4  # a skewed basis is further than this from the orthonormal one in every length and dot product


def gram(lens):
    """-> (squared lengths of right, up, forward; right . up, right . forward, up . forward) in float64, summed as lensFault sums"""
    v = [[float(x) for x in vec[:]] for vec in (lens.right, lens.up, lens.forward)]
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    return [dot(a, a) for a in v], [dot(v[0], v[1]), dot(v[0], v[2]), dot(v[1], v[2])]


def skewed(kind, sign, **kw):
    """make_lens's basis B (rows right, up, forward) -> L B with L L^T the Gram matrix wanted: float64, then rounded to binary32"""
    base = make_lens(kind, **kw)
    d = sign * SKEW_DOT
    g = np.array([[SKEW_LEN2[0], d, d], [d, SKEW_LEN2[1], d], [d, d, SKEW_LEN2[2]]], np.float64)
    rows = np.linalg.cholesky(g) @ np.array([base.right[:], base.up[:], base.forward[:]], np.float64)
    return copy_lens(base, right=rows[0], up=rows[1], forward=rows[2])


UNIT_MESSAGE = "a basis vector is not of unit length (its squared length must lie in 0.99..1.01)"
ORTHOGONAL_MESSAGE = "two basis vectors are not orthogonal (their dot product must lie in -0.01..0.01)"
BOUND_STEP, BOUND_CLEAR = 2e-6, 1e-6


def bound_records():
    """records a step either side of each bound of the basis rules -> [(name, lens, accepted, the refusal's message or None)]: the axes
    (1, 0, 0), (0, 1, 0), (0, 0, -1) with one vector scaled to a squared length of 0.99 -+ 2e-6 or 1.01 -+ 2e-6, or one vector tilted
    towards another to a dot product of +-(0.01 -+ 2e-6).  After the rounding to binary32 the float64 value lensFault computes is a clear
    1e-6 off the bound on the side wanted (asserted here), so the verdict does not hang on a rounding."""
    out = []
    fields = ("right", "up", "forward")

    def add(name, lens, value, bound, inside, message):
        assert abs(value - bound) >= BOUND_CLEAR and abs(value - bound) <= 2 * BOUND_STEP, (name, value)
        assert (lensfault_accepts(lens) is None) == inside, name
        out.append((name, lens, inside, None if inside else message))
    for i, field in enumerate(fields):
        for bound, side in ((0.99, -1), (0.99, 1), (1.01, -1), (1.01, 1)):
            lens = make_lens(EQUIRECT, forward=(0.0, 0.0, -1.0))
            lens = copy_lens(lens, **{field: np.array(getattr(lens, field)[:], np.float64) * np.sqrt(bound + side * BOUND_STEP)})
            inside = (side > 0) == (bound < 1)
            add("%s squared %g%+g" % (field, bound, side * BOUND_STEP), lens, gram(lens)[0][i], bound, inside, UNIT_MESSAGE)
    for n, (i, k) in enumerate(((0, 1), (0, 2), (1, 2))):
        for bound in (-0.01, 0.01):
            for side in (-1, 1):
                lens = make_lens(EQUIRECT, forward=(0.0, 0.0, -1.0))
                vi, vk = (np.array(getattr(lens, fields[j])[:], np.float64) for j in (i, k))
                lens = copy_lens(lens, **{fields[k]: vk + (bound + side * BOUND_STEP) * vi})
                inside = (side > 0) == (bound < 0)
                add("%s . %s %g%+g" % (fields[i], fields[k], bound, side * BOUND_STEP), lens, gram(lens)[1][n], bound, inside, ORTHOGONAL_MESSAGE)
    assert len(out) == 24 and sum(r[2] for r in out) == 12
    return out


def lensfault_accepts(lens):
    """the basis rules of lensFault restated on the float64 values -> None, or the message"""
    len2, dots = gram(lens)
    if not all(LEN2_BOUNDS[0] <= v <= LEN2_BOUNDS[1] for v in len2):
        return UNIT_MESSAGE
    if not all(DOT_BOUNDS[0] <= v <= DOT_BOUNDS[1] for v in dots):
        return ORTHOGONAL_MESSAGE
    return None


ROTATED = dict(forward=(0.3, -0.5, -0.8), up=(0.1, 1.0, 0.2))
BASES = ("skew+", "skew-", "left-handed", "rotated")


def basis_lens(kind, which):
    if which == "skew+":
        return skewed(kind, 1.0)
    if which == "skew-":
        return skewed(kind, -1.0)
    if which == "left-handed":
        base = make_lens(kind)
        return copy_lens(base, right=[-x for x in base.right[:]])
    return make_lens(kind, **ROTATED)


def bases_cases():
    return [case("basis-%s-%s" % (k, which), basis_lens(KINDS[k], which)) for k in sorted(KINDS) for which in BASES]


# ---------------------------------------------------------------- 2. spans
SCALES = (10, 30, 50, 62, 63, 64, 70, 73, 74, 80)
# what the fisheye's r * r = a * a + b * b is over the first samples of a 37 x 19 image (tests/test_lens_kinds.py holds it to this):
# |a|, |b| <= 2^-(e + 1), so r * r <= 2^-(2 e + 1): below 2^-126 from e = 63 on; a * a <= 2^-(2 e + 2) is at most half the smallest
# subnormal from e = 74 on and rounds to zero, so 2^-73 is the last scale before zero (a pixel near the centre gets there sooner)
FISHEYE_RR = {10: {"normal"}, 30: {"normal"}, 50: {"normal"}, 62: {"normal", "subnormal"}, 63: {"subnormal"}, 64: {"subnormal"},
              70: {"subnormal", "zero"}, 73: {"subnormal", "zero"}, 74: {"zero"}, 80: {"zero"}}
LAST_BEFORE_ZERO = 73
# the panorama's a and b are single products: still normal at 2^-80 (|u - 0.5| >= 2^-25 or so), subnormal from 2^-126 on, signed zeros
# at 2^-149
EQUIRECT_TINY = (126, 140, 149)
# On the built-in scene a direction that leaves forward's by 2^-64 draws the image forward draws: every sum absorbs it.  So that the
# bytes show whether r * r was flushed, the same lenses look along (0, 0, -1) over scene_kinds_lib's ground of radius 2^60: HitSpheres
# multiplies the direction's y, b k = 2^-65 or so, by the 2^60 to the ground's centre, and the hit moves by a tenth of a unit.
GROUND_SCALES, GROUND_SCENE = (63, 64, 70), "kind:ground_2^60"
MAX_ANGLES = {"2^-126": 2.0 ** -126, "2^-149": 2.0 ** -149}


def ground_lens(e):
    return make_lens(FISHEYE, forward=(0.0, 0.0, -1.0), sx=2.0 ** -e, sy=2.0 ** -e, max_angle=PI)
ORTHO_ORIGIN = (0.25, 1.0, 0.5)  # (no component is 0: origin + right * a is the origin itself once a is small enough)
ORTHO_TINY = {"2^-126": 2.0 ** -126, "2^-149": 2.0 ** -149}
FLT_MAX = float(np.finfo(f32).max)
ORTHO_HUGE = {"2^20": 2.0 ** 20, "2^64": 2.0 ** 64, "flt-max": FLT_MAX}
# how many pixels of the 37 x 19 image must hit something through a huge window: none.  The pixels are sx / 37 >= 28339 units apart
# along `right` and sy / 19 >= 55188 along `up`, and the scene, ground included, lies within 201 units of the origin: a sample hits only
# if its a and its b both fall into an interval of 402 units, and no sample of the checker's does (tests/test_lens_kinds.py asserts it)
ORTHO_HUGE_HITS = 0


def overflow_lens():
    return make_lens(ORTHO, origin=(3e38, 1.0, 0.5), forward=(0.0, 0.0, -1.0), sx=3.4e38, sy=4.0)


def spans_cases():
    out = []
    for e in SCALES:
        out.append(case("span-fisheye-2^-%d" % e, make_lens(FISHEYE, sx=2.0 ** -e, sy=2.0 ** -e, max_angle=PI)))
    for e in GROUND_SCALES:
        out.append(case("span-fisheye-2^-%d-over-the-2^60-ground" % e, ground_lens(e), scene=GROUND_SCENE))
    for name, angle in MAX_ANGLES.items():
        out.append(case("span-fisheye-max-angle-%s" % name, make_lens(FISHEYE, sx=2.0, sy=2.0, max_angle=angle)))
    for e in SCALES + EQUIRECT_TINY:
        out.append(case("span-equirect-2^-%d" % e, make_lens(EQUIRECT, sx=2.0 ** -e, sy=2.0 ** -e)))
    out.append(case("span-equirect-below-2pi-by-pi", make_lens(EQUIRECT, sx=below(TWO_PI), sy=below(PI)), spp=1))
    for name, window in ORTHO_TINY.items():
        out.append(case("span-ortho-%s" % name, make_lens(ORTHO, origin=ORTHO_ORIGIN, sx=window, sy=window)))
    for name, window in ORTHO_HUGE.items():
        out.append(case("span-ortho-%s" % name, make_lens(ORTHO, sx=window, sy=window)))
    out.append(case("span-ortho-overflow", overflow_lens()))
    return out


# ---------------------------------------------------------------- 3. origins
ORIGIN_NEAR, ORIGIN_FAR = (4, 8, 12, 20), (40, 63, 64, 100, 127)
# whether any sample of the case hits a sphere, as the checker has it (tests/test_lens_kinds.py asserts each and that both occur)
ORIGIN_HITS = {"origin-equirect-2^4": True, "origin-equirect-2^8": True, "origin-equirect-2^12": False, "origin-equirect-2^20": False,
               "origin-fisheye-2^4": True, "origin-fisheye-2^8": True, "origin-fisheye-2^12": False, "origin-fisheye-2^20": False,
               "origin-ortho-2^4": True, "origin-ortho-2^8": True, "origin-ortho-2^12": False, "origin-ortho-2^20": False,
               "origin-ortho-2^40": False, "origin-ortho-2^63": False, "origin-ortho-2^64": False, "origin-ortho-2^100": False,
               "origin-ortho-2^127": False}
GLASS = 7  # the glass sphere of the built-in scene


def glass_sphere():
    from lens_lib import default_scene
    s, _ = default_scene()
    return np.array([s["cx"][GLASS], s["cy"][GLASS], s["cz"][GLASS]], f32), f32(s["radius"][GLASS])


def origins_cases():
    out = []
    for k in sorted(KINDS):
        for e in ORIGIN_NEAR + (ORIGIN_FAR if KINDS[k] == ORTHO else ()):
            out.append(case("origin-%s-2^%d" % (k, e), make_lens(KINDS[k], origin=(0.0, 1.0, 2.0 ** e))))
    c, r = glass_sphere()
    for k in sorted(KINDS):
        out.append(case("origin-%s-on-the-surface" % k, make_lens(KINDS[k], origin=(c[0] + r, c[1], c[2]), forward=(-1.0, -0.1, 0.3))))
    for k in ("equirect", "fisheye"):
        out.append(case("origin-%s-at-the-centre" % k, make_lens(KINDS[k], origin=tuple(c), forward=(0.3, -0.2, -1.0))))
    return out


# ---------------------------------------------------------------- 4. sizes
def sizes_cases():
    return [case("size-8192x8-equirect", make_lens(EQUIRECT), w=8192, h=8, frame=3),
            case("size-8x8192-fisheye", make_lens(FISHEYE, max_angle=PI), w=8, h=8192, frame=3)]


def items_of(w, h):
    """the work items of a lens launch: whole 8 x 8 tiles"""
    return ((w + 7) // 8) * ((h + 7) // 8) * 64


def seam_shape(t):
    """2 t x t tiles, the last tile of every row and column a single pixel wide: no side a multiple of 8"""
    return 8 * (2 * t - 1) + 1, 8 * (t - 1) + 1


def seam_sizes(resident):
    """-> ((w, h) of the smallest image of seam_shape that takes 256-pixel chunks, (w, h) of the one before it, which takes tiles):
    laneRefillChunks takes chunks of 256 once numItems / 256 >= 8 * resident, that is numItems >= 2048 * resident"""
    t = 2
    while items_of(*seam_shape(t)) < 2048 * resident:
        t += 1
    above, under = seam_shape(t), seam_shape(t - 1)
    assert items_of(*under) < 2048 * resident <= items_of(*above) and items_of(*above) == 128 * t * t
    assert all(side % 8 for side in above + under) and max(above) <= 8192, (above, under)
    return above, under


def emulated_resident(cus, lds):
    """the workgroups resident at once on the emulated device: tests/hostemu/hostemu_kernels.cpp's tptTraceOccupancy, restated"""
    return cus * min(max(160 * 1024 // (lds + 256), 1), 16)


def seam_cases(resident):
    (w1, h1), (w0, h0) = seam_sizes(resident)
    return [case("size-%dx%d-chunks-of-256" % (w1, h1), make_lens(EQUIRECT), w=w1, h=h1, spp=1, frame=1),
            case("size-%dx%d-tiles" % (w0, h0), make_lens(EQUIRECT), w=w0, h=h0, spp=1, frame=1)]


# ---------------------------------------------------------------- 5. frames and samples
def wrapping_frame():
    """the first frame below 2^31 - 1 whose frame * 26699 wraps to k = 1, 2, 3, ... (mod 2^32): (frame, k)"""
    inv = pow(26699, -1, 1 << 32)
    for k in range(1, 64):
        f = (k * inv) & 0xFFFFFFFF
        if 1 << 24 < f < (1 << 31) - 1:
            return f, k
    raise AssertionError("no frame wraps to a small number")


# frameCount = 2^31 - 1 is NOT in this list: frameCount + 1 overflows a signed int in the reference's own statement of the blend
# (Test.cpp:272), in the checker and in makeFrameConsts alike, so there is nothing defined to hold the draw against
FRAMES = {"2^24+1": (1 << 24) + 1, "2^31-2": (1 << 31) - 2, "wrapping": wrapping_frame()[0]}
SAMPLES = (1, 2, 3, 64, 2047, 2048, 65536)


def frames_cases():
    out = []
    for name, frame in FRAMES.items():
        out.append(case("frame-%s-progressive-onto-noise" % name, make_lens(EQUIRECT), frame=frame, flags=FLAG_PROGRESSIVE, start="noise"))
        out.append(case("frame-%s-plain-onto-zeros" % name, make_lens(FISHEYE), frame=frame))
    return out


def samples_cases():
    kinds = sorted(KINDS)
    out = [case("samples-%d-%s" % (n, kinds[i % 3]), make_lens(KINDS[kinds[i % 3]]), w=8, h=8, spp=n, frame=1) for i, n in enumerate(SAMPLES)]
    out.append(case("samples-65536-one-pixel", make_lens(FISHEYE, max_angle=PI), w=1, h=1, spp=SAMPLES[-1], frame=1))
    return out


# ---------------------------------------------------------------- 6. scenes
LIGHTS, LDS_SWITCH = (0, 15, 16, 17), {"chosen": -1, "in-lds": 1, "out-of-lds": 0}
STRESS_ORIGIN = dict(origin=(0.0, 6.0, 20.0), forward=(0.0, -6.0, -20.0))  # toypathtracer_amd.scenes.STRESS_CAMERA's place and view
_scenes = {}


def scene(name):
    """-> (spheres, materials), built once"""
    if name not in _scenes:
        import lights_lib
        import scene_kinds_lib
        from lens_lib import default_scene
        kind, _, arg = name.partition(":")
        if name == "default":
            _scenes[name] = default_scene()
        elif kind == "kind":
            _scenes[name] = scene_kinds_lib.scene(arg)[:2]
        elif kind == "lights":
            _scenes[name] = lights_lib.default_with_lights(int(arg), seed=int(arg) + 1)
        elif name == "lights_grouped":
            _scenes[name] = lights_lib.stress_with_lights(1000, 20, 300)
        else:
            raise KeyError(name)
    return _scenes[name]


def scenes_cases():
    kinds = sorted(KINDS)
    out = [case("scene-shell-glass-equirect", make_lens(EQUIRECT), scene="kind:shell_glass"),
           case("scene-shell-mirror-fisheye", make_lens(FISHEYE, max_angle=PI), scene="kind:shell_mirror_inward")]
    n = 0
    for k in LIGHTS:
        for name, lds in LDS_SWITCH.items():
            out.append(case("scene-%d-lights-%s-%s" % (k, name, kinds[n % 3]), make_lens(KINDS[kinds[n % 3]]), scene="lights:%d" % k, lds=lds))
            n += 1
    out.append(case("scene-grouped-300-lights-equirect", make_lens(EQUIRECT, **STRESS_ORIGIN), scene="lights_grouped"))
    out.append(case("scene-shell-glass-forward-fold-ortho", make_lens(ORTHO), scene="kind:shell_glass", fold=FOLD_FORWARD))
    out.append(case("scene-17-lights-forward-fold-fisheye", make_lens(FISHEYE), scene="lights:17", fold=FOLD_FORWARD))
    return out


def own_cases():
    """tests/test_gpu_lens.py's own lenses: make_lens's defaults at its sizes and sample counts, and its spans"""
    import test_gpu_lens as own
    out = [case("own-%s-%dx%d-spp%d" % (k, w, h, spp), make_lens(KINDS[k]), w=w, h=h, spp=spp, frame=2)
           for k in sorted(KINDS) for w, h in own.SIZES for spp in (1, 4)]
    return out + [case("own-" + name, own.SPANS[name]()) for name in sorted(own.SPANS)]


SECTIONS = {"bases": bases_cases, "spans": spans_cases, "origins": origins_cases, "sizes": sizes_cases, "frames": frames_cases,
            "samples": samples_cases, "scenes": scenes_cases}
_cases = {}


def cases(section):
    if section not in _cases:
        _cases[section] = (own_cases if section == "own" else SECTIONS[section])()
        names = [c.name for c in _cases[section]]
        assert len(set(names)) == len(names), "two cases share a name"
    return _cases[section]


def start_tile(c):
    return None if c.start is None else noise_tile(c.w, c.h)


def reference(checker, c, threads=0):
    """-> (HitWorld calls, tile [h, w, 4]) of the checker for this case"""
    s, m = scene(c.scene)
    start = start_tile(c)
    return checker.render(s, m, c.lens, c.w, c.h, c.spp, c.frame, flags=c.flags, backbuffer=None if start is None else start.copy(), fold=c.fold,
                          threads=threads)


def differs(got, want):
    """(tile, rays) against the checker's (rays, tile) -> None, or what differs"""
    tile, rays = got
    want_rays, want_tile = want
    if tile.tobytes() != want_tile.tobytes():
        bad = np.argwhere(tile.view(np.uint32) != want_tile.view(np.uint32))
        at = tuple(bad[0][:2])
        return "%d words differ, first at %s: %r / %r" % (len(bad), bad[0].tolist(), tile[at], want_tile[at])
    return None if rays == want_rays else "the counter gained %d, the checker counts %d" % (rays, want_rays)


# ---------------------------------------------------------------- the child process: the cases through the host emulation
def _emu_main(root, sections):
    import tempfile
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    from toypathtracer_amd import api as tpt
    from lens_lib import LensChecker, to_api
    sys.stdout.reconfigure(line_buffering=True)  # (a run that has to be killed still says how far it came)
    checker = LensChecker(tempfile.mkdtemp(prefix="lens_kinds_"))
    tpt.load_library()
    so = C.CDLL(tpt.library_path())
    plan = (C.c_longlong * 8)()
    tpt.InitializeTest()
    failed = 0
    for section in sections:
        if section == "seam":  # the tile / chunk seam of this emulated device (HOSTEMU_CUS names its CUs)
            tile = np.zeros((8, 8, 4), f32)
            tpt.set_scene(None, None)
            tpt.set_kernel_variant(0, 3, -1)
            tpt.set_fold_mode(FOLD_RECURSIVE)
            tpt.UpdateTest(0.0, 0, 8, 8, 0)
            tpt.draw_device_lens(0, 8, 8, tile.ctypes.data, to_api(make_lens(EQUIRECT)))
            tpt.synchronize()
            so.hostemuLensPlan(plan)
            todo = seam_cases(emulated_resident(int(os.environ["HOSTEMU_CUS"]), plan[5]))
        else:
            todo = cases(section)
        for c in todo:
            s, m = scene(c.scene)
            tpt.set_scene(None, None) if c.scene == "default" else tpt.set_scene(s, m)
            tpt.set_kernel_variant(0, 3, c.lds)
            tpt.set_fold_mode(c.fold)
            tpt.set_samples_per_pixel(c.spp)
            tpt.UpdateTest(0.0, 0, c.w, c.h, 0)
            print("case: %s: begins" % c.name)
            buf = np.full((c.h + 2, c.w, 4), np.nan, f32)  # a guard row below and above
            start = start_tile(c)
            buf[1:-1] = 0 if start is None else start
            cnt = np.array([5, 1000, 5], np.uint64)
            r0 = tpt.ray_counter_read()
            tpt.draw_device_lens(c.frame, c.w, c.h, buf.ctypes.data + 16 * c.w, to_api(c.lens), c.flags, cnt.ctypes.data + 8)
            tpt.synchronize()
            assert tpt.ray_counter_read() == r0, "the context's ray counter moved"
            assert np.isnan(buf[0]).all() and np.isnan(buf[-1]).all() and cnt[0] == 5 and cnt[2] == 5, "a guard was written"
            so.hostemuLensPlan(plan)
            why = differs((buf[1:-1], int(cnt[1]) - 1000), reference(checker, c))
            failed += why is not None
            print("case: %s: %s (chunks of %d)" % (c.name, "equal" if why is None else "DIFFERS: " + why, plan[1]))
    tpt.set_scene(None, None)
    tpt.ShutdownTest()
    print("failed: %d" % failed)
    if failed:
        sys.exit(1)
    print("ok")


if __name__ == "__main__":
    _emu_main(sys.argv[1], sys.argv[2:] or list(SECTIONS))
