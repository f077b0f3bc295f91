"""TEST INFRASTRUCTURE for tptTraceRaysDevice across RAY LENGTHS, SEED WORDS, RECORDS OUTSIDE THE DOMAIN and SCENES: the ray families, the
scene list and the three comparators of tests/test_rays_kinds.py (the checker and the host emulation of the lane logic, on the CPU) and
tests/test_gpu_rays_kinds.py (the lane-refill kernel's ray mode on the GPU).  Nothing under toypathtracer_amd/ imports this module.  Run
as a program (python tests/rays_kinds_lib.py ROOT, with TPT_LIB naming a host-emulation build of the library) it is the child process
of tests/test_rays_kinds.py: every family and a subset of the scenes through the product's own laneBeginRay, rayDirFitsFilter,
hitSpheres, rayHitRecord and lanePost.

COMPARATORS
  equal_bits          byte equality of radiance, hit records and the counter's gain: wherever the reference is wholly finite
  equal_bits_or_nan   per 32-bit word: where the reference word is a NaN the other side's word is a NaN of any pattern (x86 makes
                      0xffc00000, the GPU 0x7fc00000; a NaN's pattern is not part of the contract), every other word is bit-equal; the
                      id word (hits[7]) and the k word (radiance[3]) are compared as bits always
  own_outputs_only    for records the header does not define (a non-finite component, a zero direction): the good rays' outputs are
                      the checker's for the good rays traced alone; every bad ray's records were written (the outputs start as GUARD, a
                      pattern no arithmetic makes); its k is an integer in 1 .. 11 (1 + nLights) -- kMaxDepth + 1 main rays, each with
                      at most one shadow ray per light: Trace's own bound --, its id in -1 .. nSpheres - 1; the counter gained the sum
                      of the written k

FAMILIES (each seeded and built against a scene; tests/test_rays_kinds.py asserts on the checker alone what is said here)
  length_seam    grazing rays (common.grazing_rays and rays_lib's tangent lines, eps +-1e-7 .. +-1e-5) whose direction is rescaled until
                 the kernel's own float32 dd = d.x*d.x + d.y*d.y + d.z*d.z IS a chosen value: 0.99999f and 1.00001f, the float32
                 neighbour on either side of each, and 1.0 (SEAM_CLASSES; found by search on the float32 result).  64 rays a class,
                 of which at least 8 hit their sphere with a float32 discriminant below 2^-10 r^2 and at least 8 miss.
                 WHAT THIS CANNOT SHOW: on either side of a limit the exact test and the filtered one give the same bits.  The filter
                 keeps a sphere when (K nb)^2 - S + r^2 (1 + 2^-16) >= 0 with the SAME scaled nb = co . d the exact test uses, so at
                 a hit (nb^2 >= S - r^2) it has 2^-17 nb^2 + 2^-16 r^2 >= 2^-17 S to spare against roundings of 13 u (S + r^2), whatever
                 |d| is; a limit that is off by an ulp, or `<` for `<=`, changes which code runs and no output.  What the seam classes
                 hold is that BOTH sides are right at the limit.  The same holds for the flat filter with limits as wide as 0.9 .. 1.1.
                 It does not hold for the group bounds, whose argument is geometric: with |d| > 1 the reference accepts a sphere the
                 ray's line passes at a distance (dist^2 <= r^2 + (|d|^2 - 1) w^2, w the way along the ray), while the bound of its
                 group, nearer the origin and further from the line, is rejected.  Two classes beyond the limits show it: `short`
                 (dd = 0.91f) and `long` (dd = 1.09f).  The kernel takes the exact test there; rayDirFitsFilter widened to
                 0.9 .. 1.1 fails `long` on the grouped scene (and passes on a flat one, as argued).
  length_range   camera rays, rays from inside a glass sphere and (for the three long scales) rays from 1e6 .. 1e14 away, the direction
                 scaled by 2^-23, 2^-20, 2^-10, 2^3, 2^10, 2^13.  Per (ray, sphere) the reference's roots fall BELOW kMinT (the near root
                 is at or below it: the far root is taken, or the sphere rejected), BETWEEN the limits (a hit), or ABOVE kMaxT (rejected
                 against the initial hitT).  RANGE_CLASSES says which of the three each scale can have: with |d| = 2^-10 and shorter a
                 ray from outside has nb^2 < c and no root at all, so only the inside rays reach a sphere, all of them through the far
                 root, which is about the radius: nothing above kMaxT.  The long scales have all three (above: the near root, about
                 distance / 2 |d|, passes 1e7 only from the far origins).  Also: directions with components that are 0, -0.0f or
                 denormal (1e-45, 1e-39), origins at a sphere's centre and at centre + (r, 0, 0), |d|^2 that underflows to 0 (2^-80)
                 and that overflows to +inf (a 3e38 component), and rays whose near root IS kMinT in float32 (found by search:
                 `t <= tMin` takes the far root).
                 All finite, non-zero directions: in the domain.  equal_bits_or_nan; at least half the family is wholly finite.
  seed_words     the same camera rays under each of SEED_WORDS, written through a uint32 view.  equal_bits; 0 gives 1's outputs.
  outside_domain 1024 camera rays with records the header does not define at lane 0, lane 63, a whole wave (128 .. 191), every fourth
                 ray of 256 .. 511, the first ray of a partial last chunk of 256 and of 64 when the first 1000 are traced alone (768,
                 960), and the last ray of either call (999, 1023): NaN, +Inf, -Inf in each of the six components, a zero direction
                 from outside the spheres and from inside a glass sphere, all six NaN.  own_outputs_only."""
import os
import sys

import numpy as np

f32 = np.float32
GUARD = 0x7FC12345  # a quiet NaN with a payload: what the outputs hold before a call
K_MIN_T, K_MAX_T, MAX_DEPTH = f32(0.001), f32(1.0e7), 10
SHAPE = (24, 16)  # the frame whose first-sample camera rays a scene case traces


# ---------------------------------------------------------------- comparators
def is_nan_word(w):
    w = np.asarray(w).view(np.uint32)
    return ((w & np.uint32(0x7F800000)) == np.uint32(0x7F800000)) & ((w & np.uint32(0x007FFFFF)) != 0)


def _words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _differ(what, name, g, w, bad):
    i = np.argwhere(bad)
    raise AssertionError("%s: %s: %d words differ, first at %s: %s / %s" % (
        what, name, len(i), i[0].tolist(), ["%08x" % v for v in g[i[0][0]]], ["%08x" % v for v in w[i[0][0]]]))


def equal_bits(got, want, what):
    """got, want: (counter gain, radiance [n, 4] or None, hits [n, 8] or None)"""
    for g, w, name in ((got[1], want[1], "radiance"), (got[2], want[2], "hits")):
        if g is None and w is None:
            continue
        g, w = _words(g), _words(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if (g != w).any():
            _differ(what, name, g, w, g != w)
    assert got[0] == want[0], (what, "the counter gained %d, the reference counts %d" % (got[0], want[0]))


def equal_bits_or_nan(got, want, what):
    """-> whether plain byte equality held as well"""
    plain = True
    for g, w, name, bits_word in ((got[1], want[1], "radiance", 3), (got[2], want[2], "hits", 7)):
        if g is None and w is None:
            continue
        g, w = _words(g), _words(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        either = is_nan_word(w) & is_nan_word(g)
        either[:, bits_word] = False  # the k word and the id word: bits
        bad = (g != w) & ~either
        if bad.any():
            _differ(what, name, g, w, bad)
        plain = plain and not (g != w).any()
    assert got[0] == want[0], (what, "the counter gained %d, the reference counts %d" % (got[0], want[0]))
    return plain


def nan_words(want):
    """how many words of a reference result are NaN, and how many of its rays are wholly finite"""
    rad, hit = _words(want[1]), _words(want[2])
    finite = np.isfinite(want[1][:, :3]).all(axis=1) & np.isfinite(want[2][:, :7]).all(axis=1)
    return int(is_nan_word(rad[:, :3]).sum() + is_nan_word(hit[:, :7]).sum()), int(finite.sum())


def wholly_finite(want):
    return bool(np.isfinite(want[1][:, :3]).all() and np.isfinite(want[2][:, :7]).all())


def own_outputs_only(got, bad, want_good, n_lights, n_spheres, what):
    """got: (counter gain, radiance [n, 4], hits [n, 8]) of a call whose outputs started as GUARD; bad: [n] bool; want_good: the
    checker's (total, radiance, hits) for rays[~bad] traced alone"""
    gain, rad, hit = got
    good = ~bad
    equal_bits((want_good[0], rad[good], hit[good]), want_good, what + ": the good rays")  # (a)
    r, h = _words(rad), _words(hit)
    assert not (r[bad] == np.uint32(GUARD)).any() and not (h[bad] == np.uint32(GUARD)).any(), (what, "a bad ray's record was not written")  # (b)
    k = rad[bad, 3]
    assert (k == np.floor(k)).all() and (k >= 1).all() and (k <= (MAX_DEPTH + 1) * (1 + n_lights)).all(), (what, "k", k)  # (c)
    ids = h[bad, 7].view(np.int32)
    assert (ids >= -1).all() and (ids < n_spheres).all(), (what, "ids", ids)
    assert gain == int(rad[:, 3].astype(np.float64).sum()), (what, "the counter gained %d, the written k sum to %d" % (gain, rad[:, 3].sum()))  # (d)


# ---------------------------------------------------------------- the reference's sphere test, restated per (ray, sphere) in numpy
def dd_of(d):
    """the kernel's own expression in float32, in its order"""
    d = np.asarray(d, f32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def sphere_roots(spheres, rays, ids=None):
    """HitSpheres' arithmetic (Maths.cpp:171-190) in float32 -> (discr, near root, the root taken) per ray against sphere ids[i], or as
    [n, nSpheres] against every sphere.  The root taken is near, or far where near <= kMinT; NaN where discr <= 0."""
    o, d = rays[:, 0:3].astype(f32), rays[:, 4:7].astype(f32)
    if ids is None:
        c = np.stack([spheres["cx"], spheres["cy"], spheres["cz"]], 1).astype(f32)[None]
        r2 = (spheres["radius"] * spheres["radius"]).astype(f32)[None]
        o, d = o[:, None], d[:, None]
    else:
        c = np.stack([spheres["cx"][ids], spheres["cy"][ids], spheres["cz"][ids]], 1).astype(f32)
        r2 = (spheres["radius"][ids] * spheres["radius"][ids]).astype(f32)
    with np.errstate(all="ignore"):
        co = c - o
        nb = (co[..., 0] * d[..., 0] + co[..., 1] * d[..., 1]) + co[..., 2] * d[..., 2]
        cc = ((co[..., 0] * co[..., 0] + co[..., 1] * co[..., 1]) + co[..., 2] * co[..., 2]) - r2
        discr = nb * nb - cc
        sq = np.sqrt(np.where(discr > 0, discr, f32(np.nan)), dtype=f32)
        near = nb - sq
        taken = np.where(near <= K_MIN_T, nb + sq, near)
    return discr, near, taken


# ---------------------------------------------------------------- rays
def make_rays(o, d, seeds):
    from rays_lib import make_rays as make
    return make(o, d, seeds)


def _seeds(n, salt):
    return ((np.arange(n, dtype=np.uint64) * 2654435761 + salt) % 0xFFFFFFFF + 1).astype(np.uint32)


def pick_glass(spheres, mats):
    """a dielectric sphere of ordinary size: the built-in scene's sphere 7, else the largest dielectric that is not the ground"""
    if len(spheres) == 46:
        return 7
    glass = np.nonzero((mats["type"] == 2) & (np.arange(len(spheres)) > 0))[0]
    return int(glass[np.argmax(spheres["radius"][glass])])


def centre_of(spheres, i):
    return np.array([spheres["cx"][i], spheres["cy"][i], spheres["cz"][i]], f32)


_below = lambda v: np.nextafter(f32(v), f32(-np.inf), dtype=f32)
_above = lambda v: np.nextafter(f32(v), f32(np.inf), dtype=f32)
LO, HI = f32(0.99999), f32(1.00001)
SEAM_CLASSES = {"lo-1": _below(LO), "lo": LO, "lo+1": _above(LO), "one": f32(1.0), "hi-1": _below(HI), "hi": HI, "hi+1": _above(HI)}
SEAM_NEIGHBOURS = ("lo-1", "lo+1", "hi-1", "hi+1")
BEYOND = {"short": f32(0.91), "long": f32(1.09)}  # |d| = 0.954 and 1.044: well outside the limits, inside a switch widened to 0.9 .. 1.1
SEAM_PER_CLASS = 64
GRAZING = f32(2.0 ** -10)


def rescale_to(d, target, steps=257, width=6e-7):
    """d [n, 3] float32 -> (d' [n, 3], found [n]): d * s for the float64 s near sqrt(target / dd) at which the float32 dd of the
    rounded product IS target, by search on the float32 result"""
    d64 = d.astype(np.float64)
    s0 = np.sqrt(np.float64(target) / (d64 * d64).sum(axis=1))
    s = s0[:, None] * (1.0 + np.linspace(-width, width, steps))[None, :]
    cand = (d64[:, None, :] * s[:, :, None]).astype(f32)
    hit = dd_of(cand) == f32(target)
    found = hit.any(axis=1)
    first = np.argmax(hit, axis=1)
    return cand[np.arange(len(d)), first], found


def _tangent_rays(spheres, n, rng):
    """rays_lib.catalogue's `tangent` construction around spheres of the scene, eps in +-1e-7 .. +-1e-5"""
    idx = rng.integers(1, len(spheres), n) if len(spheres) > 1 else np.zeros(n, np.int64)
    c = np.stack([spheres["cx"][idx], spheres["cy"][idx], spheres["cz"][idx]], 1).astype(f32)
    r = np.abs(spheres["radius"][idx]).astype(f32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    side = np.cross(d, rng.normal(size=(n, 3)))
    side = (side / np.linalg.norm(side, axis=1, keepdims=True)).astype(f32)
    eps = (10.0 ** rng.uniform(-7, -5, n) * rng.choice([-1.0, 1.0], n)).astype(f32)
    p = c + side * (r * (f32(1) + eps))[:, None]
    return np.concatenate([p - d * f32(4.0), d], 1).astype(f32)


def length_seam(checker, spheres, mats, seed=17, pool=3000):
    """-> (rays [n, 8], classes: name -> slice).  The choice of rays within a class is made from the reference alone."""
    from common import grazing_rays
    rng = np.random.default_rng(seed)
    targets = dict(SEAM_CLASSES, **BEYOND)
    out, classes, at = [], {}, 0
    for k, (name, target) in enumerate(targets.items()):
        base = np.concatenate([grazing_rays(spheres, pool, seed=seed + 100 + k), _tangent_rays(spheres, pool, rng)])
        d, found = rescale_to(base[:, 3:6], target)
        rays = make_rays(base[found, 0:3], d[found], _seeds(int(found.sum()), 71 + k))
        assert (dd_of(rays[:, 4:7]) == target).all()
        _, _, hits = checker.trace(spheres, mats, rays, radiance=False)
        ids = hits[:, 7].view(np.int32)
        hit = ids >= 0
        discr = np.full(len(rays), np.inf, f32)
        discr[hit] = sphere_roots(spheres, rays[hit], ids[hit])[0]
        r2 = np.zeros(len(rays), f32)
        r2[hit] = (spheres["radius"][ids[hit]] * spheres["radius"][ids[hit]]).astype(f32)
        graze = np.nonzero(hit & (discr < GRAZING * r2))[0]
        miss = np.nonzero(~hit)[0]
        other = np.nonzero(hit & ~(discr < GRAZING * r2))[0]
        n = SEAM_PER_CLASS
        take = np.concatenate([graze[:n * 4 // 9], miss[:n * 3 // 9]])
        take = np.concatenate([take, other[:n - len(take)]])
        take = np.concatenate([take, np.setdiff1d(np.arange(len(rays)), take)[:n - len(take)]])
        out.append(rays[np.sort(take)])
        classes[name] = slice(at, at + len(take))
        at += len(take)
    return np.ascontiguousarray(np.concatenate(out)), classes


def seam_census(checker, spheres, mats, rays, classes):
    """per class: (rays, grazing hits, misses), from the reference"""
    _, _, hits = checker.trace(spheres, mats, rays, radiance=False)
    ids = hits[:, 7].view(np.int32)
    out = {}
    for name, sl in classes.items():
        i, r = ids[sl], rays[sl]
        hit = i >= 0
        discr = sphere_roots(spheres, r[hit], i[hit])[0]
        r2 = (spheres["radius"][i[hit]] * spheres["radius"][i[hit]]).astype(f32)
        out[name] = (len(i), int((discr < GRAZING * r2).sum()), int((~hit).sum()))
    return out


RANGE_SCALES = (-23, -20, -10, 3, 10, 13)
RANGE_CLASSES = {-23: ("below", "between"), -20: ("below", "between"), -10: ("below", "between"),
                 3: ("below", "between", "above"), 10: ("below", "between", "above"), 13: ("below", "between", "above")}


def min_t_rays(spheres, i, want=8):
    """rays towards sphere i along +x whose NEAR root is kMinT exactly in the reference's float32 arithmetic: d = (s, 0, 0) with s about
    2^-8, the origin a few ulps outside the surface; found by search over s"""
    c, r = centre_of(spheres, i), f32(abs(spheres["radius"][i]))
    found = []
    for ulps in range(20, 400, 7):
        ox = f32(c[0] - r * f32(1 + ulps * 2.0 ** -23))
        L = f32(c[0] - ox)
        gap = np.float64(f32(f32(L * L) - f32(r * r)))  # (c of the reference's test, as it rounds it)
        # nb = L s, discr = nb^2 - gap, near = nb - sqrt(discr) = kMinT  <=>  nb = (gap + kMinT^2) / (2 kMinT)
        s0 = (gap + np.float64(K_MIN_T) ** 2) / (2 * np.float64(K_MIN_T)) / np.float64(L)
        s = f32(s0)
        cand = np.empty(4001, f32)
        v = s
        for _ in range(2000):
            v = _below(v)
        for k in range(4001):
            cand[k] = v
            v = _above(v)
        rays = np.zeros((len(cand), 8), f32)
        rays[:, 0:3] = (ox, c[1], c[2])
        rays[:, 4] = cand
        _, near, _ = sphere_roots(spheres, rays, np.full(len(cand), i))
        for k in np.nonzero(near == K_MIN_T)[0][:2]:
            found.append(rays[k])
        if len(found) >= want:
            break
    return np.array(found[:want], f32).reshape(-1, 8)


def length_range(checker, spheres, mats, cam, seed=23):
    """-> (rays, parts: name -> slice)"""
    rng = np.random.default_rng(seed)
    glass = pick_glass(spheres, mats)
    c, r = centre_of(spheres, glass), f32(spheres["radius"][glass])
    camera = checker.camera_rays(cam, 40, 25)
    camera = camera[rng.permutation(len(camera))[:40]]
    n = 24
    d = rng.normal(size=(n, 3))
    inside = make_rays(c + (rng.uniform(-0.5, 0.5, (n, 3)) * r).astype(f32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32), _seeds(n, 11))
    n = 24
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    dist = (10.0 ** np.linspace(6, 14, n)).astype(f32)
    far = make_rays(c + rng.uniform(-0.3, 0.3, (n, 3)).astype(f32) * r - d * dist[:, None], d, _seeds(n, 53))
    parts, out, at = {}, [], 0

    def add(name, rays):
        nonlocal at
        rays = np.ascontiguousarray(rays, f32).reshape(-1, 8)
        parts[name] = slice(at, at + len(rays))
        out.append(rays)
        at += len(rays)
    for e in RANGE_SCALES:
        base = np.concatenate([camera, inside] + ([far] if e > 0 else [])).copy()
        base[:, 4:7] *= f32(2.0 ** e)
        add("scale_2^%d" % e, base)
    # components that are 0, -0.0f or denormal, one or two of them
    special = camera[:24].copy()
    values = np.array([0.0, -0.0, 1e-45, 1e-39, -1e-45, -1e-39], np.float64).astype(f32)
    for k in range(24):
        special[k, 4 + k % 3] = values[k % 6]
        if k >= 12:
            special[k, 4 + (k + 1) % 3] = values[(k // 3) % 6]
    add("zero_and_denormal_components", special)
    # origins at a sphere's centre and at centre + (r, 0, 0)
    n = 12
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    o = np.tile(c, (n, 1))
    o[n // 2:, 0] = c[0] + r
    add("centre_and_surface_origins", make_rays(o, d, _seeds(n, 61)))
    tiny = np.concatenate([camera[24:28], inside[:4]]).copy()
    tiny[:, 4:7] *= f32(2.0 ** -80)
    assert (dd_of(tiny[:, 4:7]) == 0).all() and (tiny[:, 4:7] != 0).any(axis=1).all()
    add("dd_underflows", tiny)
    huge = np.concatenate([camera[28:32], inside[4:8]]).copy()
    for k in range(len(huge)):
        huge[k, 4 + k % 3] = f32(3e38) * (1 if k % 2 else -1)
    with np.errstate(over="ignore"):
        assert np.isinf(dd_of(huge[:, 4:7])).all() and np.isfinite(huge).all()
    add("dd_overflows", huge)
    add("near_root_is_min_t", min_t_rays(spheres, glass))
    rays = np.ascontiguousarray(np.concatenate(out))
    assert np.isfinite(rays[:, [0, 1, 2, 4, 5, 6]]).all() and (rays[:, 4:7] != 0).any(axis=1).all(), "length_range left the domain"
    return rays, parts


def range_census(spheres, rays):
    """per ray: whether some sphere's roots fall below kMinT, between the limits, above kMaxT (the reference's arithmetic)"""
    discr, near, taken = sphere_roots(spheres, rays)
    with np.errstate(invalid="ignore"):
        real = discr > 0
        below = (real & (near <= K_MIN_T)).any(axis=1)
        between = (real & (taken > K_MIN_T) & (taken < K_MAX_T)).any(axis=1)
        above = (real & (taken >= K_MAX_T)).any(axis=1)
    return dict(below=below, between=between, above=above)


SEED_WORDS = (0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x7F800000, 0x7F800001, 0x7FC00000, 0xFFC00000, 0x00000001, 0x00800000)
SEED_RAYS = 40


def seed_words(checker, cam, seed=29):
    """-> rays [12 * 40, 8]: block j holds the same 40 camera rays with SEED_WORDS[j] as the seed word, put there through a uint32 view"""
    rng = np.random.default_rng(seed)
    camera = checker.camera_rays(cam, 40, 25)
    camera = camera[np.sort(rng.permutation(len(camera))[:SEED_RAYS])]
    rays = np.ascontiguousarray(np.tile(camera, (len(SEED_WORDS), 1)))
    rays.view(np.uint32)[:, 3] = np.repeat(np.array(SEED_WORDS, np.uint32), SEED_RAYS)
    assert rays.view(np.uint32)[:, 3].tolist() == np.repeat(np.array(SEED_WORDS, np.uint32), SEED_RAYS).tolist()
    return rays


OUTSIDE_N, OUTSIDE_SHORT = 1024, 1000
OUTSIDE_KINDS = 21


def outside_domain(checker, spheres, mats, cam):
    """-> (rays [1024, 8], bad [1024] bool)"""
    rays = checker.camera_rays(cam, 32, 32).copy()
    assert len(rays) == OUTSIDE_N
    where = sorted(set([0, 63] + list(range(128, 192)) + list(range(256, 512, 4)) + [768, 960, OUTSIDE_SHORT - 1, OUTSIDE_N - 1]))
    glass = pick_glass(spheres, mats)
    for n, i in enumerate(where):
        kind = (n + 5) % OUTSIDE_KINDS
        if kind < 18:
            rays[i, (0, 1, 2, 4, 5, 6)[kind % 6]] = (np.nan, np.inf, -np.inf)[kind // 6]
        elif kind == 18:
            rays[i, 4:7] = 0  # a zero direction from where the camera is
        elif kind == 19:
            rays[i, 4:7] = 0
            rays[i, 0:3] = centre_of(spheres, glass) + f32(0.25) * f32(spheres["radius"][glass])
        else:
            rays[i, [0, 1, 2, 4, 5, 6]] = np.nan
    bad = np.zeros(OUTSIDE_N, bool)
    bad[where] = True
    six = rays[:, [0, 1, 2, 4, 5, 6]]
    assert (bad == (~np.isfinite(six).all(axis=1) | (six[:, 3:] == 0).all(axis=1))).all()
    return np.ascontiguousarray(rays), bad


# ---------------------------------------------------------------- the scenes of the ray call
LIGHT_GROUPED = (1000, 20, 300)  # lights_lib.stress_with_lights at one grouped size
MANY = 65534
SEES_SKY = ()  # scenes excused from the hit rate of 0.2 because their camera sees sky: none needs it (the lowest rate is 0.3)
# the cases whose reference outputs are not wholly finite -- a zero radius has invRadius = inf, and a ray that meets it gets a normal of
# inf and NaN components --: equal_bits_or_nan there, equal_bits everywhere else (tests/test_rays_kinds.py holds the list to the checker)
NONFINITE_SCENES = ("kind:zero_radius", "kind:grouped_zero_radii", "kind:flat_zero_radii")


def scene_names():
    import lights_lib
    import scene_kinds_lib
    return (["kind:" + n for n in scene_kinds_lib.CATALOGUE] + ["lights:%d" % k for k in lights_lib.LIGHT_COUNTS]
            + ["light_kind:" + k for k in lights_lib.LIGHT_KINDS] + ["lights_grouped", "spheres_%d" % MANY])


def variant_scene_names(on_every_variant):
    return ["kind:" + n for n in on_every_variant] + ["lights:0", "lights:17", "lights:46", "spheres_%d" % MANY]


_scene_cache = {}


def scene_case(name, oracle):
    """-> (spheres, mats, oracle camera at SHAPE or None, grouped: True / False / None where the name does not say)"""
    import lights_lib
    import scene_kinds_lib
    import seams_lib
    if name in _scene_cache:
        return _scene_cache[name]
    w, h = SHAPE
    kind, _, arg = name.partition(":")
    if kind == "kind":
        s, m, camera = scene_kinds_lib.scene(arg)
        out = (s, m, scene_kinds_lib.oracle_camera(oracle, camera, w, h), arg in scene_kinds_lib.GROUPED)
    elif kind == "lights":
        s, m = lights_lib.default_with_lights(int(arg), seed=int(arg) + 1)
        out = (s, m, oracle.default_camera(w, h), False)
    elif kind == "light_kind":
        s, m = lights_lib.light_kind(arg)
        out = (s, m, oracle.default_camera(w, h), False)
    elif kind == "lights_grouped":
        from toypathtracer_amd.scenes import STRESS_CAMERA
        s, m = lights_lib.stress_with_lights(*LIGHT_GROUPED)
        out = (s, m, scene_kinds_lib.oracle_camera(oracle, STRESS_CAMERA, w, h), True)
    elif name == "spheres_%d" % MANY:
        s, m = seams_lib.scene(("many", MANY))
        out = (s, m, None, True)
    else:
        raise KeyError(name)
    _scene_cache[name] = out
    return out


def planted_rays(spheres, seed=37):
    """at most 256 rays aimed at the planted ids of seams_lib's many-sphere scene: from the default camera's place towards points of each
    planted sphere, grazing rays of the planted spheres, and a slice with the direction doubled"""
    import seams_lib
    from common import grazing_rays
    rng = np.random.default_rng(seed)
    ids = sorted(seams_lib.PLANTED)
    eye = np.array([0.0, 2.0, 3.0])
    o, d = [], []
    for i in ids:
        c, r = centre_of(spheres, i).astype(np.float64), min(float(spheres["radius"][i]), 2.0)
        for _ in range(12):
            p = c + rng.uniform(-0.6, 0.6, 3) * r
            v = p - eye
            o.append(eye)
            d.append(v / np.linalg.norm(v))
    aimed = make_rays(np.array(o, f32), np.array(d, f32), _seeds(len(o), 5))
    g = grazing_rays(spheres[ids], 72, seed=seed)
    graze = make_rays(g[:, 0:3], g[:, 3:6], _seeds(len(g), 7))
    doubled = aimed[::2][:64].copy()
    doubled[:, 4:7] *= f32(2)
    rays = np.ascontiguousarray(np.concatenate([aimed, graze, doubled]))
    assert len(rays) <= 256
    return rays


def scene_rays(checker, spheres, cam, seed=41):
    """the 24 x 16 first-sample camera rays, 128 grazing rays, and 64 camera rays with the direction doubled (the exact first hit)"""
    from common import grazing_rays
    w, h = SHAPE
    camera = checker.camera_rays(cam, w, h)
    g = grazing_rays(spheres, 128, seed=seed)
    graze = make_rays(g[:, 0:3], g[:, 3:6], _seeds(len(g), 7))
    doubled = camera[3::6][:64].copy()
    doubled[:, 4:7] *= f32(2)
    return np.ascontiguousarray(np.concatenate([camera, graze, doubled]))


def rays_of_case(checker, name, oracle):
    s, m, cam, _ = scene_case(name, oracle)
    return planted_rays(s) if cam is None else scene_rays(checker, s, cam)


SWEEP_COUNTS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257)
SWEEP_CAMERA = dict(look_from=(30.0, 12.0, 28.0), look_at=(0.0, 0.0, 0.0), vfov=50.0, aperture=0.05, focus_dist=40.0)


def sweep_scene(n):
    from toypathtracer_amd.scenes import cloud_scene
    return cloud_scene(n, lights=min(n, 4))


# the scenes the CPU half also runs through the host emulation: one per scene_kinds family, lights 0 / 17 / 46, grouped ones
EMU_SCENES = ("kind:type_-1", "kind:all_glass", "kind:negated_radius_glass", "kind:zero_radius", "kind:ground_2^49", "kind:aperture_5",
              "kind:grouped_zero_radii", "kind:flat_zero_radii", "kind:kitchen_sink", "lights:0", "lights:17", "lights:46", "lights_grouped",
              "spheres_%d" % MANY)


# ---------------------------------------------------------------- the child process: everything above through the host emulation
def _emu_main(root):
    import tempfile
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    from toypathtracer_amd import api as tpt
    import rays_lib
    import scene_kinds_lib
    from oracle_lib import Oracle
    from rays_lib import RaysChecker
    sys.stdout.reconfigure(line_buffering=True)  # (a run that has to be killed still says how far it came)
    checker = RaysChecker(tempfile.mkdtemp(prefix="rays_kinds_"))
    oracle = Oracle.get()
    tpt.load_library()
    tpt.InitializeTest()
    ptr = lambda x: None if x is None else x.ctypes.data
    calls = [0]

    def run(rays):
        """-> (counter gain, radiance, hits); the outputs start as GUARD, with a guard row before and after"""
        n = len(rays)
        rad = np.full((n + 2, 4), GUARD, np.uint32).view(f32)
        hit = np.full((n + 2, 8), GUARD, np.uint32).view(f32)
        cnt = np.array([5, 1000, 5], np.uint64)
        before = rays.tobytes()
        tpt.trace_rays_device(n, ptr(rays), ptr(rad) + 16, ptr(hit) + 32, ptr(cnt) + 8)
        tpt.synchronize()
        assert rays.tobytes() == before, "the call wrote its input"
        for g in (rad, hit):
            assert (g.view(np.uint32)[[0, -1]] == GUARD).all(), "a guard row was written"
        assert cnt[0] == 5 and cnt[2] == 5
        calls[0] += 1
        return int(cnt[1]) - 1000, rad[1:-1], hit[1:-1]

    def variants():
        for hs in (0, 1):
            for fold in (0, 1):
                tpt.set_kernel_variant(hs, 3, -1)
                tpt.set_fold_mode(fold)
                yield hs, fold
        tpt.set_kernel_variant(0, 3, -1)
        tpt.set_fold_mode(0)

    for scene in ("default", "grouped"):
        s, m = rays_lib.SCENES[scene]()
        tpt.set_scene(s, m) if scene != "default" else tpt.set_scene(None, None)
        tpt.UpdateTest(0.0, 0, 16, 8, 0)
        assert (tpt.scene_info()["groups"] > 0) == (scene == "grouped")
        cam = rays_lib.scene_camera(scene, 40, 25)
        n_lights = int((m["emissive"] > 0).any(axis=1).sum())
        seam, _ = length_seam(checker, s, m)
        rng_rays, _ = length_range(checker, s, m, cam)
        seeds = seed_words(checker, cam)
        out_rays, bad = outside_domain(checker, s, m, cam)
        good = np.ascontiguousarray(out_rays[~bad])
        short, short_bad = np.ascontiguousarray(out_rays[:OUTSIDE_SHORT]), bad[:OUTSIDE_SHORT]
        for hs, fold in variants():
            what = "%s hs=%d fold=%d" % (scene, hs, fold)
            equal_bits(run(seam), checker.trace(s, m, seam, fold=fold), what + " length_seam")
            plain = equal_bits_or_nan(run(rng_rays), checker.trace(s, m, rng_rays, fold=fold), what + " length_range")
            print("length_range: %s: plain byte equality %s" % (what, "held" if plain else "did not hold"))
            print("seed_words: %s: begins (a state of 0 would never leave a rejection loop)" % what)
            got = run(seeds)
            equal_bits(got, checker.trace(s, m, seeds, fold=fold), what + " seed_words")
            assert got[1][:SEED_RAYS].tobytes() == got[1][SEED_RAYS:2 * SEED_RAYS].tobytes(), "seed 0 is not seed 1"
            r0 = tpt.ray_counter_read()
            own_outputs_only(run(out_rays), bad, checker.trace(s, m, good, fold=fold), n_lights, len(s), what + " outside_domain")
            own_outputs_only(run(short), short_bad, checker.trace(s, m, np.ascontiguousarray(short[~short_bad]), fold=fold), n_lights, len(s),
                             what + " outside_domain, the first 1000")
            equal_bits(run(good), checker.trace(s, m, good, fold=fold), what + " the good rays afterwards")
            assert tpt.ray_counter_read() == r0, "the context's ray counter moved"
        print("families: %s: equal" % scene)
    for name in EMU_SCENES:
        s, m, cam, grouped = scene_case(name, oracle)
        tpt.set_scene(s, m)
        tpt.UpdateTest(0.0, 0, 16, 8, 0)
        assert grouped is None or (tpt.scene_info()["groups"] > 0) == grouped, (name, tpt.scene_info())
        rays = rays_of_case(checker, name, oracle)
        for hs, fold in variants():
            want = checker.trace(s, m, rays, fold=fold)
            assert wholly_finite(want) == (name not in NONFINITE_SCENES), name
            if name not in NONFINITE_SCENES:
                equal_bits(run(rays), want, "%s hs=%d fold=%d" % (name, hs, fold))
            else:
                plain = equal_bits_or_nan(run(rays), want, "%s hs=%d fold=%d" % (name, hs, fold))
                print("scene %s hs=%d fold=%d: %d NaN words, plain byte equality %s" % (name, hs, fold, nan_words(want)[0], "held" if plain else "did not hold"))
        for ls, mitsuba in ((False, False), (True, True)):
            tpt.set_config(ls, 0.9, mitsuba)
            want = checker.trace(s, m, rays, light_sampling=ls, mitsuba_compare=mitsuba)
            (equal_bits_or_nan if name in NONFINITE_SCENES else equal_bits)(run(rays), want, "%s ls=%d mitsuba=%d" % (name, ls, mitsuba))
        tpt.set_config(True, 0.9, False)
        print("scene: %s: equal" % name)
    cam = scene_kinds_lib.oracle_camera(oracle, SWEEP_CAMERA, *SHAPE)
    for n in SWEEP_COUNTS:
        s, m = sweep_scene(n)
        tpt.set_scene(s, m)
        tpt.UpdateTest(0.0, 0, 16, 8, 0)
        assert (tpt.scene_info()["groups"] > 0) == (n >= 256), (n, tpt.scene_info())
        rays = scene_rays(checker, s, cam)
        equal_bits(run(rays), checker.trace(s, m, rays), "%d spheres" % n)
    print("sweep: equal")
    tpt.set_scene(None, None)
    tpt.ShutdownTest()
    print("calls: %d" % calls[0])
    print("ok")


if __name__ == "__main__":
    _emu_main(sys.argv[1])
