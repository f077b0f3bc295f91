"""tptDrawDeviceLens across bases, spans, origins, sizes, frames, sample counts and scenes, WITHOUT A GPU (tests/lens_kinds_lib.py): that
every case is what its name says, asserted on the checker alone (tests/lens_checker.c) -- which regime the fisheye's r * r is in, how many
pixels hit, that a basis lies inside the accepted interval and clear of the orthonormal one; a case that is not is a bug of the tests,
not a skip --; that every case's reference is finite, so that byte equality is a fair demand; and every case through the host runtime
on the emulated device (tests/hostemu_lens.cpp: the product's own mapItem, laneLens, hitSpheres and lanePost), the span cases in a
process of their own, so that their loops are known to end before a GPU sees them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lens_kinds_lib as lib
from lens_lib import EQUIRECT, FISHEYE, KINDS, ORTHO, LensChecker, make_lens, noise_tile, to_api
from oracle_lib import ROOT

f32 = np.float32


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return LensChecker(tmp_path_factory.mktemp("lens_kinds_checker"))


def named(section, prefix=""):
    return {c.name: c for c in lib.cases(section) if c.name.startswith(prefix)}


def directions(checker, c):
    return checker.rays(c.lens, c.w, c.h, c.frame)[:, 4:7].reshape(c.h, c.w, 3)


def test_the_restated_first_samples_are_the_checkers(checker):
    """lens_kinds_lib.first_uv (the seed and the two draws in numpy) gives the checker's own rays, also for a frame whose seed wraps"""
    lens = make_lens(FISHEYE)
    for frame in (0, lib.FRAMES["wrapping"], lib.FRAMES["2^31-2"]):
        u, v = lib.first_uv(lib.W, lib.H, frame)
        assert u.min() >= 0 and u.max() < 1 and v.min() >= 0 and v.max() < 1
        want = checker.rays(lens, lib.W, lib.H, frame)[:, [0, 1, 2, 4, 5, 6]]
        got = checker.ray_grid(lens, np.stack([u.ravel(), v.ravel()], 1))
        assert got.tobytes() == want.tobytes(), frame


def test_every_case_is_accepted_and_has_a_finite_reference(checker):
    """the binding's own statement of the rules passes every lens, and no reference has a NaN or an infinity in it: bytes can be compared"""
    from toypathtracer_amd import api
    n = 0
    for section in lib.SECTIONS:
        for c in lib.cases(section):
            api._check_lens(to_api(c.lens))
            assert 1 <= c.w <= 8192 and 1 <= c.h <= 8192 and 0 <= c.frame < 2 ** 31 - 1 and 1 <= c.spp <= 65536, c.name
            rays, tile = lib.reference(checker, c)
            assert np.isfinite(tile).all() and rays >= c.w * c.h * c.spp, c.name
            n += 1
    assert n == 12 + (2 * len(lib.SCALES) + len(lib.EQUIRECT_TINY) + len(lib.GROUND_SCALES) + 2 + 1 + 2 + 3 + 1) + (3 * 4 + 5 + 3 + 2) + 2 + 6 + 8 + (2 + 12 + 1 + 2)


# ---------------------------------------------------------------- 1. bases
@pytest.mark.parametrize("name", sorted(named("bases")))
def test_a_basis_lies_inside_the_accepted_interval(name):
    """in float64 on the binary32 values the call gets, with lensFault's bounds; a skewed basis is clear of the orthonormal one"""
    c = named("bases")[name]
    len2, dots = lib.gram(c.lens)
    print(name, len2, dots)
    assert all(lib.LEN2_BOUNDS[0] <= v <= lib.LEN2_BOUNDS[1] for v in len2), len2
    assert all(lib.DOT_BOUNDS[0] <= v <= lib.DOT_BOUNDS[1] for v in dots), dots
    vecs = np.array([c.lens.right[:], c.lens.up[:], c.lens.forward[:]], np.float64)
    if "skew" in name:
        sign = 1.0 if name.endswith("+") else -1.0
        assert all(abs(v - 1) > lib.CLEAR for v in len2) and all(sign * v > lib.CLEAR for v in dots)
        assert np.allclose(len2, lib.SKEW_LEN2, atol=1e-6, rtol=0) and np.allclose(dots, sign * lib.SKEW_DOT, atol=1e-6, rtol=0)
    else:
        assert np.allclose(len2, 1, atol=1e-6) and np.allclose(dots, 0, atol=1e-6)
        handed = float(np.dot(np.cross(vecs[2], vecs[1]), vecs[0]))  # make_lens: right = forward x up
        assert (handed < -0.99) if "left-handed" in name else (handed > 0.99), handed
    if "rotated" in name:
        assert (vecs != 0).all(), vecs


@pytest.mark.parametrize("name", sorted(named("bases", "basis-")))
def test_a_changed_basis_changes_the_directions_and_normalize_still_normalises(checker, name):
    c = named("bases")[name]
    plain = lib.case("plain", make_lens(c.lens.kind))
    d, d0 = directions(checker, c), directions(checker, plain)
    if "skew" in name or "rotated" in name:
        assert (d != d0).any(axis=2).all(), "a pixel's direction is the orthonormal lens's"
    else:  # right negated: an ORTHO ray keeps its direction and starts elsewhere
        o, o0 = (checker.rays(x.lens, x.w, x.h)[:, 0:3] for x in (c, plain))
        assert (d != d0).any(axis=2).all() if c.lens.kind != ORTHO else ((d == d0).all() and (o != o0).any(axis=1).all())
    dd = (d.astype(np.float64) ** 2).sum(axis=2)
    assert np.abs(dd - 1).max() <= 4 * 2.0 ** -23, np.abs(dd - 1).max()  # within 4 ulp of 1
    if "skew" in name:  # as given, |q| is not 1: normalize does real work
        q = np.array(c.lens.forward[:], np.float64)
        assert abs(float(q @ q) - 1) > lib.CLEAR


# ---------------------------------------------------------------- 2. spans
def test_the_fisheye_scales_cover_normal_subnormal_and_zero(checker):
    seen = set()
    for e in lib.SCALES:
        c = named("spans")["span-fisheye-2^-%d" % e]
        a, b = lib.plane_coords(c.lens, c.w, c.h)
        rr = a * a + b * b
        got = lib.regimes(rr)
        print(e, sorted(got), int((rr > 0).sum()))
        assert got == lib.FISHEYE_RR[e], (e, got)
        seen |= got
        d = directions(checker, c)
        assert np.isfinite(d).all()
        centre = checker.ray(c.lens, 0.5, 0.5)[3:6]  # (r = 0: normalize(forward))
        forward = np.array(c.lens.forward[:], f32)
        moved = (d != forward).any(axis=2) & (d != centre).any(axis=2)
        assert moved[rr > 0].all(), (e, "a direction with r > 0 is forward's")
        assert (d[rr == 0] == centre).all()
    assert seen == {"normal", "subnormal", "zero"}
    last = lib.LAST_BEFORE_ZERO
    assert last in lib.SCALES and last + 1 in lib.SCALES and "zero" not in lib.FISHEYE_RR[last] - {"zero"}
    assert lib.FISHEYE_RR[last] - {"zero"} and lib.FISHEYE_RR[last + 1] == {"zero"}, "the last scale before zero is not among the cases"


@pytest.mark.parametrize("e", lib.GROUND_SCALES)
def test_over_the_huge_ground_a_subnormal_rr_shows_in_the_image(checker, e):
    """r * r is subnormal in every pixel or nearly, and the image is not the one of r = 0 (what a kernel that flushed r * r would draw):
    pixels differ, while on the built-in scene the same pair of lenses draws the same bytes"""
    (c,) = [c for c in lib.cases("spans") if c.name == "span-fisheye-2^-%d-over-the-2^60-ground" % e]
    a, b = lib.plane_coords(c.lens, c.w, c.h)
    rr = a * a + b * b
    assert "subnormal" in lib.regimes(rr) and "normal" not in lib.regimes(rr) and 2 * (rr > 0).sum() > rr.size
    assert tuple(c.lens.forward[:]) == (0.0, 0.0, -1.0) and tuple(c.lens.up[:]) == (0.0, 1.0, 0.0)
    s, _ = lib.scene(c.scene)
    assert s["radius"][0] == 2.0 ** 60
    flushed = c._replace(lens=lib.copy_lens(c.lens, sx=2.0 ** -80, sy=2.0 ** -80))  # r * r = 0 everywhere
    (rays, tile), (rays0, tile0) = lib.reference(checker, c), lib.reference(checker, flushed)
    differ = (tile != tile0).any(axis=2)
    print(e, "%d of %d pixels differ from the r = 0 image" % (differ.sum(), differ.size))
    assert np.isfinite(tile).all() and differ.sum() >= 8  # (where a path meets the ground: most primary rays end on a small sphere)
    plain, plain0 = (x._replace(scene="default") for x in (c, flushed))
    assert lib.reference(checker, plain)[1].tobytes() == lib.reference(checker, plain0)[1].tobytes()


@pytest.mark.parametrize("name", sorted(lib.MAX_ANGLES))
def test_the_fisheye_with_a_vanishing_max_angle(checker, name):
    """r is ordinary and r * maxAngle is at the bottom of the type: 2^-126 r is subnormal below r = 1, 2^-149 r rounds to zero below
    r = 1 / 2 and to the smallest subnormal above"""
    c = named("spans")["span-fisheye-max-angle-" + name]
    a, b = lib.plane_coords(c.lens, c.w, c.h)
    r = np.sqrt(a * a + b * b)
    angle = r * f32(c.lens.maxAngle)
    got = lib.regimes(angle)
    print(name, sorted(got))
    assert got == ({"normal", "subnormal"} if name == "2^-126" else {"subnormal", "zero"}) and (r > 0).all()
    d = directions(checker, c)
    assert np.isfinite(d).all()
    # The direction leaves forward's exactly where a k does not underflow: make_lens's default basis has right = (1, 0, 0) and
    # forward.x = up.x = 0, so q.x = a k, while in y and z forward absorbs what up * (b k) adds.  With maxAngle = 2^-149 that is not
    # every pixel with r > 0: k = sin(angle) / r is one or two units of 2^-149, and a k rounds to zero where |a| k is below half a unit.
    assert tuple(c.lens.right[:]) == (1.0, 0.0, 0.0) and c.lens.forward[0] == 0 and c.lens.up[0] == 0
    k = angle / r  # (sin x = x in binary32 down here)
    moved = (d != checker.ray(c.lens, 0.5, 0.5)[3:6]).any(axis=2)
    print(name, "%d of %d directions leave forward's" % (moved.sum(), moved.size))
    assert (moved == (a * k != 0)).all() and moved.any()
    if name == "2^-126":
        assert moved.all()


def test_the_equirect_scales_reach_tiny_and_subnormal_arguments_of_both_signs(checker):
    seen = set()
    for e in lib.SCALES + lib.EQUIRECT_TINY:
        c = named("spans")["span-equirect-2^-%d" % e]
        a, b = lib.plane_coords(c.lens, c.w, c.h)
        for x in (a, b):
            assert np.signbit(x).any() and not np.signbit(x).all()
            got = lib.regimes(np.abs(x))
            want = {126: {"subnormal"}, 140: {"subnormal", "zero"}, 149: {"zero"}}  # (2^-140: |u - 0.5| < 2^-10 rounds to a zero)
            assert got == want.get(e, {"normal"}), (e, got)
            seen |= got
        s, co = checker.sincos(np.concatenate([a.ravel(), b.ravel()]))
        assert (s == np.concatenate([a.ravel(), b.ravel()])).all() if e >= 30 else np.isfinite(s).all()  # (sin x = x from 2^-12 down)
        assert np.isfinite(directions(checker, c)).all()
    assert seen == {"normal", "subnormal", "zero"}


def test_the_pole_rows_of_the_widest_panorama_keep_a_cosine(checker):
    c = named("spans")["span-equirect-below-2pi-by-pi"]
    assert c.spp == 1 and c.lens.sx == lib.below(6.2831855) < np.float32(6.2831855) and c.lens.sy == lib.below(3.1415927) < np.float32(3.1415927)
    _, b = lib.plane_coords(c.lens, c.w, c.h)
    poles = b[[0, -1]]
    assert (poles[0] < -1.4).all() and (poles[1] > 1.4).all()
    cb = checker.sincos(poles.ravel())[1]
    print("cb in the pole rows: %g .. %g" % (cb.min(), cb.max()))
    assert (cb != 0).all() and (cb > 0).all()


@pytest.mark.parametrize("name", sorted(lib.ORTHO_TINY))
def test_every_ray_of_a_vanishing_window_starts_at_the_origin(checker, name):
    c = named("spans")["span-ortho-" + name]
    a, b = lib.plane_coords(c.lens, c.w, c.h)
    assert lib.regimes(np.abs(np.concatenate([a, b]))) <= {"subnormal", "zero"} and (a != 0).any() == (name == "2^-126")
    rays = checker.rays(c.lens, c.w, c.h)
    assert (rays[:, 0:3] == np.array(c.lens.origin[:], f32)).all() and len({r.tobytes() for r in rays[:, 4:7]}) == 1


@pytest.mark.parametrize("name", sorted(lib.ORTHO_HUGE))
def test_a_huge_window_misses_everything(checker, name):
    """how many pixels must hit: lens_kinds_lib.ORTHO_HUGE_HITS, none -- every sample is one ray into the sky"""
    c = named("spans")["span-ortho-" + name]
    rays, tile = lib.reference(checker, c)
    hits = rays - c.w * c.h * c.spp  # (a sample that hits costs more than its first ray)
    assert lib.ORTHO_HUGE_HITS == 0 and hits == 0, (name, hits)
    o = checker.rays(c.lens, c.w, c.h)[:, 0:3]
    assert np.isfinite(o).all()  # (finite even at FLT_MAX: |a| <= sx / 2)
    assert (np.maximum(np.abs(o[:, 0]), np.abs(o[:, 1])) > 1000).all()  # every first sample starts far from the scene one way or the other


def test_the_overflowing_window_is_infinite_on_one_side_only(checker):
    c = named("spans")["span-ortho-overflow"]
    o = checker.rays(c.lens, c.w, c.h)[:, 0:3].reshape(c.h, c.w, 3)
    assert not np.isnan(o).any() and np.isfinite(o[..., 1:]).all()
    assert np.isfinite(o[:, :19, 0]).all() and (o[:, 23:, 0] == np.inf).all(), "finite on the left, +inf on the right"
    rays, tile = lib.reference(checker, c)
    assert np.isfinite(tile).all() and rays == c.w * c.h * c.spp  # one ray a sample


# ---------------------------------------------------------------- 3. origins
def test_far_origins_hit_or_miss_as_recorded(checker):
    got = {}
    for name in lib.ORIGIN_HITS:
        c = named("origins")[name]
        rays, tile = lib.reference(checker, c)
        got[name] = rays > c.w * c.h * c.spp
        assert np.isfinite(tile).all(), name
        assert c.lens.origin[2] == 2.0 ** int(name.rsplit("^", 1)[1])
    print(got)
    assert got == lib.ORIGIN_HITS
    assert set(got.values()) == {True, False}
    assert len(got) == 3 * len(lib.ORIGIN_NEAR) + len(lib.ORIGIN_FAR)
    with np.errstate(over="ignore"):  # oc . oc overflows inside HitSpheres from 2^64 on
        assert [bool(np.isinf(f32(2.0 ** e) * f32(2.0 ** e))) for e in lib.ORIGIN_FAR] == [False, False, True, True, True]


def test_origins_on_a_surface_and_at_a_centre(checker):
    centre, r = lib.glass_sphere()
    on, at = named("origins", "origin-"), 0
    for name, c in on.items():
        o = np.array(c.lens.origin[:], f32)
        if name.endswith("on-the-surface"):
            assert o[0] == centre[0] + r and (o[1:] == centre[1:]).all() and f32(o[0] - centre[0]) == r
            at += 1
        elif name.endswith("at-the-centre"):
            assert (o == centre).all() and c.lens.kind in (EQUIRECT, FISHEYE)
            at += 10
    assert at == 23


# ---------------------------------------------------------------- 4. sizes
def test_the_sizes_are_what_they_say():
    a, b = lib.cases("sizes")
    assert (a.w, a.h, b.w, b.h) == (8192, 8, 8, 8192) and a.spp == b.spp == 4 and a.lens.kind != b.lens.kind
    assert lib.items_of(8192, 8) == 1024 * 64 and f32(1) / f32(8192) == 2.0 ** -13
    # a whole MI355X at 4 workgroups per CU, and the emulated device of two CUs at 16
    assert lib.seam_sizes(256 * 4) == ((2041, 1017), (2025, 1009)) and lib.seam_sizes(32) == ((361, 177), (345, 169))
    for resident in (1, 2, 32, 1024, 2048, 4096):
        (w1, h1), (w0, h0) = lib.seam_sizes(resident)
        assert lib.items_of(w0, h0) // 256 < 8 * resident <= lib.items_of(w1, h1) // 256  # laneRefillChunks' own test


# ---------------------------------------------------------------- 5. frames and samples
def test_the_frames_are_what_they_say(checker):
    frame, k = lib.wrapping_frame()
    assert (frame * 26699) % 2 ** 32 == k <= 8 and frame * 26699 > 2 ** 32 and lib.FRAMES["wrapping"] == frame
    assert f32(lib.FRAMES["2^24+1"]) == 2.0 ** 24 and lib.FRAMES["2^24+1"] == 2 ** 24 + 1  # (float)frame drops the 1
    assert lib.FRAMES["2^31-2"] == 2 ** 31 - 2 and max(lib.FRAMES.values()) < 2 ** 31 - 1
    assert f32(2 ** 31 - 2) / f32(2 ** 31 - 1) == 1  # lerp is 1: the progressive draw leaves the tile as it was
    cases = named("frames")
    assert len(cases) == 6
    c = cases["frame-2^31-2-progressive-onto-noise"]
    assert lib.reference(checker, c)[1].tobytes() == noise_tile(c.w, c.h).tobytes()
    c = cases["frame-2^24+1-progressive-onto-noise"]
    assert (lib.reference(checker, c)[1][..., :3] != noise_tile(c.w, c.h)[..., :3]).any()
    seen = {cases[n].lens.kind for n in cases}
    assert len(seen) == 2


def test_the_sample_counts_are_what_they_say():
    cases = lib.cases("samples")
    assert [c.spp for c in cases] == list(lib.SAMPLES) + [65536] and lib.SAMPLES == (1, 2, 3, 64, 2047, 2048, 65536)
    assert all((c.w, c.h) == (8, 8) for c in cases[:-1]) and (cases[-1].w, cases[-1].h) == (1, 1)
    assert {c.lens.kind for c in cases} == set(KINDS.values())


# ---------------------------------------------------------------- 6. scenes
def test_the_scenes_are_what_they_say(checker):
    import lights_lib
    cases = named("scenes")
    for name in ("scene-shell-glass-equirect", "scene-shell-mirror-fisheye"):
        c = cases[name]
        s, m = lib.scene(c.scene)
        o = np.array(c.lens.origin[:], np.float64)
        assert len(s) == 47 and s["radius"][46] in (12, -12) and np.linalg.norm(o) < 11, name
        rays, _ = lib.reference(checker, c)
        assert rays >= 6 * c.w * c.h * c.spp, (name, rays)  # no path ends in the sky: they run deep
    for k in lib.LIGHTS:
        for switch, lds in lib.LDS_SWITCH.items():
            (c,) = [c for n, c in cases.items() if n.startswith("scene-%d-lights-%s-" % (k, switch))]
            assert len(lights_lib.light_ids(lib.scene(c.scene)[1])) == k and c.lds == lds
    s, m = lib.scene("lights_grouped")
    assert len(s) == 1000 and len(lights_lib.light_ids(m)) == 300
    assert {c.fold for c in cases.values()} == {0, 1}
    assert {c.scene for c in cases.values() if c.fold == 1} == {"kind:shell_glass", "lights:17"}


# ---------------------------------------------------------------- through the host runtime on the emulated device
def child(sections, cus=None):
    from test_host_logic import build
    path = build("libtpt_hostemu_lens.so", [os.path.join(ROOT, "tests", "hostemu_lens.cpp")])
    env = dict(os.environ, TPT_LIB=path, HOSTEMU_POLICY="eager")
    env.pop("TPT_LIB_DIR", None)
    if cus:
        env["HOSTEMU_CUS"] = str(cus)
    return subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "lens_kinds_lib.py"), ROOT] + sections, env=env, stdout=subprocess.PIPE,
                            stderr=subprocess.STDOUT)


def outcome(p, limit):
    try:
        out = p.communicate(timeout=limit)[0].decode()
        return p.returncode, out
    except subprocess.TimeoutExpired:  # a loop that does not end
        p.kill()
        return -1, "the child did not end within %d s:\n" % limit + p.communicate()[0].decode()


@pytest.fixture(scope="module")
def emulation():
    """tests/lens_kinds_lib.py as child processes on the host runtime built against tests/hostemu, as tests/test_lens_abi.py builds it:
    the spans alone, the other sections, and the tile / chunk seam on a device of two CUs"""
    jobs = {"spans": child(["spans"]), "rest": child([s for s in lib.SECTIONS if s != "spans"]), "seam": child(["seam"], cus=2)}
    out = {}
    for key, p in jobs.items():
        out[key] = outcome(p, 300)  # (a quarter of a minute when all is well)
    return out


def held(emulation, key, names):
    code, out = emulation[key]
    assert code == 0 and out.rstrip().endswith("ok"), out[-6000:]
    for name in names:
        assert "case: %s: equal" % name in out, (name, out[-6000:])


def test_the_spans_end_and_equal_the_checker_on_the_host_build(emulation):
    """every span case through the product's lensGetRayAt, hitSpheres and lanePost compiled for the host, before a GPU sees it: no trip
    count of the lane's loops depends on a float (tests/test_rays_kinds.py lists them), and here they are seen to end -- with r * r
    subnormal and zero, sin and cos at subnormal arguments, ray origins of +inf"""
    held(emulation, "spans", [c.name for c in lib.cases("spans")])


@pytest.mark.parametrize("section", [s for s in lib.SECTIONS if s != "spans"])
def test_a_section_through_the_emulated_runtime(emulation, section):
    held(emulation, "rest", [c.name for c in lib.cases(section)])


def test_both_sides_of_the_seam_through_the_emulated_runtime(emulation):
    """on a device of two CUs the seam lies at a few hundred pixels a side: the image past it is drawn in chunks of 256, the one before
    it in tiles, both byte for byte (tests/test_lens_abi.py pins the plans)"""
    code, out = emulation["seam"]
    assert code == 0 and out.rstrip().endswith("ok"), out[-6000:]
    lines = [ln for ln in out.splitlines() if ln.startswith("case: size-") and "begins" not in ln]
    assert len(lines) == 2 and "chunks-of-256: equal (chunks of 256)" in lines[0] and "tiles: equal (chunks of 64)" in lines[1], lines
