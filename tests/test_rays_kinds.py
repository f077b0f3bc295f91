"""tptTraceRaysDevice across ray lengths, seed words, records outside the domain and scenes, WITHOUT A GPU (tests/rays_kinds_lib.py):
that every ray family is what its description says, asserted on the checker alone (tests/rays_checker.c) -- a family that is not is a
bug of the tests, not a skip --; that every scene case has a finite reference or is listed as not having one, and hits with a fifth of
its rays; and every family and a subset of the scenes through the host emulation of the call (tests/hostemu_rays.cpp: the product's own
laneBeginRay, rayDirFitsFilter, hitSpheres, rayHitRecord and lanePost), both HitSpheres variants and both folds, light sampling off and
the mitsuba switch on, under the comparators the GPU tests use.  A defect of the lane logic shows here before any device run."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rays_kinds_lib as lib
import rays_lib
from oracle_lib import ROOT
from rays_lib import RaysChecker


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return RaysChecker(tmp_path_factory.mktemp("rays_kinds_checker"))


def scene_of(name):
    s, m = rays_lib.SCENES[name]()
    return s, m, rays_lib.scene_camera(name, 40, 25)


# ---------------------------------------------------------------- the families are what they say
@pytest.mark.parametrize("scene", ["default", "grouped"])
def test_length_seam_is_on_the_seam_and_grazing(checker, scene):
    s, m, _ = scene_of(scene)
    rays, classes = lib.length_seam(checker, s, m)
    assert len(rays) <= 24 * 16 + 192
    dd = lib.dd_of(rays[:, 4:7])
    lo, hi = np.float32(0.99999), np.float32(1.00001)
    fits = (dd >= lo) & (dd <= hi)  # rayDirFitsFilter, restated
    for name, target in dict(lib.SEAM_CLASSES, **lib.BEYOND).items():
        assert (dd[classes[name]] == target).all(), name
        assert fits[classes[name]].all() == (name in ("lo", "lo+1", "one", "hi-1", "hi")) and fits[classes[name]].any() == fits[classes[name]].all()
    census = lib.seam_census(checker, s, m, rays, classes)
    print(scene, census)
    for name, (n, grazing_hits, misses) in census.items():
        assert n >= 32 and (name in lib.BEYOND or (grazing_hits >= 8 and misses >= 8)), (name, n, grazing_hits, misses)
    _, _, hits = checker.trace(s, m, rays, radiance=False)
    for name in lib.BEYOND:
        assert (hits[classes[name], 7].view(np.int32) >= 0).sum() >= 8, name
    assert lib.wholly_finite(checker.trace(s, m, rays)), "length_seam drifted into non-finite outputs: equal_bits is no fair demand"
    assert lib.wholly_finite(checker.trace(s, m, rays, fold=rays_lib.FOLD_FORWARD))


@pytest.mark.parametrize("scene", ["default", "grouped"])
def test_length_range_crosses_both_limits(checker, scene):
    s, m, cam = scene_of(scene)
    rays, parts = lib.length_range(checker, s, m, cam)
    assert len(rays) <= 24 * 16 + 192
    census = lib.range_census(s, rays)
    for e in lib.RANGE_SCALES:
        sl = parts["scale_2^%d" % e]
        got = {k: int(v[sl].sum()) for k, v in census.items()}
        print(scene, "2^%d" % e, got)
        for k, n in got.items():
            assert (n >= 8) if k in lib.RANGE_CLASSES[e] else (n == 0), (e, got)
    d = rays[parts["zero_and_denormal_components"], 4:7]
    tiny = np.float32(1.1754944e-38)
    assert ((d == 0) & ~np.signbit(d)).any() and ((d == 0) & np.signbit(d)).any() and ((d != 0) & (np.abs(d) < tiny)).any()
    sl = parts["near_root_is_min_t"]
    assert sl.stop > sl.start, "no ray whose near root is kMinT was found"
    want = checker.trace(s, m, rays)
    ids = want[2][sl, 7].view(np.int32)
    _, near, taken = lib.sphere_roots(s, rays[sl], ids)
    assert (ids >= 0).all() and (near == lib.K_MIN_T).all() and (want[2][sl, 3] == taken).all()  # (the far root of the same sphere)
    words, finite = lib.nan_words(want)
    print(scene, "length_range: %d NaN words in the reference, %d of %d rays wholly finite" % (words, finite, len(rays)))
    assert 2 * finite >= len(rays)
    assert (want[1][:, 3] >= 1).all()


def test_seed_words_are_the_bytes_built(checker):
    s, m, cam = scene_of("default")
    rays = lib.seed_words(checker, cam)
    assert rays.view(np.uint32)[:, 3].reshape(len(lib.SEED_WORDS), -1).T.tolist() == [list(lib.SEED_WORDS)] * lib.SEED_RAYS
    assert np.ascontiguousarray(rays).tobytes() == rays.tobytes() and rays[:, 4:7].tobytes() == np.tile(rays[:lib.SEED_RAYS, 4:7], (12, 1)).tobytes()
    want = checker.trace(s, m, rays)
    assert lib.wholly_finite(want)
    blocks = want[1].reshape(len(lib.SEED_WORDS), -1, 4)
    assert blocks[0].tobytes() == blocks[1].tobytes() == blocks[10].tobytes()  # 0 counts as 1; SEED_WORDS[10] is 1 again
    assert len({b.tobytes() for b in blocks}) == len(lib.SEED_WORDS) - 2, "two seed words give the same paths: the rays do not show the seed"


@pytest.mark.parametrize("scene", ["default", "grouped"])
def test_outside_domain_leaves_the_good_rays_alone_in_the_reference(checker, scene):
    s, m, cam = scene_of(scene)
    rays, bad = lib.outside_domain(checker, s, m, cam)
    assert len(rays) == 1024 and bad[[0, 63, 768, 960, 999, 1023]].all() and bad[128:192].all() and bad[256:512:4].all() and bad.sum() == 134
    good = np.ascontiguousarray(rays[~bad])
    alone, mixed = checker.trace(s, m, good), checker.trace(s, m, rays)
    assert lib.wholly_finite(alone)
    assert mixed[1][~bad].tobytes() == alone[1].tobytes() and mixed[2][~bad].tobytes() == alone[2].tobytes()
    n_lights = int((m["emissive"] > 0).any(axis=1).sum())
    lib.own_outputs_only((mixed[0], mixed[1], mixed[2]), bad, alone, n_lights, len(s), scene)  # (the reference itself keeps to it)
    print(scene, "outside_domain: the bad rays' k in the reference:", sorted(set(mixed[1][bad, 3].tolist())))


# ---------------------------------------------------------------- the scene cases
def test_every_scene_case_has_a_fair_reference(checker, oracle):
    not_finite = []
    for name in lib.scene_names():
        s, m, cam, grouped = lib.scene_case(name, oracle)
        rays = lib.rays_of_case(checker, name, oracle)
        assert len(rays) <= 24 * 16 + 192 and np.isfinite(rays[:, [0, 1, 2, 4, 5, 6]]).all(), name
        want = checker.trace(s, m, rays)
        rate = float((want[2][:, 7].view(np.int32) >= 0).mean())
        assert rate >= 0.2 or name in lib.SEES_SKY, (name, rate)
        finite = [lib.wholly_finite(want)] + [lib.wholly_finite(checker.trace(s, m, rays, **kw)) for kw in (
            dict(fold=rays_lib.FOLD_FORWARD), dict(light_sampling=False), dict(mitsuba_compare=True))]
        assert all(finite) or not any(finite), (name, finite)
        if not finite[0]:
            not_finite.append(name)
            print("%s: %d NaN words, %d of %d rays wholly finite" % ((name,) + lib.nan_words(want) + (len(rays),)))
    assert tuple(not_finite) == lib.NONFINITE_SCENES
    ids = lib.planted_rays(lib.scene_case("spheres_%d" % lib.MANY, oracle)[0])
    s, m, _, _ = lib.scene_case("spheres_%d" % lib.MANY, oracle)
    hit = set(checker.trace(s, m, ids, radiance=False)[2][:, 7].view(np.int32).tolist())
    import seams_lib
    assert set(seams_lib.PLANTED) <= hit, "a planted id is not hit: %s" % sorted(set(seams_lib.PLANTED) - hit)
    assert {i for i in seams_lib.PLANTED if i >= 32768} and {i for i in seams_lib.PLANTED if i >= 65408}


def test_the_sweep_scenes_have_a_fair_reference(checker, oracle):
    import scene_kinds_lib
    cam = scene_kinds_lib.oracle_camera(oracle, lib.SWEEP_CAMERA, *lib.SHAPE)
    for n in lib.SWEEP_COUNTS:
        s, m = lib.sweep_scene(n)
        want = checker.trace(s, m, lib.scene_rays(checker, s, cam))
        assert len(s) == n and lib.wholly_finite(want) and (want[2][:, 7].view(np.int32) >= 0).mean() >= 0.2, n


# ---------------------------------------------------------------- the comparators themselves
def test_the_comparators_tell():
    rad, hit = np.ones((4, 4), np.float32), np.ones((4, 8), np.float32)
    want = (4, rad, hit)
    lib.equal_bits((4, rad.copy(), hit.copy()), want, "same")
    other = rad.copy()
    other.view(np.uint32)[2, 1] ^= 1
    for cmp in (lib.equal_bits, lib.equal_bits_or_nan):
        with pytest.raises(AssertionError):
            cmp((4, other, hit), want, "one bit")
        with pytest.raises(AssertionError):
            cmp((5, rad, hit), want, "the counter")
    nan_x86, nan_gpu = rad.copy(), rad.copy()
    nan_x86.view(np.uint32)[1, 0], nan_gpu.view(np.uint32)[1, 0] = 0xFFC00000, 0x7FC00000
    with pytest.raises(AssertionError):
        lib.equal_bits((4, nan_gpu, hit), (4, nan_x86, hit), "NaN patterns")
    assert lib.equal_bits_or_nan((4, nan_gpu, hit), (4, nan_x86, hit), "NaN patterns") is False
    assert lib.equal_bits_or_nan((4, nan_x86, hit), (4, nan_x86, hit), "NaN patterns") is True
    with pytest.raises(AssertionError):
        lib.equal_bits_or_nan((4, rad, hit), (4, nan_x86, hit), "a number for a NaN")
    with pytest.raises(AssertionError):
        lib.equal_bits_or_nan((4, nan_gpu, hit), (4, rad, hit), "a NaN for a number")
    k_x86, k_gpu = rad.copy(), rad.copy()
    k_x86.view(np.uint32)[1, 3], k_gpu.view(np.uint32)[1, 3] = 0xFFC00000, 0x7FC00000
    with pytest.raises(AssertionError):
        lib.equal_bits_or_nan((4, k_gpu, hit), (4, k_x86, hit), "the k word is compared as bits")
    # own_outputs_only: an unwritten record, a k out of range, a counter that is not the written sum
    bad = np.array([False, True, False, False])
    g_rad, g_hit = rad.copy(), hit.copy()
    g_rad[1], g_hit[1] = (np.nan, np.nan, np.nan, 1.0), 0
    g_hit.view(np.uint32)[1, 7] = 0xFFFFFFFF
    good = (3, rad[~bad], hit[~bad])
    lib.own_outputs_only((4, g_rad, g_hit), bad, good, 2, 46, "fine")
    for change in ("guard", "k", "id", "counter", "good"):
        r2, h2, gain = g_rad.copy(), g_hit.copy(), 4
        if change == "guard":
            h2.view(np.uint32)[1, 2] = lib.GUARD
        elif change == "k":
            r2[1, 3] = 34.0
            gain = 37
        elif change == "id":
            h2.view(np.uint32)[1, 7] = 46
        elif change == "counter":
            gain = 5
        else:
            r2[2, 0] = 2.0
        with pytest.raises(AssertionError):
            lib.own_outputs_only((gain, r2, h2), bad, good, 2, 46, change)


# ---------------------------------------------------------------- through the host emulation
@pytest.fixture(scope="module")
def emulation():
    """tests/rays_kinds_lib.py as a child process on the host runtime built against tests/hostemu, as tests/test_rays_abi.py builds it"""
    from test_host_logic import build
    path = build("libtpt_hostemu_rays.so", [os.path.join(ROOT, "tests", "hostemu_rays.cpp")])
    env = dict(os.environ, TPT_LIB=path, HOSTEMU_POLICY="eager")
    env.pop("TPT_LIB_DIR", None)
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "rays_kinds_lib.py"), ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    try:
        out = p.communicate(timeout=300)[0].decode()  # (half a minute when all is well)
    except subprocess.TimeoutExpired:  # a path that never ends, e.g. an xorshift state of 0 in a rejection loop
        p.kill()
        return -1, "the child did not end within 300 s:\n" + p.communicate()[0].decode()
    return p.returncode, out


def test_the_families_through_the_lane_logic(emulation):
    """length_seam, length_range, seed_words and outside_domain on the built-in scene and on the grouped one, both HitSpheres variants
    and both folds, each under its comparator.

    outside_domain runs here before it runs on a device.  Why a record with NaN, Inf or zero components ends, loop by loop, from
    tpt_trace.h and tpt_kernels.hip -- no loop's trip count depends on a float:
      - the candidate-mask walks (hitSpheresTwoPhase, hitSpheresCandidates: `while (cand)`; the member mask `while (mm)`): every trip
        clears the bit it took from an integer mask of at most 64 (32) bits, whatever the filter's NaN put into it; the chunk loop over
        nPairs and the simple loop over nSpheres are counted;
      - the grouped traversal's `for (;;)`: each trip clears one bit of cm0 .. cm3 and leaves when all four are zero: at most 256 trips
        per block of 128 group pairs, the blocks counted by nGroupPairs;
      - the slot queue: sqPush is called with q.n < 8 only (it is drained at 8), sqDrain pops until the integer q.n is 0;
      - the light loop: L.j only grows, one light per step, and the skip-self `while` is bounded by nLights; a shadow ray's outcome
        decides what is added, never whether j advances;
      - the rejection loops of the random draws (randomInUnitSphere, randomInUnitDisk): they read the lane's xorshift state alone, an
        integer the ray's floats never enter, which is not 0 (laneBeginRay) and so never becomes 0; randomUnitVector has no loop;
      - the depth limit: L.depth is an integer that every bounce increments, and a hit at depth kMaxDepth finishes; a miss finishes at
        once.  So a path is at most kMaxDepth + 1 main rays, each followed by at most nLights shadow rays -- own_outputs_only's bound
        on k.
    A NaN in a comparison makes it false: testSphere's `discr > 0`, `t > tMin && t < hitT` reject, so a NaN ray misses and ends in
    sky(NaN) after one HitWorld; a zero direction inside a sphere hits it (nb = 0, discr = -c > 0) and goes on with NaN directions.
    What a wave's lanes share -- the refill ballots, the chunk counter, the LDS stack (a column per lane), the wave's ray sum -- is
    indexed by lane and integer state, none by a ray's floats."""
    code, out = emulation
    assert code == 0 and out.rstrip().endswith("ok"), out[-6000:]
    for scene in ("default", "grouped"):
        assert "families: %s: equal" % scene in out, out[-6000:]
    print("\n".join(line for line in out.splitlines() if line.startswith("length_range")))


def test_a_scene_subset_through_the_lane_logic(emulation):
    """at least one scene per scene_kinds family, lights 0 / 17 / 46 and grouped scenes: HitSpheres variants, folds, light sampling off,
    the mitsuba switch"""
    import scene_kinds_lib
    code, out = emulation
    assert code == 0, out[-6000:]
    for name in lib.EMU_SCENES:
        assert "scene: %s: equal" % name in out, out[-6000:]
    assert "sweep: equal" in out  # (the sphere counts at the pair, chunk and grouping seams: grouped exactly from 256 on)
    kinds = {scene_kinds_lib.FAMILY_OF[n[5:]] for n in lib.EMU_SCENES if n.startswith("kind:")}
    assert kinds == set(scene_kinds_lib.FAMILIES) and {"lights:0", "lights:17", "lights:46"} <= set(lib.EMU_SCENES)
    print("\n".join(line for line in out.splitlines() if line.startswith("scene ") and "NaN" in line))
