"""tptTraceRaysDevice on the GPU across ray lengths, seed words, records outside the domain and scenes (tests/rays_kinds_lib.py), against
its C statement (tests/rays_checker.c).  tests/test_gpu_rays.py holds the call on two scenes with finite rays of four lengths; the draw
kernels' sweeps of lights, materials, scale, degenerate spheres and packed fields never reach the ray mode's own device code.  Held here:

  - rayDirFitsFilter's switch between the exact first HitWorld and the filtered one, with grazing rays whose float32 |d|^2 IS each limit
    and each limit's neighbours, on a scene staged in LDS, on the same scene read from global memory and on a grouped scene;
  - kMinT and kMaxT reached through the direction's length (2^-23 .. 2^13), zero, negative-zero and denormal components, |d|^2 that
    underflows or overflows, a near root that is kMinT exactly;
  - the seed word as arbitrary bits: NaN patterns, infinities, the sign bit alone, 0;
  - records the header does not define (NaN, Inf, zero directions) among good rays of the same wave: they end, write their own records,
    count their own rays and touch nothing else (tests/test_rays_kinds.py argues loop by loop why they end, and runs them first);
  - the largest call: 16777216 rays, every index and the chunk arithmetic up to 2^24 - 1;
  - rayHitRecord and the per-ray count on every scene of tests/scene_kinds_lib.py, every light count and kind of tests/lights_lib.py, a
    grouped scene with 300 lights and the 65534-sphere scene of tests/seams_lib.py (ids at and above 32768 and 65408), and on the other
    HitSpheres variant, the forward fold, the LDS scene off, light sampling off and the mitsuba switch;
  - sphere counts around the pair, chunk and grouping seams.

tests/test_rays_kinds.py proves on the CPU that every family and scene is what is said here and that the lane logic gets them right."""
import time

import numpy as np
import pytest

import rays_kinds_lib as lib
import rays_lib
import scene_kinds_lib
from oracle_lib import FOLD_FORWARD, FOLD_RECURSIVE
from rays_lib import RaysChecker
from test_gpu_lights import restore
from test_gpu_rays import check, trace
from test_gpu_scene_kinds import ON_EVERY_VARIANT

pytestmark = pytest.mark.gpu

# how a family's scene is set up: the built-in scene staged in LDS, the same read from global memory, a grouped scene
CONFIGS = {"flat_lds": ("default", (0, 3, -1)), "flat_global": ("default", (0, 3, 0)), "grouped": ("grouped", (0, 3, -1))}
VARIANTS = {"simple_hit_spheres": dict(variant=(1, 3, -1)), "forward_fold": dict(fold=FOLD_FORWARD), "lds_scene_off": dict(variant=(0, 3, 0)),
            "no_light_sampling": dict(light_sampling=False), "mitsuba_compare": dict(mitsuba_compare=True)}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return RaysChecker(tmp_path_factory.mktemp("rays_kinds_checker"))


@pytest.fixture(scope="module")
def families(checker):
    """per scene: the scene, its light count, every family's rays and the checker's outputs for them; made once, left as they are"""
    out = {}
    for name in ("default", "grouped"):
        s, m = rays_lib.SCENES[name]()
        cam = rays_lib.scene_camera(name, 40, 25)
        f = dict(s=s, m=m, lights=int((m["emissive"] > 0).any(axis=1).sum()))
        f["length_seam"] = lib.length_seam(checker, s, m)[0]
        f["length_range"] = lib.length_range(checker, s, m, cam)[0]
        f["seed_words"] = lib.seed_words(checker, cam)
        f["outside_domain"], f["bad"] = lib.outside_domain(checker, s, m, cam)
        for fam in ("length_seam", "length_range", "seed_words"):
            f["want_" + fam] = checker.trace(s, m, f[fam])
        out[name] = f
    return out


def set_up(tpt, config):
    scene, variant = CONFIGS[config]
    if scene != "default":
        s, m = rays_lib.SCENES[scene]()
        tpt.set_scene(s, m)
    tpt.set_kernel_variant(*variant)
    tpt.UpdateTest(0.0, 0, 40, 25, 0)
    assert (tpt.scene_info()["groups"] > 0) == (scene == "grouped")
    return scene


def trace_guarded(tpt, rays):
    """the call on outputs that start as GUARD, a guard row before and after each and a guard word either side of the counter ->
    (the counter's gain, radiance [n, 4], hits [n, 8]).  The records go up through an integer view: no float copy on the way."""
    import torch
    rays = np.ascontiguousarray(rays, np.float32)
    n = len(rays)
    d_rays = torch.from_numpy(rays.view(np.int32)).cuda()
    assert d_rays.cpu().numpy().tobytes() == rays.tobytes(), "the bytes uploaded are not the bytes built"
    rad = torch.full((n + 2, 4), lib.GUARD, dtype=torch.int32, device="cuda")
    hit = torch.full((n + 2, 8), lib.GUARD, dtype=torch.int32, device="cuda")
    cnt = torch.tensor([5, 1000, 5], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    r0 = tpt.ray_counter_read()
    tpt.trace_rays_device(n, d_rays.data_ptr(), rad.data_ptr() + 16, hit.data_ptr() + 32, cnt.data_ptr() + 8)
    tpt.synchronize()
    assert tpt.ray_counter_read() == r0, "the context's ray counter moved"
    assert d_rays.cpu().numpy().tobytes() == rays.tobytes(), "the call wrote its input"
    rad, hit, cnt = rad.cpu().numpy(), hit.cpu().numpy(), cnt.cpu().numpy().tolist()
    for g in (rad, hit):
        assert (g[[0, -1]] == lib.GUARD).all(), "a guard row was written"
    assert cnt[0] == 5 and cnt[2] == 5, cnt
    return cnt[1] - 1000, rad[1:-1].view(np.float32), hit[1:-1].view(np.float32)


# ---------------------------------------------------------------- 1. the ray families
@pytest.mark.parametrize("config", list(CONFIGS))
def test_length_seam(tpt_defaults, families, config):
    tpt = tpt_defaults
    try:
        f = families[set_up(tpt, config)]
        lib.equal_bits(trace_guarded(tpt, f["length_seam"]), f["want_length_seam"], config)
    finally:
        restore(tpt)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_length_range(tpt_defaults, families, config):
    tpt = tpt_defaults
    try:
        f = families[set_up(tpt, config)]
        plain = lib.equal_bits_or_nan(trace_guarded(tpt, f["length_range"]), f["want_length_range"], config)
        print("length_range, %s: %d NaN words in the reference, plain byte equality %s" % (
            config, lib.nan_words(f["want_length_range"])[0], "held" if plain else "did not hold"))
    finally:
        restore(tpt)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_seed_words(tpt_defaults, families, config):
    tpt = tpt_defaults
    try:
        f = families[set_up(tpt, config)]
        got = trace_guarded(tpt, f["seed_words"])
        lib.equal_bits(got, f["want_seed_words"], config)
        n = lib.SEED_RAYS
        assert got[1][:n].tobytes() == got[1][n:2 * n].tobytes() and got[2][:n].tobytes() == got[2][n:2 * n].tobytes(), "seed 0 is not seed 1"
    finally:
        restore(tpt)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_outside_domain(tpt_defaults, families, checker, config):
    """records the header does not define, in the same waves as good rays (tests/test_rays_kinds.py: why they end; the lane logic ran
    them on the CPU first): the whole 1024, then the first 1000 (a partial last chunk that begins with a bad record), then the good
    rays alone"""
    tpt = tpt_defaults
    try:
        f = families[set_up(tpt, config)]
        s, m, rays, bad = f["s"], f["m"], f["outside_domain"], f["bad"]
        good = np.ascontiguousarray(rays[~bad])
        if "want_good" not in f:
            f["want_good"] = checker.trace(s, m, good)
            f["want_short"] = checker.trace(s, m, np.ascontiguousarray(rays[:lib.OUTSIDE_SHORT][~bad[:lib.OUTSIDE_SHORT]]))
        lib.own_outputs_only(trace_guarded(tpt, rays), bad, f["want_good"], f["lights"], len(s), config)
        lib.own_outputs_only(trace_guarded(tpt, rays[:lib.OUTSIDE_SHORT]), bad[:lib.OUTSIDE_SHORT], f["want_short"], f["lights"], len(s),
                             config + ", the first 1000")
        lib.equal_bits(trace_guarded(tpt, good), f["want_good"], config + ", the good rays afterwards")
    finally:
        restore(tpt)


def test_largest_call(tpt_defaults, checker, oracle):
    """nRays = 16777216: one tile of 4096 camera rays, repeated 4096 times on the device; every tile of the outputs equals the first,
    the first equals the checker, the counter gained 4096 times the tile's count"""
    import torch
    tpt = tpt_defaults
    s, m = rays_lib.default_scene()
    tile = checker.camera_rays(oracle.default_camera(64, 64), 64, 64)
    want = checker.trace(s, m, tile)
    tiles, n = 4096, 4096 * 4096
    assert n == 16777216 and len(tile) == 4096
    tpt.UpdateTest(0.0, 0, 64, 64, 0)
    d_rays = torch.from_numpy(tile.view(np.int32)).cuda().repeat(tiles, 1)
    rad = torch.full((n + 2, 4), lib.GUARD, dtype=torch.int32, device="cuda")
    hit = torch.full((n + 2, 8), lib.GUARD, dtype=torch.int32, device="cuda")
    cnt = torch.tensor([5, 1000, 5], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tpt.trace_rays_device(n, d_rays.data_ptr(), rad.data_ptr() + 16, hit.data_ptr() + 32, cnt.data_ptr() + 8)
    tpt.synchronize()
    dt = time.perf_counter() - t0
    print("largest_call: %d rays, %d HitWorld calls, radiance and hits: %.4f s, %.0f Mray/s" % (n, tiles * want[0], dt, tiles * want[0] / dt / 1e6))
    for out, width, w, name in ((rad, 4, want[1], "radiance"), (hit, 8, want[2], "hits")):
        assert bool((out[0] == lib.GUARD).all()) and bool((out[-1] == lib.GUARD).all()), (name, "a guard row was written")
        body = out[1:-1].view(tiles, 4096 * width)
        first = body[0:1]
        assert first.cpu().numpy().reshape(4096, width).tobytes() == w.view(np.int32).tobytes(), (name, "the first tile is not the checker's")
        for at in range(0, tiles, 512):
            assert torch.equal(body[at:at + 512], first.expand(512, -1)), (name, "a tile from %d on differs from the first" % at)
    assert cnt.cpu().numpy().tolist() == [5, 1000 + tiles * want[0], 5]
    assert torch.equal(d_rays[-4096:].cpu(), torch.from_numpy(tile.view(np.int32))), "the call wrote its input"


# ---------------------------------------------------------------- 2. scenes
_wanted = {}


def trace_scene(tpt, checker, oracle, name, variant=(0, 3, -1), fold=FOLD_RECURSIVE, light_sampling=True, mitsuba_compare=False):
    s, m, _, grouped = lib.scene_case(name, oracle)
    key = (name, fold, light_sampling, mitsuba_compare)
    if key not in _wanted:
        rays = lib.rays_of_case(checker, name, oracle)
        _wanted[key] = (rays, checker.trace(s, m, rays, fold=fold, light_sampling=light_sampling, mitsuba_compare=mitsuba_compare))
    rays, want = _wanted[key]
    assert len(rays) <= 24 * 16 + 192
    try:
        tpt.set_scene(s, m)
        tpt.set_kernel_variant(*variant)
        tpt.set_fold_mode(fold)
        tpt.set_config(light_sampling, 0.9, mitsuba_compare)
        tpt.UpdateTest(0.0, 0, lib.SHAPE[0], lib.SHAPE[1], 0)
        info = tpt.scene_info()
        assert info["spheres"] == len(s) and (info["groups"] > 0) == grouped, (name, info)  # planned as its name says
        got = trace_guarded(tpt, rays)
    finally:
        restore(tpt)
    assert float((want[2][:, 7].view(np.int32) >= 0).mean()) >= 0.2 or name in lib.SEES_SKY
    if name in lib.NONFINITE_SCENES:
        lib.equal_bits_or_nan(got, want, name)
    else:
        assert lib.wholly_finite(want), name
        lib.equal_bits(got, want, name)


@pytest.mark.parametrize("name", lib.scene_names())
def test_every_scene(tpt_defaults, checker, oracle, name):
    trace_scene(tpt_defaults, checker, oracle, name)


@pytest.mark.parametrize("how", list(VARIANTS))
@pytest.mark.parametrize("name", lib.variant_scene_names(ON_EVERY_VARIANT))
def test_the_other_variants(tpt_defaults, checker, oracle, name, how):
    trace_scene(tpt_defaults, checker, oracle, name, **VARIANTS[how])


@pytest.mark.parametrize("n", lib.SWEEP_COUNTS)
def test_sphere_counts_at_the_pair_chunk_and_grouping_seams(tpt_defaults, checker, oracle, n):
    tpt = tpt_defaults
    s, m = lib.sweep_scene(n)
    rays = lib.scene_rays(checker, s, scene_kinds_lib.oracle_camera(oracle, lib.SWEEP_CAMERA, *lib.SHAPE))
    want = checker.trace(s, m, rays)
    try:
        tpt.set_scene(s, m)
        tpt.UpdateTest(0.0, 0, lib.SHAPE[0], lib.SHAPE[1], 0)
        info = tpt.scene_info()
        assert info["spheres"] == n and (info["groups"] > 0) == (n >= 256), info
        lib.equal_bits(trace_guarded(tpt, rays), want, "%d spheres" % n)
        check(trace(tpt, rays, radiance=False), (len(rays), None, want[2]), "%d spheres, hits only" % n)
    finally:
        restore(tpt)
