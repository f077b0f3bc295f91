"""The trace kernels across MATERIALS, SCALE, PLACEMENT and DEGENERATE SPHERES (tests/scene_kinds_lib.py), every image byte for byte and
every frame's ray count against the oracle.  The rest of the suite renders scenes from a narrow range -- roughness up to 0.6, ri 1.5,
albedo inside (0, 1), three known material types, positive radii, no coincident spheres outside the light tests, a camera outside every
sphere and within 40 units of the origin --, and code that exists on the device only depends on it.  Held here:

  - the path-queue kernel's classification with a `type` no class knows (its END arm), with populations that live in one class ring
    (all Lambert, all mirror, all glass) and with closed shells, where every path runs to the depth limit;
  - the matrix-core filter on both sides of its table's limit (a sphere's |a_k| < 60000) and from a camera whose |o|^2 is beyond it,
    where every camera ray carries the full candidate mask into phase 2 and every bounce ray a filtered one;
  - the guarded fast forms of sqrt, 1 / sqrt and the divisions in place, with a ground of r = 2^49 and 2^60 (the discriminant leaves
    [2^-96, 2^96]: tests/test_scene_kinds.py) and scenes scaled by 2^-12 ... 2^16;
  - packScene and buildGroups with negated, zero and coincident radii, flat and grouped, a group dissolved into the big list and the
    flat exit past 64 big spheres, held to tptGetSceneInfo; the lowest-index tie-break of the grouped traversal;
  - HitSpheres itself on those scenes (ids equal, t bit-equal to the oracle's), and the other entry points' instantiations and planes
    on a scene with one of each.

tests/test_scene_kinds.py proves on the CPU that every scene is finite, what its name says, and rendered right by the lane logic."""
import ctypes as C

import numpy as np
import pytest

import scene_kinds_lib as lib
from adaptive_lib import AdaptiveChecker
from aov_lib import AovChecker
from common import grazing_rays, oracle_frames
from moments_lib import MomentsChecker
from object_lib import ObjectChecker
from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE, FOLD_RECURSIVE, SEED_PER_PIXEL
from test_gpu_adaptive import draw_adaptive
from test_gpu_animation import draw_animation
from test_gpu_aov import check as check_aov, draw_aov
from test_gpu_lights import KERNELS, draw, restore
from test_gpu_moments import check as check_moments, draw_moments
from test_gpu_objects import object_planes
from test_gpu_parity import _batched
from test_gpu_views import FOUR_VIEWS, check_against_oracle, draw_views
from test_scene_kinds import group_info

pytestmark = pytest.mark.gpu

VARIANTS = dict(KERNELS, valu_filter=((3, 3, -1), FOLD_RECURSIVE), one_thread_per_pixel=((0, 0, -1), FOLD_RECURSIVE),
                lds_scene_off=((0, 3, 0), FOLD_RECURSIVE))
# one scene per family (and the mechanisms a variant could take differently), every class population
ON_EVERY_VARIANT = ("type_-1", "ri_0.5", "coincident", "negated_radius_glass", "ground_2^49", "scale_2^-12", "far_camera_246", "aperture_5",
                    "grouped_zero_radii", "kitchen_sink") + lib.FAMILIES["populations"]
assert {lib.FAMILY_OF[n] for n in ON_EVERY_VARIANT} == set(lib.FAMILIES)


def draw_scene(tpt, oracle, emu, name, kernel):
    variant, fold = VARIANTS[kernel]
    s, m, camera = lib.scene(name)
    w, h, spp, frames = lib.size_of(name)
    info, scene, per = draw(tpt, oracle, ("scene kind", name), s, m, w, h, spp, frames, variant, fold, camera=camera)
    # the plan for the scene is the one the CPU restatement derives: grouped, flat, or with dissolved groups in the big list
    groups = group_info(emu, s, m)[0]
    assert (groups > 0) == (name in lib.GROUPED)
    assert (scene["spheres"], scene["groups"]) == (len(s), groups), scene
    assert info["blocks_per_cu"] >= 1, info
    return info


# ---------------------------------------------------------------- 1. every scene on both main kernels
@pytest.mark.parametrize("kernel", ["path_queues", "lane_refill"])
@pytest.mark.parametrize("name", list(lib.CATALOGUE))
def test_every_scene(tpt_defaults, oracle, emu, name, kernel):
    draw_scene(tpt_defaults, oracle, emu, name, kernel)


# ---------------------------------------------------------------- 2. the other kernel variants
@pytest.mark.parametrize("kernel", ["all_exact", "valu_filter", "one_thread_per_pixel", "forward_fold", "lds_scene_off"])
@pytest.mark.parametrize("name", ON_EVERY_VARIANT)
def test_the_other_variants(tpt_defaults, oracle, emu, name, kernel):
    draw_scene(tpt_defaults, oracle, emu, name, kernel)


# ---------------------------------------------------------------- 3. the hit level
def mixed_rays(s, n, seed):
    """half grazing rays of the scene's spheres, half rays from random origins within two scene radii (the spheres above the ground:
    their centres' spread plus the largest radius) with unit directions"""
    rng = np.random.default_rng(seed)
    c = np.stack([s["cx"][1:], s["cy"][1:], s["cz"][1:]], 1).astype(np.float64)
    centre = c.mean(axis=0)
    radius = (np.linalg.norm(c - centre, axis=1) + np.abs(s["radius"][1:])).max()
    k = n - n // 2
    o = rng.normal(size=(k, 3))
    o = centre + o / np.linalg.norm(o, axis=1, keepdims=True) * (2 * radius * rng.uniform(0, 1, (k, 1)) ** (1 / 3))
    d = rng.normal(size=(k, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d = (d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    return np.concatenate([grazing_rays(s, n // 2, seed=seed), np.concatenate([o.astype(np.float32), d], 1)], 0).astype(np.float32)


def oracle_hits(oracle, s, rays):
    ids, ts, t = np.empty(len(rays), np.int32), np.empty(len(rays), np.float32), C.c_float()
    o, d = np.ascontiguousarray(rays[:, :3]), np.ascontiguousarray(rays[:, 3:])
    for i in range(len(rays)):
        ids[i] = oracle.lib.tpto_hit_spheres(s.ctypes.data, len(s), o[i].ctypes.data, d[i].ctypes.data, 0.001, 1.0e7, C.byref(t), None, None)
        ts[i] = t.value if ids[i] >= 0 else np.float32(1.0e7)
    return ids, ts


def rays_that_hit(make, reference, tries=8):
    """a ray set whose reference hit rate is at least 0.2 (so that the comparison is not one of misses): redrawn with another seed
    until it is -> (rays, reference ids, reference t)"""
    for seed in range(31, 31 + tries):
        rays = make(seed)
        ids, ts = reference(rays)
        if (ids >= 0).mean() >= 0.2:
            return rays, ids, ts
    raise AssertionError("no ray set of %d seeds hits the scene with a fifth of its rays" % tries)


@pytest.mark.parametrize("name", lib.FAMILIES["degenerate"] + lib.FAMILIES["placement"])
def test_hit_spheres_vs_oracle(tpt_hooks, oracle, name):
    tpt = tpt_hooks
    s, m, _ = lib.scene(name)
    assert len(s) <= 64
    rays, want_id, want_t = rays_that_hit(lambda seed: mixed_rays(s, 4000, seed), lambda r: oracle_hits(oracle, s, r))
    try:
        tpt.set_scene(s, m)
        tpt.UpdateTest(0.0, 0, 64, 64, 2)
        for hs in (0, 1):
            ids, ts = tpt.test_hit_spheres(rays, hs)
            assert np.array_equal(ids, want_id), (hs, int((ids != want_id).sum()))
            assert np.array_equal(ts.view(np.uint32), want_t.view(np.uint32)), hs
        # the table's seam on the device: the matrix-core filter runs exactly for the scenes the CPU restatement builds a table for
        if name in lib.NO_TABLE:
            with pytest.raises(tpt.TptError, match="no matrix table"):
                tpt.test_matrix_filter(rays, hits=True)
        else:
            _, ids, ts = tpt.test_matrix_filter(rays, hits=True)
            assert np.array_equal(ids, want_id) and np.array_equal(ts.view(np.uint32), want_t.view(np.uint32))
    finally:
        tpt.set_scene(None)


@pytest.mark.parametrize("name", ["grouped_negated", "grouped_coincident", "grouped_zero_radii", "flat_zero_radii"])
def test_grouped_traversal_vs_the_exact_loop_on_grazing_rays(tpt_hooks, name):
    tpt = tpt_hooks
    s, m, _ = lib.scene(name)
    try:
        tpt.set_scene(s, m)
        tpt.UpdateTest(0.0, 0, 64, 64, 2)
        assert (tpt.scene_info()["groups"] > 0) == (name in lib.GROUPED)
        rays, id1, t1 = rays_that_hit(lambda seed: grazing_rays(s, 20000, seed=seed), lambda r: tpt.test_hit_spheres(r, 1))
        id0, t0 = tpt.test_hit_spheres(rays, 0)
        assert np.array_equal(id0, id1) and np.array_equal(t0.view(np.uint32), t1.view(np.uint32))
        if name == "grouped_coincident":
            first, copies = lib.COINCIDENT_IN_GROUPS
            assert (id0 == first).sum() > 100 and not np.isin(id0, list(copies)).any()  # (equal t: the lowest index)
        if name == "grouped_negated":
            assert np.isin(id0, list(lib.NEGATED_IN_GROUPS)).sum() > 1000
    finally:
        tpt.set_scene(None)


# ---------------------------------------------------------------- 4. kitchen_sink through the other entry points
W, H, SPP, N = 66, 35, 2, 3


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    """the existing modules' CPU statements of the planes, built on first use and once"""
    built = {}

    def get(cls):
        if cls not in built:
            built[cls] = cls(tmp_path_factory.mktemp(cls.__name__))
        return built[cls]
    return get


@pytest.fixture()
def sink(tpt_defaults):
    tpt = tpt_defaults
    s, m, camera = lib.scene("kitchen_sink")
    assert camera is None
    tpt.set_scene(s, m)
    tpt.set_samples_per_pixel(SPP)
    try:
        yield tpt, s, m
    finally:
        restore(tpt)


def test_aov(sink, oracle, checkers):
    tpt, s, m = sink
    alb, nd = check_aov(checkers(AovChecker), oracle, draw_aov(tpt, W, H, range(N)), W, H, SPP, N, spheres=s, mats=m)
    assert np.isfinite(alb).all() and np.isfinite(nd).all()  # (the negated radius' normal is (p - c) * invRadius: finite, facing inward)


def test_moments(sink, oracle, checkers):
    tpt, s, m = sink
    check_moments(checkers(MomentsChecker), oracle, draw_moments(tpt, W, H, range(N)), W, H, SPP, N, spheres=s, mats=m)


def test_object_plane(sink, checkers):
    tpt, s, m = sink
    w, h = 130, 67
    tpt.UpdateTest(0.0, 0, w, h, 0)
    cam = tpt.GetSceneDesc()[2]
    got = object_planes(tpt, w, h)
    tpt.synchronize()
    got = got.cpu().numpy()
    assert got.tobytes() == checkers(ObjectChecker).plane(s, cam, w, h).tobytes()
    k = lib.KITCHEN_SINK
    first, copies = k["coincident"]
    assert (got == first).any() and not np.isin(got, list(copies)).any()  # coincident spheres: the lowest index
    assert (got == k["unknown"]).any() and (got == k["negated"]).any()


def test_views(sink, oracle):
    tpt, s, m = sink
    tiles, per = draw_views(tpt, W, H, FOUR_VIEWS, range(N))
    check_against_oracle(oracle, tiles, per, FOUR_VIEWS, W, H, SPP, N, spheres=s, mats=m)


def test_animation(sink, oracle):
    tpt, s, m = sink
    flags = FLAG_PROGRESSIVE | FLAG_ANIMATE
    times = [0.4 * j for j in range(N)]
    tile, images, per = draw_animation(tpt, W, H, times, flags=flags)
    spheres, cam, bo, got = s.copy(), oracle.default_camera(W, H), np.zeros((H, W, 4), np.float32), images.cpu().numpy()
    for f, t in enumerate(times):
        oracle.animate(spheres, t)
        r, _ = oracle.render(spheres, m, cam, W, H, SPP, f, flags, backbuffer=bo, seed_mode=SEED_PER_PIXEL)
        assert per[f] == r, (f, per[f], r)
        assert got[f].tobytes() == bo.tobytes(), "frame %d differs from the oracle" % f
    assert tile.cpu().numpy().tobytes() == bo.tobytes()


def test_adaptive(sink, oracle, checkers):
    tpt, s, m = sink
    counts = np.random.default_rng(3).choice(np.int32([0, 1, 2, 3, 5]), size=(H, W)).astype(np.int32)
    got = draw_adaptive(tpt, W, H, range(N), counts)
    per, bb, mo, alb, nd = checkers(AdaptiveChecker).frames(oracle, W, H, counts, N, spheres=s, mats=m)
    assert got[4] == per
    for name, g, want in zip(("tile", "moments", "albedo", "normal / depth"), got[:4], (bb, mo, alb, nd)):
        assert g.tobytes() == want.tobytes(), "the %s differs from the checker" % name


def test_batch_of_three_frames(sink, oracle):
    """three frames in one launch: the frame-pools kernel"""
    tpt, s, m = sink
    rays, got = _batched(tpt, W, H, [3], spp=SPP)
    ro, bo, _ = oracle_frames(oracle, W, H, SPP, 3, spheres=s, mats=m, seed_mode=SEED_PER_PIXEL)
    assert rays == ro
    assert got.tobytes() == bo.tobytes()
