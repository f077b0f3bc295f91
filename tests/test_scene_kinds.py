"""The catalogue of tests/scene_kinds_lib.py on the CPU, at the sizes tests/test_gpu_scene_kinds.py draws it on the GPU: for every scene
the oracle's image is finite (so byte equality is a fair demand), the host restatement of the kernels' lane logic (tests/lane_emu.cpp)
renders the oracle's bytes and per-frame ray counts -- emu_render with the product's filters (0), the all-exact loop (1) and the packed
VALU filter (3), both folds; emu_render_queue_classes, the path-queue kernel's class code, with 0 and 1 --, and the scene is what its name
says, proven from that restatement and not from the library under test: grouped, flat or with a dissolved group in the big list
(emu_group_info), with or without a matrix-core table (emu_matrix_masks), hit by the paths at all, which sphere the camera's rays hit first.

Every value the catalogue holds is finite at these sizes; none had to be moved.  Two things came out otherwise than expected and are
asserted as they are: the scene moved out by 240 has no table (2 x 240^2 > 60000), and a metal shell of radius +12 ends the paths that
reach it where a closed shell was to keep them -- the mirror shell that does is the one of radius -12 (19 rays per primary ray)."""
import ctypes as C

import numpy as np
import pytest

import scene_kinds_lib as lib
from common import grazing_rays
from object_lib import centre_rays
from oracle_lib import FLAG_PROGRESSIVE, FOLD_FORWARD, FOLD_RECURSIVE, SEED_PER_PIXEL
from test_lane_logic import _matrix_masks

TABLE_LIMIT = np.float32(60000.0)  # tpt_scene.h matrixPutEntry / tpt_trace.h: |a_k| and the ray's |o|^2 below it
_oracle_frames = {}


def oracle_frames_of(oracle, name, fold=FOLD_RECURSIVE):
    """(image, per-frame rays, rays per primary ray) of the scene at its test size, rendered once"""
    if (name, fold) not in _oracle_frames:
        s, m, camera = lib.scene(name)
        w, h, spp, frames = lib.size_of(name)
        cam = lib.oracle_camera(oracle, camera, w, h)
        bb, per = np.zeros((h, w, 4), np.float32), []
        for f in range(frames):
            r, _ = oracle.render(s, m, cam, w, h, spp, f, FLAG_PROGRESSIVE, seed_mode=SEED_PER_PIXEL, fold_mode=fold, backbuffer=bb)
            per.append(r)
        bb.setflags(write=False)
        _oracle_frames[name, fold] = (bb, per, sum(per) / (w * h * spp * frames))
    return _oracle_frames[name, fold]


def group_info(emu, s, m):
    """(groups, group pairs, spheres in the big list) as packScene builds them; 0 groups: a flat scene"""
    emu.emu_group_info.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    emu.emu_group_info.restype = None
    info = np.zeros(3, np.int32)
    emu.emu_group_info(s.ctypes.data, m.ctypes.data, len(s), info.ctypes.data)
    return tuple(int(v) for v in info)


def has_table(emu, s, m):
    return _matrix_masks(emu, s, m, np.zeros((1, 6), np.float32))[0] >= 0


def camera_rays(oracle, name):
    """the rays through the pixel centres and the lens centre -> float32 [w * h, 6]"""
    s, m, camera = lib.scene(name)
    w, h, _, _ = lib.size_of(name)
    o, d = centre_rays(lib.oracle_camera(oracle, camera, w, h), w, h)
    rays = np.empty((h, w, 6), np.float32)
    rays[..., :3] = o
    for k in range(3):
        rays[..., 3 + k] = d[k]
    return rays.reshape(-1, 6)


def first_hits(emu, oracle, name):
    """the sphere each of camera_rays() hits first (-1: the sky), by the all-exact loop of the restatement"""
    emu.emu_hit_spheres.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    emu.emu_hit_spheres.restype = None
    s, m, _ = lib.scene(name)
    rays = camera_rays(oracle, name)
    ids, ts = np.empty(len(rays), np.int32), np.empty(len(rays), np.float32)
    emu.emu_hit_spheres(s.ctypes.data, m.ctypes.data, len(s), 1, rays.ctypes.data, len(rays), ids.ctypes.data, ts.ctypes.data)
    return ids


def emu_frames(emu, s, m, cam, w, h, spp, frames, hs, fold):
    bb, per = np.zeros((h, w, 4), np.float32), []
    for f in range(frames):
        per.append(emu.emu_render(s.ctypes.data, m.ctypes.data, len(s), cam.ctypes.data, w, h, 0, h, spp, f, FLAG_PROGRESSIVE, SEED_PER_PIXEL,
                                  hs, fold, bb.ctypes.data))
    return bb, per


def queue_frames(emu, s, m, cam, w, h, spp, frames, hs):
    fn = emu.emu_render_queue_classes
    fn.restype = C.c_int64
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_uint, C.c_int, C.c_void_p]
    bb, per = np.zeros((h, w, 4), np.float32), []
    for f in range(frames):
        per.append(fn(s.ctypes.data, m.ctypes.data, len(s), cam.ctypes.data, w, h, spp, f, FLAG_PROGRESSIVE, hs, bb.ctypes.data))
    return bb, per


# ---------------------------------------------------------------- 1. every scene: finite, and the lane logic renders it
@pytest.mark.parametrize("name", list(lib.CATALOGUE))
def test_the_lane_logic_renders_the_oracles_bytes(emu, oracle, name):
    s, m, camera = lib.scene(name)
    w, h, spp, frames = lib.size_of(name)
    cam = lib.oracle_camera(oracle, camera, w, h)
    for fold in (FOLD_RECURSIVE, FOLD_FORWARD):
        bo, pero, _ = oracle_frames_of(oracle, name, fold)
        assert np.isfinite(bo).all(), "the oracle's own image is not finite: the scene is no fair test (tests/scene_kinds_lib.py)"
        for hs in (0, 1, 3):
            be, per = emu_frames(emu, s, m, cam, w, h, spp, frames, hs, fold)
            assert per == pero, (hs, fold, per, pero)
            assert be.tobytes() == bo.tobytes(), (hs, fold)
    bo, pero, _ = oracle_frames_of(oracle, name)
    for hs in (0, 1):
        bq, per = queue_frames(emu, s, m, cam, w, h, spp, frames, hs)
        assert per == pero, (hs, per, pero)
        assert bq.tobytes() == bo.tobytes(), hs


# ---------------------------------------------------------------- 2. every scene is what its name says
@pytest.mark.parametrize("name", list(lib.CATALOGUE))
def test_grouping_table_and_hits_are_what_the_name_says(emu, oracle, name):
    s, m, _ = lib.scene(name)
    groups, _, big = group_info(emu, s, m)
    assert (groups > 0) == (name in lib.GROUPED), (groups, big)
    assert has_table(emu, s, m) == (name not in lib.NO_TABLE)
    if lib.FAMILY_OF[name] != "grouped":
        assert len(s) <= 64  # (the table's absence is the spheres' doing, not the count's)
    _, _, rays_per_primary = oracle_frames_of(oracle, name)
    if name == "camera_inside_metal":
        # the mirror's normal points away from the camera inside it: the reflected ray points into the surface and the path ends with
        # its first hit (Test.cpp:218-221) -- every path of the frame is one ray, and all of them sit in the metal class
        assert rays_per_primary == 1.0
    else:
        assert rays_per_primary > 1.5, "the paths hardly hit the scene"


def test_the_closed_shells_keep_their_paths(emu, oracle):
    """no camera ray reaches the sky, and the shells that return their paths cost more rays than the built-in scene.  The metal shell of
    radius +12 returns none (scene_kinds_lib.closed_shell): what reaches it ends as it would in the sky, and its figure is the built-in
    scene's within the few paths whose random numbers moved -- the mirror that runs its paths to the depth limit is the one of radius -12."""
    from common import oracle_frames
    w, h, spp, frames = lib.size_of("shell_lambert")
    total, _, _ = oracle_frames(oracle, w, h, spp, frames, seed_mode=SEED_PER_PIXEL)
    plain = total / (w * h * spp * frames)
    assert 4 < plain < 5
    for name in lib.CLOSED_SHELLS + ("shell_mirror",):
        assert (first_hits(emu, oracle, name) >= 0).all(), "a camera ray reaches the sky"
    for name in lib.CLOSED_SHELLS:
        assert oracle_frames_of(oracle, name)[2] > plain, name
    assert oracle_frames_of(oracle, "shell_mirror_inward")[2] > 3 * plain
    assert abs(oracle_frames_of(oracle, "shell_mirror")[2] - plain) < 0.1


# ---------------------------------------------------------------- 3. the mechanisms the catalogue is there for
@pytest.mark.parametrize("name", lib.FAMILIES["materials"][-3:] + ("kitchen_sink",))
def test_camera_rays_end_on_a_type_no_class_knows(emu, oracle, name):
    """the Q_END arm of the path-queue kernel's classification is taken by first hits, in number"""
    s, m, _ = lib.scene(name)
    unknown = np.nonzero(~np.isin(m["type"], (lib.LAMBERT, lib.METAL, lib.DIELECTRIC)))[0]
    assert unknown.tolist() == (list(lib.UNKNOWN_TYPE_IDS) if name != "kitchen_sink" else [lib.KITCHEN_SINK["unknown"]])
    ids = first_hits(emu, oracle, name)
    assert np.isin(ids, unknown).sum() >= 50 and all((ids == i).sum() >= 50 for i in unknown if i in (2, 3)), np.unique(ids, return_counts=True)


@pytest.mark.parametrize("name,kind", [("all_lambert", lib.LAMBERT), ("all_mirror", lib.METAL), ("all_glass", lib.DIELECTRIC)])
def test_one_class_populations_have_one_class(name, kind):
    _, m, _ = lib.scene(name)
    assert (m["type"] == kind).all() and (kind != lib.METAL or (m["roughness"] == 0).all())


def test_coincident_spheres_show_the_lowest_index(emu, oracle):
    for name, (first, copies) in (("coincident", lib.COINCIDENT), ("grouped_coincident", lib.COINCIDENT_IN_GROUPS),
                                  ("kitchen_sink", lib.KITCHEN_SINK["coincident"])):
        s, _, _ = lib.scene(name)
        for i in copies:
            assert all(s[k][i] == s[k][first] for k in ("cx", "cy", "cz", "radius"))
        ids = first_hits(emu, oracle, name)
        assert not np.isin(ids, list(copies)).any(), (name, np.unique(ids, return_counts=True))
        if name != "grouped_coincident":  # (there the coincident spheres stand beside the camera's view: bounce and shadow rays reach them)
            assert (ids == first).sum() >= 50, name
        # rays aimed at them: the all-exact loop and the product's traversal both answer with the lowest index
        m = lib.scene(name)[1]
        rays = grazing_rays(s[[first] + list(copies)], 4000, seed=7)
        for hs in (0, 1, 3):
            ids, ts = np.empty(len(rays), np.int32), np.empty(len(rays), np.float32)
            emu.emu_hit_spheres(s.ctypes.data, m.ctypes.data, len(s), hs, rays.ctypes.data, len(rays), ids.ctypes.data, ts.ctypes.data)
            assert (ids == first).sum() >= 500 and not np.isin(ids, list(copies)).any(), (name, hs)


def test_negated_and_zero_radii_are_in_view(emu, oracle):
    for name, negated in (("negated_radius_glass", [7]), ("negated_radius_metal", [5]), ("negated_radius_lambert", [2]),
                          ("grouped_negated", list(lib.NEGATED_IN_GROUPS)), ("kitchen_sink", [lib.KITCHEN_SINK["negated"]])):
        s, _, _ = lib.scene(name)
        assert (s["radius"][negated] < 0).all() and (s["radius"] < 0).sum() == len(negated)
        ids = first_hits(emu, oracle, name)
        assert np.isin(ids, negated).sum() >= 50, name  # (a sphere of negated radius is hit like any other: r enters as r^2)
    for name, zeros in (("zero_radius", [5]), ("grouped_zero_radii", list(lib.ZEROS_IN_DISTINCT_GROUPS))):
        s, _, _ = lib.scene(name)
        assert (s["radius"][zeros] == 0).all() and np.isinf(s["invRadius"][zeros]).all()
        assert not np.isin(first_hits(emu, oracle, name), zeros).any()  # (discriminant <= 0: never hit)
    s, m, _ = lib.scene("hollow_glass")
    assert s["radius"][46] == np.float32(-0.9) * s["radius"][7] and m["type"][46] == lib.DIELECTRIC


@pytest.mark.parametrize("name,i", [("camera_inside_glass", 7), ("camera_inside_lambert", 2), ("camera_inside_metal", 5)])
def test_a_camera_inside_a_sphere_sees_that_sphere_alone(emu, oracle, name, i):
    assert (first_hits(emu, oracle, name) == i).all()  # (the far root)


def test_build_groups_dissolve_and_flat_exits(emu):
    """a zero radius makes rho = a / r infinite: its group of eight goes to the big list, whole (tpt_scene.h buildGroups); the big list
    holds 64 spheres, past that the scene stays flat"""
    from toypathtracer_amd.scenes import stress_scene
    groups0, _, big0 = group_info(emu, *stress_scene(1000, 20))
    assert groups0 == 125 and big0 == 5  # (the ground and the four lights)
    s, m, _ = lib.scene("grouped_zero_radii")
    groups, _, big = group_info(emu, s, m)
    assert groups == groups0 - len(lib.ZEROS_IN_DISTINCT_GROUPS) and big == big0 + 8 * len(lib.ZEROS_IN_DISTINCT_GROUPS) <= 64, (groups, big)
    s, m, _ = lib.scene("flat_zero_radii")
    assert (s["radius"] == 0).sum() == 70 and group_info(emu, s, m) == (0, 0, 0)
    for name in ("grouped_negated", "grouped_coincident", "grouped_glass", "grouped_offset_240", "grouped_offset_10000"):
        assert group_info(emu, *lib.scene(name)[:2])[0::2] == (groups0, big0), name  # (|r|, coincident members, a far origin: grouped as ever)


def test_the_table_ends_at_60000(emu, oracle):
    """a sphere's a_k = c_x^2 crosses the limit between x = 244.9 and 245; a camera ray from |o|^2 >= 60000 keeps every sphere of a table
    that exists (tpt_trace.h phase1MatrixH), a bounce ray inside the scene is filtered"""
    for x, table in ((244, True), (244.9, True), (245, False), (300, False)):
        s, m, _ = lib.scene("big_sphere_at_%g" % x)
        assert (s["cx"][9] * s["cx"][9] < TABLE_LIMIT) == table == has_table(emu, s, m), x
    everything = np.uint64(((1 << 46) - 1) << 18)
    for d in (244, 246, 2000):
        name = "far_camera_%d" % d
        s, m, camera = lib.scene(name)
        rays = camera_rays(oracle, name)
        o = rays[0, :3]
        assert (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2] >= TABLE_LIMIT
        r1, masks, _, _ = _matrix_masks(emu, s, m, rays)
        assert r1 >= 0 and (masks == everything).all()
        inside = rays.copy()
        inside[:, :3] = (0.0, 0.5, 0.0)
        _, masks, _, _ = _matrix_masks(emu, s, m, inside)
        assert np.mean([bin(int(x)).count("1") for x in masks[::50]]) < 6
    # the default camera is inside the table's range: its rays are filtered
    _, masks, _, _ = _matrix_masks(emu, *lib.scene("aperture_0")[:2], camera_rays(oracle, "aperture_0"))
    assert (masks != everything).all()


def test_the_huge_grounds_leave_the_fast_square_root_range(oracle):
    """tpt_math.h tsqrt: the five-instruction form holds for 2^-96 <= x <= 2^96, outside it the compiler's expansion runs.  The ground's
    discriminant nb^2 - (|c - o|^2 - r^2) for the camera's rays, restated as HitSpheres computes it (Test.cpp:329, one float32 operation
    per step): with r = 2^49 the downward rays steeper than 30 degrees pass 2^96, with r = 2^60 every downward ray does -- the guard is
    reached in those frames.  With r = 2^30 and in the scaled scenes (2^-12 ... 2^16) the root's arguments stay inside."""
    hi, lo = np.float32(2.0 ** 96), np.float32(2.0 ** -96)

    def discriminants(name):
        s, _, _ = lib.scene(name)
        rays = camera_rays(oracle, name)
        with np.errstate(over="ignore"):
            co = [s[k][0] - rays[:, j] for j, k in enumerate(("cx", "cy", "cz"))]
            nb = (co[0] * rays[:, 3] + co[1] * rays[:, 4]) + co[2] * rays[:, 5]
            c = ((co[0] * co[0] + co[1] * co[1]) + co[2] * co[2]) - s["radius"][0] * s["radius"][0]
            return (nb * nb - c).astype(np.float32), rays[:, 4]
    d, dy = discriminants("ground_2^49")
    assert (d[dy < -0.51] > hi).all() and (d > hi).mean() > 0.3
    d, dy = discriminants("ground_2^60")
    assert (d[dy < -1e-3] > hi).all() and (d > hi).mean() > 0.5
    for name in ("ground_2^30", "scale_2^-12", "scale_2^16"):
        d, _ = discriminants(name)
        assert ((d <= 0) | ((d >= lo) & (d <= hi))).all(), name
