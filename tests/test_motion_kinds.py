"""The catalogue of tests/motion_kinds_lib.py on the CPU, at the sizes tests/test_gpu_motion_kinds.py draws it on the GPU.  Every case is
what its name says, proven from the host restatement (packScene's mxR1 per frame: the table_seam patterns, the seam itself found by
bisection), the oracle's HitSpheres (the ties) and the cameras (the camera inside a moved sphere); every frame shows a moved sphere and a
static one on 5 % of its pixels, by the oracle's object plane, except where the catalogue says that none can and this file proves why;
and tpt_trace.h compiled for the host (tests/lane_emu.cpp emu_hit_spheres_moved) finds, with the filter data of the scene a launch STAGES
-- its last frame's --, the mask of the moved spheres and frame j's table of centres, the sphere, the bits of t and the normal that the
exact loop finds over frame j's own spheres: hitSpheresTwoPhase<true, KEYS> always, hitSpheresCandidates<true, KEYS> behind the
matrix-core filter's restatement where the staged scene has a table.  The host's routing is driven on the emulated runtime."""
import ctypes as C

import numpy as np
import pytest

import motion_kinds_lib as lib
from isa_lib import run_refusals
from object_lib import ObjectChecker, centre_rays
from oracle_lib import Oracle
from test_lane_logic import _matrix_masks

f32 = np.float32


def matrix_r1(emu, s, m):
    emu.emu_matrix_r1.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    emu.emu_matrix_r1.restype = C.c_int
    s, m = np.ascontiguousarray(s), np.ascontiguousarray(m)
    return emu.emu_matrix_r1(s.ctypes.data, m.ctypes.data, len(s))


def bisect_floats(inside, outside, has_table):
    """adjacent binary32 values (last with a table, first without) between `inside` (has one) and `outside` (has none), both positive"""
    a, b = int(f32(inside).view(np.uint32)), int(f32(outside).view(np.uint32))
    assert a < b and has_table(f32(inside)) and not has_table(f32(outside))
    while b - a > 1:
        mid = (a + b) // 2
        if has_table(np.uint32(mid).view(f32)):
            a = mid
        else:
            b = mid
    return np.uint32(a).view(f32), np.uint32(b).view(f32)


def table_seam_of(emu):
    """sphere 9 of scene_kinds_lib.big_sphere_at (r = 30): the last x at which packScene builds a matrix table and the first at which
    it builds none"""
    import scene_kinds_lib as kinds
    s, m, _ = kinds.scene("big_sphere_at_244")

    def has_table(x):
        t = s.copy()
        t["cx"][lib.SEAM_ID] = x
        return matrix_r1(emu, t, m) >= 0
    return bisect_floats(244.9, 245.0, has_table)


@pytest.fixture(scope="module", autouse=True)
def seam(emu):
    lib.set_table_seam(*table_seam_of(emu))
    return lib.TABLE_SEAM


@pytest.fixture(scope="module")
def object_checker(tmp_path_factory):
    return ObjectChecker(tmp_path_factory.mktemp("object_checker"))


def cameras_of(views, w, h):
    o = Oracle.get()
    return [o.camera(v[0:3], v[3:6], (0, 1, 0), v[6], w / h, v[7], v[8]) for v in views]


def test_the_seam_is_where_the_static_catalogue_brackets_it(seam):
    inside, outside = seam
    assert f32(244.9) <= inside < outside <= f32(245) and np.nextafter(inside, f32(np.inf)) == outside
    print("the table ends between x = %r and %r (r = 30)" % (float(inside), float(outside)))


# ---------------------------------------------------------------- 1. every case is what its name says
def test_the_catalogue_is_whole():
    assert set(lib.FAMILIES) == {"reach", "table_seam", "ties", "lights", "degenerate", "ids"}
    assert {lib.META[n]["reach_k"] for n in lib.FAMILIES["reach"]} == {-24, -20, 0, 4, 7, 10, 20, 40, 60, 127}
    assert all(("reach_2^%d_%s" % (k, tag)) in lib.CATALOGUE for k in lib.REACH_K for tag in ("mid", "last"))
    for n in range(1, 9):
        assert len(lib.case("moved_%d" % n)[3]) == n
    assert len(lib.FALLBACKS) == 6 and all(lib.META[n]["launches"] == 3 for n in lib.FALLBACKS)


@pytest.mark.parametrize("name", list(lib.CATALOGUE))
def test_a_case_is_well_formed(name):
    s, m, views, ids, centres, flags, first = lib.case(name)
    w, h, spp = lib.META[name]["size"]
    n = len(views)
    assert n == (33 if name == "seam_33_frames" else 3) and (w, h, spp) == ((48, 27, 1) if n == 33 else (96, 54, 2))
    assert centres.shape == (n, len(ids), 3) and centres.dtype == f32 and views.shape == (n, 9) and np.isfinite(centres).all()
    assert len(set(ids.tolist())) == len(ids) and ids.min() >= 0 and ids.max() < len(s) == len(m)
    with np.errstate(divide="ignore"):
        assert (s["invRadius"].view(np.uint32) == (f32(1) / s["radius"]).view(np.uint32)).all()
    frame_by_frame = len(ids) > 8 or ids.max() >= 64 or len(s) >= 256
    assert (lib.META[name]["launches"] == n) == frame_by_frame == (name in lib.FALLBACKS)
    if not frame_by_frame:
        assert lib.META[name]["launches"] == (n + 31) // 32


@pytest.mark.parametrize("name", lib.FAMILIES["reach"])
def test_reach_moves_by_what_the_name_says(name):
    s, m, views, ids, centres, _, _ = lib.case(name)
    k = lib.META[name]["reach_k"]
    home = lib.centres_of(s, ids, 1)[0]
    away = [j for j in range(3) if centres[j].tobytes() != home.tobytes()]
    assert away == ([2] if name.endswith("_last") else [1]) and tuple(ids) == lib.REACH_IDS
    moved = centres[away[0]]
    if k == 127:
        assert (np.abs(moved).max(axis=1) == f32(3e38)).all()
    elif k == -24:
        assert (moved[:, 0].view(np.uint32) == home[:, 0].view(np.uint32) + 1).all() and moved[:, 1:].tobytes() == home[:, 1:].tobytes()
    else:
        assert (moved[:, 0] == home[:, 0] + f32(2.0 ** k)).all() and (moved[:, 0] != home[:, 0]).all()
        assert moved[:, 1:].tobytes() == home[:, 1:].tobytes()
        if k >= 10:  # the far frame's view stands outside the binary16 range of the filter's ray operands
            o = views[away[0], :3].astype(np.float64)
            assert (o * o).sum() >= 60000.0


@pytest.mark.parametrize("name", lib.FAMILIES["table_seam"])
def test_the_table_comes_and_goes_as_the_name_says(emu, name):
    s, m, views, ids, centres, _, _ = lib.case(name)
    want = lib.META[name]["table"]
    got = tuple(matrix_r1(emu, lib.scene_of(s, ids, centres, j), m) >= 0 for j in range(len(views)))
    assert got == tuple(want), (got, want)
    assert True in got and False in got
    if len(views) == 33:
        assert got[31] and not got[32] and False in got[:31], "the two launches are to stage scenes of different kinds"
    if "exact" in name or len(views) == 33:
        assert set(centres[:, 0, 0].tolist()) >= {float(v) for v in lib.TABLE_SEAM}


def oracle_first_hits(oracle, s, cam, w, h):
    o, d = centre_rays(cam, w, h)
    o = np.ascontiguousarray(o, f32)
    dirs = np.ascontiguousarray(np.stack(d, axis=-1).reshape(-1, 3), f32)
    ids, t = np.empty(w * h, np.int32), C.c_float()
    s = np.ascontiguousarray(s)
    for i in range(w * h):
        ids[i] = oracle.lib.tpto_hit_spheres(s.ctypes.data, len(s), o.ctypes.data, dirs[i].ctypes.data, 0.001, 1.0e7, C.byref(t), None, None)
    return ids


@pytest.mark.parametrize("name", [n for n in lib.CATALOGUE if "tie" in lib.META[n]])
def test_a_tie_shows_the_lower_index(oracle, name):
    s, m, views, ids, centres, _, _ = lib.case(name)
    w, h, _ = lib.META[name]["size"]
    frame, shown, hidden = lib.META[name]["tie"]
    assert shown < hidden
    for j in range(len(views)):
        sj = lib.scene_of(s, ids, centres, j)
        same = all(sj[k][shown] == sj[k][hidden] for k in ("cx", "cy", "cz", "radius"))
        assert same == (j == frame)
        if j == frame:
            got = oracle_first_hits(oracle, sj, cameras_of(views, w, h)[j], w, h)
            assert (got == shown).sum() >= 200 and (got == hidden).sum() == 0, np.unique(got, return_counts=True)


@pytest.mark.parametrize("name", [n for n in lib.CATALOGUE if "inside" in lib.META[n]])
def test_the_camera_is_inside_in_one_frame_only(name):
    s, m, views, ids, centres, _, _ = lib.case(name)
    frame, i = lib.META[name]["inside"]
    assert i in ids
    for j in range(len(views)):
        sj = lib.scene_of(s, ids, centres, j)
        d2 = sum((float(views[j, a]) - float(sj[k][i])) ** 2 for a, k in enumerate(("cx", "cy", "cz")))
        r2 = float(sj["radius"][i]) ** 2
        assert d2 < 0.9 * r2 if j == frame else d2 >= r2, (j, d2)  # (well inside in its frame, not inside at all in the others)


def test_the_light_cases_move_both_lights():
    for name in lib.FAMILIES["lights"]:
        s, m, views, ids, centres, _, _ = lib.case(name)
        assert set(lib.LIGHTS) <= set(ids.tolist()) and lib.META[name]["light_sampling"] == (not name.endswith("_nols"))
        home = lib.centres_of(s, ids, 1)[0]
        assert all((centres[j, :2] != home[:2]).any() for j in (1, 2)) and (centres[1:, :2] != home[:2]).any(axis=(0, 2)).all()
    s, m, _, ids, c, _, _ = lib.case("lights_far")
    assert np.abs(c[1, :2]).max() >= 2.0 ** 20 and np.abs(c[2, :2]).max() >= 2.0 ** 20
    s, m, _, ids, c, _, _ = lib.case("lights_coincident")
    assert c[1, 0].tobytes() == c[1, 1].tobytes() and c[2, 0].tobytes() == c[2, 1].tobytes() != c[1, 0].tobytes()
    s, m, _, ids, c, _, _ = lib.case("lights_on_the_floor")
    g = s[0]
    for j in (1, 2):
        for k in (0, 1):  # the centre is on the ground sphere to a few ulps of its radius: the floor around it is inside the light
            d = np.sqrt(sum((np.float64(c[j, k, a]) - np.float64(g[n])) ** 2 for a, n in enumerate(("cx", "cy", "cz"))))
            assert abs(d - 100.0) < 1e-4 and s["radius"][ids[k]] == f32(0.3)


def test_the_degenerate_cases_are_degenerate():
    s, _, _, ids, c, _, _ = lib.case("moved_zero_radius")
    assert s["radius"][ids[0]] == 0 and np.isinf(s["invRadius"][ids[0]])
    s, _, _, ids, c, _, _ = lib.case("moved_negated_radius")
    assert s["radius"][ids[0]] < 0
    _, _, _, _, c, _, _ = lib.case("same_centres_twice")
    assert c[1].tobytes() == c[2].tobytes() != c[0].tobytes()
    s, _, _, ids, c, _, _ = lib.case("own_centres_of_eight")
    assert len(ids) == 8 and all(c[j].tobytes() == lib.centres_of(s, ids, 1)[0].tobytes() for j in range(3))
    _, _, _, _, c, _, _ = lib.case("negative_zero")
    assert np.signbit(c[1:]).sum() >= 6 and (c[1:][np.signbit(c[1:])] == 0).sum() >= 6


# ---------------------------------------------------------------- 2. every frame has something to show
def object_planes_of(object_checker, name):
    s, m, views, ids, centres, _, _ = lib.case(name)
    w, h, _ = lib.META[name]["size"]
    cams = cameras_of(views, w, h)
    return [object_checker.plane(lib.scene_of(s, ids, centres, j), cams[j], w, h)[0] for j in range(len(views))]


@pytest.mark.parametrize("name", list(lib.CATALOGUE))
def test_every_frame_shows_a_moved_and_a_static_sphere(object_checker, name):
    s, m, views, ids, centres, _, _ = lib.case(name)
    meta = lib.META[name]
    w, h, _ = meta["size"]
    planes = object_planes_of(object_checker, name)
    for j, plane in enumerate(planes):
        moved = np.isin(plane, ids).mean()
        static = ((plane >= 0) & ~np.isin(plane, ids)).mean()
        assert moved >= 0.05, (name, j, moved)
        if j in meta["no_static"]:
            # why no static sphere can fill 5 % of this view: the camera is inside a moved sphere, which over 95 % of its rays hit first; or it
            # stands so far from every static sphere that their discs together (pi (r / d)^2 each, more than a sphere's share
            # of the image plane) stay below 5 % of the image plane's 4 tan^2(vfov / 2) w / h
            if "inside" in meta and meta["inside"][0] == j:
                assert (plane == meta["inside"][1]).mean() > 0.95, (name, j)
            else:
                sj = lib.scene_of(s, ids, centres, j)
                still = ~np.isin(np.arange(len(s)), ids)
                d2 = sum((sj[k][still].astype(np.float64) - float(views[j, a])) ** 2 for a, k in enumerate(("cx", "cy", "cz")))
                discs = (np.pi * sj["radius"][still].astype(np.float64) ** 2 / d2).sum()
                assert discs < 0.05 * 4.0 * np.tan(np.radians(float(views[j, 6])) / 2) ** 2 * w / h, (name, j, discs)
                assert d2.min() >= 1000.0 ** 2  # (beside a sphere 2^10 or more away)
        else:
            assert static >= 0.05, (name, j, static)
    if not (meta["family"] == "reach" and meta["reach_k"] >= 10):
        assert any(j not in meta["no_static"] for j in range(len(planes)))


# ---------------------------------------------------------------- 3. the host-compiled trace code
def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def rays_of_frame(cam, w, h, sj, ids, rng, aimed=500, surface=500):
    """the frame's camera rays; rays from the camera aimed at each moved sphere with a jitter of up to 1.2 radii; rays that start on
    each moved sphere's surface along a seeded direction of the outward hemisphere -> float32 [n, 6]"""
    o, d = centre_rays(cam, w, h)
    out = [np.concatenate([np.broadcast_to(o, (w * h, 3)), np.stack(d, axis=-1).reshape(-1, 3)], axis=1)]
    for i in ids:
        c = np.array([sj["cx"][i], sj["cy"][i], sj["cz"][i]], np.float64)
        r = abs(float(sj["radius"][i]))
        to = c - o.astype(np.float64)
        dist = max(np.linalg.norm(to), 1e-30)
        jitter = rng.normal(size=(aimed, 3)) * (0.6 * max(r, 0.05) / dist)
        da = unit(to / dist + jitter) if np.isfinite(dist) else unit(np.sign(to) + jitter)
        out.append(np.concatenate([np.broadcast_to(o, (aimed, 3)), da], axis=1))
        n = unit(rng.normal(size=(surface, 3)))
        ds = unit(rng.normal(size=(surface, 3)))
        ds = np.where((ds * n).sum(axis=1, keepdims=True) < 0, -ds, ds)
        with np.errstate(over="ignore"):
            origin = (c + n * r * (1.0 + 1e-4)).astype(f32)
        origin = np.where(np.isfinite(origin), origin, c.astype(f32))
        out.append(np.concatenate([origin, ds], axis=1))
        # and back through the sphere from beside it: the near root on the moved sphere
        out.append(np.concatenate([(c + n * (r + 2.0)).astype(f32), unit(-n + rng.normal(size=(surface, 3)) * 0.1)], axis=1))
    rays = np.ascontiguousarray(np.concatenate(out, axis=0), f32)
    rays[:, 3:] = unit(rays[:, 3:]).astype(f32)
    return rays[np.isfinite(rays).all(axis=1)]


def hit_moved(emu, staged, own, m, keyed, mask, table, rays):
    fn = emu.emu_hit_spheres_moved
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_ulonglong] + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 7
    n = len(rays)
    ids = [np.full(n, -7, np.int32) for _ in range(3)]
    ts = [np.full(n, -7, f32) for _ in range(3)]
    info = np.zeros(2, np.int32)
    staged, own, m = np.ascontiguousarray(staged), np.ascontiguousarray(own), np.ascontiguousarray(m)
    bad = fn(staged.ctypes.data, own.ctypes.data, m.ctypes.data, len(staged), keyed, mask, table.ctypes.data, rays.ctypes.data, n,
             ids[0].ctypes.data, ts[0].ctypes.data, ids[1].ctypes.data, ts[1].ctypes.data, ids[2].ctypes.data, ts[2].ctypes.data, info.ctypes.data)
    return bad, ids, ts, info


def key_table(ids, centres_j):
    """the launch-uniform mask (sphere i at bit 63 - i) and the frame's table: the centres in ascending sphere index"""
    mask, table = 0, np.zeros((8, 4), f32)
    for i in ids:
        mask |= 1 << (63 - int(i))
    for slot, k in enumerate(np.argsort(ids)):
        table[slot, :3] = centres_j[k]
    return mask, table


def check_frame(emu, staged, own, m, keyed, mask, table, rays, what):
    bad, ids, ts, info = hit_moved(emu, staged, own, m, keyed, mask, table, rays)
    assert np.array_equal(ids[0], ids[2]), (what, "two-phase", int((ids[0] != ids[2]).sum()))
    hit = ids[2] >= 0
    assert np.array_equal(ts[0].view(np.uint32)[hit], ts[2].view(np.uint32)[hit]), (what, "two-phase t")
    if info[0] >= 0:
        assert np.array_equal(ids[1], ids[2]), (what, "behind the matrix filter", int((ids[1] != ids[2]).sum()))
        assert np.array_equal(ts[1].view(np.uint32)[hit], ts[2].view(np.uint32)[hit]), (what, "behind the matrix filter: t")
    assert bad == 0, (what, "normals", bad)
    return ids[2], info


@pytest.mark.parametrize("name", list(lib.CATALOGUE))
def test_the_staged_filter_and_the_table_find_what_the_exact_loop_finds(emu, name):
    """frame j of a launch: the filter data of the launch's LAST frame, the mask, frame j's centres.  A call that goes frame by frame
    stages every frame's own scene and has no mask."""
    s, m, views, ids, centres, _, _ = lib.case(name)
    w, h, _ = lib.META[name]["size"]
    n = len(views)
    cams = cameras_of(views, w, h)
    rng = np.random.default_rng(sum(map(ord, name)))
    per_launch = 1 if name in lib.FALLBACKS else 32
    on_moved, with_table, dropped = 0, 0, 0
    for j in range(n):
        last = min(n - 1, (j // per_launch) * per_launch + per_launch - 1)
        own, staged = lib.scene_of(s, ids, centres, j), lib.scene_of(s, ids, centres, last)
        if per_launch == 1:
            mask, table = 0, np.zeros((8, 4), f32)
        else:
            mask, table = key_table(ids, centres[j])
        rays = rays_of_frame(cams[j], w, h, own, ids, rng, *((60, 60) if n > 3 else (500, 500)))
        want, info = check_frame(emu, staged, own, m, 1, mask, table, rays, (name, j))
        on_moved += int(np.isin(want, ids).sum())
        with_table += int(info[0] >= 0)
        if name == "seam_small_sphere_in_in_the_last" and j < last:
            # what the mask is for, behind the matrix table: rays whose nearest hit is the small sphere although the staged table's
            # filter, which knows the sphere at its last frame's place, does not keep it
            _, masks, _, _ = _matrix_masks(emu, staged, m, rays)
            kept = (masks >> np.uint64(63 - lib.SEAM_SMALL)) & np.uint64(1)
            dropped += int(((want == lib.SEAM_SMALL) & (kept == 0)).sum())
    assert on_moved >= 1000, (name, on_moved)
    if lib.META[name]["family"] == "table_seam":
        # hitSpheresCandidates ran behind the staged table in exactly the frames whose launch stages a scene that has one
        table = lib.META[name]["table"]
        assert with_table == sum(table[min(n - 1, (j // 32) * 32 + 31)] for j in range(n)), (name, with_table)
    if name == "seam_small_sphere_in_in_the_last":
        assert dropped >= 500, dropped


# ---------------------------------------------------------------- 4. the three time-driven calls
def animated(s, t):
    a = s.copy()
    Oracle.get().animate(a, float(t))
    return a


def test_the_times_cover_zero_pi_denormal_and_flt_max():
    got = lib.timed("timed_every_time")[2]
    assert got[:2] == [0.0, -0.0] and np.signbit(got[1]) and got[2] == float(f32(np.pi)) and got[3:] == [1e-40, -2.5, 100.0, 1e6, 1e30, 3.4e38]
    t = lib.timed("timed_equal_times")[2]
    assert len(t) == 3 and len(set(t)) == 1


def test_the_timed_cases_are_what_their_names_say(oracle):
    s, m, times, views, flags, _ = lib.timed("timed_lights")
    assert (m["emissive"][1] > 0).any() and not (m["emissive"][8] > 0).any() and flags & lib.FLAG_ANIMATE
    # glass around the camera at one time only
    s, m, times, views, _, _ = lib.timed("timed_glass_around_the_camera")
    assert m["type"][1] == lib.DIELECTRIC
    inside = []
    for j, t in enumerate(times):
        a = animated(s, t)
        d2 = sum((float(views[j, k]) - float(a[n][1])) ** 2 for k, n in enumerate(("cx", "cy", "cz")))
        inside.append(d2 < 0.9 * 0.25 if j == 1 else d2 < 0.25)
    assert inside == [False, True, False]
    # the ties: coincident at the searched time only, the lower index in view there
    for name, lower, higher, at in (("timed_tie_on_a_higher_static", 1, 9, 1), ("timed_tie_on_a_lower_static", 3, 8, None)):
        s, m, times, views, _, _ = lib.timed(name)
        w, h, _ = lib.SIZE
        cams = cameras_of(views, w, h)
        same = []
        for j, t in enumerate(times):
            a = animated(s, t)
            same.append(all(a[k][lower] == a[k][higher] for k in ("cx", "cy", "cz", "radius")))
            if same[-1]:
                got = oracle_first_hits(oracle, a, cams[j], w, h)
                assert (got == lower).sum() >= 200 and (got == higher).sum() == 0, (name, j)
        assert same == ([False, True, False] if at == 1 else [False, True, True]), (name, same)


def timed_seam_x(emu):
    """sphere 1 (r = 30) at (x, cos t + 1, 104.4): the last x with a table at t = 0 (y = 2) and the first without"""
    def has_table(x):
        s, m = lib.timed_seam(x)[:2]
        return matrix_r1(emu, animated(s, 0.0), m) >= 0
    return bisect_floats(lib.TIMED_SEAM_XZ[0] - 2.0, lib.TIMED_SEAM_XZ[0] + 2.0, has_table)


def test_the_time_decides_the_side_of_the_seam(emu, object_checker):
    """at the first x without a table at t = 0 (y = 2), the scene has one at t = pi (y = 0): the clip's times alternate"""
    _, x = timed_seam_x(emu)
    s, m, times, views, _, _ = lib.timed_seam(x)
    got = [matrix_r1(emu, animated(s, t), m) >= 0 for t in times]
    assert got == [True, False, True], got
    w, h, _ = lib.SIZE
    cams = cameras_of(views, w, h)
    for j, t in enumerate(times):
        plane = object_checker.plane(animated(s, t), cams[j], w, h)[0]
        assert (plane == 1).mean() >= 0.05 and ((plane >= 0) & (plane != 1) & (plane != 8)).mean() >= 0.05, (j, (plane == 1).mean())


@pytest.mark.parametrize("name", list(lib.TIMED) + ["timed_seam"])
def test_the_animation_kernels_hits_equal_the_exact_loop(emu, name):
    """movedSphere: the staged scene of a launch is the scene at its last time, spheres 1 and 8 come from the frame's two centres"""
    s, m, times, views, _, _ = lib.timed_seam(timed_seam_x(emu)[1]) if name == "timed_seam" else lib.timed(name)
    w, h, _ = lib.SIZE
    cams = cameras_of(views, w, h)
    rng = np.random.default_rng(sum(map(ord, name)))
    staged = animated(s, times[-1])
    on_moved = 0
    for j, t in enumerate(times):
        own = animated(s, t)
        table = np.zeros((8, 4), f32)
        for slot, i in enumerate((1, 8)):
            table[slot, :3] = (own["cx"][i], own["cy"][i], own["cz"][i])
        want, _ = check_frame(emu, staged, own, m, 0, 0, table, rays_of_frame(cams[j], w, h, own, [1, 8], rng, 300, 300), (name, j))
        on_moved += int(np.isin(want, (1, 8)).sum())
    assert on_moved >= 1000, (name, on_moved)


# ---------------------------------------------------------------- 5. the host's routing, on the emulated runtime
ROUTING = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from toypathtracer_amd import api as tpt
import motion_kinds_lib as lib
lib.set_table_seam(%r, %r)
so = C.CDLL(tpt.library_path())
so.hostemuObjectPlaneConsts.restype = C.POINTER(C.c_float * 18)
so.hostemuObjectPlaneConsts.argtypes = [C.c_int]
so.hostemuObjectPlaneOut.restype = C.c_void_p
tpt.InitializeTest()
for name in ("reach_2^20_mid", "reach_2^20_last", "seam_33_frames"):
    s, m, views, ids, centres, flags, first = lib.case(name)
    w, h, spp = lib.META[name]["size"]
    n = len(views)
    tpt.set_scene(s, m)
    tpt.set_samples_per_pixel(spp)
    tpt.UpdateTest(0.0, first, w, h, flags)
    tile, mo = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    objs = np.full((n, h, w), -9, np.int32)
    before = so.hostemuObjectPlaneLaunches()
    tpt.kernel_timing_begin(2 * n)
    cams = tpt.draw_device_keyframe_clip(views, ids, centres, first, w, h, tile.ctypes.data, mo.ctypes.data, flags, objects_ptr=objs.ctypes.data)
    ms, launches = tpt.kernel_timing_end()
    tpt.synchronize()
    assert launches == lib.META[name]["launches"] == (n + 31) // 32, (name, launches)
    assert so.hostemuObjectPlaneLaunches() == before + n, name
    got = tpt.GetSceneDesc()[0]
    want = lib.scene_of(s, ids, centres, n - 1)
    for k in ("cx", "cy", "cz", "radius"):
        assert got[k].tobytes() == want[k].tobytes(), (name, "the context's spheres are not S_{n-1}", k)
    cams = np.ascontiguousarray(cams).view(np.uint8).reshape(n, 88)
    for j in range(max(0, n - 8), n):  # (the emulated launcher keeps its last eight launches)
        k = np.array(so.hostemuObjectPlaneConsts(before + j).contents, np.float32)
        assert k[:12].tobytes() == cams[j, :48].tobytes(), (name, j, "the object plane is not traced through the frame's camera")
        own = lib.scene_of(s, ids, centres, j)
        assert k[12:15].tobytes() == np.float32([own["cx"][1], own["cy"][1], own["cz"][1]]).tobytes(), (name, j, "sphere 1's centre")
        assert name != "seam_33_frames" or (1 in ids and centres[j, list(ids).index(1)].tobytes() != centres[j - 1, list(ids).index(1)].tobytes())
        assert so.hostemuObjectPlaneSpheres(before + j) == len(s) and so.hostemuObjectPlaneOut(before + j) == objs.ctypes.data + 4 * w * h * j
    print("routed:", name, launches)
tpt.ShutdownTest()
print("ok")
'''


def test_host_routing_on_the_emulated_runtime(seam):
    """a far clip (the far frame in the middle, then last) and the 33-frame seam clip: the trace launches, the context's spheres
    afterwards, and every object-plane launch with its own frame's camera and centres"""
    out = run_refusals(ROUTING % (float(seam[0]), float(seam[1])), "libtpt_hostemu_objects.so", ["hostemu_objects.cpp"])
    assert out.count("routed:") == 3, out
