"""tests/rays_checker.c, the CPU reference of tptTraceRaysDevice, held against the oracle it is made of: on the rays a frame's first
samples start with it is tpto_render at 1 spp with per-pixel seeds, byte for byte and ray for ray; its hit records are
tpto_hit_spheres'; a seed word of 0 behaves as 1.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from oracle_lib import FOLD_FORWARD, FOLD_RECURSIVE, Oracle
from rays_lib import RaysChecker, all_rays, catalogue, default_scene, grouped_scene, scene_camera

W, H = 48, 30


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return RaysChecker(tmp_path_factory.mktemp("rays_checker"))


@pytest.mark.parametrize("light_sampling", [True, False], ids=["lights", "no-light-sampling"])
@pytest.mark.parametrize("fold", [FOLD_RECURSIVE, FOLD_FORWARD], ids=["recursive", "forward"])
@pytest.mark.parametrize("frame", [0, 3])
def test_camera_rays_give_the_render(checker, fold, light_sampling, frame):
    s, m = default_scene()
    cam = scene_camera("default", W, H)
    rays = checker.camera_rays(cam, W, H, frame)
    assert np.isfinite(rays[:, [0, 1, 2, 4, 5, 6]]).all() and (rays[:, 3].view(np.uint32) != 0).all() and (rays[:, 7] == 0).all()
    total, rad, _ = checker.trace(s, m, rays, hits=False, fold=fold, light_sampling=light_sampling)
    want_rays, bb = checker.render(s, m, cam, W, H, frame, fold=fold, light_sampling=light_sampling)
    # (a zeroed buffer and lerp 0: the frame's colour is prev * 0 + col * 1, the bytes of 0.0f + col)
    assert rad.reshape(H, W, 4)[..., :3].tobytes() == bb[..., :3].tobytes()
    assert total == want_rays and int(rad[:, 3].astype(np.int64).sum()) == want_rays
    assert (rad[:, 3] >= 1).all() and (rad[:, 3] == np.floor(rad[:, 3])).all()
    # ... and the shared oracle library renders the same frame
    o_rays, o_bb = Oracle.get().render(s, m, cam, W, H, 1, frame, 0, seed_mode=1, fold_mode=fold, light_sampling=light_sampling)
    assert o_rays == want_rays and o_bb.tobytes() == bb.tobytes()


@pytest.mark.parametrize("scene", ["default", "grouped"])
def test_hit_records_are_hit_spheres(checker, scene):
    s, m = default_scene() if scene == "default" else grouped_scene()
    cam = scene_camera(scene, 40, 25)
    rays, where = all_rays(catalogue(checker, s, cam))
    total, rad, hits = checker.trace(s, m, rays, radiance=False)
    assert rad is None and total == len(rays)  # hits only: k = 1 for every ray
    lib = Oracle.get().lib
    n_hit = 0
    for i, r in enumerate(rays):
        t, pos, nrm = C.c_float(), np.zeros(3, np.float32), np.zeros(3, np.float32)
        o, d = np.ascontiguousarray(r[0:3]), np.ascontiguousarray(r[4:7])
        rid = lib.tpto_hit_spheres(s.ctypes.data, len(s), o.ctypes.data, d.ctypes.data, 0.001, 1e7, C.byref(t), pos.ctypes.data, nrm.ctypes.data)
        want = np.zeros(8, np.float32)
        want[7:8].view(np.int32)[0] = rid
        if rid >= 0:
            want[0:3], want[3], want[4:7] = pos, t.value, nrm
            n_hit += 1
        assert hits[i].tobytes() == want.tobytes(), (i, hits[i], want)
    # the catalogue does what it says: hits and misses both, the sky rays all miss, the rays from inside all hit
    assert 0 < n_hit < len(rays)
    assert (hits[where["sky"], 7].view(np.int32) == -1).all() and (hits[where["inside"], 7].view(np.int32) >= 0).all()
    ids = hits[where["tangent"], 7].view(np.int32)
    assert (ids >= 0).any() and len(set(ids.tolist())) > 1


def test_a_zero_seed_word_is_one(checker):
    s, m = default_scene()
    rays = checker.camera_rays(scene_camera("default", 16, 10), 16, 10)
    zero, one = rays.copy(), rays.copy()
    zero[:, 3].view(np.uint32)[:] = 0
    one[:, 3].view(np.uint32)[:] = 1
    a, b = checker.trace(s, m, zero), checker.trace(s, m, one)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    # (and the seed matters: the frame's own seeds give other paths)
    assert checker.trace(s, m, rays)[1].tobytes() != a[1].tobytes()


def test_radiance_and_hits_together_are_each_alone(checker):
    s, m = grouped_scene()
    rays, _ = all_rays(catalogue(checker, s, scene_camera("grouped", 40, 25)))
    total, rad, hits = checker.trace(s, m, rays)
    t1, rad1, none = checker.trace(s, m, rays, hits=False)
    t2, none2, hits2 = checker.trace(s, m, rays, radiance=False)
    assert none is None and none2 is None
    assert rad.tobytes() == rad1.tobytes() and hits.tobytes() == hits2.tobytes() and total == t1 and t2 == len(rays)
    assert np.isfinite(rad).all() and not np.signbit(rad[:, :3][rad[:, :3] == 0]).any()
