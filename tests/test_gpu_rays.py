"""tptTraceRaysDevice on the GPU, held byte for byte against its C statement (tests/rays_checker.c: the oracle's Trace, TraceForward and
HitSpheres): the ray counts around a lane group, a chunk and a wave's refills; the ray catalogue of tests/rays_lib.py on the built-in
scene (staged in LDS, flat) and on a grouped scene (global memory, the grouped traversal), both HitSpheres variants, both folds, light
sampling on and off; radiance only, hits only and both; the counter word; guard rows around every output.  The radiance of a frame's
own camera rays is tptDrawDevice's colour at 1 spp, and a draw after the call still equals its golden.  Finite rays only."""
import numpy as np
import pytest

from common import case_id, per_pixel_goldens
from oracle_lib import FOLD_FORWARD, FOLD_RECURSIVE, fnv1a
from rays_lib import SCENES, RaysChecker, all_rays, catalogue, scene_camera

pytestmark = pytest.mark.gpu
COUNTS = [1, 63, 64, 65, 255, 256, 257, 5000]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return RaysChecker(tmp_path_factory.mktemp("rays_checker"))


@pytest.fixture(scope="module")
def cases(checker):
    """per scene: (spheres, materials, the catalogue as one buffer, where each entry lies); made once, left as they are"""
    out = {}
    for name, make in SCENES.items():
        s, m = make()
        rays, where = all_rays(catalogue(checker, s, scene_camera(name, 40, 25)))
        out[name] = (s, m, rays, where)
    return out


@pytest.fixture(scope="module")
def frame_rays(checker, oracle):
    """camera_rays of a 100 x 50 frame of the built-in scene (5000 rays), and the checker on them"""
    from rays_lib import default_scene
    s, m = default_scene()
    rays = checker.camera_rays(oracle.default_camera(100, 50), 100, 50)
    return s, m, rays, checker.trace(s, m, rays)


def trace(tpt, rays, radiance=True, hits=True, counted=True):
    """the call with a guard row of NaN before and after each output and a guard word either side of the counter -> host arrays"""
    import torch
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
    rad = torch.full((n + 2, 4), float("nan"), dtype=torch.float32, device="cuda") if radiance else None
    hit = torch.full((n + 2, 8), float("nan"), dtype=torch.float32, device="cuda") if hits else None
    cnt = torch.tensor([5, 1000, 5], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    tpt.trace_rays_device(n, d_rays.data_ptr(), rad.data_ptr() + 16 if radiance else None, hit.data_ptr() + 32 if hits else None,
                          cnt.data_ptr() + 8 if counted else None)
    tpt.synchronize()
    assert d_rays.cpu().numpy().tobytes() == np.ascontiguousarray(rays).tobytes(), "the call wrote its input"
    return (rad.cpu().numpy() if radiance else None, hit.cpu().numpy() if hits else None, cnt.cpu().numpy().tolist(), counted)


def check(got, want, what):
    rad, hit, cnt, counted = got
    total, wrad, whit = want
    for g, w, name in ((rad, wrad, "radiance"), (hit, whit, "hits")):
        if g is None:
            continue
        assert np.isnan(g[0]).all() and np.isnan(g[-1]).all(), (what, name, "a guard row was written")
        if g[1:-1].tobytes() != w.tobytes():
            bad = np.argwhere(g[1:-1].view(np.uint32) != w.view(np.uint32))
            raise AssertionError("%s: %s: %d words differ, first at %s: %r / %r" % (what, name, len(bad), bad[0], g[1:-1][bad[0][0]], w[bad[0][0]]))
    assert cnt == [5, 1000 + (total if counted else 0), 5], (what, cnt, total)


@pytest.mark.parametrize("n", COUNTS)
def test_ray_counts(tpt_defaults, frame_rays, checker, n):
    """1 ray; fewer rays than lanes; a partial last chunk of 64 and of 256; 5000: several refills per wave"""
    tpt = tpt_defaults
    s, m, rays, full = frame_rays
    tpt.UpdateTest(0.0, 0, 100, 50, 0)
    r = np.ascontiguousarray(rays[:n])
    want = full if n == len(rays) else checker.trace(s, m, r)
    r0 = tpt.ray_counter_read()
    check(trace(tpt, r), want, "n = %d" % n)
    assert tpt.ray_counter_read() == r0, "the context's ray counter moved"


@pytest.mark.parametrize("fold", [FOLD_RECURSIVE, FOLD_FORWARD], ids=["recursive", "forward"])
@pytest.mark.parametrize("hs", [0, 1], ids=["two_phase", "simple"])
@pytest.mark.parametrize("scene", ["default", "grouped"])
def test_catalogue_equals_the_checker(tpt_defaults, cases, checker, scene, hs, fold):
    tpt = tpt_defaults
    s, m, rays, where = cases[scene]
    if scene != "default":
        tpt.set_scene(s, m)
    tpt.set_kernel_variant(hs, 3, -1)
    tpt.set_fold_mode(fold)
    tpt.UpdateTest(0.0, 0, 40, 25, 0)
    assert (tpt.scene_info()["groups"] > 0) == (scene == "grouped")
    both = checker.trace(s, m, rays, fold=fold)
    check(trace(tpt, rays), both, "both")
    check(trace(tpt, rays, hits=False, counted=False), (both[0], both[1], None), "radiance only")
    got = trace(tpt, rays, radiance=False)
    check(got, (len(rays), None, both[2]), "hits only")  # k = 1 for every ray: the counter word gains the ray count
    ids = both[2][:, 7].view(np.int32)
    assert (ids[where["sky"]] == -1).all() and (ids[where["inside"]] >= 0).all() and (both[1][:, 3] >= 1).all()
    # light sampling off: other paths, other counts
    tpt.set_config(light_sampling=False)
    off = checker.trace(s, m, rays, fold=fold, light_sampling=False)
    assert off[0] < both[0] and off[2].tobytes() == both[2].tobytes()
    check(trace(tpt, rays), off, "no light sampling")


@pytest.mark.parametrize("fold", [FOLD_RECURSIVE, FOLD_FORWARD], ids=["recursive", "forward"])
def test_camera_rays_give_the_draw(tpt_defaults, checker, fold):
    """the radiance along a frame's own first-sample rays is the colour plane tptDrawDevice writes at 1 spp, frame 0, into a zeroed
    tile (alpha apart: the tile's is kept, the radiance's is the path's ray count), and the ray counts agree"""
    import torch
    tpt = tpt_defaults
    w, h = 40, 25
    tpt.set_samples_per_pixel(1)
    tpt.set_fold_mode(fold)
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r0 = tpt.ray_counter_read()
    tpt.UpdateTest(0.0, 0, w, h, 0)
    tpt.draw_device(0.0, 0, w, h, tile.data_ptr(), 0)
    tpt.synchronize()
    drawn = tpt.ray_counter_read() - r0
    cam = tpt.GetSceneDesc()[2]
    rad, _, cnt, _ = trace(tpt, checker.camera_rays(cam, w, h, 0), hits=False)
    img = tile.cpu().numpy()
    assert rad[1:-1].reshape(h, w, 4)[..., :3].tobytes() == img[..., :3].tobytes()
    assert (img[..., 3] == 0).all() and cnt[1] - 1000 == drawn == int(rad[1:-1, 3].sum())


def test_a_draw_after_the_call_equals_its_golden(tpt_defaults, frame_rays):
    tpt = tpt_defaults
    s, m, rays, full = frame_rays
    case = min(per_pixel_goldens(), key=lambda c: c["width"] * c["height"] * c["spp"] * c["frames"])
    tpt.UpdateTest(0.0, 0, 100, 50, 0)
    check(trace(tpt, rays), full, "before the draw")
    tpt.set_samples_per_pixel(case["spp"])
    bb = np.zeros((case["height"], case["width"], 4), np.float32)
    total = 0
    for f in range(case["frames"]):
        tpt.UpdateTest(case["time"], f, case["width"], case["height"], case["flags"])
        total += tpt.DrawTest(case["time"], f, case["width"], case["height"], bb, case["flags"])
    assert total == case["rays"] and "%08x" % fnv1a(bb) == case["fnv"], case_id(case)
    tpt.UpdateTest(0.0, 0, 100, 50, 0)
    check(trace(tpt, rays), full, "after the draw")
