"""tptDrawDeviceAnimation: frames of an animated scene (kFlagAnimate, Test.cpp:304-308) traced up to 32 per launch -- every frame image,
every frame's ray count and the final tile held byte for byte against the oracle, and against the tptUpdate / tptDrawDevice sequence the
call replaces, in every configuration the call serves with one launch per batch and in those it serves frame by frame."""
import numpy as np
import pytest

from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE, SEED_PER_PIXEL

pytestmark = pytest.mark.gpu

ANIMATED = FLAG_PROGRESSIVE | FLAG_ANIMATE


def irregular_times(n, seed=5):
    """a clip's times: increasing, irregular steps, a repeated time and a jump back"""
    rng = np.random.default_rng(seed)
    t = np.cumsum(rng.uniform(0.0, 0.4, n)).astype(np.float32) - np.float32(1.0)
    if n > 6:
        t[5] = t[4]
        t[n // 2] = -2.5
    return [float(v) for v in t]


def draw_animation(tpt, w, h, times, first=0, flags=ANIMATED):
    """one tptDrawDeviceAnimation call -> (tile, frame images [n, h, w, 4], per-frame rays), all on the device except the rays"""
    import torch
    n = len(times)
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    images = torch.full((n, h, w, 4), -3.0, dtype=torch.float32, device="cuda")
    rays = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    tpt.UpdateTest(times[0], first, w, h, flags)  # (the call refuses a size no tptUpdate has seen)
    r0 = tpt.ray_counter_read()
    tpt.draw_device_animation(times, first, w, h, tile.data_ptr(), flags, images.data_ptr(), rays.data_ptr())
    r1 = tpt.ray_counter_read()
    per = rays.cpu().tolist()
    assert r1 - r0 == sum(per), (r1 - r0, sum(per))
    return tile, images, per


def draw_sequence(tpt, w, h, times, first=0, flags=ANIMATED):
    """the same frames as tptUpdate + tptDrawDevice per frame, the tile read after each"""
    import torch
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    images, per = [], []
    for j, t in enumerate(times):
        tpt.UpdateTest(t, first + j, w, h, flags)
        r0 = tpt.ray_counter_read()
        tpt.draw_device(t, first + j, w, h, tile.data_ptr(), flags)
        per.append(tpt.ray_counter_read() - r0)  # (synchronises: the tile holds frame j)
        images.append(tile.clone())
    torch.cuda.synchronize()
    return tile, torch.stack(images), per


def same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def assert_same_as_sequence(tpt, w, h, times, first=0, flags=ANIMATED):
    ta, ia, pa = draw_animation(tpt, w, h, times, first, flags)
    tb, ib, pb = draw_sequence(tpt, w, h, times, first, flags)
    assert pa == pb
    for j in range(len(times)):
        assert same(ia[j], ib[j]), "frame %d differs from the tptUpdate + tptDrawDevice sequence" % j
    assert same(ta, tb)


def test_forty_frames_equal_the_oracle(tpt_defaults, oracle):
    """96x64x4, 40 irregular times, animated + progressive: two launches, every frame image, ray count and the tile against the oracle"""
    tpt = tpt_defaults
    w, h, n = 96, 64, 40
    times = irregular_times(n)
    tile, images, per = draw_animation(tpt, w, h, times)
    spheres, mats = oracle.default_scene()
    cam = oracle.default_camera(w, h)
    bo = np.zeros((h, w, 4), np.float32)
    got = images.cpu().numpy()
    for f, t in enumerate(times):
        oracle.animate(spheres, t)
        r, _ = oracle.render(spheres, mats, cam, w, h, 4, f, ANIMATED, backbuffer=bo, seed_mode=SEED_PER_PIXEL)
        assert per[f] == r, (f, per[f], r)
        assert got[f].tobytes() == bo.tobytes(), "frame %d differs from the oracle" % f
    assert tile.cpu().numpy().tobytes() == bo.tobytes()
    info = tpt.launch_info()
    assert info["blocks_per_cu"] == 2, info  # (the centres take the LDS of the path records the kernel gives up)


@pytest.mark.parametrize("n", [8, 32])
def test_full_size_equals_the_sequence(tpt_defaults, n):
    tpt = tpt_defaults
    assert_same_as_sequence(tpt, 1280, 720, [0.02 * k for k in range(n)], first=3)


def test_three_launches_ragged_size(tpt_defaults):
    tpt = tpt_defaults
    assert_same_as_sequence(tpt, 203, 117, irregular_times(70, seed=11), first=1)


def flat_scene():
    """200 spheres, flat (under 256): no matrix-core table, the packed VALU filter; spheres 1-4 are lights (sphere 1 moves, 8 not a light)"""
    from toypathtracer_amd.scenes import stress_scene
    return stress_scene(200, 16)


def test_flat_scene_of_200_spheres(tpt_defaults):
    from toypathtracer_amd.scenes import STRESS_CAMERA
    tpt = tpt_defaults
    s, m = flat_scene()
    tpt.set_scene(s, m)
    c = STRESS_CAMERA
    tpt.set_camera(c["look_from"], c["look_at"], c["vfov"], c["aperture"], c["focus_dist"])
    tpt.UpdateTest(0.0, 0, 160, 96, ANIMATED)
    info = tpt.scene_info()
    assert info["spheres"] == 200 and info["groups"] == 0, info
    assert_same_as_sequence(tpt, 160, 96, irregular_times(40, seed=3))
    tpt.set_camera(None)
    tpt.set_scene(None)


def test_sphere_one_emissive_sphere_eight_not(tpt_defaults, oracle):
    """the light list: a moving light (sphere 1) and a moving sphere that is not one (sphere 8)"""
    tpt = tpt_defaults
    s, m = oracle.default_scene()
    m[1]["emissive"] = (4.0, 3.0, 2.0)
    m[8]["emissive"] = (0.0, 0.0, 0.0)
    tpt.set_scene(s, m)
    assert_same_as_sequence(tpt, 128, 80, irregular_times(36, seed=8))
    tpt.set_scene(None)


@pytest.mark.parametrize("light_sampling,smoothing,mitsuba", [(True, 0.9, True), (False, 0.9, False), (True, 0.5, False)],
                         ids=["mitsuba", "no-light-sampling", "smoothing-0.5"])
def test_configurations(tpt_defaults, light_sampling, smoothing, mitsuba):
    tpt = tpt_defaults
    tpt.set_config(light_sampling, smoothing, mitsuba)
    assert_same_as_sequence(tpt, 128, 72, irregular_times(34, seed=4))
    tpt.set_config()


@pytest.mark.parametrize("scene", ["default", "flat"])
def test_one_trace_launch_per_32_frames(tpt_defaults, scene):
    import torch
    tpt = tpt_defaults
    if scene == "flat":
        s, m = flat_scene()
        tpt.set_scene(s, m)
    w, h = 64, 40
    for n in (1, 32, 33, 70):
        tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        tpt.UpdateTest(0.0, 0, w, h, ANIMATED)
        tpt.kernel_timing_begin(16)
        tpt.draw_device_animation([0.1 * k for k in range(n)], 0, w, h, tile.data_ptr(), ANIMATED)
        ms, launches = tpt.kernel_timing_end()
        assert launches == (n + 31) // 32 and ms > 0.0, (n, launches)
    tpt.set_scene(None)


@pytest.mark.parametrize("case", ["row-serial", "forward-fold", "lane-refill", "grouped"])
def test_configurations_served_frame_by_frame(tpt_defaults, case):
    tpt = tpt_defaults
    w, h = 64, 40
    n = 12
    if case == "row-serial":
        tpt.set_seed_mode(0)
    elif case == "forward-fold":
        tpt.set_fold_mode(1)
    elif case == "lane-refill":
        tpt.set_kernel_variant(1, 1, -1)
    else:
        from toypathtracer_amd.scenes import stress_scene
        s, m = stress_scene(4096, 64)
        tpt.set_scene(s, m)
        n = 5
    times = irregular_times(n, seed=9)
    assert_same_as_sequence(tpt, w, h, times)
    import torch
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tpt.UpdateTest(times[0], 0, w, h, ANIMATED)
    tpt.kernel_timing_begin(16)
    tpt.draw_device_animation(times, 0, w, h, tile.data_ptr(), ANIMATED)
    _, launches = tpt.kernel_timing_end()
    assert launches == n
    tpt.set_scene(None)


def test_without_animate_it_is_the_batch(tpt_defaults):
    """kFlagAnimate off: nothing moves, the frames are tptDrawDeviceBatch's (and the sequence's)"""
    import torch
    tpt = tpt_defaults
    w, h, n = 160, 90, 40
    times = irregular_times(n)
    ta, ia, pa = draw_animation(tpt, w, h, times, first=2, flags=FLAG_PROGRESSIVE)
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tpt.UpdateTest(times[0], 2, w, h, FLAG_PROGRESSIVE)
    r0 = tpt.ray_counter_read()
    tpt.draw_device_batch(times[0], 2, n, w, h, tile.data_ptr(), FLAG_PROGRESSIVE)
    rb = tpt.ray_counter_read() - r0
    assert same(ta, tile) and sum(pa) == rb
    tb, ib, pb = draw_sequence(tpt, w, h, times, first=2, flags=FLAG_PROGRESSIVE)
    assert pa == pb and same(ia, ib) and same(ta, tb)


def test_eight_spheres_do_not_move(tpt_defaults, oracle):
    """the tptUpdate guard (Test.cpp:304): a scene of 8 spheres is static even with kFlagAnimate"""
    tpt = tpt_defaults
    s, m = oracle.default_scene()
    tpt.set_scene(s[:8].copy(), m[:8].copy())
    assert_same_as_sequence(tpt, 96, 64, irregular_times(10))
    tpt.set_scene(None)


@pytest.mark.parametrize("update", [False, True], ids=["draw-only", "update-and-draw"])
def test_the_context_afterwards(tpt_defaults, oracle, update):
    """spheres 1 and 8 at the last time (tptGetSceneDesc), and the next tptDrawDevice -- with or without tptUpdate -- continues the
    sequence exactly"""
    import torch
    tpt = tpt_defaults
    w, h, n = 128, 72, 37
    times = irregular_times(n, seed=2)
    nxt = times[-1] + 0.3
    ta, _, _ = draw_animation(tpt, w, h, times)
    s, _, _, _ = tpt.GetSceneDesc()
    want, _ = oracle.default_scene()
    oracle.animate(want, times[-1])
    for i in (1, 8):
        assert [s[i][k] for k in ("cx", "cy", "cz", "radius")] == [want[i][k] for k in ("cx", "cy", "cz", "radius")], i
    if update:
        tpt.UpdateTest(nxt, n, w, h, ANIMATED)
    tpt.draw_device(nxt, n, w, h, ta.data_ptr(), ANIMATED)
    tb, _, _ = draw_sequence(tpt, w, h, times)
    if update:
        tpt.UpdateTest(nxt, n, w, h, ANIMATED)
    tpt.draw_device(nxt, n, w, h, tb.data_ptr(), ANIMATED)
    tpt.synchronize()
    torch.cuda.synchronize()
    assert same(ta, tb)


def test_null_outputs_and_counter(tpt_defaults):
    """without the optional outputs the tile and the running counter are the same"""
    import torch
    tpt = tpt_defaults
    w, h, times = 96, 64, irregular_times(20, seed=6)
    ta, _, pa = draw_animation(tpt, w, h, times)
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tpt.UpdateTest(times[0], 0, w, h, ANIMATED)
    r0 = tpt.ray_counter_read()
    tpt.draw_device_animation(times, 0, w, h, tile.data_ptr(), ANIMATED)
    assert tpt.ray_counter_read() - r0 == sum(pa)
    assert same(ta, tile)


@pytest.mark.parametrize("hit_spheres", [0, 3], ids=["matrix-filter", "valu-filter"])
def test_small_moving_spheres(tpt_defaults, oracle, hit_spheres):
    """spheres 1 and 8 of radius 0.05 and 0.02 that move up to ~40 radii over a batch: the filter's data of the batch's staged scene
    says nothing about them in the other frames -- they are candidates of every ray -- and every frame still equals the sequence"""
    tpt = tpt_defaults
    s, m = oracle.default_scene()
    s[1]["radius"], s[8]["radius"] = 0.05, 0.02
    s["invRadius"] = np.float32(1.0) / s["radius"]
    tpt.set_scene(s, m)
    tpt.set_kernel_variant(hit_spheres, 3, -1)
    assert_same_as_sequence(tpt, 160, 96, [float(t) for t in np.float32(np.linspace(0.0, 6.3, 40))])
    tpt.set_kernel_variant(0, 3, -1)
    tpt.set_scene(None)


def test_non_finite_times(tpt_defaults):
    """an infinite or NaN time (cosf / sinf give NaN: the sphere vanishes from that frame) touches its own frame only"""
    tpt = tpt_defaults
    times = irregular_times(12, seed=7)
    times[3], times[8] = float("inf"), float("nan")
    assert_same_as_sequence(tpt, 96, 64, times)
