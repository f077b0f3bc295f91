"""tptDrawDeviceBatchMoments on the GPU, byte for byte and ray for ray: against the sequence include/tpt_hip.h states -- frame-by-frame
tptDrawDeviceMoments with the guide blends done on the host in numpy float32 (tests/batch_moments_lib.py) --, against the independent CPU
statement over tests/moments_checker.c, and against tptDrawDeviceBatch for the tile; across the launch seams (32 | 1, 32 | 32 | 1), first
frames, flags, initial contents and calls that continue one another; at sizes of one pixel, one pixel past a wave and one pixel past a
pass of the fold's grid; with either or both guide planes left out; on the scenes that go frame by frame; refusals that write nothing;
and the planes as the input of tptDenoiseDeviceVariance.  No tolerance anywhere."""
import os
import re

import numpy as np
import pytest

from batch_moments_lib import blend, cpu_statement, lerp_factor
from moments_lib import MomentsChecker
from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE, ROOT

pytestmark = pytest.mark.gpu

W, H = 44, 20  # 880 pixels: neither dimension a multiple of 8, not a multiple of 256
COUNTS = (1, 3, 33, 65)  # one launch, and the seams 32 | 1 and 32 | 32 | 1
NAMES = ("tile", "moments", "albedo", "normal_depth")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return MomentsChecker(tmp_path_factory.mktemp("moments_checker"))


def initial(w, h, kind):
    """the four planes before the first call: zeroed, or finite and non-zero (each plane its own numbers, .w included)"""
    if kind == "zeroed":
        return [np.zeros((h, w, 4), np.float32) for _ in range(4)]
    rng = np.random.default_rng(5)
    return [(rng.random((h, w, 4), dtype=np.float32) * np.float32(3) - np.float32(0.75) + np.float32(k)) for k in range(4)]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def call(tpt, w, h, first, counts, flags, start, guides=(True, True)):
    """the new call, once per entry of `counts` (consecutive frames) -> (the four planes as host arrays, a left-out guide as it
    started; the ray counter's advance)"""
    import torch
    planes = [dev(p) for p in start]
    torch.cuda.synchronize()
    tpt.UpdateTest(0.0, first, w, h, flags)
    before = tpt.ray_counter_read()
    at = first
    for n in counts:
        tpt.draw_device_batch_moments(0.0, at, n, w, h, planes[0].data_ptr(), planes[1].data_ptr(), flags,
                                      albedo_ptr=planes[2].data_ptr() if guides[0] else None,
                                      normal_depth_ptr=planes[3].data_ptr() if guides[1] else None)
        at += n
    tpt.synchronize()
    return [p.cpu().numpy() for p in planes], tpt.ray_counter_read() - before


def sequence(tpt, w, h, first, n, flags, start, guides=(True, True), snapshots=()):
    """the statement: tptDrawDeviceMoments frame by frame into scratch guide planes, the guides blended on the host -> {frames: (planes,
    rays)} after each count of `snapshots` and after n"""
    import torch
    tile, mo = dev(start[0]), dev(start[1])
    alb, nd = start[2].copy(), start[3].copy()
    a_j, nd_j = (torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    tpt.UpdateTest(0.0, first, w, h, flags)
    before = tpt.ray_counter_read()
    out = {}
    for j in range(n):
        tpt.draw_device_moments(0.0, first + j, w, h, tile.data_ptr(), mo.data_ptr(), flags, albedo_ptr=a_j.data_ptr(),
                                normal_depth_ptr=nd_j.data_ptr())
        tpt.synchronize()
        if guides[0]:
            blend(alb, a_j.cpu().numpy(), lerp_factor(first + j, flags))
        if guides[1]:
            blend(nd, nd_j.cpu().numpy(), lerp_factor(first + j, flags))
        if j + 1 in snapshots or j + 1 == n:
            out[j + 1] = ([tile.cpu().numpy(), mo.cpu().numpy(), alb.copy(), nd.copy()], tpt.ray_counter_read() - before)
    return out


_references = {}


def reference(tpt, first, flags, kind):
    """the sequence at W x H over 65 frames, computed once per (first frame, flags, initial contents) and shared: its state after 1, 3,
    33 and 65 frames"""
    key = (first, flags, kind)
    if key not in _references:
        _references[key] = sequence(tpt, W, H, first, max(COUNTS), flags, initial(W, H, kind), snapshots=COUNTS)
    return _references[key]


def assert_same(got, want, what):
    for name, g, w_ in zip(NAMES, got[0], want[0]):
        assert g.tobytes() == w_.tobytes(), "%s: %s differs (%d of %d values)" % (what, name, int((g.view(np.int32) != w_.view(np.int32)).sum()), g.size)
    assert got[1] == want[1], "%s: the ray counter advanced by %d, the sequence's by %d" % (what, got[1], want[1])


# ---------------------------------------------------------------- 1. against the sequence, and against the CPU statement
@pytest.mark.parametrize("kind", ["zeroed", "finite"])
@pytest.mark.parametrize("flags", [FLAG_PROGRESSIVE, 0], ids=["progressive", "each-frame-its-own"])
@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("n", COUNTS)
def test_call_equals_the_sequence(tpt_defaults, n, first, flags, kind):
    tpt = tpt_defaults
    start = initial(W, H, kind)
    got = call(tpt, W, H, first, [n], flags, start)
    assert_same(got, reference(tpt, first, flags, kind)[n], "%d frames from %d" % (n, first))
    for k in (0, 1):  # the tile's alpha and the moments' .w are nobody's to write
        assert got[0][k][..., 3].tobytes() == start[k][..., 3].tobytes(), NAMES[k]


@pytest.mark.parametrize("n,first,flags,kind", [(3, 0, FLAG_PROGRESSIVE, "zeroed"), (33, 5, FLAG_PROGRESSIVE, "finite"), (3, 5, 0, "finite"),
                                                (33, 0, FLAG_PROGRESSIVE, "zeroed")])
def test_call_equals_the_cpu_statement(tpt_defaults, checker, oracle, n, first, flags, kind):
    """tests/moments_checker.c's per-frame planes, blended in numpy float32: nothing of the library in the reference"""
    start = initial(W, H, kind)
    got, rays = call(tpt_defaults, W, H, first, [n], flags, start)
    want = cpu_statement(checker, oracle, W, H, 4, first, n, flags, *start)
    for name, g, w_ in zip(NAMES, got, want[1:]):
        assert g.tobytes() == w_.tobytes(), "%s differs from the CPU statement" % name
    assert rays == sum(want[0])


@pytest.mark.parametrize("flags", [FLAG_PROGRESSIVE, 0], ids=["progressive", "each-frame-its-own"])
def test_calls_continue_one_another(tpt_defaults, flags):
    """33 frames in one call, and in calls of 20 + 13"""
    tpt = tpt_defaults
    one = call(tpt, W, H, 5, [33], flags, initial(W, H, "finite"))
    assert_same(call(tpt, W, H, 5, [20, 13], flags, initial(W, H, "finite")), one, "20 + 13 frames against 33")
    assert_same(one, reference(tpt, 5, flags, "finite")[33], "33 frames")


# ---------------------------------------------------------------- 2. against tptDrawDeviceBatch
@pytest.mark.parametrize("flags", [FLAG_PROGRESSIVE, 0], ids=["progressive", "each-frame-its-own"])
def test_the_tile_is_tptDrawDeviceBatch_s(tpt_defaults, flags):
    import torch
    tpt = tpt_defaults
    start = initial(W, H, "finite")
    got, rays = call(tpt, W, H, 5, [65], flags, start)
    tile = dev(start[0])
    torch.cuda.synchronize()
    tpt.UpdateTest(0.0, 5, W, H, flags)
    before = tpt.ray_counter_read()
    tpt.draw_device_batch(0.0, 5, 65, W, H, tile.data_ptr(), flags)
    tpt.synchronize()
    assert got[0].tobytes() == tile.cpu().numpy().tobytes() and rays == tpt.ray_counter_read() - before


# ---------------------------------------------------------------- 3. small and strided sizes
def one_pass_of_the_fold():
    """pixels one pass of the fold's grid covers: the launcher's cap on workgroups per plane, 256 pixels each"""
    text = open(os.path.join(ROOT, "toypathtracer_amd", "csrc", "tpt_device.h")).read()
    return 256 * int(re.search(r"#define TPT_FOLD_BLOCKS_PER_PLANE (\d+)", text).group(1))


def smallest_size_past(pixels):
    """the smallest w x h > pixels with both sides at most 8192"""
    for n in range(pixels + 1, pixels + 4096):
        for h in range(1, 65):
            if n % h == 0 and n // h <= 8192:
                return n // h, h
    raise AssertionError("no size found")


@pytest.mark.parametrize("size", ["1x1", "257x1", "past-one-pass"])
def test_small_and_strided_sizes(tpt_defaults, size):
    tpt = tpt_defaults
    w, h = {"1x1": (1, 1), "257x1": (257, 1)}.get(size) or smallest_size_past(one_pass_of_the_fold())
    if size == "past-one-pass":
        assert w * h == one_pass_of_the_fold() + 1 == 32769, (w, h)  # (3641 x 9: the last pixel alone is a second pass's)
    n = 2 if size == "past-one-pass" else 34
    start = initial(w, h, "finite")
    assert_same(call(tpt, w, h, 0, [n], FLAG_PROGRESSIVE, start), sequence(tpt, w, h, 0, n, FLAG_PROGRESSIVE, start)[n], "%d x %d" % (w, h))


# ---------------------------------------------------------------- 4. pointer and channel cases
@pytest.mark.parametrize("guides", [(False, True), (True, False), (False, False)], ids=["no-albedo", "no-normal-depth", "neither"])
def test_guide_planes_left_out(tpt_defaults, guides):
    """a guide pointer NULL: the other planes are the full call's, and the plane that was not given is not touched"""
    tpt = tpt_defaults
    start = initial(W, H, "finite")
    got, rays = call(tpt, W, H, 5, [33], FLAG_PROGRESSIVE, start, guides)
    want, want_rays = reference(tpt, 5, FLAG_PROGRESSIVE, "finite")[33]
    for k, name in enumerate(NAMES):
        given = k < 2 or guides[k - 2]
        assert got[k].tobytes() == (want[k] if given else start[k]).tobytes(), name
    assert rays == want_rays


def test_alpha_and_moments_w_are_preserved(tpt_defaults):
    """distinct sentinels in the tile's alpha and the moments' .w; the guides' fourth channels are blended like the others"""
    tpt = tpt_defaults
    start = initial(W, H, "zeroed")
    start[0][..., 3], start[1][..., 3] = np.float32(-7.5), np.float32(1234.25)
    got, _ = call(tpt, W, H, 0, [33], FLAG_PROGRESSIVE, start)
    assert (got[0][..., 3] == np.float32(-7.5)).all() and (got[1][..., 3] == np.float32(1234.25)).all()
    want = reference(tpt, 0, FLAG_PROGRESSIVE, "zeroed")[33][0]
    assert got[0][..., :3].tobytes() == want[0][..., :3].tobytes() and got[1][..., :3].tobytes() == want[1][..., :3].tobytes()
    assert got[2].tobytes() == want[2].tobytes() and got[3].tobytes() == want[3].tobytes()
    assert (got[2][..., 3] != 0).any() and (got[3][..., 3] != 0).any(), "coverage and depth are averaged too"


# ---------------------------------------------------------------- 5. the scenes that go frame by frame
@pytest.mark.parametrize("scene", ["four-spheres", "256-spheres"])
def test_the_other_paths(tpt_defaults, oracle, scene):
    tpt = tpt_defaults
    if scene == "four-spheres":
        s, m = oracle.default_scene()
        tpt.set_scene(s[:4].copy(), m[:4].copy())
    else:
        from toypathtracer_amd.scenes import stress_scene
        tpt.set_scene(*stress_scene(256, 16))
    w, h, n = 24, 16, 3
    start = initial(w, h, "finite")
    try:
        assert_same(call(tpt, w, h, 2, [n], FLAG_PROGRESSIVE, start), sequence(tpt, w, h, 2, n, FLAG_PROGRESSIVE, start)[n], scene)
        assert tpt.scene_info()["spheres"] == (4 if scene == "four-spheres" else 256)
    finally:
        tpt.set_scene(None)


# ---------------------------------------------------------------- 6. refusals
def test_refusals_write_nothing(tpt_defaults):
    import torch
    import lights_lib
    tpt = tpt_defaults
    lib = tpt.load_library()
    w, h = 16, 8
    nan_bits = 0x7FC01234  # (a payload of its own: "still NaN" would not notice a NaN written over a NaN)
    planes = [torch.full((h, w, 4), nan_bits, dtype=torch.int32, device="cuda").view(torch.float32) for _ in range(4)]
    two = torch.full((2, h, w, 4), nan_bits, dtype=torch.int32, device="cuda").view(torch.float32)
    torch.cuda.synchronize()
    tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
    before = tpt.ray_counter_read()
    ptrs = [p.data_ptr() for p in planes]
    plane = w * h * 16
    refusals = 0

    def refused(what, first=0, n=3, ww=w, hh=h, p=None, flags=FLAG_PROGRESSIVE):
        nonlocal refusals
        p = ptrs if p is None else p
        rc = lib.tptDrawDeviceBatchMoments(0.0, first, n, ww, hh, p[0], p[1], p[2], p[3], flags)
        msg = lib.tptGetLastError().decode()
        assert rc != 0 and "tptDrawDeviceBatchMoments" in msg, (what, rc, msg)
        refusals += 1

    refused("0 frames", n=0)
    refused("-3 frames", n=-3)
    refused("firstFrame -1", first=-1)
    refused("a last frame past 2^31 - 1", first=2 ** 31 - 2, n=3)
    refused("kFlagAnimate", flags=FLAG_PROGRESSIVE | FLAG_ANIMATE)
    refused("an unknown flag", flags=FLAG_PROGRESSIVE | 4)
    refused("tile NULL", p=[None] + ptrs[1:])
    refused("moments NULL", p=[ptrs[0], None] + ptrs[2:])
    refused("no tptUpdate at this size", hh=h + 1)
    refused("moments is the tile", p=[ptrs[0], ptrs[0]] + ptrs[2:])
    refused("albedo is the normal / depth", p=ptrs[:3] + [ptrs[2]])
    refused("normal / depth is the tile", p=ptrs[:3] + [ptrs[0]])
    refused("albedo ends in the normal / depth's first pixel", p=ptrs[:2] + [two.data_ptr(), two.data_ptr() + plane - 4])
    tpt.set_seed_mode(tpt.SEED_ROW_SERIAL); refused("row-serial seeds"); tpt.set_seed_mode(tpt.SEED_PER_PIXEL)
    tpt.set_fold_mode(1); refused("forward fold"); tpt.set_fold_mode(tpt.FOLD_RECURSIVE)
    tpt.set_kernel_variant(0, 1, -1); refused("the lane-refill kernel"); tpt.set_kernel_variant(0, 3, -1)
    tpt.set_samples_per_pixel(2048); refused("2048 spp"); tpt.set_samples_per_pixel(4)
    tpt.set_row_shard(8, 2, 0); refused("row sharding"); tpt.set_row_shard(0, 1, 0)
    mirror = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    tpt.set_tile_mirror(mirror.data_ptr()); refused("tile mirror"); tpt.set_tile_mirror(None)
    try:
        tpt.set_scene(*lights_lib.stress_with_lights(4096, 64, 3072))
        tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
        refused("3072 lights")
        assert "3072 emissive spheres" in lib.tptGetLastError().decode()
    finally:
        tpt.set_scene(None)
    tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
    tpt.synchronize()
    assert refusals == 20
    for name, p in zip(NAMES + ("a pair of planes",), planes + [two]):
        assert (p.view(torch.int32) == nan_bits).all().item(), "a refused call wrote to %s" % name
    assert tpt.ray_counter_read() == before and (mirror == 0).all().item()
    # ... and the context still works
    start = initial(w, h, "zeroed")
    assert_same(call(tpt, w, h, 0, [2], FLAG_PROGRESSIVE, start), sequence(tpt, w, h, 0, 2, FLAG_PROGRESSIVE, start)[2], "after the refusals")


# ---------------------------------------------------------------- 7. the consumer
def test_planes_feed_the_variance_filter(tpt_defaults):
    """the new call's planes and the sequence's, each through tptDenoiseDeviceVariance with the samples the header names"""
    import torch
    tpt = tpt_defaults
    first, n = 0, 33
    got, _ = call(tpt, W, H, first, [n], FLAG_PROGRESSIVE, initial(W, H, "zeroed"))
    want, _ = reference(tpt, first, FLAG_PROGRESSIVE, "zeroed")[n]
    samples = tpt.moment_samples(4, first + n - 1, FLAG_PROGRESSIVE)
    assert samples == 4.0 * n
    outs = []
    for planes in (got, want):
        tile, mo, alb, nd = (dev(p) for p in planes)
        out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        tpt.denoise_device_variance(W, H, tile.data_ptr(), mo.data_ptr(), samples, out.data_ptr(), albedo_ptr=alb.data_ptr(),
                                    normal_depth_ptr=nd.data_ptr())
        tpt.synchronize()
        outs.append(out.cpu().numpy())
    assert np.isfinite(outs[0][..., :3]).all()
    assert outs[0].tobytes() == outs[1].tobytes()
