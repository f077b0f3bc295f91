"""A pool of chunks per frame in the plain batched launch of the path-queue kernel (csrc/tpt_frame_pools.h): a launch of 2..8 frames
deals its workgroups to the frames, each workgroup takes chunks of its own frame only and leaves when that frame's pool is dry.  Every
pixel is traced by the same code with the same seeds as before, so the tile bytes and the ray counts stay the oracle's -- at the shapes
where the mapping of workgroups to frames can go wrong, at the shapes that keep the shared pool, and for a streaming caller whose
launches re-arm and re-use the counters."""
import numpy as np
import pytest

from oracle_lib import FLAG_PROGRESSIVE, SEED_PER_PIXEL

pytestmark = pytest.mark.gpu

_ORACLE = {}


def oracle_prefixes(o, w, h, spp, frames):
    """frames 0..frames-1 of the default scene on a zeroed buffer, once per shape: the ray count of every frame and the tile bytes after
    every frame (shared by the cases of one shape, never modified)"""
    key = (w, h, spp)
    if key not in _ORACLE or len(_ORACLE[key][0]) < frames:
        spheres, mats = o.default_scene()
        cam = o.default_camera(w, h)
        bb = np.zeros((h, w, 4), np.float32)
        per, tiles = [], []
        for f in range(frames):
            r, _ = o.render(spheres, mats, cam, w, h, spp, f, FLAG_PROGRESSIVE, backbuffer=bb, seed_mode=SEED_PER_PIXEL)
            per.append(r)
            tiles.append(bb.tobytes())
        _ORACLE[key] = (per, tiles)
    return _ORACLE[key]


def batch_once(tpt, w, h, spp, n):
    """one tptDrawDeviceBatch of n frames into a zeroed tile -> (rays, tile bytes, workgroups of the launch)"""
    import torch
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tpt.set_samples_per_pixel(spp)
    r0 = tpt.ray_counter_read()
    tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
    tpt.draw_device_batch(0.0, 0, n, w, h, tile.data_ptr(), FLAG_PROGRESSIVE)
    rays = tpt.ray_counter_read() - r0
    return rays, tile.cpu().numpy().tobytes(), tpt.launch_info()["grid_blocks"]


# (w, h, spp, n, pools): pools = the launch takes a pool per frame (2 <= n <= 8 and at least 2 n workgroups)
CASES = [
    (72, 40, 2, 2, True), (72, 40, 2, 3, True), (72, 40, 2, 5, True), (72, 40, 2, 8, True),  # 45 chunks per frame; n does not divide the grid
    (70, 33, 1, 3, True),     # the last chunk of a frame is partial
    (8, 8, 4, 8, False),      # one chunk per frame: a grid of one workgroup, fewer than 2 n -- the shared pool
    (200, 120, 1, 8, True),   # more chunks per frame than workgroups per frame
    (72, 40, 2, 9, False), (72, 40, 2, 32, False),  # more than 8 frames: the shared pool
]


@pytest.mark.parametrize("w,h,spp,n,pools", CASES, ids=["%dx%dx%d-n%d" % c[:4] for c in CASES])
def test_batched_launch_with_frame_pools_equals_the_oracle(tpt_defaults, oracle, w, h, spp, n, pools):
    per, tiles = oracle_prefixes(oracle, w, h, spp, n)
    rays, got, grid = batch_once(tpt_defaults, w, h, spp, n)
    print("frame pools %dx%dx%d n=%d: grid %d, rays %d (oracle %d)" % (w, h, spp, n, grid, rays, sum(per[:n])))
    # the path this case is here for (csrc/tpt_frame_pools.h, framePoolsOfLaunch)
    assert (2 <= n <= 8 and grid >= 2 * n) == pools, (n, grid)
    if (w, h) == (200, 120):
        assert ((w + 7) // 8) * ((h + 7) // 8) > grid // n  # (a workgroup's waves come back to the pool)
    assert rays == sum(per[:n])
    assert got == tiles[n - 1]


def test_same_launch_twice_re_arms_the_pools(tpt_defaults, oracle):
    """the launch's last wave zeroes the frames' counters beside the shared one: 40 launches of 5 frames go round the slot ring (32 slots
    in the deepest pipeline) and every launch finds them at zero -- one that did not would trace nothing of those frames"""
    import torch
    tpt = tpt_defaults
    w, h, spp, n, launches = 72, 40, 2, 5, 40
    per, tiles = oracle_prefixes(oracle, w, h, spp, n)
    tpt.set_samples_per_pixel(spp)
    out = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(launches)]
    torch.cuda.synchronize()
    r0 = tpt.ray_counter_read()
    tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
    for t in out:
        tpt.draw_device_batch(0.0, 0, n, w, h, t.data_ptr(), FLAG_PROGRESSIVE)
    rays = tpt.ray_counter_read() - r0
    assert rays == launches * sum(per[:n])
    assert all(t.cpu().numpy().tobytes() == tiles[n - 1] for t in out)


def _stream(tpt, w, h, frames, first=0, tile=None):
    """`frames` consecutive tptDrawDevice calls without a wait; the blend of every call leaves the running ray total in a slot of its own
    (tptSetTileMirror's counter) -> (tile bytes after the final synchronise, the totals after each call, trace launches)"""
    import torch
    if tile is None:
        tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    mirror = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    totals = torch.zeros(frames, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    tpt.kernel_timing_begin(frames)
    try:
        for f in range(frames):
            tpt.set_tile_mirror(mirror.data_ptr(), totals[f].data_ptr())
            tpt.UpdateTest(0.0, first + f, w, h, FLAG_PROGRESSIVE)
            tpt.draw_device(0.0, first + f, w, h, tile.data_ptr(), FLAG_PROGRESSIVE)
        tpt.synchronize()
    finally:
        tpt.set_tile_mirror(None)
    _, launches = tpt.kernel_timing_end()
    assert mirror.cpu().numpy().tobytes() == tile.cpu().numpy().tobytes()
    return tile, totals.cpu().numpy().tolist(), launches


def test_two_streams_of_small_frames_re_use_the_pools(tpt_defaults, oracle):
    """24 tptDrawDevice calls at 72x40x2 without a wait: the stream rule batches such small frames 8 to a launch at every depth above 1
    (two plain launches first, then three launches of 8 frames, each with a pool per frame), and a second stream right behind the
    first finds the counters re-armed.  Tile and every call's ray count against the oracle."""
    tpt = tpt_defaults
    w, h, spp, frames = 72, 40, 2, 24
    per, tiles = oracle_prefixes(oracle, w, h, spp, 2 * frames)
    tpt.set_samples_per_pixel(spp)
    depth = tpt.pipeline_info()["overlap_effective"]
    r = tpt.ray_counter_read()
    tile = None
    for first in (0, frames):
        tile, totals, launches = _stream(tpt, w, h, frames, first, tile)
        want = r + np.cumsum(per[first:first + frames])
        print("frame pools stream from %d: depth %d, %d launches, totals %s" % (first, depth, launches, totals))
        assert tile.cpu().numpy().tobytes() == tiles[first + frames - 1]
        assert tpt.ray_counter_read() == want[-1]
        # a call's total holds its own frame and every earlier one ...
        assert all(want[f] <= totals[f] <= want[-1] for f in range(frames)), (totals, want.tolist())
        if launches < frames:
            # ... and nothing else where the frames come 8 to a launch: a stream launch's frames are counted where they are blended, in
            # call order.  The p plain launches a stream starts with (at most 2, until the calls are seen to be consecutive frames; 3
            # launches of 8 behind them) count where they are traced, so the last of them is exact and the earlier ones are bounded above.
            p = launches - 3
            assert 0 <= p <= 2, launches
            assert totals[max(p - 1, 0):] == want[max(p - 1, 0):].tolist()
        r = int(want[-1])
