"""tptDenoiseClipDevice on the GPU: the frames of a clip through the temporal pass and the variance-guided filter in one call, the
filter's iterations one launch per chunk of frames.  Every byte of the output is held (no tolerance anywhere) against the per-frame
entry points the call replaces, driven on the GPU, and against the CPU statements of the chain's links (tests/clip_denoise_lib.py):
spatial-only on synthetic planes at sizes whose wide taps leave the image, the plain pass on a camera clip's planes, the
object-following pass on a keyframe clip's, the chunk seam of a 33-frame clip and its continuation over two calls, refusals, and the
context's traced-ahead frames."""
import ctypes as C

import numpy as np
import pytest

from clip_denoise_lib import camera_records, cpu_chain, filter_kwargs, gpu_chain, stacks_of, synthetic_clip
from moments_lib import VarianceChecker, random_moments, random_planes
from object_lib import ObjectChecker
from oracle_lib import FLAG_ANIMATE, FLAG_PROGRESSIVE
from temporal_lib import TemporalChecker
from test_gpu_animation_moments import GUARD, guarded, guards_intact, same
from test_gpu_camera_clip import orbit_views
from test_gpu_keyframe_clip import draw_keyframe_clip

pytestmark = pytest.mark.gpu

SPP = 4  # (tests/conftest.py's default)


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    d = tmp_path_factory.mktemp("clip_denoise_checkers")
    return dict(variance=VarianceChecker(d), temporal=TemporalChecker(d), objects=ObjectChecker(d))


def clip(tpt, w, h, stacks, samples, **kw):
    """one denoise_clip_device call on device stacks -> the [n, h, w, 4] output; its guard planes are checked, and no input changes"""
    import torch
    n = stacks["images"].shape[0]
    out = guarded(n, h, w)
    watched = [t for t in list(stacks.values()) + [kw.get("objects"), kw.get("motion")] if t is not None]
    before = [t.clone() for t in watched]
    torch.cuda.synchronize()
    named = dict(albedo_ptr=stacks.get("albedo"), normal_depth_ptr=stacks.get("nd"), objects_ptr=kw.pop("objects", None),
                 motion_ptr=kw.pop("motion", None), history_ptr=kw.pop("history", None))
    tpt.denoise_clip_device(w, h, n, stacks["images"].data_ptr(), stacks["moments"].data_ptr(), out[1].data_ptr(), samples,
                            **{k: None if t is None else t.data_ptr() for k, t in named.items()}, **kw)
    tpt.synchronize()
    torch.cuda.synchronize()
    assert guards_intact(out), "the call wrote outside deviceFrameOut"
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(watched, before)), "the call wrote an input"
    return out[1:n + 1]


def floats_of(cams):
    """a CAMERA_DT array -> float32 [n, 22], one row per record (what the CPU statements take)"""
    return np.ascontiguousarray(cams).view(np.float32).reshape(-1, 22)


def assert_planes(got, want, what):
    for j in range(got.shape[0]):
        g, w_ = got[j].cpu().numpy(), want[j] if isinstance(want[j], np.ndarray) else want[j].cpu().numpy()
        assert g.tobytes() == w_.tobytes(), "frame %d differs from %s: %d words" % (j, what, int((g.view(np.uint32) != w_.view(np.uint32)).sum()))


# ---------------------------------------------------------------- 1. spatial-only, synthetic planes that differ per frame
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("size", [(1, 1), (17, 1), (1, 17), (130, 67)], ids=lambda s: "%dx%d" % s)
def test_spatial_only_equals_the_filter_per_frame(tpt_defaults, checkers, size, n):
    """iterations 1, 2 and 5 (at 5 the step-16 taps leave a 17-pixel image on both sides: under a flat index they would read the
    neighbouring frames, which differ), with and without the normal / depth plane, with and without demodulation"""
    import torch
    tpt = tpt_defaults
    w, h = size
    rng = np.random.default_rng([7, w, h, n])
    frames = []
    for _ in range(n):
        colour, albedo, nd = random_planes(rng, h, w)
        frames.append((colour, albedo, nd, random_moments(rng, colour)))
    full = stacks_of(frames)
    assert n == 1 or not torch.equal(full["images"][0], full["images"][1])
    for iterations in (1, 2, 5):
        for guide in (True, False):
            for demodulate in (True, False):
                stacks = dict(full) if guide else {k: v for k, v in full.items() if k != "nd"}
                kw = dict(iterations=iterations, demodulate=demodulate)
                got = clip(tpt, w, h, stacks, float(SPP), spatial_only=True, **kw)
                want, _ = gpu_chain(tpt, w, h, stacks, float(SPP), spatial_only=True, **kw)
                assert_planes(got, want, "tptDenoiseDeviceVariance (%d iterations, guide %s, demodulate %s)" % (iterations, guide, demodulate))
                if size == (130, 67):
                    host = [(c, a, nd if guide else None, m) for c, a, nd, m in frames]
                    cpu, _ = cpu_chain(checkers["variance"], host, float(SPP),
                                       filter_kw=filter_kwargs(tpt, guide, demodulate, iterations))
                    assert_planes(got, cpu, "the CPU statement")
    # without an albedo plane (no demodulation), at another sample count
    bare = {k: full[k] for k in ("images", "moments")}
    got = clip(tpt, w, h, bare, 2.0, spatial_only=True)
    assert_planes(got, gpu_chain(tpt, w, h, bare, 2.0, spatial_only=True)[0], "tptDenoiseDeviceVariance without guides")


# ---------------------------------------------------------------- 2. the plain temporal pass on a camera clip's planes
def test_camera_clip_through_the_plain_chain(tpt_defaults, checkers):
    """tptDrawDeviceCameraClip, default scene, 130 x 67 x 4 spp, 5 frames of a 0.5-degree orbit over the animated scene, the call
    enqueued directly behind the draw; then the same planes again after a synchronise, the per-frame chain on the GPU, the CPU chain"""
    import torch
    tpt = tpt_defaults
    w, h, n = 130, 67, 5
    times, views = [0.05 * j for j in range(n)], orbit_views(n, step=0.5)
    tile, mo = (torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(2))
    stacks = {k: torch.full((n, h, w, 4), GUARD, dtype=torch.float32, device="cuda") for k in ("images", "albedo", "nd", "moments")}
    behind = guarded(n, h, w)
    history = torch.full((3, h, w, 4), GUARD, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tpt.UpdateTest(times[0], 0, w, h, FLAG_ANIMATE)
    cams = tpt.draw_device_camera_clip(times, views, 0, w, h, tile.data_ptr(), mo.data_ptr(), FLAG_ANIMATE,
                                       images_ptr=stacks["images"].data_ptr(), albedo_ptr=stacks["albedo"].data_ptr(),
                                       normal_depth_ptr=stacks["nd"].data_ptr(), frame_moments_ptr=stacks["moments"].data_ptr())
    tpt.denoise_clip_device(w, h, n, stacks["images"].data_ptr(), stacks["moments"].data_ptr(), behind[1].data_ptr(), float(SPP),
                            albedo_ptr=stacks["albedo"].data_ptr(), normal_depth_ptr=stacks["nd"].data_ptr(), cameras=cams,
                            history_ptr=history.data_ptr())  # (no synchronise in between)
    tpt.synchronize()
    torch.cuda.synchronize()
    assert guards_intact(behind)
    got = clip(tpt, w, h, stacks, float(SPP), cameras=cams)
    assert_planes(behind[1:n + 1], got, "the same call after a synchronise")
    want, last = gpu_chain(tpt, w, h, stacks, float(SPP), cams=cams)
    assert_planes(got, want, "the per-frame chain on the GPU")
    assert same(history, last), "deviceHistory differs from the chain's last temporal outputs"
    N = last[2][..., 3].cpu().numpy()
    assert (N >= 2).sum() > 0 and (N == 1).sum() > 0, "the history is not exercised: N >= 2 on %d pixels, N == 1 on %d" % ((N >= 2).sum(), (N == 1).sum())
    frames = [tuple(stacks[k][j].cpu().numpy() for k in ("images", "albedo", "nd", "moments")) for j in range(n)]
    cpu, cpu_last = cpu_chain(checkers["variance"], frames, float(SPP), temporal_checker=checkers["temporal"], cams=floats_of(cams),
                              filter_kw=filter_kwargs(tpt), temporal_kw=tpt.TEMPORAL_DEFAULTS)
    assert_planes(got, cpu, "the CPU chain")
    assert all(history[k].cpu().numpy().tobytes() == cpu_last[k].tobytes() for k in range(3))
    assert bool(torch.isfinite(got[..., :3]).all())


# ---------------------------------------------------------------- 3. the object-following pass on a keyframe clip's planes
def test_keyframe_clip_through_the_object_following_chain(tpt_defaults, checkers):
    """tptDrawDeviceKeyframeClip, 3 frames, sphere 5 (the metal sphere in front of the camera, about 100 pixels at this size, none of
    them hidden on its way) moved by its radius per frame; api.motion_table tables with a cap of 2 on the metal and glass spheres,
    uploaded as one stack (table 0 is not read: the call starts a sequence); and without tables"""
    import torch
    tpt = tpt_defaults
    w, h, n = 66, 35, 3
    spheres, mats = tpt.GetSceneDesc()[:2]
    moved = 5
    ids = [moved]
    radius = np.float32(spheres["radius"][moved])
    centres = np.array([[[spheres["cx"][moved] + radius * j, spheres["cy"][moved], spheres["cz"][moved]]] for j in range(n)], np.float32)
    src = draw_keyframe_clip(tpt, w, h, (spheres, mats), orbit_views(n, step=0.5), ids, centres, 0, 0,
                             prev=(np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)))
    objects = src["objects"].contiguous()
    assert all(int((objects[j] == moved).sum()) > 20 for j in range(n)), "the moved sphere is not in view"
    caps = np.where(mats["type"] != 0, 2.0, 0.0).astype(np.float32)
    tables = [np.zeros((len(spheres), 4), np.float32)]
    for j in range(1, n):
        a, b = spheres.copy(), spheres.copy()
        a["cx"][moved], b["cx"][moved] = centres[j - 1, 0, 0], centres[j, 0, 0]
        tables.append(tpt.motion_table(a, b, caps))
    assert all(t[moved, 0] == -radius and np.count_nonzero(t[:, :3]) == 1 for t in tables[1:]) and (tables[1][:, 3] == caps).all()
    motion = torch.from_numpy(np.stack(tables)).cuda()
    stacks = {"images": src["images"].contiguous(), "albedo": src["albedo"].contiguous(), "nd": src["nd"].contiguous(),
              "moments": src["fmo"].contiguous()}
    cams = src["cams"]
    got = clip(tpt, w, h, stacks, float(SPP), cameras=cams, objects=objects, motion=motion, n_objects=len(spheres))
    want, last = gpu_chain(tpt, w, h, stacks, float(SPP), cams=cams, objects=objects, motion=motion, n_objects=len(spheres))
    assert_planes(got, want, "the per-frame object-following chain on the GPU")
    frames = [tuple(stacks[k][j].cpu().numpy() for k in ("images", "albedo", "nd", "moments")) for j in range(n)]
    host_objects = [objects[j].cpu().numpy() for j in range(n)]
    cpu, _ = cpu_chain(checkers["variance"], frames, float(SPP), object_checker=checkers["objects"], cams=floats_of(cams), objects=host_objects,
                       tables=tables, filter_kw=filter_kwargs(tpt), temporal_kw=tpt.TEMPORAL_DEFAULTS)
    assert_planes(got, cpu, "the CPU chain")
    on = host_objects[n - 1] == moved
    assert (last[2][..., 3].cpu().numpy()[on] >= 2).sum() > 0, "no pixel of the moved sphere kept its history"
    # without a table: nothing moves, nothing is capped -- other bytes, the same agreement
    bare = clip(tpt, w, h, stacks, float(SPP), cameras=cams, objects=objects)
    assert_planes(bare, gpu_chain(tpt, w, h, stacks, float(SPP), cams=cams, objects=objects)[0], "the chain without a table")
    assert not same(bare, got)
    # ... and the plain pass on the same planes is yet another result (the id test and the table count)
    assert not same(clip(tpt, w, h, stacks, float(SPP), cameras=cams), got)


# ---------------------------------------------------------------- 4. the chunk seam, and a clip continued over two calls
def test_chunk_seam_and_continuation(tpt_defaults, checkers):
    """33 synthetic frames at 34 x 9: frame 32 is a chunk of its own whose temporal pass reads frame 31's outputs from the staging the
    chunk before filled.  Then the same clip as 20 + 13 frames with deviceHistory passed in place"""
    import torch
    tpt = tpt_defaults
    w, h, n = 34, 9, 33
    cam_floats, frames = synthetic_clip(n, w, h)
    cams = camera_records(tpt, cam_floats)
    stacks = stacks_of(frames)
    history = torch.full((5, h, w, 4), GUARD, dtype=torch.float32, device="cuda")  # (3 planes between two guards)
    got = clip(tpt, w, h, stacks, float(SPP), cameras=cams, history=history[1:4])
    want, last = gpu_chain(tpt, w, h, stacks, float(SPP), cams=cams)
    assert_planes(got[31:], want[31:], "the per-frame chain across the chunk seam")
    assert_planes(got, want, "the per-frame chain")
    assert same(history[1:4], last) and guards_intact(history), "deviceHistory is not the chain's T_32"
    N = last[2][..., 3].cpu().numpy()
    assert (N >= 2).sum() > 0 and (N == 4).sum() > 0, "the history is not exercised"
    cpu, cpu_last = cpu_chain(checkers["variance"], frames, float(SPP), temporal_checker=checkers["temporal"], cams=cam_floats,
                              filter_kw=filter_kwargs(tpt), temporal_kw=tpt.TEMPORAL_DEFAULTS)
    assert_planes(got[30:], cpu[30:], "the CPU chain")
    assert all(history[1 + k].cpu().numpy().tobytes() == cpu_last[k].tobytes() for k in range(3))
    # 20 + 13: the second call continues the first through deviceHistory, passed in place, and frame 19's camera and guides
    cut = 20
    history[1:4] = GUARD
    head = {k: v[:cut].contiguous() for k, v in stacks.items()}
    tail = {k: v[cut:].contiguous() for k, v in stacks.items()}
    a = clip(tpt, w, h, head, float(SPP), cameras=cams[:cut], history=history[1:4])
    b = clip(tpt, w, h, tail, float(SPP), cameras=cams[cut:], history=history[1:4], prev=(cams[cut - 1], stacks["nd"][cut - 1].data_ptr()))
    assert_planes(torch.cat([a, b]), got, "the one call over 33 frames")
    assert same(history[1:4], last) and guards_intact(history)


# ---------------------------------------------------------------- 5. refusals on the device
def test_refusals_write_nothing(tpt_defaults):
    import torch
    tpt = tpt_defaults
    lib = tpt.load_library()
    w, h, n = 34, 9, 3
    cam_floats, frames = synthetic_clip(n, w, h)
    cams = camera_records(tpt, cam_floats)
    stacks = stacks_of(frames)
    out = torch.full((n, h, w, 4), GUARD, dtype=torch.float32, device="cuda")
    history = torch.full((3, h, w, 4), GUARD, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def refused(what, **changes):
        a = tpt.ClipDenoiseArgs(
            screenWidth=w, screenHeight=h, nFrames=n, clipFlags=0, deviceFrameImages=stacks["images"].data_ptr(),
            deviceFrameMoments=stacks["moments"].data_ptr(), deviceFrameAlbedo=stacks["albedo"].data_ptr(),
            deviceFrameNormalDepth=stacks["nd"].data_ptr(), cameras=cams.ctypes.data, deviceFrameOut=out.data_ptr(),
            deviceHistory=history.data_ptr(), iterations=5, denoiseFlags=1, samples=4.0, sigmaLuminance=4.0, sigmaNormal=0.03,
            sigmaDepth=0.5, maxHistory=4.0, depthTolerance=0.1, normalTolerance=0.25, coverageTolerance=0.0)
        for k, v in changes.items():
            setattr(a, k, v)
        rc = lib.tptDenoiseClipDevice(C.byref(a))
        msg = lib.tptGetLastError().decode()
        assert rc != 0 and "tptDenoiseClipDevice" in msg, (what, rc, msg)

    plane = w * h * 16
    refused("out is the images", deviceFrameOut=stacks["images"].data_ptr())
    refused("out's last plane is the head of the history", deviceHistory=out.data_ptr() + 2 * plane)
    refused("the history's last plane is the first albedo plane", deviceHistory=stacks["albedo"].data_ptr() - 2 * plane)
    refused("spatial-only with a history", clipFlags=tpt.CLIP_DENOISE_SPATIAL_ONLY)
    refused("a prev plane without prevCamera", devicePrevNormalDepth=stacks["nd"].data_ptr())
    refused("sigmaNormal 1e-7", sigmaNormal=1e-7)
    refused("sigmaLuminance 0", sigmaLuminance=0.0)
    bad = cam_floats.copy()
    bad[2, 6:9] = 0
    refused("camera 2: dot(H, H) == 0", cameras=bad.ctypes.data)
    bad = cam_floats.copy()
    bad[1, 4] = np.inf
    refused("camera 1: a non-finite field", cameras=bad.ctypes.data)
    with pytest.raises(tpt.TptError, match="tptDenoiseClipDevice"):
        tpt.denoise_clip_device(w, h, n, stacks["images"].data_ptr(), stacks["moments"].data_ptr(), stacks["moments"].data_ptr() + plane,
                                4.0, albedo_ptr=stacks["albedo"].data_ptr(), normal_depth_ptr=stacks["nd"].data_ptr(), cameras=cams)
    tpt.synchronize()
    torch.cuda.synchronize()
    assert bool((out == GUARD).all()) and bool((history == GUARD).all()), "a refused call wrote"


# ---------------------------------------------------------------- 6. the context's traced-ahead frames
def test_streamed_frames_lose_nothing(tpt_defaults):
    """12 streamed tptDrawDevice frames at 640 x 360 x 4, every tile taken through the call (spatial-only, one frame) straight after its
    draw: the tiles, the rays, the look-ahead hits and the trace launches are those of the same stream without the call -- as around
    tptDenoiseDevice (tests/test_gpu_denoise.py)"""
    import torch
    tpt = tpt_defaults
    w, h, n = 640, 360, 12
    stream = torch.cuda.Stream()
    moments = torch.rand((h, w, 4), dtype=torch.float32, device="cuda")

    def run(denoise):
        tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        outs = torch.full((n, h, w, 4), float("nan"), dtype=torch.float32, device="cuda")
        stream.wait_stream(torch.cuda.current_stream())
        torch.cuda.synchronize()
        tpt.set_stream(stream.cuda_stream)
        tiles = []
        try:
            r0 = tpt.ray_counter_read()
            hits0 = tpt.lookahead_hits()
            tpt.kernel_timing_begin(64)
            tpt.UpdateTest(0.0, 0, w, h, FLAG_PROGRESSIVE)
            with torch.cuda.stream(stream):
                for f in range(n):
                    tpt.draw_device(0.0, f, w, h, tile.data_ptr(), FLAG_PROGRESSIVE)
                    if denoise:
                        tpt.denoise_clip_device(w, h, 1, tile.data_ptr(), moments.data_ptr(), outs[f].data_ptr(), 4.0, spatial_only=True,
                                                iterations=3)
                    tiles.append(tile.clone())  # (stream-ordered behind the frame's blend)
            _, launches = tpt.kernel_timing_end()
            hits = tpt.lookahead_hits() - hits0
            rays = tpt.ray_counter_read() - r0
            stream.synchronize()
        finally:
            tpt.set_stream(None)
        return tiles, rays, hits, launches, outs

    # (the staging grows to this size here, not inside the streams that are compared)
    warm = torch.zeros((2, h, w, 4), dtype=torch.float32, device="cuda")
    tpt.denoise_clip_device(w, h, 1, warm[0].data_ptr(), moments.data_ptr(), warm[1].data_ptr(), 4.0, spatial_only=True, iterations=3)
    tpt.synchronize()
    plain = run(False)
    den = run(True)
    assert all(same(a, b) for a, b in zip(den[0], plain[0])), "a tile changed"
    assert den[1] == plain[1], (den[1], plain[1])
    assert den[2] == plain[2] and den[3] == plain[3], (den[2:4], plain[2:4])
    # ... and each output is the per-frame filter of its frame's tile
    want = torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda")
    for f in (0, n - 1):
        tpt.denoise_device_variance(w, h, den[0][f].data_ptr(), moments.data_ptr(), 4.0, want.data_ptr(), iterations=3)
        tpt.synchronize()
        assert same(den[4][f], want), f
