"""Test infrastructure for tptDrawDeviceBatchMoments (test infrastructure only): the statement of include/tpt_hip.h in numpy float32 --
frame after frame, tptDrawDeviceMoments' tile and moments, and the frame's guide planes blended into the running ones with the tile's
lerp factor, all four channels, `one = float32(1) - lerp` formed in float32, products and the sum rounded one by one (no FMA).  The
per-frame planes come from whoever traces the frames: tests/moments_checker.c on the CPU (cpu_statement), the library's own
tptDrawDeviceMoments on the GPU (the GPU tests' reference sequence)."""
import numpy as np

from oracle_lib import FLAG_PROGRESSIVE

f32 = np.float32


def lerp_factor(frame, flags):
    """the factor tptDrawDevice blends frame `frame` with (Test.cpp:272-276), for flags kFlagProgressive or 0"""
    assert not flags & ~FLAG_PROGRESSIVE
    return f32(frame) / f32(frame + 1) if flags & FLAG_PROGRESSIVE else f32(0)


def blend(running, frame_plane, lerp, channels=4):
    """blendPixel on the first `channels` channels of an [h, w, 4] float32 plane, in place; the others are left alone"""
    lerp = f32(lerp)
    one = f32(1) - lerp
    with np.errstate(all="ignore"):
        running[..., :channels] = running[..., :channels] * lerp + frame_plane[..., :channels] * one
    return running


def fold_frames(tile, moments, albedo, normal_depth, frames, first_frame, flags):
    """The statement's blends over per-frame planes.  `frames`: an iterable of (colour, moments, albedo, normal_depth) of frames
    first_frame, first_frame + 1, ... ([h, w, 4] float32 each; a guide may be None when its running plane is).  tile.xyz and moments.xyz
    are blended (.w kept), the guides in all four channels; every plane is updated in place (None: not wanted)."""
    for j, (c, m, a, nd) in enumerate(frames):
        lerp = lerp_factor(first_frame + j, flags)
        blend(tile, c, lerp, 3)
        blend(moments, m, lerp, 3)
        if albedo is not None:
            blend(albedo, a, lerp)
        if normal_depth is not None:
            blend(normal_depth, nd, lerp)
    return tile, moments, albedo, normal_depth


def cpu_statement(checker, oracle, w, h, spp, first_frame, n_frames, flags, tile=None, moments=None, albedo=None, normal_depth=None):
    """tptDrawDeviceBatchMoments on the built-in scene and camera over tests/moments_checker.c (a MomentsChecker): -> (rays of each frame,
    tile, moments, albedo, normal_depth), the four planes starting from the given ones (zeros when not given)."""
    spheres, mats = oracle.default_scene()
    cam = oracle.default_camera(w, h)
    planes = [np.zeros((h, w, 4), f32) if p is None else np.ascontiguousarray(p, f32).copy() for p in (tile, moments, albedo, normal_depth)]
    rays = []
    for j in range(n_frames):
        f = first_frame + j
        # (the checker blends the tile and the moments itself, with the same lerp factor: Test.cpp:293-295)
        r, _, _, a, nd = checker.render(spheres, mats, cam, w, h, spp, f, flags, backbuffer=planes[0], moments=planes[1])
        rays.append(r)
        blend(planes[2], a, lerp_factor(f, flags))
        blend(planes[3], nd, lerp_factor(f, flags))
    return (rays,) + tuple(planes)
