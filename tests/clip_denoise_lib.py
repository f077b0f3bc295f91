"""Test infrastructure for tptDenoiseClipDevice (test infrastructure only): the chain the call replaces, twice.  cpu_chain composes the
CPU statements of its links -- tests/temporal_checker.c or tests/object_checker.c, then tests/variance_checker.c (temporal_lib,
object_lib, moments_lib) -- frame after frame on host planes; gpu_chain drives the existing per-frame entry points through the Python
binding on device stacks.  Both return every frame's filtered plane and the last frame's temporal outputs {colour, albedo, moments},
which is what the call leaves in deviceHistory.  synthetic_clip makes seeded frames whose history survives from frame to frame."""
import numpy as np

from moments_lib import DEMODULATE
from temporal_lib import look_at_camera, random_frame

PLANES = ("images", "albedo", "nd", "moments")


def cpu_chain(variance_checker, frames, samples, temporal_checker=None, cams=None, object_checker=None, objects=None, tables=None,
              prev=None, filter_kw=None, temporal_kw=None):
    """frames: per frame (colour, albedo, normal_depth, moments) host planes.  Without temporal_checker / object_checker: the filter
    alone on each frame (albedo / normal_depth may be None).  With one: T_j from the checker -- object_checker with objects[j],
    objects[j - 1] and tables[j] (tables None: no table) -- then the filter of (T_j.colour, T_j.albedo, normal_depth_j, T_j.variance).
    prev: None or (camera, colour, albedo, normal_depth, moments[, object]) of the frame before frame 0.
    -> (filtered planes, last T as (colour, albedo, moments) or None)"""
    filter_kw, temporal_kw = dict(filter_kw or {}), dict(temporal_kw or {})
    outs, last = [], None
    for j, (colour, albedo, nd, moments) in enumerate(frames):
        if temporal_checker is None and object_checker is None:
            outs.append(variance_checker.run(colour, albedo, nd, moments, samples, **filter_kw))
            continue
        if object_checker is not None:
            t = object_checker.run(cams[j], (colour, albedo, nd, moments), objects[j], prev,
                                   None if tables is None or prev is None else tables[j], **temporal_kw)
            nxt = (cams[j], t[0], t[1], nd, t[2], objects[j])
        else:
            t = temporal_checker.run(cams[j], (colour, albedo, nd, moments), prev, **temporal_kw)
            nxt = (cams[j], t[0], t[1], nd, t[2])
        outs.append(variance_checker.run(t[0], t[1], nd, t[3], samples, **filter_kw))
        prev, last = nxt, (t[0], t[1], t[2])
    return outs, last


def filter_kwargs(api, nd=True, demodulate=True, iterations=None):
    """denoise_device_variance's defaults as VarianceChecker.run's keywords (a guide's sigma is 0 without its plane)"""
    d = api.DENOISE_VARIANCE_DEFAULTS
    return dict(iterations=d["iterations"] if iterations is None else iterations, sigma_luminance=d["sigma_luminance"],
                sigma_normal=d["sigma_normal"] if nd else 0.0, sigma_depth=d["sigma_depth"] if nd else 0.0,
                flags=DEMODULATE if demodulate else 0)


def gpu_chain(tpt, w, h, stacks, samples, cams=None, spatial_only=False, objects=None, motion=None, n_objects=0, prev=None, history=None,
              **kw):
    """The per-frame entry points on device stacks.  stacks: dict of [n, h, w, 4] float32 device tensors "images", "moments" and
    (optional when spatial_only) "albedo", "nd".  objects: None or an [n, h, w] int32 device tensor; motion: None or an [n, n_objects, 4]
    device tensor.  prev / history as denoise_clip_device takes them (history: a [3, h, w, 4] device tensor, read only here).  kw:
    iterations and demodulate for the filter.  -> ([n, h, w, 4] filtered planes, last T as a [3, h, w, 4] tensor or None)"""
    import torch
    n = stacks["images"].shape[0]
    out = torch.full((n, h, w, 4), float("nan"), dtype=torch.float32, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    if spatial_only:
        for j in range(n):
            tpt.denoise_device_variance(w, h, stacks["images"][j].data_ptr(), stacks["moments"][j].data_ptr(), samples, out[j].data_ptr(),
                                        albedo_ptr=ptr(stacks["albedo"][j]) if stacks.get("albedo") is not None else None,
                                        normal_depth_ptr=ptr(stacks["nd"][j]) if stacks.get("nd") is not None else None, **kw)
        tpt.synchronize()
        return out, None
    t = torch.full((2, 4, h, w, 4), float("nan"), dtype=torch.float32, device="cuda")  # T of even and odd frames
    before = None
    if prev is not None:
        before = (prev[0], history[0].data_ptr(), history[1].data_ptr(), prev[1], history[2].data_ptr()) + tuple(prev[2:])
    for j in range(n):
        cur = [stacks[k][j].data_ptr() for k in PLANES]
        o = [t[j & 1, k].data_ptr() for k in range(4)]
        if objects is not None:
            table = motion is not None and before is not None
            tpt.temporal_accumulate_objects_device(w, h, cams[j], *cur, objects[j].data_ptr(), *o, prev=before,
                                                   motion_ptr=motion[j].data_ptr() if table else None, n_objects=n_objects if table else 0)
            before = (cams[j], o[0], o[1], cur[2], o[2], objects[j].data_ptr())
        else:
            tpt.temporal_accumulate_device(w, h, cams[j], *cur, *o, prev=before)
            before = (cams[j], o[0], o[1], cur[2], o[2])
        tpt.denoise_device_variance(w, h, o[0], o[3], samples, out[j].data_ptr(), albedo_ptr=o[1], normal_depth_ptr=cur[2], **kw)
    tpt.synchronize()
    return out, t[(n - 1) & 1, :3].clone()


def synthetic_clip(n, w, h, seed=0):
    """n seeded frames in the shape the clip draws leave them, and their cameras.  All frames share their guides (coverage, normal,
    depth) and most share their camera, so every pixel's own tap agrees and the history grows; every seventh camera stands 5 cm to the
    side (fractional taps, most of the history lost).  -> (cams float32 [n, 22], frames as a list of (colour, albedo, nd, moments))"""
    rng = np.random.default_rng([seed, n, w, h])
    base = random_frame(rng, h, w)
    frames, cams = [], []
    for j in range(n):
        colour, albedo, _, moments = random_frame(rng, h, w)
        albedo[..., 3] = base[1][..., 3]
        albedo[..., :3] *= (base[1][..., 3] > 0)[..., None]
        frames.append((colour, np.ascontiguousarray(albedo), base[2].copy(), moments))
        cams.append(look_at_camera([0.05 if j % 7 == 6 else 0.0, 2.0, 3.0], [0.0, 0.0, 0.0], w, h))
    return np.stack(cams), frames


def camera_records(api, cams):
    """float32 [n, 22] -> a CAMERA_DT array of n records"""
    return np.ascontiguousarray(cams, np.float32).reshape(-1).view(api.CAMERA_DT).copy()


def stacks_of(frames):
    """host frames -> dict of [n, h, w, 4] device tensors"""
    import torch
    return {k: torch.from_numpy(np.stack([f[i] for f in frames])).cuda() for i, k in enumerate(PLANES)}
