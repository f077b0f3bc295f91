"""tptRectifyHistoryDevice on the GPU: the pass held byte for byte against its C statement (tests/rectify_checker.c) on the synthetic
planes of tests/test_rectify_checker.py and on a real animated clip chained through tptTemporalAccumulateDevice, plain and in place;
its inputs left alone; refusals that write nothing; and the quality of pass + rectification + filter against pass + filter on the
first frame after the lights of a scene were switched on."""
import ctypes as C

import numpy as np
import pytest

from oracle_lib import FLAG_ANIMATE
from rectify_lib import NAMES, SIZES, RectifyChecker, synthetic_case
from test_gpu_temporal import accumulate, dev, figures, host, plane, spatial, trace_frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return RectifyChecker(tmp_path_factory.mktemp("rectify_checker"))


def rectify(tpt, w, h, colour, moments, acc_colour, acc_moments, in_place=False, **kw):
    """the pass on device planes -> its three outputs on the device (in_place: the first two ARE acc_colour and acc_moments)"""
    import torch
    outs = ([acc_colour, acc_moments] if in_place else [plane(h, w, float("nan")) for _ in range(2)]) + [plane(h, w, float("nan"))]
    torch.cuda.synchronize()
    tpt.rectify_history_device(w, h, colour.data_ptr(), moments.data_ptr(), acc_colour.data_ptr(), acc_moments.data_ptr(),
                               *[t.data_ptr() for t in outs], **kw)
    return outs


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_synthetic_planes(tpt_defaults, checker, size, radius):
    tpt = tpt_defaults
    w, h = size
    planes = synthetic_case(w, h)
    for gamma in (0.0, 0.75, 3.0):
        want = checker.run(*planes, radius=radius, gamma=gamma)
        d = [dev(a) for a in planes]
        outs = rectify(tpt, w, h, *d, radius=radius, gamma=gamma)
        tpt.synchronize()
        for name, g, wnt in zip(NAMES, host(outs), want):
            assert g.tobytes() == wnt.tobytes(), "out %s differs from the checker (gamma %r)" % (name, gamma)
        for a, t in zip(planes, d):
            assert a.tobytes() == t.cpu().numpy().tobytes(), "an input was written"
        outs = rectify(tpt, w, h, *d, in_place=True, radius=radius, gamma=gamma)
        tpt.synchronize()
        for name, g, wnt in zip(NAMES, host(outs), want):
            assert g.tobytes() == wnt.tobytes(), "in place: out %s differs from the checker (gamma %r)" % (name, gamma)
        assert all(a.tobytes() == t.cpu().numpy().tobytes() for a, t in zip(planes[:2], d[:2])), "an input was written"


def test_animated_chain_plain_and_in_place(tpt_defaults, checker):
    """8 animated frames of 96x54 at 4 spp: trace, tptTemporalAccumulateDevice, the new pass, whose outputs are the next frame's prev
    planes -- once into planes of its own and once in place, both equal to the checker on the GPU's own inputs, frame by frame"""
    tpt = tpt_defaults
    w, h, frames = 96, 54, 8
    kw = dict(radius=2, gamma=1.0)
    prev = {"plain": None, "in place": None}
    clipped = 0
    for j in range(frames):
        cam, cur = trace_frame(tpt, w, h, j, FLAG_ANIMATE, 0.05 * j)
        tpt.synchronize()
        got = {}
        for form in prev:
            acc = accumulate(tpt, w, h, cam, cur, prev[form], max_history=16.0)
            tpt.synchronize()
            before = host(cur) + host(acc)
            outs = rectify(tpt, w, h, cur[0], cur[3], acc[0], acc[2], in_place=form == "in place", **kw)
            tpt.synchronize()
            got[form] = host(outs)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(before[:4], host(cur))), "frame %d: an input was written" % j
            if form == "plain":
                assert all(a.tobytes() == b.tobytes() for a, b in zip(before[4:], host(acc))), "frame %d: an input was written" % j
            want = checker.run(before[0], before[3], before[4], before[6], **kw)
            for name, g, wnt in zip(NAMES, got[form], want):
                assert g.tobytes() == wnt.tobytes(), "frame %d, %s: out %s differs from the checker" % (j, form, name)
            clipped += int((got[form][0] != before[4]).any(axis=-1).sum())
            prev[form] = (cam, outs[0], acc[1], cur[2], outs[1])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got["plain"], got["in place"])), "frame %d: the two forms differ" % j
    N = got["plain"][1][..., 3]
    assert clipped > 0 and (N > 1).mean() > 0.5 and (N != np.floor(N)).any()  # (the clamp acted, and shortened histories by fractions)


def test_refusals_leave_out_untouched(tpt_defaults):
    import torch
    tpt = tpt_defaults
    lib = tpt.load_library()
    w, h = 64, 40
    ins = [dev(a) for a in synthetic_case(w, h)]
    outs = [plane(h, w, float("nan")) for _ in range(3)]
    big = plane(2 * h, w, float("nan"))
    torch.cuda.synchronize()
    count = [0]

    def refused(what, ww=w, hh=h, i=None, o=None, radius=2, gamma=1.0):
        ptrs = [t.data_ptr() for t in ins + outs]
        for k, v in list((i or {}).items()) + [(4 + k, v) for k, v in (o or {}).items()]:
            ptrs[k] = v
        rc = lib.tptRectifyHistoryDevice(ww, hh, *[C.c_void_p(p) if p else None for p in ptrs], radius, C.c_float(gamma))
        msg = lib.tptGetLastError().decode()
        assert rc != 0 and "tptRectifyHistoryDevice" in msg, (what, msg)
        tpt.synchronize()
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in outs + [big]), "a refused call wrote an output: " + what
        count[0] += 1

    refused("w 0", ww=0)
    refused("h 8193", hh=8193)
    for k in range(4):
        refused("input %d NULL" % k, i={k: 0})
    for k in range(3):
        refused("output %d NULL" % k, o={k: 0})
    for r in (0, 4, -2):
        refused("radius %d" % r, radius=r)
    for g in (-0.5, float("nan"), float("inf")):
        refused("gamma %r" % g, gamma=g)
    refused("outColour is this frame's colour", o={0: ins[0].data_ptr()})
    refused("outColour is accMoments", o={0: ins[3].data_ptr()})
    refused("outMoments is accColour", o={1: ins[2].data_ptr()})
    refused("outVariance is accMoments", o={2: ins[3].data_ptr()})
    refused("outColour overlaps accColour's tail", i={2: big.data_ptr()}, o={0: big.data_ptr() + 16 * (w * h - 1)})
    refused("two outputs overlap", o={0: big.data_ptr(), 2: big.data_ptr() + 16 * 9})
    refused("two outputs are one", o={1: outs[0].data_ptr()})
    assert count[0] == 2 + 4 + 3 + 3 + 3 + 7


def test_quality_after_a_light_switch(tpt_defaults):
    """96x54, camera and spheres still, 4 spp, maxHistory 16: seven frames with the scene's two emissive materials dark, then
    tptSetScene switches them on.  On that eighth frame, against the same frame at 1024 spp, pass + rectification (RECTIFY_DEFAULTS) +
    filter (DENOISE_VARIANCE_DEFAULTS) beats pass + filter in the linear and in the relative squared error.  The CPU statements of the
    same chain (tools/rectify_rate.py --cpu-switch) give 8.14 -> 2.09 linear and 0.111 -> 0.050 relative: a factor of
    3.9 and of 2.2, so the assertion is a plain `<`."""
    tpt = tpt_defaults
    w, h, frames, spp = 96, 54, 8, 4
    spheres, mats, _, _ = tpt.GetSceneDesc()
    dark = mats.copy()
    dark["emissive"] = 0
    assert (mats["emissive"] > 0).any()
    try:
        prev = {"T": None, "T+R": None}
        for j in range(frames):
            tpt.set_scene(spheres, dark if j < frames - 1 else mats)
            cam, cur = trace_frame(tpt, w, h, j, 0, 0.0)
            outs = {}
            for form in prev:
                acc = accumulate(tpt, w, h, cam, cur, prev[form], max_history=16.0)
                if form == "T+R":
                    colour, moments, variance = rectify(tpt, w, h, cur[0], cur[3], acc[0], acc[2])
                else:
                    colour, moments, variance = acc[0], acc[2], acc[3]
                outs[form] = (colour, acc[1], variance)
                prev[form] = (cam, colour, acc[1], cur[2], moments)
        tpt.synchronize()
        tpt.set_samples_per_pixel(1024)
        _, ref = trace_frame(tpt, w, h, frames - 1, 0, 0.0)
        tpt.synchronize()
        tpt.set_samples_per_pixel(spp)
        ref = ref[0].cpu().numpy()[..., :3].astype(np.float64)
        r = {form: figures(spatial(tpt, w, h, o[0], o[1], cur[2], o[2], spp), ref) for form, o in outs.items()}
    finally:
        tpt.set_scene(None)
    print("light switch 96x54, squared error against 1024 spp (linear / relative): T+S %.4f / %.4f   T+R+S %.4f / %.4f"
          % (r["T"] + r["T+R"]))
    assert r["T+R"][0] < r["T"][0] and r["T+R"][1] < r["T"][1], r
