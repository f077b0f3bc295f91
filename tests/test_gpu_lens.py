"""tptDrawDeviceLens on the GPU, held byte for byte against its C statement (tests/lens_checker.c: the three projections in front of the
oracle's Trace and TraceForward): image sizes of whole tiles, with padding both ways and a partial last chunk, of one pixel and of a strip;
1 and 4 samples; the built-in scene staged in LDS and read from global memory, a grouped scene, the simple HitSpheres, both folds, light
sampling off; the largest and tiny spans, the largest fisheye angle, an orthographic window inside a sphere; progressive frames onto
noise and a plain draw over garbage; the counter word and guard rows.  A 1-spp draw is tptTraceRaysDevice on the lens's rays, the device's
sin / cos are the checker's on the lenses' argument domain, and tptDrawDevice after a lens draw is what it was before."""
import numpy as np
import pytest

from lens_lib import EQUIRECT, FISHEYE, FOLD_FORWARD, FOLD_RECURSIVE, KINDS, ORTHO, PI, TWO_PI, LensChecker, default_scene, grouped_scene
from lens_lib import make_lens, noise_tile, to_api

pytestmark = pytest.mark.gpu
SIZES = [(24, 16), (37, 19), (1, 1), (300, 3)]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return LensChecker(tmp_path_factory.mktemp("lens_checker"))


def draw(tpt, lens, w, h, frame=0, flags=0, start=None, counted=True):
    """the call on a tile with a guard row of NaN below and above (`start`: the tile's contents before, zeros if None) and a guard word
    either side of the counter -> (tile [h, w, 4], counter's gain)"""
    import torch
    buf = np.full((h + 2, w, 4), np.nan, np.float32)
    buf[1:-1] = 0 if start is None else start
    tile = torch.from_numpy(buf).cuda()
    cnt = torch.tensor([5, 1000, 5], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    r0 = tpt.ray_counter_read()
    tpt.draw_device_lens(frame, w, h, tile.data_ptr() + 16 * w, to_api(lens), flags, cnt.data_ptr() + 8 if counted else None)
    tpt.synchronize()
    assert tpt.ray_counter_read() == r0, "the context's ray counter moved"
    out, c = tile.cpu().numpy(), cnt.cpu().numpy().tolist()
    assert np.isnan(out[0]).all() and np.isnan(out[-1]).all(), "a guard row was written"
    assert c[0] == 5 and c[2] == 5 and (counted or c[1] == 1000), c
    return out[1:-1], c[1] - 1000


def same(got, want, what):
    tile, rays = got
    want_rays, want_tile = want
    if tile.tobytes() != want_tile.tobytes():
        bad = np.argwhere(tile.view(np.uint32) != want_tile.view(np.uint32))
        raise AssertionError("%s: %d words differ, first at %s: %r / %r" % (what, len(bad), bad[0], tile[tuple(bad[0][:2])], want_tile[tuple(bad[0][:2])]))
    assert rays == want_rays, (what, rays, want_rays)


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_sizes_and_samples(tpt_defaults, checker, kind, size, spp):
    tpt = tpt_defaults
    w, h = size
    s, m = default_scene()
    lens = make_lens(KINDS[kind])
    tpt.set_samples_per_pixel(spp)
    tpt.UpdateTest(0.0, 0, w, h, 0)
    same(draw(tpt, lens, w, h, frame=2), checker.render(s, m, lens, w, h, spp, 2), "%s %dx%d spp %d" % (kind, w, h, spp))


VARIANTS = {
    "global-memory": dict(lds=0),
    "grouped": dict(scene="grouped"),
    "simple": dict(hs=1),
    "grouped-simple": dict(scene="grouped", hs=1),
    "forward": dict(fold=FOLD_FORWARD),
    "forward-global": dict(fold=FOLD_FORWARD, lds=0),
    "no-light-sampling": dict(light_sampling=False),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_scenes_and_variants(tpt_defaults, checker, kind, variant):
    tpt = tpt_defaults
    v = dict(scene="default", hs=0, lds=-1, fold=FOLD_RECURSIVE, light_sampling=True)
    v.update(VARIANTS[variant])
    w, h, spp = 37, 19, 4
    s, m = default_scene() if v["scene"] == "default" else grouped_scene()
    if v["scene"] != "default":
        tpt.set_scene(s, m)
    tpt.set_kernel_variant(v["hs"], 3, v["lds"])
    tpt.set_fold_mode(v["fold"])
    tpt.set_config(light_sampling=v["light_sampling"])
    tpt.UpdateTest(0.0, 0, w, h, 0)
    assert (tpt.scene_info()["groups"] > 0) == (v["scene"] == "grouped" and len(s) >= 300)
    lens = make_lens(KINDS[kind], origin=(0.0, 1.0, 0.5) if v["scene"] == "default" else (0.2, 0.1, -0.3))
    want = checker.render(s, m, lens, w, h, spp, 1, fold=v["fold"], light_sampling=v["light_sampling"])
    same(draw(tpt, lens, w, h, frame=1), want, "%s %s" % (kind, variant))


def _inside_lens():
    s, _ = default_scene()
    glass = 7  # the glass sphere of the built-in scene (Test.cpp:13-31)
    r = float(s["radius"][glass])
    return make_lens(ORTHO, origin=(float(s["cx"][glass]), float(s["cy"][glass]), float(s["cz"][glass])), forward=(0.3, -0.2, -1.0),
                     sx=0.8 * r, sy=0.8 * r)


SPANS = {
    "equirect-2pi-by-pi": lambda: make_lens(EQUIRECT, sx=TWO_PI, sy=PI, forward=(0.3, -0.5, -0.8), up=(0.1, 1.0, 0.2)),
    "equirect-1e-3": lambda: make_lens(EQUIRECT, sx=1e-3, sy=1e-3),
    "fisheye-largest-angle": lambda: make_lens(FISHEYE, sx=4.0, sy=4.0, max_angle=PI),
    "fisheye-1e-3": lambda: make_lens(FISHEYE, sx=1e-3, sy=1e-3, max_angle=PI),
    "ortho-inside-a-sphere": _inside_lens,
    "ortho-1e-3": lambda: make_lens(ORTHO, sx=1e-3, sy=1e-3),
}


@pytest.mark.parametrize("name", sorted(SPANS))
def test_spans_and_places(tpt_defaults, checker, name):
    tpt = tpt_defaults
    w, h, spp = 37, 19, 4
    s, m = default_scene()
    lens = SPANS[name]()
    tpt.UpdateTest(0.0, 0, w, h, 0)
    want = checker.render(s, m, lens, w, h, spp, 0)
    same(draw(tpt, lens, w, h), want, name)
    assert (want[1][..., :3] > 0).any()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_progressive_frames_onto_noise_keep_the_alpha(tpt_defaults, checker, kind):
    tpt = tpt_defaults
    w, h, spp = 37, 19, 4
    s, m = default_scene()
    lens = make_lens(KINDS[kind])
    tpt.UpdateTest(0.0, 0, w, h, 0)
    got = want = noise_tile(w, h)
    for frame in range(3):
        want_rays, want = checker.render(s, m, lens, w, h, spp, frame, flags=2, backbuffer=want.copy())
        got, rays = draw(tpt, lens, w, h, frame=frame, flags=2, start=got)
        same((got, rays), (want_rays, want), "%s frame %d" % (kind, frame))
    assert (got[..., 3] == noise_tile(w, h)[..., 3]).all() and np.isfinite(got).all()


def test_a_plain_draw_over_garbage(tpt_defaults, checker):
    """without TPT_FLAG_PROGRESSIVE lerp is 0 whatever the frame: prev is read, multiplied by 0 and added (finite garbage: the bytes of
    0 * prev + colour), the alpha is the garbage's"""
    tpt = tpt_defaults
    w, h, spp = 37, 19, 4
    s, m = default_scene()
    lens = make_lens(FISHEYE)
    garbage = (np.random.default_rng(9).uniform(-1, 1, (h, w, 4)) * 3e38).astype(np.float32)
    tpt.UpdateTest(0.0, 0, w, h, 0)
    want = checker.render(s, m, lens, w, h, spp, 7, flags=0, backbuffer=garbage.copy())
    got = draw(tpt, lens, w, h, frame=7, flags=0, start=garbage, counted=False)
    same((got[0], want[0]), want, "garbage")
    assert (got[0][..., 3] == garbage[..., 3]).all()


@pytest.mark.parametrize("frame", [0, 5])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_one_sample_is_the_ray_call_on_the_lens_rays(tpt_defaults, checker, kind, frame):
    """three ways to the same bytes: the draw at 1 spp on a zeroed tile, tptTraceRaysDevice on the rays the checker says the first
    samples start with, and (test_sizes_and_samples) the checker's render"""
    import torch
    tpt = tpt_defaults
    w, h = 37, 19
    lens = make_lens(KINDS[kind])
    tpt.set_samples_per_pixel(1)
    tpt.UpdateTest(0.0, 0, w, h, 0)
    tile, rays = draw(tpt, lens, w, h, frame=frame)
    d_rays = torch.from_numpy(checker.rays(lens, w, h, frame)).cuda()
    rad = torch.full((h * w, 4), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tpt.trace_rays_device(h * w, d_rays.data_ptr(), rad.data_ptr(), None, None)
    tpt.synchronize()
    rad = rad.cpu().numpy()
    assert tile[..., :3].tobytes() == rad.reshape(h, w, 4)[..., :3].tobytes() and (tile[..., 3] == 0).all()
    assert rays == int(rad[:, 3].astype(np.int64).sum()) and rays >= h * w


def lens_arguments():
    """the arguments the lenses hand to sin / cos: both signs of the 64 neighbours either side of 2^-12, pi / 4 and n pi / 2 (n <= 6), and
    of 2^20 evenly spaced bit patterns of [2^-13, 9]"""
    points = [np.float32(2.0 ** -12), np.float32(np.pi / 4)] + [np.float32(n * np.pi / 2) for n in range(1, 7)]
    near = np.concatenate([(p.view(np.uint32).astype(np.int64) + np.arange(-64, 65)).astype(np.uint32).view(np.float32) for p in points])
    lo, hi = int(np.float32(2.0 ** -13).view(np.uint32)), int(np.float32(9.0).view(np.uint32))
    spaced = np.linspace(lo, hi, 1 << 20).astype(np.uint32).view(np.float32)
    x = np.concatenate([near, spaced, np.float32([0.0])])
    return np.concatenate([x, -x])


def test_device_sincos_on_the_lens_domain(tpt_hooks, checker):
    """tptTestMath ops 8 / 9 (the sine / cosine of tsincosf) against tptm_sinf / tptm_cosf: the exhaustive device test covers the 2^24
    non-negative arguments of the path only; the lenses add negative angles and everything up to 9"""
    x = lens_arguments()
    assert x.min() < -8.9 and x.max() > 8.9 and np.isfinite(x).all() and len(x) > 2 << 20
    want_s, want_c = checker.sincos(x)
    got_s, got_c = tpt_hooks.test_math(8, x), tpt_hooks.test_math(9, x)
    for got, want, name in ((got_s, want_s, "sin"), (got_c, want_c, "cos")):
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert len(bad) == 0, (name, len(bad), x[bad[:4]], got[bad[:4]], want[bad[:4]])


def test_draw_device_after_a_lens_draw_is_what_it_was(tpt_defaults, checker):
    import torch
    tpt = tpt_defaults
    w, h = 64, 40
    s, m = default_scene()

    def frames():
        tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r0 = tpt.ray_counter_read()
        for f in range(3):
            tpt.UpdateTest(0.0, f, w, h, 2)
            tpt.draw_device(0.0, f, w, h, tile.data_ptr(), 2)
        tpt.synchronize()
        return tile.cpu().numpy().tobytes(), tpt.ray_counter_read() - r0

    before = frames()
    for kind in sorted(KINDS):
        lens = make_lens(KINDS[kind])
        same(draw(tpt, lens, 37, 19, frame=1), checker.render(s, m, lens, 37, 19, 4, 1), kind)
    assert frames() == before
