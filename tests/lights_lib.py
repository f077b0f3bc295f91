"""TEST INFRASTRUCTURE: scenes whose LIGHT LIST is the subject -- how many emissive spheres there are and of what kind -- for
tests/test_gpu_lights.py (the trace kernels on the GPU) and tests/test_lights_plan.py (the host's plan on the emulation build).  Every
builder is seeded and returns (spheres, materials) in oracle_lib's record layouts; nothing under toypathtracer_amd/ imports this module.

Every scene here renders to a finite image with the oracle (tests/test_lights_plan.py asserts it for each, on the CPU), so byte equality
is a fair demand everywhere -- also for a light that encloses shading points: there 1 - r^2/d^2 < 0, the cone's cosine is NaN and the
shadow ray hits nothing."""
import numpy as np

from oracle_lib import Oracle

LAMBERT, METAL, DIELECTRIC = 0, 1, 2
DEFAULT_LIGHTS = (8, 45)  # the built-in scene's own emissive spheres (Test.cpp:13-31)
LIGHT_KINDS = ("metal", "glass", "ground", "enclosing", "tiny", "huge", "coincident", "one-channel", "mixed-sign", "black-albedo")
LIGHT_COUNTS = (0, 1, 15, 16, 17, 46)


def _finish(s, m):
    s["invRadius"] = np.float32(1.0) / s["radius"]
    return s, m


def light_ids(m):
    """the spheres the library and the oracle sample as lights: a positive emissive channel (Test.cpp:334)"""
    return [int(i) for i in np.nonzero((m["emissive"] > 0).any(axis=1))[0]]


def default_with_lights(k, seed=1):
    """The built-in 46 spheres with exactly k emissive ones, colours random in [0.5, 8): for k < 46 spheres 1..k -- so Lambert, metal
    (3..6) and glass (7) spheres become lights, and for k >= 8 both spheres kFlagAnimate moves (1 and 8) --, for k == 46 every sphere,
    the ground included."""
    assert 0 <= k <= 46
    s, m = Oracle.get().default_scene()
    rng = np.random.default_rng(seed)
    colours = rng.uniform(0.5, 8.0, (46, 3)).astype(np.float32)
    m["emissive"][:] = 0
    ids = np.arange(46) if k == 46 else np.arange(1, k + 1)
    m["emissive"][ids] = colours[ids]
    assert light_ids(m) == ids.tolist()
    return _finish(s, m)


def light_kind(name):
    """The built-in scene (lights: spheres 8 and 45) changed in one way.  `tiny` and `huge` have a light whose r^2 lies outside
    [2^-60, 2^60]: the packed scene loses SCENE_LIGHT_R2_DIV_SAFE and the light ray's r^2 / d^2 takes the plain division."""
    s, m = Oracle.get().default_scene()
    assert light_ids(m) == list(DEFAULT_LIGHTS), "the built-in scene's lights moved: tests/lights_lib.py is written for 8 and 45"
    f = np.float32
    if name == "metal":
        assert m["type"][5] == METAL
        m["emissive"][5] = (4.0, 3.0, 2.0)
    elif name == "glass":
        assert m["type"][7] == DIELECTRIC
        m["emissive"][7] = (4.0, 3.0, 2.0)
    elif name == "ground":
        assert s["radius"][0] == 100
        m["emissive"][0] = (0.25, 0.25, 0.25)
    elif name == "enclosing":
        s["radius"][8] = f(3.0)
    elif name == "tiny":
        s["radius"][45] = f(2.0 ** -31)
    elif name == "huge":
        s["radius"][45] = f(2.0 ** 31)
        s["cz"][45] = f(-(2.0 ** 32))
    elif name == "coincident":
        for k in ("cx", "cy", "cz", "radius"):
            s[k][45] = s[k][8]
    elif name == "one-channel":
        m["emissive"][8] = (0.0, 0.0, 5.0)
    elif name == "mixed-sign":
        m["emissive"][8] = (-1.0, 0.0, 5.0)
    elif name == "black-albedo":
        m["albedo"][8] = 0
    else:
        raise KeyError(name)
    return _finish(s, m)


def r2_div_safe(s, m):
    """SCENE_LIGHT_R2_DIV_SAFE as packScene sets it (csrc/tpt_scene.h): every light's float32 r * r lies in [2^-60, 2^60]"""
    r2 = (s["radius"][light_ids(m)] * s["radius"][light_ids(m)]).astype(np.float32)
    return bool(((r2 >= np.float32(2.0 ** -60)) & (r2 <= np.float32(2.0 ** 60))).all())


def stress_with_lights(n, grid, k):
    """toypathtracer_amd.scenes.stress_scene(n, grid) with every emissive colour cleared and spheres 1..k given (0.5, 0.4, 0.3): k
    dim lights all over the lattice, next to the shading points (spheres 1..4 keep their place above it)."""
    from toypathtracer_amd.scenes import stress_scene
    assert 0 <= k < n
    s, m = stress_scene(n, grid)
    m["emissive"][:] = 0
    m["emissive"][1:k + 1] = (0.5, 0.4, 0.3)
    assert len(light_ids(m)) == k
    return _finish(s, m)
