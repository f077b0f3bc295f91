"""tptDrawDeviceLens without a GPU: the declaration, binding and export; the binding's argument checks; the structs' layout; lensGetRay of
csrc/tpt_trace.h compiled for the host against tests/lens_checker.c bit for bit; the code object's kernel set (no kernel of its own);
and, through the host runtime compiled against tests/hostemu with tests/hostemu_lens.cpp as the launcher, every refusal (no operation
run, no byte written) and the accepted draws held byte for byte against the checker; the binding's and the library's statements of the
basis rules held together a step either side of every bound; and the launch's plan -- chunk size, shift and count, the grid -- on both
sides of the seam between 8 x 8 tiles and chunks of 256 pixels and at 8192 x 8192 (tests/lens_kinds_lib.py has the records and sizes)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from isa_lib import code_object, exported_symbols, header, header_params, no_library, refusal_messages, run_refusals  # noqa: F401  (code_object: a fixture)
from kernel_manifest import TRACE, family
from lens_lib import EQUIRECT, FISHEYE, ORTHO, PI, TWO_PI, Lens, LensChecker, make_lens
from oracle_lib import ROOT

NAME = "tptDrawDeviceLens"
CTYPES_OF = {"int": C.c_int, "unsigned": C.c_uint, "float": C.c_float}


def struct_fields(name):
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), header(), flags=re.S)
    assert body, "%s is not declared in include/tpt_hip.h" % name
    fields = []
    for decl in body.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ctype, names = re.match(r"(.*?[\s*])(\w[\w\[\], ]*)$", decl).groups()
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
            fields.append((m.group(1), ctype.strip(), int(m.group(2)) if m.group(2) else 0))
    return fields


def test_header_declares_the_entry_point_and_states_it():
    from toypathtracer_amd import api
    assert header_params(NAME) == ["const tptDrawLensArgs* args"]
    lens = struct_fields("tptLens")
    assert lens == [("kind", "int", 0), ("origin", "float", 3), ("right", "float", 3), ("up", "float", 3), ("forward", "float", 3),
                    ("sx", "float", 0), ("sy", "float", 0), ("maxAngle", "float", 0)]
    args = struct_fields("tptDrawLensArgs")
    assert args == [("screenWidth", "int", 0), ("screenHeight", "int", 0), ("frameCount", "int", 0), ("flags", "unsigned", 0),
                    ("lens", "tptLens", 0), ("deviceTile", "float*", 0), ("deviceRayCount", "unsigned long long*", 0)]
    for fields, mirror in ((lens, api.Lens), (args, api.DrawLensArgs)):
        assert [n for n, _, _ in fields] == [n for n, _ in mirror._fields_]
        for (name, ctype, dim), (_, m) in zip(fields, mirror._fields_):
            want = C.c_void_p if ctype.endswith("*") else (api.Lens if ctype == "tptLens" else CTYPES_OF[ctype])
            assert m is want or (dim and m._type_ is want and m._length_ == dim), (name, ctype, m)
    assert re.search(r"enum\s*\{\s*TPT_LENS_EQUIRECT\s*=\s*1\s*,\s*TPT_LENS_FISHEYE\s*=\s*2\s*,\s*TPT_LENS_ORTHO\s*=\s*3\s*\}", header())
    assert (api.LENS_EQUIRECT, api.LENS_FISHEYE, api.LENS_ORTHO) == (1, 2, 3)
    text = open(os.path.join(ROOT, "include", "tpt_hip.h")).read()
    doc = text[text.index("OTHER LENSES"):text.index("enum { TPT_LENS_EQUIRECT")]
    for words in ("Binary32, in the order written, no FMA, correctly rounded division and square root", "x*1973 + y*9277 + frameCount*26699",
                  "right*(cb*sa) + up*sb + forward*(cb*ca)", "k = r > 0 ? st / r : 0.0f", "(origin + right*a) + up*b", "normalize(q)",
                  "1.0f / (float)spp", "the alpha is untouched", "tptRayCounterRead", "Refused", "0.99..1.01", "6.2831855f",
                  "TPT_MAX_LIGHTS", "whatever tptSetSeedMode says", "no aperture"):
        assert words in doc, words


def test_struct_layout_matches_the_ctypes_mirror(tmp_path):
    from toypathtracer_amd import api
    probes = [("tptLens", api.Lens), ("tptDrawLensArgs", api.DrawLensArgs)]
    src = tmp_path / "layout.c"
    lines = []
    for cname, mirror in probes:
        lines.append('    printf("%%zu\\n", sizeof(%s));\n' % cname)
        lines += ['    printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, n) for n, _ in mirror._fields_]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tpt_hip.h"\nint main(void) {\n' + "".join(lines) + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    want = []
    for _, mirror in probes:
        want += [C.sizeof(mirror)] + [getattr(mirror, n).offset for n, _ in mirror._fields_]
    assert got == want
    assert C.sizeof(api.Lens) == 64 == C.sizeof(Lens) and C.sizeof(api.DrawLensArgs) == 96


def test_binding_and_export():
    from toypathtracer_amd import api
    lib = api.load_library()
    assert NAME in api.C_ABI_SYMBOLS and hasattr(lib, NAME) and callable(api.draw_device_lens)
    assert re.search(r"\bT %s\b" % NAME, exported_symbols(api.library_path()))
    assert re.search(r"^\s*tpt\*;", open(os.path.join(ROOT, "toypathtracer_amd", "csrc", "exports.map")).read(), flags=re.M)


def test_the_lens_builders_make_an_orthonormal_right_handed_basis():
    from toypathtracer_amd import api
    for make in (api.lens_equirect, api.lens_fisheye, api.lens_ortho):
        lens = make(origin=(1, 2, 3), forward=(0.3, -0.5, -2.0), up=(0.1, 3.0, 0.2))
        r, u, f = (np.array(v[:], np.float64) for v in (lens.right, lens.up, lens.forward))
        assert np.allclose([r @ r, u @ u, f @ f], 1, atol=1e-6) and np.allclose([r @ u, r @ f, u @ f], 0, atol=1e-6)
        assert np.allclose(np.cross(f, u), r, atol=1e-6) and u[1] > 0 and tuple(lens.origin[:]) == (1.0, 2.0, 3.0)
    lens = api.lens_equirect(forward=(0, 0, -1), up=(0, 1, 0))
    assert (tuple(lens.right[:]), tuple(lens.up[:]), tuple(lens.forward[:])) == ((1, 0, 0), (0, 1, 0), (0, 0, -1))
    assert lens.kind == 1 and lens.sx == np.float32(6.2831855) and lens.sy == np.float32(3.1415927) and lens.maxAngle == 0
    assert api.lens_fisheye().kind == 2 and api.lens_ortho().kind == 3
    for bad in (dict(forward=(0, 0, 0)), dict(up=(0, 0, -2), forward=(0, 0, -1)), dict(origin=(np.nan, 0, 0)), dict(forward=(1, 2))):
        with pytest.raises(ValueError):
            api.lens_equirect(**bad)


def _api_lens(**kw):
    from toypathtracer_amd import api
    lens = api.lens_equirect()
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(lens, k)[:] = v
        else:
            setattr(lens, k, v)
    return lens


LENS_FAULTS = [
    dict(kind=0), dict(kind=4), dict(kind=-1), dict(origin=(np.nan, 0, 0)), dict(right=(np.inf, 0, 0)), dict(sx=np.nan), dict(sy=np.inf),
    dict(maxAngle=np.nan), dict(right=(1.006, 0, 0)), dict(up=(0, 0.994, 0)), dict(forward=(0, 0, 0)), dict(up=(0.011, 1, 0)),
    dict(forward=(0, 0.011, -1)), dict(forward=(0.011, 0, -1)), dict(sx=0.0), dict(sy=-1.0), dict(sx=6.2831860), dict(sy=3.1415930),
    dict(maxAngle=0.5), dict(kind=3, maxAngle=1e-9), dict(kind=2, maxAngle=0.0), dict(kind=2, maxAngle=3.1415930),
    dict(kind=2, maxAngle=-1.0), dict(kind=2, maxAngle=1.0, sx=4.0000005, sy=1.0), dict(kind=2, maxAngle=1.0, sx=1.0, sy=4.5),
]


@pytest.mark.parametrize("args", [
    dict(w=0), dict(w=8193), dict(w=2.0), dict(w=True), dict(h=0), dict(h=-3), dict(h=8193), dict(h=None), dict(frame=-1), dict(frame=1.0),
    dict(frame=True), dict(frame=2 ** 31), dict(flags=1), dict(flags=3), dict(flags=4), dict(flags=True), dict(flags=None), dict(tile=0),
    dict(tile=None), dict(tile=-16), dict(tile=1.5), dict(tile="t"), dict(count=-1), dict(count=2.5), dict(count=True),
    dict(count=4096 + 8), dict(count=4096 + 16 * 16 * 8 - 1), dict(count=4096 - 7), dict(lens=None), dict(lens="equirect"),
    dict(lens=Lens()),
] + [dict(lens_fault=f) for f in LENS_FAULTS], ids=lambda a: ",".join("%s=%.40r" % (k, "Lens()" if isinstance(v, Lens) else v) for k, v in a.items()))
def test_binding_checks_arguments_before_the_library(monkeypatch, args):
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    a = dict(frame=0, w=16, h=8, tile=4096, lens=api.lens_equirect(), flags=0, count=None)
    if "lens_fault" in args:
        a["lens"] = _api_lens(**args["lens_fault"])
    else:
        a.update(args)
    with pytest.raises(ValueError):
        api.draw_device_lens(a["frame"], a["w"], a["h"], a["tile"], a["lens"], a["flags"], a["count"])


def test_the_binding_passes_what_the_library_accepts(monkeypatch):
    """the limits themselves are not refused: the call reaches the library"""
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    for lens in (api.lens_equirect(), api.lens_equirect(lon_span=1e-3, lat_span=1e-3), api.lens_fisheye(max_angle=3.1415927, sx=4.0, sy=4.0),
                 api.lens_ortho(), _api_lens(right=(1.004, 0, 0)), _api_lens(up=(0.009, 1, 0))):
        for kw in (dict(), dict(count=4096 + 16 * 8 * 16), dict(count=4096 - 8), dict(flags=2, frame=2 ** 31 - 1), dict(w=8192, h=1)):
            a = dict(frame=0, w=16, h=8, tile=4096, flags=0, count=None)
            a.update(kw)
            with pytest.raises(AssertionError, match="the library was called"):
                api.draw_device_lens(a["frame"], a["w"], a["h"], a["tile"], lens, a["flags"], a["count"])


# ---------------------------------------------------------------- lensGetRay, compiled for the host, against the checker
HOST_RAY = r'''
#include "tpt_trace.h"
static_assert(sizeof(tpt::LensPOD) == 64, "tptLens word for word");
extern "C" void host_lens_rays(const tpt::LensPOD* lens, int n, const float* uv, float* out6)
{
    for (int i = 0; i < n; ++i) {
        tpt::f3 o, d;
        tpt::lensGetRay(*lens, uv[2 * i], uv[2 * i + 1], o, d);
        float* p = out6 + 6 * (size_t)i;
        p[0] = o.x; p[1] = o.y; p[2] = o.z; p[3] = d.x; p[4] = d.y; p[5] = d.z;
    }
}
'''
TARGETS = [2.0 ** -12, np.pi / 4] + [n * np.pi / 2 for n in range(1, 6)]


def neighbours(x, steps=3):
    out, lo, hi = [np.float32(x)], np.float32(x), np.float32(x)
    for _ in range(steps):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return out


def ray_grid(lens):
    """(u, v) in [0, 1): 0, 0.5 and the largest float below 1 in every pairing, and around every point where a, b (along an axis) or
    r * maxAngle (along an axis and along both diagonals) meets +-2^-12, +-pi/4 or +-n pi/2, n = 1..5, as far as the lens reaches them"""
    one = np.nextafter(np.float32(1), np.float32(0))
    uv = [(u, v) for u in (np.float32(0), np.float32(0.5), one) for v in (np.float32(0), np.float32(0.5), one)]
    scale = lens.maxAngle if lens.kind == FISHEYE else 1.0  # (the angle per unit of a or b)
    for t in TARGETS:
        for sign in (1.0, -1.0):
            du, dv = sign * t / (scale * lens.sx), sign * t / (scale * lens.sy)
            axis = [(0.5 + du, 0.5), (0.5, 0.5 + dv)]
            diag = [(0.5 + du / np.sqrt(2), 0.5 + dv / np.sqrt(2)), (0.5 + du / np.sqrt(2), 0.5 - dv / np.sqrt(2))] if lens.kind == FISHEYE else []
            for u0, v0 in axis + diag:
                if 0 <= u0 < 1 and 0 <= v0 < 1:
                    uv += [(u, np.float32(v0)) for u in neighbours(u0)] + [(np.float32(u0), v) for v in neighbours(v0)]
    uv = np.array([p for p in uv if 0 <= p[0] < 1 and 0 <= p[1] < 1], np.float32)
    return np.unique(uv, axis=0)


def angles(lens, uv):
    """the binary32 arguments of sin / cos the contract makes of uv: (a, b), or r * maxAngle"""
    a, b = (uv[:, 0] - np.float32(0.5)) * np.float32(lens.sx), (uv[:, 1] - np.float32(0.5)) * np.float32(lens.sy)
    if lens.kind == FISHEYE:
        return [np.sqrt(a * a + b * b) * np.float32(lens.maxAngle)]
    return [a, b]


GRID_LENSES = {
    # (lens, the targets each argument reaches from both sides -- a and b, or r * maxAngle; b of the full span stops short of pi / 2)
    "equirect-largest": (dict(kind=EQUIRECT, sx=TWO_PI, sy=PI), [[2.0 ** -12, np.pi / 4, np.pi / 2], [2.0 ** -12, np.pi / 4]]),
    "equirect-tiny": (dict(kind=EQUIRECT, sx=1e-3, sy=1e-3, forward=(0.3, -0.5, -0.8)), [[2.0 ** -12], [2.0 ** -12]]),
    "fisheye-largest": (dict(kind=FISHEYE, sx=4.0, sy=4.0, max_angle=PI, forward=(0.3, -0.5, -0.8)), [TARGETS]),
    "fisheye-tiny": (dict(kind=FISHEYE, sx=1e-3, sy=1e-3, max_angle=PI), [[2.0 ** -12]]),
    "fisheye-tiny-angle": (dict(kind=FISHEYE, sx=2.0, sy=2.0, max_angle=1e-3), [[2.0 ** -12]]),
    "ortho-largest": (dict(kind=ORTHO, sx=1e4, sy=1e4, forward=(0.3, -0.5, -0.8)), [[], []]),
    "ortho-tiny": (dict(kind=ORTHO, sx=1e-3, sy=1e-3), [[], []]),
}


@pytest.fixture(scope="module")
def host_ray(tmp_path_factory):
    d = tmp_path_factory.mktemp("lens_host_ray")
    src, so = d / "host_ray.cpp", str(d / "libhost_ray.so")
    src.write_text(HOST_RAY)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "toypathtracer_amd", "csrc"), str(src), "-o", so])
    lib = C.CDLL(so)
    lib.host_lens_rays.restype = None
    lib.host_lens_rays.argtypes = [C.POINTER(Lens), C.c_int, C.c_void_p, C.c_void_p]
    return lib, LensChecker(d)


@pytest.mark.parametrize("name", sorted(GRID_LENSES))
def test_lens_get_ray_on_the_host_is_the_checker_bit_for_bit(host_ray, name):
    lib, checker = host_ray
    kw, reached = GRID_LENSES[name]
    lens = make_lens(**kw)
    uv = ray_grid(lens)
    # the grid does what it says: every target the lens reaches has arguments on both sides of it, in both signs
    for arg, targets in zip(angles(lens, uv), reached):
        for t in targets:
            signs = (1.0,) if lens.kind == FISHEYE else (1.0, -1.0)  # (r * maxAngle is never negative)
            for s in signs:
                # (a step of u or v near 1 moves the argument by 2^-24 x the span x the angle per unit: "around" is a few of those)
                step = 2.0 ** -23 * max(lens.sx, lens.sy) * (lens.maxAngle if lens.kind == FISHEYE else 1.0)
                near = arg[np.abs(arg.astype(np.float64) - s * t) <= 5 * step + 8 * np.spacing(np.float32(t))]
                assert (near.astype(np.float64) < s * t).any() and (near.astype(np.float64) > s * t).any(), (name, s * t, near)
    got = np.full((len(uv), 6), np.nan, np.float32)
    lib.host_lens_rays(C.byref(lens), len(uv), uv.ctypes.data, got.ctypes.data)
    want = checker.ray_grid(lens, uv)
    assert np.isfinite(want).all()
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError("%s: %d of %d words differ, first at uv %r: %r / %r" % (name, len(bad), got.size, uv[bad[0][0]], got[bad[0][0]],
                                                                                   want[bad[0][0]]))
    print("%s: %d rays equal" % (name, len(uv)))


# ---------------------------------------------------------------- the code object
def test_the_code_object_has_no_kernel_of_its_own(code_object):  # noqa: F811
    """the lens is a mode of the lane-refill kernel: its eight instantiations and nothing named after lenses (the whole set:
    tests/test_isa_contract.py holds the library to exactly tests/kernel_manifest.py)"""
    import kernel_manifest
    bodies, meta = code_object
    assert sorted(n for n in meta if "tptTraceKernel" in n) == sorted(family(TRACE))
    assert set(meta) == kernel_manifest.ALL
    assert not [n for n in meta if re.search(r"lens", n, flags=re.I) and "tptTrace" not in n]


# ---------------------------------------------------------------- the host runtime on the emulated device
SCRIPT = r'''
import ctypes as C, os, sys, tempfile
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from toypathtracer_amd import api as tpt
from toypathtracer_amd.scenes import cloud_scene
from lens_lib import EQUIRECT, FISHEYE, ORTHO, KINDS, PI, TWO_PI, LensChecker, make_lens, noise_tile, to_api
REFUSALS = sys.argv[2] == "refusals"
lib = tpt.load_library()
so = C.CDLL(tpt.library_path())
checker = LensChecker(tempfile.mkdtemp(prefix="lens_abi_"))
ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
def msg(): return lib.tptGetLastError().decode()
def ops():
    st = (C.c_longlong * 2)(); so.hostemu_stats(st); return st[0]
def raw(w, h, frame, flags, lens, tile, count):
    a = tpt.DrawLensArgs(screenWidth=w, screenHeight=h, frameCount=frame, flags=flags, lens=to_api(lens), deviceTile=ptr(tile), deviceRayCount=ptr(count))
    return lib.tptDrawDeviceLens(C.byref(a))
W, H = 16, 8
if sys.argv[2] == "bounds":
    # every bound of the basis rules, a step inside and a step outside, through the C call and the binding's own statement of the
    # rules with the same records: both accept, or both refuse -- the C call with the message, nothing enqueued and nothing written
    import lens_kinds_lib
    tpt.InitializeTest()
    tpt.UpdateTest(0.0, 0, W, H, 0)
    tpt.synchronize()
    s, m = tpt.GetSceneDesc()[:2]
    tpt.set_samples_per_pixel(1)
    for name, lens, inside, message in lens_kinds_lib.bound_records():
        tile, tile2 = (np.full((H, W, 4), 7.0, np.float32) for _ in range(2))  # (finite: a plain draw adds 0 * what was there)
        tpt.synchronize()
        ops0 = ops()
        rc = raw(W, H, 0, 0, lens, tile, None)
        said = msg()
        try:
            tpt.draw_device_lens(0, W, H, ptr(tile2), to_api(lens))
            binding = True
        except ValueError as e:
            binding = False
            assert ("unit length" in str(e)) == ("unit length" in message) and ("orthogonal" in str(e)) == ("orthogonal" in message), (name, e)
        assert (rc == 0) == binding == inside, (name, rc, binding, inside, said)
        tpt.synchronize()
        if inside:
            want = checker.render(s, m, lens, W, H, 1, backbuffer=np.full((H, W, 4), 7.0, np.float32))[1].tobytes()
            assert tile.tobytes() == want and tile2.tobytes() == want and (tile[..., :3] != 7).any(), name
        else:
            assert said == "tptDrawDeviceLens: " + message, (name, said)
            assert ops() == ops0 and (tile == 7).all() and (tile2 == 7).all(), (name, "a refused call enqueued or wrote")
        print("bound: %s: %s" % (name, "accepted by both" if inside else "refused by both -- " + said))
    tpt.ShutdownTest()
    print("ok")
    sys.exit(0)
if sys.argv[2] == "plans":
    # what laneRefillChunks makes of an image on either side of the seam between 8 x 8 tiles and chunks of 256 pixels, and of the
    # largest image: KernelArgs and the grid as the launcher gets them (hostemuLensPlan), on a device whose CUs HOSTEMU_CUS names
    import lens_kinds_lib
    tpt.InitializeTest()
    tpt.UpdateTest(0.0, 0, W, H, 0)
    plan = (C.c_longlong * 8)()
    small = np.zeros((8, 8, 4), np.float32)
    tpt.set_samples_per_pixel(4)
    tpt.draw_device_lens(0, 8, 8, ptr(small), to_api(make_lens(EQUIRECT)))
    tpt.synchronize()
    so.hostemuLensPlan(plan)
    assert list(plan)[:5] == [64, 64, 6, 1, 1] and plan[6] == 1, list(plan)
    resident = lens_kinds_lib.emulated_resident(int(os.environ["HOSTEMU_CUS"]), plan[5])
    above, under = lens_kinds_lib.seam_sizes(resident)
    so.hostemuLensPlanOnly(1)  # the launcher records the plan and runs nothing: the call fails after its planning, the tile is not touched
    for (w, h), chunk in ((under, 64), (above, 256), ((8192, 8192), 256), ((8192, 8), 256 if 1024 * 64 >= 2048 * resident else 64)):
        assert raw(w, h, 0, 0, make_lens(FISHEYE), small, None) != 0 and "tptLaunchTraceLens" in msg(), msg()
        so.hostemuLensPlan(plan)
        items = lens_kinds_lib.items_of(w, h)
        chunks = (items + chunk - 1) // chunk
        want = [items, chunk, {64: 6, 256: 8}[chunk], chunks, min(chunks, resident), plan[5], (w + 7) // 8, chunks]
        assert list(plan) == want, ((w, h), list(plan), want)
        print("plan: %d x %d: %d items in %d chunks of %d (shift %d), %d workgroups of %d resident" % (w, h, items, chunks, chunk, plan[2], plan[4], resident))
    so.hostemuLensPlanOnly(0)
    assert lens_kinds_lib.items_of(*under) < 2048 * resident <= lens_kinds_lib.items_of(*above)
    tpt.draw_device_lens(0, 8, 8, ptr(small), to_api(make_lens(EQUIRECT)))  # and the context draws on
    tpt.synchronize()
    assert small.tobytes() == checker.render(tpt.GetSceneDesc()[0], tpt.GetSceneDesc()[1], make_lens(EQUIRECT), 8, 8, 4)[1].tobytes()
    tpt.ShutdownTest()
    print("ok")
    sys.exit(0)
if REFUSALS:
    count = np.full(4, 7, np.uint64)
    tile = np.full((H * W + 4, 4), np.nan, np.float32)
    def edited(lens, **kw):
        for k, v in kw.items():
            if isinstance(v, tuple): getattr(lens, k)[:] = v
            else: setattr(lens, k, v)
        return lens
    def refused(what, before_update=False, **kw):
        a = dict(w=W, h=H, frame=0, flags=0, lens=make_lens(EQUIRECT, forward=(0, 0, -1)), tile=tile, count=count)
        a.update(kw)
        tpt.synchronize()
        ops0 = ops()
        rc = raw(a["w"], a["h"], a["frame"], a["flags"], a["lens"], a["tile"], a["count"])
        assert rc != 0 and "tptDrawDeviceLens" in msg(), (what, rc, msg())
        tpt.synchronize()
        assert ops() == ops0, (what, "a refused call enqueued an operation")
        assert np.isnan(tile).all() and (count == 7).all(), (what, "a refused call wrote")
        print("refused:", what, "--", msg())
    rc = raw(W, H, 0, 0, make_lens(EQUIRECT), tile, count)
    assert rc != 0 and "not initialised" in msg(), msg()
    print("refused: no context --", msg())
    tpt.InitializeTest()
    refused("before any tptUpdate")
    tpt.UpdateTest(0.0, 0, W, H, 0)
    tpt.synchronize()
    assert lib.tptDrawDeviceLens(None) != 0 and "tptDrawDeviceLens" in msg()
    print("refused: args NULL --", msg())
    for w, h in ((0, H), (-1, H), (8193, H), (W, 0), (W, 8193), (W, -(1 << 31))):
        refused("size %d x %d" % (w, h), w=w, h=h)
    for frame in (-1, -(1 << 31)):
        refused("frameCount %d" % frame, frame=frame)
    for flags in (1, 3, 4, 0x80000000):
        refused("flags %#x" % flags, flags=flags)
    refused("deviceTile NULL", tile=None)
    b = tile.ctypes.data
    for what, c in (("the counter at the tile's head", b), ("the counter in the tile's last pixel", b + 16 * W * H - 8),
                    ("the counter's tail in the tile's head", b - 4), ("the counter's head in the tile's tail", b + 16 * W * H - 4)):
        refused("overlap: " + what, count=c)
    E, F, O = (lambda k=k, **kw: edited(make_lens(k, forward=(0, 0, -1)), **kw) for k in (EQUIRECT, FISHEYE, ORTHO))
    nan, inf = float("nan"), float("inf")
    faults = [("kind 0", E(kind=0)), ("kind 4", E(kind=4)), ("kind -1", E(kind=-1)),
              ("origin NaN", E(origin=(nan, 0, 0))), ("origin inf", O(origin=(0, inf, 0))), ("right inf", E(right=(inf, 0, 0))),
              ("up NaN", F(up=(0, nan, 0))), ("forward -inf", E(forward=(0, 0, -inf))), ("sx NaN", E(sx=nan)), ("sy inf", O(sy=inf)),
              ("maxAngle NaN", F(maxAngle=nan)), ("maxAngle inf", E(maxAngle=inf)),
              ("right too long", E(right=(1.006, 0, 0))), ("up too short", F(up=(0, 0.994, 0))), ("forward zero", O(forward=(0, 0, 0))),
              ("right . up", E(up=(0.011, 1, 0))), ("up . forward", F(forward=(0, 0.011, -1))), ("right . forward", O(forward=(0.011, 0, -1))),
              ("sx 0", E(sx=0.0)), ("sy negative", F(sy=-1.0)), ("sx -0", O(sx=-0.0)),
              ("equirect sx past 2 pi", E(sx=float(np.nextafter(np.float32(TWO_PI), np.float32(7))))),
              ("equirect sy past pi", E(sy=float(np.nextafter(np.float32(PI), np.float32(4))))),
              ("fisheye sx past 4", F(sx=float(np.nextafter(np.float32(4), np.float32(5))))), ("fisheye sy past 4", F(sy=4.5)),
              ("fisheye maxAngle 0", F(maxAngle=0.0)), ("fisheye maxAngle negative", F(maxAngle=-1.0)),
              ("fisheye maxAngle past pi", F(maxAngle=float(np.nextafter(np.float32(PI), np.float32(4))))),
              ("equirect with a maxAngle", E(maxAngle=0.5)), ("ortho with a maxAngle", O(maxAngle=1e-9))]
    for what, lens in faults:
        refused("lens: " + what, lens=lens)
    # two rules broken at once: the one that is checked first is the one reported
    def order(expect, **kw):
        refused("order", **kw)
        assert msg() == "tptDrawDeviceLens: " + expect, (expect, kw, msg())
        print("order:", sorted(kw), "--", expect)
    order("screenWidth and screenHeight must lie in 1..8192", w=0, frame=-1)
    order("frameCount must not be negative", frame=-1, flags=1)
    order("flags must be 0 or TPT_FLAG_PROGRESSIVE", flags=1, tile=None)
    order("deviceTile is required", tile=None, lens=E(kind=0))
    order("deviceRayCount lies inside the tile", count=b, lens=E(kind=0))
    order("unknown lens kind", lens=E(kind=0, sx=nan))
    # what a scene can do
    s, m = cloud_scene(3100, lights=3073)
    tpt.set_scene(s, m)
    tpt.UpdateTest(0.0, 0, W, H, 0)
    assert len(tpt.GetSceneDesc()[3]) == 3073
    refused("3073 emissive spheres")
    order("a fisheye scale beyond 4", lens=F(sx=4.5))  # (the lens before the scene)
    tpt.set_kernel_variant(2, 1, 1)
    tpt.UpdateTest(0.0, 0, W, H, 0)
    order("too many emissive spheres for the LDS light table (3072 at most)")  # (the lights before the LDS fit)
    tpt.set_kernel_variant(0, 3, -1)
    s, m = cloud_scene(3000)
    tpt.set_scene(s, m)
    tpt.set_kernel_variant(2, 1, 1)  # flat, and staged in LDS whatever its size: 3000 x 68 B
    tpt.UpdateTest(0.0, 0, W, H, 0)
    refused("a scene whose LDS does not fit")
    tpt.set_kernel_variant(0, 3, -1)
    tpt.set_scene(None, None)
    tpt.UpdateTest(0.0, 0, W, H, 0)
    tpt.synchronize()
    assert so.hostemuLensLaunches() == 0, "a refused call reached the launcher"
    # accepted at the limits of what is refused: the counter right behind and right before the tile, the largest spans, the basis bounds
    s, m = tpt.GetSceneDesc()[:2]
    tpt.set_samples_per_pixel(2)
    buf = np.zeros((H * W + 2, 4), np.float32)
    for lens, cnt_at in ((make_lens(EQUIRECT, sx=TWO_PI, sy=PI), 16 * (W * H + 1)), (make_lens(FISHEYE, sx=4.0, sy=4.0, max_angle=PI), 8),
                         (edited(make_lens(ORTHO, forward=(0, 0, -1)), right=(1.004, 0, 0), up=(0.009, 1, 0)), 16 * (W * H + 1))):
        buf[:] = 0
        b = buf.ctypes.data
        assert raw(W, H, 0, 0, lens, b + 16, b + cnt_at) == 0, msg()
        tpt.synchronize()
        total, want = checker.render(s, m, lens, W, H, 2)
        assert buf[1:-1].tobytes() == want.tobytes() and int(buf.view(np.uint64).ravel()[cnt_at // 8]) == total
    assert so.hostemuLensLaunches() == 3
    print("accepted: at the limits")
    tpt.ShutdownTest()
    print("ok")
    sys.exit(0)

# ---------------------------------------------------------------- accepted draws against the checker
tpt.InitializeTest()
tpt.UpdateTest(0.0, 0, W, H, 0)
s, m = tpt.GetSceneDesc()[:2]
# the draw's colour plane (Context::dLensColour) grows between the draws of one sequence: 8 x 8, 24 x 16, 8 x 8 again with no wait in
# between.  The growth itself drains the context stream (under the lazy schedule nothing else runs the first draw before its plane
# goes), and every tile is the checker's.  In the forward fold, which has no bounce-stack spill: the plane is the only buffer that grows.
def stats():
    st = (C.c_longlong * 2)(); so.hostemu_stats(st); return st[0], st[1]
tpt.set_samples_per_pixel(2)
tpt.set_fold_mode(1)
lens = make_lens(FISHEYE, max_angle=PI)
tiles = [np.zeros((h, w, 4), np.float32) for w, h in ((8, 8), (24, 16), (8, 8))]
tpt.draw_device_lens(0, 8, 8, ptr(tiles[0]), to_api(lens))
ran, frees = stats()
tpt.draw_device_lens(1, 24, 16, ptr(tiles[1]), to_api(lens))
assert stats()[1] == frees + 1, "the colour plane did not grow"
assert stats()[0] > ran, "the growth did not drain the context stream"
tpt.draw_device_lens(2, 8, 8, ptr(tiles[2]), to_api(lens))
assert stats()[1] == frees + 1, "the plane was replaced again"
tpt.synchronize()
tpt.set_fold_mode(0)
for frame, tile in enumerate(tiles):
    assert tile.tobytes() == checker.render(s, m, lens, tile.shape[1], tile.shape[0], 2, frame, fold=1)[1].tobytes(), ("growth", frame)
print("accepted: the colour plane grows between draws")
n_draws = 0
for kind in sorted(KINDS):
    lens = make_lens(KINDS[kind])
    for w, h in ((24, 16), (37, 19)):
        for spp in (1, 3):
            tpt.set_samples_per_pixel(spp)
            tile = np.zeros((h + 2, w, 4), np.float32)  # a guard row below and above
            tile[0] = tile[-1] = np.nan
            tile[1:-1] = noise_tile(w, h)
            want = tile[1:-1].copy()
            cnt = np.array([5, 1000, 5], np.uint64)
            total = 0
            for frame in range(3):
                r0 = tpt.ray_counter_read()
                tpt.draw_device_lens(frame, w, h, ptr(tile) + 16 * w, to_api(lens), 2, ptr(cnt) + 8)
                tpt.synchronize()
                k, want = checker.render(s, m, lens, w, h, spp, frame, flags=2, backbuffer=want)
                total += k
                assert tile[1:-1].tobytes() == want.tobytes(), (kind, w, h, spp, frame)
                assert np.isnan(tile[0]).all() and np.isnan(tile[-1]).all(), "a guard row was written"
                assert cnt.tolist() == [5, 1000 + total, 5], (kind, w, h, spp, frame, cnt, total)
                assert tpt.ray_counter_read() == r0, "the context's ray counter moved"
                n_draws += 1
            assert (tile[1:-1, :, 3] == noise_tile(w, h)[..., 3]).all()
print("accepted: %d draws equal the checker" % n_draws)
tpt.set_samples_per_pixel(2)

# both folds, the simple HitSpheres, light sampling off, a grouped scene; without a counter; not progressive over garbage
lens = make_lens(FISHEYE, max_angle=PI)
for scene in ("default", "grouped"):
    if scene == "grouped":
        import lens_lib
        gs, gm = lens_lib.grouped_scene()
        tpt.set_scene(gs, gm)
    tpt.UpdateTest(0.0, 0, W, H, 0)
    assert (tpt.scene_info()["groups"] > 0) == (scene == "grouped")
    s, m = tpt.GetSceneDesc()[:2]
    for fold in (0, 1):
        tpt.set_fold_mode(fold)
        for hs in (0, 1):
            tpt.set_kernel_variant(hs, 3, -1)
            for ls in (True, False):
                tpt.set_config(light_sampling=ls)
                tile = np.full((19, 37, 4), 1e30, np.float32)
                tpt.draw_device_lens(5, 37, 19, ptr(tile), to_api(lens), 0, None)
                tpt.synchronize()
                _, want = checker.render(s, m, lens, 37, 19, 2, 5, fold=fold, light_sampling=ls, backbuffer=np.full((19, 37, 4), 1e30, np.float32))
                assert tile.tobytes() == want.tobytes(), (scene, fold, hs, ls)
    tpt.set_fold_mode(0); tpt.set_kernel_variant(0, 3, -1); tpt.set_config()
tpt.set_scene(None, None)
tpt.UpdateTest(0.0, 0, W, H, 0)
print("accepted: folds, variants, scenes")

# the seed mode plays no part, and two draws back to back share the buffers in order
s, m = tpt.GetSceneDesc()[:2]
tpt.set_seed_mode(0)
a, b = np.zeros((16, 24, 4), np.float32), np.zeros((19, 37, 4), np.float32)
la, lb = make_lens(EQUIRECT), make_lens(ORTHO)
tpt.draw_device_lens(1, 24, 16, ptr(a), to_api(la))
tpt.draw_device_lens(1, 37, 19, ptr(b), to_api(lb))
tpt.synchronize()
tpt.set_seed_mode(1)
assert a.tobytes() == checker.render(s, m, la, 24, 16, 2, 1)[1].tobytes() and b.tobytes() == checker.render(s, m, lb, 37, 19, 2, 1)[1].tobytes()
print("accepted: row-serial context, back to back")
tpt.ShutdownTest()
print("ok")
'''


# (the script's order cases: the message each is held to, and how many of them)
ORDER = {"tptDrawDeviceLens: screenWidth and screenHeight must lie in 1..8192": 1, "tptDrawDeviceLens: frameCount must not be negative": 1,
         "tptDrawDeviceLens: flags must be 0 or TPT_FLAG_PROGRESSIVE": 1, "tptDrawDeviceLens: deviceTile is required": 1,
         "tptDrawDeviceLens: deviceRayCount lies inside the tile": 1, "tptDrawDeviceLens: unknown lens kind": 1,
         "tptDrawDeviceLens: a fisheye scale beyond 4": 1,
         "tptDrawDeviceLens: too many emissive spheres for the LDS light table (3072 at most)": 1}
ORDER_CASES = sum(ORDER.values())


def run_script(mode, policy, cus=None):
    from test_host_logic import build
    path = build("libtpt_hostemu_lens.so", [os.path.join(ROOT, "tests", "hostemu_lens.cpp")])
    env = dict(os.environ, TPT_LIB=path, HOSTEMU_POLICY=policy)
    env.pop("TPT_LIB_DIR", None)
    if cus:
        env["HOSTEMU_CUS"] = str(cus)
    p = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, mode], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.rstrip().endswith("ok"), out[-4000:]
    return out


def test_refusals_through_the_host_runtime():
    out = run_script("refusals", "lazy")
    assert out.count("refused:") == 1 + 1 + 1 + 6 + 2 + 4 + 1 + 4 + 30 + 2 + ORDER_CASES, out
    assert "accepted: at the limits" in out
    assert out.count("order:") == ORDER_CASES, out
    messages = refusal_messages(out)
    for message, cases in ORDER.items():  # (an order case is a refused case too, and is held to its message by the script)
        messages[message] -= cases
    assert messages == {
        "tpt: not initialised (call tptInitialize / InitializeTest first)": 1,
        "tptDrawDeviceLens: call tptUpdate first": 1,
        "tptDrawDeviceLens: args is required": 1,
        "tptDrawDeviceLens: screenWidth and screenHeight must lie in 1..8192": 6,
        "tptDrawDeviceLens: frameCount must not be negative": 2,
        "tptDrawDeviceLens: flags must be 0 or TPT_FLAG_PROGRESSIVE": 4,
        "tptDrawDeviceLens: deviceTile is required": 1,
        "tptDrawDeviceLens: deviceRayCount lies inside the tile": 4,
        "tptDrawDeviceLens: unknown lens kind": 3,
        "tptDrawDeviceLens: a non-finite lens field": 9,
        "tptDrawDeviceLens: a basis vector is not of unit length (its squared length must lie in 0.99..1.01)": 3,
        "tptDrawDeviceLens: two basis vectors are not orthogonal (their dot product must lie in -0.01..0.01)": 3,
        "tptDrawDeviceLens: sx and sy must be positive": 3,
        "tptDrawDeviceLens: an equirectangular span beyond 2 pi x pi": 2,
        "tptDrawDeviceLens: a fisheye scale beyond 4": 2,
        "tptDrawDeviceLens: a fisheye maxAngle outside (0, pi]": 3,
        "tptDrawDeviceLens: maxAngle must be 0 for this lens kind": 2,
        "tptDrawDeviceLens: too many emissive spheres for the LDS light table (3072 at most)": 1,
        "tptDrawDeviceLens: scene too large for LDS staging; use tptSetKernelVariant(.., .., 0)": 1,
    }


def test_the_binding_and_the_library_agree_at_every_bound_of_the_basis_rules():
    """the Python binding states the basis rules a second time (api._check_lens): records a clear 1e-6 inside and outside each bound --
    the squared length of each vector at 0.99 and 1.01, each dot product at -0.01 and 0.01 -- get the same verdict from both, the
    library's with its message"""
    import lens_kinds_lib
    records = lens_kinds_lib.bound_records()
    out = run_script("bounds", "lazy")
    assert out.count("bound:") == len(records) == 24, out
    assert out.count(": accepted by both") == 12, out
    assert out.count(": refused by both -- tptDrawDeviceLens: " + lens_kinds_lib.UNIT_MESSAGE) == 6, out
    assert out.count(": refused by both -- tptDrawDeviceLens: " + lens_kinds_lib.ORTHOGONAL_MESSAGE) == 6, out
    for name, _, inside, _ in records:
        assert "bound: %s: %s" % (name, "accepted" if inside else "refused") in out, name


@pytest.mark.parametrize("cus", [2, 256])
def test_the_plan_on_both_sides_of_the_seam_and_at_the_largest_image(cus):
    """chunkSize, chunkShift, numChunks and the grid as the launcher gets them, where the resident workgroups are known exactly: a
    device of two CUs (the seam at 361 x 177) and one of 256 (the seam at 4089 x 2041, 8192 x 8 still in tiles)"""
    out = run_script("plans", "eager", cus)
    plans = [ln for ln in out.splitlines() if ln.startswith("plan:")]
    assert len(plans) == 4 and "chunks of 64 (shift 6)" in plans[0] and "chunks of 256 (shift 8)" in plans[1], plans
    assert plans[2].startswith("plan: 8192 x 8192: 67108864 items in 262144 chunks of 256 (shift 8), %d workgroups" % (cus * 16)), plans
    assert ("chunks of 256 (shift 8)" if cus == 2 else "chunks of 64 (shift 6)") in plans[3], plans


@pytest.mark.parametrize("policy", ["eager", "lazy"])
def test_accepted_draws_equal_the_checker(policy):
    out = run_script("accepted", policy)
    assert "accepted: 36 draws equal the checker" in out, out
    for line in ("the colour plane grows between draws", "folds, variants, scenes", "row-serial context, back to back"):
        assert "accepted: " + line in out, out


def test_a_build_without_the_launcher_refuses():
    """the host runtime with the emulated kernels alone: tptLaunchTraceLens is a weak symbol nobody defines"""
    script = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from toypathtracer_amd import api as tpt
lib = tpt.load_library()
from toypathtracer_amd.scenes import cloud_scene
tpt.InitializeTest()
tile = np.full((8, 16, 4), np.nan, np.float32)
a = tpt.DrawLensArgs(screenWidth=16, screenHeight=8, frameCount=0, flags=0, lens=tpt.lens_equirect(), deviceTile=tile.ctypes.data, deviceRayCount=None)
# the launcher is looked for last: a scene whose LDS does not fit is still refused as that
s, m = cloud_scene(3000)
tpt.set_scene(s, m)
tpt.set_kernel_variant(2, 1, 1)
tpt.UpdateTest(0.0, 0, 16, 8, 0)
assert lib.tptDrawDeviceLens(C.byref(a)) != 0
m = lib.tptGetLastError().decode()
assert m == "tptDrawDeviceLens: scene too large for LDS staging; use tptSetKernelVariant(.., .., 0)", m
tpt.set_kernel_variant(0, 3, -1)
tpt.set_scene(None, None)
tpt.UpdateTest(0.0, 0, 16, 8, 0)
assert lib.tptDrawDeviceLens(C.byref(a)) != 0
m = lib.tptGetLastError().decode()
assert "tptDrawDeviceLens" in m and "launcher" in m, m
assert m == "tptDrawDeviceLens: this build has no lens launcher", m
tpt.synchronize()
assert np.isnan(tile).all()
tpt.ShutdownTest()
print("ok")
'''
    run_refusals(script)
