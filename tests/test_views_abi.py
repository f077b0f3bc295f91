"""tptDrawDeviceViews without a GPU: the declaration, the binding and the export of the entry point; the gfx950 code of the views
kernels in the shipped library (the contract of the path-queue kernels, tests/test_isa_contract.py); and its refusals, driven through
the host runtime compiled against tests/hostemu (a refused call returns before anything is enqueued, so no kernel is emulated)."""
import re

import pytest

from isa_lib import code_object, count, exported_symbols, header_params, run_refusals  # noqa: F401  (code_object: a module fixture)
from kernel_manifest import VIEWS


def test_header_declares_the_entry_point():
    params = header_params("tptDrawDeviceViews")
    assert params == ["float time", "int frameCount", "int screenWidth", "int screenHeight", "int nViews", "const float* views",
                      "float* deviceTiles", "int64_t* deviceViewRays", "unsigned testFlags"], params


def test_binding_and_export():
    from toypathtracer_amd import api
    assert "tptDrawDeviceViews" in api.C_ABI_SYMBOLS
    assert callable(api.draw_device_views)
    lib = api.load_library()
    assert hasattr(lib, "tptDrawDeviceViews")
    assert re.search(r"\bT tptDrawDeviceViews\b", exported_symbols(api.library_path()))


def test_views_argument_shape_is_checked_before_the_library():
    from toypathtracer_amd import api
    with pytest.raises(ValueError):
        api.draw_device_views(0.0, 0, 8, 8, [[0.0] * 8], 0, 0)


@pytest.mark.parametrize("lds", [1, 0], ids=["lds-scene", "grouped"])
def test_views_kernels_keep_the_queue_kernel_contract(code_object, lds):
    bodies, meta = code_object
    name = VIEWS % lds
    assert name in meta and name in bodies, "the views kernel is missing from the shipped code object"
    body, m = bodies[name], meta[name]
    assert count(body, r"flat_") == 0, "a FLAT instruction: an LDS pointer lost its address space"
    assert count(body, r"ds_(read|load)") >= 30 and count(body, r"ds_(write|store)") >= 15
    assert m["agpr_count"] == 0
    assert m["vgpr_count"] <= 128, m
    assert m["max_flat_workgroup_size"] == 512 and m["wavefront_size"] == 64
    # phase 1 on the matrix cores for the <= 64-sphere table; none in the grouped-scene instantiation
    assert count(body, r"v_mfma_f32_32x32x16_f16") == (8 if lds else 0)
    assert count(body, r"v_mfma") == count(body, r"v_mfma_f32_32x32x16_f16")
    if lds:
        assert m["vgpr_count"] <= 120, m  # (as the single-view kernel: the resolve kernel's waves start beside it)


REFUSALS = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from toypathtracer_amd import api as tpt
lib = tpt.load_library()
tpt.InitializeTest()
w, h = 16, 8
tiles = np.full((2, h, w, 4), 7.25, np.float32)
rays = np.full(2, -5, np.int64)
views = np.array([[0, 2, 3, 0, 0, 0, 60, 0.02, 3], [3, 1.5, 2, 0, 0.5, 0, 45, 0.1, 3.5]], np.float32)
many = np.zeros((33, 9), np.float32)
five = np.repeat(views[:1], 5, axis=0)
def refused(what, ww=w, hh=h, n=2, v=views, t=True):
    rc = lib.tptDrawDeviceViews(0.0, 0, ww, hh, n, v.ctypes.data if v is not None else None, tiles.ctypes.data if t else None, rays.ctypes.data, 2)
    msg = lib.tptGetLastError().decode()
    assert rc != 0 and "tptDrawDeviceViews" in msg, (what, rc, msg)
    print("refused:", what, "--", msg)
def reset():
    tpt.set_seed_mode(1); tpt.set_fold_mode(0); tpt.set_kernel_variant(0, 3, -1); tpt.set_row_shard(0, 1, 0)
refused("before any tptUpdate")
tpt.UpdateTest(0.0, 0, w, h, 2)
refused("0 views", n=0)
refused("33 views", n=33, v=many)
refused("views NULL", v=None)
refused("tiles NULL", t=False)
refused("no tptUpdate at this size", hh=h + 1)
tpt.UpdateTest(0.0, 0, 8200, 8, 2)
refused("wider than 8192", ww=8200, hh=8)
tpt.UpdateTest(0.0, 0, 8192, 8192, 2)
refused("5 GiB of colour", ww=8192, hh=8192, n=5, v=five)
tpt.UpdateTest(0.0, 0, w, h, 2)
tpt.set_seed_mode(0); refused("row-serial seeds"); reset()
tpt.set_fold_mode(1); refused("forward fold"); reset()
for hs, persist in ((0, 1), (0, 0), (1, 3), (2, 1)):
    tpt.set_kernel_variant(hs, persist, -1); refused("variant %d/%d" % (hs, persist))
reset()
tpt.set_row_shard(8, 2, 0); refused("row sharding"); reset()
tpt.comm_init_loopback(2, 8); refused("communicator"); tpt.comm_destroy(); reset()
mirror = np.zeros((h, w, 4), np.float32)
tpt.set_tile_mirror(mirror.ctypes.data); refused("tile mirror"); tpt.set_tile_mirror(None)
tpt.synchronize()
assert (tiles == 7.25).all() and list(rays) == [-5, -5], "a refused call wrote a tile or a ray count"
tpt.ShutdownTest()
print("ok")
'''


def test_refusals_through_the_host_runtime(tmp_path):
    out = run_refusals(REFUSALS)
    assert out.count("refused:") == 17, out
