"""tptDrawDeviceAov without a GPU: the declaration, the binding and the export of the entry point; the binding's argument checks; the
gfx950 code of the AOV kernels in the shipped library against their plain single-frame counterparts (tests/test_isa_contract.py); and
the refusals, driven through the host runtime compiled against tests/hostemu (a refused call returns before anything is enqueued, so no
kernel is emulated)."""
import re

import pytest

from isa_lib import code_object, count, exported_symbols, header_params, no_library, run_refusals  # noqa: F401  (code_object: a module fixture)
from kernel_manifest import AOV, QUEUE


def test_header_declares_the_entry_point():
    params = header_params("tptDrawDeviceAov")
    assert params == ["float time", "int frameCount", "int screenWidth", "int screenHeight", "float* deviceTile", "float* deviceAlbedo",
                      "float* deviceNormalDepth", "unsigned testFlags"], params


def test_binding_and_export():
    from toypathtracer_amd import api
    assert "tptDrawDeviceAov" in api.C_ABI_SYMBOLS
    assert callable(api.draw_device_aov)
    lib = api.load_library()
    assert hasattr(lib, "tptDrawDeviceAov")
    assert re.search(r"\bT tptDrawDeviceAov\b", exported_symbols(api.library_path()))


@pytest.mark.parametrize("args", [
    dict(w=0), dict(h=-3), dict(w=8.0), dict(h=True),
    dict(tile=0), dict(tile=None), dict(tile=1.5),
    dict(albedo=None, nd=None), dict(albedo=0, nd=0), dict(albedo="x"), dict(nd=-16), dict(nd=2.0),
], ids=lambda a: ",".join("%s=%r" % kv for kv in a.items()))
def test_binding_checks_arguments_before_the_library(monkeypatch, args):
    """every bad argument raises ValueError in Python: the library is never reached (load_library would fail the test)"""
    from toypathtracer_amd import api
    monkeypatch.setattr(api, "load_library", no_library)
    a = dict(w=16, h=8, tile=4096, albedo=8192, nd=16384)
    a.update(args)
    with pytest.raises(ValueError):
        api.draw_device_aov(0.0, 0, a["w"], a["h"], a["tile"], 2, albedo_ptr=a["albedo"], normal_depth_ptr=a["nd"])


@pytest.mark.parametrize("lds", [1, 0], ids=["lds-scene", "grouped"])
def test_aov_kernels_keep_the_queue_kernel_contract(code_object, lds):
    bodies, meta = code_object
    name, twin = AOV % lds, QUEUE % (lds, 0)
    assert name in meta and name in bodies, "the AOV kernel is missing from the shipped code object"
    body, m, t = bodies[name], meta[name], meta[twin]
    assert count(body, r"flat_") == 0, "a FLAT instruction: an LDS pointer lost its address space"
    assert m["agpr_count"] == 0
    assert m["max_flat_workgroup_size"] == 512 and m["wavefront_size"] == 64
    # the LDS it declares is its single-frame twin's (the sums live in global memory): two workgroups per CU as before
    assert m["group_segment_fixed_size"] == t["group_segment_fixed_size"]
    # the VGPR budget of the queue kernels: 120 beside the resolve kernel's waves, 128 for the grouped instantiation
    assert m["vgpr_count"] <= (120 if lds else 128), m
    # no scratch in the loop: what is parked in scratch are binary64 constants LLVM hoists to the entry (a store each there, a load each
    # in the class code), as in the grouped queue kernels (tests/test_isa_contract.py)
    assert m["vgpr_spill_count"] <= 6 and m["private_segment_fixed_size"] <= 28, m
    assert count(body, r"scratch_store") == count(body, r"scratch_load") <= 3
    # the sums: global loads and stores beyond the twin's (the twin's own global stores: the colour, the stack)
    assert count(body, r"global_store_dwordx4") > count(bodies[twin], r"global_store_dwordx4")
    # phase 1 on the matrix cores for the <= 64-sphere table, as in the twin
    assert count(body, r"v_mfma") == count(bodies[twin], r"v_mfma")


REFUSALS = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from toypathtracer_amd import api as tpt
lib = tpt.load_library()
tpt.InitializeTest()
w, h = 16, 8
tile = np.full((h, w, 4), 7.25, np.float32)
alb = np.full((h, w, 4), -3.5, np.float32)
nd = np.full((h, w, 4), 11.0, np.float32)
def refused(what, ww=w, hh=h, t=True, a=True, n=True):
    rc = lib.tptDrawDeviceAov(C.c_float(0.0), 0, ww, hh, tile.ctypes.data if t else None, alb.ctypes.data if a else None,
                              nd.ctypes.data if n else None, 2)
    msg = lib.tptGetLastError().decode()
    assert rc != 0 and "tptDrawDeviceAov" in msg, (what, rc, msg)
    print("refused:", what, "--", msg)
def reset():
    tpt.set_seed_mode(1); tpt.set_fold_mode(0); tpt.set_kernel_variant(0, 3, -1); tpt.set_row_shard(0, 1, 0); tpt.set_samples_per_pixel(4)
lib.tptDrawDeviceAov.argtypes = [C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint]
refused("before any tptUpdate")
tpt.UpdateTest(0.0, 0, w, h, 2)
refused("both planes NULL", a=False, n=False)
refused("tile NULL", t=False)
refused("tile NULL, one plane", t=False, a=False)
refused("no tptUpdate at this size", hh=h + 1)
tpt.UpdateTest(0.0, 0, 8200, 8, 2)
refused("wider than 8192", ww=8200, hh=8)
tpt.UpdateTest(0.0, 0, 8, 8193, 2)
refused("taller than 8192", ww=8, hh=8193)
tpt.UpdateTest(0.0, 0, w, h, 2)
tpt.set_seed_mode(0); refused("row-serial seeds"); reset()
tpt.set_fold_mode(1); refused("forward fold"); reset()
for hs, persist in ((0, 1), (0, 0), (1, 3), (2, 1)):
    tpt.set_kernel_variant(hs, persist, -1); refused("variant %d/%d" % (hs, persist))
reset()
tpt.set_samples_per_pixel(2048); refused("2048 spp"); reset()
tpt.set_row_shard(8, 2, 0); refused("row sharding"); reset()
tpt.comm_init_loopback(2, 8); refused("communicator"); tpt.comm_destroy(); reset()
mirror = np.zeros((h, w, 4), np.float32)
tpt.set_tile_mirror(mirror.ctypes.data); refused("tile mirror"); tpt.set_tile_mirror(None)
tpt.synchronize()
assert (tile == 7.25).all() and (alb == -3.5).all() and (nd == 11.0).all(), "a refused call wrote the tile or a plane"
tpt.ShutdownTest()
print("ok")
'''


def test_refusals_through_the_host_runtime(tmp_path):
    out = run_refusals(REFUSALS)
    assert out.count("refused:") == 17, out
