"""What DESIGN.md says about the gfx950 code of the path-queue kernels, checked on the code object INSIDE the shipped library
(no GPU needed: the fat binary is unbundled and disassembled with the ROCm LLVM tools).  Each assertion is a property that cost
a profiling session to find when it was lost:

  * the LDS rings / pair lists / stack level 0 are DS operations -- a volatile access through a generic pointer compiles to a
    FLAT load, which reaches LDS through the vector-memory path (rounds 2-3: flat_load_ushort in the pop and push spins);
  * phase 1 of HitSpheres runs on the matrix cores (v_mfma_f32_32x32x16_f16), 8 of them for the <= 64-sphere table;
  * 120 VGPRs for the kernels that stage the scene in LDS: four waves per SIMD, i.e. two 8-wave workgroups per CU, and room left for
    the resolve kernel's waves; 128 for the grouped-scene instantiations (round 5: 32 -> 22 spilled registers, HBM traffic 11.3 x -> 5.9 x);
  * register spills stay where they were measured in round 5 (headline: 2 VGPRs, 12 B of scratch, 33 SGPRs spilled to lanes; grouped: 22 VGPRs, 92 B);
  * the hot path holds no IEEE division expansion beyond the cold fallbacks of the short forms (tpt_math.h).
"""
import pytest

import kernel_manifest
from isa_lib import HAVE_TOOLS, code_object, count  # noqa: F401  (code_object: a module fixture)
from kernel_manifest import QUEUE

pytestmark = pytest.mark.skipif(not HAVE_TOOLS, reason="ROCm LLVM tools not installed")


def test_every_kernel_of_the_library_is_there(code_object):
    """the inventory: the library ships exactly the kernels of tests/kernel_manifest.py, no more and no fewer"""
    bodies, meta = code_object
    names = set(meta)
    unexpected, missing = sorted(names - kernel_manifest.ALL), sorted(kernel_manifest.ALL - names)
    assert names == kernel_manifest.ALL, ("in the library but not in the manifest: %s\nin the manifest but not in the library: %s"
                                          % (unexpected or "none", missing or "none"))
    assert not any("Test" in k for k in names), "unit-test kernels belong to the hooks build only"
    assert set(bodies) >= names


def test_queue_kernels_keep_lds_traffic_on_ds_instructions(code_object):
    bodies, _ = code_object
    for lds in (0, 1):
        for batch in (0, 1):
            body = bodies[QUEUE % (lds, batch)]
            assert count(body, r"flat_") == 0, "a FLAT instruction in %s: an LDS pointer lost its address space" % (QUEUE % (lds, batch))
            assert count(body, r"ds_(read|load)") >= 30 and count(body, r"ds_(write|store)") >= 15
            assert count(body, r"buffer_(load|store|atomic)") == 0


def test_phase_one_runs_on_the_matrix_cores(code_object):
    bodies, _ = code_object
    for batch in (0, 1):
        # <= 64 spheres: two sphere tiles x two k steps x two ray tiles
        assert count(bodies[QUEUE % (1, batch)], r"v_mfma_f32_32x32x16_f16") == 8
        # grouped scenes: NO matrix-core instruction in the product's instantiation since round 6 (a wave that has executed the
        # matrix-core filter of the groups' bounds is not safe in a time-sliced process; the hooks build carries that path)
        assert count(bodies[QUEUE % (0, batch)], r"v_mfma") == 0
        assert count(bodies[QUEUE % (0, batch)], r"v_permlane32_swap") == 0
    for name, body in bodies.items():
        assert count(body, r"v_mfma") == count(body, r"v_mfma_f32_32x32x16_f16"), name


def test_register_budget_of_the_queue_kernels(code_object):
    bodies, meta = code_object
    for lds in (0, 1):
        for batch in (0, 1):
            m = meta[QUEUE % (lds, batch)]
            assert m["vgpr_count"] <= 128, "more than 128 VGPRs: three waves per SIMD, one workgroup per CU"
            assert m["agpr_count"] == 0
            assert m["max_flat_workgroup_size"] == 512 and m["wavefront_size"] == 64
    head = meta[QUEUE % (1, 0)]
    assert head["vgpr_count"] <= 120, head  # (the resolve kernel's waves start beside a machine full of these: DESIGN 3.4)
    assert head["vgpr_spill_count"] <= 2 and head["private_segment_fixed_size"] <= 12, head
    assert head["sgpr_spill_count"] <= 36, head  # round 5: 63 -> 33 (scalars made where they are used: uniformHere)
    assert meta[QUEUE % (1, 1)]["vgpr_count"] <= 120 and meta[QUEUE % (1, 1)]["vgpr_spill_count"] <= 2
    # the grouped-scene kernels hold the dealing state on top: 128 registers since round 5; since round 6 (no matrix-core
    # path in them) nothing is spilled inside the traversal -- what is left are two or three binary64 constants of pow5 / sin-cos that LLVM
    # hoists to the kernel's entry and parks in scratch (4-6 registers: a store each at the entry, a load each in the class code)
    for batch in (0, 1):
        m = meta[QUEUE % (0, batch)]
        assert m["vgpr_spill_count"] <= 6 and m["private_segment_fixed_size"] <= 28, m
        body = bodies[QUEUE % (0, batch)]
        assert count(body, r"scratch_") <= 6, count(body, r"scratch_")
        assert count(body, r"scratch_store") == count(body, r"scratch_load") <= 3  # (dwordx2 each: one per constant)


def test_big_spheres_of_a_grouped_scene_come_through_scalar_loads(code_object):
    """hitSpheresGroupedDeal reads {centre, r^2} and the index of every big sphere (ground, lights) wave-uniformly: as s_load_dwordx4 through
    the constant address space.  As vector loads with a wait behind each they were five serial L2 round trips per call (10.7 % of the wave
    time at configs[4], profiles/r06/r06_run22.log / r06_run24.log)."""
    bodies, _ = code_object
    for batch in (0, 1):
        assert count(bodies[QUEUE % (0, batch)], r"s_load_dwordx4") >= 6, count(bodies[QUEUE % (0, batch)], r"s_load_dwordx4")


def test_divisions_of_the_hot_path_are_the_short_forms(code_object):
    bodies, _ = code_object
    for lds in (0, 1):
        body = bodies[QUEUE % (lds, 0)]
        # what is left are the cold fallbacks: tdivSafeNum / tdivByPi / trsqrt2 out of their proven ranges, the dielectric's
        # and the camera's few general quotients (v_div_fixup closes one IEEE expansion each)
        assert count(body, r"v_div_fixup_f32") <= 10, count(body, r"v_div_fixup_f32")
        assert count(body, r"v_\w+_f64") <= 61  # sin / cos / pow5 in binary64 (glibc's algorithms), nothing else
