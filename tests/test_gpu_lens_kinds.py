"""tptDrawDeviceLens on the GPU across bases, spans, origins, sizes, frames, sample counts and scenes (tests/lens_kinds_lib.py lists the
cases, tests/test_lens_kinds.py proves on the CPU that each is what its name says and has a finite reference): every case drawn with
tests/test_gpu_lens.py's `draw` -- guard rows of NaN around the tile, guard words around the counter -- and held against
LensChecker.render in the tile's bytes and the counter's gain.  There is no tolerance anywhere."""
import numpy as np
import pytest

import lens_kinds_lib as lib
from lens_lib import LensChecker
from test_gpu_lens import draw, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return LensChecker(tmp_path_factory.mktemp("lens_kinds_checker"))


def held(tpt, checker, c):
    s, m = lib.scene(c.scene)
    if c.scene != "default":
        tpt.set_scene(s, m)
    tpt.set_kernel_variant(0, 3, c.lds)
    tpt.set_fold_mode(c.fold)
    tpt.set_samples_per_pixel(c.spp)
    tpt.UpdateTest(0.0, 0, c.w, c.h, 0)
    want = lib.reference(checker, c)
    assert np.isfinite(want[1]).all(), c.name
    same(draw(tpt, c.lens, c.w, c.h, frame=c.frame, flags=c.flags, start=lib.start_tile(c)), want, c.name)
    return want


def names(section):
    return [c.name for c in lib.cases(section)]


def named(section, name):
    (c,) = [c for c in lib.cases(section) if c.name == name]
    return c


@pytest.mark.parametrize("name", names("bases"))
def test_bases_at_the_accepted_bounds(tpt_defaults, checker, name):
    held(tpt_defaults, checker, named("bases", name))


@pytest.mark.parametrize("name", names("spans"))
def test_spans_down_to_nothing_and_up_to_the_types_end(tpt_defaults, checker, name):
    held(tpt_defaults, checker, named("spans", name))


@pytest.mark.parametrize("name", names("origins"))
def test_origins_far_out_on_a_surface_and_at_a_centre(tpt_defaults, checker, name):
    c = named("origins", name)
    rays, _ = held(tpt_defaults, checker, c)
    if name in lib.ORIGIN_HITS:
        assert (rays > c.w * c.h * c.spp) == lib.ORIGIN_HITS[name]


@pytest.mark.parametrize("name", names("sizes"))
def test_the_longest_rows_and_columns(tpt_defaults, checker, name):
    held(tpt_defaults, checker, named("sizes", name))


def lens_resident(tpt):
    """the workgroups of a lens launch that are resident at once, which laneRefillChunks sizes the chunks by -> (resident, launch_info()).
    tptGetLaunchInfo reports the plan of the last FRAME (chooseKernel / sizeGrid), and tptDrawDeviceLens does not record its own there.
    What lies behind it does say it: the lens launch takes laneRefillOccupancy(ldsScene, lds) x the device's CUs, with ldsScene and lds
    from laneRefillLds -- and chooseKernel plans a frame that the lane-refill kernel traces (tptSetKernelVariant(0, 1, -1)) with the same
    two functions on the same scene, fold and HitSpheres variant.  So: one small frame on that kernel, and its plan."""
    import torch
    w, h = 64, 40
    tile = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    tpt.set_kernel_variant(0, 1, -1)
    tpt.UpdateTest(0.0, 0, w, h, 2)
    tpt.draw_device(0.0, 0, w, h, tile.data_ptr(), 2)
    tpt.synchronize()
    info = tpt.launch_info()
    tpt.set_kernel_variant(0, 3, -1)
    assert info["blocks_per_cu"] >= 1 and info["num_cus"] >= 1, info
    return info["num_cus"] * info["blocks_per_cu"], info


def test_both_sides_of_the_seam_between_tiles_and_chunks_of_256(tpt_defaults, checker):
    """the smallest image of 2 t x t tiles (no side a multiple of 8) that laneRefillChunks hands out in chunks of 256 pixels on THIS
    device, and the one before it, which still goes out as 8 x 8 tiles; 1 spp.  On a whole MI355X at 4 workgroups per CU: 2041 x 1017
    and 2025 x 1009.  (tests/test_lens_abi.py pins chunkSize, chunkShift, numChunks and the grid on both sides on the emulated device.)"""
    tpt = tpt_defaults
    resident, info = lens_resident(tpt)
    above, under = lib.seam_sizes(resident)
    print("resident workgroups %d (%r): %dx%d in chunks of 256, %dx%d in tiles" % ((resident, info) + above + under))
    assert lib.items_of(*above) // 256 >= 8 * resident > lib.items_of(*under) // 256  # laneRefillChunks' own test, either side
    for c in lib.seam_cases(resident):
        held(tpt, checker, c)


@pytest.mark.parametrize("name", names("frames"))
def test_large_and_wrapping_frame_numbers(tpt_defaults, checker, name):
    held(tpt_defaults, checker, named("frames", name))


@pytest.mark.parametrize("name", names("samples"))
def test_sample_counts_up_to_the_largest(tpt_defaults, checker, name):
    held(tpt_defaults, checker, named("samples", name))


@pytest.mark.parametrize("name", names("scenes"))
def test_shells_light_counts_and_folds(tpt_defaults, checker, name):
    tpt = tpt_defaults
    c = named("scenes", name)
    held(tpt, checker, c)
    assert (tpt.scene_info()["groups"] > 0) == (c.scene == "lights_grouped")
