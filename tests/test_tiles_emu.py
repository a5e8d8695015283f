"""The sliding-window tile kernels (csrc/cl_tiles.hip) called directly on the wavefront emulator, at wave and class-bucket edges, against plain torch on the CPU
(tests/tiles_cases.py has the cases, the references and the bound).  tests/test_tiles_gpu.py runs the same checks on the MI355X, plus predict_3d_tiled through the
HIP path, which only a GPU tensor reaches."""
import pytest

from tests import tiles_cases as cases

DEV = "cpu"


@pytest.fixture(autouse=True)
def emu_backend():
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


# ---- 1. gather ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", cases.GATHER_CASES)
def test_gather_is_bitwise_flip_of_the_padded_slice(cid):
    cases.gather(DEV, cid)


# ---- 2. blend -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", cases.DTYPES)
@pytest.mark.parametrize("nonlin", cases.NONLIN)
@pytest.mark.parametrize("sid", cases.BLEND_MAIN)
def test_blend_against_the_float64_tile_loop(sid, nonlin, dtype):
    cases.blend(DEV, sid, nonlin, dtype)


@pytest.mark.parametrize("dtype", cases.DTYPES)
@pytest.mark.parametrize("nonlin", cases.NONLIN)
@pytest.mark.parametrize("sid", cases.BLEND_FURTHER)
def test_blend_offset_box_repeated_origin_and_full_table(sid, nonlin, dtype):
    cases.blend(DEV, sid, nonlin, dtype, variants=(("xyz", True),))


@pytest.mark.parametrize("sid", cases.BLEND_SWEEP)
def test_blend_at_the_upper_edge_of_each_class_bucket(sid):
    cases.blend(DEV, sid, "softmax", "fp32", variants=(("xyz", True),))


def test_blend_cases_have_uncovered_voxels_inside_the_box():
    cases.blend_box_has_uncovered_voxels()


# ---- 3. finalize ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", cases.FINALIZE_K)
@pytest.mark.parametrize("sid", cases.FINALIZE_SHAPES)
def test_finalize_is_bitwise_division_and_first_maximum_argmax(sid, K):
    cases.finalize(DEV, sid, K)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", cases.REFUSALS)
def test_refused_blend_leaves_score_and_weight_alone(which):
    cases.blend_refusal(DEV, which)


def test_each_successful_call_counts_one_launch():
    cases.launch_counts(DEV)
