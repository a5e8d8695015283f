"""The sliding-window tile kernels (csrc/cl_tiles.hip) called directly on the MI355X, at wave and class-bucket edges, against plain torch on the CPU
(tests/tiles_cases.py has the cases, the references and the bound): everything tests/test_tiles_emu.py runs, plus predict_3d_tiled through the HIP path."""
import pytest

from tests import tiles_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda"


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


# ---- 5. predict_3d_tiled through the HIP path ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirror_axes", cases.PREDICT_AXES, ids=lambda a: "axes" + "".join(map(str, a)))
@pytest.mark.parametrize("variant", cases.PREDICT_VARIANTS)
def test_predict_3d_tiled_with_a_batch_invariant_net(variant, mirror_axes):
    cases.predict_tiled(DEV, variant, mirror_axes)
