"""The planar plumbing kernels (csrc/planar_ops.hip), the modules over them and the stand-alone GELU on the MI355X, at ragged and edge shapes, against float64
torch on the CPU (tests/planar_cases.py has the cases, the references and the tolerances).  Everything tests/test_planar_emu.py runs, plus what it leaves out."""
import pytest

from tests import planar_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ---- 1. BatchNorm kernels -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("shape", cases.BN_SHAPES, ids=cases.shape_id)
def test_batchnorm_ragged_and_edge_shapes(shape, affine):
    cases.batchnorm(DEV, shape, affine)


# ---- 2. pivot robustness -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cases.PIVOT_KINDS)
@pytest.mark.parametrize("shape", cases.PIVOT_SHAPES, ids=cases.shape_id)
def test_batchnorm_with_an_atypical_first_voxel(shape, kind):
    cases.pivot(DEV, shape, kind)


# ---- 3. modules over these kernels ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum", [0.1, None])
def test_batchnorm3d_running_statistics_over_two_iterations(momentum):
    cases.batchnorm3d_module(DEV, momentum)


def test_instancenorm_at_the_grid_limit_of_65535_planes():
    cases.instancenorm_grid_limit(DEV)


def test_instancenorm_of_65536_planes_takes_the_stock_path():
    cases.instancenorm_past_grid_limit(DEV)


def test_batchnorm_entry_refuses_65536_planes_and_launches_nothing():
    cases.batchnorm_entry_past_grid_limit(DEV)


def test_one_value_per_channel_raises_as_the_stock_layers_do():
    cases.one_value_per_channel(DEV)


def test_groupnorm_planar_forward_on_odd_rows():
    cases.groupnorm_odd_row(DEV)


def test_batchnorm_entries_take_a_transposed_x_and_refuse_other_dtypes():
    cases.batchnorm_transposed_and_wrong_dtype(DEV)


# ---- 4. pointwise planar kernels -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout", cases.PW_PAIRS)
def test_pointwise_every_menu_entry(cin, cout):
    cases.pointwise(DEV, 2, cin, cout, cases.PW_SPATIAL)


@pytest.mark.parametrize("cin,cout", cases.PW_FORWARD_ONLY)
def test_pointwise_forward_only_widths(cin, cout):
    cases.pointwise_forward_only(DEV, cin, cout)


@pytest.mark.parametrize("n", cases.PW_TAILS)
def test_pointwise_mfma_tails(n):
    cases.pointwise(DEV, 2, 16, 14, (1, 1, n))


@pytest.mark.parametrize("B,pair,spatial,chunk", cases.PW_CHUNKS, ids=lambda v: cases.shape_id(v))
def test_pointwise_weight_gradient_chunk_choices(B, pair, spatial, chunk):
    cases.pointwise_chunk(DEV, B, pair, spatial, chunk)


@pytest.mark.parametrize("cin,cout", cases.PW_NCT4)
def test_pointwise_weight_gradient_of_33_to_64_input_channels(cin, cout):
    cases.pointwise_nct4(DEV, cin, cout)


def test_pointwise_weight_gradient_refuses_17_output_channels():
    cases.pointwise_wgrad_refuses_cout_17(DEV)


def test_pointwise_unaligned_plane_falls_back():
    cases.pointwise_unaligned_falls_back(DEV)


# ---- 5. GELU -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.GELU_SIZES)
def test_gelu_f32(n):
    cases.gelu_f32(DEV, n)


@pytest.mark.parametrize("n", cases.GELU_SIZES)
def test_gelu_bf16(n):
    cases.gelu_bf16(DEV, n)
