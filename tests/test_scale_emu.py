"""The backward shortcuts of the fp32 token path off unit scale, on the wavefront emulator (tests/scale_cases.py has the construction, the checks and the
bounds; tests/test_scale_gpu.py runs the shapes that reach every member of the half hand-over on the MI355X).  Tiny volumes here: the emulator runs the same
kernel sources lane by lane."""
import pytest

from tests import scale_cases as cases


@pytest.fixture(scope="module", autouse=True)
def emu_backend(oracle):
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


DEV = "cpu"


@pytest.mark.parametrize("k", cases.K_ALL)
def test_token_block_at_scale(k):
    """cl_deform_goff2_kernel -> cl_wgrad_samp_kernel with t at 2^k: (a) oracle protocol, (b) hand-over vs the gathering kernel, (c) against the k = 0 run."""
    cases.block(DEV, 1, 32, (3, 4, 5), k)


@pytest.mark.parametrize("k", (-24, 20))
def test_token_block_at_scale_16_row_writer(k):
    """The same through cl_deform_goff16_kernel (DLKA_GOFF16_MIN_ROWS=1)."""
    cases.block(DEV, 1, 32, (4, 4, 4), k, goff16=True)


@pytest.mark.parametrize("k", (-24, 20))
def test_token_block_at_scale_two_chunks(k):
    cases.handover(DEV, 1, 64, (2, 3, 4), k)


@pytest.mark.parametrize("k", (-20, 20))
def test_token_block_at_scale_bf16(k):
    """bf16 samples have fp32's exponent range: the bf16 path is scale-free as it stands."""
    cases.handover(DEV, 1, 32, (4, 4, 4), k, bf16=True)


@pytest.mark.parametrize("x_log2,go_log2", cases.SCALES_CL)
def test_deform3d_cl_at_scale(x_log2, go_log2):
    """Single-operator channels-last entry, forward and all four gradients against the oracle with x / grad_out at 2^(x_log2, go_log2): the fixed-point grad_input
    scale and the bf16 splits are scale-free (a small volume here; the window members run in the GPU file)."""
    cases.deform_cl(DEV, 32, (3, 4, 5), x_log2, go_log2)


def test_deform3d_cl_one_loud_row_per_brick():
    cases.deform_cl_loud_rows(DEV, 32, (4, 4, 8))
