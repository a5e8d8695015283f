"""Multi-wave workgroups of the weight-gradient kernels (cl_wgrad.hip) on the MI355X: the cases of tests/test_wgrad_wg_emu.py (fewer row tiles than waves,
tile counts that are no multiple of the waves, rows across a batch boundary, the N16 variants and the padded kernel, pointwise K = 1 through the token block),
the C = 256 volume in both dtypes, each against the ATen / oracle reference at the contract's tolerances, under the default and under DLKA_WGRAD_WAVES=1."""
import pytest
import torch

from tests import wgrad_wg_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(oracle):
    assert torch.cuda.is_available(), "needs the MI355X"


def _id(c):
    return f"B{c[0]}-C{c[1]}-{'x'.join(map(str, c[2]))}"


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("case", cases.CONV_CASES + [cases.WIDE_CASE], ids=_id)
def test_dense_wgrad_vs_aten(case, mode):
    cases.dense(DEV, case, mode)


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("case", cases.CONV_CASES + [cases.WIDE_CASE], ids=_id)
def test_deform_wgrad_vs_oracle(case, mode):
    cases.deform(DEV, case, mode)


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", cases.TOKEN_CASES + [(2, 256, (4, 4, 4))], ids=_id)
def test_token_block_pointwise_and_finalize_table(case, bf16, mode):
    cases.tokens(DEV, case, mode, bf16=bf16)


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("case", [cases.CONV_CASES[0], cases.CONV_CASES[2], cases.CONV_CASES[7]], ids=_id)
def test_dense_wgrad_reproducible(case, mode):
    cases.dense_twice_equal(DEV, case, mode)
