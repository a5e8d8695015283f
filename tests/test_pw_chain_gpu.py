"""The workgroup-tiled pointwise chain (cl_pointwise_chain_kernel) on the MI355X at the three real stage shapes: fused against DLKA_PW_UNFUSED=1, with the
launch counters of a forward + backward (2 chain launches per block, the depthwise pair unchanged)."""
import pytest
import torch

from tests import pw_chain

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C,dims", [(64, (16, 16, 16)), (128, (8, 8, 8)), (256, (4, 4, 4))])
def test_pw_chain_equals_two_launches(C, dims, dtype, oracle):
    # not bitwise at block level: the backward pass of a block has fp32 atomics upstream of nothing the chain reads, but grad_input of the deformable conv
    # (and with it x.grad) collects its halo in arrival order; y and the saved f / g1 / m are compared bit for bit below
    pw_chain.check_chain("cuda:0", 2, C, dims, dtype, bitwise=False)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C,dims", [(64, (16, 16, 16)), (128, (8, 8, 8)), (256, (4, 4, 4))])
def test_pw_chain_forward_is_bit_identical(C, dims, dtype, oracle):
    pw_chain.check_chain("cuda:0", 2, C, dims, dtype, bitwise="forward")
