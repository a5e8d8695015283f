"""-m gpu: the plain 2-D LKA block on the MI355X at the cases of tests/lka2d_plain_cases.py — the two depthwise members of csrc/cl_dw2d.hip with guard bands
(what the hardware range check answers is seen here, not on the emulator) and under the launch trace, LKA_Attention fused and per-op against the float64 oracle,
the path each width takes, bitwise reproducibility, LKABlock and MyDecoderLayer."""
import pytest
import torch

from tests import lka2d_plain_cases as cases
from tests import parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def hip_backend():
    from deformablelka_amd import _lib
    _lib._set_backend_for_tests(None)
    assert torch.cuda.is_available()
    _lib.get_lib()
    yield


# ---- operator level ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.OP_CASES, ids=cases.case_id)
def test_depthwise_members_with_guard_bands(case):
    cases.single_op(DEV, *case, trace=True)


# ---- block level ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.BLOCK_CASES, ids=cases.case_id)
def test_block_vs_float64_oracle(case):
    shape, mode = case
    cases.compare_attention(shape, mode, cases.run_attention(DEV, shape, mode))


@pytest.mark.parametrize("case", cases.BLOCK_CASES, ids=cases.case_id)
def test_path_each_width_takes(case):
    """Covered widths: the cl_dw2d kernels of the run's storage type, forward and data gradient and weight gradient of both members, in one fused call per
    direction — and no cl_ddw2d* kernel.  C = 48: the general kernels, none of cl_dw2d.hip."""
    shape, mode = case
    names = parity.kernels_launched(lambda: cases.run_attention(DEV, shape, mode))
    dw = sorted(n for n in names if n.startswith("cl_dw2d"))
    print(f"[{cases.case_id(case)}] launched: {', '.join(sorted(names))}")
    assert not any(n.startswith("cl_ddw2d") for n in names), sorted(names)
    if mode == "per_op":
        assert dw == [], dw
        return
    t = "bf16_t" if mode == "bf16" else "float"
    assert dw == sorted([f"cl_dw2d_kernel<{t}, 5, 1, 8>", f"cl_dw2d_kernel<{t}, 7, 3, 8>", f"cl_dw2d_wgrad_kernel<{t}, 5, 1, 8>",
                         f"cl_dw2d_wgrad_kernel<{t}, 7, 3, 8>"]), dw
    assert any(n.startswith("cl_wgrad_finalize") for n in names), sorted(names)   # the fold of the partial tiles


@pytest.mark.parametrize("case", cases.BLOCK_CASES[:3], ids=cases.case_id)
def test_fused_block_is_bitwise_reproducible(case):
    shape, mode = case
    a, b = cases.run_attention(DEV, shape, mode), cases.run_attention(DEV, shape, mode)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: {int((a[k] != b[k]).sum())} elements differ between two identical calls"


def test_lkablock_vs_float64_restatement():
    cases.lkablock(DEV)


@pytest.mark.parametrize("last", [False, True])
def test_decoder_layer_forward_backward(last):
    from deformablelka_amd.decoder2d_lka import MyDecoderLayer
    torch.manual_seed(0)
    h = w = 4
    m = MyDecoderLayer((h, w), [32, 32, 32, 32, 16], 1, "mix_skip", n_class=3, is_last=last).to(DEV)
    x1 = torch.randn(2, h * w, 16, device=DEV, requires_grad=True)
    x2 = torch.randn(2, h, w, 32, device=DEV, requires_grad=True)
    y = m(x1, x2)
    assert tuple(y.shape) == ((2, 3, 4 * h, 4 * w) if last else (2, 4 * h * w, 16))
    y.backward(torch.randn_like(y))
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(x1.grad).all()) and bool(torch.isfinite(x2.grad).all())
    for k, p in m.named_parameters():
        if k.startswith("layer_lka_2.") or k.startswith("concat_linear."):   # constructed, never run (MaxViT_LKA_Decoder.py:553-559)
            assert p.grad is None, k
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k


def test_decoder_layer_without_skip_leaves_the_lka_blocks_without_gradient():
    from deformablelka_amd.decoder2d_lka import MyDecoderLayer
    torch.manual_seed(0)
    m = MyDecoderLayer((4, 4), [32, 32, 32, 32, 32], 1, "mix_skip").to(DEV)
    x1 = torch.randn(2, 16, 32, device=DEV, requires_grad=True)
    y = m(x1)
    assert tuple(y.shape) == (2, 64, 16)
    y.backward(torch.randn_like(y))
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(x1.grad).all())
    for k, p in m.named_parameters():
        assert (p.grad is None) == (not k.startswith("layer_up.")), k
