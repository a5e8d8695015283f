"""The UNETR++ efficient paired attention (csrc/cl_epa.hip; EPA and TransformerBlock of deformablelka_amd/transformerblock.py and acdc.py) on the
MI355X: the cases of tests/test_epa_emu.py (tests/epa_cases.py) with guard bands around every output and under the launch trace, the path each width
takes, bitwise reproducibility, and the assembled net.  Contract: forward 1e-4 absolute, gradients 1e-3 (the reference's own records and the float64
restatement tests/epa_ref.py)."""
import pytest
import torch

from tests import epa_cases as C
from tests import parity

pytestmark = pytest.mark.gpu
DEV = "cuda"

FORWARD_KERNELS = {"cl_epa_gram_kernel", "cl_epa_finish_kernel", "cl_epa_apply_kernel"}
BACKWARD_KERNELS = {"cl_epa_bwd_tokens_kernel", "cl_epa_bwd_finish_kernel", "cl_epa_bwd_apply_kernel"}


def _epa_kernels(names):
    return {n.split("<")[0] for n in names if n.startswith("cl_epa_")}


@pytest.mark.parametrize("tag", ["synapse_epa", "acdc_epa", "synapse_block", "acdc_block"])
def test_module_reproduces_the_reference(tag):
    C.check_module_against_reference(tag, DEV)


@pytest.mark.parametrize("case", C.OPERATOR_CASES, ids=C.case_id)
def test_operator_cases(case):
    names = parity.kernels_launched(lambda: C.check_operator(DEV, *case, guard=True))
    assert _epa_kernels(names) == FORWARD_KERNELS | BACKWARD_KERNELS, names


@pytest.mark.parametrize("case", [(8, 32, 120), (32, 64, 60), (64, 64, 600)], ids=C.case_id)
def test_operator_with_masks(case):
    C.check_operator(DEV, *case, guard=True, masks=True)


def test_zero_columns_take_the_clamp_path():
    C.check_operator(DEV, 8, 32, 120, guard=True, zero_cols=True)
    C.check_operator(DEV, 16, 64, 60, guard=True, zero_cols=True, masks=True)


def test_large_logits_need_the_max_subtraction():
    C.check_operator(DEV, 8, 32, 60, guard=True, scale=8.0, temp=30.0)


@pytest.mark.parametrize("case", [(8, 64, 600), (64, 64, 600)], ids=C.case_id)
def test_two_identical_calls_give_the_same_bits(case):
    args = C.make_operator(*case, masks=True)
    C.same_bits(C.run_operator(DEV, *args), C.run_operator(DEV, *args))


@pytest.mark.parametrize("tag", ["synapse_epa", "acdc_epa"])
def test_training_mode_with_injected_masks(tag):
    m = C.check_module_against_restatement(DEV, tag, train_masks=True)
    assert (m.E is m.F) == tag.startswith("synapse")


def test_covered_width_takes_the_fused_kernels_and_no_token_softmax():
    """A covered width launches the cl_epa_* kernels; nothing the module launches through torch on the way is a softmax (the N x P map is never a tensor)."""
    from torch.profiler import ProfilerActivity, profile
    m, rec = C.load_module("synapse_epa", DEV)
    x = rec["inputs"][0].to(DEV).requires_grad_(True)
    got = {}

    def run():
        with profile(activities=[ProfilerActivity.CPU]) as prof:
            y = m(x)
            y.backward(rec["grad_output"].to(DEV))
        got["ops"] = {e.key for e in prof.key_averages()}

    names = parity.kernels_launched(run)
    assert _epa_kernels(names) == FORWARD_KERNELS | BACKWARD_KERNELS, names
    assert not any("softmax" in k.lower() for k in got["ops"]), sorted(k for k in got["ops"] if "softmax" in k.lower())


def test_uncovered_width_runs_operator_by_operator():
    got = {}
    names = parity.kernels_launched(lambda: got.update(m=C.check_module_against_restatement(DEV, C=48, N=60, P=32)))
    assert not _epa_kernels(names), names
    assert not got["m"].fused(torch.zeros(2, 60, 48, device=DEV))


def test_bf16_autocast_runs_operator_by_operator():
    m, rec = C.load_module("synapse_epa", DEV)
    x = rec["inputs"][0].to(DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not m.fused(x)
        names = parity.kernels_launched(lambda: m(x))
    assert not _epa_kernels(names), names


def test_block_under_bf16_autocast_runs_operator_by_operator():
    """No input is refused: inside bf16 autocast the wrapper and its EPA compose torch operators, and none of the library's kernels run."""
    m, rec = C.load_module("acdc_block", DEV)
    x = rec["inputs"][0].to(DEV)
    got = {}
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not m.on_kernels(x)
        names = parity.kernels_launched(lambda: got.update(y=m(x)))
    assert not names, names
    parity.assert_close("acdc_block under bf16 autocast", got["y"].detach().float(), rec["output"], rtol=parity.BF16_RTOL)   # the project's bf16 contract


def test_unaligned_views_are_accepted():
    C.check_offset_views(DEV)


def test_net_with_the_epa_block_trains():
    C.check_net(DEV)
