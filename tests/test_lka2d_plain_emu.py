"""The plain 2-D LKA block without a GPU: the modules' state_dict keys against the name lists of tests/lka2d_plain_cases.py, strict loading, the refusals, and
— on the wavefront emulator, which compiles csrc/cl_dw2d.hip like every other kernel file — the operator-level shapes and the small block-level cases against the
same float64 oracle.  The emulator answers a buffer load beyond its descriptor in software; what the hardware answers, and the kernel names, are the GPU file's."""
import pytest
import torch

from tests import lka2d_plain_cases as cases

DEV = "cpu"


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


def _modules():
    from deformablelka_amd import decoder2d_lka as d
    from deformablelka_amd.LKA import LKA_Attention
    return {
        "LKA_Attention": (LKA_Attention(8), cases.ATTENTION_KEYS),
        "SpatialAttention": (d.SpatialAttention(8), cases.ATTENTION_KEYS),
        "LKABlock": (d.LKABlock(8), cases.BLOCK_KEYS),
        "MyDecoderLayer": (d.MyDecoderLayer((4, 4), [8, 8, 8, 8, 16], 1, "mix_skip"), cases.DECODER_KEYS),
        "MyDecoderLayer_last": (d.MyDecoderLayer((4, 4), [8, 8, 8, 8, 16], 1, "mix_skip", n_class=3, is_last=True), cases.DECODER_LAST_KEYS),
    }


@pytest.mark.parametrize("name", ["LKA_Attention", "SpatialAttention", "LKABlock", "MyDecoderLayer", "MyDecoderLayer_last"])
def test_state_dict_keys_and_strict_loading(name):
    m, keys = _modules()[name]
    assert list(m.state_dict()) == keys
    gen = torch.Generator().manual_seed(1)
    sd = {k: torch.randn(v.shape, generator=gen) for k, v in m.state_dict().items()}
    assert list(sd) == keys
    m.load_state_dict(sd, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_decoder_shapes_of_the_reference_constructors():
    m, _ = _modules()["MyDecoderLayer_last"]
    sd = m.state_dict()
    assert tuple(sd["concat_linear.weight"].shape) == (8, 32) and tuple(sd["last_layer.weight"].shape) == (3, 8, 1, 1)
    assert tuple(sd["layer_up.expand.weight"].shape) == (128, 8) and tuple(sd["layer_lka_1.mlp.fc1.weight"].shape) == (32, 8, 1, 1)
    m, _ = _modules()["MyDecoderLayer"]
    assert tuple(m.state_dict()["concat_linear.weight"].shape) == (8, 16) and m.last_layer is None


def test_decoder_module_aliases_are_the_lka_classes():
    from deformablelka_amd import decoder2d, decoder2d_lka as d
    from deformablelka_amd.LKA import LKA, LKA_Attention
    assert issubclass(d.AttentionModule, LKA) and issubclass(d.SpatialAttention, LKA_Attention)
    assert isinstance(d.SpatialAttention(8).spatial_gating_unit, d.AttentionModule) and d.SpatialAttention(8).d_model == 8
    assert d.Mlp is decoder2d.Mlp and d.DropPath is decoder2d.DropPath and d.PatchExpand is decoder2d.PatchExpand
    assert d.FinalPatchExpand_X4 is decoder2d.FinalPatchExpand_X4


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_mixed_dtypes_are_refused_before_any_library_call(monkeypatch):
    from deformablelka_amd import _lib as L
    from deformablelka_amd.LKA import LKA_Attention
    from tests.mixed_dtype_cases import _NoLibraryCall
    monkeypatch.setattr(L, "get_lib", lambda: _NoLibraryCall())
    x = torch.randn(1, 32, 4, 4)
    m = LKA_Attention(32)
    m.spatial_gating_unit.conv0.weight.data = m.spatial_gating_unit.conv0.weight.data.double()   # one float64 parameter among float32 ones: the fused path
    with pytest.raises(RuntimeError, match="`conv0_w`"):
        m(x)
    with pytest.raises(RuntimeError, match="float32 parameters"):   # float64 activations next to float32 parameters
        LKA_Attention(32)(x.double())
    with pytest.raises(RuntimeError, match="float32 parameters"):   # bfloat16 parameters next to float32 activations
        LKA_Attention(32).bfloat16()(x)
    with pytest.raises(RuntimeError, match="float32 parameters"):   # a width outside the fused set takes bf16 activations only with bf16 parameters
        LKA_Attention(48)(torch.randn(1, 48, 4, 4).bfloat16())
    with pytest.raises(RuntimeError, match="`weight`"):
        cases.lka2d_plain.dwconv2d_forward_cl(x.permute(0, 2, 3, 1).contiguous(), torch.randn(32, 1, 5, 5).bfloat16(), None, 2, 1)
    with pytest.raises(RuntimeError, match="`grad_out`"):
        cases.lka2d_plain.dwconv2d_backward_cl(x.permute(0, 2, 3, 1).contiguous(), torch.randn(32, 1, 5, 5), x.permute(0, 2, 3, 1).bfloat16(), 2, 1)


def test_autocast_at_an_uncovered_width_stays_float32_on_the_per_op_path():
    from deformablelka_amd.LKA import LKA_Attention
    m = LKA_Attention(16)
    x = torch.randn(1, 16, 5, 6)
    assert not m.fused(x)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        y = m(x)
    assert y.dtype == torch.float32
    P = {k: v.detach().double() for k, v in m.state_dict().items()}
    cases.assert_matches("LKA_Attention C=16 under autocast", y.detach(), cases.attention_f64(x.double(), P), "f32", forward=True)


def test_unsupported_surfaces_as_the_usual_error():
    P = list(cases._attention_state(48, 0).values())
    with pytest.raises(RuntimeError, match=r"lka2d_plain_attention_forward: .*dlka status -8"):
        cases.lka2d_plain.attention_forward(torch.randn(1, 48, 4, 4), P)
    x = torch.randn(1, 4, 4, 32)
    with pytest.raises(RuntimeError, match=r"dlka status -8"):     # 3x3: not one of the two members
        cases.lka2d_plain.dwconv2d_forward_cl(x, torch.randn(32, 1, 3, 3), None, 1, 1)
    with pytest.raises(RuntimeError, match=r"dlka status -8"):     # 7x7 dilation 3 with the wrong padding
        cases.lka2d_plain.dwconv2d_forward_cl(x, torch.randn(32, 1, 7, 7), None, 3, 3)
    with pytest.raises(RuntimeError, match=r"dlka status -8"):     # C = 48
        cases.lka2d_plain.dwconv2d_forward_cl(torch.randn(1, 4, 4, 48), torch.randn(48, 1, 5, 5), None, 2, 1)


# ---- the kernels on the emulator ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.OP_CASES, ids=cases.case_id)
def test_depthwise_members_with_guard_bands(case):
    cases.single_op(DEV, *case)


@pytest.mark.parametrize("case", cases.BLOCK_CASES, ids=cases.case_id)
def test_block_vs_float64_oracle(case):
    shape, mode = case
    cases.compare_attention(shape, mode, cases.run_attention(DEV, shape, mode))


def test_block_is_bitwise_reproducible():
    shape, mode = cases.BLOCK_CASES[0]
    a, b = cases.run_attention(DEV, shape, mode), cases.run_attention(DEV, shape, mode)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_lkablock_vs_float64_restatement():
    cases.lkablock(DEV)
