"""Three findings of the round-6 advisor file, CPU side: the cl_conv_kw predicate, the wrapper block's dropout multipliers at the ends of [0, 1],
and pickling a module after the weight-gradient overlap has registered an application.  tests/test_small_fixes_gpu.py has the GPU side."""
import io
import pickle

import pytest
import torch
import torch.nn.functional as F

import deformablelka_amd as dk
from deformablelka_amd import transformerblock as tb


@pytest.fixture(scope="module")
def emu_lib():
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield _lib.get_lib()
    _lib._set_backend_for_tests(None)


# ---- cl_conv_kw_applies -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [2, 3])
def test_conv_kw_refuses_the_aux_epilogue_with_planar_output(emu_lib, split):
    """C = 32 -> Cout = 81 (NP = 96), 27 taps, a volume: the kernel's planar store (OMODE 1) never adds `aux`, so epi = 3 must not select it; every neighbouring
    combination keeps its answer."""
    ap = emu_lib.dlka_conv_kw_applies
    assert ap(0, 1, split, 27, 3, 96, 0, 1) == 0      # planar output + aux epilogue
    assert ap(0, 1, split, 27, 0, 96, 0, 1) == 1      # planar output, no epilogue
    assert ap(0, 0, split, 27, 3, 96, 0, 1) == 1      # channels-last output + aux epilogue
    assert ap(0, 0, split, 27, 0, 96, 0, 1) == 1


# ---- _draw_drop_mask ------------------------------------------------------------------------------------------------------------------------------------------------
def drop_mask_matches_dropout3d(dev, p):
    B, C = 3, 32
    m = dk.TransformerBlock_3D_single_deform_LKA(8, C, C, 4, dropout_rate=0.1)
    m.conv8[0].p = p
    gen_state = (lambda: torch.cuda.get_rng_state(dev)) if dev != "cpu" else torch.get_rng_state
    seed = (lambda s: torch.cuda.manual_seed(s)) if dev != "cpu" else torch.manual_seed
    seed(7)
    before = gen_state()
    got = m._draw_drop_mask(B, C, torch.float32, torch.device(dev))
    after = gen_state()
    seed(7)
    want = F.dropout3d(torch.ones(B, C, 1, 1, 1, device=dev), p, True).view(B, C)
    after_ref = gen_state()
    assert got.shape == (B, C) and torch.isfinite(got).all()
    assert torch.equal(got, want), (p, got, want)
    assert torch.equal(after, after_ref), "generator consumption differs from F.dropout3d's"
    if p >= 1:
        assert torch.equal(got, torch.zeros_like(got)) and torch.equal(before, after)
    if p == 0:
        assert torch.equal(got, torch.ones_like(got)) and torch.equal(before, after)


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 1.0])
def test_drop_mask_equals_dropout3d_multipliers(p):
    drop_mask_matches_dropout3d("cpu", p)


# ---- pickling ---------------------------------------------------------------------------------------------------------------------------------------------------------
class _Ctx:
    pass


@pytest.mark.parametrize("make", [lambda: dk.LKA_Attention3d_deform(32), lambda: dk.TransformerBlock_3D_single_deform_LKA(8, 32, 32, 4)], ids=["lka", "wrapper"])
def test_module_pickles_after_an_application_was_registered(make):
    """What the side-stream schedule does in every training forward (transformerblock._note_application) leaves nothing unpicklable on the module."""
    m = make()
    ctx1, ctx2 = _Ctx(), _Ctx()
    tb._note_application(m, ctx1)
    tb._note_application(m, ctx2)
    assert ctx1.wgrad_shared[0] and ctx2.wgrad_shared[0]      # the registry still does its job: two live applications are marked shared
    m2 = pickle.loads(pickle.dumps(m))
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    m3 = torch.load(buf, weights_only=False)
    for other in (m2, m3):
        sd, so = m.state_dict(), other.state_dict()
        assert sd.keys() == so.keys() and all(torch.equal(sd[k], so[k]) for k in sd)
    ctx3 = _Ctx()
    tb._note_application(m2, ctx3)
    assert not ctx3.wgrad_shared[0]                               # the copy starts with no live application
