"""GPU side of tests/test_small_fixes.py: the dropout multipliers from the device generator, the wrapper block's forward at p = 1, and pickling a model after a
training step with the weight-gradient overlap on."""
import io
import pickle

import pytest
import torch

import deformablelka_amd as dk
from tests.test_small_fixes import drop_mask_matches_dropout3d

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 1.0])
def test_drop_mask_equals_dropout3d_multipliers(p):
    drop_mask_matches_dropout3d(DEV, p)


def _wrapper(C=32, dims=(4, 4, 4)):
    from oracle import blocks
    torch.manual_seed(0)
    H, W, D = dims
    m = dk.TransformerBlock_3D_single_deform_LKA(H * W * D, C, C, 4, dropout_rate=0.1, pos_embed=True)
    blocks.randomize_offsets_(m, std=0.3)
    return m.to(DEV).train(), torch.randn(2, C, H, W, D, device=DEV)


def test_wrapper_block_forward_is_finite_with_everything_dropped():
    m, x = _wrapper()
    m.conv8[0].p = 1.0
    y = m(x)
    assert torch.isfinite(y).all()


def test_model_pickles_after_a_training_step_with_wgrad_overlap():
    m, x = _wrapper()
    m.wgrad_overlap = True
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)

    def step(model, optimizer):
        optimizer.zero_grad(set_to_none=True)
        model(x).square().mean().backward()
        torch.cuda.synchronize()
        optimizer.step()

    step(m, opt)
    blob = pickle.dumps(m)
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    for m2 in (pickle.loads(blob), torch.load(buf, weights_only=False)):
        sd, so = m.state_dict(), m2.state_dict()
        assert sd.keys() == so.keys() and all(torch.equal(sd[k], so[k]) for k in sd)
        assert m2.wgrad_overlap
        step(m2, torch.optim.SGD(m2.parameters(), lr=1e-3))
        assert all(torch.isfinite(p).all() for p in m2.parameters())
