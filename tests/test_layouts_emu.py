"""The composite blocks' `saved` / `workspace` layouts on the CPU (host build of the library, tests/emu).

1. Every buffer-size and buffer-offset export reproduces tests/golden/block_layouts.json exactly (recorded by tests/golden/make_golden_layouts.py): each
   query is derived from the layout function that carves the buffer, and the table pins what those derivations must give.
2. Each block runs forward and backward in buffers of exactly the queried size with guard bytes on both sides: no kernel writes outside them, and `saved`,
   which is sized without slack, is refused (DLKA_ERR_WORKSPACE, nothing written) when it is one byte short."""
import importlib.util
import json
import os

import pytest
import torch

GUARD = 4096
PATTERN = 0xA5
ERR_WORKSPACE = "(dlka status -7)"


@pytest.fixture(scope="module", autouse=True)
def emu_backend(oracle):
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


def test_every_size_and_offset_query_reproduces_the_recorded_table():
    from deformablelka_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_golden_layouts", os.path.join(here, "golden", "make_golden_layouts.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(gen.OUT) as f:
        want = json.load(f)
    assert want["grid"] == gen.GRID, "the table was recorded over another grid: regenerate it on the commit whose layouts it is to pin"
    got = gen.collect(_lib.get_lib())
    assert sorted(got) == sorted(want["values"])
    for name, recorded in want["values"].items():
        assert len(recorded) == sum(len(vals) for _, vals in got[name]), name
        at = 0
        for args, vals in got[name]:
            assert vals == recorded[at:at + len(vals)], f"{name}{args}: recorded {recorded[at:at + len(vals)]}, now {vals}"
            at += len(vals)


class GuardedScratch:
    """tests/test_ws_canary_gpu.py's allocator on CPU tensors: every buffer the host side hands the C-ABI sits between two guard areas."""

    def __init__(self):
        self.live = []

    def __call__(self, nbytes, like):
        n = max(int(nbytes), 1)
        buf = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.uint8)
        self.live.append((buf, n))
        return buf[GUARD:GUARD + n]

    def verify(self, what):
        for buf, n in self.live:
            bad_h, bad_t = int((buf[:GUARD] != PATTERN).sum()), int((buf[GUARD + n:] != PATTERN).sum())
            assert bad_h == 0 and bad_t == 0, f"{what}: {bad_h} bytes in front of / {bad_t} bytes behind a {n}-byte buffer were overwritten"
        k = len(self.live)
        self.live.clear()
        return k


@pytest.fixture()
def guarded(monkeypatch):
    from deformablelka_amd import _lib
    g = GuardedScratch()
    monkeypatch.setattr(_lib, "scratch", g)
    return g


class ShortSaved:
    """The library with every saved-size query one byte short: the forward wrappers in ops.py then allocate and pass `saved_bytes - 1`."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if "saved_bytes" in name:
            return lambda *a: fn(*a) - 1
        return fn


def refused(guarded, monkeypatch, what, forward, backward_with, saved_bytes):
    """forward() with `saved` one byte short, then backward_with(a `saved` one byte short): both DLKA_ERR_WORKSPACE, guards intact."""
    from deformablelka_amd import _lib
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "_lib", ShortSaved(_lib.get_lib()))
        with pytest.raises(RuntimeError) as e:
            forward()
    assert ERR_WORKSPACE in str(e.value), e.value
    with pytest.raises(RuntimeError) as e:
        backward_with(guarded(saved_bytes - 1, None))
    assert ERR_WORKSPACE in str(e.value), e.value
    assert guarded.verify(what + ", saved one byte short") >= 4


def token_block(C, dims, dtype, seed=0):
    import deformablelka_amd as dk
    from oracle import blocks
    torch.manual_seed(seed)
    H, W, D = dims
    m = dk.LKA_Attention3d_deform(C)
    blocks.randomize_offsets_(m, std=0.3)
    x = torch.randn(1, H * W * D, C).to(dtype)
    gy = torch.randn(1, H * W * D, C).to(dtype)
    return m, [p.detach() for p in m.block_params()], x, gy


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,dims", [(32, (3, 4, 5)), (256, (2, 2, 2))])
def test_token_block_in_buffers_of_exactly_the_queried_size(guarded, monkeypatch, C, dims, dtype):
    from deformablelka_amd import ops
    m, params, x, gy = token_block(C, dims, dtype)
    what = f"tokens C={C} {dims} {dtype}"
    y, saved = ops.lka3d_attention_tokens_forward(x, params, dims, m.variant)
    gx, grads = ops.lka3d_attention_tokens_backward(x, params, gy, saved, dims, m.variant)
    assert guarded.verify(what) == 3   # saved, forward workspace, backward workspace
    for t in [y, gx, *grads]:
        assert bool(torch.isfinite(t.float()).all())
    refused(guarded, monkeypatch, what, lambda: ops.lka3d_attention_tokens_forward(x, params, dims, m.variant),
            lambda short: ops.lka3d_attention_tokens_backward(x, params, gy, short, dims, m.variant), saved.numel())


def test_token_block_phased_backward_equals_the_one_call_pass_bit_for_bit(guarded, monkeypatch):
    """Phase 1, phase 2 with a block-private partials buffer and the fold, against the one-call pass: the same kernels on the same operands, so every gradient
    is equal bit for bit.  The emulator runs workgroups on one worker thread here (HIPEMU_THREADS, read per launch): the depthwise weight gradients add into
    their staging rows with fp32 atomics, and with several workers two runs of the SAME call already differ in the last bit (1e-9 .. 6e-8 on conv0 / conv_spatial)."""
    from deformablelka_amd import ops
    monkeypatch.setenv("HIPEMU_THREADS", "1")
    dims = (3, 4, 5)
    m, params, x, gy = token_block(32, dims, torch.float32)
    y, saved = ops.lka3d_attention_tokens_forward(x, params, dims, m.variant)
    gx0, g0 = ops.lka3d_attention_tokens_backward(x, params, gy, saved, dims, m.variant)
    gx1, g1, keep = ops.lka3d_attention_tokens_backward(x, params, gy, saved, dims, m.variant, side_stream="inline")   # phase 1, phase 2, the fold
    assert guarded.verify("tokens, phased backward") == 5   # saved, three workspaces, the partials buffer
    for k, (a, b) in enumerate(zip([gx0, *g0], [gx1, *g1])):
        assert torch.equal(a, b), (k, float((a - b).abs().max()))


def test_wrapper_block_in_buffers_of_exactly_the_queried_size(guarded, monkeypatch):
    import deformablelka_amd as dk
    from deformablelka_amd import ops
    from oracle import blocks
    torch.manual_seed(0)
    B, C, dims = 1, 32, (3, 4, 5)
    H, W, D = dims
    m = dk.TransformerBlock_3D_single_deform_LKA(H * W * D, C, C, 4, dropout_rate=0.1, pos_embed=True).train()
    blocks.randomize_offsets_(m, std=0.3)
    x, gy = torch.randn(B, H * W * D, C), torch.randn(B, H * W * D, C)
    tparams = [None if p is None else p.detach() for p in m.wrapper_params()]
    lparams = [p.detach() for p in m.epa_block.block_params()]
    stats, mask = torch.empty(6 * C), torch.ones(B, C)

    def forward():
        return ops.tblock3d_forward(x, False, tparams, lparams, mask, True, stats, dims)

    def backward(saved, **kw):
        return ops.tblock3d_backward(tparams, lparams, mask, True, stats, gy, saved, dims, **kw)

    y, saved = forward()
    whole = backward(saved)                         # phase 0
    split = backward(saved, side_stream="inline")   # phases 1 + 2
    assert guarded.verify("tblock") == 4
    for r in (whole, split):
        for t in [r[0], *[t for t in r[1] if t is not None], *r[2]]:
            assert bool(torch.isfinite(t).all())
    refused(guarded, monkeypatch, "tblock", forward, backward, saved.numel())


def test_lka2d_block_in_buffers_of_exactly_the_queried_size(guarded, monkeypatch):
    import deformablelka_amd as dk
    from deformablelka_amd import ops
    from oracle import blocks
    torch.manual_seed(0)
    m = dk.deformable_LKA_Attention(32)
    blocks.randomize_offsets_(m, std=0.05)
    params = [p.detach() for p in m.block_params()]
    x, gy = torch.randn(1, 32, 5, 6), torch.randn(1, 32, 5, 6)
    y, saved = ops.lka2d_attention_forward(x, params)
    gx, grads = ops.lka2d_attention_backward(x, params, gy, saved)
    assert guarded.verify("lka2d") == 3
    for t in [y, gx, *grads]:
        assert bool(torch.isfinite(t).all())
    refused(guarded, monkeypatch, "lka2d", lambda: ops.lka2d_attention_forward(x, params), lambda short: ops.lka2d_attention_backward(x, params, gy, short),
            saved.numel())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lka2d_plain_block_in_buffers_of_exactly_the_queried_size(guarded, monkeypatch, dtype):
    from deformablelka_amd.ops import lka2d_plain
    from tests.lka2d_plain_cases import _attention_state
    gen = torch.Generator().manual_seed(0)
    params = list(_attention_state(32, 0).values())
    x, gy = (torch.randn(1, 32, 7, 6, generator=gen).to(dtype) for _ in range(2))
    what = f"lka2d_plain {dtype}"
    y, saved = lka2d_plain.attention_forward(x, params)
    gx, grads = lka2d_plain.attention_backward(x, params, gy, saved)
    assert guarded.verify(what) == 3
    for t in [y, gx, *grads]:
        assert bool(torch.isfinite(t.float()).all())
    refused(guarded, monkeypatch, what, lambda: lka2d_plain.attention_forward(x, params),
            lambda short: lka2d_plain.attention_backward(x, params, gy, short), saved.numel())
