"""The workgroup-tiled pointwise chain (cl_pointwise_chain_kernel) on the wavefront emulator: fused against DLKA_PW_UNFUSED=1 at small volumes.
One emulator thread (HIPEMU_THREADS=1) makes the whole block deterministic, so the comparison is torch.equal; with more threads the bounds of
check_lka3d_tokens_pointwise_pair apply.  Every backward launch carries riding zero fills (the block's atomics targets); (3, 3, 5) and (5, 3, 5) have row counts
that are not multiples of the 32-row tile."""
import os

import pytest
import torch

from tests import pw_chain


@pytest.fixture(scope="module", autouse=True)
def emu_backend(oracle):
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


CASES = [
    # C, B, dims
    (64, 1, (3, 3, 5)),     # 45 rows: a partial second row tile
    (64, 2, (4, 4, 4)),     # whole tiles
    (128, 1, (3, 3, 5)),
    (128, 2, (2, 4, 4)),
    (256, 1, (5, 3, 5)),    # 75 rows; two slices per wave
]


# (emulator time: C = 256 runs in fp32 here, and in both dtypes in tests/test_pw_chain_gpu.py)
@pytest.mark.parametrize("C,B,dims,dtype", [c + (dt,) for c in CASES for dt in (torch.float32, torch.bfloat16) if not (c[0] == 256 and dt == torch.bfloat16)])
def test_pw_chain_equals_two_launches_bitwise(C, B, dims, dtype, monkeypatch):
    monkeypatch.setenv("HIPEMU_THREADS", "1")
    pw_chain.check_chain("cpu", B, C, dims, dtype, bitwise=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C,B,dims", [(64, 2, (3, 3, 5)), (128, 1, (3, 3, 5))])
def test_pw_chain_equals_two_launches_threads(C, B, dims, dtype):
    pw_chain.check_chain("cpu", B, C, dims, dtype, bitwise=os.environ.get("HIPEMU_THREADS") == "1")
