"""Multi-wave workgroups of the weight-gradient kernels (cl_wgrad.hip) on the wavefront emulator: every case against the ATen / oracle reference at the
contract's tolerances (tests/parity.py), under the default and under DLKA_WGRAD_WAVES=1.  The emulator runs a workgroup's waves as fibers and aborts on a
barrier that not every live work-item reaches, so the cases with fewer row tiles than waves check that the waves without rows take part in the LDS sum.
The summation order differs between the two settings: they are compared with the reference, never with each other."""
import pytest

from tests import wgrad_wg_cases as cases


@pytest.fixture(scope="module", autouse=True)
def emu_backend(oracle):
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


def _id(c):
    return f"B{c[0]}-C{c[1]}-{'x'.join(map(str, c[2]))}"


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("case", cases.CONV_CASES + [cases.WIDE_CASE], ids=_id)
def test_dense_wgrad_vs_aten(case, mode):
    cases.dense("cpu", case, mode)


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("case", cases.CONV_CASES + [cases.WIDE_CASE], ids=_id)
def test_deform_wgrad_vs_oracle(case, mode):
    cases.deform("cpu", case, mode)


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", cases.TOKEN_CASES, ids=_id)
def test_token_block_pointwise_and_finalize_table(case, bf16, mode):
    cases.tokens("cpu", case, mode, bf16=bf16)


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("case", [cases.CONV_CASES[0], cases.CONV_CASES[2], cases.CONV_CASES[4]], ids=_id)
def test_dense_wgrad_reproducible(case, mode, monkeypatch):
    monkeypatch.setenv("HIPEMU_THREADS", "1")
    cases.dense_twice_equal("cpu", case, mode)


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
def test_partials_shrink_with_the_waves_per_workgroup(dtype):
    """No kernel runs.  dlka_lka3d_tokens_partials_bytes_v at the four headline stage shapes (B = 2): with four waves per workgroup in every family the
    partial tile sets are cdiv(row chunks, 4), so at stages 0 - 2 (11 or more row chunks per gradient; only the 2 (K + 1) C floats of depthwise staging
    do not shrink) the area is at most a third of the one-wave area; at stage 3 (4 and 2 row chunks) it is no larger.  A query under DLKA_WGRAD_WAVES=1
    returns the one-wave sizes."""
    from deformablelka_amd import _lib
    lib = _lib.get_lib()
    for s, (C, dims) in enumerate(cases.STAGES):
        new, old = cases.partials_bytes(lib, C, dims, "wg", dtype), cases.partials_bytes(lib, C, dims, "one_wave", dtype)
        print(f"stage {s}: partials {old} -> {new} bytes ({old / new:.2f} x)")
        assert 0 < new <= old
        if s < 3:
            assert 3 * new <= old, (s, new, old)
