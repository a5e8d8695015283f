"""The dense channels-last conv kernels (csrc/cl_igemm.hip, cl_conv_wave.hip, cl_conv_kw.hip) on the wavefront emulator at the shapes of tests/dense_conv_cases.py,
against F.conv3d in float64: the value checks, the fp32 equivalence of the three-term forward and the guard bands of groups K1 to K5, W and E.  Left to the GPU
file: the member names (the launch trace is GPU-only) and the two large-row groups — K6 / K7 (16 900 rows: several column tiles per workgroup) and I1 (16 512
rows: cl_igemm_kernel with three-term operands, the swizzled grid).  The emulator answers a buffer load beyond its descriptor in software and runs the
workgroups of a tap split one after the other; what the hardware answers, and atomics that really meet, are the GPU file's to see."""
import pytest

from tests import dense_conv_cases as cases
from tests import parity


@pytest.fixture(scope="module", autouse=True)
def emu_backend(oracle):
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    """DLKA_IGEMM_NT and DLKA_XCD_MIN unset; the library's cached switches follow the environment into the test and out of it."""
    monkeypatch.delenv("DLKA_IGEMM_NT", raising=False)
    monkeypatch.delenv("DLKA_XCD_MIN", raising=False)
    parity._refresh_switches()
    yield
    monkeypatch.undo()
    parity._refresh_switches()


DEV = "cpu"


@pytest.mark.parametrize("case", [c for c in cases.K_CASES if not c.gpu_only], ids=cases.case_id)
def test_wave_split_members_are_right_and_reproducible(case):
    cases.reproducible(DEV, case)


@pytest.mark.parametrize("case", cases.W_CASES, ids=cases.case_id)
def test_tap_split_members(case):
    cases.single_op(DEV, case)


@pytest.mark.parametrize("case,runs", cases.W5_CASES, ids=lambda v: cases.case_id(v) if isinstance(v, cases.Case) else "")
def test_forced_column_tiles(case, runs, monkeypatch):
    cases.forced_column_tiles(DEV, case, runs, monkeypatch)


@pytest.mark.parametrize("case", cases.E_CASES, ids=cases.case_id)
def test_pointwise_with_planar_output_on_the_exact_mfma(case):
    cases.exact_pointwise_planar(DEV, case)
