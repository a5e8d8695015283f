"""Mixed dtypes are refused before any launch (tests/mixed_dtype_cases.py), on the wavefront emulator."""
import pytest

from tests import mixed_dtype_cases as cases


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


DEV = "cpu"


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_mixed_dtype_is_refused_before_any_library_call(case, monkeypatch):
    cases.refuses(DEV, *case, monkeypatch)


@pytest.mark.parametrize("entry", sorted(cases.ENTRIES))
def test_uniform_dtype_still_runs(entry):
    cases.same_dtype_still_runs(DEV, entry)
