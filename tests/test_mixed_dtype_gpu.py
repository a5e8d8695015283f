"""Mixed dtypes are refused before any launch (tests/mixed_dtype_cases.py), on the MI355X: the call raises and the library's launch trace stays empty."""
import pytest

from tests import mixed_dtype_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_mixed_dtype_is_refused_with_an_empty_launch_trace(case, monkeypatch):
    cases.refuses(DEV, *case, monkeypatch)


@pytest.mark.parametrize("entry", sorted(cases.ENTRIES))
def test_uniform_dtype_still_runs(entry):
    cases.same_dtype_still_runs(DEV, entry)
