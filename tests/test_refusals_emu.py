"""The pipeline entry points refuse bad calls with the statuses recorded from the commit before their checks moved into csrc/cl_pipeline.h
(tests/golden/refusal_codes.json), on the wavefront emulator's host build of the same sources.  No call reaches a launch.  Cases:
tests/refusal_cases.py."""
import pytest

from tests import refusal_cases as C

RECORDED = C.load_fixture()
CASES = C.cases()


@pytest.fixture(scope="module")
def statuses():
    from deformablelka_amd import _lib
    from tests import emu
    lib = _lib.bind(emu.load())
    counters = [n for n in _lib.SIGNATURES if n.endswith("_launch_count")]
    before = {n: getattr(lib, n)() for n in counters}
    got = C.run(lib)
    assert {n: getattr(lib, n)() for n in counters} == before, "a refused call counted a launch"
    return got


def test_the_table_and_the_record_name_the_same_cases():
    assert sorted(RECORDED) == sorted(CASES)
    assert all(v != 0 for k, v in RECORDED.items() if k not in C.NO_WORK) and all(RECORDED[k] == 0 for k in C.NO_WORK)
    entries = {name for name, _ in CASES.values()}
    assert len(entries) >= 30 and all(sum(1 for n, _ in CASES.values() if n == e) >= 2 for e in entries)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_refusal_status_is_the_recorded_one(statuses, cid):
    assert statuses[cid] == RECORDED[cid]
