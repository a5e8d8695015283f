"""The block stack on the MI355X against its record (tests/golden/stack_sequences.json): in every configuration a small DLKABlockStack launches the
recorded kernels in the recorded order, template arguments included, over the pass that records the finalize plan and the two sealed passes behind it.
The lists hold the side stream's launches too, in host issue order, but not the stream of a launch: see tests/stack_seq_cases.py for what holds that."""
import pytest

from tests import stack_seq_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RECORDED = C.load_fixture()


def test_the_record_names_the_same_cases():
    assert sorted(RECORDED["launches"]) == sorted(C.CASE_IDS)
    assert all(sorted(p) == sorted(C.PASSES) and all(p.values()) for p in RECORDED["launches"].values())


@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_stack_launches_the_recorded_kernels_in_order(cid):
    from deformablelka_amd import _lib
    _lib._set_backend_for_tests(None)
    got = C.sequences(DEV, cid)
    for name in C.PASSES:
        print(f"[{cid}/{name}] {len(got[name])} launches: {got[name]}")
    assert got == RECORDED["launches"][cid]
