"""The general NCDHW path on the MI355X against its record (tests/golden/planar_sequences.json): the size queries return the recorded numbers, and each
backward entry point launches the recorded kernels in the recorded order, template arguments included.  Cases: tests/planar_seq_cases.py."""
import pytest

from tests import planar_seq_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RECORDED = C.load_fixture()


@pytest.fixture(scope="module")
def sizes():
    from deformablelka_amd import _lib
    _lib._set_backend_for_tests(None)
    return C.sizes(_lib.get_lib())


@pytest.mark.parametrize("cid", sorted(RECORDED["sizes"]))
def test_size_query_returns_the_recorded_bytes(sizes, cid):
    assert sizes[cid] == RECORDED["sizes"][cid]


@pytest.mark.parametrize("cid", C.LAUNCH_IDS)
def test_backward_entry_launches_the_recorded_kernels_in_order(cid):
    got = C.launches(DEV, cid)
    print(f"[{cid}] {len(got)} launches: {got}")
    assert got == RECORDED["launches"][cid]
