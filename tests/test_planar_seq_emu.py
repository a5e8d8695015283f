"""The size queries of the general NCDHW path return the recorded numbers (tests/golden/planar_sequences.json) on the wavefront emulator's host build of
the same sources.  Cases: tests/planar_seq_cases.py; the launch sequences need the GPU's launch trace (tests/test_planar_seq_gpu.py)."""
import pytest

from tests import planar_seq_cases as C

RECORDED = C.load_fixture()


@pytest.fixture(scope="module")
def sizes():
    from deformablelka_amd import _lib
    from tests import emu
    return C.sizes(_lib.bind(emu.load()))


def test_the_record_names_the_same_cases(sizes):
    assert sorted(RECORDED["sizes"]) == sorted(sizes) and sorted(RECORDED["launches"]) == sorted(C.LAUNCH_IDS)
    assert all(v > 0 for v in RECORDED["sizes"].values()) and all(RECORDED["launches"].values())


@pytest.mark.parametrize("cid", sorted(RECORDED["sizes"]))
def test_size_query_returns_the_recorded_bytes(sizes, cid):
    assert sizes[cid] == RECORDED["sizes"][cid]
