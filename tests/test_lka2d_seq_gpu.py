"""The two channels-last 2-D attention blocks on the MI355X against their record (tests/golden/lka2d_sequences.json): one forward and one backward call of
each launch the recorded kernels in the recorded order, template arguments included.  Cases: tests/lka2d_seq_cases.py."""
import json

import pytest

from tests import lka2d_seq_cases as C

pytestmark = pytest.mark.gpu

with open(C.FIXTURE) as f:
    RECORDED = json.load(f)["launches"]


@pytest.mark.parametrize("cid", C.IDS)
def test_block_call_launches_the_recorded_kernels_in_order(cid):
    """The ordered list over ALL streams: the trace takes a launch on one of the library's internal streams (the deformable backward forks onto them by
    default) at the point where the host issued it.  Which stream a launch went to is not in the trace; test_lka2d_backward_forks_equal_one_stream
    (tests/test_parity_gpu.py) holds the forked pass to the one-stream pass."""
    from deformablelka_amd import _lib
    _lib._set_backend_for_tests(None)
    got = C.launches("cuda:0", cid)
    print(f"[{cid}] {len(got)} launches: {got}")
    assert got == RECORDED[cid]
