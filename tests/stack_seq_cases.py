"""Shared cases of tests/test_stack_seq_gpu.py and tests/golden/make_golden_stack_sequences.py: what "behaviour unchanged" means for the HOST code of the
block stack, deformablelka_amd/stack.py — the kernels a small `DLKABlockStack` launches, in the order the host issues them, template arguments included, over
its first three steps: the first records the finalize plan (per-block folds), the second and the third run it sealed.  The lists are RECORDED
(tests/golden/stack_sequences.json) from the commit before `backward()` was split into one method per schedule and the settled knobs were retired, and never
taken from the code under test.

The launch trace (include/dlka.h dlka_trace_*) records every launch on the stream it goes to, so the lists DO hold the side stream's launches (the weight
gradients and their folds), in host issue order; they do not say which stream a launch went to.  Stream placement and the event waits are held by the
numerical tests: test_stack_grouped_folds_on_the_side_stream_equal_the_single_launch, test_stack_prepare_then_backward_is_stream_safe and
tests/test_stack_fullsize_gpu.py."""
import contextlib
import json
import os

import torch

from deformablelka_amd.stack import DLKABlockStack
from tests.planar_seq_cases import kernel_sequence

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stack_sequences.json")
STAGES = ((32, (2, 3, 4), 2), (64, (2, 2, 2), 1))   # the sizes of the emulator's stack tests: three blocks, two widths
PASSES = ("recording", "sealed_1", "sealed_2")
ENV_KNOBS = ("DLKA_STACK_FINALIZE_GROUP", "DLKA_STACK_WGRAD_OVERLAP")

# id: (environment, constructor keywords, k of a backward pass in two slices backward(k, None); backward(0, k) — None: one call)
CASES = {
    "default": ({}, {}, None),
    "finalize_group_0": ({"DLKA_STACK_FINALIZE_GROUP": "0"}, {}, None),
    "finalize_group_2": ({"DLKA_STACK_FINALIZE_GROUP": "2"}, {}, None),
    "overlap_wgrad_false": ({}, {"overlap_wgrad": False}, None),
    "defer_finalize_false": ({}, {"defer_finalize": False}, None),
    "sliced_backward": ({}, {}, 2),
}
CASE_IDS = list(CASES)


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@contextlib.contextmanager
def _environ(env):
    old = {k: os.environ.pop(k, None) for k in ENV_KNOBS}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in ENV_KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def sequences(dev, cid):
    """{pass: kernel names in launch order} of three forward + backward steps of the small stack in configuration `cid`."""
    env, kw, k = CASES[cid]
    with _environ(env):
        st = DLKABlockStack(1, stages=STAGES, device=dev, seed=5, **kw)

        def step():
            st.forward()
            if k is None:
                st.backward()
            else:
                st.backward(k, None)
                st.backward(0, k)
            torch.cuda.synchronize()   # (the trace's stop waits for the last launch ISSUED; the side stream may still run)

        return {name: kernel_sequence(step) for name in PASSES}
