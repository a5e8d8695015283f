"""``deformablelka_amd.ops`` exposes what it exposed as one file: the same public functions with the same signatures, the same constants with the
same values, and the underscore names other code reaches — against tests/golden/ops_surface.json, recorded from the commit before the split
(tests/golden/make_golden_ops_surface.py).  Neither the GPU nor the library is needed."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_golden_ops_surface", os.path.join(GOLDEN, "make_golden_ops_surface.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

with open(G.FIXTURE) as f:
    RECORDED = json.load(f)


@pytest.fixture(scope="module")
def ops():
    from deformablelka_amd import ops
    return ops


def test_the_record_is_not_empty():
    kinds = [d["kind"] for d in RECORDED["public"].values()]
    assert kinds.count("function") >= 90 and kinds.count("constant") >= 3 and len(RECORDED["private"]) >= 8


def test_public_names_are_exactly_the_recorded_ones(ops):
    assert sorted(G.public_surface(ops)) == sorted(RECORDED["public"])


@pytest.mark.parametrize("name", sorted(RECORDED["public"]))
def test_public_name_is_as_recorded(ops, name):
    assert G.describe(getattr(ops, name)) == RECORDED["public"][name]


@pytest.mark.parametrize("name", sorted(RECORDED["private"]))
def test_private_name_used_outside_is_as_recorded(ops, name):
    assert G.describe(getattr(ops, name)) == RECORDED["private"][name]


def test_launch_counters_are_plain_functions_under_their_own_names(ops):
    counters = [n for n in RECORDED["public"] if n.endswith("_launch_count")]
    assert len(counters) >= 8
    for n in counters:
        assert getattr(ops, n).__name__ == n
