"""The UNETR++ efficient paired attention (csrc/cl_epa.hip; EPA and TransformerBlock of deformablelka_amd/transformerblock.py and acdc.py) on the
wavefront emulator: the reference's own output and gradients (tests/golden/reference_epa*.pt), the float64 restatement (tests/epa_ref.py) checked
against the same records and then used as the oracle for the operator cases of tests/epa_cases.py.  Contract: forward 1e-4 absolute, gradients 1e-3."""
import os
import subprocess
import sys

import pytest
import torch

from tests import epa_cases as C


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)


@pytest.mark.parametrize("tag", ["synapse_epa", "acdc_epa"])
def test_restatement_reproduces_the_reference(tag):
    C.check_restatement_against_reference(tag)


@pytest.mark.parametrize("tag", ["synapse_epa", "acdc_epa", "synapse_block", "acdc_block"])
def test_module_reproduces_the_reference(tag):
    C.check_module_against_reference(tag, "cpu")


@pytest.mark.parametrize("case", C.EMU_OPERATOR_CASES, ids=C.case_id)
def test_operator_cases(case):
    C.check_operator("cpu", *case)


@pytest.mark.parametrize("case", [(8, 32, 120), (32, 64, 60)], ids=C.case_id)
def test_operator_with_masks(case):
    C.check_operator("cpu", *case, masks=True)


def test_zero_columns_take_the_clamp_path():
    C.check_operator("cpu", 8, 32, 120, zero_cols=True)
    C.check_operator("cpu", 16, 64, 60, zero_cols=True, masks=True)


def test_large_logits_need_the_max_subtraction():
    C.check_operator("cpu", 8, 32, 60, scale=8.0, temp=30.0)


def test_two_identical_calls_give_the_same_bits(monkeypatch):
    monkeypatch.setenv("HIPEMU_THREADS", "1")
    args = C.make_operator(8, 64, 600, masks=True)
    C.same_bits(C.run_operator("cpu", *args), C.run_operator("cpu", *args))


@pytest.mark.parametrize("tag", ["synapse_epa", "acdc_epa"])
def test_training_mode_with_injected_masks(tag):
    """E is F (Synapse: the shared layer's gradient is the sum of both uses) and separate E, F (ACDC)."""
    m = C.check_module_against_restatement("cpu", tag, train_masks=True)
    assert (m.E is m.F) == tag.startswith("synapse")


def test_uncovered_width_runs_operator_by_operator():
    m = C.check_module_against_restatement("cpu", C=48, N=60, P=32)
    assert not m.fused(torch.zeros(2, 60, 48))


def test_module_interface():
    from deformablelka_amd import acdc, transformerblock
    from deformablelka_amd.ops import epa
    for tag, keys in C.STATE_KEYS.items():
        cfg = dict(input_size=120, hidden_size=32, proj_size=32, num_heads=4)
        m = C.classes(tag)(**cfg) if tag.endswith("epa") else C.classes(tag)(**cfg, dropout_rate=0.1, pos_embed=True)
        assert list(m.state_dict().keys()) == keys, tag
        e = m if tag.endswith("epa") else m.epa_block
        assert e.no_weight_decay() == {"temperature", "temperature2"}
        assert (e.E is e.F) == tag.startswith("synapse")
    assert isinstance(acdc.TransformerBlock(120, 32, 32, 4).conv52, type(transformerblock.TransformerBlock(120, 32, 32, 4).conv51))
    assert epa.supported(32, 4, 32, torch.float32) and epa.supported(256, 4, 64, torch.float32)
    assert not epa.supported(48, 4, 32, torch.float32) and not epa.supported(32, 4, 48, torch.float32) and not epa.supported(32, 4, 32, torch.bfloat16)
    with pytest.raises(RuntimeError, match="not implemented|unsupported|-8"):
        t = C.make_operator(12, 32, 60)[0]
        epa.attention_forward(t["qkvv"], t["kp"], t["vp"], t["temperature"], t["temperature2"])
    m = transformerblock.EPA(60, 32, 32).train()   # eval mode or p = 0: no mask exists
    assert m._draw_masks(2, 60, "cpu")[0] is not None and m.eval()._draw_masks(2, 60, "cpu")[:2] == (None, None)
    assert transformerblock.EPA(60, 32, 32, channel_attn_drop=0.0, spatial_attn_drop=0.0).train()._draw_masks(2, 60, "cpu")[:2] == (None, None)


@pytest.mark.parametrize("tag", ["synapse_epa", "acdc_epa", "synapse_block", "acdc_block"])
def test_per_op_forward_reproduces_the_reference(tag):
    """What an uncovered width, bf16 autocast or a CPU tensor takes: forward_per_op, torch only, against the reference's own records."""
    C.check_module_against_reference(tag, "cpu", per_op=True)


def test_block_routes_what_the_kernels_do_not_cover():
    from deformablelka_amd import _lib, transformerblock
    m = transformerblock.TransformerBlock(24, 48, 32, 4, pos_embed=True).eval()
    x = torch.randn(1, 48, 2, 3, 4)
    assert not m.on_kernels(x) and m.on_kernels(torch.randn(1, 64, 2, 3, 4))
    assert m(x).shape == x.shape                      # hidden_size 48: no multiple of 32
    m = transformerblock.TransformerBlock(24, 32, 32, 4).eval()
    x = torch.randn(1, 32, 2, 3, 4)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert not m.on_kernels(x)
        assert bool(torch.isfinite(m(x).float()).all())
    backend, _lib._test_backend = _lib._test_backend, False   # a CPU tensor without the emulator behind the library
    try:
        assert not m.on_kernels(x) and not m.epa_block.fused(x.flatten(2).transpose(1, 2))
        assert m(x).shape == x.shape
    finally:
        _lib._test_backend = backend


def test_unaligned_views_are_accepted():
    C.check_offset_views("cpu")


REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF + "/3D/d_lka_former"), reason="/root/reference is not mounted here")

_IMPORT_SITES = """
sites = [   # (file of the reference that imports block classes by name, module path it imports them from, this package's module)
    ("3D/d_lka_former/network_architecture/synapse/model_components.py", "d_lka_former.network_architecture.synapse.transformerblock", dk.transformerblock),
    ("3D/d_lka_former/network_architecture/synapse/d_lka_former_synapse.py", "d_lka_former.network_architecture.synapse.transformerblock", dk.transformerblock),
    ("3D/d_lka_former/network_architecture/acdc/model_components.py", "d_lka_former.network_architecture.acdc.transformerblock", dk.acdc),
    ("3D/pancreas_code/networks/d_lka_former/model_components.py", "networks.d_lka_former.transformerblock", dk.transformerblock),
    ("3D/pancreas_code/networks/d_lka_former/d_lka_net_synapse.py", "networks.d_lka_former.transformerblock", dk.transformerblock),
]
"""


@needs_ref
def test_reference_import_lines_get_the_blocks():
    """INTEGRATION.md section 5i, executed in a fresh interpreter: after install_reference_blocks() the reference's own ``from ...transformerblock import
    TransformerBlock, TransformerBlock_3D_LKA, ...`` lines — read from its model_components.py / net files and executed as they stand — succeed, bind
    TransformerBlock (and EPA, TransformerBlock_3D_single_deform_LKA) to this package's classes and every ablation block to the reference's own; and
    run_training.py's lookup ``getattr(importlib.import_module(path), "TransformerBlock")`` gives the same class."""
    code = ("import sys, types, importlib\n"
            "import deformablelka_amd as dk\n"
            "REF = %r\n"
            "sys.path.insert(0, 'tests/golden')\n"
            "import make_golden\n"
            "make_golden._install_stubs(native=False)\n"
            "dk.install_reference_aliases(names=('D3D',) + dk.NET_ALIASES, torchvision_ops=True)\n"
            "sys.path[:0] = [REF + '/3D', REF + '/3D/pancreas_code']\n"
            "for name, path in (('d_lka_former', '/3D/d_lka_former'), ('d_lka_former.network_architecture', '/3D/d_lka_former/network_architecture'),\n"
            "                   ('d_lka_former.network_architecture.synapse', '/3D/d_lka_former/network_architecture/synapse'),\n"
            "                   ('d_lka_former.network_architecture.acdc', '/3D/d_lka_former/network_architecture/acdc'),\n"
            "                   ('networks', '/3D/pancreas_code/networks'), ('networks.d_lka_former', '/3D/pancreas_code/networks/d_lka_former')):\n"
            "    m = types.ModuleType(name); m.__path__ = [REF + path]; sys.modules[name] = m\n"
            "mods = dk.install_reference_blocks()\n"
            "assert [m.__name__ for m in mods] == list(dk.BLOCK_ALIASES) and all(m.__file__.startswith(REF) for m in mods)\n"
            + _IMPORT_SITES +
            "for rel, path, ours in sites:\n"
            "    lines = [l for l in open(REF + '/' + rel).read().splitlines() if l.startswith('from ' + path + ' import ')]\n"
            "    assert len(lines) == 1, (rel, lines)\n"
            "    ns = {}\n"
            "    exec(lines[0], ns)\n"
            "    names = [k for k in ns if k != '__builtins__']\n"
            "    assert 'TransformerBlock' in names and len(names) >= 2, (rel, names)\n"
            "    for k in names:\n"
            "        if k in dk.BLOCK_NAMES:\n"
            "            assert ns[k] is getattr(ours, k), (rel, k)\n"
            "        else:\n"
            "            assert ns[k].__module__ == path, (rel, k, ns[k].__module__)\n"
            "    assert getattr(importlib.import_module(path), 'TransformerBlock') is ours.TransformerBlock\n"
            "    assert importlib.import_module(path).EPA is ours.EPA\n"
            "try:\n"
            "    dk.install_reference_blocks(names=('no.such.module',))\n"
            "except KeyError:\n"
            "    print('blocks ok')\n") % REF
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, env=dict(os.environ, PYTHONPATH=root))
    assert out.returncode == 0 and "blocks ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
