"""Generates tests/golden/reference_epa.pt, reference_epa_block_synapse.pt, reference_epa_block_acdc.pt and reference_epa_block_acdc_conv_grads.pt by running the REFERENCE'S OWN ``EPA`` and ``TransformerBlock`` (synapse/transformerblock.py:6-138 and
acdc/transformerblock.py:6-137, imported through the helpers of make_golden.py, not edited) on the CPU in eval mode: input, state_dict, output and
every gradient at C = 32, N = 4 * 5 * 6, P = 32, B = 2, with temperature, temperature2 and gamma moved off their initial values.  N != C, so the
fixture pins the permute-and-reshape order of x_SA.  Run:  python tests/golden/make_golden_epa.py"""
import importlib
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402

B, C, DIMS, P, HEADS = 2, 32, (4, 5, 6), 32, 4
N = DIMS[0] * DIMS[1] * DIMS[2]


def _prepare(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("temperature") or name.endswith("temperature2"):
                p.copy_(0.5 + 2.0 * torch.rand(p.shape, generator=g))
            elif name.endswith("gamma"):
                p.copy_(0.5 + 0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith("pos_embed"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
        for name, b in m.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.1 * torch.randn(b.shape, generator=g))
            elif name.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
    return m.eval()


def main():
    tb_syn = make_golden._import_reference()[0]
    name = "d_lka_former.network_architecture.acdc"
    pkg = types.ModuleType(name)
    pkg.__path__ = [f"{make_golden.REF}/3D/d_lka_former/network_architecture/acdc"]
    sys.modules[name] = pkg
    tb_acdc = importlib.import_module(name + ".transformerblock")
    out = {"config": {"B": B, "C": C, "dims": DIMS, "P": P, "heads": HEADS}}
    for tag, tb in (("synapse", tb_syn), ("acdc", tb_acdc)):
        torch.manual_seed(7)
        epa = _prepare(tb.EPA(input_size=N, hidden_size=C, proj_size=P, num_heads=HEADS), 1)
        x = torch.randn(B, N, C, generator=torch.Generator().manual_seed(2))
        out[tag + "_epa"] = make_golden._run(epa, [x], seed=3)
        blk = _prepare(tb.TransformerBlock(input_size=N, hidden_size=C, proj_size=P, num_heads=HEADS, dropout_rate=0.1, pos_embed=True), 4)
        xv = torch.randn(B, C, *DIMS, generator=torch.Generator().manual_seed(5))
        out[tag + "_block"] = make_golden._run(blk, [xv], seed=6)
    # one file per record group, each inside the committed-file limit.  The ACDC block's four 3^3 conv weights alone are 442 KB, so their gradients go to a
    # file of their own (tests/epa_cases.py puts them back into the record's grad_params)
    gp = out["acdc_block"]["grad_params"]
    out["acdc_block_conv_grads"] = {k: gp.pop(k) for k in [k for k in gp if k.startswith("conv5") and k.endswith("conv.weight")]}
    assert len(out["acdc_block_conv_grads"]) == 4
    for name, keys in (("reference_epa.pt", ("synapse_epa", "acdc_epa")), ("reference_epa_block_synapse.pt", ("synapse_block",)),
                       ("reference_epa_block_acdc.pt", ("acdc_block",)), ("reference_epa_block_acdc_conv_grads.pt", ("acdc_block_conv_grads",))):
        path = os.path.join(make_golden.OUT, name)
        torch.save({"config": out["config"], **{k: out[k] for k in keys}}, path)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
