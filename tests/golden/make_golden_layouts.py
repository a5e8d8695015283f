"""Records what every buffer-size / buffer-offset export of the composite blocks returns (host-compiled library, tests/emu; nothing runs on a device):

    python tests/golden/make_golden_layouts.py        # writes tests/golden/block_layouts.json

The table is the contract of the blocks' `saved` / `workspace` layouts: DLKABlockStack's flat buffers and tests/pw_chain.py compute positions from these
values, and memory use is behaviour.  tests/test_layouts_emu.py asserts that the tree reproduces every value exactly.  Regenerate only when a layout is
changed on purpose.  (The plain 2-D block's and dlka_dwconv2d_cl_workspace's rows were recorded from the commit before csrc/capi_lka2d_frame.h existed;
the rows already recorded did not move.)

File format: {"grid": GRID, "values": {export name: [numbers]}}.  An export's numbers are what its calls returned (return value, then its output values), in
the order collect() makes the calls: that order is a function of GRID alone, which the file repeats so that a changed grid cannot be mistaken for a changed
layout."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "block_layouts.json")

GRID = {
    "dw_lds": [0, 1],                                                # DLKA_DW_LDS unset / "1" (dlka_env_refresh after each change)
    "batches": [1, 2],
    "dtypes": [0, 1],                                                # DLKA_F32, DLKA_BF16
    "widths3d": [32, 64, 128, 256, 48],                              # 48: outside the token path (0 / DLKA_ERR_UNSUPPORTED)
    "volumes": [[4, 4, 4], [8, 8, 8], [3, 9, 17], [5, 6, 7], [32, 32, 32], [4, 0, 4]],   # the last: a zero extent
    "variants": [0, 1, 2],                                           # 2: no such variant
    "widths2d": [96, 384, 40],
    "planes": [[56, 56], [14, 14], [11, 11], [0, 11]],
    "lka2d_general": [0, 1],                                         # dlka_lka2d_force_general, for dlka_lka2d_saved_offsets (the sizes do not depend on it)
    "dw2d_members": [[5, 1, 2], [7, 3, 9]],                          # (k, dilation, padding) of dlka_dwconv2d_cl_workspace, forward and backward
}


def collect(lib):
    """lib: a ctypes library bound by deformablelka_amd._lib.bind.  Returns {export: [(arguments and switches, [values]), ...]}; leaves DLKA_DW_LDS unset and
    the 2-D path switch as it found it."""
    from deformablelka_amd._lib import ConvGeom
    rows = {}

    def rec(name, args, *vals):
        rows.setdefault(name, []).append((tuple(args), [int(v) for v in vals]))

    def outs(fn, args, n):
        o = (ctypes.c_size_t * n)()
        return [int(fn(*args, o))] + [int(v) for v in o]

    old_general = lib.dlka_lka2d_force_general(0)
    try:
        for lds in GRID["dw_lds"]:
            if lds:
                os.environ["DLKA_DW_LDS"] = str(lds)
            else:
                os.environ.pop("DLKA_DW_LDS", None)
            lib.dlka_env_refresh()
            for C in GRID["widths3d"]:
                for (D, H, W) in GRID["volumes"]:
                    for B in GRID["batches"]:
                        for dt in GRID["dtypes"]:
                            a = (B, C, D, H, W, dt)
                            for name in ("dlka_lka3d_saved_bytes", "dlka_lka3d_workspace_bytes", "dlka_lka3d_tokens_saved_bytes",
                                         "dlka_lka3d_tokens_workspace_bytes", "dlka_tblock3d_saved_bytes", "dlka_tblock3d_workspace_bytes"):
                                rec(name, a + (lds,), getattr(lib, name)(*a))
                            for v in GRID["variants"]:
                                av = a + (v,)
                                for name in ("dlka_lka3d_tokens_saved_bytes_v", "dlka_lka3d_tokens_workspace_bytes_v", "dlka_lka3d_tokens_partials_bytes_v",
                                             "dlka_tblock3d_saved_bytes_v", "dlka_tblock3d_workspace_bytes_v"):
                                    rec(name, av + (lds,), getattr(lib, name)(*av))
                                rec("dlka_lka3d_tokens_saved_offsets_v", av + (lds,), *outs(lib.dlka_lka3d_tokens_saved_offsets_v, av, 1))
                                rec("dlka_tblock3d_saved_offsets_v", av + (lds,), *outs(lib.dlka_tblock3d_saved_offsets_v, av, 1))
                                rec("dlka_tblock3d_saved_activations_v", av + (lds,), *outs(lib.dlka_tblock3d_saved_activations_v, av, 2))
            for C in GRID["widths2d"]:
                for (H, W) in GRID["planes"]:
                    for B in GRID["batches"]:
                        for dt in GRID["dtypes"]:
                            a = (B, C, H, W, dt)
                            rec("dlka_lka2d_saved_bytes", a + (lds,), lib.dlka_lka2d_saved_bytes(*a))
                            rec("dlka_lka2d_workspace_bytes", a + (lds,), lib.dlka_lka2d_workspace_bytes(*a))
                            for general in GRID["lka2d_general"]:
                                lib.dlka_lka2d_force_general(general)
                                o = (ctypes.c_size_t * 2)()
                                eb = ctypes.c_int(0)
                                rc = lib.dlka_lka2d_saved_offsets(*a, o, ctypes.byref(eb))
                                rec("dlka_lka2d_saved_offsets", a + (lds, general), rc, o[0], o[1], eb.value)
                            lib.dlka_lka2d_force_general(0)
                            rec("dlka_lka2d_plain_saved_bytes", a + (lds,), lib.dlka_lka2d_plain_saved_bytes(*a))
                            rec("dlka_lka2d_plain_workspace_bytes", a + (lds,), lib.dlka_lka2d_plain_workspace_bytes(*a))
                            for (k, dil, pad) in GRID["dw2d_members"]:
                                g = ConvGeom(B, C, 1, H, W, C, 1, k, k, 1, 1, 1, 0, pad, pad, 1, dil, dil, C, 1, 64)
                                for backward in (0, 1):
                                    rec("dlka_dwconv2d_cl_workspace", a + (k, backward, lds), lib.dlka_dwconv2d_cl_workspace(ctypes.byref(g), dt, backward))
    finally:
        os.environ.pop("DLKA_DW_LDS", None)
        lib.dlka_env_refresh()
        lib.dlka_lka2d_force_general(old_general)
    return rows


def main():
    sys.path.insert(0, ROOT)
    from deformablelka_amd import _lib
    from tests import emu
    rows = collect(_lib.bind(emu.load()))
    values = {name: [v for _, vals in rows[name] for v in vals] for name in sorted(rows)}
    with open(OUT, "w") as f:
        f.write('{"grid": ' + json.dumps(GRID, separators=(",", ":")) + ',\n "values": {\n')
        f.write(",\n".join(json.dumps(name) + ":" + json.dumps(v, separators=(",", ":")) for name, v in values.items()))
        f.write("\n}}\n")
    print(f"{OUT}: {sum(len(v) for v in values.values())} values of {len(values)} exports")


if __name__ == "__main__":
    main()
