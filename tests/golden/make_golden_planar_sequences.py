"""Generates tests/golden/planar_sequences.json: what the size queries of the general NCDHW path return and which kernels its backward entry points
launch, in order (tests/planar_seq_cases.py has the shapes and the calls).  Run from the repository root, on a machine with the GPU:

    python tests/golden/make_golden_planar_sequences.py --recorded-from COMMIT [--out FILE]

with the library built from COMMIT, the commit BEFORE csrc/dlka_capi.hip's backward launch sequences were written once (deform_bwd_seq / conv_bwd_seq): the
record is that commit's, a regression record of a host-code refactor.  It is never regenerated from the code under test.  The fixture holds names
and integers only."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from deformablelka_amd import _lib   # noqa: E402
from tests import planar_seq_cases as C  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=C.FIXTURE)
    ap.add_argument("--recorded-from", required=True, help="the commit the library was built from")
    args = ap.parse_args()
    lib = _lib.get_lib()
    rec = {"recorded_from": f"commit {args.recorded_from}: the parent of the commit that introduced deform_bwd_seq / conv_bwd_seq",
           "sizes": C.sizes(lib), "launches": {cid: C.launches("cuda:0", cid) for cid in C.LAUNCH_IDS}}
    assert all(v > 0 for v in rec["sizes"].values()), [k for k, v in rec["sizes"].items() if v <= 0]
    assert all(rec["launches"].values())
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {len(rec['sizes'])} sizes, {len(rec['launches'])} launch sequences of {sorted(len(v) for v in rec['launches'].values())} kernels")


if __name__ == "__main__":
    main()
