"""Generates tests/golden/stack_sequences.json: which kernels a small DLKABlockStack launches over its first three steps, in order, in each
configuration of tests/stack_seq_cases.py.  Run from the repository root, on a machine with the GPU:

    python tests/golden/make_golden_stack_sequences.py --recorded-from COMMIT [--out FILE]

with the library AND deformablelka_amd/stack.py of COMMIT, the commit BEFORE DLKABlockStack.backward() was split into one method per schedule and the
settled experiments were retired: the record is that commit's, a regression record of a host-code refactor.  It is never regenerated from the code
under test.  The fixture holds names only."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import stack_seq_cases as C  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=C.FIXTURE)
    ap.add_argument("--recorded-from", required=True, help="the commit the library and stack.py were taken from")
    args = ap.parse_args()
    rec = {"recorded_from": f"commit {args.recorded_from}: the parent of the commit that split DLKABlockStack.backward() and retired the settled experiments",
           "launches": {cid: C.sequences("cuda:0", cid) for cid in C.CASE_IDS}}
    assert all(all(p.values()) for p in rec["launches"].values())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: " + ", ".join(f"{cid} {[len(v) for v in p.values()]}" for cid, p in rec["launches"].items()))


if __name__ == "__main__":
    main()
