"""Generates tests/golden/refusal_codes.json: the status every call of tests/refusal_cases.py returns.  Run from the repository root:

    python tests/golden/make_golden_refusals.py --parent-lib LIB

LIB is a wavefront-emulator build (tests/emu) of the commit BEFORE csrc/cl_pipeline.h, whose entry points still carry their own hand-written
checks: the statuses are that commit's, a regression record of which refusal each bad descriptor gets and which of two bad fields is reported
first.  They are never taken from the code under test.  The fixture holds names and integers only."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from deformablelka_amd import _lib   # noqa: E402
from tests import refusal_cases as C  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    args = ap.parse_args()
    codes = C.run(_lib.bind(ctypes.CDLL(os.path.abspath(args.parent_lib))))
    launched = [k for k, v in codes.items() if v == 0 and k not in C.NO_WORK]
    assert not launched, f"not refused: {launched}"
    with open(C.FIXTURE, "w") as f:
        json.dump(codes, f, indent=0, sort_keys=True)
        f.write("\n")
    hist = {}
    for v in codes.values():
        hist[v] = hist.get(v, 0) + 1
    print(f"{C.FIXTURE}: {len(codes)} cases, statuses {dict(sorted(hist.items()))}")


if __name__ == "__main__":
    main()
