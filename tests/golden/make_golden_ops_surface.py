"""Generates tests/golden/ops_surface.json: the names ``deformablelka_amd.ops`` exposes, with their signatures (functions) and values (constants).
Run from the repository root; neither the GPU nor the library is needed:

    python tests/golden/make_golden_ops_surface.py --recorded-from COMMIT [--out FILE]

on a checkout of COMMIT, the commit BEFORE ops.py became the package ops/: the record is that commit's, a regression record of a refactor that
must leave the surface alone.  It is never regenerated from the code under test.  Recorded: every public function and plain-data constant in
``vars(ops)``, and the underscore names that code outside ops reaches through ``ops`` (deformablelka_amd/, tests/ and scripts/ are scanned for
them).  The fixture holds names, signature strings and reprs only."""
import argparse
import inspect
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "ops_surface.json")
CONSTANT_TYPES = (bool, int, float, str, tuple, list, dict, frozenset)
SCANNED = ("deformablelka_amd", "tests", "scripts")


def describe(value):
    """The record of one name, or None for what is neither a function nor a plain-data constant (modules, imported types, ...)."""
    if inspect.isfunction(value):
        return {"kind": "function", "signature": str(inspect.signature(value))}
    if isinstance(value, CONSTANT_TYPES):
        return {"kind": "constant", "repr": repr(value)}
    return None


def public_surface(ops):
    """name -> record of the public functions and constants in vars(ops)."""
    return {n: d for n, d in ((n, describe(v)) for n, v in vars(ops).items() if not n.startswith("_")) if d is not None}


def private_names_used_outside():
    """The underscore names reached through ``ops`` from outside deformablelka_amd/ops (file or package)."""
    own = os.path.join(ROOT, "deformablelka_amd", "ops")
    names = set()
    for top in SCANNED:
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                path = os.path.join(dirpath, f)
                if f.endswith(".py") and path != own + ".py" and not path.startswith(own + os.sep):
                    with open(path, encoding="utf-8") as fh:
                        names.update(re.findall(r"ops\.(_[A-Za-z]\w*)", fh.read()))
    return sorted(names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--recorded-from", required=True, help="the commit this checkout is at")
    args = ap.parse_args()
    from deformablelka_amd import ops
    private = {n: describe(getattr(ops, n)) for n in private_names_used_outside()}
    assert all(private.values()), [n for n, d in private.items() if d is None]
    rec = {"recorded_from": f"commit {args.recorded_from}: the parent of the commit that turned ops.py into the package ops/",
           "public": public_surface(ops), "private": private}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    kinds = [d["kind"] for d in rec["public"].values()]
    print(f"{args.out}: {kinds.count('function')} public functions, {kinds.count('constant')} public constants, {len(private)} private names")


if __name__ == "__main__":
    main()
