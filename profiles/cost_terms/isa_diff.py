#!/usr/bin/env python3
"""The device assembly of every translation unit of two trees, kernel by kernel (`dump` and `kernels` of
profiles/build_table/isa_diff.py over _lib.translation_units(), the list build() compiles):

    python profiles/cost_terms/isa_diff.py dump OUTDIR [--root TREE] [-j JOBS]     # OUTDIR/<unit>.s
    python profiles/cost_terms/isa_diff.py diff PARENT_DIR BRANCH_DIR              # the table of isa_diff.txt

Both trees are compiled by this tree's command lines.  diff counts, per unit, the parent's kernels that differ, that are gone and the
kernels that are new, names the new ones by their template, and exits 1 if a kernel of the parent differs or is gone."""
import argparse
import importlib.util
import os
import re
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from srbd_horizon_amd import _lib  # noqa: E402

_spec = importlib.util.spec_from_file_location("build_table_isa_diff", os.path.join(ROOT, "profiles", "build_table", "isa_diff.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="mode", required=True)
    d = sub.add_parser("dump")
    d.add_argument("outdir")
    d.add_argument("--root", default=ROOT)
    d.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    c = sub.add_parser("diff")
    c.add_argument("parent")
    c.add_argument("branch")
    args = ap.parse_args()
    units = [name for name, _ in _lib.translation_units()]
    if args.mode == "dump":
        os.makedirs(args.outdir, exist_ok=True)
        with ThreadPoolExecutor(max_workers=max(1, args.j)) as ex:
            for unit in ex.map(lambda u: base.dump(u, args.root, args.outdir), units):
                print("dumped", unit, file=sys.stderr, flush=True)
        return 0
    both = differing = gone = 0
    fresh = set()
    for unit in sorted(units):
        kp, kb = base.kernels(os.path.join(args.parent, unit + ".s")), base.kernels(os.path.join(args.branch, unit + ".s"))
        diff = [n for n in sorted(set(kp) & set(kb)) if kp[n] != kb[n]]
        lost, new = sorted(set(kp) - set(kb)), sorted(set(kb) - set(kp))
        both += len(set(kp) & set(kb))
        differing += len(diff)
        gone += len(lost)
        fresh |= {re.match(r"(_ZN4sddp\d+[a-z_0-9]+?)I", n).group(1) if re.match(r"(_ZN4sddp\d+[a-z_0-9]+?)I", n) else n for n in new}
        print(f"{unit:<14} {len(kp):>3} kernels of the parent, differing: {len(diff)}, gone: {len(lost)}, new: {len(new)}"
              + "".join("\n    differs: " + n for n in diff) + "".join("\n    gone: " + n for n in lost))
    print(f"{len(units)} units, {both} kernels in both trees, differing kernels: {differing}")
    print("new kernels: " + ", ".join(sorted(fresh)))
    return 1 if differing or gone else 0


if __name__ == "__main__":
    sys.exit(main())
