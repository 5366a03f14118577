#!/usr/bin/env python3
"""Device assembly of every translation unit of the model builds (srbd_horizon_amd/_lib.py translation_units), and its
comparison between two trees, kernel by kernel: the proof that a refactor left the device code alone.

    python tools/isa_diff.py dump OUTDIR [--root TREE] [-j JOBS]     # OUTDIR/<unit>.s, compiled with --save-temps
    python tools/isa_diff.py diff PARENT_DIR BRANCH_DIR

dump compiles csrc/sddp_inst.hip of TREE (default: this tree) by TREE's own _lib: its unit list and its command line, so two
trees whose unit recipes differ are each compiled exactly as their own build() compiles them.  diff drops comments, takes the
function number out of the basic-block labels and compares what is left of every kernel line by line.  Kernels are matched by name:
in their own unit where both trees have them there, else wherever the other tree holds them, reported under the branch's unit as
"moved <from> -> <to>: same | differing".  The two trees need not hold the same units.  It exits 1 if a kernel differs, is gone
from the branch, or is in the branch alone."""
import argparse
import difflib
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lib_of(root):
    """srbd_horizon_amd/_lib.py of the tree at `root`, loaded beside whatever this process has imported"""
    spec = importlib.util.spec_from_file_location("_lib_of_tree", os.path.join(root, "srbd_horizon_amd", "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dump(lib, unit, outdir):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = lib.compile_command(unit) + ["--save-temps", "-c", os.path.join(lib.CSRC, "sddp_inst.hip"), "-o", os.path.join(tmp, "inst.o")]
        subprocess.run(cmd, check=True, cwd=tmp, capture_output=True)
        shutil.copy(os.path.join(tmp, "sddp_inst-hip-amdgcn-amd-amdhsa-gfx950.s"), os.path.join(outdir, unit + ".s"))
    return unit


def kernels(path):
    """kernel name -> its normalised body"""
    lines = open(path).read().split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    start = {l.split(":")[0]: i for i, l in enumerate(lines) if re.match(r"^[A-Za-z_][\w.$]*:\s*(;.*)?$", l)}
    out = {}
    for name in names:
        i = j = start[name]
        while not lines[j].startswith(".Lfunc_end"):
            j += 1
        # (.Lpost_getpc<n>, the label of a long branch, is numbered through the module like the functions)
        body = (re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r";.*$", "", l).rstrip())) for l in lines[i + 1:j])
        out[name] = [l for l in body if l.strip()]
    return out


def units_in(path):
    return {f[:-2] for f in os.listdir(path) if f.endswith(".s")}


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
    if args.mode == "dump":
        lib = lib_of(os.path.abspath(args.root))
        os.makedirs(args.outdir, exist_ok=True)
        with ThreadPoolExecutor(max_workers=max(1, args.j)) as ex:
            for unit in ex.map(lambda u: dump(lib, u, args.outdir), [name for name, _ in lib.translation_units()]):
                print("dumped", unit, file=sys.stderr, flush=True)
        return 0
    up, ub = units_in(args.parent), units_in(args.branch)
    for unit in sorted(up ^ ub):
        print(f"{unit:<14} only in {args.parent if unit in up else args.branch}")
    parent = {u: kernels(os.path.join(args.parent, u + ".s")) for u in up}
    branch = {u: kernels(os.path.join(args.branch, u + ".s")) for u in ub}
    # a kernel that its own unit no longer holds is looked for in the rest of the other tree: (name, parent unit) <-> (name, branch unit)
    left = {(n, u) for u in up for n in parent[u] if n not in branch.get(u, {})}
    came_from = {}
    for u in sorted(ub):
        for n in sorted(set(branch[u]) - set(parent.get(u, {}))):
            src = min((pu for pn, pu in left if pn == n), default=None)
            if src is not None:
                left.discard((n, src))
                came_from[(n, u)] = src
    total = differing = moved = 0
    for unit in sorted(up | ub):
        kp, kb = parent.get(unit, {}), branch.get(unit, {})
        bad = sorted([n for n in kp if (n, unit) in left] + [n for n in kb if n not in kp and (n, unit) not in came_from])      # gone, new
        notes, lines = [], 0
        for name in sorted(kb):
            src = unit if name in kp else came_from.get((name, unit))
            if src is None:
                continue
            lines += len(kb[name])
            same = parent[src][name] == kb[name]
            if not same:
                bad.append(name)
                for x in list(difflib.unified_diff(parent[src][name], kb[name], lineterm="", n=0))[:8]:
                    print("   ", x)
            if src != unit:
                moved += 1
                notes.append(f"{name}  moved {src} -> {unit}: {'same' if same else 'differing'}")
        total += len(kb)
        differing += len(bad)
        if unit in ub or bad:
            print(f"{unit:<14} {len(kb):>3} kernels, {lines:>8} instructions and labels, differing kernels: {len(bad)}"
                  + "".join("\n    " + b for b in bad + notes))
    print(f"{len(up & ub)} units in both, {len(up ^ ub)} in one only, {total} kernels, differing kernels: {differing}"
          + (f", moved: {moved}" if moved else ""))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
