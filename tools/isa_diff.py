#!/usr/bin/env python3
"""Device assembly of every translation unit of the model builds (srbd_horizon_amd/_lib.py translation_units), and its
comparison between two trees, kernel by kernel: the proof that a refactor left the device code alone.

    python tools/isa_diff.py dump OUTDIR [--root TREE] [-j JOBS]     # OUTDIR/<unit>.s, compiled with --save-temps
    python tools/isa_diff.py diff PARENT_DIR BRANCH_DIR

dump compiles csrc/sddp_inst.hip of TREE (default: this tree) by TREE's own _lib: its unit list and its command line, so two
trees whose unit recipes differ are each compiled exactly as their own build() compiles them.  diff drops comments, takes the
function number out of the basic-block labels and compares what is left of every kernel line by line; it exits 1 if the two
directories hold different units, a unit holds different kernel names, or a kernel differs."""
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
        body = (re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r";.*$", "", l).rstrip()) for l in lines[i + 1:j])
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
    total = differing = 0
    for unit in sorted(up & ub):
        kp, kb = kernels(os.path.join(args.parent, unit + ".s")), kernels(os.path.join(args.branch, unit + ".s"))
        bad = sorted(set(kp) ^ set(kb))
        lines = 0
        for name in sorted(set(kp) & set(kb)):
            lines += len(kb[name])
            if kp[name] != kb[name]:
                bad.append(name)
                for x in list(difflib.unified_diff(kp[name], kb[name], lineterm="", n=0))[:8]:
                    print("   ", x)
        total += len(kb)
        differing += len(bad)
        print(f"{unit:<14} {len(kb):>3} kernels, {lines:>8} instructions and labels, differing kernels: {len(bad)}" + "".join("\n    " + b for b in bad))
    print(f"{len(up & ub)} units in both, {len(up ^ ub)} in one only, {total} kernels, differing kernels: {differing}")
    return 1 if differing or up ^ ub else 0


if __name__ == "__main__":
    sys.exit(main())
