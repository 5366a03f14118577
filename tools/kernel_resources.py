"""Code-object resources of every kernel of every translation unit of the model builds (srbd_horizon_amd/_lib.py translation_units:
one unit per entry of INSTANCES, the side units `<build>_resume` and `<build>_log` of the plain builds' further solve variants,
_lib.VARIANTS, and every build's `<build>_inspect` unit of the kernels that only read a plan): SGPRs, VGPRs, AGPRs, scratch bytes per lane, occupancy (waves per SIMD) and static LDS, as the compiler reports
them for gfx950.

    python tools/kernel_resources.py [-j JOBS] [--only srbd13,srbd13_resume] [--root OTHER_TREE] > resources.txt

Each unit is compiled device-only with build()'s own command (_lib.compile_command) plus -Rpass-analysis=kernel-resource-usage;
nothing is linked or written beside the table.  Two trees compile to the same kernels exactly when their tables are equal line by
line: what a change that must leave the existing kernels alone is checked with (profiles/iteration_refactor, profiles/hetero,
profiles/build_table, profiles/solve_variants; tools/isa_diff.py compares the instructions).  --root compiles another tree's csrc
by THIS tree's unit list and definitions: a tree whose unit recipe differs is tabulated by its own copy of this tool.  The LDS
column is 0 for every kernel that uses dynamic LDS only."""
import argparse
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from srbd_horizon_amd import _lib  # noqa: E402

FIELDS = (("SGPR", r"TotalSGPRs: (\d+)"), ("VGPR", r"\bVGPRs: (\d+)"), ("AGPR", r"\bAGPRs: (\d+)"),
          ("Scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("Occ", r"Occupancy \[waves/SIMD\]: (\d+)"),
          ("LDS", r"LDS Size \[bytes/block\]: (\d+)"))


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool or not names:
        return names                          # the mangled names identify the kernels as well
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
    return out.stdout.splitlines()


def compile_one(fn, root=ROOT):
    cmd = _lib.compile_command(fn, root) + ["--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                            os.path.join(root, "srbd_horizon_amd", "csrc", "sddp_inst.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{fn}: {r.stderr[-2000:]}")
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = dict(name=m.group(1))
            rows.append(cur)
            continue
        if cur is not None:
            for key, pat in FIELDS:
                m = re.search(pat, line)
                if m:
                    cur[key] = int(m.group(1))
    for row, name in zip(rows, demangle([r_["name"] for r_ in rows])):
        row["name"] = re.sub(r"\(.*$", "", name)
    return fn, rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--only", default="", help="comma-separated unit names of _lib.translation_units()")
    ap.add_argument("--root", default=ROOT, help="the tree whose csrc is compiled, with this tree's unit list and command (default: this tree)")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    jobs = [name for name, _ in _lib.translation_units() if not only or name in only]
    with ThreadPoolExecutor(max_workers=max(1, args.j)) as ex:
        done = dict(ex.map(lambda fn: compile_one(fn, args.root), jobs))
    print(f"{'build':<10} {'kernel':<72} {'SGPR':>5} {'VGPR':>5} {'AGPR':>5} {'Scratch':>8} {'Occ':>4} {'LDS':>7}")
    for fn in sorted(done):
        for r in done[fn]:
            print(f"{fn:<10} {r['name'][:72]:<72} {r.get('SGPR', 0):>5} {r.get('VGPR', 0):>5} {r.get('AGPR', 0):>5} "
                  f"{r.get('Scratch', 0):>8} {r.get('Occ', 0):>4} {r.get('LDS', 0):>7}")


if __name__ == "__main__":
    main()
