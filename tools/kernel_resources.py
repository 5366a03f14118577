"""Code-object resources of every kernel of every model build (srbd_horizon_amd/_lib.py INSTANCES): SGPRs, VGPRs, AGPRs, scratch
bytes per lane, occupancy (waves per SIMD) and static LDS, as the compiler reports them for gfx950.

    python tools/kernel_resources.py [-j JOBS] [--only srbd13,srbd37] > resources.txt

Each build is compiled device-only with build()'s own flags plus -Rpass-analysis=kernel-resource-usage; nothing is linked or
written beside the table.  Two trees compile to the same kernels exactly when their tables are equal line by line: what a change
that must leave the existing kernels alone is checked with (profiles/iteration_refactor, profiles/hetero).  The LDS column is 0
for every kernel that uses dynamic LDS only."""
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


def compile_one(job):
    fn, model, mname = job
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-I" + _lib.INCLUDE, "-I" + _lib.CSRC,
           "-DSDDP_INST_MODEL=" + model, "-DSDDP_INST_FN=ops_" + fn, '-DSDDP_INST_NAME="' + mname + '"', *_lib.INSTANCE_FLAGS.get(fn, []),
           "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(_lib.CSRC, "sddp_inst.hip"), "-o", os.devnull]
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
    ap.add_argument("--only", default="", help="comma-separated accessor suffixes of _lib.INSTANCES")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    jobs = [j for j in _lib.INSTANCES if not only or j[0] in only]
    with ThreadPoolExecutor(max_workers=max(1, args.j)) as ex:
        done = dict(ex.map(compile_one, jobs))
    print(f"{'build':<10} {'kernel':<72} {'SGPR':>5} {'VGPR':>5} {'AGPR':>5} {'Scratch':>8} {'Occ':>4} {'LDS':>7}")
    for fn in sorted(done):
        for r in done[fn]:
            print(f"{fn:<10} {r['name'][:72]:<72} {r.get('SGPR', 0):>5} {r.get('VGPR', 0):>5} {r.get('AGPR', 0):>5} "
                  f"{r.get('Scratch', 0):>8} {r.get('Occ', 0):>4} {r.get('LDS', 0):>7}")


if __name__ == "__main__":
    main()
