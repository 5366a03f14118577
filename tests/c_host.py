"""The plain-C host program of examples/, built for tests/test_abi.py (no device: fails loudly) and tests/test_gpu_shim.py (solves)."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_c_host(tmp_path):
    """examples/c_abi_solve.c: a plain-C host on include/sddp.h (gcc, no Python, no torch in the process)"""
    import subprocess
    exe = str(tmp_path / "c_abi_solve")
    libdir = os.path.join(ROOT, "srbd_horizon_amd")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_abi_solve.c"),
                    "-o", exe, "-L" + libdir, "-lsddp_hip", "-Wl,-rpath," + libdir, "-lm"], check=True, capture_output=True)
    return exe
