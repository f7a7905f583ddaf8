"""Sanitizers on the host code of ffmp_dwa / ffmp_dwa_check (the argument checks, the footprint scan, the
byte-range arithmetic of the overlap test), as tests/test_host_sanitize.py does for the rest of the C ABI.

ffmp_dwa.hip is built into a library with AddressSanitizer + UndefinedBehaviorSanitizer on its HOST code only
(`-Xarch_host -fsanitize=...`; GPU code is never sanitized here), beside tests/dwa_sanitize_shim.cc — the two
helpers of ffmp_kernels.hip it calls, so that the step's kernels need not be compiled —, and driven by the
stand-alone C program tests/dwa_sanitize.c, which needs no GPU and launches nothing.  LeakSanitizer runs too.
CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CLANG = "/opt/rocm/llvm/bin/clang"
SRCS = [os.path.join(ROOT, "flow_field_based_motion_planner_amd", "csrc", "ffmp_dwa.hip"), os.path.join(ROOT, "tests", "dwa_sanitize_shim.cc")]


@pytest.mark.skipif(not (shutil.which(HIPCC) and os.path.exists(CLANG)), reason="ROCm toolchain absent")
def test_dwa_host_code_under_asan_ubsan(tmp_path):
    lib = tmp_path / "libffmp_dwa_san.so"
    san = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC",
                    "-shared", "-I" + os.path.join(ROOT, "include")] + san + ["-o", str(lib)] + SRCS,
                   check=True, capture_output=True, cwd=str(tmp_path))
    exe = tmp_path / "dwa_sanitize"
    subprocess.run([CLANG, "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "dwa_sanitize.c"),
                    "-L" + str(tmp_path), "-lffmp_dwa_san", "-lm", "-Wl,-rpath," + str(tmp_path), "-o", str(exe)],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    report = r.stdout + r.stderr
    assert r.returncode == 0, report
    assert "all host-side checks passed" in r.stdout
    assert "AddressSanitizer" not in report and "runtime error" not in report and "LeakSanitizer" not in report
