"""Builds tests/native/partitiond_selftest.cpp (a program with its own main
over smi/csrc/partitiond_metrics.hpp: the counter sample against a scripted
api, and the sample cache on a hand-set clock; no Python, no GPU, nothing
of libamd_smi but its header's types) once with AddressSanitizer + UBSan and
once with ThreadSanitizer, and runs each directly, the way
tests/test_native_selftests.py does for the store's two programs. The
sanitizer runtimes are linked statically into the program."""

import os
import platform
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "partitiond_selftest.cpp"
INC = ROOT / "instaslice_amd" / "smi" / "csrc"
ROCM = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))

VARIANTS = {
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                   "-static-libasan", "-static-libubsan"],
    "tsan": ["-fsanitize=thread", "-static-libtsan"],
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_partitiond_selftest(variant, tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the partitiond selftest"
    exe = tmp_path / f"partitiond_selftest_{variant}"
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Wextra",
         *VARIANTS[variant], f"-I{INC}", f"-I{ROCM / 'include'}", str(SRC),
         "-o", str(exe)],
        capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True,
                         timeout=120)
    if "unexpected memory mapping" in run.stderr and not run.stdout:
        # the sanitizer runtime gave up before main(): it cannot place its
        # shadow memory under this kernel's address-space randomisation.
        # Same program, randomisation off for that one process; if it still
        # cannot start, the assertions below fail with the runtime's message.
        setarch = shutil.which("setarch")
        if setarch:
            run = subprocess.run(
                [setarch, platform.machine(), "-R", str(exe)],
                capture_output=True, text=True, timeout=120)
    report = (run.stdout + run.stderr)[-6000:]
    assert run.returncode == 0, report
    assert "partitiond selftest OK" in run.stdout, report
    # TSan reports and carries on unless told otherwise: no report at all
    assert "ThreadSanitizer" not in run.stderr, report
    assert "runtime error" not in run.stderr, report
