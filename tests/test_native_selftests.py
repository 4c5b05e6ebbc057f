"""Builds the stand-alone self-tests under tests/native/ (each a program with
its own main over a header of store/csrc: netwire_selftest.cpp over
netwire_core.hpp, stored_selftest.cpp over stored_core.hpp; no Python, no
GPU) once with AddressSanitizer + UBSan and once with ThreadSanitizer, and
runs each directly. The sanitizer runtimes are linked statically into the
program, so nothing about the process environment matters to them."""

import platform
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native"
INC = ROOT / "instaslice_amd" / "store" / "csrc"

PROGRAMS = ["netwire", "stored"]

VARIANTS = {
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                   "-static-libasan", "-static-libubsan"],
    "tsan": ["-fsanitize=thread", "-static-libtsan"],
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("program", PROGRAMS)
def test_native_selftest(program, variant, tmp_path):
    cxx = shutil.which("g++")
    assert cxx, f"g++ is needed to build the {program} selftest"
    exe = tmp_path / f"{program}_selftest_{variant}"
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Wextra",
         *VARIANTS[variant], f"-I{INC}", str(SRC / f"{program}_selftest.cpp"),
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
    assert f"{program} selftest OK" in run.stdout, report
    # TSan reports and carries on unless told otherwise: no report at all
    assert "ThreadSanitizer" not in run.stderr, report
    assert "runtime error" not in run.stderr, report
