"""Verify a carved partition against the profile that was requested.

`instaslice-payload verify` runs the first-party probes inside whatever
device set the environment exposes (XCD census, vecadd, the bf16 MFMA GEMM
exact check, the bandwidth probe, a timed GEMM) and prints one JSON report.
This module runs that verb in a fresh child with a pod's environment and
judges the report against a profile name such as `cpx-1x36`:

    from instaslice_amd.ops import verify
    verdict = verify.run("cpx-1x36", env={"ROCR_VISIBLE_DEVICES": uuid})
    verdict["ok"], verdict["failed"]

Judged: vecadd and GEMM exactness (max error 0) and the visible XCD count.
Bandwidth, TFLOP/s, CU count and memory size are carried in the report and
never judged: there are no measured per-partition values to hold them to.

A live verifier holds the device for its run (a second or two), which blocks
partition mode flips for that long: run it after a partition is handed over,
not while the agent is re-carving the GPU.
"""

from __future__ import annotations

import json
import os
import subprocess
from typing import Callable, Dict, Optional

from instaslice_amd.partition.profiles import parse_profile_name

CHILD_TIMEOUT_S = 60.0

BIN_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "bin", "instaslice-payload")


def expected_xcds(profile_name: str) -> int:
    """XCDs a partition of this profile exposes. ValueError on a name that
    does not parse."""
    _mode, xcds, _gb = parse_profile_name(profile_name)
    return xcds


def _is_zero(value) -> bool:
    # a missing or non-numeric error field is a failure, not a pass
    return isinstance(value, (int, float)) and not isinstance(value, bool) \
        and value == 0


def judge(report: dict, profile_name: str) -> dict:
    """Recompute the verdict from the report's fields against the profile.
    Pure; the report's own `ok` / `failed` are not trusted."""
    want = expected_xcds(profile_name)
    failed = []
    if not _is_zero(report.get("vecadd_max_err")):
        failed.append("vecadd")
    if not _is_zero(report.get("gemm_max_err")):
        failed.append("gemm")
    if report.get("xcds_visible") != want:
        failed.append("xcds")
    return {"ok": not failed, "failed": failed, "profile": profile_name,
            "report": report}


def _not_run(profile_name: str, reason: str, report: Optional[dict] = None) -> dict:
    return {"ok": False, "failed": [], "profile": profile_name,
            "reason": reason, "report": report}


def run(profile_name: str, env: Optional[Dict[str, str]] = None,
        runner: Callable = subprocess.run) -> dict:
    """Run `instaslice-payload verify` in a fresh child with `env` (the pod's
    ROCR_VISIBLE_DEVICES and the like, laid over this process's environment)
    and judge its report. Every way the child can fail to produce a report
    comes back as `ok: False` with a `reason`; only an unparseable profile
    name raises (ValueError)."""
    want = expected_xcds(profile_name)
    child_env = dict(os.environ)
    child_env.update({k: str(v) for k, v in (env or {}).items()})
    try:
        proc = runner([BIN_PATH, "verify", str(want)], capture_output=True,
                      text=True, timeout=CHILD_TIMEOUT_S, env=child_env)
    except FileNotFoundError:
        return _not_run(profile_name, f"payload binary not found: {BIN_PATH}")
    except subprocess.TimeoutExpired:
        return _not_run(profile_name,
                        f"verify timed out after {CHILD_TIMEOUT_S:.0f} s")
    except OSError as e:
        return _not_run(profile_name, f"could not start payload binary: {e}")

    lines = [ln for ln in (proc.stdout or "").splitlines() if ln.strip()]
    try:
        report = json.loads(lines[-1]) if lines else None
    except ValueError:
        report = None
    if not isinstance(report, dict):
        tail = (proc.stdout or "").strip()[-200:]
        return _not_run(profile_name,
                        f"non-JSON output (exit {proc.returncode}): {tail!r}")
    if "xcds_visible" not in report:
        # the binary's catch-all error line: {"ok": false, "error": "..."}
        return _not_run(profile_name,
                        f"verify failed (exit {proc.returncode}): "
                        f"{report.get('error', 'no report fields')}", report)
    verdict = judge(report, profile_name)
    if proc.returncode != 0 and verdict["ok"]:
        # the fields look clean but the child says otherwise: believe the exit
        verdict["ok"] = False
        verdict["reason"] = f"payload exited {proc.returncode}"
    elif proc.returncode != 0:
        verdict["reason"] = f"payload exited {proc.returncode}"
    return verdict
