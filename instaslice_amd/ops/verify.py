"""Verify a carved partition against the profile that was requested.

`instaslice-payload verify` runs the first-party probes inside whatever
device set the environment exposes (XCD census, vecadd, the bf16 MFMA GEMM
exact check, the bandwidth probe, a timed GEMM) and prints one JSON report.
This module runs that verb in a fresh child with a pod's environment and
judges the report against a profile name such as `cpx-1x36`:

    from instaslice_amd.ops import verify
    verdict = verify.run("cpx-1x36", env={"ROCR_VISIBLE_DEVICES": uuid})
    verdict["ok"], verdict["failed"]

Judged: vecadd and GEMM exactness (max error 0), the visible XCD count and
the bandwidth probe's copy (`membw_bad_units`, the 16-byte units of its
destination that do not hold the pattern, must be 0: a rate from a copy that
did not copy proves nothing). Bandwidth, TFLOP/s, CU count and memory size are carried in the report and
never judged: there are no measured per-partition values to hold them to.

A live verifier holds the device for its run (a second or two), which blocks
partition mode flips for that long: run it after a partition is handed over,
not while the agent is re-carving the GPU.

Memory has a probe of its own. `run_memcheck` runs `instaslice-payload
memcheck` (a moving-inversions test with an address-derived pattern) over one
buffer sized in GiB or as a fraction of the profile's own memory, and
`judge_memcheck` fails "memory" unless the whole requested size was swept and
no word came back wrong. A partition that cannot allocate the size comes back
`ok: False` with the HIP error as the reason. The chip has a 256 MiB Infinity
Cache: a buffer of that size or less can be served back from cache, so such a
run proves the kernel, not the HBM (the report's `beyond_llc` says which it
was). Operational runs should be well above 256 MiB.

The low-precision matrix path has a probe of its own too. `run_mxgemm` runs
`instaslice-payload mxgemm` (the MXFP8 block-scaled MFMA GEMM: e4m3 operands,
E8M0 scales, exact-checked and timed at 4096 x 4096 x 2048) and `judge_mxgemm`
fails "mxgemm" unless the maximum error is exactly zero. It exercises a
different instruction and datapath than the bf16 GEMM that `verify` runs, so a
partition can pass one and fail the other. Its TFLOP/s is carried in the
report and never judged.

The 4-bit matrix path has one as well. `run_mx4gemm` runs `instaslice-payload
mx4gemm` (the MXFP4 block-scaled MFMA GEMM: e2m1 operands packed two to a
byte, E8M0 scales, the same pattern, shape and checks as `mxgemm`) and
`judge_mx4gemm` fails "mx4gemm" unless the maximum error is exactly zero. It is
the same instruction with other format selectors and half the operand
registers, at twice the MXFP8 rate per clock, so a partition can pass `mxgemm`
and still be wrong or slow here. Its TFLOP/s is carried in the report and
never judged.

So has the serving path. `run_attn` runs `instaslice-payload attn` (KV-cache
decode attention: single-token grouped-query attention at head dim 128, K and
V streamed through the bf16 MFMA with an fp32 online softmax and a split-KV
merge; a self-check, then a timed run over 512 MiB of K and V) and
`judge_attn` fails "attn" unless the exact pattern's maximum error is zero and
the dense pattern's error relative to max |v| is within 2**-8, the bound that
rounding the softmax weights to bf16 allows twice over. KV bytes/s, decode
steps/s and tokens/s are carried in the report and never judged.
"""

from __future__ import annotations

import json
import os
import subprocess
import math
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
    if not _is_zero(report.get("membw_bad_units")):
        failed.append("membw")
    return _verdict(report, profile_name, failed)


def _verdict(report: dict, profile_name: str, failed: list) -> dict:
    return {"ok": not failed, "failed": failed, "profile": profile_name,
            "report": report}


def _judge_one(report: dict, profile_name: str, name: str,
               clean: Callable[[dict], bool]) -> dict:
    # a probe with one judged item: `name` fails unless `clean(report)`
    parse_profile_name(profile_name)
    return _verdict(report, profile_name, [] if clean(report) else [name])


def _is_count(value) -> bool:
    return isinstance(value, int) and not isinstance(value, bool)


def _counts_from_one(report: dict, keys) -> bool:
    return all(_is_count(report.get(key)) and report[key] >= 1 for key in keys)


def _not_run(profile_name: str, reason: str, report: Optional[dict] = None) -> dict:
    return {"ok": False, "failed": [], "profile": profile_name,
            "reason": reason, "report": report}


def _run_child(profile_name: str, argv_tail: list, timeout_s: float, marker: str,
               judge_report: Callable, env: Optional[Dict[str, str]],
               runner: Callable) -> dict:
    """Run `instaslice-payload` with `argv_tail` (the verb first) in a fresh
    child with `env` laid over this process's environment, and judge the last
    JSON line of its output with `judge_report(report)`. `marker` is the field
    that tells a real report from the binary's catch-all error line. Every way
    the child can fail to produce a report comes back as `ok: False` with a
    `reason`."""
    verb = argv_tail[0]
    child_env = dict(os.environ)
    child_env.update({k: str(v) for k, v in (env or {}).items()})
    try:
        proc = runner([BIN_PATH, *argv_tail], capture_output=True, text=True,
                      timeout=timeout_s, env=child_env)
    except FileNotFoundError:
        return _not_run(profile_name, f"payload binary not found: {BIN_PATH}")
    except subprocess.TimeoutExpired:
        return _not_run(profile_name,
                        f"{verb} timed out after {timeout_s:.0f} s")
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
    if marker not in report:
        # the binary's catch-all error line: {"ok": false, "error": "..."}
        return _not_run(profile_name,
                        f"{verb} failed (exit {proc.returncode}): "
                        f"{report.get('error', 'no report fields')}", report)
    verdict = judge_report(report)
    if proc.returncode != 0:
        # clean-looking fields do not outvote a non-zero exit
        verdict["ok"] = False
        verdict["reason"] = f"payload exited {proc.returncode}"
    return verdict


def run(profile_name: str, env: Optional[Dict[str, str]] = None,
        runner: Callable = subprocess.run) -> dict:
    """Run `instaslice-payload verify` in a fresh child with `env` (the pod's
    ROCR_VISIBLE_DEVICES and the like, laid over this process's environment)
    and judge its report. Every way the child can fail to produce a report
    comes back as `ok: False` with a `reason`; only an unparseable profile
    name raises (ValueError)."""
    want = expected_xcds(profile_name)
    return _run_child(profile_name, ["verify", str(want)], CHILD_TIMEOUT_S,
                      "xcds_visible", lambda report: judge(report, profile_name),
                      env, runner)


# ---- memcheck ---------------------------------------------------------------

GIB = 1 << 30  # a profile's "GB" is 2^30 bytes, as in the report's total_mem_gb

# One child: hipMalloc of the buffer, four traversals per pass, exit.
# Measured once on an MI355X in SPX (profiles/memcheck_probe.md): 128 GiB, one
# pass, 3.58 s wall for the whole child, of which 0.086 s between upload and
# result; the rest is process start, hipMalloc and teardown (32 GiB: 1.39 s,
# 2 GiB: 0.4 s). Scaled linearly, 0.9 of spx-8x288 is about 7.5 s and a further
# pass about 0.2 s, so 120 s leaves more than a tenfold margin.
MEMCHECK_TIMEOUT_S = 120.0


def judge_memcheck(report: dict, profile_name: str, want_bytes: int) -> dict:
    """Judge an `instaslice-payload memcheck` report: "memory" fails unless
    the whole of `want_bytes` (rounded down to 16) was swept at least once and
    no word came back wrong. Pure; the report's own `ok` is not trusted.
    ValueError on a profile name that does not parse."""
    def clean(report):
        return (_is_zero(report.get("bad_words"))
                and _is_count(report.get("first_bad_offset"))
                and report["first_bad_offset"] == -1
                and _is_count(report.get("bytes"))
                and report["bytes"] == int(want_bytes) // 16 * 16
                and _counts_from_one(report, ("passes",)))
    return _judge_one(report, profile_name, "memory", clean)


def memcheck_bytes(profile_name: str, gb: Optional[float] = None,
                   fraction: Optional[float] = None) -> int:
    """Buffer size for a memcheck of this profile: `gb` GiB, or `fraction` of
    the profile's own memory, rounded down to 16 bytes; 1 GiB when neither is
    given. ValueError on both, on a non-positive size and on a bad name."""
    _mode, _xcds, profile_gb = parse_profile_name(profile_name)
    if gb is not None and fraction is not None:
        raise ValueError("give at most one of gb and fraction")
    if fraction is not None:
        if not 0 < fraction <= 1:
            raise ValueError(f"fraction must be in (0, 1], got {fraction!r}")
        size = fraction * profile_gb * GIB
    else:
        size = (1 if gb is None else gb) * GIB
    nbytes = int(size) // 16 * 16
    if nbytes < 16:
        raise ValueError("memcheck size must be at least 16 bytes")
    return nbytes


def run_memcheck(profile_name: str, env: Optional[Dict[str, str]] = None,
                 gb: Optional[float] = None, fraction: Optional[float] = None,
                 passes: int = 1, runner: Callable = subprocess.run) -> dict:
    """Run `instaslice-payload memcheck` in a fresh child with `env` and judge
    its report, with the same contract as `run`. The buffer is `gb` GiB or
    `fraction` of the profile's own memory (fraction=0.9 on cpx-1x36 demands
    that 32.4 GiB be allocatable and hold data); default 1 GiB. A child that
    cannot allocate comes back `ok: False` with the HIP error in `reason`.
    ValueError on a bad profile name, on both gb and fraction, and on
    passes < 1."""
    want_bytes = memcheck_bytes(profile_name, gb=gb, fraction=fraction)
    if not _is_count(passes) or passes < 1:
        raise ValueError(f"passes must be an integer >= 1, got {passes!r}")
    return _run_child(profile_name, ["memcheck", str(want_bytes), str(passes)],
                      MEMCHECK_TIMEOUT_S, "bad_words",
                      lambda report: judge_memcheck(report, profile_name,
                                                    want_bytes),
                      env, runner)


# ---- mxgemm -----------------------------------------------------------------

def _mx_fields_clean(report: dict) -> bool:
    return _is_zero(report.get("max_err")) \
        and _counts_from_one(report, ("m", "n", "k", "iters"))


def judge_mxgemm(report: dict, profile_name: str) -> dict:
    """Judge an `instaslice-payload mxgemm` report: "mxgemm" fails unless
    `max_err` is a numeric zero and `m`, `n`, `k`, `iters` are integer counts
    >= 1. `tflops` is carried and never judged. Pure; the report's own `ok`
    is not trusted. ValueError on a profile name that does not parse."""
    return _judge_one(report, profile_name, "mxgemm", _mx_fields_clean)


def run_mxgemm(profile_name: str, env: Optional[Dict[str, str]] = None,
               runner: Callable = subprocess.run) -> dict:
    """Run `instaslice-payload mxgemm` (default shape and iterations) in a
    fresh child with `env` and judge its report, with the same contract as
    `run_memcheck`: every way the child can fail comes back as `ok: False`
    with a `reason`, and only an unparseable profile name raises
    (ValueError)."""
    parse_profile_name(profile_name)
    return _run_child(profile_name, ["mxgemm"], CHILD_TIMEOUT_S, "max_err",
                      lambda report: judge_mxgemm(report, profile_name),
                      env, runner)


# ---- mx4gemm ----------------------------------------------------------------

def judge_mx4gemm(report: dict, profile_name: str) -> dict:
    """Judge an `instaslice-payload mx4gemm` report: "mx4gemm" fails unless
    `max_err` is a numeric zero and `m`, `n`, `k`, `iters` are integer counts
    >= 1. `tflops` is carried and never judged. Pure; the report's own `ok`
    is not trusted. ValueError on a profile name that does not parse."""
    return _judge_one(report, profile_name, "mx4gemm", _mx_fields_clean)


def run_mx4gemm(profile_name: str, env: Optional[Dict[str, str]] = None,
                runner: Callable = subprocess.run) -> dict:
    """Run `instaslice-payload mx4gemm` (default shape and iterations) in a
    fresh child with `env` and judge its report, with the same contract as
    `run_mxgemm`: every way the child can fail comes back as `ok: False`
    with a `reason`, and only an unparseable profile name raises
    (ValueError)."""
    parse_profile_name(profile_name)
    return _run_child(profile_name, ["mx4gemm"], CHILD_TIMEOUT_S, "max_err",
                      lambda report: judge_mx4gemm(report, profile_name),
                      env, runner)


# ---- attn -------------------------------------------------------------------

# max |o - fp64 reference| / max |v| of the dense pattern: each weight rounded
# to bf16 is off by at most 2**-9 relative while the normaliser is summed from
# the unrounded weights, so the output is off by at most 2**-9 max |v| plus
# fp32 terms of order 1e-6; the bound doubles that
ATTN_MAX_REL = 2.0 ** -8


def _is_real(value) -> bool:
    return isinstance(value, (int, float)) and not isinstance(value, bool) \
        and math.isfinite(value)


def _attn_fields_clean(report: dict, max_rel: float) -> bool:
    return (_is_zero(report.get("max_err"))
            and _is_real(report.get("max_rel"))
            and 0 <= report["max_rel"] <= max_rel
            and _counts_from_one(report, ("batch", "hq", "hkv", "len", "iters")))


def judge_attn(report: dict, profile_name: str) -> dict:
    """Judge an `instaslice-payload attn` report: "attn" fails unless
    `max_err` is a numeric zero, `max_rel` is a real number in [0, 2**-8] and
    `batch`, `hq`, `hkv`, `len`, `iters` are integer counts >= 1.
    `kv_gb_per_s`, `steps_per_s` and `tok_per_s` are carried and never judged.
    Pure; the report's own `ok` is not trusted. ValueError on a profile name
    that does not parse."""
    return _judge_one(report, profile_name, "attn",
                      lambda r: _attn_fields_clean(r, ATTN_MAX_REL))


def run_attn(profile_name: str, env: Optional[Dict[str, str]] = None,
             runner: Callable = subprocess.run) -> dict:
    """Run `instaslice-payload attn` (default shape and iterations) in a fresh
    child with `env` and judge its report, with the same contract as
    `run_mxgemm`: every way the child can fail comes back as `ok: False` with
    a `reason`, and only an unparseable profile name raises (ValueError)."""
    parse_profile_name(profile_name)
    return _run_child(profile_name, ["attn"], CHILD_TIMEOUT_S, "max_err",
                      lambda report: judge_attn(report, profile_name),
                      env, runner)


# ---- prefill ----------------------------------------------------------------

# the numerics contract is decode's (bf16 weights, the normaliser summed from
# the unrounded weights, one true division), so its bound carries over with
# the derivation above ATTN_MAX_REL
PREFILL_MAX_REL = ATTN_MAX_REL


def judge_prefill(report: dict, profile_name: str) -> dict:
    """Judge an `instaslice-payload prefill` report: "prefill" fails unless
    `max_err` is a numeric zero, `max_rel` is a real number in [0, 2**-8],
    `batch`, `hq`, `hkv`, `len`, `iters` are integer counts >= 1 and `causal`
    is a bool. `tflops` and `tok_per_s` are carried and never judged. Pure; the
    report's own `ok` is not trusted. ValueError on a profile name that does
    not parse."""
    return _judge_one(report, profile_name, "prefill",
                      lambda r: _attn_fields_clean(r, PREFILL_MAX_REL)
                      and isinstance(r.get("causal"), bool))


def run_prefill(profile_name: str, env: Optional[Dict[str, str]] = None,
                runner: Callable = subprocess.run) -> dict:
    """Run `instaslice-payload prefill` (default shape and iterations, causal)
    in a fresh child with `env` and judge its report, with the same contract
    as `run_attn`: every way the child can fail comes back as `ok: False` with
    a `reason`, and only an unparseable profile name raises (ValueError)."""
    parse_profile_name(profile_name)
    return _run_child(profile_name, ["prefill"], CHILD_TIMEOUT_S, "max_err",
                      lambda report: judge_prefill(report, profile_name),
                      env, runner)
