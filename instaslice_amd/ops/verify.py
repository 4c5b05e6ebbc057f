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

Double precision is a matrix path of its own. `run_dgemm` runs
`instaslice-payload dgemm` (the FP64 MFMA GEMM: fp64 operands and
accumulation on `v_mfma_f64_16x16x4_f64`, exact-checked and timed at 4096 x
4096 x 1024 on an integer pattern scaled by 2**-16, whose results span 46
bits) and `judge_dgemm` fails "dgemm" unless the maximum error is exactly
zero: anything that multiplies or accumulates in less than fp64 gets a wrong
answer, not a slightly different one. None of the other probes issues a
double-precision instruction, so a partition can pass all of them and still
fail here. Its TFLOP/s is carried in the report and never judged.

So is the integer one. `run_igemm` runs `instaslice-payload igemm` (the INT8
MFMA GEMM: int8 operands and int32 accumulation on `v_mfma_i32_32x32x32_i8`,
exact-checked and timed at 4096 x 4096 x 4096 on a pattern that covers the
whole int8 range, -128 included) and `judge_igemm` fails "igemm" unless the
maximum error is exactly zero: an integer result is right or wrong, never
close. It is the path a W8A8-quantised model runs on, an instruction family
and accumulator layout none of the other probes issues. Its `tflops` field
counts integer operations (2 M N K per launch, in units of 10**12 per second);
it is carried in the report and never judged.

So has the routed path. `run_moe` runs `instaslice-payload moe` (the
mixture-of-experts grouped GEMM: routing on the device with LDS histograms and
integer atomics, a gathered bf16 MFMA GEMM per expert scheduled from the tile
table the routing wrote, the gate, and the combine over a token's top-k
experts, exact-checked and timed at 8192 tokens x 4096 x 1024 over 32 experts,
top-4) and `judge_moe` fails "moe" unless the maximum error is exactly zero
and `bm`, the tile height the host chose, is 32 or 128. None of the dense
probes takes an index, so a partition can pass all of them and be wrong here.
Its rates are carried in the report and never judged.

So has the serving path. `run_attn` runs `instaslice-payload attn` (KV-cache
decode attention: single-token grouped-query attention at head dim 128, K and
V streamed through the bf16 MFMA with an fp32 online softmax and a split-KV
merge; a self-check, then a timed run over 512 MiB of K and V) and
`judge_attn` fails "attn" unless the exact pattern's maximum error is zero and
the dense pattern's error relative to max |v| is within 2**-8, the bound that
rounding the softmax weights to bf16 allows twice over. KV bytes/s, decode
steps/s and tokens/s are carried in the report and never judged.

So has the cache a serving stack really keeps. `run_paged` runs
`instaslice-payload paged` (the same attention over a pool of fixed-size pages
reached through a block table by scalar loads, with lengths that differ within
the batch and a split into work items that a plan kernel writes on the device
in every launch; a ragged self-check under a scrambled table, then a timed run
over 512 MiB of K and V in 64-key pages) and `judge_paged` fails "paged" unless
the exact pattern's maximum error is zero, the dense pattern's error is within
the same 2**-8, the counts (`items` among them) are integers >= 1 and `page`
is 32, 64, 128 or 256. `attn` addresses a chunk as base + chunk * 8 KiB, so a
partition whose scalar-load-then-vector-load path is wrong passes it and fails
here. Rates are carried in the report and never judged.

So has the cache a serving stack keeps when it wants the bytes halved.
`run_paged8` runs `instaslice-payload paged8` (the paged attention over OCP
e4m3 codes with a scale per kv head, widened to bf16 in registers in front of
the bf16 MFMA; the self-check with NaN codes in everything that must not be
read, then a timed run beside the bf16 kernel) and `judge_paged8` fails
"paged8" on the same terms as `judge_paged`, with `page` 64, 128 or 256.
Nothing else puts 8-bit loads and the fp8 conversion instructions in front of
the matrix cores. `quant_rel`, the error of the format itself, is carried and
never judged.

And so has the step between decode and a cold prompt. `run_extend` runs
`instaslice-payload extend` (chunked prefill: a run of new tokens per sequence
over the paged cache and, causally, each other; the pool's chunk images found
through the block table and staged through LDS for 128 query columns, bound by
the matrix cores) and `judge_extend` fails "extend" on `judge_paged`'s terms
for `max_err`, `max_rel` and `page`, with `new` among the counts.
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


# ---- dgemm ------------------------------------------------------------------

def judge_dgemm(report: dict, profile_name: str) -> dict:
    """Judge an `instaslice-payload dgemm` report: "dgemm" fails unless
    `max_err` is a numeric zero and `m`, `n`, `k`, `iters` are integer counts
    >= 1. `tflops` is carried and never judged. Pure; the report's own `ok`
    is not trusted. ValueError on a profile name that does not parse."""
    return _judge_one(report, profile_name, "dgemm", _mx_fields_clean)


def run_dgemm(profile_name: str, env: Optional[Dict[str, str]] = None,
              runner: Callable = subprocess.run) -> dict:
    """Run `instaslice-payload dgemm` (default shape and iterations) in a
    fresh child with `env` and judge its report, with the same contract as
    `run_mxgemm`: every way the child can fail comes back as `ok: False`
    with a `reason`, and only an unparseable profile name raises
    (ValueError)."""
    parse_profile_name(profile_name)
    return _run_child(profile_name, ["dgemm"], CHILD_TIMEOUT_S, "max_err",
                      lambda report: judge_dgemm(report, profile_name),
                      env, runner)


# ---- igemm ------------------------------------------------------------------

def judge_igemm(report: dict, profile_name: str) -> dict:
    """Judge an `instaslice-payload igemm` report: "igemm" fails unless
    `max_err` is a numeric zero and `m`, `n`, `k`, `iters` are integer counts
    >= 1. `tflops` (integer operations) is carried and never judged. Pure; the
    report's own `ok` is not trusted. ValueError on a profile name that does
    not parse."""
    return _judge_one(report, profile_name, "igemm", _mx_fields_clean)


def run_igemm(profile_name: str, env: Optional[Dict[str, str]] = None,
              runner: Callable = subprocess.run) -> dict:
    """Run `instaslice-payload igemm` (default shape and iterations) in a
    fresh child with `env` and judge its report, with the same contract as
    `run_mxgemm`: every way the child can fail comes back as `ok: False`
    with a `reason`, and only an unparseable profile name raises
    (ValueError)."""
    parse_profile_name(profile_name)
    return _run_child(profile_name, ["igemm"], CHILD_TIMEOUT_S, "max_err",
                      lambda report: judge_igemm(report, profile_name),
                      env, runner)


# ---- moe --------------------------------------------------------------------

def _moe_fields_clean(report: dict) -> bool:
    return _is_zero(report.get("max_err")) \
        and _counts_from_one(report, ("tokens", "n", "k", "experts", "topk",
                                      "iters")) \
        and _is_count(report.get("bm")) and report["bm"] in (32, 128)


def judge_moe(report: dict, profile_name: str) -> dict:
    """Judge an `instaslice-payload moe` report: "moe" fails unless `max_err`
    is a numeric zero, `tokens`, `n`, `k`, `experts`, `topk`, `iters` are
    integer counts >= 1 and `bm` is 32 or 128. `tflops` and `tokens_per_s` are
    carried and never judged. Pure; the report's own `ok` is not trusted.
    ValueError on a profile name that does not parse."""
    return _judge_one(report, profile_name, "moe", _moe_fields_clean)


def run_moe(profile_name: str, env: Optional[Dict[str, str]] = None,
            runner: Callable = subprocess.run) -> dict:
    """Run `instaslice-payload moe` (default shape and iterations) in a fresh
    child with `env` and judge its report, with the same contract as
    `run_igemm`: every way the child can fail comes back as `ok: False` with
    a `reason`, and only an unparseable profile name raises (ValueError)."""
    parse_profile_name(profile_name)
    return _run_child(profile_name, ["moe"], CHILD_TIMEOUT_S, "max_err",
                      lambda report: judge_moe(report, profile_name),
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


# ---- paged ------------------------------------------------------------------

PAGED_PAGES = (32, 64, 128, 256)


def judge_paged(report: dict, profile_name: str) -> dict:
    """Judge an `instaslice-payload paged` report: "paged" fails unless
    `max_err` is a numeric zero, `max_rel` is a real number in [0, 2**-8],
    `batch`, `hq`, `hkv`, `len`, `iters`, `items` are integer counts >= 1 and
    `page` is 32, 64, 128 or 256. `kv_gb_per_s`, `steps_per_s` and `tok_per_s`
    are carried and never judged. Pure; the report's own `ok` is not trusted.
    ValueError on a profile name that does not parse."""
    return _judge_one(report, profile_name, "paged",
                      lambda r: _attn_fields_clean(r, ATTN_MAX_REL)
                      and _counts_from_one(r, ("items",))
                      and _is_count(r.get("page")) and r["page"] in PAGED_PAGES)


def run_paged(profile_name: str, env: Optional[Dict[str, str]] = None,
              runner: Callable = subprocess.run) -> dict:
    """Run `instaslice-payload paged` (default shape, page size and
    iterations) in a fresh child with `env` and judge its report, with the
    same contract as `run_attn`: every way the child can fail comes back as
    `ok: False` with a `reason`, and only an unparseable profile name raises
    (ValueError)."""
    parse_profile_name(profile_name)
    return _run_child(profile_name, ["paged"], CHILD_TIMEOUT_S, "max_err",
                      lambda report: judge_paged(report, profile_name),
                      env, runner)


# ---- paged8 -----------------------------------------------------------------

PAGED8_PAGES = (64, 128, 256)


def judge_paged8(report: dict, profile_name: str) -> dict:
    """Judge an `instaslice-payload paged8` report: "paged8" fails unless
    `max_err` is a numeric zero, `max_rel` is a real number in [0, 2**-8]
    (widening e4m3 to bf16 is exact, so the bound is `judge_paged`'s),
    `batch`, `hq`, `hkv`, `len`, `iters`, `items` are integer counts >= 1 and
    `page` is 64, 128 or 256. `us`, `bf16_us`, `kv_gb_per_s`, `steps_per_s`,
    `tok_per_s` and `quant_rel` (the error of the format itself) are carried
    and never judged. Pure; the report's own `ok` is not trusted. ValueError
    on a profile name that does not parse."""
    return _judge_one(report, profile_name, "paged8",
                      lambda r: _attn_fields_clean(r, ATTN_MAX_REL)
                      and _counts_from_one(r, ("items",))
                      and _is_count(r.get("page")) and r["page"] in PAGED8_PAGES)


def run_paged8(profile_name: str, env: Optional[Dict[str, str]] = None,
               runner: Callable = subprocess.run) -> dict:
    """Run `instaslice-payload paged8` (default shape, page size and
    iterations) in a fresh child with `env` and judge its report, with the
    same contract as `run_paged`: every way the child can fail comes back as
    `ok: False` with a `reason`, and only an unparseable profile name raises
    (ValueError)."""
    parse_profile_name(profile_name)
    return _run_child(profile_name, ["paged8"], CHILD_TIMEOUT_S, "max_err",
                      lambda report: judge_paged8(report, profile_name),
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


# ---- extend -----------------------------------------------------------------

def judge_extend(report: dict, profile_name: str) -> dict:
    """Judge an `instaslice-payload extend` report: "extend" fails unless
    `max_err` is a numeric zero, `max_rel` is a real number in [0, 2**-8] (the
    numerics contract is decode's, see ATTN_MAX_REL), `batch`, `hq`, `hkv`,
    `len`, `new`, `iters`, `items` are integer counts >= 1 and `page` is 32,
    64, 128 or 256. `tflops` and `tok_per_s` are carried and never judged.
    Pure; the report's own `ok` is not trusted. ValueError on a profile name
    that does not parse."""
    return _judge_one(report, profile_name, "extend",
                      lambda r: _attn_fields_clean(r, ATTN_MAX_REL)
                      and _counts_from_one(r, ("new", "items"))
                      and _is_count(r.get("page")) and r["page"] in PAGED_PAGES)


def run_extend(profile_name: str, env: Optional[Dict[str, str]] = None,
               runner: Callable = subprocess.run) -> dict:
    """Run `instaslice-payload extend` (default shape, run of new tokens, page
    size and iterations) in a fresh child with `env` and judge its report,
    with the same contract as `run_paged`: every way the child can fail comes
    back as `ok: False` with a `reason`, and only an unparseable profile name
    raises (ValueError)."""
    parse_profile_name(profile_name)
    return _run_child(profile_name, ["extend"], CHILD_TIMEOUT_S, "max_err",
                      lambda report: judge_extend(report, profile_name),
                      env, runner)
