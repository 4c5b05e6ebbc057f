"""The four oldest payloads (ops/csrc/payload_core.hpp): vecadd, the streaming
copy of the bandwidth probe, busy and the XCD census. Argument checks and
`grid_for` on CPU; the kernels, their self-checks and the binary's verbs on a
real MI355X.

The references are numpy, written here and independent of the header. A lone
IEEE addition is correctly rounded and cannot be contracted into anything
else, and the kernels' code object keeps fp32 subnormals, so vecadd is
compared bit for bit (NaN for NaN); a copy is compared bit for bit as words.
"""

import functools
import json
import math
import os
import subprocess
import time

import numpy as np
import pytest

BIN = os.path.join(os.path.dirname(__file__), "..", "instaslice_amd", "bin",
                   "instaslice-payload")


@pytest.fixture(scope="module")
def payload():
    from instaslice_amd.ops import _payload

    return _payload


def bits(values):
    return np.array(values, dtype=np.uint32).view(np.float32)


# ---- CPU: grid_for --------------------------------------------------------

@pytest.mark.parametrize("n4,want", [
    (0, 1),                   # never an empty grid
    (1, 1),
    (256, 1),                 # one full block
    (257, 2),
    (65535 * 256, 65535),     # the last size below the cap
    (65535 * 256 + 1, 65535),  # the cap: from here on the kernels stride
    (1 << 40, 65535),
])
def test_grid_for(payload, n4, want):
    assert payload.grid_for(n4) == want


# ---- CPU: argument errors come before any HIP call ------------------------
#
# ValueError specifically: on a machine without a GPU an argument that gets as
# far as the first HIP call raises RuntimeError ("HIP error: ...") instead, and
# that is how these tests tell "validated" from "failed later".

@pytest.mark.parametrize("ms", [math.nan, math.inf, -math.inf, -1.0, -1e-9,
                                60000.001, 1e30])
def test_run_busy_rejects_bad_ms(payload, ms):
    with pytest.raises(ValueError, match="run_busy"):
        payload.run_busy(ms)
    with pytest.raises(ValueError, match="run_busy"):
        payload.run_busy(ms, max_iters=10)


def test_run_vecadd_rejects_zero(payload):
    with pytest.raises(ValueError, match="run_vecadd"):
        payload.run_vecadd(0)


@pytest.mark.parametrize("kw", [
    dict(bytes=1024, iters=0),
    dict(bytes=1024, iters=-3),
    dict(bytes=15, iters=1),
    dict(bytes=0, iters=1),
    dict(bytes=1024, iters=1, blocks=-1),
    dict(bytes=1024, iters=1, blocks=65536),
])
def test_run_membw_rejects_bad_arguments(payload, kw):
    with pytest.raises(ValueError, match="run_membw"):
        payload.run_membw_check(**kw)
    if "blocks" not in kw:  # run_membw has no blocks argument
        with pytest.raises(ValueError, match="run_membw"):
            payload.run_membw(**kw)


@pytest.mark.parametrize("blocks", [0, -1, (1 << 20) + 1])
def test_run_xcd_census_rejects_bad_blocks(payload, blocks):
    with pytest.raises(ValueError, match="run_xcd_census"):
        payload.run_xcd_census(blocks=blocks)


def test_vecadd_rejects_bad_arguments(payload):
    f = np.zeros
    with pytest.raises(ValueError, match="vecadd"):  # 2-D
        payload.vecadd(f((2, 4), np.float32), f((2, 4), np.float32))
    with pytest.raises(ValueError, match="vecadd"):  # 0-D
        payload.vecadd(np.float32(1.0), np.float32(2.0))
    with pytest.raises(ValueError, match="vecadd"):  # lengths differ
        payload.vecadd(f(4, np.float32), f(5, np.float32))
    with pytest.raises(ValueError, match="vecadd"):  # empty
        payload.vecadd(f(0, np.float32), f(0, np.float32))
    for blocks in (-1, 65536):
        with pytest.raises(ValueError, match="vecadd"):
            payload.vecadd(f(4, np.float32), f(4, np.float32), blocks=blocks)
    with pytest.raises((TypeError, ValueError)):
        payload.vecadd("not an array", f(4, np.float32))


def test_stream_copy_rejects_bad_arguments(payload):
    f = np.zeros
    with pytest.raises(ValueError, match="stream_copy"):  # 2-D
        payload.stream_copy(f((2, 4), np.uint32))
    with pytest.raises(ValueError, match="stream_copy"):  # empty
        payload.stream_copy(f(0, np.uint32))
    for blocks in (-1, 65536):
        with pytest.raises(ValueError, match="stream_copy"):
            payload.stream_copy(f(4, np.uint32), blocks=blocks)
        with pytest.raises(ValueError, match="stream_copy"):
            payload.stream_copy(f(4, np.uint32), nontemporal=True, blocks=blocks)
    with pytest.raises((TypeError, ValueError)):
        payload.stream_copy("not an array")


# the binary: one error line that names the function, and no HIP call made
BAD_VERBS = [
    (("busy", "nan"), "run_busy"),
    (("busy", "-1"), "run_busy"),
    (("busy", "1e30"), "run_busy"),
    (("vecadd", "0"), "run_vecadd"),
    (("vecadd", "abc"), "run_vecadd"),
    (("membw", "1024", "0"), "run_membw"),
]


@pytest.mark.parametrize("args,who", BAD_VERBS)
def test_binary_rejects_bad_arguments(args, who):
    out = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1, out.stdout + out.stderr
    res = json.loads(out.stdout)
    assert set(res) == {"ok", "error"} and res["ok"] is False
    assert who in res["error"] and "HIP error" not in res["error"]


def test_serve_rejects_bad_arguments():
    # serve has no membw verb: the other rejections, then proof that the
    # worker is still answering
    asks = [(" ".join(args), who) for args, who in BAD_VERBS if args[0] != "membw"]
    w = subprocess.Popen([BIN, "serve"], stdin=subprocess.PIPE,
                         stdout=subprocess.PIPE, text=True, bufsize=1)
    try:
        out, _ = w.communicate("".join(a + "\n" for a, _ in asks) + "ping\nquit\n",
                               timeout=60)
    finally:
        if w.poll() is None:
            w.kill()
    lines = [json.loads(ln) for ln in out.splitlines()]
    assert len(lines) == len(asks) + 2
    for (ask, who), res in zip(asks, lines):
        assert set(res) == {"ok", "error"} and res["ok"] is False, ask
        assert who in res["error"] and "HIP error" not in res["error"], ask
    assert lines[-2] == {"ok": True, "cmd": "ping"}
    assert lines[-1] == {"ok": True}


# ---- GPU: vecadd against numpy --------------------------------------------

# lengths in floats: around one float4, around one block of float4s' worth of
# floats, and a last one that with blocks=3 gives every thread several strides
# and a ragged last one (1553 float4s over 768 threads) plus a padded tail
LENGTHS = [1, 3, 4, 5, 1023, 1024, 1025, 4 * (256 * 3 * 2 + 17) + 2]
BLOCKS = [0, 1, 3]


def finite(words):
    """uint32 patterns with inf and NaN mapped to finite values."""
    words = words.copy()
    words[(words & 0x7F800000) == 0x7F800000] &= np.uint32(0xBFFFFFFF)
    return words


@functools.lru_cache(maxsize=None)
def vecadd_case(n):
    """(a, b, a + b in float32) for n floats: random bit patterns filtered to
    finite values, so every magnitude from subnormal to 2^127 occurs. Half of
    b is drawn the same way (exponents far apart: the sum is the larger
    operand, or overflows); the other half has its exponent within 3 of a's
    and a random sign and mantissa, so that the add rounds, cancels and
    carries."""
    rng = np.random.default_rng(7000 + n)
    wa = finite(rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32))
    wb = finite(rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32))
    exp = (wa >> 23).astype(np.int64) & 0xFF
    near = np.clip(exp + rng.integers(-3, 4, size=n), 0, 254).astype(np.uint32)
    wb_near = (wb & np.uint32(0x807FFFFF)) | (near << 23)
    wb = np.where(np.arange(n) % 2 == 0, wb, wb_near).astype(np.uint32)
    a, b = wa.view(np.float32), wb.view(np.float32)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    with np.errstate(over="ignore", invalid="ignore"):
        ref = a + b
    assert ref.dtype == np.float32
    for arr in (a, b, ref):
        arr.setflags(write=False)
    return a, b, ref


def assert_same_floats(got, ref):
    """Tolerance 0: bit for bit where the reference is not NaN, NaN for NaN."""
    assert got.dtype == np.float32 and got.shape == ref.shape
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    gw, rw = got.view(np.uint32), ref.view(np.uint32)
    wrong = np.flatnonzero((gw != rw) & ~nan)
    assert wrong.size == 0, (
        f"{wrong.size} of {ref.size} differ, first at {wrong[0]}: "
        f"got 0x{gw[wrong[0]]:08x}, want 0x{rw[wrong[0]]:08x}")


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("n", LENGTHS)
def test_vecadd_matches_numpy(payload, n, blocks):
    a, b, ref = vecadd_case(n)
    c, guard_changed = payload.vecadd(a, b, blocks=blocks)
    assert_same_floats(c, ref)
    assert guard_changed == 0


# (a, b, a + b) as bit patterns, worked out by hand
EDGES = [
    (0x00000000, 0x00000000, 0x00000000),  # +0 + +0 = +0
    (0x00000000, 0x80000000, 0x00000000),  # +0 + -0 = +0
    (0x80000000, 0x00000000, 0x00000000),  # -0 + +0 = +0
    (0x80000000, 0x80000000, 0x80000000),  # -0 + -0 = -0
    (0x7F800000, 0xFF800000, None),        # inf + -inf = NaN
    (0x7F800000, 0x3F800000, 0x7F800000),  # inf + 1 = inf
    (0xFF800000, 0x7F7FFFFF, 0xFF800000),  # -inf + max = -inf
    (0x7FC00000, 0x3F800000, None),        # NaN + 1 = NaN
    (0x7F7FFFFF, 0x7F7FFFFF, 0x7F800000),  # max + max overflows to inf
    (0x7F7FFFFF, 0x73000000, 0x7F800000),  # max + half an ulp: the tie goes to inf
    (0x7F7FFFFF, 0x72FFFFFF, 0x7F7FFFFF),  # max + just under half an ulp stays
    (0xFF7FFFFF, 0xFF7FFFFF, 0xFF800000),  # and to -inf
    (0x3FC00000, 0xBFC00000, 0x00000000),  # 1.5 - 1.5 = +0, exact cancellation
    (0x4B7FFFFF, 0xCB7FFFFE, 0x3F800000),  # 16777215 - 16777214 = 1
    (0x3F800000, 0x33800000, 0x3F800000),  # 1 + 2^-24: tie to even, down
    (0x3F800001, 0x33800000, 0x3F800002),  # (1 + 2^-23) + 2^-24: tie to even, up
    (0x00000001, 0x00000001, 0x00000002),  # subnormal + subnormal
    (0x00000003, 0x80000001, 0x00000002),  # subnormal - subnormal
    (0x007FFFFF, 0x00000001, 0x00800000),  # subnormals that sum to the first normal
    (0x00000001, 0x80000001, 0x00000000),  # subnormal cancellation = +0
    (0x00800000, 0x80000001, 0x007FFFFF),  # normal - subnormal = subnormal
    (0x00800000, 0x00000001, 0x00800001),  # normal + subnormal
    (0x3F800000, 0x00000001, 0x3F800000),  # 1 + the least subnormal = 1
    (0x80000001, 0x00800001, 0x00800000),  # subnormal + normal, signs mixed
    (0x00000001, 0x7F7FFFFF, 0x7F7FFFFF),  # the least and the greatest
]


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [0, 1])
def test_vecadd_edge_table(payload, blocks):
    a = bits([e[0] for e in EDGES])
    b = bits([e[1] for e in EDGES])
    with np.errstate(over="ignore", invalid="ignore"):
        ref = a + b
    # the reference itself: numpy on this host agrees with the hand-written
    # column (it would not if the host flushed subnormals)
    for (wa, wb, want), r in zip(EDGES, ref.view(np.uint32)):
        if want is None:
            assert np.isnan(np.uint32(r).view(np.float32)), (hex(wa), hex(wb))
        else:
            assert r == want, (hex(wa), hex(wb), hex(r))
    c, guard_changed = payload.vecadd(a, b, blocks=blocks)
    assert_same_floats(c, ref)
    assert guard_changed == 0


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
def test_vecadd_pins_element_and_operand_order(payload, blocks):
    """a is a permutation of 0 .. n-1 and b is n times another permutation:
    all exact (n^2 < 2^24), and since a alone already differs everywhere, no
    two elements have the same sum. A swap of lanes inside a float4 or an
    element read from the wrong index gives a wrong value wherever it acts, and
    one operand read twice (a + a, b + b) is wrong at all but one element."""
    n = 4 * (256 * 3 + 5) + 3  # 3095: blocks=3 strides, and a padded tail
    i = np.arange(n, dtype=np.int64)
    p = (i * 1237) % n
    q = (i * 2221 + 17) % n
    assert len(np.unique(p)) == n and len(np.unique(q)) == n
    assert n * n < 1 << 24
    a = p.astype(np.float32)
    b = (n * q).astype(np.float32)
    ref = (p + n * q).astype(np.float32)
    assert np.array_equal(ref.astype(np.int64), p + n * q)
    assert len(np.unique(ref)) == n
    # one operand read twice matches at most where p == n q, that is p = q = 0
    assert np.count_nonzero(a + a == ref) <= 1 and np.count_nonzero(b + b == ref) <= 1
    c, guard_changed = payload.vecadd(a, b, blocks=blocks)
    assert np.array_equal(c, ref)
    assert np.array_equal(c, a + b)
    assert guard_changed == 0


@pytest.mark.gpu
def test_vecadd_converts_strided_and_f64_input(payload):
    a = np.arange(40, dtype=np.float64)[::2]  # f64, strided
    b = np.arange(20, dtype=np.float32) * 3
    c, guard_changed = payload.vecadd(a, b)
    assert np.array_equal(c, np.arange(20, dtype=np.float32) * 5)
    assert guard_changed == 0


# ---- GPU: the streaming copies --------------------------------------------

@functools.lru_cache(maxsize=None)
def copy_case(n):
    """n uniformly random words: NaN, inf and subnormal patterns included."""
    x = np.random.default_rng(9000 + n).integers(
        0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    x.setflags(write=False)
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("nontemporal", [False, True])
@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("n", LENGTHS)
def test_stream_copy_is_identical(payload, n, blocks, nontemporal):
    x = copy_case(n)
    y, guard_changed = payload.stream_copy(x, nontemporal=nontemporal, blocks=blocks)
    assert y.dtype == np.uint32 and y.shape == x.shape
    wrong = np.flatnonzero(y != x)
    assert wrong.size == 0, f"{wrong.size} of {n} words differ, first at {wrong[0]}"
    assert guard_changed == 0


@pytest.mark.gpu
@pytest.mark.parametrize("nontemporal", [False, True])
def test_stream_copy_keeps_nan_payloads(payload, nontemporal):
    x = np.array([0x7F800001, 0x7FC00000, 0xFFFFFFFF, 0x7FA5A5A5, 0xFF800001,
                  0x00000001, 0x80000000, 0x7F800000, 0xA5A5A5A5],
                 dtype=np.uint32)
    y, guard_changed = payload.stream_copy(x, nontemporal=nontemporal)
    assert np.array_equal(y, x)
    assert guard_changed == 0


# ---- GPU: the self-checks -------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 1025, 1 << 20])
def test_run_vecadd_is_exact(payload, n):
    assert payload.run_vecadd(n) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("nontemporal", [False, True])
@pytest.mark.parametrize("blocks", [0, 2])
def test_run_membw_check_is_clean(payload, blocks, nontemporal):
    # 1 MiB + 16 B: 65537 units, one past a multiple of every power of two
    r = payload.run_membw_check((1 << 20) + 16, 2, blocks=blocks,
                                nontemporal=nontemporal)
    assert set(r) == {"gb_per_s", "bad_units"}
    assert r["bad_units"] == 0
    assert math.isfinite(r["gb_per_s"]) and r["gb_per_s"] > 0


@pytest.mark.gpu
def test_run_membw_still_returns_the_rate(payload):
    gbs = payload.run_membw((1 << 20) + 16, 2)
    assert isinstance(gbs, float) and math.isfinite(gbs) and gbs > 0


# ---- GPU: the binary ------------------------------------------------------

def run_bin(*args):
    out = subprocess.run([BIN, *args], capture_output=True, text=True,
                         timeout=120)
    return out.returncode, json.loads(out.stdout), out


@pytest.mark.gpu
def test_binary_membw_prints_bad_units():
    rc, res, out = run_bin("membw", "1048592", "2", "3", "1")
    assert rc == 0, out.stdout + out.stderr
    assert set(res) == {"ok", "cmd", "bytes", "iters", "blocks", "nontemporal",
                        "gb_per_s", "bad_units"}
    assert res["ok"] is True and res["cmd"] == "membw"
    assert (res["bytes"], res["iters"], res["blocks"]) == (1048592, 2, 3)
    assert res["nontemporal"] is True and res["bad_units"] == 0


@pytest.mark.gpu
def test_binary_verify_prints_membw_bad_units():
    rc, res, out = run_bin("verify")
    assert rc == 0, out.stdout + out.stderr
    assert res["membw_bad_units"] == 0 and res["vecadd_max_err"] == 0
    assert res["failed"] == [] and res["gb_per_s"] > 0
    assert isinstance(res["membw_bad_units"], int)


@pytest.mark.gpu
def test_binary_vecadd_and_busy_keys():
    rc, res, out = run_bin("vecadd", "1025")
    assert rc == 0, out.stdout + out.stderr
    assert res == {"ok": True, "cmd": "vecadd", "n": 1025, "max_err": 0}
    rc, res, out = run_bin("busy", "5")
    assert rc == 0, out.stdout + out.stderr
    assert set(res) == {"ok", "cmd", "ms", "elapsed_ms", "iters", "guard_hit"}
    assert res["ok"] is True and res["ms"] == 5.0 and res["guard_hit"] is False
    assert res["elapsed_ms"] >= 5.0 and res["iters"] >= 1


# ---- GPU: census ----------------------------------------------------------

@pytest.fixture(scope="module")
def census(payload):
    return {blocks: payload.run_xcd_census(blocks=blocks)
            for blocks in (1, 7, 4096)}


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [1, 7, 4096])
def test_census_counts_every_workgroup_once(census, blocks):
    counts = census[blocks]
    print(f"\ncensus at {blocks} blocks: {counts}")
    assert len(counts) == 8
    assert sum(counts) == blocks
    assert sum(1 for c in counts if c) >= 1


@pytest.mark.gpu
def test_census_small_grids_stay_inside_the_partition(payload, census):
    nonzero = {b: {x for x, c in enumerate(census[b]) if c} for b in census}
    assert len(nonzero[1]) == 1
    assert nonzero[7] <= nonzero[4096]
    assert nonzero[1] <= nonzero[4096]
    assert payload.device_info()["xcd_count_visible"] == len(nonzero[4096])


# ---- GPU: busy ------------------------------------------------------------

@pytest.mark.gpu
def test_busy_spins_for_the_time_asked(payload):
    t0 = time.monotonic()
    r = payload.run_busy(50.0)
    host_ms = (time.monotonic() - t0) * 1000
    print(f"\nbusy(50): device {r['elapsed_ms']:.4f} ms "
          f"(overshoot {r['elapsed_ms'] - 50.0:.4f} ms), {r['iters']} trips, "
          f"host {host_ms:.1f} ms")
    assert set(r) == {"elapsed_ms", "iters", "guard_hit"}
    assert r["guard_hit"] is False
    # the loop's own exit condition, so exact
    assert r["elapsed_ms"] >= 50.0
    assert r["iters"] >= 1
    # the host waited for the kernel; no upper bound, the machine is shared
    assert host_ms >= 50.0


@pytest.mark.gpu
def test_busy_zero_returns_at_once(payload):
    r = payload.run_busy(0.0)
    assert r["guard_hit"] is False and r["iters"] == 0


@pytest.mark.gpu
def test_busy_iteration_guard_ends_the_spin(payload):
    # 1000 trips of a clock read and an add are over long before 2 s: a
    # broken guard costs 2 s, not a hang
    r = payload.run_busy(2000.0, max_iters=1000)
    print(f"\nbusy(2000, max_iters=1000): device {r['elapsed_ms']:.4f} ms")
    assert r["guard_hit"] is True
    assert r["iters"] == 1000
    assert r["elapsed_ms"] < 2000.0
