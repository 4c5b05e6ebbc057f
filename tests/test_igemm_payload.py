"""The INT8 MFMA GEMM payload (ops/csrc/payload_igemm.hpp): argument checks,
the quantiser and the judge on CPU; the kernel's two epilogues, its bindings,
the binary's `igemm` verb and `verify.run_igemm` on a real MI355X.

Every GPU check is exact. An int8 product is at most 2^14 in magnitude, so a
sum of K <= 131071 of them fits int32 (131071 * 2^14 < 2^31) and the int64
reference. The W8A8 reference is the same three fp32 operations in the same
order: an int32 -> float32 conversion (round-to-nearest-even in numpy and on
the device) and two float32 products; with |acc| >= 1 or acc == 0 and scales
in [2^-10, 1] every result is zero or normal.
"""

import json
import os
import subprocess

import numpy as np
import pytest

from instaslice_amd.ops import verify

BIN = os.path.join(os.path.dirname(__file__), "..", "instaslice_amd", "bin",
                   "instaslice-payload")


@pytest.fixture(scope="module")
def payload():
    from instaslice_amd.ops import _payload

    return _payload


def run_bin(*args):
    out = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=120)
    return out.returncode, json.loads(out.stdout), out


def i8(*shape):
    return np.zeros(shape, np.int8)


def ones(n):
    return np.ones(n, np.float32)


# ---- CPU ------------------------------------------------------------------

@pytest.mark.parametrize("a,b,error", [
    (i8(2, 3, 4), i8(4, 2), ValueError), (i8(3), i8(3, 2), ValueError),  # rank
    (i8(2, 3), i8(3), ValueError),
    (i8(2, 3), i8(4, 2), ValueError),                                    # K differs
    (i8(1, 131072), i8(131072, 1), ValueError),                          # K limit
    (np.zeros((2, 3), np.int32), i8(3, 2), TypeError),                   # dtype
    (i8(2, 3), np.zeros((3, 2), np.uint8), TypeError),
    (i8(2, 3), np.zeros((3, 2), np.float32), TypeError),
])
def test_gemm_i8_and_w8a8_reject_bad_operands(payload, a, b, error):
    with pytest.raises(error):
        payload.gemm_i8(a, b)
    with pytest.raises(error):
        payload.gemm_w8a8(a, b, ones(a.shape[0]), ones(b.shape[-1]))


@pytest.mark.parametrize("sa,sb", [
    (ones(3), ones(5)), (ones(4), ones(4)), (ones((4, 1)), ones(5)),  # length
    (np.array([1, np.inf, 1, 1], np.float32), ones(5)),
    (ones(4), np.array([1, 1, np.nan, 1, 1], np.float32)),
    (ones(4), np.array([1, 1, 1, 1, -np.inf], np.float32)),
])
def test_gemm_w8a8_rejects_bad_scales(payload, sa, sb):
    with pytest.raises(ValueError):
        payload.gemm_w8a8(i8(4, 40), i8(40, 5), sa, sb)


def test_quantize_i8_is_the_documented_rule(payload):
    x = np.random.default_rng(3).standard_normal((5, 70)).astype(np.float32)
    x[1] = 0.0
    x[3, 17] = -9.5  # the row's absmax is a negative element
    x[4] = np.float32(1e-44) * np.sign(x[4])  # subnormals: absmax / 127 is zero
    codes, scales = payload.quantize_i8(x)
    quotient = np.abs(x).max(axis=-1) / np.float32(127.0)
    want_scales = np.where(quotient > 0, quotient, np.float32(1.0)).astype(np.float32)
    want_codes = np.clip(np.rint(x / want_scales[:, None]), -127, 127).astype(np.int8)
    assert codes.dtype == np.int8 and scales.dtype == np.float32
    assert scales.tobytes() == want_scales.tobytes()
    assert scales[1] == 1.0 and scales[4] == 1.0 and not codes[4].any()
    assert np.array_equal(codes, want_codes)
    assert codes.min() == -127 and codes[3, 17] == -127 and not codes[1].any()
    for bad in (np.inf, -np.inf, np.nan):
        x[2, 69] = bad
        with pytest.raises(ValueError):
            payload.quantize_i8(x)


def report(**over):
    r = {"ok": True, "cmd": "igemm", "m": 4096, "n": 4096, "k": 4096,
         "iters": 10, "tflops": 1400.0, "max_err": 0}
    r.update(over)
    return r


def test_judge_igemm_pass():
    rep = report()
    v = verify.judge_igemm(rep, "cpx-1x36")
    assert v == {"ok": True, "failed": [], "profile": "cpx-1x36", "report": rep}
    assert verify.judge_igemm(report(tflops=0.0, ok=False, max_err=0.0),
                              "cpx-1x36")["ok"] is True
    with pytest.raises(ValueError):
        verify.judge_igemm(rep, "not-a-profile")


@pytest.mark.parametrize("over", [
    {"max_err": 1}, {"max_err": 1e300}, {"max_err": True},
    {"max_err": None}, {"m": 0}, {"n": 0}, {"k": 0}, {"iters": 0}])
def test_judge_igemm_fail(over):
    assert verify.judge_igemm(report(**over), "cpx-1x36")["failed"] == ["igemm"]
    rep = report()
    del rep[next(iter(over))]
    v = verify.judge_igemm(rep, "cpx-1x36")
    assert v["ok"] is False and v["failed"] == ["igemm"]


# ---- GPU: the kernel ------------------------------------------------------

SHAPES = [
    (32, 32, 32),      # one MFMA
    (32, 32, 128),     # all four sub-steps of a K-step
    (1, 1, 1),         # everything is padding
    (33, 17, 40),      # ragged everywhere
    (96, 160, 224),    # several workgroups, K no power of two
    (130, 70, 1040),   # nine K-steps, multi-tile
]


def operands(m, n, k):
    rng = np.random.default_rng(1000 * m + 10 * n + k)
    return (rng.integers(-128, 127, size=(m, k), endpoint=True, dtype=np.int8),
            rng.integers(-128, 127, size=(k, n), endpoint=True, dtype=np.int8))


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_gemm_i8_exact_vs_int64(payload, m, n, k):
    a, b = operands(m, n, k)
    out = payload.gemm_i8(a, b)
    assert out.dtype == np.int32 and out.shape == (m, n)
    assert np.array_equal(out, a.astype(np.int64) @ b.astype(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("other,want", [(-128, 2147467264), (127, -2130690176)])
def test_gemm_i8_whole_accumulator_range(payload, other, want):
    a = np.full((1, 131071), -128, np.int8)
    b = np.full((131071, 1), other, np.int8)
    out = payload.gemm_i8(a, b)
    assert out.dtype == np.int32 and out.tolist() == [[want]]


@pytest.mark.gpu
def test_gemm_i8_one_hot_a_pins_k_and_the_32x32_map(payload):
    rng = np.random.default_rng(7)
    perm = rng.permutation(128)
    a = i8(128, 128)
    a[np.arange(128), perm] = 1
    b = rng.integers(-128, 127, size=(128, 48), endpoint=True, dtype=np.int8)
    assert np.array_equal(payload.gemm_i8(a, b), b[perm].astype(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", SHAPES[3:])
def test_gemm_w8a8_bitwise_vs_float32(payload, m, n, k):
    a, b = operands(m, n, k)
    rng = np.random.default_rng(k)
    sa = rng.uniform(2.0 ** -10, 1.0, size=m).astype(np.float32)
    sb = rng.uniform(2.0 ** -10, 1.0, size=n).astype(np.float32)
    acc = (a.astype(np.int64) @ b.astype(np.int64)).astype(np.int32)
    want = (acc.astype(np.float32) * sa[:, None]) * sb[None, :]
    out = payload.gemm_w8a8(a, b, sa, sb)
    assert out.dtype == np.float32 and out.shape == (m, n)
    assert want.dtype == np.float32 and out.tobytes() == want.tobytes()


@pytest.mark.gpu
def test_run_igemm_check_exact_and_k_limit(payload):
    assert payload.run_igemm_check(96, 160, 224) == 0.0
    with pytest.raises(ValueError):
        payload.run_igemm_check(64, 64, 131072)
    with pytest.raises(ValueError):
        payload.run_igemm(64, 64, 131072, iters=1)


@pytest.mark.gpu
def test_run_igemm_timed(payload):
    r = payload.run_igemm(1024, 1024, 512, iters=3)
    print(f"\nrun_igemm 1024x1024x512: {r['tflops']:.1f} TOP/s")
    assert (r["m"], r["n"], r["k"], r["iters"]) == (1024, 1024, 512, 3)
    assert r["max_err"] == 0.0
    assert np.isfinite(r["tflops"]) and r["tflops"] > 0


# ---- GPU: the binary and the probe ------------------------------------------

@pytest.mark.gpu
def test_binary_igemm():
    rc, res, out = run_bin("igemm", "96", "160", "224", "1")
    assert rc == 0, out.stdout + out.stderr
    assert res["ok"] is True and res["cmd"] == "igemm" and res["max_err"] == 0
    assert (res["m"], res["n"], res["k"], res["iters"]) == (96, 160, 224, 1)


@pytest.mark.gpu
def test_serve_igemm():
    out = subprocess.run([BIN, "serve"], input="igemm 64 64 64\nquit\n",
                         capture_output=True, text=True, timeout=60)
    ig, quit_ = [json.loads(ln) for ln in out.stdout.splitlines()]
    assert ig == {"ok": True, "cmd": "igemm", "m": 64, "n": 64, "k": 64, "max_err": 0}
    assert quit_ == {"ok": True}


@pytest.mark.gpu
def test_run_igemm_judges_the_real_partition():
    from instaslice_amd.partition.profiles import mi355x_catalog

    rc, census, out = run_bin("census")
    assert rc == 0, out.stdout + out.stderr
    name = next(p.name for p in mi355x_catalog().profiles
                if p.xcds == census["xcds_visible"])
    v = verify.run_igemm(name)
    print(f"\nrun_igemm({name}): {v}")
    assert v["ok"] is True and v["failed"] == [] and v["profile"] == name
