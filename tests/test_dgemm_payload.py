"""The FP64 MFMA GEMM payload (ops/csrc/payload_dgemm.hpp): argument checks
and the judge on CPU; the kernel, its bindings, the binary's `dgemm` verb and
`verify.run_dgemm` on a real MI355X.

The integer GPU test is exact: operands in [-2^20, 2^20] give products below
2^40 and sums of K <= 1040 of them, in any order, below 2^50.1, inside fp64's
53 bits and int64's 63. The bound of the general test is derived, not
measured: each of the K accumulation steps may add one ulp (2^-52 relative: a
truncating fused adder, or a multiply and an add each rounded to nearest) of
a partial sum that never exceeds sum |a| |b|.
"""

import json
import os
import subprocess
from fractions import Fraction

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


# ---- CPU ------------------------------------------------------------------

def test_gemm_f64_rejects_bad_arguments(payload):
    f = np.zeros
    with pytest.raises(ValueError):
        payload.gemm_f64(f((2, 3, 4)), f((4, 2)))
    with pytest.raises(ValueError):
        payload.gemm_f64(f(3), f((3, 2)))
    with pytest.raises(ValueError):
        payload.gemm_f64(f((2, 3)), f((4, 2)))
    with pytest.raises((TypeError, ValueError)):
        payload.gemm_f64("not an array", f((4, 2)))
    for bad in (np.inf, -np.inf, np.nan):
        a, b = np.ones((2, 40)), np.ones((40, 3))
        a[1, 33] = bad
        with pytest.raises(ValueError):
            payload.gemm_f64(a, b)
        with pytest.raises(ValueError):
            payload.gemm_f64(b.T.copy(), a.T.copy())


def report(**over):
    r = {"ok": True, "cmd": "dgemm", "m": 4096, "n": 4096, "k": 1024,
         "iters": 10, "tflops": 61.5, "max_err": 0}
    r.update(over)
    return r


def test_judge_dgemm_pass():
    rep = report()
    v = verify.judge_dgemm(rep, "cpx-1x36")
    assert v == {"ok": True, "failed": [], "profile": "cpx-1x36", "report": rep}
    assert verify.judge_dgemm(report(tflops=0.0, ok=False, max_err=0.0),
                              "cpx-1x36")["ok"] is True
    with pytest.raises(ValueError):
        verify.judge_dgemm(rep, "not-a-profile")


@pytest.mark.parametrize("over", [
    {"max_err": 2.0 ** -32}, {"max_err": 1e300}, {"max_err": True},
    {"max_err": None}, {"m": 0}, {"n": 0}, {"k": 0}, {"iters": 0}])
def test_judge_dgemm_fail(over):
    assert verify.judge_dgemm(report(**over), "cpx-1x36")["failed"] == ["dgemm"]
    rep = report()
    del rep[next(iter(over))]
    v = verify.judge_dgemm(rep, "cpx-1x36")
    assert v["ok"] is False and v["failed"] == ["dgemm"]


# ---- GPU: the kernel ------------------------------------------------------

SHAPES = [
    (16, 16, 4),       # one MFMA
    (16, 16, 8),       # both doubles of one slot
    (1, 1, 1),         # everything is padding
    (33, 17, 40),      # ragged everywhere
    (96, 160, 224),    # several workgroups on both axes, K no power of two
    (130, 70, 1040),   # many K-steps, multi-tile
]


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_gemm_f64_exact_vs_int64(payload, m, n, k):
    rng = np.random.default_rng(1000 * m + 10 * n + k)
    a = rng.integers(-2 ** 20, 2 ** 20, size=(m, k), endpoint=True)
    b = rng.integers(-2 ** 20, 2 ** 20, size=(k, n), endpoint=True)
    out = payload.gemm_f64(a.astype(np.float64), b.astype(np.float64))
    assert out.dtype == np.float64 and out.shape == (m, n)
    assert np.array_equal(out, (a.astype(np.int64) @ b.astype(np.int64))
                          .astype(np.float64))


@pytest.mark.gpu
def test_gemm_f64_one_hot_a_pins_k_and_rows(payload):
    rng = np.random.default_rng(7)
    perm = rng.permutation(64)
    a = np.zeros((64, 64))
    a[np.arange(64), perm] = 1.0
    b = rng.standard_normal((64, 48))  # full 53-bit mantissas
    assert payload.gemm_f64(a, b).tobytes() == b[perm].tobytes()


@pytest.mark.gpu
def test_gemm_f64_general_doubles_vs_exact_rational(payload):
    m, n, k = 48, 40, 100
    rng = np.random.default_rng(11)
    a, b = rng.uniform(-1, 1, size=(m, k)), rng.uniform(-1, 1, size=(k, n))
    fa = [[Fraction(x) for x in row] for row in a]
    fb = [[Fraction(x) for x in col] for col in b.T]
    out = payload.gemm_f64(a, b)
    err = np.array([[float(abs(Fraction(out[i, j]) -
                               sum(x * y for x, y in zip(fa[i], fb[j]))))
                     for j in range(n)] for i in range(m)])
    bound = k * 2.0 ** -52 * (np.abs(a) @ np.abs(b))
    print(f"\nmax |err| / bound = {(err / bound).max():.4f}, "
          f"max |err| = {err.max():.3e}")
    assert out.shape == (m, n)
    assert (err <= bound).all()


@pytest.mark.gpu
def test_run_dgemm_check_exact_and_k_limit(payload):
    assert payload.run_dgemm_check(96, 160, 224) == 0.0
    with pytest.raises(ValueError):
        payload.run_dgemm_check(64, 64, 65537)
    with pytest.raises(ValueError):
        payload.run_dgemm(64, 64, 65537, iters=1)


@pytest.mark.gpu
def test_run_dgemm_timed(payload):
    r = payload.run_dgemm(1024, 1024, 512, iters=3)
    print(f"\nrun_dgemm 1024x1024x512: {r['tflops']:.1f} TFLOP/s")
    assert (r["m"], r["n"], r["k"], r["iters"]) == (1024, 1024, 512, 3)
    assert r["max_err"] == 0.0
    assert np.isfinite(r["tflops"]) and r["tflops"] > 0


# ---- GPU: the binary and the probe ------------------------------------------

@pytest.mark.gpu
def test_binary_dgemm():
    rc, res, out = run_bin("dgemm", "96", "160", "224", "1")
    assert rc == 0, out.stdout + out.stderr
    assert res["ok"] is True and res["cmd"] == "dgemm" and res["max_err"] == 0
    assert (res["m"], res["n"], res["k"], res["iters"]) == (96, 160, 224, 1)


@pytest.mark.gpu
def test_serve_dgemm():
    out = subprocess.run([BIN, "serve"], input="dgemm 64 64 64\nquit\n",
                         capture_output=True, text=True, timeout=60)
    dg, quit_ = [json.loads(ln) for ln in out.stdout.splitlines()]
    assert dg == {"ok": True, "cmd": "dgemm", "m": 64, "n": 64, "k": 64, "max_err": 0}
    assert quit_ == {"ok": True}


@pytest.mark.gpu
def test_run_dgemm_judges_the_real_partition():
    from instaslice_amd.partition.profiles import mi355x_catalog

    rc, census, out = run_bin("census")
    assert rc == 0, out.stdout + out.stderr
    name = next(p.name for p in mi355x_catalog().profiles
                if p.xcds == census["xcds_visible"])
    v = verify.run_dgemm(name)
    print(f"\nrun_dgemm({name}): {v}")
    assert v["ok"] is True and v["failed"] == [] and v["profile"] == name
