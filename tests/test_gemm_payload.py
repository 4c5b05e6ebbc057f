"""The bf16 MFMA GEMM payload (ops/csrc/payload_gemm.hpp): host-side bf16
rounding on CPU; the kernel, its bindings and the binary's `gemm` / `verify`
verbs on a real MI355X.

Integer inputs in [-4, 4] are exact in bf16 and every partial sum is an
integer below 2^24, so the correct fp32 result is bit-exact in any
accumulation order: those tests compare with tolerance 0.
"""

import json
import os
import subprocess

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


def torch_bf16_bits(x):
    import torch

    return (torch.tensor(x).to(torch.bfloat16).view(torch.int16)
            .numpy().view(np.uint16))


# ---- CPU: to_bf16 ---------------------------------------------------------

def test_to_bf16_matches_torch_on_normals(payload):
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    got = payload.to_bf16(x)
    assert got.dtype == np.uint16 and got.shape == x.shape
    assert np.array_equal(got, torch_bf16_bits(x))


def test_to_bf16_edge_values(payload):
    x = np.concatenate([
        np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0], dtype=np.float32),
        bits([
            0x3F808000,  # tie, rounds to even: down to 0x3F80
            0x3F818000,  # tie, rounds to even: up to 0x3F82
            0x7F7FFFFF,  # largest float: rounds to inf
            0x00000001, 0x00008000, 0x00018000, 0x807FFFFF,  # subnormals
            0x00800000,  # smallest normal
        ]),
    ])
    got = payload.to_bf16(x)
    assert np.array_equal(got, torch_bf16_bits(x))
    assert list(got[:9]) == [0x0000, 0x8000, 0x7F80, 0xFF80, 0x3F80, 0xBF80,
                             0x3F80, 0x3F82, 0x7F80]
    assert got[10] == 0x0000 and got[11] == 0x0002  # ties among subnormals
    assert got[12] == 0x8080  # rounded up into the normals, not flushed
    assert got[13] == 0x0080


def test_to_bf16_nan_stays_nan(payload):
    x = bits([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF])
    got = payload.to_bf16(x).astype(np.uint32)
    back = (got << 16).view(np.float32)
    assert np.isnan(back).all()


def test_to_bf16_keeps_shape_and_converts_input(payload):
    x = np.arange(12, dtype=np.float64).reshape(3, 4)[:, ::2]  # f64, strided
    got = payload.to_bf16(x)
    assert got.shape == (3, 2)
    assert np.array_equal(got, torch_bf16_bits(np.ascontiguousarray(x, np.float32)))


def test_gemm_bf16_rejects_bad_arguments(payload):
    # argument checks come before any device work
    f = np.zeros
    with pytest.raises(ValueError):
        payload.gemm_bf16(f((2, 3, 4), np.float32), f((4, 2), np.float32))
    with pytest.raises(ValueError):
        payload.gemm_bf16(f(3, np.float32), f((3, 2), np.float32))
    with pytest.raises(ValueError):
        payload.gemm_bf16(f((2, 3), np.float32), f((4, 2), np.float32))
    with pytest.raises((TypeError, ValueError)):
        payload.gemm_bf16("not an array", f((4, 2), np.float32))


# ---- GPU: kernel through the bindings -------------------------------------

SHAPES = [
    (16, 16, 32),     # one MFMA
    (1, 1, 1),        # everything is padding
    (33, 17, 40),     # ragged in every dimension
    (64, 64, 64),     # several K-steps
    (96, 160, 224),   # several workgroups on both axes, K not a power of two
    (130, 70, 1024),  # the K limit, ragged, multi-tile
]


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_gemm_bf16_exact_vs_numpy(payload, m, n, k):
    rng = np.random.default_rng(1000 * m + 10 * n + k)
    a = rng.integers(-4, 5, size=(m, k)).astype(np.float32)
    b = rng.integers(-4, 5, size=(k, n)).astype(np.float32)
    out = payload.gemm_bf16(a, b)
    ref = (a.astype(np.int64) @ b.astype(np.int64)).astype(np.float32)
    assert out.dtype == np.float32 and out.shape == (m, n)
    assert np.array_equal(out, ref)


@pytest.mark.gpu
def test_gemm_bf16_one_hot_a_pins_k_order(payload):
    perm = np.random.default_rng(7).permutation(64)
    a = np.zeros((64, 64), dtype=np.float32)
    a[np.arange(64), perm] = 1.0
    # integers 0..255 (exact in bf16), asymmetric, every row different
    b = ((np.arange(64)[:, None] + 67 * np.arange(48)[None, :]) % 256)
    b = b.astype(np.float32)
    assert len(np.unique(b[:, 0])) == 64  # rows are told apart in column 0
    out = payload.gemm_bf16(a, b)
    assert np.array_equal(out, b[perm])


@pytest.mark.gpu
def test_gemm_bf16_converts_strided_and_f64_input(payload):
    rng = np.random.default_rng(3)
    a = rng.integers(-4, 5, size=(40, 33)).astype(np.float64)
    b = rng.integers(-4, 5, size=(20, 33)).astype(np.float32).T  # (33,20) strided
    out = payload.gemm_bf16(a, b)
    assert np.array_equal(out, (a @ b).astype(np.float32))


@pytest.mark.gpu
def test_gemm_bf16_rounded_input_numerics(payload):
    """|C - ref| <= K * 2^-23 * (|A| @ |B|) elementwise, ref in float64 on the
    bf16-rounded inputs. Derived, not measured: bf16 x bf16 products are exact
    in fp32 and each of the K accumulations adds at most one fp32 ulp of the
    magnitude sum (2^-23 rather than 2^-24 allows a truncating adder)."""
    m, n, k = 96, 160, 224
    rng = np.random.default_rng(11)
    a = rng.uniform(-1, 1, size=(m, k)).astype(np.float32)
    b = rng.uniform(-1, 1, size=(k, n)).astype(np.float32)
    ar = (payload.to_bf16(a).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    br = (payload.to_bf16(b).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    out = payload.gemm_bf16(a, b).astype(np.float64)
    ref = ar @ br
    bound = k * 2.0 ** -23 * (np.abs(ar) @ np.abs(br))
    err = np.abs(out - ref)
    print(f"\nmax |err| / bound = {(err / bound).max():.4f}, "
          f"max |err| = {err.max():.3e}")
    assert (err <= bound).all()


@pytest.mark.gpu
def test_run_gemm_check_exact(payload):
    assert payload.run_gemm_check(96, 160, 224) == 0.0


@pytest.mark.gpu
def test_run_gemm_check_rejects_k_above_limit(payload):
    with pytest.raises(ValueError):
        payload.run_gemm_check(64, 64, 2048)


@pytest.mark.gpu
def test_run_gemm_timed(payload):
    r = payload.run_gemm(1024, 1024, 512, iters=3)
    print(f"\nrun_gemm 1024x1024x512: {r['tflops']:.1f} TFLOP/s")
    assert r["max_err"] == 0.0
    assert np.isfinite(r["tflops"]) and r["tflops"] > 0


# ---- GPU: the binary ------------------------------------------------------

def run_bin(*args):
    out = subprocess.run([BIN, *args], capture_output=True, text=True,
                         timeout=120)
    return out.returncode, json.loads(out.stdout), out


@pytest.mark.gpu
def test_binary_gemm():
    rc, res, out = run_bin("gemm", "96", "160", "224", "1")
    assert rc == 0, out.stdout + out.stderr
    assert res["ok"] is True and res["cmd"] == "gemm" and res["max_err"] == 0
    assert (res["m"], res["n"], res["k"], res["iters"]) == (96, 160, 224, 1)


@pytest.fixture(scope="module")
def verify_report():
    rc, res, out = run_bin("verify")
    assert rc == 0, out.stdout + out.stderr
    return res


@pytest.mark.gpu
def test_binary_verify_unchecked(verify_report):
    res = verify_report
    print(f"\nverify: {res}")
    assert res["ok"] is True and res["failed"] == []
    assert res["xcds_expected"] == 0
    assert res["xcds_visible"] == sum(1 for c in res["per_xcd"] if c) >= 1
    assert res["vecadd_max_err"] == 0 and res["gemm_max_err"] == 0
    for key in ("cu_count", "total_mem_gb", "gb_per_s", "tflops",
                "gb_per_s_per_xcd", "tflops_per_xcd"):
        assert res[key] > 0


@pytest.mark.gpu
def test_binary_verify_xcds(verify_report):
    xcds = verify_report["xcds_visible"]
    rc, res, out = run_bin("verify", str(xcds))
    assert rc == 0, out.stdout + out.stderr
    assert res["ok"] is True and res["xcds_expected"] == xcds
    rc, res, out = run_bin("verify", str(xcds + 1))
    assert rc == 1
    assert res["ok"] is False and res["failed"] == ["xcds"]


@pytest.mark.gpu
def test_verify_run_judges_the_real_partition(verify_report):
    """ops/verify.run end to end, against the profile matching this device."""
    from instaslice_amd.ops import verify
    from instaslice_amd.partition.profiles import mi355x_catalog

    xcds = verify_report["xcds_visible"]
    name = next(p.name for p in mi355x_catalog().profiles if p.xcds == xcds)
    v = verify.run(name)
    assert v["ok"] is True and v["failed"] == [] and v["profile"] == name


@pytest.mark.gpu
def test_serve_gemm():
    w = subprocess.Popen([BIN, "serve"], stdin=subprocess.PIPE,
                         stdout=subprocess.PIPE, text=True, bufsize=1)
    try:
        out, _ = w.communicate("vecadd 1048576\ngemm 64 64 64\nping\nquit\n",
                               timeout=60)
    finally:
        if w.poll() is None:
            w.kill()
    vec, gemm, ping, quit_ = [json.loads(ln) for ln in out.splitlines()]
    assert vec["ok"] and vec["max_err"] == 0
    assert gemm["ok"] is True and gemm["cmd"] == "gemm" and gemm["max_err"] == 0
    assert (gemm["m"], gemm["n"], gemm["k"]) == (64, 64, 64)
    assert ping == {"ok": True, "cmd": "ping"}
    assert quit_["ok"]
