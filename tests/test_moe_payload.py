"""The routed mixture-of-experts grouped GEMM payload (ops/csrc/payload_moe.hpp):
argument checks and the judge on CPU; the routing kernels, both geometries of
the grouped GEMM, the combine, the bindings, the binary's `moe` verb and
`verify.run_moe` on a real MI355X.

The exact checks are honest because zero is attainable: with |x|, |w| <= 4, K
<= 1024, gates in {0.25, 0.5, 1, 2} and topk <= 8 every partial sum times 4 is
an integer of magnitude at most 4 * 16 * 1024 * 2 * 8 = 2^20 < 2^24, so fp32 is
exact in any order and equals the int64 reference over 4.
"""

import json
import os
import subprocess

import numpy as np
import pytest

from instaslice_amd.ops import verify

BIN = os.path.join(os.path.dirname(__file__), "..", "instaslice_amd", "bin",
                   "instaslice-payload")
BMS = [32, 128]


@pytest.fixture(scope="module")
def payload():
    from instaslice_amd.ops import _payload

    return _payload


def run_bin(*args):
    out = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=120)
    return out.returncode, json.loads(out.stdout), out


def operands(t, n, k, e, topk, experts=None, integer=True):
    """x, w, ids (a token's experts all different, drawn from `experts`), gates."""
    rng = np.random.default_rng([t, n, k, e, topk])
    if integer:
        x = rng.integers(-4, 4, size=(t, k), endpoint=True).astype(np.float32)
        w = rng.integers(-4, 4, size=(e, k, n), endpoint=True).astype(np.float32)
        gates = rng.choice(np.float32([0.25, 0.5, 1, 2]), size=(t, topk))
    else:
        x, w, gates = (rng.uniform(-1, 1, size=s).astype(np.float32)
                       for s in ((t, k), (e, k, n), (t, topk)))
    pool = np.arange(e) if experts is None else np.asarray(experts)
    ids = np.stack([rng.permutation(pool)[:topk] for _ in range(t)]).astype(np.int32)
    return x, w, ids, gates


def reference(x, w, ids, gates, dtype=np.float64):
    """sum_j gates[t, j] * (x[t] @ w[ids[t, j]]) in `dtype`"""
    x, w, gates = (np.asarray(v).astype(dtype) for v in (x, w, gates))
    return sum(gates[:, j, None] * np.einsum("tk,tkn->tn", x, w[ids[:, j]])
               for j in range(ids.shape[1]))


# ---- CPU ------------------------------------------------------------------

def f32(*shape):
    return np.zeros(shape, np.float32)


def idm(*rows):
    return np.array(rows, np.int32)


OK = dict(x=f32(2, 3), w=f32(4, 3, 5), ids=idm([0, 1], [2, 3]))
INF = np.array([[1, np.inf], [1, 1]], np.float32)
NAN = np.array([[1, 1], [np.nan, 1]], np.float32)


@pytest.mark.parametrize("over,error", [
    (dict(x=f32(3)), ValueError), (dict(x=f32(2, 3, 1)), ValueError),      # ranks
    (dict(w=f32(3, 5)), ValueError), (dict(ids=idm(0, 1)), ValueError),
    (dict(x=f32(2, 4)), ValueError),                                       # K differs
    (dict(w=f32(257, 3, 5)), ValueError),                                  # E = 257
    (dict(w=f32(16, 3, 5), ids=np.arange(18, dtype=np.int32).reshape(2, 9) % 16),
     ValueError),                                                          # topk = 9
    (dict(w=f32(1, 3, 5), ids=idm([0, 0], [0, 0])), ValueError),           # topk > E
    (dict(ids=idm([0, -1], [2, 3])), ValueError),                          # id of -1
    (dict(ids=idm([0, 1], [2, 4])), ValueError),                           # id of E
    (dict(ids=idm([0, 1], [3, 3])), ValueError),                           # twice
    (dict(gates=f32(2, 3)), ValueError), (dict(gates=f32(2)), ValueError),
    (dict(gates=INF), ValueError), (dict(gates=NAN), ValueError),
    (dict(bm=64), ValueError),
    (dict(ids=np.array([[0., 1.], [2., 3.]])), TypeError),                 # float ids
])
def test_moe_gemm_rejects_bad_arguments(payload, over, error):
    with pytest.raises(error):
        payload.moe_gemm(**{**OK, **over})


def report(**over):
    r = {"ok": True, "cmd": "moe", "tokens": 8192, "n": 4096, "k": 1024,
         "experts": 32, "topk": 4, "bm": 128, "iters": 10, "tflops": 300.0,
         "tokens_per_s": 1e7, "max_err": 0}
    r.update(over)
    return r


def test_judge_moe_pass():
    rep = report()
    v = verify.judge_moe(rep, "cpx-1x36")
    assert v == {"ok": True, "failed": [], "profile": "cpx-1x36", "report": rep}
    assert verify.judge_moe(report(tflops=0.0, ok=False, max_err=0.0, bm=32),
                            "cpx-1x36")["ok"] is True
    with pytest.raises(ValueError):
        verify.judge_moe(rep, "not-a-profile")


@pytest.mark.parametrize("over", [
    {"max_err": 1}, {"max_err": 1e300}, {"max_err": True}, {"max_err": None},
    {"tokens": 0}, {"n": 0}, {"k": 0}, {"experts": 0}, {"topk": 0}, {"iters": 0},
    {"bm": 64}, {"bm": 32.0}])
def test_judge_moe_fail(over):
    assert verify.judge_moe(report(**over), "cpx-1x36")["failed"] == ["moe"]
    rep = report()
    del rep[next(iter(over))]
    v = verify.judge_moe(rep, "cpx-1x36")
    assert v["ok"] is False and v["failed"] == ["moe"]


# ---- GPU: the kernels -------------------------------------------------------

CASES = [
    (1, 1, 1, 1, 1, None),             # everything is padding
    (5, 17, 40, 4, 2, None),           # ragged everywhere, under a tile per expert
    (40, 130, 96, 3, 3, None),         # every token to every expert, two tiles in N
    (300, 64, 64, 2, 1, None),         # runs that span tiles and end inside one
    (64, 48, 1024, 8, 8, None),        # largest topk, largest exact K
    (70, 32, 72, 6, 2, (0, 2, 3, 5)),  # experts 1 and 4 empty
]


@pytest.mark.gpu
@pytest.mark.parametrize("bm", BMS)
@pytest.mark.parametrize("t,n,k,e,topk,experts", CASES)
def test_moe_gemm_exact_vs_int64(payload, t, n, k, e, topk, experts, bm):
    x, w, ids, gates = operands(t, n, k, e, topk, experts)
    want4 = reference(x, w, ids, gates * 4, np.int64)
    out = payload.moe_gemm(x, w, ids, gates, bm=bm)
    assert out.dtype == np.float32 and out.shape == (t, n)
    assert np.array_equal(out, want4 / 4.0)


@pytest.mark.gpu
@pytest.mark.parametrize("bm", BMS)
def test_moe_gemm_one_hot_pins_gather_expert_perm_and_gate(payload, bm):
    rng = np.random.default_rng(11)
    p = rng.permutation(96)
    x = f32(96, 96)
    x[np.arange(96), p] = 1
    w = np.broadcast_to(rng.permutation(256)[:192].reshape(2, 96, 1),
                        (2, 96, 24)).astype(np.float32)
    ids = np.stack([rng.permutation(2) for _ in range(96)]).astype(np.int64)
    gates = np.tile(np.float32([1, 0.5]), (96, 1))
    out = payload.moe_gemm(x, w, ids, gates, bm=bm)
    assert np.array_equal(out, w[ids[:, 0], p] + 0.5 * w[ids[:, 1], p])


@pytest.mark.gpu
@pytest.mark.parametrize("bm", BMS)
def test_moe_gemm_dense_numerics_vs_float64(payload, bm):
    t, n, k, e, topk = 70, 96, 200, 6, 2
    x, w, ids, gates = operands(t, n, k, e, topk, integer=False)
    # to_bf16 gives the bits; shifted up they are the rounded values as float32
    xb, wb = ((payload.to_bf16(v).astype(np.uint32) << 16).view(np.float32)
              for v in (x, w))
    for g in (gates, None):  # absent: all ones
        gv = np.ones_like(gates) if g is None else g
        bound = (k + topk + 1) * 2.0 ** -23 * reference(np.abs(xb), np.abs(wb), ids,
                                                        np.abs(gv))
        err = np.abs(payload.moe_gemm(x, w, ids, g, bm=bm) - reference(xb, wb, ids, gv))
        print(f"\nbm {bm}: max err / bound = {(err / bound).max():.3f}")
        assert (err <= bound).all()


@pytest.mark.gpu
def test_moe_route_sorts_slots_by_expert(payload):
    _, _, ids, _ = operands(300, 1, 1, 6, 2, experts=(0, 1, 3, 5))
    perm, seg = payload.moe_route(ids, 6)
    assert perm.dtype == np.int32 and seg.dtype == np.int32
    counts = np.bincount(ids.ravel(), minlength=6)
    assert np.array_equal(seg, np.concatenate([[0], np.cumsum(counts)]))
    assert np.array_equal(np.sort(perm), np.arange(600))
    for e in range(6):
        assert set(perm[seg[e]:seg[e + 1]]) == set(np.flatnonzero(ids.ravel() == e))


@pytest.mark.gpu
def test_run_moe_check_exact_and_k_limit(payload):
    for bm in BMS:
        assert payload.run_moe_check(300, 160, 224, 6, 2, bm=bm) == 0.0
    with pytest.raises(ValueError):
        payload.run_moe_check(64, 64, 1025, 4, 2)
    with pytest.raises(ValueError):
        payload.run_moe(64, 64, 1025, 4, 2, iters=1)


@pytest.mark.gpu
def test_run_moe_timed(payload):
    r = payload.run_moe(512, 256, 256, 8, 2, iters=3)
    print(f"\nrun_moe 512x256x256, 8 experts, top-2: {r['tflops']:.1f} TFLOP/s")
    assert (r["tokens"], r["n"], r["k"], r["experts"], r["topk"], r["iters"]) == \
        (512, 256, 256, 8, 2, 3)
    assert r["bm"] == 128 and r["max_err"] == 0.0
    assert np.isfinite(r["tflops"]) and r["tflops"] > 0


# ---- GPU: the binary and the probe ------------------------------------------

@pytest.mark.gpu
def test_binary_moe():
    rc, res, out = run_bin("moe", "300", "160", "224", "6", "2", "1")
    assert rc == 0, out.stdout + out.stderr
    assert res["ok"] is True and res["cmd"] == "moe" and res["max_err"] == 0
    assert [res[key] for key in ("tokens", "n", "k", "experts", "topk", "iters")] == \
        [300, 160, 224, 6, 2, 1]


@pytest.mark.gpu
def test_serve_moe():
    out = subprocess.run([BIN, "serve"], input="moe\nquit\n",
                         capture_output=True, text=True, timeout=60)
    moe, quit_ = [json.loads(ln) for ln in out.stdout.splitlines()]
    assert moe == {"ok": True, "cmd": "moe", "tokens": 300, "n": 160, "k": 224,
                   "experts": 6, "topk": 2, "max_err": 0}
    assert quit_ == {"ok": True}


@pytest.mark.gpu
def test_run_moe_judges_the_real_partition():
    from instaslice_amd.partition.profiles import mi355x_catalog

    rc, census, out = run_bin("census")
    assert rc == 0, out.stdout + out.stderr
    name = next(p.name for p in mi355x_catalog().profiles
                if p.xcds == census["xcds_visible"])
    v = verify.run_moe(name)
    print(f"\nrun_moe({name}): {v}")
    assert v["ok"] is True and v["failed"] == [] and v["profile"] == name
