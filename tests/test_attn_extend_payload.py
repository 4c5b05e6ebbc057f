"""The paged chunked-prefill ("extend") attention payload
(ops/csrc/payload_attn_extend.hpp): the plan, the argument checks and the judge
on CPU; the kernel, its bindings, the binary's `extend` verb, `serve` and
`verify.run_extend` on a real MI355X.

The reference is numpy fp64 from the definition, on the bf16-rounded dense
tensors that the pool was scattered from: token i of the last n of a sequence's
len keys attends to the keys t <= len - n + i.

exact     prefill's selection pattern (prefill_check_pattern, causal): a causal
          row depends on the keys at or below it only, so the extend rows are
          rows len - n .. len - 1 of that closed form, bit for bit.
bounded   general data: |o - ref| <= 2^-8 max |v|, the bound derived in the
          docstring of tests/test_attn_paged_payload.py for these numerics.
"""

import json
import os
import subprocess

import numpy as np
import pytest

from instaslice_amd.ops import verify

BIN = os.path.join(os.path.dirname(__file__), "..", "instaslice_amd", "bin",
                   "instaslice-payload")
D = 128
REL = 2.0 ** -8
# (len, n): a single key; an empty prefix across a chunk edge; whole chunks;
# decode-shaped; a second column block that is almost empty (G = 8: 136
# columns); a prefix that ends inside a chunk and a page; a last tile with one
# real column at G = 3
PAIRS = [(1, 1), (33, 33), (64, 64), (300, 1), (300, 17), (129, 5), (100, 11)]
LENS, QLENS = [p[0] for p in PAIRS], [p[1] for p in PAIRS]


@pytest.fixture(scope="module")
def payload():
    from instaslice_amd.ops import _payload

    return _payload


def scatter(k, v, lens, page, seed, spare=3):
    """Dense (B, Hkv, L, 128) K and V into a pool under a seeded permutation
    table. Pages no entry names are NaN, table entries above a length are -1,
    stale keys of the last read 32-key chunk are 1e30."""
    B, Hkv, L, _ = k.shape
    W = -(-L // page)
    P = B * W + spare
    table = np.random.default_rng(seed).permutation(P)[:B * W].reshape(B, W)
    table = table.astype(np.int32)
    kp = np.full((P, Hkv, page, D), np.nan, np.float32)
    vp = kp.copy()
    for b, n in enumerate(lens):
        table[b, -(-n // page):] = -1
        for t in range(-(-n // 32) * 32):
            kp[table[b, t // page], :, t % page] = k[b, :, t] if t < n else 1e30
            vp[table[b, t // page], :, t % page] = v[b, :, t] if t < n else 1e30
    return kp, vp, table


def ref_extend(q, k, v, pairs):
    """q packed (Tq, Hq, 128), k and v dense: fp64 from the definition"""
    G = q.shape[1] // k.shape[1]
    out = np.empty(q.shape)
    at = 0
    for b, (ln, n) in enumerate(pairs):
        for i in range(n):
            for h in range(q.shape[1]):
                keys = ln - n + i + 1
                s = k[b, h // G, :keys].astype(np.float64) @ q[at + i, h].astype(np.float64)
                w = np.exp((s - s.max()) / np.sqrt(128.0))
                out[at + i, h] = (w @ v[b, h // G, :keys].astype(np.float64)) / w.sum()
        at += n
    return out


def bf16_round(payload, x):
    bits = payload.to_bf16(np.ascontiguousarray(x, dtype=np.float32))
    return (bits.astype(np.uint32) << 16).view(np.float32)


# ---- CPU ------------------------------------------------------------------

@pytest.mark.parametrize("qlens,G", [
    ([1], 1), ([17], 8), ([1] * 300, 16), ([1, 33, 64, 1, 17, 5, 11, 700], 3)])
def test_plan_covers_every_column_once(payload, qlens, G):
    items, cu = payload.attn_extend_plan(qlens, G)
    assert items.dtype == np.int32 and items.shape[1] == 2
    assert len(items) <= -(-sum(qlens) * G // 128) + len(qlens)
    assert np.array_equal(cu, np.cumsum([0] + qlens[:-1]))
    assert np.array_equal(items[:, 0], np.sort(items[:, 0]))    # in order of b
    for b, n in enumerate(qlens):
        first = items[items[:, 0] == b, 1]
        assert np.array_equal(first, np.arange(0, n * G, 128))  # blocks of 128 columns


@pytest.mark.parametrize("exc,change", [
    (ValueError, {"qlens": [0, 2]}), (ValueError, {"qlens": [3, 65]}),
    (ValueError, {"q": np.ones((6, 2, D), np.float32)}),         # Tq != sum(qlens)
    (ValueError, {"kp": np.ones((4, 1, 48, D), np.float32)}),    # a page of 48
    (ValueError, {"table": np.array([[0, 4], [2, 3]])}),         # needed entries
    (ValueError, {"q": np.full((5, 2, D), np.inf, np.float32)}),
    (ValueError, {"q": np.ones((5, 17, D), np.float32)}),        # G = 17
    (TypeError, {"qlens": [3.0, 2.0]})])
def test_rejects_bad_arguments(payload, exc, change):
    a = {"kp": np.ones((4, 1, 64, D), np.float32), "lens": [100, 64], "qlens": [3, 2],
         "table": np.array([[0, 1], [2, 3]], np.int32)}
    a.update(change)
    a.setdefault("q", np.ones((int(sum(a["qlens"])), 2, D), np.float32))
    with pytest.raises(exc):
        payload.attn_paged_extend(a["q"], a["kp"], a["kp"], a["table"], a["lens"],
                                  a["qlens"])


def report(**over):
    r = {"ok": True, "cmd": "extend", "batch": 8, "hq": 64, "hkv": 8, "len": 4096,
         "new": 1024, "page": 64, "iters": 10, "ragged": False, "items": 512,
         "tflops": 400.0, "tok_per_s": 1e6, "max_err": 0, "max_rel": 0.0003}
    r.update(over)
    return r


@pytest.mark.parametrize("over", [
    {}, {"ok": False, "tflops": 0.0}, {"page": 256}, {"max_rel": 2.0 ** -8}])
def test_judge_extend_passes(over):
    v = verify.judge_extend(report(**over), "cpx-1x36")
    assert v["ok"] is True and v["failed"] == []


@pytest.mark.parametrize("over", [
    {"max_err": 1e-30}, {"max_err": None}, {"max_rel": float("nan")},
    {"max_rel": float(np.nextafter(2.0 ** -8, 1.0))}, {"page": 48}, {"page": 64.0},
    {"items": 0}, {"new": 0}, {"new": 1.5}, {"batch": 0}])
def test_judge_extend_fails(over):
    v = verify.judge_extend(report(**over), "cpx-1x36")
    assert v["ok"] is False and v["failed"] == ["extend"]


# ---- GPU: the kernel against fp64 and the closed form -------------------------

@pytest.fixture(scope="module")
def dense(payload):
    """(q packed, k, v, fp64 reference) per head shape, computed once"""
    made = {}
    for hq, hkv in ((2, 2), (6, 2), (8, 1), (16, 1)):
        rng = np.random.default_rng(100 * hq + hkv)
        q = bf16_round(payload, 4 * rng.standard_normal((sum(QLENS), hq, D)))
        k = bf16_round(payload, rng.standard_normal((len(PAIRS), hkv, max(LENS), D)))
        v = bf16_round(payload, rng.uniform(-1, 1, k.shape))
        made[hq, hkv] = (q, k, v, ref_extend(q, k, v, PAIRS))
    return made


@pytest.mark.gpu
@pytest.mark.parametrize("page", [32, 64])
@pytest.mark.parametrize("hq,hkv", [(2, 2), (6, 2), (8, 1), (16, 1)])
def test_random_bounded(payload, dense, hq, hkv, page):
    q, k, v, ref = dense[hq, hkv]
    kp, vp, table = scatter(k, v, LENS, page, seed=7 * page + hq)
    out = payload.attn_paged_extend(q, kp, vp, table, LENS, QLENS)
    assert out.dtype == np.float32 and out.shape == q.shape
    err = np.abs(out.astype(np.float64) - ref).max() / np.abs(v).max()
    print(f"\npage {page} ({hq},{hkv}): max_rel {err:.3e}")
    assert np.isfinite(out).all() and err <= REL


@pytest.mark.gpu
@pytest.mark.parametrize("hq,hkv,page", [(6, 2, 32), (16, 1, 64)])
def test_pattern_exact(payload, hq, hkv, page):
    q, k, v, expected = payload.prefill_check_pattern(len(PAIRS), hq, hkv, max(LENS),
                                                      causal=True)

    def rows(x):  # (B, Hq, L, 128) -> the packed rows len - n .. len - 1
        return np.concatenate([x[b, :, ln - n:ln].transpose(1, 0, 2)
                               for b, (ln, n) in enumerate(PAIRS)])

    kp, vp, table = scatter(k, v, LENS, page, seed=page + hq)
    out = payload.attn_paged_extend(rows(q), kp, vp, table, LENS, QLENS)
    assert np.array_equal(out, rows(expected))


@pytest.mark.gpu
def test_shared_prefix(payload, dense):
    q, k, v, _ = dense[6, 2]
    pairs = [(300, 17), (200, 40)]
    q, k, v = q[:57], k[:2].copy(), v[:2].copy()
    k[1, :, :128], v[1, :, :128] = k[0, :, :128], v[0, :, :128]   # a common prefix
    lens, qlens = [p[0] for p in pairs], [p[1] for p in pairs]
    kp, vp, table = scatter(k, v, lens, 64, seed=5)
    private = payload.attn_paged_extend(q, kp, vp, table, lens, qlens)
    kp[table[1, :2]] = vp[table[1, :2]] = np.nan   # its own copy of the prefix goes
    table[1, :2] = table[0, :2]
    shared = payload.attn_paged_extend(q, kp, vp, table, lens, qlens)
    assert np.isfinite(shared).all()
    assert np.array_equal(shared.view(np.uint32), private.view(np.uint32))
    assert np.abs(shared - ref_extend(q, k, v, pairs)).max() <= REL * np.abs(v).max()


# ---- GPU: the self-check, the timed run, the binary, serve, the runner -------

@pytest.mark.gpu
@pytest.mark.parametrize("args", [(8, 8, 2, 300, 64), (5, 3, 1, 100, 32)])
def test_run_attn_extend_check(payload, args):
    r = payload.run_attn_extend_check(*args)
    print(f"\nrun_attn_extend_check{args}: {r}")
    assert set(r) == {"max_err", "max_rel"}
    assert r["max_err"] == 0 and 0 <= r["max_rel"] <= REL


@pytest.mark.gpu
def test_run_attn_extend_timed(payload):
    r = payload.run_attn_extend(9, 8, 2, 512, 100, 64, iters=2, ragged=True)
    print(f"\nrun_attn_extend 9 8 2 512 100 64 ragged: {r}")
    assert set(r) == {"batch", "hq", "hkv", "len", "new", "page", "iters", "ragged",
                      "items", "tflops", "tok_per_s", "max_rel"}
    assert 0 <= r["max_rel"] <= REL and r["items"] >= 9
    for rate in ("tflops", "tok_per_s"):
        assert np.isfinite(r[rate]) and r[rate] > 0


@pytest.mark.gpu
def test_binary_and_serve_extend():
    out = subprocess.run([BIN, "extend", "3", "8", "2", "500", "70", "128", "2", "1"],
                         capture_output=True, text=True, timeout=120)
    res = json.loads(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert set(res) == set(report())
    assert res["ok"] is True and res["cmd"] == "extend" and res["ragged"] is True
    assert (res["new"], res["page"], res["iters"]) == (70, 128, 2)
    assert verify.judge_extend(res, "spx-8x288")["failed"] == []
    out = subprocess.run([BIN, "serve"], input="extend\nquit\n", capture_output=True,
                         text=True, timeout=60)
    rep, quit_ = [json.loads(ln) for ln in out.stdout.splitlines()]
    assert rep["ok"] is True and rep["cmd"] == "extend" and rep["page"] == 64
    assert rep["max_err"] == 0 and 0 <= rep["max_rel"] <= REL
    assert quit_ == {"ok": True}


@pytest.mark.gpu
def test_run_extend_judges_the_real_partition():
    v = verify.run_extend("spx-8x288")
    print(f"\nrun_extend(spx-8x288): {v}")
    assert v["ok"] is True and v["failed"] == [] and v["profile"] == "spx-8x288"
    rep = v["report"]
    assert tuple(rep[f] for f in ("batch", "hq", "hkv", "len", "new", "page", "iters")) \
        == (8, 64, 8, 4096, 1024, 64, 10)
    assert rep["max_err"] == 0 and 0 <= rep["max_rel"] <= REL and rep["tflops"] > 0
