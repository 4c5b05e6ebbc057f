"""The FP8 KV-cache variant of the paged decode attention payload
(ops/csrc/payload_attn_fp8.hpp): the 64-key plan, the argument checks and the
judge on CPU; the kernel, its bindings, the binary's `paged8` verb, `serve` and
`verify.run_paged8` on a real MI355X.

The reference is numpy fp64 from the definition on the dequantised cache,
K' = from_e4m3(k_codes) * k_scale[g] and V' likewise:

    o[b,h,:] = softmax_t(q[b,h,:] . K'[b,g,t,:] / sqrt(128)) . V'[b,g,t,:], t < len[b]

exact     the e4m3 selection pattern of run_attn_paged_fp8_check: tolerance 0.
bounded   |o - ref| <= 2^-8 max |V'|: widening e4m3 to bf16 is exact, so the
          roundings are the bf16 kernel's (each softmax weight rounded to bf16
          is off by at most 2^-9 relative, the normaliser is summed from the
          unrounded weights; the bound doubles that).
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
# one key; an empty second 32-key k-step; one short of, at and one past the
# 64-key chunk; a page boundary at both page sizes; several chunks per wave
LENS = [1, 33, 63, 64, 65, 129, 300]
SHAPES = [(page, hq, hkv) for page in (64, 128)
          for hq, hkv in ((2, 2), (8, 2), (16, 1))]
CODES = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)  # no NaN
K_SCALE, V_SCALE = 2.0 ** -9, 2.0 ** -3


@pytest.fixture(scope="module")
def payload():
    from instaslice_amd.ops import _payload

    return _payload


def scatter(kc, vc, lens, page, seed, spare=3):
    """Dense (B, Hkv, L, 128) codes into pools under a seeded permutation
    table. Pages no needed entry names and chunks beyond the last read one are
    NaN codes (0x7F), table entries above a length are -1, stale keys of the
    last read 64-key chunk are 448 (0x7E)."""
    B, Hkv, L, _ = kc.shape
    W = -(-L // page)
    P = B * W + spare
    table = np.random.default_rng(seed).permutation(P)[:B * W].reshape(B, W)
    table = table.astype(np.int32)
    kp = np.full((P, Hkv, page, D), 0x7F, np.uint8)
    vp = kp.copy()
    for b, n in enumerate(lens):
        table[b, -(-n // page):] = -1
        for t in range(-(-n // 64) * 64):
            kp[table[b, t // page], :, t % page] = kc[b, :, t] if t < n else 0x7E
            vp[table[b, t // page], :, t % page] = vc[b, :, t] if t < n else 0x7E
    return kp, vp, table


def ref_attn(payload, q, kc, vc, ks, vs, lens):
    B, Hq, _ = q.shape
    G = Hq // kc.shape[1]
    k = payload.from_e4m3(kc).astype(np.float64) * ks[None, :, None, None]
    v = payload.from_e4m3(vc).astype(np.float64) * vs[None, :, None, None]
    out = np.empty((B, Hq, D))
    for b, n in enumerate(lens):
        for h in range(Hq):
            s = k[b, h // G, :n] @ q[b, h].astype(np.float64)
            w = np.exp((s - s.max()) / np.sqrt(128.0))
            out[b, h] = (w @ v[b, h // G, :n]) / w.sum()
    return out, np.abs(v).max()


# ---- CPU ------------------------------------------------------------------

@pytest.mark.parametrize("lens,target", [
    ([1], 1), ([63, 64, 65, 129, 300], 1), ([63, 64, 65, 129, 300], 4),
    ([32768] + [100] * 31, 16)])
def test_plan_in_64_key_chunks(payload, lens, target):
    items, seq = payload.attn_paged_plan(lens, target, chunk=64)
    assert 1 <= len(items) <= target + len(lens)
    at = 0
    for b, n in enumerate(lens):
        mine = items[items[:, 0] == b]
        assert tuple(seq[b]) == (4 * at, 4 * len(mine))
        assert np.array_equal(items[at:at + len(mine)], mine)  # in order of b
        assert mine[0, 1] == 0 and mine[-1, 2] == -(-n // 64)
        assert np.array_equal(mine[1:, 1], mine[:-1, 2])
        sizes = mine[:, 2] - mine[:, 1]
        assert sizes.min() >= 1 and sizes.max() - sizes.min() <= 1
        at += len(mine)


def test_plan_default_chunk_is_32(payload):
    lens = [1, 33, 64, 300, 32768]
    for a, b in zip(payload.attn_paged_plan(lens, 16),
                    payload.attn_paged_plan(lens, 16, chunk=32)):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        payload.attn_paged_plan(lens, 16, chunk=48)


def test_rejects_bad_arguments(payload):
    q = np.ones((2, 2, D), np.float32)
    kp = np.full((4, 1, 64, D), 0x38, np.uint8)               # 1.0
    one = np.ones(1, np.float32)
    table = np.array([[0, 1], [2, 3]], np.int32)
    ok = [q, kp, kp, one, one, table, [100, 64]]

    def bad(exc, i, value):
        args = list(ok)
        args[i] = value
        with pytest.raises(exc):
            payload.attn_paged_decode_fp8(*args)

    bad(TypeError, 1, kp.astype(np.float32))                  # float pools
    bad(TypeError, 2, kp.astype(np.float32))
    bad(ValueError, 2, kp[:3])                                # k / v extents
    bad(ValueError, 3, np.ones(2, np.float32))                # scales
    for s in (0.0, -1.0, np.nan, np.inf):
        bad(ValueError, 3, np.full(1, s, np.float32))
        bad(ValueError, 4, np.full(1, s, np.float32))
    bad(ValueError, 6, [0, 64])                               # lengths
    bad(ValueError, 6, [129, 64])
    bad(ValueError, 5, np.array([[0, -1], [2, 3]]))           # needed entries
    bad(ValueError, 5, np.array([[0, 4], [2, 3]]))
    nan = kp.copy()
    nan[1, 0, 35, 5] = 0xFF                                   # key 99 < 100
    bad(ValueError, 1, nan)
    nan = kp.copy()
    nan[1, 0, 63, 5] = 0x7F                                   # stale, chunk read
    bad(ValueError, 2, nan)
    k32 = np.full((4, 1, 32, D), 0x38, np.uint8)              # a page of 32
    with pytest.raises(ValueError):
        payload.attn_paged_decode_fp8(q, k32, k32, one, one, table, [32, 32])
    with pytest.raises(ValueError):
        payload.run_attn_paged_fp8_check(2, 8, 2, 100, 32)


def report(**over):
    r = {"ok": True, "cmd": "paged8", "batch": 32, "hq": 64, "hkv": 8, "len": 4096,
         "page": 64, "iters": 10, "items": 32, "us": 60.0, "bf16_us": 99.2,
         "kv_gb_per_s": 4400.1, "steps_per_s": 16666.6, "tok_per_s": 533333.3,
         "quant_rel": 0.02, "max_err": 0, "max_rel": 0.000275}
    r.update(over)
    return r


@pytest.mark.parametrize("over,ok", [
    ({}, True), ({"quant_rel": 0.5}, True), ({"max_rel": 2.0 ** -8}, True),
    ({"max_err": 1e-30}, False),
    ({"max_rel": float(np.nextafter(2.0 ** -8, 1.0))}, False),
    ({"max_rel": None}, False), ({"page": 32}, False)])
def test_judge_paged8(over, ok):
    v = verify.judge_paged8(report(**over), "cpx-1x36")
    assert v["ok"] is ok and v["failed"] == ([] if ok else ["paged8"])
    missing = report()
    del missing["max_err"]
    assert verify.judge_paged8(missing, "cpx-1x36")["failed"] == ["paged8"]


# ---- GPU ------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("workgroups", [1, 16])
@pytest.mark.parametrize("page,hq,hkv", SHAPES)
def test_pattern_exact(payload, page, hq, hkv, workgroups):
    r = payload.run_attn_paged_fp8_check(8, hq, hkv, 300, page, workgroups, ragged=True)
    print(f"\npage {page} ({hq},{hkv}) workgroups {workgroups}: {r}")
    assert r["max_err"] == 0 and 0 <= r["max_rel"] <= REL


@pytest.fixture(scope="module")
def dense(payload):
    """(q, k codes, v codes, scales, fp64 reference, max |V'|) per head shape,
    computed once: q ~ N(0, 1) rounded to bf16, codes uniform over the 254
    non-NaN bytes, so the scores have a standard deviation near 0.2"""
    made = {}
    for hq, hkv in {(hq, hkv) for _, hq, hkv in SHAPES}:
        rng = np.random.default_rng(100 * hq + hkv)
        q = rng.standard_normal((len(LENS), hq, D)).astype(np.float32)
        q = (payload.to_bf16(q).astype(np.uint32) << 16).view(np.float32)
        kc = rng.choice(CODES, (len(LENS), hkv, max(LENS), D))
        vc = rng.choice(CODES, kc.shape)
        ks = np.full(hkv, K_SCALE, np.float32)
        vs = np.full(hkv, V_SCALE, np.float32)
        made[hq, hkv] = (q, kc, vc, ks, vs, *ref_attn(payload, q, kc, vc, ks, vs, LENS))
    return made


@pytest.mark.gpu
@pytest.mark.parametrize("workgroups", [1, 16])
@pytest.mark.parametrize("page,hq,hkv", SHAPES)
def test_dense_bounded(payload, dense, page, hq, hkv, workgroups):
    q, kc, vc, ks, vs, ref, vmax = dense[hq, hkv]
    kp, vp, table = scatter(kc, vc, LENS, page, seed=7 * page + hq)
    out = payload.attn_paged_decode_fp8(q, kp, vp, ks, vs, table, LENS,
                                        workgroups=workgroups)
    err = np.abs(out.astype(np.float64) - ref).max() / vmax
    print(f"\npage {page} ({hq},{hkv}) workgroups {workgroups}: max_rel {err:.3e}")
    assert out.dtype == np.float32 and np.isfinite(out).all() and err <= REL


@pytest.mark.gpu
def test_prefix_sharing(payload, dense):
    q, kc, vc, ks, vs, _, _ = dense[8, 2]
    q, kc, vc, lens = q[[0, 0]], kc[[0, 0]], vc[[0, 0]], [64, 64]
    ref, vmax = ref_attn(payload, q, kc, vc, ks, vs, lens)
    kp, vp, table = scatter(kc[:, :, :64], vc[:, :, :64], lens, 64, seed=5)
    kp[table[1, 0]] = vp[table[1, 0]] = 0x7F       # its own copy of the page goes
    table[1, 0] = table[0, 0]
    out = payload.attn_paged_decode_fp8(q, kp, vp, ks, vs, table, lens, workgroups=4)
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
    assert np.isfinite(out).all() and np.abs(out - ref).max() <= REL * vmax


@pytest.mark.gpu
def test_binary_and_serve_paged8():
    out = subprocess.run([BIN, "paged8", "3", "8", "2", "500", "128", "2"],
                         capture_output=True, text=True, timeout=120)
    res = json.loads(out.stdout)
    print(f"\npaged8 3 8 2 500 128 2: {res}")
    assert out.returncode == 0, out.stdout + out.stderr
    assert res["cmd"] == "paged8" and res["page"] == 128 and res["bf16_us"] > 0
    assert verify.judge_paged8(res, "spx-8x288")["failed"] == []
    out = subprocess.run([BIN, "serve"], input="paged8 5 4 2 70 64\nquit\n",
                         capture_output=True, text=True, timeout=60)
    rep, quit_ = [json.loads(ln) for ln in out.stdout.splitlines()]
    assert rep["ok"] is True and rep["cmd"] == "paged8" and rep["page"] == 64
    assert rep["max_err"] == 0 and 0 <= rep["max_rel"] <= REL
    assert quit_ == {"ok": True}


@pytest.mark.gpu
def test_run_paged8_judges_the_real_partition():
    v = verify.run_paged8("spx-8x288")
    print(f"\nrun_paged8(spx-8x288): {v}")
    assert v["ok"] is True and "paged8" not in v["failed"]
    rep = v["report"]
    assert rep["max_err"] == 0 and 0 <= rep["max_rel"] <= REL and rep["items"] >= 32
