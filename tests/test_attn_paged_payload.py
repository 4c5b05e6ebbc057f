"""The paged, ragged-batch decode attention payload
(ops/csrc/payload_attn_paged.hpp): the plan, the argument checks and the judge
on CPU; the kernels, their bindings, the binary's `paged` verb, `serve` and
`verify.run_paged` on a real MI355X.

The reference is numpy fp64 from the definition, on the dense tensors that the
pool was scattered from:

    o[b,h,:] = softmax_t(scale * q[b,h,:] . k[b,g,t,:]) . v[b,g,t,:], t < len[b]

exact     the selection pattern of attn_check_pattern: tolerance 0.
bounded   general data: |o - ref| <= 2^-8 max |v| (each softmax weight rounded
          to bf16 is off by at most 2^-9 relative, the normaliser is summed
          from the unrounded weights; the bound doubles that). It does not
          depend on how the keys are split.
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
LENS = [1, 33, 64, 300]
SHAPES = [(page, hq, hkv) for page in (32, 64)
          for hq, hkv in ((2, 2), (8, 2), (16, 1))]


@pytest.fixture(scope="module")
def payload():
    from instaslice_amd.ops import _payload

    return _payload


def scatter(k, v, lens, page, seed, spare=3):
    """Dense (B, Hkv, L, 128) K and V into a pool under a seeded permutation
    table. Pages no entry names are NaN, table entries above a length are -1,
    stale keys of the last read 32-key chunk are 1e30, and what lies beyond
    that chunk in its page is NaN."""
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


def ref_attn(q, k, v, lens):
    B, Hq, _ = q.shape
    G = Hq // k.shape[1]
    out = np.empty((B, Hq, D))
    for b, n in enumerate(lens):
        for h in range(Hq):
            s = k[b, h // G, :n].astype(np.float64) @ q[b, h].astype(np.float64)
            w = np.exp((s - s.max()) / np.sqrt(128.0))
            out[b, h] = (w @ v[b, h // G, :n].astype(np.float64)) / w.sum()
    return out


def bf16_round(payload, x):
    bits = payload.to_bf16(np.ascontiguousarray(x, dtype=np.float32))
    return (bits.astype(np.uint32) << 16).view(np.float32)


# ---- CPU ------------------------------------------------------------------

@pytest.mark.parametrize("lens,target", [
    ([1], 1), ([300], 4), (LENS, 1), (LENS, 16), ([32768] + [100] * 31, 16),
    ([4096] * 32, 16), ([33] * 300, 7), ([1, 2 ** 28], 4096)])
def test_plan_covers_every_chunk_once(payload, lens, target):
    items, seq = payload.attn_paged_plan(lens, target)
    assert items.dtype == np.int32 and seq.shape == (len(lens), 2)
    assert 1 <= len(items) <= target + len(lens)
    assert (items[:, 1] < items[:, 2]).all()
    at = 0
    for b, n in enumerate(lens):
        mine = items[items[:, 0] == b]
        assert tuple(seq[b]) == (4 * at, 4 * len(mine))
        assert np.array_equal(items[at:at + len(mine)], mine)  # in order of b
        assert mine[0, 1] == 0 and mine[-1, 2] == -(-n // 32)
        assert np.array_equal(mine[1:, 1], mine[:-1, 2])
        sizes = mine[:, 2] - mine[:, 1]
        assert sizes.max() - sizes.min() <= 1
        at += len(mine)
    # the budget: no item is longer than ceil(C / target) chunks
    chunks = sum(-(-n // 32) for n in lens)
    assert (items[:, 2] - items[:, 1]).max() <= -(-chunks // target)


def test_rejects_bad_arguments(payload):
    q = np.ones((2, 2, D), np.float32)
    kp = np.ones((4, 1, 64, D), np.float32)
    table = np.array([[0, 1], [2, 3]], np.int32)
    lens = [100, 64]
    ok = (q, kp, kp, table, lens)

    def bad(exc, i=None, value=None, **kw):
        args = list(ok)
        if i is not None:
            args[i] = value
        with pytest.raises(exc):
            payload.attn_paged_decode(*args, **kw)

    bad(ValueError, 0, q[0])                                  # ranks
    bad(ValueError, 1, kp[0])
    bad(ValueError, 3, table[0])
    bad(ValueError, 4, [lens])
    bad(ValueError, 4, [100])                                 # lens not (B,)
    bad(ValueError, 0, np.ones((2, 17, D), np.float32))       # Hq / Hkv = 17
    bad(ValueError, 0, np.ones((2, 2, 64), np.float32))       # head dim
    bad(ValueError, 2, np.ones((4, 1, 32, D), np.float32))    # k / v mismatch
    bad(ValueError, 4, [0, 64])                               # lengths
    bad(ValueError, 4, [129, 64])
    bad(ValueError, 3, np.array([[0, -1], [2, 3]]))           # needed entries
    bad(ValueError, 3, np.array([[0, 4], [2, 3]]))
    bad(TypeError, 3, table.astype(np.float32))
    bad(TypeError, 4, [100.0, 64.0])
    bad(ValueError, workgroups=-1)
    bad(ValueError, workgroups=4097)
    bad(ValueError, scale=float("inf"))
    nan = kp.copy()
    nan[1, 0, 63, 5] = np.nan                                 # key 127 < 128 read
    bad(ValueError, 1, nan)
    k48 = np.ones((4, 1, 48, D), np.float32)                  # a page of 48
    with pytest.raises(ValueError):
        payload.attn_paged_decode(q, k48, k48, table, [48, 48])
    for args in ((2, 8, 2, 100, 48), (2, 17, 1, 100, 64), (2, 8, 2, 0, 64)):
        with pytest.raises(ValueError):
            payload.run_attn_paged_check(*args)
        with pytest.raises(ValueError):
            payload.run_attn_paged(*args)
    with pytest.raises(ValueError):
        payload.run_attn_paged(2, 8, 2, 100, 64, iters=0)
    for lens_, target in (([0], 4), ([5], 0), ([5], 4097)):
        with pytest.raises(ValueError):
            payload.attn_paged_plan(lens_, target)
    with pytest.raises(TypeError):
        payload.attn_paged_plan([5.0], 4)


def test_accepts_a_table_out_of_range_above_the_length(payload):
    # everything is checked and accepted; without a device the first HIP call
    # then fails, with one it runs
    q = np.ones((2, 2, D), np.float32)
    kp = np.ones((4, 1, 64, D), np.float32)
    kp[3] = np.nan                                            # page 3: not named
    kp[1, 0, 32:] = np.nan                                    # beyond the last read chunk
    table = np.array([[0, 99], [1, -1]], np.int32)
    try:
        out = payload.attn_paged_decode(q, kp, kp, table, [64, 20])
    except RuntimeError as e:
        assert "HIP error" in str(e)
    else:
        assert np.array_equal(out, np.ones((2, 2, D), np.float32))


def report(**over):
    r = {"ok": True, "cmd": "paged", "batch": 32, "hq": 64, "hkv": 8, "len": 4096,
         "page": 64, "iters": 10, "items": 32, "kv_gb_per_s": 3400.1,
         "steps_per_s": 6333.3, "tok_per_s": 202665.6, "max_err": 0,
         "max_rel": 0.000275}
    r.update(over)
    return r


@pytest.mark.parametrize("over,ok", [
    ({}, True), ({"ok": False, "kv_gb_per_s": 0.0}, True), ({"page": 256}, True),
    ({"max_rel": 2.0 ** -8}, True),
    ({"max_err": 1e-30}, False), ({"max_err": None}, False),
    ({"max_rel": float(np.nextafter(2.0 ** -8, 1.0))}, False),
    ({"max_rel": float("nan")}, False),
    ({"page": 48}, False), ({"page": 64.0}, False), ({"page": None}, False),
    ({"items": 0}, False), ({"items": 1.5}, False), ({"batch": 0}, False)])
def test_judge_paged(over, ok):
    v = verify.judge_paged(report(**over), "cpx-1x36")
    assert v["ok"] is ok and v["failed"] == ([] if ok else ["paged"])
    with pytest.raises(ValueError):
        verify.judge_paged(report(), "not-a-profile")


def test_cli_paged(monkeypatch, capsys):
    from instaslice_amd.cli import main
    from types import SimpleNamespace

    seen = []

    def runner(cmd, **kw):
        seen.append(cmd)
        return SimpleNamespace(stdout=json.dumps(report()), stderr="", returncode=0)

    real = verify.run_paged
    monkeypatch.setattr(verify, "run_paged",
                        lambda profile, **kw: real(profile, runner=runner, **kw))
    rc = main(["paged", "--profile", "cpx-1x36"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 0 and out["ok"] is True and seen == [[verify.BIN_PATH, "paged"]]


# ---- GPU: the kernels against the closed form and fp64 -----------------------

@pytest.mark.gpu
@pytest.mark.parametrize("workgroups", [1, 16])
@pytest.mark.parametrize("page,hq,hkv", SHAPES)
def test_pattern_exact(payload, page, hq, hkv, workgroups):
    q, k, v, expected = payload.attn_check_pattern(len(LENS), hq, hkv, max(LENS),
                                                   lengths=LENS)
    kp, vp, table = scatter(k, v, LENS, page, seed=page + hq)
    out = payload.attn_paged_decode(q, kp, vp, table, LENS, workgroups=workgroups)
    assert out.dtype == np.float32 and np.isfinite(out).all()
    assert np.array_equal(out, expected)


@pytest.fixture(scope="module")
def dense(payload):
    """(q, k, v, fp64 reference) per head shape, computed once"""
    made = {}
    for hq, hkv in {(hq, hkv) for _, hq, hkv in SHAPES}:
        rng = np.random.default_rng(100 * hq + hkv)
        q = bf16_round(payload, 4 * rng.standard_normal((len(LENS), hq, D)))
        k = bf16_round(payload, rng.standard_normal((len(LENS), hkv, max(LENS), D)))
        v = bf16_round(payload, rng.uniform(-1, 1, k.shape))
        made[hq, hkv] = (q, k, v, ref_attn(q, k, v, LENS))
    return made


@pytest.mark.gpu
@pytest.mark.parametrize("workgroups", [1, 16])
@pytest.mark.parametrize("page,hq,hkv", SHAPES)
def test_dense_bounded_and_deterministic(payload, dense, page, hq, hkv, workgroups):
    q, k, v, ref = dense[hq, hkv]
    kp, vp, table = scatter(k, v, LENS, page, seed=7 * page + hq)
    out = payload.attn_paged_decode(q, kp, vp, table, LENS, workgroups=workgroups)
    err = np.abs(out.astype(np.float64) - ref).max() / np.abs(v).max()
    print(f"\npage {page} ({hq},{hkv}) workgroups {workgroups}: max_rel {err:.3e}")
    assert np.isfinite(out).all() and err <= REL
    again = payload.attn_paged_decode(q, kp, vp, table, LENS, workgroups=workgroups)
    assert np.array_equal(out.view(np.uint32), again.view(np.uint32))


@pytest.mark.gpu
def test_prefix_sharing(payload, dense):
    q, k, v, _ = dense[8, 2]
    q, k, v, lens = q[:2], k[:2].copy(), v[:2].copy(), [200, 300]
    k[1, :, :128], v[1, :, :128] = k[0, :, :128], v[0, :, :128]   # a common prefix
    kp, vp, table = scatter(k, v, lens, 64, seed=5)
    kp[table[1, :2]] = vp[table[1, :2]] = np.nan   # its own copy of the prefix goes
    table[1, :2] = table[0, :2]
    out = payload.attn_paged_decode(q, kp, vp, table, lens, workgroups=4)
    err = np.abs(out - ref_attn(q, k, v, lens)).max(axis=(1, 2)) / np.abs(v).max()
    print(f"\nprefix sharing: max_rel per sequence {err}")
    assert np.isfinite(out).all() and (err <= REL).all()


@pytest.mark.gpu
def test_bf16_and_fp8_caches_agree_on_the_same_values(payload):
    """The two paged kernels run the same chunk step, each in its own body, so
    on the same real numbers (e4m3 codes under scales of 1, and the decoded
    codes as bf16 pages) they may differ only through how the keys are grouped.
    With lengths that are multiples of 64 and one work item per sequence both
    plans cut the same key ranges, but a wave takes 32-key chunks round-robin
    in one kernel and 64-key chunks in the other, so the partials differ and
    bit-equality of the merged result cannot be had: on random data a weight is
    rounded to bf16 under one running maximum here and another there, and the
    two results are 2e-4 max |v| apart (measured, on the unfolded kernels too).

    So the data takes the weights' rounding out. K holds the codes of the
    integers -4 .. 4, every q row is +-1 at two places, and scale is float32
    ln 2, for which scale * log2(e) is exactly 1 in fp32: every score, every
    running maximum and every difference of the two is an integer, every weight
    an exact power of two that bf16 holds, alpha and the merge weights too. V
    draws from all non-negative non-NaN codes, so no sum cancels. What is left
    are the fp32 roundings of non-negative sums taken in another order: per
    result at most two chunk accumulations per wave, four merge terms and one
    division, for o and for l. Counting the MFMA's inner sum as up to four
    roundings that is below 16 half-ulps twice over, so the two results are
    asserted within 16 ulps of each other, element by element, and each within
    2^-8 max |v| of fp64. A wrong key index, l update, guard or rescale in
    either body moves a result by whole weights, not ulps."""
    lens, hq, hkv, page = [64, 128, 192], 4, 2, 64
    for chunk in (32, 64):
        items, _ = payload.attn_paged_plan(lens, 1, chunk)
        keys = [(b, c0 * chunk, c1 * chunk) for b, c0, c1 in items.tolist()]
        assert keys == [(b, 0, n) for b, n in enumerate(lens)]
    rng = np.random.default_rng(8)
    small = payload.to_e4m3(np.arange(-4, 5, dtype=np.float32))
    W = max(lens) // page
    P = len(lens) * W
    table = rng.permutation(P).reshape(len(lens), W).astype(np.int32)
    kc = rng.choice(small, (P, hkv, page, D))
    vc = rng.integers(0, 0x7F, (P, hkv, page, D), dtype=np.uint8)
    k, v = payload.from_e4m3(kc), payload.from_e4m3(vc)
    assert np.array_equal(k, np.rint(k)) and np.abs(k).max() == 4 and v.min() == 0
    q = np.zeros((len(lens), hq, D), np.float32)
    for row in q.reshape(-1, D):
        row[rng.choice(D, 2, replace=False)] = rng.choice([-1.0, 1.0], 2)
    one = np.ones(hkv, np.float32)
    ln2 = float(np.float32(np.log(2.0)))
    assert np.float32(ln2) * np.float32(1.4426950408889634) == np.float32(1.0)
    a = payload.attn_paged_decode(q, k, v, table, lens, scale=ln2, workgroups=1)
    b = payload.attn_paged_decode_fp8(q, kc, vc, one, one, table, lens, scale=ln2,
                                      workgroups=1)
    ref = np.empty(a.shape)
    n_eff = []
    for i, n in enumerate(lens):
        kd, vd = (x[table[i]].transpose(1, 0, 2, 3).reshape(hkv, W * page, D)[:, :n]
                  .astype(np.float64) for x in (k, v))
        for h in range(hq):
            sc = kd[h // (hq // hkv)] @ q[i, h].astype(np.float64)
            w = np.exp2(sc - sc.max())
            ref[i, h] = (w @ vd[h // (hq // hkv)]) / w.sum()
            n_eff.append(w.sum() ** 2 / (w * w).sum())
    vmax = np.abs(v).max()
    err_a, err_b = (np.abs(x.astype(np.float64) - ref).max() / vmax for x in (a, b))
    ulps = np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))
    print(f"\nbf16 {err_a:.3e} fp8 {err_b:.3e} apart {ulps.max():.1f} ulps, keys with "
          f"weight {min(n_eff):.1f} .. {max(n_eff):.1f}, "
          f"bit-identical {np.array_equal(a.view(np.uint32), b.view(np.uint32))}")
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert err_a <= REL and err_b <= REL
    assert ulps.max() <= 16


# ---- GPU: the self-check, the timed run, the binary, serve, the runner -------

@pytest.mark.gpu
@pytest.mark.parametrize("args", [(4, 8, 2, 300, 64, 0), (5, 16, 1, 257, 128, 3),
                                  (4, 6, 2, 40, 256, 1), (4, 4, 4, 100, 32, 64)])
def test_run_attn_paged_check(payload, args):
    r = payload.run_attn_paged_check(*args)
    print(f"\nrun_attn_paged_check{args}: {r}")
    assert set(r) == {"max_err", "max_rel"}
    assert r["max_err"] == 0 and 0 <= r["max_rel"] <= REL


@pytest.mark.gpu
@pytest.mark.parametrize("ragged", [False, True])
def test_run_attn_paged_timed(payload, ragged):
    r = payload.run_attn_paged(9, 8, 2, 512, 64, iters=2, ragged=ragged)
    print(f"\nrun_attn_paged 9 8 2 512 ragged={ragged}: {r}")
    assert set(r) == {"batch", "hq", "hkv", "len", "page", "iters", "ragged", "items",
                      "kv_gb_per_s", "steps_per_s", "tok_per_s", "max_err"}
    assert r["max_err"] == 0 and r["items"] >= 9 and r["kv_gb_per_s"] > 0
    assert r["tok_per_s"] == pytest.approx(9 * r["steps_per_s"])


@pytest.mark.gpu
def test_binary_and_serve_paged():
    out = subprocess.run([BIN, "paged", "3", "8", "2", "500", "128", "2"],
                         capture_output=True, text=True, timeout=120)
    res = json.loads(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert set(res) == {"ok", "cmd", "batch", "hq", "hkv", "len", "page", "iters",
                        "items", "kv_gb_per_s", "steps_per_s", "tok_per_s", "max_err",
                        "max_rel"}
    assert res["ok"] is True and res["cmd"] == "paged" and res["page"] == 128
    assert res["max_err"] == 0 and 0 <= res["max_rel"] <= REL and res["items"] >= 3
    out = subprocess.run([BIN, "serve"], input="paged\npaged 5 4 2 70 32\nquit\n",
                         capture_output=True, text=True, timeout=60)
    first, second, quit_ = [json.loads(ln) for ln in out.stdout.splitlines()]
    for rep, shape in ((first, (4, 8, 2, 300, 64)), (second, (5, 4, 2, 70, 32))):
        assert rep["ok"] is True and rep["cmd"] == "paged"
        assert rep["max_err"] == 0 and 0 <= rep["max_rel"] <= REL
        assert tuple(rep[f] for f in ("batch", "hq", "hkv", "len", "page")) == shape
    assert quit_ == {"ok": True}


@pytest.mark.gpu
def test_run_paged_judges_the_real_partition():
    v = verify.run_paged("spx-8x288")
    print(f"\nrun_paged(spx-8x288): {v}")
    assert v["ok"] is True and v["failed"] == [] and v["profile"] == "spx-8x288"
    rep = v["report"]
    assert tuple(rep[f] for f in ("batch", "hq", "hkv", "len", "page", "iters")) == \
        (32, 64, 8, 4096, 64, 10)
    assert rep["max_err"] == 0 and 0 <= rep["max_rel"] <= REL and rep["items"] >= 32
