"""The KV-cache decode attention payload (ops/csrc/payload_attn.hpp): the check
pattern, argument checks, the judge, the runner and the CLI on CPU; the
kernel, its bindings, the binary's `attn` verb, the `serve` verb and
`verify.run_attn` on a real MI355X.

The reference is written here in numpy fp64 from the definition,
independently of the header:

    o[b,h,:] = softmax_t(scale * q[b,h,:] . k[b,g,t,:]) . v[b,g,t,:], t < len[b]
    with g = h // (Hq // Hkv)

Two kinds of comparison:

  exact      the selection pattern: K is 0 at n = min(32, largest power of two
             <= len) keys and <= -16 elsewhere, q >= 2, so a selected score is
             exactly 0 and any other is <= -4096 scale (about -362), whose
             weight is exactly 0 in fp32. The result is the mean of at most 32
             integers in [-4, 4] over a power of two: bit-exact in any order
             and for any split count. Tolerance 0.
  bounded    general data: |o - ref| <= 2^-8 max |v|. The kernel rounds each
             softmax weight to bf16 (at most 2^-9 relative) and sums the
             normaliser from the unrounded weights, so the output is off by
             at most 2^-9 max |v| plus fp32 terms of order 1e-6; the bound
             doubles that. max |v| is taken over the keys that take part.
"""

import json
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from instaslice_amd.ops import verify

BIN = os.path.join(os.path.dirname(__file__), "..", "instaslice_amd", "bin",
                   "instaslice-payload")
D = 128
REL = 2.0 ** -8


@pytest.fixture(scope="module")
def payload():
    from instaslice_amd.ops import _payload

    return _payload


# ---- the numpy reference --------------------------------------------------

def ref_attn(q, k, v, lengths=None, scale=None):
    """fp64 softmax attention from the definition."""
    B, Hq, _ = q.shape
    Hkv, L = k.shape[1], k.shape[2]
    G = Hq // Hkv
    scale = 1.0 / np.sqrt(np.float64(D)) if scale is None else np.float64(scale)
    out = np.empty((B, Hq, D), dtype=np.float64)
    for b in range(B):
        n = L if lengths is None else int(lengths[b])
        for h in range(Hq):
            g = h // G
            s = k[b, g, :n].astype(np.float64) @ q[b, h].astype(np.float64) * scale
            w = np.exp(s - s.max())
            out[b, h] = (w @ v[b, g, :n].astype(np.float64)) / w.sum()
    return out


def bf16_round(payload, x):
    """x rounded to bf16 (the payload's own host rounding), back as float32."""
    bits = payload.to_bf16(np.ascontiguousarray(x, dtype=np.float32))
    return (bits.astype(np.uint32) << 16).view(np.float32)


def sel_count(n):
    c = 1
    while c * 2 <= n and c < 32:
        c *= 2
    return c


# (batch, hq, hkv, length, lengths)
PATTERN_SHAPES = [
    (2, 8, 2, 100, None),
    (1, 16, 1, 257, None),
    (1, 6, 2, 64, None),
    (1, 1, 1, 33, None),
    (1, 4, 4, 1, None),
    (3, 4, 4, 64, [1, 2, 64]),
]


# ---- CPU: attn_check_pattern ----------------------------------------------

@pytest.mark.parametrize("B,Hq,Hkv,L,lengths", PATTERN_SHAPES)
def test_check_pattern(payload, B, Hq, Hkv, L, lengths):
    q, k, v, expected = payload.attn_check_pattern(B, Hq, Hkv, L, lengths=lengths)
    assert q.shape == (B, Hq, D) and expected.shape == (B, Hq, D)
    assert k.shape == (B, Hkv, L, D) and v.shape == (B, Hkv, L, D)
    for a in (q, k, v, expected):
        assert a.dtype == np.float32
    # every input is exact in bf16
    for a in (q, k, v):
        assert np.array_equal(bf16_round(payload, a), a)
    assert q.min() >= 2 and np.abs(v).max() <= 4

    G = Hq // Hkv
    scale = 1.0 / np.sqrt(128.0)
    for b in range(B):
        n = L if lengths is None else lengths[b]
        for g in range(Hkv):
            sel = np.flatnonzero((k[b, g, :n] == 0).all(axis=1))
            # distinct by construction of flatnonzero, below len, the right count
            assert len(sel) == sel_count(n) and (sel < n).all()
            i = np.arange(sel_count(n))
            want = np.sort((i * n // sel_count(n) + b + g) % n)
            assert np.array_equal(sel, want) and len(np.unique(want)) == len(want)
            others = np.setdiff1d(np.arange(n), sel)
            for h in range(g * G, (g + 1) * G):
                s = k[b, g, :n].astype(np.float64) @ q[b, h].astype(np.float64) * scale
                assert (s[sel] == 0).all()
                if len(others):
                    assert s[others].max() <= -300
    # the closed form is the fp64 softmax, bit for bit
    ref = ref_attn(q, k, v, lengths).astype(np.float32)
    assert np.array_equal(expected, ref)


def test_check_pattern_rejects_bad_arguments(payload):
    for args in [(0, 4, 4, 8), (1, 0, 1, 8), (1, 4, 0, 8), (1, 4, 4, 0),
                 (1, 3, 2, 8), (1, 17, 1, 8)]:
        with pytest.raises(ValueError):
            payload.attn_check_pattern(*args)
    for lengths in ([0, 1], [1, 9], [1], [[1, 1]]):
        with pytest.raises(ValueError):
            payload.attn_check_pattern(2, 4, 4, 8, lengths=lengths)


# ---- CPU: attn_decode argument checks (raised before any HIP call) ----------

def _qkv(B=1, Hq=2, Hkv=1, L=4, d=D):
    return (np.ones((B, Hq, d), np.float32), np.ones((B, Hkv, L, d), np.float32),
            np.ones((B, Hkv, L, d), np.float32))


def test_attn_decode_rejects_bad_arguments(payload):
    q, k, v = _qkv()
    bad = [
        ((q[0], k, v), {}),                                   # q not 3-D
        ((q, k[0], v[0]), {}),                                # k, v not 4-D
        ((q, k[..., None], v[..., None]), {}),                # k, v 5-D
        (_qkv(d=64), {}),                                     # D != 128
        (_qkv(Hq=3, Hkv=2), {}),                              # Hq % Hkv != 0
        (_qkv(Hq=17, Hkv=1), {}),                             # G > 16
        (_qkv(B=0), {}),                                      # empty batch
        (_qkv(L=0), {}),                                      # empty cache
        ((q[:, :0], k, v), {}),                               # no query heads
        ((q, k, v[:, :, :3]), {}),                            # k / v mismatch
        ((q, k, np.ones((1, 1, 4, 64), np.float32)), {}),     # v with D = 64
        ((np.ones((2, 2, D), np.float32), k, v), {}),         # batch mismatch
        ((q, k, v), {"lengths": [1, 1]}),                     # lengths not (B,)
        ((q, k, v), {"lengths": [[4]]}),
        ((q, k, v), {"lengths": [0]}),                        # outside 1 .. L
        ((q, k, v), {"lengths": [5]}),
        ((q, k, v), {"splits": -1}),
        ((q, k, v), {"splits": 65}),
        ((q, k, v), {"scale": float("nan")}),
    ]
    for args, kw in bad:
        with pytest.raises(ValueError):
            payload.attn_decode(*args, **kw)
    for which in range(3):
        for junk in (np.nan, np.inf, -np.inf):
            args = [a.copy() for a in (q, k, v)]
            args[which].flat[-1] = junk
            with pytest.raises(ValueError):
                payload.attn_decode(*args)
    with pytest.raises(ValueError):
        payload.run_attn_check(1, 3, 2, 8)
    with pytest.raises(ValueError):
        payload.run_attn_check(1, 2, 1, 8, splits=65)
    with pytest.raises(ValueError):
        payload.run_attn(1, 17, 1, 8)
    with pytest.raises(ValueError):
        payload.run_attn(1, 2, 1, 8, iters=0)


# too many sequences, too many kv heads, too long a cache
TOO_LARGE_SHAPES = [(70000, 4, 4, 8), (1, 70000 * 16, 70000, 8),
                    (1, 4, 4, 2 ** 28 + 1)]


@pytest.mark.parametrize("shape", TOO_LARGE_SHAPES)
def test_attn_rejects_too_large_shapes(payload, shape):
    # at once: the last shape would otherwise ask for tens of GiB
    with pytest.raises(ValueError):
        payload.attn_check_pattern(*shape)
    with pytest.raises(ValueError):
        payload.run_attn_check(*shape)
    with pytest.raises(ValueError):
        payload.run_attn(*shape)


# ---- CPU: judge_attn --------------------------------------------------------

def report(**over):
    """What the binary prints for a clean default run."""
    r = {"ok": True, "cmd": "attn", "batch": 32, "hq": 64, "hkv": 8,
         "len": 4096, "iters": 10, "kv_gb_per_s": 3456.7, "steps_per_s": 6438.9,
         "tok_per_s": 206044.8, "max_err": 0, "max_rel": 0.000275}
    r.update(over)
    return r


def test_judge_attn_pass():
    rep = report()
    v = verify.judge_attn(rep, "cpx-1x36")
    assert v == {"ok": True, "failed": [], "profile": "cpx-1x36", "report": rep}
    # rates are carried, never judged; the report's own ok is not trusted
    assert verify.judge_attn(report(kv_gb_per_s=0.0, steps_per_s=0.0,
                                    tok_per_s=0.0, ok=False), "cpx-1x36")["ok"]
    assert verify.judge_attn(report(max_err=0.0), "cpx-1x36")["ok"] is True
    assert verify.judge_attn(report(max_rel=0), "cpx-1x36")["ok"] is True
    assert verify.judge_attn(report(max_rel=2.0 ** -8), "cpx-1x36")["ok"] is True
    rep = report()
    for rate in ("kv_gb_per_s", "steps_per_s", "tok_per_s"):
        del rep[rate]
    assert verify.judge_attn(rep, "cpx-1x36")["ok"] is True


def test_judge_attn_non_zero_error():
    for err in (0.0625, 1e-30, 1e300, -1, float("nan")):
        v = verify.judge_attn(report(ok=True, max_err=err), "cpx-1x36")
        assert v["ok"] is False and v["failed"] == ["attn"]


def test_judge_attn_max_rel():
    above = float(np.nextafter(2.0 ** -8, 1.0))
    for rel in (above, 0.1, 1e300, -1e-9, float("nan"), float("inf"),
                "0.001", None, True, False):
        v = verify.judge_attn(report(ok=True, max_rel=rel), "cpx-1x36")
        assert v["ok"] is False and v["failed"] == ["attn"], rel


@pytest.mark.parametrize("field", ["max_err", "max_rel", "batch", "hq", "hkv",
                                   "len", "iters"])
def test_judge_attn_missing_or_non_numeric_field(field):
    rep = report()
    del rep[field]
    assert verify.judge_attn(rep, "cpx-1x36")["failed"] == ["attn"]
    for junk in ("0", None, True, False):
        assert verify.judge_attn(report(**{field: junk}),
                                 "cpx-1x36")["failed"] == ["attn"]


@pytest.mark.parametrize("field", ["batch", "hq", "hkv", "len", "iters"])
def test_judge_attn_counts_must_be_positive_integers(field):
    for junk in (0, -1, 1.0, 4096.5):
        assert verify.judge_attn(report(**{field: junk}),
                                 "cpx-1x36")["failed"] == ["attn"]


def test_judge_attn_unknown_profile():
    with pytest.raises(ValueError):
        verify.judge_attn(report(), "not-a-profile")


# ---- CPU: verify.run_attn with a fake child --------------------------------

def fake_runner(stdout="", returncode=0, raises=None, seen=None):
    def runner(cmd, **kw):
        if seen is not None:
            seen.append((cmd, kw))
        if raises is not None:
            raise raises
        return SimpleNamespace(stdout=stdout, stderr="", returncode=returncode)
    return runner


def test_run_attn_pass():
    seen = []
    v = verify.run_attn("cpx-1x36", env={"ROCR_VISIBLE_DEVICES": "GPU-abc"},
                        runner=fake_runner(json.dumps(report()), seen=seen))
    assert v["ok"] is True and v["failed"] == [] and v["profile"] == "cpx-1x36"
    assert v["report"]["kv_gb_per_s"] == 3456.7
    (cmd, kw), = seen
    assert cmd == [verify.BIN_PATH, "attn"]
    assert kw["env"]["ROCR_VISIBLE_DEVICES"] == "GPU-abc"
    assert kw["timeout"] == verify.CHILD_TIMEOUT_S


def test_run_attn_unknown_profile_raises():
    seen = []
    with pytest.raises(ValueError):
        verify.run_attn("bogus", runner=fake_runner(json.dumps(report()), seen=seen))
    assert seen == []


def test_run_attn_child_failures():
    v = verify.run_attn("cpx-1x36", runner=fake_runner("Segmentation fault\n", 0))
    assert v["ok"] is False and "non-JSON" in v["reason"]
    v = verify.run_attn("cpx-1x36", runner=fake_runner("", 0))
    assert v["ok"] is False and "non-JSON" in v["reason"]
    v = verify.run_attn("cpx-1x36", runner=fake_runner("[1, 2]\n", 0))
    assert v["ok"] is False and "non-JSON" in v["reason"]
    exc = subprocess.TimeoutExpired(cmd="instaslice-payload", timeout=1)
    v = verify.run_attn("cpx-1x36", runner=fake_runner(raises=exc))
    assert v["ok"] is False and "timed out" in v["reason"]
    v = verify.run_attn("cpx-1x36", runner=fake_runner(raises=FileNotFoundError()))
    assert v["ok"] is False and "not found" in v["reason"]
    v = verify.run_attn("cpx-1x36",
                        runner=fake_runner(raises=PermissionError("denied")))
    assert v["ok"] is False and "could not start" in v["reason"]
    # the binary's catch-all line
    err = json.dumps({"ok": False, "error": "HIP error: no ROCm-capable device"})
    v = verify.run_attn("cpx-1x36", runner=fake_runner(err, 1))
    assert v["ok"] is False and v["failed"] == []
    assert "no ROCm-capable device" in v["reason"] and "exit 1" in v["reason"]
    # a failing report is judged, and the exit status is carried
    for rep in (report(ok=False, max_err=0.0625), report(ok=False, max_rel=0.25)):
        v = verify.run_attn("cpx-1x36", runner=fake_runner(json.dumps(rep), 1))
        assert v["ok"] is False and v["failed"] == ["attn"]
        assert "exited 1" in v["reason"]
        # nor does a clean exit outvote a bad field
        v = verify.run_attn("cpx-1x36", runner=fake_runner(json.dumps(rep), 0))
        assert v["ok"] is False and v["failed"] == ["attn"]
    # clean-looking fields do not outvote a non-zero exit
    v = verify.run_attn("cpx-1x36", runner=fake_runner(json.dumps(report()), 1))
    assert v["ok"] is False and "exited 1" in v["reason"]


def test_run_attn_missing_binary_real_subprocess(monkeypatch, tmp_path):
    monkeypatch.setattr(verify, "BIN_PATH", str(tmp_path / "no-such-binary"))
    v = verify.run_attn("cpx-1x36")
    assert v["ok"] is False and "not found" in v["reason"]


# ---- CPU: the CLI command -------------------------------------------------

def _patch_runner(monkeypatch, runner):
    real = verify.run_attn
    monkeypatch.setattr(
        verify, "run_attn",
        lambda profile, **kw: real(profile, runner=runner, **kw))


def test_cli_attn_ok(monkeypatch, capsys):
    from instaslice_amd.cli import main

    seen = []
    _patch_runner(monkeypatch, fake_runner(json.dumps(report()), seen=seen))
    rc = main(["attn", "--profile", "cpx-1x36", "--visible-devices", "3"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 0 and out["ok"] is True and out["profile"] == "cpx-1x36"
    assert seen[0][0][1:] == ["attn"]
    assert seen[0][1]["env"]["ROCR_VISIBLE_DEVICES"] == "3"


def test_cli_attn_fail(monkeypatch, capsys):
    from instaslice_amd.cli import main

    rep = report(ok=False, max_rel=0.5)
    _patch_runner(monkeypatch, fake_runner(json.dumps(rep), 1))
    rc = main(["attn", "--profile", "cpx-1x36"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 1 and out["ok"] is False and out["failed"] == ["attn"]


def test_cli_attn_bad_profile(monkeypatch, capsys):
    from instaslice_amd.cli import main

    _patch_runner(monkeypatch, fake_runner(json.dumps(report())))
    rc = main(["attn", "--profile", "bogus"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 1 and out["ok"] is False and "bogus" in out["reason"]
    assert out["report"] is None


# ---- GPU: the self-check ----------------------------------------------------

CHECK_SHAPES = [
    (2, 8, 2, 100, 1),    # single split
    (2, 8, 2, 100, 3),    # several splits
    (1, 16, 1, 257, 5),   # G = 16, L = chunk multiple + 1
    (1, 6, 2, 64, 0),     # G = 3, auto splits
    (1, 1, 1, 33, 7),     # more splits than chunks: empty splits
    (1, 4, 4, 1, 0),      # a single key
]


@pytest.mark.gpu
@pytest.mark.parametrize("B,Hq,Hkv,L,splits", CHECK_SHAPES)
def test_run_attn_check(payload, B, Hq, Hkv, L, splits):
    r = payload.run_attn_check(B, Hq, Hkv, L, splits=splits)
    print(f"\nrun_attn_check{(B, Hq, Hkv, L, splits)}: {r}")
    assert set(r) == {"max_err", "max_rel"}
    assert r["max_err"] == 0
    assert 0 <= r["max_rel"] <= REL


@pytest.mark.gpu
def test_attn_decode_pattern_with_lengths_exact(payload):
    lengths = [1, 2, 64]
    q, k, v, expected = payload.attn_check_pattern(3, 4, 4, 64, lengths=lengths)
    out = payload.attn_decode(q, k, v, lengths=lengths, splits=4)
    assert out.dtype == np.float32 and out.shape == (3, 4, D)
    assert np.array_equal(out, expected)


# ---- GPU: general data against the fp64 reference ---------------------------

def random_problem(payload, B, Hq, Hkv, L, seed):
    rng = np.random.default_rng(seed)
    q = bf16_round(payload, 4 * rng.standard_normal((B, Hq, D)))
    k = bf16_round(payload, rng.standard_normal((B, Hkv, L, D)))
    v = bf16_round(payload, rng.uniform(-1, 1, (B, Hkv, L, D)))
    return q, k, v


def check_bounded(out, q, k, v, lengths=None, scale=None, what=""):
    ref = ref_attn(q, k, v, lengths, scale)
    n = k.shape[2] if lengths is None else max(lengths)
    vmax = np.abs(v[:, :, :n]).max()
    err = np.abs(out.astype(np.float64) - ref).max()
    print(f"\n{what}: max |o - ref| / max |v| = {err / vmax:.3e} (bound {REL:.3e})")
    assert out.dtype == np.float32 and out.shape == ref.shape
    assert np.isfinite(out).all()
    assert err <= REL * vmax


@pytest.fixture(scope="module")
def problem_300(payload):
    return random_problem(payload, 2, 8, 2, 300, seed=300)


@pytest.mark.gpu
@pytest.mark.parametrize("splits", [1, 3])
def test_attn_decode_random(payload, problem_300, splits):
    q, k, v = problem_300
    out = payload.attn_decode(q, k, v, splits=splits)
    check_bounded(out, q, k, v, what=f"(2,8,2,300) splits={splits}")


@pytest.mark.gpu
def test_attn_decode_random_scale(payload, problem_300):
    q, k, v = problem_300
    out = payload.attn_decode(q, k, v, scale=0.03, splits=2)
    check_bounded(out, q, k, v, scale=0.03, what="(2,8,2,300) scale=0.03")


@pytest.mark.gpu
def test_attn_decode_random_short_length_padding_does_not_leak(payload):
    q, k, v = random_problem(payload, 1, 16, 1, 513, seed=513)
    k[:, :, 400:] = 1e30    # finite in bf16
    v[:, :, 400:] = -1e30
    out = payload.attn_decode(q, k, v, lengths=[400])
    check_bounded(out, q, k, v, lengths=[400], what="(1,16,1,513) len=400")


@pytest.mark.gpu
@pytest.mark.parametrize("splits", [1, 3])
def test_attn_decode_spike_in_last_chunk(payload, problem_300, splits):
    """The running maximum jumps at the very last key: everything accumulated
    before it has to be rescaled (away)."""
    q, k, v = (a.copy() for a in problem_300)
    G = q.shape[1] // k.shape[1]
    for g in range(k.shape[1]):
        k[:, g, -1] = bf16_round(payload, k[:, g, -1] + 8 * q[:, g * G])
    out = payload.attn_decode(q, k, v, splits=splits)
    check_bounded(out, q, k, v, what=f"spike, splits={splits}")
    # the spiked heads see the last key alone
    assert np.abs(out[:, ::G] - v[:, :, -1]).max() <= REL


# ---- GPU: the timed run, the binary, serve, the runner ----------------------

@pytest.mark.gpu
def test_run_attn_timed(payload):
    r = payload.run_attn(2, 8, 2, 512, iters=2)
    print(f"\nrun_attn 2 8 2 512: {r}")
    assert set(r) == {"batch", "hq", "hkv", "len", "iters", "kv_gb_per_s",
                      "steps_per_s", "tok_per_s", "max_err"}
    assert (r["batch"], r["hq"], r["hkv"], r["len"], r["iters"]) == (2, 8, 2, 512, 2)
    assert r["max_err"] == 0
    for rate in ("kv_gb_per_s", "steps_per_s", "tok_per_s"):
        assert np.isfinite(r[rate]) and r[rate] > 0
    assert r["tok_per_s"] == pytest.approx(2 * r["steps_per_s"])


def run_bin(*args):
    out = subprocess.run([BIN, *args], capture_output=True, text=True,
                         timeout=120)
    return out.returncode, json.loads(out.stdout), out


@pytest.mark.gpu
def test_binary_attn():
    rc, res, out = run_bin("attn", "2", "8", "2", "512", "2")
    assert rc == 0, out.stdout + out.stderr
    assert set(res) == {"ok", "cmd", "batch", "hq", "hkv", "len", "iters",
                        "kv_gb_per_s", "steps_per_s", "tok_per_s", "max_err",
                        "max_rel"}
    assert res["ok"] is True and res["cmd"] == "attn"
    assert res["max_err"] == 0 and 0 <= res["max_rel"] <= REL
    assert (res["batch"], res["hq"], res["hkv"], res["len"], res["iters"]) == \
        (2, 8, 2, 512, 2)
    assert res["kv_gb_per_s"] > 0 and res["steps_per_s"] > 0 and res["tok_per_s"] > 0


@pytest.mark.gpu
def test_serve_attn():
    w = subprocess.Popen([BIN, "serve"], stdin=subprocess.PIPE,
                         stdout=subprocess.PIPE, text=True, bufsize=1)
    try:
        out, _ = w.communicate("attn\nattn 1 4 2 70\nquit\n", timeout=60)
    finally:
        if w.poll() is None:
            w.kill()
    first, second, quit_ = [json.loads(ln) for ln in out.splitlines()]
    for rep, shape in ((first, (2, 8, 2, 300)), (second, (1, 4, 2, 70))):
        assert set(rep) == {"ok", "cmd", "batch", "hq", "hkv", "len", "max_err",
                            "max_rel"}
        assert rep["ok"] is True and rep["cmd"] == "attn"
        assert rep["max_err"] == 0 and 0 <= rep["max_rel"] <= REL
        assert (rep["batch"], rep["hq"], rep["hkv"], rep["len"]) == shape
    assert quit_ == {"ok": True}


@pytest.mark.gpu
def test_run_attn_judges_the_real_partition():
    """ops/verify.run_attn end to end: the only run at the default shape."""
    v = verify.run_attn("spx-8x288")
    print(f"\nrun_attn(spx-8x288): {v}")
    assert v["ok"] is True and v["failed"] == [] and v["profile"] == "spx-8x288"
    rep = v["report"]
    assert (rep["batch"], rep["hq"], rep["hkv"], rep["len"], rep["iters"]) == \
        (32, 64, 8, 4096, 10)
    assert rep["max_err"] == 0 and 0 <= rep["max_rel"] <= REL
    assert rep["kv_gb_per_s"] > 0
