"""The causal prefill attention payload (ops/csrc/payload_prefill.hpp): the
check pattern, argument checks, the judge, the runner and the CLI on CPU; the
kernel, its bindings, the binary's `prefill` verb, the `serve` verb and
`verify.run_prefill` on a real MI355X.

The reference is written here in numpy fp64 from the definition,
independently of the header:

    o[b,h,i,:] = softmax_t(scale * q[b,h,i,:] . k[b,g,t,:]) . v[b,g,t,:]
    with g = h // (Hq // Hkv) and t <= i if causal, else t < L

Two kinds of comparison:

  exact      the selection pattern: K is 0 at the selected keys (key 0 and
             every t with (t + b + 2 g) % 5 == 0) and <= -16 elsewhere, q >= 2,
             so a selected score is exactly 0 and any other is <= -4096 scale
             (about -362), whose weight is exactly 0 in fp32. The result is an
             integer sum of v over an integer count, rounded once by the
             division: bit-exact in any tile order. Tolerance 0.
  bounded    general data: |o - ref| <= 2^-8 max |v|. The kernel rounds each
             softmax weight to bf16 (at most 2^-9 relative) and sums the
             normaliser from the unrounded weights, so the output is off by
             at most 2^-9 max |v| plus fp32 terms of order 1e-6; the bound
             doubles that (the derivation above verify.ATTN_MAX_REL: the
             numerics contract is decode's). max |v| is taken over the keys
             that take part.

The GPU shapes are the smallest at which the kernel takes every path: with R =
PREFILL_ROWS query rows per workgroup and T = PREFILL_KEYS keys per LDS tile,
lengths of 1, below and just above T, R - 1, R + 1 and 2 R + T + 5 (several row
blocks, a ragged last block and a ragged last tile).
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

def ref_prefill(q, k, v, causal=True, scale=None, keys=None):
    """fp64 softmax attention from the definition; `keys` caps the visible
    keys at t < keys on top of the mask."""
    B, Hq, L, _ = q.shape
    Hkv = k.shape[1]
    G = Hq // Hkv
    scale = 1.0 / np.sqrt(np.float64(D)) if scale is None else np.float64(scale)
    t = np.arange(L)
    visible = (t[None, :] <= t[:, None]) if causal else np.ones((L, L), bool)
    if keys is not None:
        visible = visible & (t[None, :] < keys)
    out = np.empty((B, Hq, L, D), dtype=np.float64)
    for b in range(B):
        for h in range(Hq):
            g = h // G
            s = q[b, h].astype(np.float64) @ k[b, g].astype(np.float64).T * scale
            s = np.where(visible, s, -np.inf)
            w = np.exp(s - s.max(axis=1, keepdims=True))
            out[b, h] = (w @ v[b, g].astype(np.float64)) / w.sum(axis=1, keepdims=True)
    return out


def bf16_round(payload, x):
    """x rounded to bf16 (the payload's own host rounding), back as float32."""
    bits = payload.to_bf16(np.ascontiguousarray(x, dtype=np.float32))
    return (bits.astype(np.uint32) << 16).view(np.float32)


# (batch, hq, hkv, length)
PATTERN_SHAPES = [(2, 4, 2, 200), (1, 3, 1, 129), (1, 1, 1, 1), (1, 2, 2, 33),
                  (1, 16, 1, 70)]


# ---- CPU: prefill_check_pattern ----------------------------------------------

@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("B,Hq,Hkv,L", PATTERN_SHAPES)
def test_check_pattern(payload, B, Hq, Hkv, L, causal):
    q, k, v, expected = payload.prefill_check_pattern(B, Hq, Hkv, L, causal=causal)
    assert q.shape == (B, Hq, L, D) and expected.shape == (B, Hq, L, D)
    assert k.shape == (B, Hkv, L, D) and v.shape == (B, Hkv, L, D)
    for a in (q, k, v, expected):
        assert a.dtype == np.float32
    # every input is exact in bf16, and a small integer
    for a in (q, k, v):
        assert np.array_equal(bf16_round(payload, a), a)
        assert np.array_equal(np.round(a), a)
    assert q.min() >= 2 and q.max() <= 5 and np.abs(v).max() <= 4
    if L > 1:
        assert (q[:, :, 0] != q[:, :, 1]).any()   # q varies with the row

    G = Hq // Hkv
    scale = 1.0 / np.sqrt(128.0)
    t = np.arange(L)
    for b in range(B):
        for g in range(Hkv):
            zero = (k[b, g] == 0).all(axis=1)
            want = (t == 0) | ((t + b + 2 * g) % 5 == 0)
            assert np.array_equal(zero, want) and zero[0]
            assert (k[b, g][~zero] <= -16).all()
            for h in range(g * G, (g + 1) * G):
                s = q[b, h].astype(np.float64) @ k[b, g].astype(np.float64).T * scale
                assert (s[:, zero] == 0).all()
                if (~zero).any():
                    assert s[:, ~zero].max() <= -300
    # the closed form is the fp64 softmax, bit for bit
    ref = ref_prefill(q, k, v, causal=causal).astype(np.float32)
    assert np.array_equal(expected, ref)


def test_check_pattern_default_is_causal(payload):
    a = payload.prefill_check_pattern(1, 2, 1, 40)
    b = payload.prefill_check_pattern(1, 2, 1, 40, causal=True)
    c = payload.prefill_check_pattern(1, 2, 1, 40, causal=False)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[3], c[3])


def test_constants(payload):
    R, T = payload.PREFILL_ROWS, payload.PREFILL_KEYS
    assert isinstance(R, int) and isinstance(T, int)
    assert T == 64 and R >= T and R % T == 0


# ---- CPU: argument checks (raised before any HIP call) -----------------------

BAD_SHAPES = [(0, 4, 4, 8), (1, 0, 1, 8), (1, 4, 0, 8), (1, 4, 4, 0), (1, 3, 2, 8),
              (-1, 4, 4, 8), (1, 4, 4, 2 ** 24 + 1), (70000, 4, 4, 8),
              (1, 70000, 70000, 8), (65535, 65535, 1, 128)]


def test_check_pattern_rejects_bad_arguments(payload):
    for args in BAD_SHAPES:
        with pytest.raises(ValueError):
            payload.prefill_check_pattern(*args)


def _qkv(B=1, Hq=2, Hkv=1, L=4, d=D):
    return (np.ones((B, Hq, L, d), np.float32), np.ones((B, Hkv, L, d), np.float32),
            np.ones((B, Hkv, L, d), np.float32))


def test_attn_prefill_rejects_bad_arguments(payload):
    q, k, v = _qkv()
    bad = [
        ((q[0], k, v), {}),                                   # q not 4-D
        ((q, k[0], v[0]), {}),                                # k, v not 4-D
        ((q[..., None], k, v), {}),                           # q 5-D
        ((q, k[..., None], v[..., None]), {}),                # k, v 5-D
        (_qkv(d=64), {}),                                     # D != 128
        (_qkv(Hq=3, Hkv=2), {}),                              # Hq % Hkv != 0
        (_qkv(B=0), {}),                                      # empty batch
        (_qkv(L=0), {}),                                      # empty prompt
        ((q[:, :0], k, v), {}),                               # no query heads
        ((q, k[:, :0], v[:, :0]), {}),                        # no kv heads
        ((q, k, v[:, :, :3]), {}),                            # k / v mismatch
        ((q, k[:, :, :3], v[:, :, :3]), {}),                  # q / k length mismatch
        ((q, k, np.ones((1, 1, 4, 64), np.float32)), {}),     # v with D = 64
        ((np.ones((2, 2, 4, D), np.float32), k, v), {}),      # batch mismatch
        ((q, k, v), {"scale": float("nan")}),
        ((q, k, v), {"scale": float("inf")}),
        ((q, k, v), {"scale": float("-inf")}),
    ]
    for args, kw in bad:
        with pytest.raises(ValueError):
            payload.attn_prefill(*args, **kw)
    for which in range(3):
        for junk in (np.nan, np.inf, -np.inf):
            args = [a.copy() for a in (q, k, v)]
            args[which].flat[-1] = junk
            with pytest.raises(ValueError):
                payload.attn_prefill(*args)
            with pytest.raises(ValueError):
                payload.attn_prefill(*args, causal=False)


def test_run_prefill_rejects_bad_arguments(payload):
    for args in BAD_SHAPES:
        with pytest.raises(ValueError):
            payload.run_prefill_check(*args)
        with pytest.raises(ValueError):
            payload.run_prefill(*args)
    with pytest.raises(ValueError):
        payload.run_prefill(1, 2, 1, 8, iters=0)
    with pytest.raises(ValueError):
        payload.run_prefill(1, 2, 1, 8, iters=-3)
    with pytest.raises(ValueError):
        payload.run_prefill(1, 2, 1, 8, pattern=2)


# ---- CPU: judge_prefill ---------------------------------------------------

def report(**over):
    """What the binary prints for a clean default run."""
    r = {"ok": True, "cmd": "prefill", "batch": 8, "hq": 64, "hkv": 8,
         "len": 4096, "iters": 10, "causal": True, "tflops": 456.78,
         "tok_per_s": 1234567.8, "max_err": 0, "max_rel": 0.000275}
    r.update(over)
    return r


def test_judge_prefill_pass():
    rep = report()
    v = verify.judge_prefill(rep, "cpx-1x36")
    assert v == {"ok": True, "failed": [], "profile": "cpx-1x36", "report": rep}
    # rates are carried, never judged; the report's own ok is not trusted
    assert verify.judge_prefill(report(tflops=0.0, tok_per_s=0.0, ok=False),
                                "cpx-1x36")["ok"]
    assert verify.judge_prefill(report(max_err=0.0), "cpx-1x36")["ok"] is True
    assert verify.judge_prefill(report(max_rel=0), "cpx-1x36")["ok"] is True
    assert verify.judge_prefill(report(max_rel=2.0 ** -8), "cpx-1x36")["ok"] is True
    assert verify.judge_prefill(report(causal=False), "cpx-1x36")["ok"] is True
    rep = report()
    for rate in ("tflops", "tok_per_s"):
        del rep[rate]
    assert verify.judge_prefill(rep, "cpx-1x36")["ok"] is True


def test_judge_prefill_non_zero_error():
    for err in (0.0625, 1e-30, 1e300, -1, float("nan")):
        v = verify.judge_prefill(report(ok=True, max_err=err), "cpx-1x36")
        assert v["ok"] is False and v["failed"] == ["prefill"]


def test_judge_prefill_max_rel():
    above = float(np.nextafter(2.0 ** -8, 1.0))
    for rel in (above, 0.1, 1e300, -1e-9, float("nan"), float("inf"),
                "0.001", None, True, False):
        v = verify.judge_prefill(report(ok=True, max_rel=rel), "cpx-1x36")
        assert v["ok"] is False and v["failed"] == ["prefill"], rel


@pytest.mark.parametrize("field", ["max_err", "max_rel", "batch", "hq", "hkv",
                                   "len", "iters"])
def test_judge_prefill_missing_or_non_numeric_field(field):
    rep = report()
    del rep[field]
    assert verify.judge_prefill(rep, "cpx-1x36")["failed"] == ["prefill"]
    for junk in ("0", None, True, False):
        assert verify.judge_prefill(report(**{field: junk}),
                                    "cpx-1x36")["failed"] == ["prefill"]


@pytest.mark.parametrize("field", ["batch", "hq", "hkv", "len", "iters"])
def test_judge_prefill_counts_must_be_positive_integers(field):
    for junk in (0, -1, 1.0, 4096.5):
        assert verify.judge_prefill(report(**{field: junk}),
                                    "cpx-1x36")["failed"] == ["prefill"]


def test_judge_prefill_causal_must_be_a_bool():
    rep = report()
    del rep["causal"]
    assert verify.judge_prefill(rep, "cpx-1x36")["failed"] == ["prefill"]
    for junk in (1, 0, "true", None, 1.0):
        assert verify.judge_prefill(report(causal=junk),
                                    "cpx-1x36")["failed"] == ["prefill"]


def test_judge_prefill_unknown_profile():
    with pytest.raises(ValueError):
        verify.judge_prefill(report(), "not-a-profile")


# ---- CPU: verify.run_prefill with a fake child -------------------------------

def fake_runner(stdout="", returncode=0, raises=None, seen=None):
    def runner(cmd, **kw):
        if seen is not None:
            seen.append((cmd, kw))
        if raises is not None:
            raise raises
        return SimpleNamespace(stdout=stdout, stderr="", returncode=returncode)
    return runner


def test_run_prefill_pass():
    seen = []
    v = verify.run_prefill("cpx-1x36", env={"ROCR_VISIBLE_DEVICES": "GPU-abc"},
                           runner=fake_runner(json.dumps(report()), seen=seen))
    assert v["ok"] is True and v["failed"] == [] and v["profile"] == "cpx-1x36"
    assert v["report"]["tflops"] == 456.78
    (cmd, kw), = seen
    assert cmd == [verify.BIN_PATH, "prefill"]
    assert kw["env"]["ROCR_VISIBLE_DEVICES"] == "GPU-abc"
    assert kw["timeout"] == verify.CHILD_TIMEOUT_S


def test_run_prefill_unknown_profile_raises():
    seen = []
    with pytest.raises(ValueError):
        verify.run_prefill("bogus", runner=fake_runner(json.dumps(report()), seen=seen))
    assert seen == []


def test_run_prefill_child_failures():
    v = verify.run_prefill("cpx-1x36", runner=fake_runner("Segmentation fault\n", 0))
    assert v["ok"] is False and "non-JSON" in v["reason"]
    v = verify.run_prefill("cpx-1x36", runner=fake_runner("", 0))
    assert v["ok"] is False and "non-JSON" in v["reason"]
    v = verify.run_prefill("cpx-1x36", runner=fake_runner("[1, 2]\n", 0))
    assert v["ok"] is False and "non-JSON" in v["reason"]
    exc = subprocess.TimeoutExpired(cmd="instaslice-payload", timeout=1)
    v = verify.run_prefill("cpx-1x36", runner=fake_runner(raises=exc))
    assert v["ok"] is False and "timed out" in v["reason"]
    v = verify.run_prefill("cpx-1x36", runner=fake_runner(raises=FileNotFoundError()))
    assert v["ok"] is False and "not found" in v["reason"]
    v = verify.run_prefill("cpx-1x36",
                           runner=fake_runner(raises=PermissionError("denied")))
    assert v["ok"] is False and "could not start" in v["reason"]
    # the binary's catch-all line
    err = json.dumps({"ok": False, "error": "HIP error: no ROCm-capable device"})
    v = verify.run_prefill("cpx-1x36", runner=fake_runner(err, 1))
    assert v["ok"] is False and v["failed"] == []
    assert "no ROCm-capable device" in v["reason"] and "exit 1" in v["reason"]
    # a failing report is judged, and the exit status is carried
    for rep in (report(ok=False, max_err=0.0625), report(ok=False, max_rel=0.25)):
        v = verify.run_prefill("cpx-1x36", runner=fake_runner(json.dumps(rep), 1))
        assert v["ok"] is False and v["failed"] == ["prefill"]
        assert "exited 1" in v["reason"]
        # nor does a clean exit outvote a bad field
        v = verify.run_prefill("cpx-1x36", runner=fake_runner(json.dumps(rep), 0))
        assert v["ok"] is False and v["failed"] == ["prefill"]
    # clean-looking fields do not outvote a non-zero exit
    v = verify.run_prefill("cpx-1x36", runner=fake_runner(json.dumps(report()), 1))
    assert v["ok"] is False and "exited 1" in v["reason"]


def test_run_prefill_missing_binary_real_subprocess(monkeypatch, tmp_path):
    monkeypatch.setattr(verify, "BIN_PATH", str(tmp_path / "no-such-binary"))
    v = verify.run_prefill("cpx-1x36")
    assert v["ok"] is False and "not found" in v["reason"]


# ---- CPU: the CLI command -------------------------------------------------

def _patch_runner(monkeypatch, runner):
    real = verify.run_prefill
    monkeypatch.setattr(
        verify, "run_prefill",
        lambda profile, **kw: real(profile, runner=runner, **kw))


def test_cli_prefill_ok(monkeypatch, capsys):
    from instaslice_amd.cli import main

    seen = []
    _patch_runner(monkeypatch, fake_runner(json.dumps(report()), seen=seen))
    rc = main(["prefill", "--profile", "cpx-1x36", "--visible-devices", "3"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 0 and out["ok"] is True and out["profile"] == "cpx-1x36"
    assert seen[0][0][1:] == ["prefill"]
    assert seen[0][1]["env"]["ROCR_VISIBLE_DEVICES"] == "3"


def test_cli_prefill_fail(monkeypatch, capsys):
    from instaslice_amd.cli import main

    rep = report(ok=False, max_rel=0.5)
    _patch_runner(monkeypatch, fake_runner(json.dumps(rep), 1))
    rc = main(["prefill", "--profile", "cpx-1x36"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 1 and out["ok"] is False and out["failed"] == ["prefill"]


def test_cli_prefill_bad_profile(monkeypatch, capsys):
    from instaslice_amd.cli import main

    _patch_runner(monkeypatch, fake_runner(json.dumps(report())))
    rc = main(["prefill", "--profile", "bogus"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 1 and out["ok"] is False and "bogus" in out["reason"]
    assert out["report"] is None


# ---- GPU: the self-check ----------------------------------------------------

# lengths in terms of R = PREFILL_ROWS and T = PREFILL_KEYS
LENGTHS = {"1": lambda R, T: 1, "33": lambda R, T: 33, "70": lambda R, T: 70,
           "T+1": lambda R, T: T + 1, "R-1": lambda R, T: R - 1,
           "R+1": lambda R, T: R + 1, "2R+T+5": lambda R, T: 2 * R + T + 5}

# (batch, hq, hkv, length)
CHECK_SHAPES = [(1, 1, 1, "1"), (1, 2, 2, "33"), (1, 4, 1, "T+1"), (2, 6, 2, "R-1"),
                (1, 3, 1, "R+1"), (2, 8, 2, "2R+T+5"), (1, 16, 1, "70")]


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("B,Hq,Hkv,length", CHECK_SHAPES)
def test_run_prefill_check(payload, B, Hq, Hkv, length, causal):
    L = LENGTHS[length](payload.PREFILL_ROWS, payload.PREFILL_KEYS)
    r = payload.run_prefill_check(B, Hq, Hkv, L, causal=causal)
    print(f"\nrun_prefill_check{(B, Hq, Hkv, L, causal)}: {r}")
    assert set(r) == {"max_err", "max_rel"}
    assert r["max_err"] == 0
    assert 0 <= r["max_rel"] <= REL


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [True, False])
def test_attn_prefill_pattern_exact(payload, causal):
    R, T = payload.PREFILL_ROWS, payload.PREFILL_KEYS
    L = R + T + 3
    q, k, v, expected = payload.prefill_check_pattern(2, 6, 2, L, causal=causal)
    out = payload.attn_prefill(q, k, v, causal=causal)
    assert out.dtype == np.float32 and out.shape == (2, 6, L, D)
    assert np.array_equal(out, expected)


# ---- GPU: general data against the fp64 reference ---------------------------

def random_problem(payload, B, Hq, Hkv, L, seed):
    rng = np.random.default_rng(seed)
    q = bf16_round(payload, 4 * rng.standard_normal((B, Hq, L, D)))
    k = bf16_round(payload, rng.standard_normal((B, Hkv, L, D)))
    v = bf16_round(payload, rng.uniform(-1, 1, (B, Hkv, L, D)))
    return q, k, v


def check_bounded(out, ref, vmax, what=""):
    err = np.abs(out.astype(np.float64) - ref).max()
    print(f"\n{what}: max |o - ref| / max |v| = {err / vmax:.3e} (bound {REL:.3e})")
    assert out.dtype == np.float32 and out.shape == ref.shape
    assert np.isfinite(out).all()
    assert err <= REL * vmax


@pytest.fixture(scope="module")
def problem(payload):
    R = payload.PREFILL_ROWS
    return random_problem(payload, 2, 8, 2, 2 * R + 37, seed=2 * R + 37)


@pytest.mark.gpu
@pytest.mark.parametrize("causal,scale", [(True, None), (False, None), (True, 0.03)])
def test_attn_prefill_random(payload, problem, causal, scale):
    q, k, v = problem
    out = payload.attn_prefill(q, k, v, causal=causal, scale=scale)
    ref = ref_prefill(q, k, v, causal=causal, scale=scale)
    check_bounded(out, ref, np.abs(v).max(),
                  what=f"{q.shape} causal={causal} scale={scale}")


@pytest.mark.gpu
def test_attn_prefill_diagonal_spike(payload, problem):
    """Every row's maximum jumps at its last visible key, inside the masked
    tile: everything accumulated before it has to be rescaled (away)."""
    q, k, v = (a.copy() for a in problem)
    G = q.shape[1] // k.shape[1]
    for g in range(k.shape[1]):
        k[:, g] = bf16_round(payload, k[:, g] + 8 * q[:, g * G])
    out = payload.attn_prefill(q, k, v, causal=True)
    check_bounded(out, ref_prefill(q, k, v, causal=True), np.abs(v).max(),
                  what="diagonal spike")
    # row i of a spiked head sees key i alone
    assert np.abs(out[:, ::G] - v).max() <= REL


@pytest.mark.gpu
def test_attn_prefill_future_keys_do_not_leak(payload):
    R, T = payload.PREFILL_ROWS, payload.PREFILL_KEYS
    L, t0 = R + T + 9, R + 5
    q, k, v = random_problem(payload, 1, 4, 2, L, seed=L)
    k[:, :, t0:] = 1e30    # finite in bf16
    v[:, :, t0:] = -1e30
    out = payload.attn_prefill(q, k, v, causal=True)
    assert out.shape == (1, 4, L, D)
    ref = ref_prefill(q, k, v, causal=True, keys=t0)
    check_bounded(out[:, :, :t0], ref[:, :, :t0], np.abs(v[:, :, :t0]).max(),
                  what=f"rows below {t0} of {L}")


# ---- GPU: the timed run, the binary, serve, the runner ----------------------

@pytest.mark.gpu
def test_run_prefill_timed(payload):
    R = payload.PREFILL_ROWS
    r = payload.run_prefill(2, 8, 2, 2 * R, iters=2)
    print(f"\nrun_prefill 2 8 2 {2 * R}: {r}")
    assert set(r) == {"batch", "hq", "hkv", "len", "iters", "causal", "tflops",
                      "tok_per_s", "max_rel"}
    assert (r["batch"], r["hq"], r["hkv"], r["len"], r["iters"]) == (2, 8, 2, 2 * R, 2)
    assert r["causal"] is True
    assert 0 <= r["max_rel"] <= REL
    for rate in ("tflops", "tok_per_s"):
        assert np.isfinite(r[rate]) and r[rate] > 0


def run_bin(*args):
    out = subprocess.run([BIN, *args], capture_output=True, text=True,
                         timeout=120)
    return out.returncode, json.loads(out.stdout), out


@pytest.mark.gpu
def test_binary_prefill(payload):
    R = payload.PREFILL_ROWS
    rc, res, out = run_bin("prefill", "2", "8", "2", str(2 * R), "2")
    assert rc == 0, out.stdout + out.stderr
    assert set(res) == {"ok", "cmd", "batch", "hq", "hkv", "len", "iters", "causal",
                        "tflops", "tok_per_s", "max_err", "max_rel"}
    assert res["ok"] is True and res["cmd"] == "prefill" and res["causal"] is True
    assert res["max_err"] == 0 and 0 <= res["max_rel"] <= REL
    assert (res["batch"], res["hq"], res["hkv"], res["len"], res["iters"]) == \
        (2, 8, 2, 2 * R, 2)
    assert res["tflops"] > 0 and res["tok_per_s"] > 0


@pytest.mark.gpu
def test_serve_prefill(payload):
    w = subprocess.Popen([BIN, "serve"], stdin=subprocess.PIPE,
                         stdout=subprocess.PIPE, text=True, bufsize=1)
    try:
        out, _ = w.communicate("prefill\nprefill 1 4 2 70\nquit\n", timeout=60)
    finally:
        if w.poll() is None:
            w.kill()
    first, second, quit_ = [json.loads(ln) for ln in out.splitlines()]
    for rep, shape in ((first, None), (second, (1, 4, 2, 70))):
        assert set(rep) == {"ok", "cmd", "batch", "hq", "hkv", "len", "causal",
                            "max_err", "max_rel"}
        assert rep["ok"] is True and rep["cmd"] == "prefill"
        assert rep["max_err"] == 0 and 0 <= rep["max_rel"] <= REL
        if shape is not None:
            assert (rep["batch"], rep["hq"], rep["hkv"], rep["len"]) == shape
    # the default shape crosses a row-block edge
    assert first["len"] > payload.PREFILL_ROWS
    assert quit_ == {"ok": True}


@pytest.mark.gpu
def test_run_prefill_judges_the_real_partition():
    """ops/verify.run_prefill end to end: the only run at the default shape."""
    v = verify.run_prefill("spx-8x288")
    print(f"\nrun_prefill(spx-8x288): {v}")
    assert v["ok"] is True and v["failed"] == [] and v["profile"] == "spx-8x288"
    rep = v["report"]
    assert (rep["batch"], rep["hq"], rep["hkv"], rep["len"], rep["iters"]) == \
        (8, 64, 8, 4096, 10)
    assert rep["causal"] is True
    assert rep["max_err"] == 0 and 0 <= rep["max_rel"] <= REL
    assert rep["tflops"] > 0
