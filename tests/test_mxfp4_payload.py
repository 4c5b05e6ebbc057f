"""The MXFP4 block-scaled MFMA GEMM payload (ops/csrc/payload_mxfp4.hpp): the
e2m1 conversion, the MX quantizer, the nibble packer, argument checks, the
judge, the runner and the CLI on CPU; the kernel, its bindings, the binary's
`mx4gemm` verb and `verify.run_mx4gemm` on a real MI355X.

The formats are re-implemented here in numpy from their definitions,
independently of the header:

    e2m1 code (4 bits): 1 sign, 2 exponent (bias 1), 1 mantissa bit. Exponent
    0 is subnormal (m * 0.5), everything else (1 + m/2) * 2^(e - 1): the
    magnitudes of codes 0..7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6. No NaN, no
    infinity, both zeros. Conversion: the nearest of the 8 magnitudes, a tie
    to the even code, anything beyond 6 to 6.

    MX block (32 elements): scale byte = clamp(floor(log2(amax)) - 2 + 127,
    0, 254), 127 for an all-zero block; elements = e2m1(x / 2^(scale - 127)).

    Device image: element k of a row in byte k // 2, even k in bits 3:0, odd
    k in bits 7:4, an odd tail padded with code 0.

Exactness of the all-codes GPU test. Elements are multiples of 0.5 with
|x| <= 6 and scale bytes 125..129 on both sides, so the reference works in
units of 2^-6: each side is round(2 * value) << (scale - 125), an integer of
magnitude <= 12 * 2^4, and the product of the two, divided by 64, is the term.
The scale product is within 2^-4 .. 2^4, so a term is at most 144 * 2^8 = 36864
units, and every partial sum of K terms stays at or below 2^24 units for
K <= 455 (455 * 36864 = 16773120 <= 2^24 = 16777216): fp32 holds every partial
sum exactly, which makes the fp32 result the same bits in any accumulation
order. Those tests compare with np.array_equal. One listed shape, (64, 64,
512), lies beyond that worst-case K; there the test asserts the same property
on its own data instead: the sum of the magnitudes of an output's K terms,
which bounds every partial sum in any order, stays at or below 2^24 units
(random codes and scales reach about 4e5).

The integer pattern of run_mx4gemm_check is the MXFP8 payload's (integers in
[-4, 4], scales 2^-2 .. 2^2), exact for K <= 2048 by the argument given there.
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


@pytest.fixture(scope="module")
def payload():
    from instaslice_amd.ops import _payload

    return _payload


# ---- the numpy reference --------------------------------------------------

def _e2m1_table():
    t = np.empty(16, dtype=np.float64)
    for c in range(16):
        e, m = (c >> 1) & 3, c & 1
        v = m * 0.5 if e == 0 else (1 + m / 2) * 2.0 ** (e - 1)
        t[c] = -v if c & 8 else v
    return t


TABLE = _e2m1_table()
POS = TABLE[:8]  # the non-negative values, ascending: 0 .. 6


def ref_to_e2m1(x):
    """Nearest e2m1 code of each element of x (float64 arithmetic, exact for
    float32 inputs), ties to the even code, saturating."""
    x = np.asarray(x, dtype=np.float64)
    ax = np.abs(x)
    hi = np.clip(np.searchsorted(POS, ax, side="left"), 0, 7)
    lo = np.clip(hi - 1, 0, 7)
    dlo, dhi = ax - POS[lo], POS[hi] - ax
    code = np.where(dlo < dhi, lo,
                    np.where(dhi < dlo, hi, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(ax >= 6, 7, code)
    return (code | np.where(np.signbit(x), 8, 0)).astype(np.uint8)


def ref_mx4_quantize(x):
    """(codes, scales) of a 2-D float32 array along its last axis."""
    x = np.asarray(x, dtype=np.float32)
    rows, k = x.shape
    blocks = -(-k // 32)
    codes = np.zeros((rows, k), dtype=np.uint8)
    scales = np.zeros((rows, blocks), dtype=np.uint8)
    for r in range(rows):
        for b in range(blocks):
            seg = x[r, 32 * b:32 * b + 32].astype(np.float64)
            amax = np.abs(seg).max()
            if amax == 0:
                s = 127
            else:
                _m, e = np.frexp(amax)  # amax = m * 2^e, m in [0.5, 1)
                s = int(np.clip((e - 1) - 2 + 127, 0, 254))
            scales[r, b] = s
            codes[r, 32 * b:32 * b + 32] = ref_to_e2m1(seg * 2.0 ** (127 - s))
    return codes, scales


def ref_pack(codes):
    """Byte image along the last axis: even k low nibble, odd k high."""
    codes = np.asarray(codes, dtype=np.uint8)
    k = codes.shape[-1]
    if k % 2:
        pad = np.zeros(codes.shape[:-1] + (1,), np.uint8)
        codes = np.concatenate([codes, pad], axis=-1)
    return (codes[..., 0::2] | (codes[..., 1::2] << 4)).astype(np.uint8)


def test_reference_table_landmarks(payload):
    assert TABLE[2] == 1.0 and TABLE[7] == 6.0 and TABLE[15] == -6.0
    assert TABLE[8] == 0 and np.signbit(TABLE[8])
    assert list(POS) == [0, 0.5, 1, 1.5, 2, 3, 4, 6]
    got = payload.from_e2m1(np.array([2, 7, 15, 8], np.uint8))
    assert list(got[:3]) == [1.0, 6.0, -6.0]
    assert got[3] == 0 and np.signbit(got[3])


# ---- CPU: to_e2m1 / from_e2m1 ---------------------------------------------

def test_to_e2m1_matches_reference(payload):
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    x = (x / np.abs(x).max() * 6).astype(np.float32)
    assert np.abs(x).max() <= 6
    got = payload.to_e2m1(x)
    assert got.dtype == np.uint8 and got.shape == x.shape
    assert got.max() <= 15
    assert np.array_equal(got, ref_to_e2m1(x))
    small = (x * 2.0 ** -3).astype(np.float32)
    assert np.array_equal(payload.to_e2m1(small), ref_to_e2m1(small))


def test_to_e2m1_ties_go_to_the_even_code(payload):
    x = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], dtype=np.float32)
    want = np.array([0, 2, 2, 4, 4, 6, 6], dtype=np.uint8)
    assert np.array_equal(payload.to_e2m1(x), want)
    assert np.array_equal(payload.to_e2m1(-x), want | 8)
    assert np.array_equal(ref_to_e2m1(x), want)
    # one float32 step either side of a tie goes to the nearer value
    up = np.nextafter(x, np.float32(10))
    dn = np.nextafter(x, np.float32(0))
    assert np.array_equal(payload.to_e2m1(up), np.arange(1, 8, dtype=np.uint8))
    assert np.array_equal(payload.to_e2m1(dn), np.arange(0, 7, dtype=np.uint8))


def test_to_e2m1_saturates(payload):
    x = np.array([6.0, 7.0, 1e9, np.inf], dtype=np.float32)
    assert list(payload.to_e2m1(x)) == [7] * 4
    assert list(payload.to_e2m1(-x)) == [15] * 4


def test_to_e2m1_keeps_both_zeros(payload):
    assert list(payload.to_e2m1(np.array([0.0, -0.0], np.float32))) == [0, 8]


def test_to_e2m1_nan_raises(payload):
    for bits in (0x7FC00000, 0xFFC00000, 0x7F800001):
        x = np.ones(5, np.float32)
        x[3] = np.array([bits], np.uint32).view(np.float32)[0]
        with pytest.raises(ValueError):
            payload.to_e2m1(x)


def test_to_e2m1_keeps_shape_and_converts_input(payload):
    x = (np.arange(12, dtype=np.float64).reshape(3, 4) / 2)[:, ::2]  # f64, strided
    got = payload.to_e2m1(x)
    assert got.shape == (3, 2)
    assert np.array_equal(got, ref_to_e2m1(np.ascontiguousarray(x)))


def test_from_e2m1_is_the_table(payload):
    codes = np.arange(16, dtype=np.uint8)
    got = payload.from_e2m1(codes)
    assert got.dtype == np.float32 and got.shape == (16,)
    assert np.array_equal(got.astype(np.float64), TABLE)
    assert np.signbit(got[8]) and got[8] == 0 and not np.signbit(got[0])
    assert payload.from_e2m1(codes.reshape(4, 4)).shape == (4, 4)
    assert np.array_equal(payload.to_e2m1(got), codes)
    for bad in (16, 255):
        with pytest.raises(ValueError):
            payload.from_e2m1(np.array([0, bad], np.uint8))


# ---- CPU: mx4_quantize ----------------------------------------------------

@pytest.mark.parametrize("k", [32, 40, 128])
def test_mx4_quantize_random_rows(payload, k):
    rng = np.random.default_rng(k)
    # rows of very different magnitude, so scales differ from row to row
    x = (rng.standard_normal((6, k)) *
         (10.0 ** rng.integers(-6, 7, size=(6, 1)))).astype(np.float32)
    codes, scales = payload.mx4_quantize(x)
    assert codes.dtype == np.uint8 and codes.shape == (6, k)
    assert scales.dtype == np.uint8 and scales.shape == (6, -(-k // 32))
    ref_codes, ref_scales = ref_mx4_quantize(x)
    assert np.array_equal(scales, ref_scales)
    assert np.array_equal(codes, ref_codes)
    assert len(np.unique(scales[:, 0])) > 1


def test_mx4_quantize_special_blocks(payload):
    rng = np.random.default_rng(5)
    base = rng.uniform(-1, 1, size=32).astype(np.float32)
    base[7] = 1.0  # amax of `base` is exactly 1
    rows = np.stack([
        base,                            # amax 1: scale 125, 1 * 2^2 = 4
        np.zeros(32, np.float32),        # all zero: scale 127
        base * np.float32(7),            # amax 7 -> scale 127, 7 saturates
        base * np.float32(2.0 ** -125),  # the scale clamps at 0
        base * np.float32(1e-40),        # fp32 subnormals, clamped as well
    ]).astype(np.float32)
    rows[1, 3] = -0.0
    codes, scales = payload.mx4_quantize(rows)
    ref_codes, ref_scales = ref_mx4_quantize(rows)
    assert np.array_equal(scales, ref_scales)
    assert np.array_equal(codes, ref_codes)
    assert list(scales[:, 0]) == [125, 127, 127, 0, 0]
    assert codes[0, 7] == 6              # 4.0
    assert codes[1, 3] == 8 and not codes[1, :3].any() and not codes[1, 4:].any()
    assert codes[2, 7] == 7              # 7 -> 6
    assert codes[3, 7] == 6              # 2^-125 * 2^127 = 4


def test_mx4_quantize_nan_raises(payload):
    x = np.ones((2, 40), np.float32)
    x[1, 35] = np.nan
    with pytest.raises(ValueError):
        payload.mx4_quantize(x)


def test_mx4_quantize_shapes(payload):
    x = np.arange(2 * 3 * 40, dtype=np.float64).reshape(2, 3, 40)
    codes, scales = payload.mx4_quantize(x)
    assert codes.shape == (2, 3, 40) and scales.shape == (2, 3, 2)
    ref_codes, ref_scales = ref_mx4_quantize(x.reshape(6, 40))
    assert np.array_equal(codes.reshape(6, 40), ref_codes)
    assert np.array_equal(scales.reshape(6, 2), ref_scales)
    codes, scales = payload.mx4_quantize(np.ones(5, np.float32))
    assert codes.shape == (5,) and scales.shape == (1,)


def dequantize(payload, codes, scales):
    k = codes.shape[-1]
    s = np.repeat(scales.astype(np.float64), 32, axis=-1)[..., :k]
    return payload.from_e2m1(codes).astype(np.float64) * 2.0 ** (s - 127)


def test_mx4_quantize_reproduces_representable_input(payload):
    rng = np.random.default_rng(9)
    vals = TABLE[rng.integers(0, 16, size=(8, 96))]
    exps = rng.integers(-20, 21, size=(8, 3))
    x = (vals * 2.0 ** np.repeat(exps, 32, axis=1)).astype(np.float32)
    codes, scales = payload.mx4_quantize(x)
    assert np.array_equal(dequantize(payload, codes, scales), x.astype(np.float64))


# ---- CPU: pack_fp4 ----------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 7, 32, 41])
def test_pack_fp4_matches_reference(payload, k):
    codes = np.random.default_rng(k).integers(0, 16, size=(5, k)).astype(np.uint8)
    got = payload.pack_fp4(codes)
    assert got.dtype == np.uint8 and got.shape == (5, (k + 1) // 2)
    assert np.array_equal(got, ref_pack(codes))
    # even k in bits 3:0, odd k in bits 7:4, the odd tail's high nibble zero
    assert (got[:, 0] & 15 == codes[:, 0]).all()
    if k > 1:
        assert (got[:, 0] >> 4 == codes[:, 1]).all()
    if k % 2:
        assert (got[:, -1] >> 4 == 0).all()


def test_pack_fp4_shapes_and_errors(payload):
    codes = np.random.default_rng(3).integers(0, 16, size=(2, 3, 9)).astype(np.uint8)
    got = payload.pack_fp4(codes)
    assert got.shape == (2, 3, 5)
    assert np.array_equal(got, ref_pack(codes))
    assert payload.pack_fp4(np.array([1, 2, 3], np.uint8)).tolist() == [0x21, 0x03]
    with pytest.raises(ValueError):
        payload.pack_fp4(np.array([1, 16], np.uint8))


# ---- CPU: argument errors come before any device work ---------------------

def test_gemm_mxfp4_rejects_bad_arguments(payload):
    f = np.zeros
    with pytest.raises(ValueError):
        payload.gemm_mxfp4(f((2, 3, 4), np.float32), f((4, 2), np.float32))
    with pytest.raises(ValueError):
        payload.gemm_mxfp4(f(3, np.float32), f((3, 2), np.float32))
    with pytest.raises(ValueError):
        payload.gemm_mxfp4(f((2, 3), np.float32), f((4, 2), np.float32))
    with pytest.raises((TypeError, ValueError)):
        payload.gemm_mxfp4("not an array", f((4, 2), np.float32))
    for bad in (np.inf, -np.inf, np.nan):
        a = np.ones((2, 40), np.float32)
        b = np.ones((40, 3), np.float32)
        a[1, 33] = bad
        with pytest.raises(ValueError):
            payload.gemm_mxfp4(a, b)
        with pytest.raises(ValueError):
            payload.gemm_mxfp4(b.T.copy(), a.T.copy())


def test_gemm_mxfp4_raw_rejects_bad_arguments(payload):
    u = lambda *shape: np.zeros(shape, np.uint8)  # noqa: E731
    sixteen_a, sixteen_b = u(4, 40), u(40, 3)
    sixteen_a[3, 39] = 16
    sixteen_b[39, 2] = 16
    bad = [
        (u(4, 40, 1), u(4, 2), u(40, 3), u(2, 3)),   # ndim
        (u(4, 40), u(4, 2), u(40), u(2, 3)),
        (u(4, 40), u(4, 2), u(41, 3), u(2, 3)),      # K differs
        (u(4, 40), u(4, 1), u(40, 3), u(2, 3)),      # a_scales: blocks
        (u(4, 40), u(3, 2), u(40, 3), u(2, 3)),      # a_scales: rows
        (u(4, 40), u(8), u(40, 3), u(2, 3)),         # a_scales: ndim
        (u(4, 40), u(4, 2), u(40, 3), u(3, 2)),      # b_scales transposed
        (u(4, 40), u(4, 2), u(40, 3), u(2, 4)),      # b_scales: columns
        (u(0, 40), u(0, 2), u(40, 3), u(2, 3)),      # empty
        (sixteen_a, u(4, 2), u(40, 3), u(2, 3)),     # a code of 16
        (u(4, 40), u(4, 2), sixteen_b, u(2, 3)),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            payload.gemm_mxfp4_raw(*args)


# ---- CPU: judge_mx4gemm ---------------------------------------------------

def report(**over):
    """What the binary prints for a clean default run."""
    r = {"ok": True, "cmd": "mx4gemm", "m": 4096, "n": 4096, "k": 2048,
         "iters": 10, "tflops": 2345.67, "max_err": 0}
    r.update(over)
    return r


def test_judge_mx4gemm_pass():
    rep = report()
    v = verify.judge_mx4gemm(rep, "cpx-1x36")
    assert v == {"ok": True, "failed": [], "profile": "cpx-1x36", "report": rep}
    # the rate is carried, never judged; the report's own ok is not trusted
    assert verify.judge_mx4gemm(report(tflops=0.0, ok=False), "cpx-1x36")["ok"]
    assert verify.judge_mx4gemm(report(max_err=0.0), "cpx-1x36")["ok"] is True


def test_judge_mx4gemm_non_zero_error():
    for err in (0.0625, 1e300, -1):
        v = verify.judge_mx4gemm(report(ok=True, max_err=err), "cpx-1x36")
        assert v["ok"] is False and v["failed"] == ["mx4gemm"]


@pytest.mark.parametrize("field", ["max_err", "m", "n", "k", "iters"])
def test_judge_mx4gemm_missing_or_non_numeric_field(field):
    rep = report()
    del rep[field]
    assert verify.judge_mx4gemm(rep, "cpx-1x36")["failed"] == ["mx4gemm"]
    for junk in ("0", None, True, False):
        assert verify.judge_mx4gemm(report(**{field: junk}),
                                    "cpx-1x36")["failed"] == ["mx4gemm"]


@pytest.mark.parametrize("field", ["m", "n", "k", "iters"])
def test_judge_mx4gemm_counts_must_be_positive_integers(field):
    for junk in (0, -1, 1.0, 4096.5):
        assert verify.judge_mx4gemm(report(**{field: junk}),
                                    "cpx-1x36")["failed"] == ["mx4gemm"]


def test_judge_mx4gemm_unknown_profile():
    with pytest.raises(ValueError):
        verify.judge_mx4gemm(report(), "not-a-profile")


# ---- CPU: verify.run_mx4gemm with a fake child ------------------------------

def fake_runner(stdout="", returncode=0, raises=None, seen=None):
    def runner(cmd, **kw):
        if seen is not None:
            seen.append((cmd, kw))
        if raises is not None:
            raise raises
        return SimpleNamespace(stdout=stdout, stderr="", returncode=returncode)
    return runner


def test_run_mx4gemm_pass():
    seen = []
    v = verify.run_mx4gemm("cpx-1x36", env={"ROCR_VISIBLE_DEVICES": "GPU-abc"},
                           runner=fake_runner(json.dumps(report()), seen=seen))
    assert v["ok"] is True and v["failed"] == [] and v["profile"] == "cpx-1x36"
    assert v["report"]["tflops"] == 2345.67
    (cmd, kw), = seen
    assert cmd == [verify.BIN_PATH, "mx4gemm"]
    assert kw["env"]["ROCR_VISIBLE_DEVICES"] == "GPU-abc"
    assert kw["timeout"] == verify.CHILD_TIMEOUT_S


def test_run_mx4gemm_unknown_profile_raises():
    seen = []
    with pytest.raises(ValueError):
        verify.run_mx4gemm("bogus",
                           runner=fake_runner(json.dumps(report()), seen=seen))
    assert seen == []


def test_run_mx4gemm_child_failures():
    v = verify.run_mx4gemm("cpx-1x36",
                           runner=fake_runner("Segmentation fault\n", 0))
    assert v["ok"] is False and "non-JSON" in v["reason"]
    v = verify.run_mx4gemm("cpx-1x36", runner=fake_runner("", 0))
    assert v["ok"] is False and "non-JSON" in v["reason"]
    exc = subprocess.TimeoutExpired(cmd="instaslice-payload", timeout=1)
    v = verify.run_mx4gemm("cpx-1x36", runner=fake_runner(raises=exc))
    assert v["ok"] is False and "timed out" in v["reason"]
    v = verify.run_mx4gemm("cpx-1x36",
                           runner=fake_runner(raises=FileNotFoundError()))
    assert v["ok"] is False and "not found" in v["reason"]
    v = verify.run_mx4gemm("cpx-1x36",
                           runner=fake_runner(raises=PermissionError("denied")))
    assert v["ok"] is False and "could not start" in v["reason"]
    # the binary's catch-all line
    err = json.dumps({"ok": False, "error": "HIP error: no ROCm-capable device"})
    v = verify.run_mx4gemm("cpx-1x36", runner=fake_runner(err, 1))
    assert v["ok"] is False and v["failed"] == []
    assert "no ROCm-capable device" in v["reason"] and "exit 1" in v["reason"]
    # a failing report is judged, and the exit status is carried
    rep = report(ok=False, max_err=0.0625)
    v = verify.run_mx4gemm("cpx-1x36", runner=fake_runner(json.dumps(rep), 1))
    assert v["ok"] is False and v["failed"] == ["mx4gemm"]
    assert "exited 1" in v["reason"]
    # clean-looking fields do not outvote a non-zero exit
    v = verify.run_mx4gemm("cpx-1x36", runner=fake_runner(json.dumps(report()), 1))
    assert v["ok"] is False and "exited 1" in v["reason"]
    # nor does a clean exit outvote a non-zero error
    v = verify.run_mx4gemm("cpx-1x36", runner=fake_runner(json.dumps(rep), 0))
    assert v["ok"] is False and v["failed"] == ["mx4gemm"]


def test_run_mx4gemm_missing_binary_real_subprocess(monkeypatch, tmp_path):
    monkeypatch.setattr(verify, "BIN_PATH", str(tmp_path / "no-such-binary"))
    v = verify.run_mx4gemm("cpx-1x36")
    assert v["ok"] is False and "not found" in v["reason"]


# ---- CPU: the CLI command -------------------------------------------------

def _patch_runner(monkeypatch, runner):
    real = verify.run_mx4gemm
    monkeypatch.setattr(
        verify, "run_mx4gemm",
        lambda profile, **kw: real(profile, runner=runner, **kw))


def test_cli_mx4gemm_ok(monkeypatch, capsys):
    from instaslice_amd.cli import main

    seen = []
    _patch_runner(monkeypatch, fake_runner(json.dumps(report()), seen=seen))
    rc = main(["mx4gemm", "--profile", "cpx-1x36", "--visible-devices", "3"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 0 and out["ok"] is True and out["profile"] == "cpx-1x36"
    assert seen[0][0][1:] == ["mx4gemm"]
    assert seen[0][1]["env"]["ROCR_VISIBLE_DEVICES"] == "3"


def test_cli_mx4gemm_fail(monkeypatch, capsys):
    from instaslice_amd.cli import main

    rep = report(ok=False, max_err=2.0)
    _patch_runner(monkeypatch, fake_runner(json.dumps(rep), 1))
    rc = main(["mx4gemm", "--profile", "cpx-1x36"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 1 and out["ok"] is False and out["failed"] == ["mx4gemm"]


def test_cli_mx4gemm_bad_profile(monkeypatch, capsys):
    from instaslice_amd.cli import main

    _patch_runner(monkeypatch, fake_runner(json.dumps(report())))
    rc = main(["mx4gemm", "--profile", "bogus"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 1 and out["ok"] is False and "bogus" in out["reason"]
    assert out["report"] is None


# ---- GPU: the kernel through the raw entry ---------------------------------

ONE = 2  # 1.0 in e2m1

SHAPES = [
    (16, 16, 128),     # one MFMA
    (1, 1, 1),         # everything is padding
    (33, 17, 41),      # ragged everywhere, a partial block, a padded nibble
    (64, 64, 512),     # several K-steps
    (96, 160, 224),    # several workgroups on both axes
    (130, 70, 448),    # the K limit of this pattern, ragged, multi-tile
]


def expand(scales, k, axis):
    """One value per element from one value per 32-element block."""
    return np.take(np.repeat(scales, 32, axis=axis), np.arange(k), axis=axis)


# Both scale arrays are random here, so every shape with more than one block
# also covers the case where neither side is all-127.
@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_gemm_mxfp4_raw_exact_vs_numpy_all_codes(payload, m, n, k):
    rng = np.random.default_rng(1000 * m + 10 * n + k)
    blocks = -(-k // 32)
    a = rng.integers(0, 16, size=(m, k)).astype(np.uint8)
    b = rng.integers(0, 16, size=(k, n)).astype(np.uint8)
    sa = rng.integers(125, 130, size=(m, blocks))
    sb = rng.integers(125, 130, size=(blocks, n))
    out = payload.gemm_mxfp4_raw(a, sa.astype(np.uint8), b, sb.astype(np.uint8))
    # int64 in units of 2^-6: each side in units of 2^-3
    a2 = np.round(2 * TABLE[a]).astype(np.int64) << (expand(sa, k, 1) - 125)
    b2 = np.round(2 * TABLE[b]).astype(np.int64) << (expand(sb, k, 0) - 125)
    units = a2 @ b2
    # the sum of the terms' magnitudes bounds every partial sum in any order
    assert k <= 455 or (np.abs(a2) @ np.abs(b2)).max() <= 2 ** 24
    ref = (units.astype(np.float64) / 64).astype(np.float32)
    assert out.dtype == np.float32 and out.shape == (m, n)
    assert np.array_equal(out, ref)


@pytest.mark.gpu
def test_gemm_mxfp4_one_hot_a_pins_k_and_nibble_order(payload):
    perm = np.random.default_rng(7).permutation(256)
    a = np.zeros((256, 256), dtype=np.uint8)
    a[np.arange(256), perm] = ONE
    # codes 0..7, asymmetric; columns 0, 1, 2 spell the row index in base 8
    # (two digits and a top digit 0..3), so every row is different
    k, j = np.arange(256)[:, None], np.arange(48)[None, :]
    b = (3 * k + 5 * j + (k >> 3)) % 8
    b[:, 0], b[:, 1], b[:, 2] = (np.arange(256) & 7, (np.arange(256) >> 3) & 7,
                                 np.arange(256) >> 6)
    assert len(np.unique(b, axis=0)) == 256
    assert b.shape[0] != b.shape[1] and b.max() == 7
    b = b.astype(np.uint8)
    out = payload.gemm_mxfp4_raw(a, np.full((256, 8), 127, np.uint8),
                                 b, np.full((8, 48), 127, np.uint8))
    assert np.array_equal(out, TABLE[b][perm].astype(np.float32))


def _scale_exp_a(row, block):
    return (3 * row + block) % 5 - 2


def _scale_exp_b(block, col):
    return (block + 3 * col) % 5 - 2


@pytest.mark.gpu
def test_gemm_mxfp4_scale_block_map_a_side(payload):
    m, n, k = 80, 512, 512
    ea = _scale_exp_a(np.arange(m)[:, None], np.arange(k // 32)[None, :])
    assert (ea[:, 1:] != ea[:, :-1]).all() and (ea[1:] != ea[:-1]).all()
    ksel = np.random.default_rng(21).permutation(k)  # column j selects k = ksel[j]
    b = np.zeros((k, n), dtype=np.uint8)
    b[ksel, np.arange(n)] = ONE
    out = payload.gemm_mxfp4_raw(
        np.full((m, k), ONE, np.uint8), (127 + ea).astype(np.uint8),
        b, np.full((k // 32, n), 127, np.uint8))
    assert np.array_equal(out, (2.0 ** ea[:, ksel // 32]).astype(np.float32))


@pytest.mark.gpu
def test_gemm_mxfp4_scale_block_map_b_side(payload):
    m, n, k = 512, 80, 512
    eb = _scale_exp_b(np.arange(k // 32)[:, None], np.arange(n)[None, :])
    assert (eb[1:] != eb[:-1]).all() and (eb[:, 1:] != eb[:, :-1]).all()
    ksel = np.random.default_rng(22).permutation(k)  # row i selects k = ksel[i]
    a = np.zeros((m, k), dtype=np.uint8)
    a[np.arange(m), ksel] = ONE
    out = payload.gemm_mxfp4_raw(
        a, np.full((m, k // 32), 127, np.uint8),
        np.full((k, n), ONE, np.uint8), (127 + eb).astype(np.uint8))
    assert np.array_equal(out, (2.0 ** eb[ksel // 32, :]).astype(np.float32))


@pytest.mark.gpu
def test_gemm_mxfp4_quantized_input_numerics(payload):
    """|C - ref| <= K * 2^-23 * (|Aq| @ |Bq|) elementwise, ref in float64 on
    the dequantized operands (mx4_quantize + from_e2m1). Derived, not
    measured, as for MXFP8: products of two e2m1 values and power-of-two
    scalings are exact in fp32 and each of the K accumulations adds at most
    one fp32 ulp of the magnitude sum (2^-23 rather than 2^-24 allows a
    truncating adder)."""
    m, n, k = 96, 160, 224
    rng = np.random.default_rng(11)
    a = rng.uniform(-1, 1, size=(m, k)).astype(np.float32)
    b = rng.uniform(-1, 1, size=(k, n)).astype(np.float32)
    aq = dequantize(payload, *payload.mx4_quantize(a))
    bq = dequantize(payload, *payload.mx4_quantize(np.ascontiguousarray(b.T))).T
    out = payload.gemm_mxfp4(a, b).astype(np.float64)
    ref = aq @ bq
    bound = k * 2.0 ** -23 * (np.abs(aq) @ np.abs(bq))
    err = np.abs(out - ref)
    print(f"\nmax |err| / bound = {(err / bound).max():.4f}, "
          f"max |err| = {err.max():.3e}, "
          f"max |ref - fp32 product| = {np.abs(ref - a.astype(np.float64) @ b).max():.3e}")
    assert out.shape == (m, n)
    assert (err <= bound).all()


@pytest.mark.gpu
def test_run_mx4gemm_check_exact(payload):
    assert payload.run_mx4gemm_check(130, 70, 2048) == 0.0
    assert payload.run_mx4gemm_check(96, 160, 224) == 0.0


@pytest.mark.gpu
def test_run_mx4gemm_check_rejects_k_above_limit(payload):
    with pytest.raises(ValueError):
        payload.run_mx4gemm_check(64, 64, 4096)
    with pytest.raises(ValueError):
        payload.run_mx4gemm(64, 64, 4096, iters=1)


@pytest.mark.gpu
def test_run_mx4gemm_timed(payload):
    r = payload.run_mx4gemm(1024, 1024, 512, iters=3)
    print(f"\nrun_mx4gemm 1024x1024x512: {r['tflops']:.1f} TFLOP/s")
    assert (r["m"], r["n"], r["k"], r["iters"]) == (1024, 1024, 512, 3)
    assert r["max_err"] == 0.0
    assert np.isfinite(r["tflops"]) and r["tflops"] > 0


# ---- GPU: the binary ------------------------------------------------------

def run_bin(*args):
    out = subprocess.run([BIN, *args], capture_output=True, text=True,
                         timeout=120)
    return out.returncode, json.loads(out.stdout), out


@pytest.mark.gpu
def test_binary_mx4gemm():
    rc, res, out = run_bin("mx4gemm", "96", "160", "224", "1")
    assert rc == 0, out.stdout + out.stderr
    assert set(res) == {"ok", "cmd", "m", "n", "k", "iters", "tflops", "max_err"}
    assert res["ok"] is True and res["cmd"] == "mx4gemm" and res["max_err"] == 0
    assert (res["m"], res["n"], res["k"], res["iters"]) == (96, 160, 224, 1)
    assert res["tflops"] > 0


@pytest.mark.gpu
def test_serve_mx4gemm():
    w = subprocess.Popen([BIN, "serve"], stdin=subprocess.PIPE,
                         stdout=subprocess.PIPE, text=True, bufsize=1)
    try:
        out, _ = w.communicate("mx4gemm 128 128 128\nping\nquit\n", timeout=60)
    finally:
        if w.poll() is None:
            w.kill()
    mx, ping, quit_ = [json.loads(ln) for ln in out.splitlines()]
    assert set(mx) == {"ok", "cmd", "m", "n", "k", "max_err"}
    assert mx["ok"] is True and mx["cmd"] == "mx4gemm" and mx["max_err"] == 0
    assert (mx["m"], mx["n"], mx["k"]) == (128, 128, 128)
    assert ping == {"ok": True, "cmd": "ping"}
    assert quit_ == {"ok": True}


@pytest.mark.gpu
def test_run_mx4gemm_judges_the_real_partition():
    """ops/verify.run_mx4gemm end to end, against the profile matching this
    device: the only run at the default shape."""
    from instaslice_amd.partition.profiles import mi355x_catalog

    rc, census, out = run_bin("census")
    assert rc == 0, out.stdout + out.stderr
    xcds = census["xcds_visible"]
    name = next(p.name for p in mi355x_catalog().profiles if p.xcds == xcds)
    v = verify.run_mx4gemm(name)
    print(f"\nrun_mx4gemm({name}): {v}")
    assert v["ok"] is True and v["failed"] == [] and v["profile"] == name
    rep = v["report"]
    assert (rep["m"], rep["n"], rep["k"], rep["iters"]) == (4096, 4096, 2048, 10)
    assert rep["max_err"] == 0 and rep["tflops"] > 0
