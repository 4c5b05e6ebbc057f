"""The MXFP8 block-scaled MFMA GEMM payload (ops/csrc/payload_mxgemm.hpp): the
e4m3 conversion, the MX quantizer, argument checks, the judge, the runner and
the CLI on CPU; the kernel, its bindings, the binary's `mxgemm` verb and
`verify.run_mxgemm` on a real MI355X.

The formats are re-implemented here in numpy from their definitions,
independently of the header:

    e4m3fn byte: 1 sign, 4 exponent (bias 7), 3 mantissa bits. Exponent 0 is
    subnormal (m * 2^-9), exponent 15 with mantissa 7 is NaN, everything else
    (1 + m/8) * 2^(e - 7); the largest finite value is 448 (0x7E).
    Conversion: the nearest of the 127 non-negative finite values, a tie to
    the even code, anything beyond 448 to 448.

    MX block (32 elements): scale byte = clamp(floor(log2(amax)) - 8 + 127,
    0, 254), 127 for an all-zero block; elements = e4m3(x / 2^(scale - 127)).

Integer elements in [-4, 4] with scales 2^-2 .. 2^2 make every product a
multiple of 2^-4 of magnitude <= 2^8, so any partial sum over K <= 2048 terms
is an integer below 2^24 in units of 2^-4 and the correct fp32 result is
bit-exact in any accumulation order: those tests compare with tolerance 0.
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

def _e4m3_table():
    t = np.empty(256, dtype=np.float64)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = np.nan
        elif e == 0:
            v = m * 2.0 ** -9
        else:
            v = (1 + m / 8) * 2.0 ** (e - 7)
        t[c] = -v if c & 0x80 else v
    return t


TABLE = _e4m3_table()
POS = TABLE[:0x7F]  # the non-negative finite values, ascending: 0 .. 448


def ref_to_e4m3(x):
    """Nearest e4m3 code of each element of x (float64 arithmetic, exact for
    float32 inputs), ties to the even code, saturating; NaN -> 0x7F | sign."""
    x = np.asarray(x, dtype=np.float64)
    ax = np.abs(x)
    finite = np.where(np.isnan(ax), 0.0, ax)
    hi = np.clip(np.searchsorted(POS, finite, side="left"), 0, 0x7E)
    lo = np.clip(hi - 1, 0, 0x7E)
    dlo, dhi = finite - POS[lo], POS[hi] - finite
    code = np.where(dlo < dhi, lo,
                    np.where(dhi < dlo, hi, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(np.isnan(ax), 0x7F, code)
    return (code | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


def ref_mx_quantize(x):
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
                s = int(np.clip((e - 1) - 8 + 127, 0, 254))
            scales[r, b] = s
            codes[r, 32 * b:32 * b + 32] = ref_to_e4m3(seg * 2.0 ** (127 - s))
    return codes, scales


def test_reference_table_landmarks():
    assert TABLE[0x38] == 1.0 and TABLE[0x7E] == 448.0 and TABLE[0xFE] == -448.0
    assert TABLE[0x01] == 2.0 ** -9 and TABLE[0x08] == 2.0 ** -6
    assert np.isnan(TABLE[0x7F]) and np.isnan(TABLE[0xFF])
    assert (np.diff(POS) > 0).all()


def torch_e4m3_bits(x):
    import torch

    return (torch.tensor(np.ascontiguousarray(x, dtype=np.float32))
            .to(torch.float8_e4m3fn).view(torch.uint8).numpy())


# ---- CPU: to_e4m3 / from_e4m3 ---------------------------------------------

def test_to_e4m3_matches_torch_on_normals(payload):
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    x = (x / np.abs(x).max() * 448).astype(np.float32)
    assert np.abs(x).max() <= 448
    got = payload.to_e4m3(x)
    assert got.dtype == np.uint8 and got.shape == x.shape
    assert np.array_equal(got, torch_e4m3_bits(x))
    assert np.array_equal(got, ref_to_e4m3(x))
    # the same draw three decades down: mostly subnormals of e4m3
    small = (x * 2.0 ** -14).astype(np.float32)
    assert np.array_equal(payload.to_e4m3(small), torch_e4m3_bits(small))
    assert np.array_equal(payload.to_e4m3(small), ref_to_e4m3(small))


def test_to_e4m3_edge_values(payload):
    just_above = np.nextafter(np.float32(2.0 ** -10), np.float32(1))
    x = np.array([0.0, -0.0, 1.0, 448.0, 464.0, 2.0 ** -9, 2.0 ** -10,
                  just_above, 2.0 ** -6, 17.0, 18.0, 19.0], dtype=np.float32)
    got = payload.to_e4m3(x)
    assert np.array_equal(got, torch_e4m3_bits(x))
    assert np.array_equal(got, ref_to_e4m3(x))
    assert list(got) == [0x00, 0x80, 0x38, 0x7E, 0x7E, 0x01, 0x00, 0x01, 0x08,
                         0x58, 0x59, 0x5A]
    assert np.array_equal(payload.to_e4m3(-x), got ^ 0x80)


def test_to_e4m3_saturates_beyond_torchs_range(payload):
    x = np.array([480.0, 1e9, np.inf], dtype=np.float32)
    assert list(payload.to_e4m3(x)) == [0x7E] * 3
    assert list(payload.to_e4m3(-x)) == [0xFE] * 3


def test_to_e4m3_nan_stays_nan(payload):
    x = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF],
                 dtype=np.uint32).view(np.float32)
    got = payload.to_e4m3(x)
    assert list(got) == [0x7F, 0xFF, 0x7F, 0x7F]
    assert np.isnan(payload.from_e4m3(got)).all()


def test_to_e4m3_keeps_shape_and_converts_input(payload):
    x = np.arange(12, dtype=np.float64).reshape(3, 4)[:, ::2]  # f64, strided
    got = payload.to_e4m3(x)
    assert got.shape == (3, 2)
    assert np.array_equal(got, ref_to_e4m3(np.ascontiguousarray(x)))


def test_from_e4m3_is_the_table(payload):
    codes = np.arange(256, dtype=np.uint8)
    got = payload.from_e4m3(codes)
    assert got.dtype == np.float32 and got.shape == (256,)
    assert np.isnan(got[0x7F]) and np.isnan(got[0xFF])
    keep = ~np.isnan(TABLE)
    assert keep.sum() == 254
    assert np.array_equal(got[keep].astype(np.float64), TABLE[keep])
    assert np.signbit(got[0x80]) and got[0x80] == 0
    assert payload.from_e4m3(codes.reshape(16, 16)).shape == (16, 16)


# ---- CPU: mx_quantize -----------------------------------------------------

@pytest.mark.parametrize("k", [32, 40, 128])
def test_mx_quantize_random_rows(payload, k):
    rng = np.random.default_rng(k)
    # rows of very different magnitude, so scales differ from row to row
    x = (rng.standard_normal((6, k)) *
         (10.0 ** rng.integers(-6, 7, size=(6, 1)))).astype(np.float32)
    codes, scales = payload.mx_quantize(x)
    assert codes.dtype == np.uint8 and codes.shape == (6, k)
    assert scales.dtype == np.uint8 and scales.shape == (6, -(-k // 32))
    ref_codes, ref_scales = ref_mx_quantize(x)
    assert np.array_equal(scales, ref_scales)
    assert np.array_equal(codes, ref_codes)


def test_mx_quantize_special_blocks(payload):
    rng = np.random.default_rng(5)
    base = rng.uniform(-1, 1, size=32).astype(np.float32)
    base[7] = 1.0  # amax of `base` is exactly 1
    rows = np.stack([
        base * 4,                        # amax an exact power of two
        np.zeros(32, np.float32),        # all zero: scale 127
        base * np.float32(1.9),          # scaled amax in (448, 512): saturates
        base * np.float32(2.0 ** -125),  # the scale clamps at 0
        base * np.float32(1e-40),        # fp32 subnormals, clamped as well
    ]).astype(np.float32)
    rows[1, 3] = -0.0
    codes, scales = payload.mx_quantize(rows)
    ref_codes, ref_scales = ref_mx_quantize(rows)
    assert np.array_equal(scales, ref_scales)
    assert np.array_equal(codes, ref_codes)
    assert list(scales[:, 0]) == [2 - 8 + 127, 127, 0 - 8 + 127, 0, 0]
    assert codes[0, 7] == 0x78           # 4 / 2^-6 = 256
    assert codes[1, 3] == 0x80 and not codes[1, :3].any()
    assert codes[2, 7] == 0x7E           # 1.9 * 256 = 486.4 -> 448
    assert codes[3, 7] == 0x48           # 2^-125 * 2^127 = 4


def test_mx_quantize_shapes(payload):
    x = np.arange(2 * 3 * 40, dtype=np.float64).reshape(2, 3, 40)
    codes, scales = payload.mx_quantize(x)
    assert codes.shape == (2, 3, 40) and scales.shape == (2, 3, 2)
    ref_codes, ref_scales = ref_mx_quantize(x.reshape(6, 40))
    assert np.array_equal(codes.reshape(6, 40), ref_codes)
    assert np.array_equal(scales.reshape(6, 2), ref_scales)
    codes, scales = payload.mx_quantize(np.ones(5, np.float32))
    assert codes.shape == (5,) and scales.shape == (1,)


def dequantize(payload, codes, scales):
    k = codes.shape[-1]
    s = np.repeat(scales.astype(np.float64), 32, axis=-1)[..., :k]
    return payload.from_e4m3(codes).astype(np.float64) * 2.0 ** (s - 127)


def test_mx_quantize_reproduces_representable_input(payload):
    rng = np.random.default_rng(9)
    ints = rng.integers(-4, 5, size=(8, 96)).astype(np.float64)
    exps = rng.integers(-20, 21, size=(8, 3))
    x = (ints * 2.0 ** np.repeat(exps, 32, axis=1)).astype(np.float32)
    codes, scales = payload.mx_quantize(x)
    assert np.array_equal(dequantize(payload, codes, scales), x.astype(np.float64))


# ---- CPU: argument errors come before any device work ---------------------

def test_gemm_mxfp8_rejects_bad_arguments(payload):
    f = np.zeros
    with pytest.raises(ValueError):
        payload.gemm_mxfp8(f((2, 3, 4), np.float32), f((4, 2), np.float32))
    with pytest.raises(ValueError):
        payload.gemm_mxfp8(f(3, np.float32), f((3, 2), np.float32))
    with pytest.raises(ValueError):
        payload.gemm_mxfp8(f((2, 3), np.float32), f((4, 2), np.float32))
    with pytest.raises((TypeError, ValueError)):
        payload.gemm_mxfp8("not an array", f((4, 2), np.float32))
    for bad in (np.inf, -np.inf, np.nan):
        a = np.ones((2, 40), np.float32)
        b = np.ones((40, 3), np.float32)
        a[1, 33] = bad
        with pytest.raises(ValueError):
            payload.gemm_mxfp8(a, b)
        with pytest.raises(ValueError):
            payload.gemm_mxfp8(b.T.copy(), a.T.copy())


def test_gemm_mxfp8_raw_rejects_bad_arguments(payload):
    u = lambda *shape: np.zeros(shape, np.uint8)  # noqa: E731
    good = (u(4, 40), u(4, 2), u(40, 3), u(2, 3))
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
    ]
    assert len(good) == 4
    for args in bad:
        with pytest.raises(ValueError):
            payload.gemm_mxfp8_raw(*args)


# ---- CPU: judge_mxgemm ----------------------------------------------------

def report(**over):
    """What the binary prints for a clean default run."""
    r = {"ok": True, "cmd": "mxgemm", "m": 4096, "n": 4096, "k": 2048,
         "iters": 10, "tflops": 1234.56, "max_err": 0}
    r.update(over)
    return r


def test_judge_mxgemm_pass():
    rep = report()
    v = verify.judge_mxgemm(rep, "cpx-1x36")
    assert v == {"ok": True, "failed": [], "profile": "cpx-1x36", "report": rep}
    # the rate is carried, never judged; the report's own ok is not trusted
    assert verify.judge_mxgemm(report(tflops=0.0, ok=False), "cpx-1x36")["ok"]
    assert verify.judge_mxgemm(report(max_err=0.0), "cpx-1x36")["ok"] is True


def test_judge_mxgemm_non_zero_error():
    for err in (0.0625, 1e300, -1):
        v = verify.judge_mxgemm(report(ok=True, max_err=err), "cpx-1x36")
        assert v["ok"] is False and v["failed"] == ["mxgemm"]


@pytest.mark.parametrize("field", ["max_err", "m", "n", "k", "iters"])
def test_judge_mxgemm_missing_or_non_numeric_field(field):
    rep = report()
    del rep[field]
    assert verify.judge_mxgemm(rep, "cpx-1x36")["failed"] == ["mxgemm"]
    for junk in ("0", None, True, False):
        assert verify.judge_mxgemm(report(**{field: junk}),
                                   "cpx-1x36")["failed"] == ["mxgemm"]


@pytest.mark.parametrize("field", ["m", "n", "k", "iters"])
def test_judge_mxgemm_counts_must_be_positive_integers(field):
    for junk in (0, -1, 1.0, 4096.5):
        assert verify.judge_mxgemm(report(**{field: junk}),
                                   "cpx-1x36")["failed"] == ["mxgemm"]


def test_judge_mxgemm_unknown_profile():
    with pytest.raises(ValueError):
        verify.judge_mxgemm(report(), "not-a-profile")


# ---- CPU: verify.run_mxgemm with a fake child ------------------------------

def fake_runner(stdout="", returncode=0, raises=None, seen=None):
    def runner(cmd, **kw):
        if seen is not None:
            seen.append((cmd, kw))
        if raises is not None:
            raise raises
        return SimpleNamespace(stdout=stdout, stderr="", returncode=returncode)
    return runner


def test_run_mxgemm_pass():
    seen = []
    v = verify.run_mxgemm("cpx-1x36", env={"ROCR_VISIBLE_DEVICES": "GPU-abc"},
                          runner=fake_runner(json.dumps(report()), seen=seen))
    assert v["ok"] is True and v["failed"] == [] and v["profile"] == "cpx-1x36"
    assert v["report"]["tflops"] == 1234.56
    (cmd, kw), = seen
    assert cmd == [verify.BIN_PATH, "mxgemm"]
    assert kw["env"]["ROCR_VISIBLE_DEVICES"] == "GPU-abc"
    assert kw["timeout"] == verify.CHILD_TIMEOUT_S


def test_run_mxgemm_unknown_profile_raises():
    seen = []
    with pytest.raises(ValueError):
        verify.run_mxgemm("bogus",
                          runner=fake_runner(json.dumps(report()), seen=seen))
    assert seen == []


def test_run_mxgemm_child_failures():
    v = verify.run_mxgemm("cpx-1x36",
                          runner=fake_runner("Segmentation fault\n", 0))
    assert v["ok"] is False and "non-JSON" in v["reason"]
    v = verify.run_mxgemm("cpx-1x36", runner=fake_runner("", 0))
    assert v["ok"] is False and "non-JSON" in v["reason"]
    exc = subprocess.TimeoutExpired(cmd="instaslice-payload", timeout=1)
    v = verify.run_mxgemm("cpx-1x36", runner=fake_runner(raises=exc))
    assert v["ok"] is False and "timed out" in v["reason"]
    v = verify.run_mxgemm("cpx-1x36",
                          runner=fake_runner(raises=FileNotFoundError()))
    assert v["ok"] is False and "not found" in v["reason"]
    v = verify.run_mxgemm("cpx-1x36",
                          runner=fake_runner(raises=PermissionError("denied")))
    assert v["ok"] is False and "could not start" in v["reason"]
    # the binary's catch-all line
    err = json.dumps({"ok": False, "error": "HIP error: no ROCm-capable device"})
    v = verify.run_mxgemm("cpx-1x36", runner=fake_runner(err, 1))
    assert v["ok"] is False and v["failed"] == []
    assert "no ROCm-capable device" in v["reason"] and "exit 1" in v["reason"]
    # a failing report is judged, and the exit status is carried
    rep = report(ok=False, max_err=0.0625)
    v = verify.run_mxgemm("cpx-1x36", runner=fake_runner(json.dumps(rep), 1))
    assert v["ok"] is False and v["failed"] == ["mxgemm"]
    assert "exited 1" in v["reason"]
    # clean-looking fields do not outvote a non-zero exit
    v = verify.run_mxgemm("cpx-1x36", runner=fake_runner(json.dumps(report()), 1))
    assert v["ok"] is False and "exited 1" in v["reason"]
    # nor does a clean exit outvote a non-zero error
    v = verify.run_mxgemm("cpx-1x36", runner=fake_runner(json.dumps(rep), 0))
    assert v["ok"] is False and v["failed"] == ["mxgemm"]


def test_run_mxgemm_missing_binary_real_subprocess(monkeypatch, tmp_path):
    monkeypatch.setattr(verify, "BIN_PATH", str(tmp_path / "no-such-binary"))
    v = verify.run_mxgemm("cpx-1x36")
    assert v["ok"] is False and "not found" in v["reason"]


# ---- CPU: the CLI command -------------------------------------------------

def _patch_runner(monkeypatch, runner):
    real = verify.run_mxgemm
    monkeypatch.setattr(
        verify, "run_mxgemm",
        lambda profile, **kw: real(profile, runner=runner, **kw))


def test_cli_mxgemm_ok(monkeypatch, capsys):
    from instaslice_amd.cli import main

    seen = []
    _patch_runner(monkeypatch, fake_runner(json.dumps(report()), seen=seen))
    rc = main(["mxgemm", "--profile", "cpx-1x36", "--visible-devices", "3"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 0 and out["ok"] is True and out["profile"] == "cpx-1x36"
    assert seen[0][0][1:] == ["mxgemm"]
    assert seen[0][1]["env"]["ROCR_VISIBLE_DEVICES"] == "3"


def test_cli_mxgemm_fail(monkeypatch, capsys):
    from instaslice_amd.cli import main

    rep = report(ok=False, max_err=2.0)
    _patch_runner(monkeypatch, fake_runner(json.dumps(rep), 1))
    rc = main(["mxgemm", "--profile", "cpx-1x36"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 1 and out["ok"] is False and out["failed"] == ["mxgemm"]


def test_cli_mxgemm_bad_profile(monkeypatch, capsys):
    from instaslice_amd.cli import main

    _patch_runner(monkeypatch, fake_runner(json.dumps(report())))
    rc = main(["mxgemm", "--profile", "bogus"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 1 and out["ok"] is False and "bogus" in out["reason"]
    assert out["report"] is None


# ---- GPU: the kernel through the raw entry ---------------------------------

ONE = 0x38  # 1.0 in e4m3

SHAPES = [
    (16, 16, 128),     # one MFMA
    (1, 1, 1),         # everything is padding
    (33, 17, 40),      # ragged in every dimension, a partial MX block
    (64, 64, 256),     # several K-steps
    (96, 160, 224),    # several workgroups on both axes
    (130, 70, 2048),   # the K limit, ragged, multi-tile
]


def expand(scales, k, axis):
    """One value per element from one value per 32-element block."""
    return np.take(np.repeat(scales, 32, axis=axis), np.arange(k), axis=axis)


# Both scale arrays are random here, so every shape with more than one block
# also covers the case where neither side is all-127.
@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_gemm_mxfp8_raw_exact_vs_numpy(payload, m, n, k):
    rng = np.random.default_rng(1000 * m + 10 * n + k)
    blocks = -(-k // 32)
    a = rng.integers(-4, 5, size=(m, k))
    b = rng.integers(-4, 5, size=(k, n))
    sa = rng.integers(125, 130, size=(m, blocks))
    sb = rng.integers(125, 130, size=(blocks, n))
    out = payload.gemm_mxfp8_raw(
        payload.to_e4m3(a.astype(np.float32)), sa.astype(np.uint8),
        payload.to_e4m3(b.astype(np.float32)), sb.astype(np.uint8))
    # int64 in units of 2^-4: each side in units of 2^-2
    a4 = a.astype(np.int64) << (expand(sa, k, 1) - 125)
    b4 = b.astype(np.int64) << (expand(sb, k, 0) - 125)
    ref = ((a4 @ b4).astype(np.float64) / 16).astype(np.float32)
    assert out.dtype == np.float32 and out.shape == (m, n)
    assert np.array_equal(out, ref)


@pytest.mark.gpu
def test_gemm_mxfp8_one_hot_a_pins_k_order(payload):
    perm = np.random.default_rng(7).permutation(128)
    a = np.zeros((128, 128), dtype=np.uint8)
    a[np.arange(128), perm] = ONE
    # integers 0..15 (exact in e4m3), asymmetric; columns 0 and 1 spell the
    # row index in base 16, so every row is different
    k, j = np.arange(128)[:, None], np.arange(48)[None, :]
    b = (7 * k + 11 * j + (k >> 3)) % 16
    b[:, 0], b[:, 1] = np.arange(128) & 15, np.arange(128) >> 4
    assert len(np.unique(b, axis=0)) == 128
    assert b.shape[0] != b.shape[1]
    b = b.astype(np.float32)
    codes = payload.to_e4m3(b)
    assert np.array_equal(payload.from_e4m3(codes), b)
    out = payload.gemm_mxfp8_raw(a, np.full((128, 4), 127, np.uint8),
                                 codes, np.full((4, 48), 127, np.uint8))
    assert np.array_equal(out, b[perm])


def _scale_exp_a(row, block):
    return (3 * row + block) % 5 - 2


def _scale_exp_b(block, col):
    return (block + 3 * col) % 5 - 2


@pytest.mark.gpu
def test_gemm_mxfp8_scale_block_map_a_side(payload):
    m, n, k = 80, 256, 256
    ea = _scale_exp_a(np.arange(m)[:, None], np.arange(k // 32)[None, :])
    assert (ea[:, 1:] != ea[:, :-1]).all() and (ea[1:] != ea[:-1]).all()
    ksel = np.random.default_rng(21).permutation(k)  # column j selects k = ksel[j]
    b = np.zeros((k, n), dtype=np.uint8)
    b[ksel, np.arange(n)] = ONE
    out = payload.gemm_mxfp8_raw(
        np.full((m, k), ONE, np.uint8), (127 + ea).astype(np.uint8),
        b, np.full((k // 32, n), 127, np.uint8))
    assert np.array_equal(out, (2.0 ** ea[:, ksel // 32]).astype(np.float32))


@pytest.mark.gpu
def test_gemm_mxfp8_scale_block_map_b_side(payload):
    m, n, k = 256, 80, 256
    eb = _scale_exp_b(np.arange(k // 32)[:, None], np.arange(n)[None, :])
    assert (eb[1:] != eb[:-1]).all() and (eb[:, 1:] != eb[:, :-1]).all()
    ksel = np.random.default_rng(22).permutation(k)  # row i selects k = ksel[i]
    a = np.zeros((m, k), dtype=np.uint8)
    a[np.arange(m), ksel] = ONE
    out = payload.gemm_mxfp8_raw(
        a, np.full((m, k // 32), 127, np.uint8),
        np.full((k, n), ONE, np.uint8), (127 + eb).astype(np.uint8))
    assert np.array_equal(out, (2.0 ** eb[ksel // 32, :]).astype(np.float32))


@pytest.mark.gpu
def test_gemm_mxfp8_quantized_input_numerics(payload):
    """|C - ref| <= K * 2^-23 * (|Aq| @ |Bq|) elementwise, ref in float64 on
    the dequantized operands (mx_quantize + from_e4m3). Derived, not measured:
    products of two e4m3 values and power-of-two scalings are exact in fp32
    and each of the K accumulations adds at most one fp32 ulp of the magnitude
    sum (2^-23 rather than 2^-24 allows a truncating adder)."""
    m, n, k = 96, 160, 224
    rng = np.random.default_rng(11)
    a = rng.uniform(-1, 1, size=(m, k)).astype(np.float32)
    b = rng.uniform(-1, 1, size=(k, n)).astype(np.float32)
    aq = dequantize(payload, *payload.mx_quantize(a))
    bq = dequantize(payload, *payload.mx_quantize(np.ascontiguousarray(b.T))).T
    out = payload.gemm_mxfp8(a, b).astype(np.float64)
    ref = aq @ bq
    bound = k * 2.0 ** -23 * (np.abs(aq) @ np.abs(bq))
    err = np.abs(out - ref)
    print(f"\nmax |err| / bound = {(err / bound).max():.4f}, "
          f"max |err| = {err.max():.3e}, "
          f"max |ref - fp32 product| = {np.abs(ref - a.astype(np.float64) @ b).max():.3e}")
    assert out.shape == (m, n)
    assert (err <= bound).all()


@pytest.mark.gpu
def test_run_mxgemm_check_exact(payload):
    assert payload.run_mxgemm_check(96, 160, 224) == 0.0


@pytest.mark.gpu
def test_run_mxgemm_check_rejects_k_above_limit(payload):
    with pytest.raises(ValueError):
        payload.run_mxgemm_check(64, 64, 4096)
    with pytest.raises(ValueError):
        payload.run_mxgemm(64, 64, 4096, iters=1)


@pytest.mark.gpu
def test_run_mxgemm_timed(payload):
    r = payload.run_mxgemm(1024, 1024, 512, iters=3)
    print(f"\nrun_mxgemm 1024x1024x512: {r['tflops']:.1f} TFLOP/s")
    assert (r["m"], r["n"], r["k"], r["iters"]) == (1024, 1024, 512, 3)
    assert r["max_err"] == 0.0
    assert np.isfinite(r["tflops"]) and r["tflops"] > 0


# ---- GPU: the binary ------------------------------------------------------

def run_bin(*args):
    out = subprocess.run([BIN, *args], capture_output=True, text=True,
                         timeout=120)
    return out.returncode, json.loads(out.stdout), out


@pytest.mark.gpu
def test_binary_mxgemm():
    rc, res, out = run_bin("mxgemm", "96", "160", "224", "1")
    assert rc == 0, out.stdout + out.stderr
    assert set(res) == {"ok", "cmd", "m", "n", "k", "iters", "tflops", "max_err"}
    assert res["ok"] is True and res["cmd"] == "mxgemm" and res["max_err"] == 0
    assert (res["m"], res["n"], res["k"], res["iters"]) == (96, 160, 224, 1)
    assert res["tflops"] > 0


@pytest.mark.gpu
def test_serve_mxgemm():
    w = subprocess.Popen([BIN, "serve"], stdin=subprocess.PIPE,
                         stdout=subprocess.PIPE, text=True, bufsize=1)
    try:
        out, _ = w.communicate("mxgemm 128 128 128\nping\nquit\n", timeout=60)
    finally:
        if w.poll() is None:
            w.kill()
    mx, ping, quit_ = [json.loads(ln) for ln in out.splitlines()]
    assert set(mx) == {"ok", "cmd", "m", "n", "k", "max_err"}
    assert mx["ok"] is True and mx["cmd"] == "mxgemm" and mx["max_err"] == 0
    assert (mx["m"], mx["n"], mx["k"]) == (128, 128, 128)
    assert ping == {"ok": True, "cmd": "ping"}
    assert quit_ == {"ok": True}


@pytest.mark.gpu
def test_run_mxgemm_judges_the_real_partition():
    """ops/verify.run_mxgemm end to end, against the profile matching this
    device: the only run at the default shape."""
    from instaslice_amd.partition.profiles import mi355x_catalog

    rc, census, out = run_bin("census")
    assert rc == 0, out.stdout + out.stderr
    xcds = census["xcds_visible"]
    name = next(p.name for p in mi355x_catalog().profiles if p.xcds == xcds)
    v = verify.run_mxgemm(name)
    print(f"\nrun_mxgemm({name}): {v}")
    assert v["ok"] is True and v["failed"] == [] and v["profile"] == name
    rep = v["report"]
    assert (rep["m"], rep["n"], rep["k"], rep["iters"]) == (4096, 4096, 2048, 10)
    assert rep["max_err"] == 0 and rep["tflops"] > 0
