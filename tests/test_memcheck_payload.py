"""The memcheck payload (ops/csrc/payload_memcheck.hpp): the host pattern,
argument checks, the judge, the runner and the CLI on CPU; the kernels, the
bindings, the binary's `memcheck` verb and `verify.run_memcheck` on a real
MI355X.

The pattern is re-implemented here in numpy, independently of the header:

    mix64(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
              z = (z ^ (z >> 27)) * 0x94D049BB133111EB
              return z ^ (z >> 31)
    key(seed) = mix64(seed + 0x9E3779B97F4A7C15)
    unit q: h = mix64(q ^ key); word0 = h; word1 = ~rotl64(h, 31)

All of it on np.uint64 arrays, which wrap silently. Every comparison is exact.
The GPU sizes are tiny on purpose: they prove the kernels, not the HBM (a
buffer below the 256 MiB Infinity Cache can be served from cache).
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

MIB = 1 << 20
GIB = 1 << 30
ALL_ONES = (1 << 64) - 1


@pytest.fixture(scope="module")
def payload():
    from instaslice_amd.ops import _payload

    return _payload


# ---- the numpy reference --------------------------------------------------

def u64(x):
    return np.array([x], dtype=np.uint64)


def mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def ref_key(seed):
    return mix64(u64(seed) + u64(0x9E3779B97F4A7C15))


def ref_words(first_word, n_words, seed=0, invert=False):
    """Words first_word .. first_word+n_words-1 of the pattern."""
    w = u64(first_word) + np.arange(n_words, dtype=np.uint64)
    h = mix64((w >> np.uint64(1)) ^ ref_key(seed))
    word1 = ~((h << np.uint64(31)) | (h >> np.uint64(33)))
    out = np.where((w & np.uint64(1)) == np.uint64(1), word1, h)
    return ~out if invert else out


def test_reference_key_is_splitmix64():
    # key(0) is the first output of SplitMix64 seeded with 0, a published value
    assert int(ref_key(0)[0]) == 0xE220A8397B1DCDAF


# ---- CPU: the host pattern ------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 1 << 63])
def test_pattern_matches_numpy(payload, seed):
    got = payload.memcheck_pattern(0, 4096, seed)
    assert got.dtype == np.uint64 and got.shape == (4096,)
    assert np.array_equal(got, ref_words(0, 4096, seed))


@pytest.mark.parametrize("first_word", [7, (1 << 33) - 3])
def test_pattern_odd_start_and_64_bit_index(payload, first_word):
    got = payload.memcheck_pattern(first_word, 1001, 5)
    assert np.array_equal(got, ref_words(first_word, 1001, 5))
    # the unit index beyond 32 bits takes part: same low bits, other data
    low = payload.memcheck_pattern(first_word & 0xFFFFFFFF, 1001, 5)
    if first_word >> 32:
        assert not np.array_equal(got, low)


def test_pattern_default_seed_is_zero(payload):
    assert np.array_equal(payload.memcheck_pattern(0, 64),
                          payload.memcheck_pattern(0, 64, 0))


def test_pattern_units_are_distinct(payload):
    words = payload.memcheck_pattern(0, 2 * 65536, 3)
    assert len(np.unique(words[0::2])) == 65536


# ---- CPU: argument errors come before any device work ---------------------

def test_run_memcheck_argument_errors(payload):
    with pytest.raises(ValueError):
        payload.run_memcheck(bytes=8)
    with pytest.raises(ValueError):
        payload.run_memcheck(bytes=1024, passes=0)
    with pytest.raises(ValueError):
        payload.run_memcheck(bytes=1024, flip_offset=1024, flip_mask=1)
    with pytest.raises(ValueError):
        # 1039 rounds down to 1024: the offset is past the tested bytes
        payload.run_memcheck(bytes=1039, flip_offset=1030, flip_mask=1)
    with pytest.raises(ValueError):
        payload.memcheck_fill(8)


# ---- CPU: judge_memcheck --------------------------------------------------

def report(**over):
    """What the binary prints for a clean 1 GiB sweep."""
    r = {
        "ok": True, "cmd": "memcheck", "bytes": GIB, "passes": 1,
        "bad_words": 0, "first_bad_offset": -1, "bad_bits": "0x0",
        "fill_gb_per_s": 3000.0, "check_gb_per_s": 3000.0, "ms": 2.0,
        "beyond_llc": True,
    }
    r.update(over)
    return r


def test_judge_memcheck_pass():
    rep = report()
    v = verify.judge_memcheck(rep, "cpx-1x36", GIB)
    assert v == {"ok": True, "failed": [], "profile": "cpx-1x36", "report": rep}
    # want_bytes is rounded down to 16 like the binary rounds
    assert verify.judge_memcheck(rep, "cpx-1x36", GIB + 15)["ok"] is True


def test_judge_memcheck_bad_word():
    v = verify.judge_memcheck(
        report(ok=True, bad_words=1, first_bad_offset=4104, bad_bits="0xff"),
        "cpx-1x36", GIB)
    assert v["ok"] is False and v["failed"] == ["memory"]
    # a count without an offset, or the reverse, is not clean either
    assert verify.judge_memcheck(report(bad_words=1), "cpx-1x36",
                                 GIB)["failed"] == ["memory"]
    assert verify.judge_memcheck(report(first_bad_offset=0), "cpx-1x36",
                                 GIB)["failed"] == ["memory"]


@pytest.mark.parametrize("field", ["bad_words", "first_bad_offset", "bytes",
                                   "passes"])
def test_judge_memcheck_missing_or_non_numeric_field(field):
    rep = report()
    del rep[field]
    assert verify.judge_memcheck(rep, "cpx-1x36", GIB)["failed"] == ["memory"]
    for junk in ("0", None, True):
        assert verify.judge_memcheck(report(**{field: junk}), "cpx-1x36",
                                     GIB)["failed"] == ["memory"]


def test_judge_memcheck_short_bytes_and_passes():
    v = verify.judge_memcheck(report(bytes=GIB // 2), "cpx-1x36", GIB)
    assert v["ok"] is False and v["failed"] == ["memory"]
    assert verify.judge_memcheck(report(passes=0), "cpx-1x36",
                                 GIB)["failed"] == ["memory"]
    assert verify.judge_memcheck(report(passes=3), "cpx-1x36", GIB)["ok"] is True


def test_judge_memcheck_unknown_profile():
    with pytest.raises(ValueError):
        verify.judge_memcheck(report(), "not-a-profile", GIB)


# ---- CPU: verify.run_memcheck with a fake child ----------------------------

def fake_runner(stdout="", returncode=0, raises=None, seen=None):
    def runner(cmd, **kw):
        if seen is not None:
            seen.append((cmd, kw))
        if raises is not None:
            raise raises
        return SimpleNamespace(stdout=stdout, stderr="", returncode=returncode)
    return runner


def test_run_memcheck_bytes_from_gb():
    seen = []
    want = GIB // 16  # gb=0.0625 is 64 MiB
    v = verify.run_memcheck(
        "cpx-1x36", env={"ROCR_VISIBLE_DEVICES": "GPU-abc"}, gb=0.0625, passes=2,
        runner=fake_runner(json.dumps(report(bytes=want, passes=2)), seen=seen))
    assert v["ok"] is True and v["failed"] == [] and v["profile"] == "cpx-1x36"
    (cmd, kw), = seen
    assert cmd[1:] == ["memcheck", str(want), "2"]
    assert kw["env"]["ROCR_VISIBLE_DEVICES"] == "GPU-abc"
    assert kw["timeout"] == verify.MEMCHECK_TIMEOUT_S


def test_run_memcheck_default_is_one_gib():
    seen = []
    v = verify.run_memcheck("cpx-1x36",
                            runner=fake_runner(json.dumps(report()), seen=seen))
    assert v["ok"] is True
    assert seen[0][0][1:] == ["memcheck", str(GIB), "1"]


def test_run_memcheck_bytes_from_fraction_of_the_profile():
    for name, profile_gb in (("cpx-1x36", 36), ("qpx-2x72", 72)):
        seen = []
        want = int(0.5 * profile_gb * GIB)
        v = verify.run_memcheck(
            name, fraction=0.5,
            runner=fake_runner(json.dumps(report(bytes=want)), seen=seen))
        assert v["ok"] is True
        assert seen[0][0][1:] == ["memcheck", str(want), "1"]
    # a size that is no multiple of 16 is rounded down, and judged as such
    seen = []
    verify.run_memcheck("cpx-1x36", fraction=0.9,
                        runner=fake_runner(json.dumps(report()), seen=seen))
    sent = int(seen[0][0][2])
    assert sent % 16 == 0 and 0 <= 0.9 * 36 * GIB - sent < 16


def test_run_memcheck_argument_errors_raise():
    runner = fake_runner(json.dumps(report()))
    with pytest.raises(ValueError):
        verify.run_memcheck("cpx-1x36", gb=1, fraction=0.5, runner=runner)
    with pytest.raises(ValueError):
        verify.run_memcheck("bogus", runner=runner)
    with pytest.raises(ValueError):
        verify.run_memcheck("cpx-1x36", passes=0, runner=runner)
    with pytest.raises(ValueError):
        verify.run_memcheck("cpx-1x36", fraction=0, runner=runner)


def test_run_memcheck_judges_the_size_it_asked_for():
    # the child swept less than was asked
    v = verify.run_memcheck("cpx-1x36", gb=2,
                            runner=fake_runner(json.dumps(report(bytes=GIB))))
    assert v["ok"] is False and v["failed"] == ["memory"]


def test_run_memcheck_child_failures():
    v = verify.run_memcheck("cpx-1x36",
                            runner=fake_runner("Segmentation fault\n", 0))
    assert v["ok"] is False and "non-JSON" in v["reason"]
    exc = subprocess.TimeoutExpired(cmd="instaslice-payload", timeout=1)
    v = verify.run_memcheck("cpx-1x36", runner=fake_runner(raises=exc))
    assert v["ok"] is False and "timed out" in v["reason"]
    v = verify.run_memcheck("cpx-1x36",
                            runner=fake_runner(raises=FileNotFoundError()))
    assert v["ok"] is False and "not found" in v["reason"]
    # the binary's catch-all line: a partition without the memory ends here
    err = json.dumps({"ok": False,
                      "error": "HIP error: out of memory at hipMalloc(&p, bytes)"})
    v = verify.run_memcheck("cpx-1x36", fraction=0.9,
                            runner=fake_runner(err, 1))
    assert v["ok"] is False and v["failed"] == []
    assert "out of memory" in v["reason"]
    # a failing report is judged, and the exit status is carried
    rep = report(ok=False, bad_words=2, first_bad_offset=64, bad_bits="0x1")
    v = verify.run_memcheck("cpx-1x36", runner=fake_runner(json.dumps(rep), 1))
    assert v["ok"] is False and v["failed"] == ["memory"]
    assert "exited 1" in v["reason"]
    # clean-looking fields do not outvote a non-zero exit
    v = verify.run_memcheck("cpx-1x36",
                            runner=fake_runner(json.dumps(report()), 1))
    assert v["ok"] is False and "exited 1" in v["reason"]


def test_run_memcheck_missing_binary_real_subprocess(monkeypatch, tmp_path):
    monkeypatch.setattr(verify, "BIN_PATH", str(tmp_path / "no-such-binary"))
    v = verify.run_memcheck("cpx-1x36")
    assert v["ok"] is False and "not found" in v["reason"]


# ---- CPU: the CLI command -------------------------------------------------

def _patch_runner(monkeypatch, runner):
    real = verify.run_memcheck
    monkeypatch.setattr(
        verify, "run_memcheck",
        lambda profile, **kw: real(profile, runner=runner, **kw))


def test_cli_memcheck_ok(monkeypatch, capsys):
    from instaslice_amd.cli import main

    seen = []
    want = 2 * GIB
    _patch_runner(monkeypatch, fake_runner(
        json.dumps(report(bytes=want, passes=3)), seen=seen))
    rc = main(["memcheck", "--profile", "cpx-1x36", "--gb", "2", "--passes",
               "3", "--visible-devices", "3"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 0 and out["ok"] is True and out["profile"] == "cpx-1x36"
    assert seen[0][0][1:] == ["memcheck", str(want), "3"]
    assert seen[0][1]["env"]["ROCR_VISIBLE_DEVICES"] == "3"


def test_cli_memcheck_fail(monkeypatch, capsys):
    from instaslice_amd.cli import main

    rep = report(ok=False, bad_words=1, first_bad_offset=8, bad_bits="0x4")
    _patch_runner(monkeypatch, fake_runner(json.dumps(rep), 1))
    rc = main(["memcheck", "--profile", "cpx-1x36"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 1 and out["ok"] is False and out["failed"] == ["memory"]


def test_cli_memcheck_fraction_and_bad_profile(monkeypatch, capsys):
    from instaslice_amd.cli import main

    seen = []
    want = 9 * GIB  # a quarter of cpx-1x36
    _patch_runner(monkeypatch,
                  fake_runner(json.dumps(report(bytes=want)), seen=seen))
    rc = main(["memcheck", "--profile", "cpx-1x36", "--fraction", "0.25"])
    assert rc == 0 and json.loads(capsys.readouterr().out)["ok"] is True
    assert seen[0][0][2] == str(want)
    rc = main(["memcheck", "--profile", "bogus"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 1 and out["ok"] is False and "bogus" in out["reason"]


# ---- GPU: the fill kernel against the numpy pattern ------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("nbytes", [16, 48, 256 * 16 * 3 + 16])
def test_fill_matches_numpy_default_grid(payload, nbytes):
    got = payload.memcheck_fill(nbytes, seed=1)
    assert got.dtype == np.uint64 and got.shape == (nbytes // 16 * 2,)
    assert np.array_equal(got, ref_words(0, nbytes // 8, 1))


@pytest.mark.gpu
def test_fill_grid_stride_loop(payload):
    # 4096 units over 2 blocks of 256 lanes: 8 trips per lane
    got = payload.memcheck_fill(64 * 1024, seed=2, blocks=2)
    assert np.array_equal(got, ref_words(0, 8192, 2))


@pytest.mark.gpu
def test_fill_rounds_down_and_inverts(payload):
    got = payload.memcheck_fill(48 + 15, seed=0, invert=True)
    assert got.shape == (6,)
    assert np.array_equal(got, ref_words(0, 6, 0, invert=True))


@pytest.mark.gpu
@pytest.mark.parametrize("base_unit", [(1 << 28) - 2, (1 << 32) - 2])
def test_fill_base_unit_crosses_32_bits(payload, base_unit):
    # 2^28 - 2: the byte offset crosses 4 GiB; 2^32 - 2: the unit index does
    got = payload.memcheck_fill(64, seed=4, base_unit=base_unit)
    assert np.array_equal(got, ref_words(2 * base_unit, 8, 4))


# ---- GPU: clean runs and detection ----------------------------------------

SMALL = MIB + 16  # 65537 units: 257 blocks by default, the last one ragged


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [0, 2])
def test_clean_run(payload, blocks):
    r = payload.run_memcheck(SMALL + 5, passes=2, blocks=blocks)
    print(f"\nrun_memcheck {SMALL} B, blocks={blocks}: {r}")
    assert r["bytes"] == SMALL and r["passes"] == 2
    assert r["bad_words"] == 0 and r["first_bad_offset"] == -1
    assert r["bad_bits"] == 0
    assert r["fill_gb_s"] > 0 and r["check_gb_s"] > 0 and r["ms"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("flip_mask", [1, 1 << 63, 0xFF00])
@pytest.mark.parametrize("flip_offset,blocks", [
    (0, 0), (12, 0), (SMALL - 1, 0), (SMALL - 1, 2), (524296, 2)])
def test_detects_one_flipped_word(payload, flip_offset, blocks, flip_mask):
    # two passes: every check after the one that meets the flip must be clean
    r = payload.run_memcheck(SMALL, passes=2, blocks=blocks,
                             flip_offset=flip_offset, flip_mask=flip_mask)
    assert r["bad_words"] == 1
    assert r["first_bad_offset"] == flip_offset & ~7
    assert r["bad_bits"] == flip_mask


@pytest.mark.gpu
def test_flip_with_zero_mask_is_clean(payload):
    r = payload.run_memcheck(SMALL, flip_offset=12, flip_mask=0)
    assert r["bad_words"] == 0 and r["first_bad_offset"] == -1
    assert r["bad_bits"] == 0


@pytest.mark.gpu
def test_counts_both_words_of_a_unit_once(payload):
    # all 64 bits of one word: the complement pass must not count it again
    r = payload.run_memcheck(SMALL, passes=2, flip_offset=8, flip_mask=ALL_ONES)
    assert (r["bad_words"], r["first_bad_offset"], r["bad_bits"]) == \
        (1, 8, ALL_ONES)


# ---- GPU: the binary ------------------------------------------------------

def run_bin(*args, timeout=120):
    out = subprocess.run([BIN, *args], capture_output=True, text=True,
                         timeout=timeout)
    return out.returncode, json.loads(out.stdout), out


REPORT_FIELDS = {"ok", "cmd", "bytes", "passes", "bad_words",
                 "first_bad_offset", "bad_bits", "fill_gb_per_s",
                 "check_gb_per_s", "ms", "beyond_llc"}


@pytest.mark.gpu
def test_binary_memcheck_clean():
    rc, res, out = run_bin("memcheck", "1048592", "1")
    assert rc == 0, out.stdout + out.stderr
    assert set(res) == REPORT_FIELDS
    assert res["ok"] is True and res["cmd"] == "memcheck"
    assert (res["bytes"], res["passes"]) == (1048592, 1)
    assert res["bad_words"] == 0 and res["first_bad_offset"] == -1
    assert res["bad_bits"] == "0x0" and res["beyond_llc"] is False


@pytest.mark.gpu
def test_binary_memcheck_flip():
    rc, res, out = run_bin("memcheck", "1048592", "1", "4104", "255")
    assert rc == 1, out.stdout + out.stderr
    assert res["ok"] is False and res["bad_words"] == 1
    assert res["first_bad_offset"] == 4104 and res["bad_bits"] == "0xff"


@pytest.mark.gpu
def test_binary_memcheck_offset_beyond_4_gib():
    """The only test that catches a byte offset truncated to 32 bits on the
    way out. 4 GiB + 64 KiB, four traversals: the child has a time limit of
    its own."""
    nbytes = 4 * GIB + 64 * 1024
    flip = 4 * GIB + 4104
    rc, res, out = run_bin("memcheck", str(nbytes), "1", str(flip), "0x8001",
                           timeout=120)
    print(f"\nmemcheck {nbytes} B: {res}")
    assert rc == 1, out.stdout + out.stderr
    assert res["bytes"] == nbytes and res["beyond_llc"] is True
    assert res["bad_words"] == 1
    assert res["first_bad_offset"] == flip
    assert res["bad_bits"] == "0x8001"


@pytest.mark.gpu
def test_serve_memcheck():
    w = subprocess.Popen([BIN, "serve"], stdin=subprocess.PIPE,
                         stdout=subprocess.PIPE, text=True, bufsize=1)
    try:
        out, _ = w.communicate("memcheck 1048576\nping\nquit\n", timeout=60)
    finally:
        if w.poll() is None:
            w.kill()
    mem, ping, quit_ = [json.loads(ln) for ln in out.splitlines()]
    assert set(mem) == REPORT_FIELDS
    assert mem["ok"] is True and mem["cmd"] == "memcheck"
    assert mem["bytes"] == 1048576 and mem["bad_words"] == 0
    assert ping == {"ok": True, "cmd": "ping"}
    assert quit_ == {"ok": True}


@pytest.mark.gpu
def test_run_memcheck_judges_the_real_partition():
    """ops/verify.run_memcheck end to end, against the profile matching this
    device (64 MiB: the plumbing, not the HBM)."""
    from instaslice_amd.partition.profiles import mi355x_catalog

    rc, census, out = run_bin("census")
    assert rc == 0, out.stdout + out.stderr
    xcds = census["xcds_visible"]
    name = next(p.name for p in mi355x_catalog().profiles if p.xcds == xcds)
    v = verify.run_memcheck(name, gb=0.0625)
    assert v["ok"] is True and v["failed"] == [] and v["profile"] == name
    assert v["report"]["bytes"] == 64 * MIB
