"""ops/verify.py: judging an `instaslice-payload verify` report against a
profile, and running the verb in a child. All on CPU: the child is faked
through the injectable runner."""

import json
import subprocess
from types import SimpleNamespace

import pytest

from instaslice_amd.ops import verify


def report(**over):
    """What the binary prints for a healthy one-XCD partition."""
    r = {
        "ok": True, "cmd": "verify", "xcds_expected": 1, "xcds_visible": 1,
        "per_xcd": [0, 0, 0, 2048, 0, 0, 0, 0], "cu_count": 32,
        "total_mem_gb": 36.0, "vecadd_max_err": 0, "gemm_max_err": 0,
        "membw_bad_units": 0,
        "gb_per_s": 700.0, "tflops": 90.0, "gb_per_s_per_xcd": 700.0,
        "tflops_per_xcd": 90.0, "failed": [],
    }
    r.update(over)
    return r


def fake_runner(stdout="", returncode=0, raises=None, seen=None):
    def runner(cmd, **kw):
        if seen is not None:
            seen.append((cmd, kw))
        if raises is not None:
            raise raises
        return SimpleNamespace(stdout=stdout, stderr="", returncode=returncode)
    return runner


# ---- expected_xcds / judge ------------------------------------------------

def test_expected_xcds():
    assert verify.expected_xcds("cpx-1x36") == 1
    assert verify.expected_xcds("qpx-2x72") == 2
    assert verify.expected_xcds("spx-8x288") == 8
    with pytest.raises(ValueError):
        verify.expected_xcds("1g.5gb")


def test_judge_pass():
    rep = report()
    v = verify.judge(rep, "cpx-1x36")
    assert v == {"ok": True, "failed": [], "profile": "cpx-1x36", "report": rep}


def test_judge_xcd_mismatch():
    v = verify.judge(report(xcds_visible=8), "cpx-1x36")
    assert v["ok"] is False
    assert v["failed"] == ["xcds"]


def test_judge_does_not_trust_the_reports_own_ok():
    v = verify.judge(report(ok=True, failed=[], gemm_max_err=3.0), "cpx-1x36")
    assert v["ok"] is False
    assert "gemm" in v["failed"]


def test_judge_vecadd_and_missing_fields():
    assert verify.judge(report(vecadd_max_err=0.5), "cpx-1x36")["failed"] == ["vecadd"]
    rep = report()
    del rep["gemm_max_err"]
    assert verify.judge(rep, "cpx-1x36")["failed"] == ["gemm"]


def test_judge_membw_bad_units():
    v = verify.judge(report(membw_bad_units=3), "cpx-1x36")
    assert v["ok"] is False and v["failed"] == ["membw"]
    rep = report()
    del rep["membw_bad_units"]
    v = verify.judge(rep, "cpx-1x36")
    assert v["ok"] is False and v["failed"] == ["membw"]
    # a count that is not a number is not a zero
    assert verify.judge(report(membw_bad_units="0"), "cpx-1x36")["failed"] == ["membw"]
    assert verify.judge(report(membw_bad_units=None), "cpx-1x36")["failed"] == ["membw"]


def test_judge_rates_are_not_judged():
    v = verify.judge(report(gb_per_s=0.0, tflops=0.0, cu_count=1,
                            total_mem_gb=0.1), "cpx-1x36")
    assert v["ok"] is True


def test_judge_unknown_profile():
    with pytest.raises(ValueError):
        verify.judge(report(), "not-a-profile")


# ---- run ------------------------------------------------------------------

def test_run_good_json():
    seen = []
    v = verify.run("cpx-1x36", env={"ROCR_VISIBLE_DEVICES": "GPU-abc"},
                   runner=fake_runner(json.dumps(report()) + "\n", seen=seen))
    assert v["ok"] is True and v["failed"] == []
    assert v["report"]["xcds_visible"] == 1
    (cmd, kw), = seen
    assert cmd[1:] == ["verify", "1"]
    assert kw["env"]["ROCR_VISIBLE_DEVICES"] == "GPU-abc"
    assert kw["timeout"] == verify.CHILD_TIMEOUT_S == 60.0


def test_run_judges_against_the_profile_not_the_binary():
    # binary says ok (it was told to expect 8), the profile wants 1
    rep = report(xcds_expected=8, xcds_visible=8)
    v = verify.run("cpx-1x36", runner=fake_runner(json.dumps(rep)))
    assert v["ok"] is False and v["failed"] == ["xcds"]


def test_run_garbage_stdout():
    v = verify.run("cpx-1x36", runner=fake_runner("Segmentation fault\n", 0))
    assert v["ok"] is False
    assert "non-JSON" in v["reason"]


def test_run_nonzero_exit():
    # failing report: judged, and the exit status is carried as the reason
    rep = report(ok=False, gemm_max_err=2.0, failed=["gemm"])
    v = verify.run("cpx-1x36", runner=fake_runner(json.dumps(rep), 1))
    assert v["ok"] is False and v["failed"] == ["gemm"]
    assert "exited 1" in v["reason"]
    # clean-looking fields do not outvote a non-zero exit
    v = verify.run("cpx-1x36", runner=fake_runner(json.dumps(report()), 1))
    assert v["ok"] is False and "exited 1" in v["reason"]
    # the binary's catch-all error line
    err = json.dumps({"ok": False, "error": "HIP error: no ROCm-capable device"})
    v = verify.run("cpx-1x36", runner=fake_runner(err, 1))
    assert v["ok"] is False and "no ROCm-capable device" in v["reason"]
    # no output at all
    v = verify.run("cpx-1x36", runner=fake_runner("", 139))
    assert v["ok"] is False and "139" in v["reason"]


def test_run_timeout():
    exc = subprocess.TimeoutExpired(cmd="instaslice-payload", timeout=60)
    v = verify.run("cpx-1x36", runner=fake_runner(raises=exc))
    assert v["ok"] is False
    assert "timed out" in v["reason"]


def test_run_missing_binary():
    v = verify.run("cpx-1x36", runner=fake_runner(raises=FileNotFoundError()))
    assert v["ok"] is False
    assert "not found" in v["reason"]


def test_run_missing_binary_real_subprocess(monkeypatch, tmp_path):
    monkeypatch.setattr(verify, "BIN_PATH", str(tmp_path / "no-such-binary"))
    v = verify.run("cpx-1x36")
    assert v["ok"] is False and "not found" in v["reason"]


def test_run_unknown_profile():
    with pytest.raises(ValueError):
        verify.run("bogus", runner=fake_runner("{}"))


# ---- CLI ------------------------------------------------------------------

def _patch_runner(monkeypatch, runner):
    real = verify.run
    monkeypatch.setattr(
        verify, "run",
        lambda profile, env=None: real(profile, env=env, runner=runner))


def test_cli_verify_ok(monkeypatch, capsys):
    from instaslice_amd.cli import main

    seen = []
    _patch_runner(monkeypatch, fake_runner(json.dumps(report()), seen=seen))
    rc = main(["verify", "--profile", "cpx-1x36", "--visible-devices", "3"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 0 and out["ok"] is True and out["profile"] == "cpx-1x36"
    assert seen[0][1]["env"]["ROCR_VISIBLE_DEVICES"] == "3"


def test_cli_verify_fail(monkeypatch, capsys):
    from instaslice_amd.cli import main

    _patch_runner(monkeypatch,
                  fake_runner(json.dumps(report(xcds_visible=2)), 0))
    rc = main(["verify", "--profile", "cpx-1x36"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 1 and out["ok"] is False and out["failed"] == ["xcds"]


def test_cli_verify_bad_profile(capsys):
    from instaslice_amd.cli import main

    rc = main(["verify", "--profile", "bogus"])
    out = json.loads(capsys.readouterr().out)
    assert rc == 1 and out["ok"] is False and "bogus" in out["reason"]
