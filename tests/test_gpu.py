"""Real-MI355X tests (run via gpurun; auto-skipped without a GPU).

Covers the device boundary the CPU tiers fake: libamd_smi enumeration through
the C++ partitiond shim, partition mode get/set, and the gfx950 payload
kernels — including the XCD census that *proves* partition visibility.
"""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def smi():
    from instaslice_amd.smi.native import NativeAmdSmi

    s = NativeAmdSmi()
    s.init()
    yield s


@pytest.fixture(scope="module")
def payload():
    from instaslice_amd.ops import _payload

    assert _payload.device_count() > 0
    return _payload


class TestNativeSmi:
    def test_enumeration(self, smi):
        gpus = smi.list_gpus()
        assert len(gpus) >= 1
        g = gpus[0]
        print(f"\ngpu0: {g.model} uuid={g.uuid} mem={g.memory_gb}GB "
              f"mode={g.compute_mode}/{g.memory_mode} parts={len(g.partitions)}")
        assert g.memory_gb > 0
        assert g.compute_mode in ("SPX", "DPX", "TPX", "QPX", "CPX")
        assert len(g.partitions) >= 1
        assert all(p.uuid for p in g.partitions)

    def test_enumeration_cached_and_stable(self, smi):
        a = smi.list_gpus()
        b = smi.list_gpus()
        assert [g.uuid for g in a] == [g.uuid for g in b]

    def test_get_compute_partition(self, smi):
        g = smi.list_gpus()[0]
        mode = smi.get_compute_partition(g.uuid)
        assert mode == g.compute_mode

    def test_metrics(self, smi):
        g = smi.list_gpus()[0]
        m = smi.get_metrics(g.uuid)
        print(f"\nmetrics: {m}")
        assert isinstance(m, dict) and "vram_used_mb" in m

    def test_profile_config_or_fallback(self, smi):
        """Profile discovery may be unsupported (VM guest) — then the static
        MI355X catalog takes over; either way the agent must get a catalog."""
        from instaslice_amd.partition.profiles import catalog_from_amdsmi_profiles
        from instaslice_amd.smi.base import SmiError

        g = smi.list_gpus()[0]
        try:
            raw = smi.get_profile_config(g.uuid)
            print(f"\ndiscovered profiles: {raw}")
        except SmiError as e:
            print(f"\nprofile discovery unsupported: {e}")
            raw = []
        cat = catalog_from_amdsmi_profiles(g.model, g.memory_gb, raw)
        assert cat.profiles


class TestPayloadKernels:
    def test_vecadd_exact(self, payload):
        err = payload.run_vecadd(1 << 24)
        assert err == 0.0

    def test_vecadd_matches_numpy_reference(self, payload):
        # numerics contract: HIP kernel vs plain fp32 reference
        import numpy as np

        rng = np.random.default_rng(1024)
        a = rng.standard_normal(1024).astype(np.float32)
        b = (rng.standard_normal(1024) * 1e3).astype(np.float32)
        ref = a + b  # one correctly rounded fp32 add per element
        c, guard_changed = payload.vecadd(a, b)
        assert c.dtype == np.float32 and c.shape == ref.shape
        assert np.array_equal(c.view(np.uint32), ref.view(np.uint32))
        assert guard_changed == 0
        # the constant operands of the first version of this test
        c, _ = payload.vecadd(np.full(1024, 1.25, dtype=np.float32),
                              np.full(1024, 2.5, dtype=np.float32))
        assert np.array_equal(c, np.full(1024, 3.75, dtype=np.float32))
        assert payload.run_vecadd(1024) == 0.0

    def test_membw_sane(self, payload):
        gbs = payload.run_membw(1 << 30, 10)
        print(f"\nstreaming-copy bandwidth: {gbs:.0f} GB/s")
        # whole MI355X measures ~6300 GB/s; even a 1-XCD CPX partition
        # should beat 100 GB/s by an order of magnitude
        assert gbs > 100.0

    def test_busy_occupies(self, payload):
        import time

        t0 = time.monotonic()
        payload.run_busy(200.0)
        dt = (time.monotonic() - t0) * 1000
        assert dt >= 150.0, f"busy(200ms) returned in {dt:.0f}ms"

    def test_xcd_census(self, payload):
        census = payload.run_xcd_census()
        info = payload.device_info(0)
        visible = sum(1 for c in census if c)
        print(f"\ncensus: {census} -> {visible} XCD(s); CUs={info['cu_count']} "
              f"arch={info['gcn_arch']}")
        assert visible >= 1
        # CU count should be ~32 per visible XCD on MI355X
        assert info["cu_count"] >= 16 * visible

    def test_payload_binary(self):
        bin_path = os.path.join(
            os.path.dirname(__file__), "..", "instaslice_amd", "bin",
            "instaslice-payload",
        )
        if not os.path.exists(bin_path):
            pytest.skip("instaslice-payload not built")
        out = subprocess.run([bin_path, "vecadd", "1000000"],
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        res = json.loads(out.stdout)
        assert res["ok"] and res["max_err"] == 0.0


class TestPartitionSet:
    """The write path: flip a GPU's compute mode and back. Skipped gracefully
    when the platform refuses (VM guest / no permission)."""

    def test_cpx_roundtrip(self, smi):
        from instaslice_amd.smi.base import SmiBusy, SmiError, SmiNotSupported, SmiPermission

        g = smi.list_gpus()[0]
        original = g.compute_mode
        target = "CPX" if original != "CPX" else "SPX"
        try:
            smi.set_compute_partition(g.uuid, target)
        except (SmiNotSupported, SmiPermission, SmiBusy) as e:
            pytest.skip(f"compute-partition set unavailable here: {e}")
        except SmiError as e:
            pytest.skip(f"compute-partition set failed ({e}); platform limit")
        try:
            fresh = smi.list_gpus()
            mine = [x for x in fresh if x.uuid == g.uuid]
            assert mine, "physical uuid lost across mode change"
            got = mine[0]
            print(f"\nafter set {target}: mode={got.compute_mode} "
                  f"partitions={len(got.partitions)}")
            assert got.compute_mode == target
            expect = {"SPX": 1, "DPX": 2, "TPX": 3, "QPX": 4, "CPX": 8}[target]
            assert len(got.partitions) == expect
        finally:
            smi.set_compute_partition(g.uuid, original)
            back = [x for x in smi.list_gpus() if x.uuid == g.uuid][0]
            assert back.compute_mode == original


class TestSmokeEntry:
    def test_graft_smoke(self):
        sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
        import __graft_entry__

        __graft_entry__.smoke()


class TestPayloadServe:
    """The warm payload worker (instaslice-payload serve): HIP init paid
    once, then kernels per request — what bench.py's --payload-every pool
    and a production validation sidecar rely on."""

    def test_serve_warm_kernel_rate(self):
        import subprocess
        import time as _time

        bin_path = os.path.join(
            os.path.dirname(__file__), "..", "instaslice_amd", "bin",
            "instaslice-payload")
        if not os.path.exists(bin_path):
            pytest.skip("instaslice-payload not built")
        w = subprocess.Popen([bin_path, "serve"], stdin=subprocess.PIPE,
                             stdout=subprocess.PIPE, text=True, bufsize=1,
                             env=dict(os.environ, ROCR_VISIBLE_DEVICES="0"))
        try:
            def ask(cmd):
                w.stdin.write(cmd + "\n")
                w.stdin.flush()
                return json.loads(w.stdout.readline())

            first = ask("vecadd 1048576")
            assert first["ok"] and first["max_err"] == 0.0
            t0 = _time.monotonic()
            for _ in range(5):
                res = ask("vecadd 1048576")
                assert res["ok"]
            dt = (_time.monotonic() - t0) / 5
            # warm dispatch must be far under one-shot child cost (~320ms)
            assert dt < 0.1, f"warm vecadd took {dt*1000:.0f} ms"
            assert ask("ping")["ok"]
        finally:
            try:
                w.stdin.write("quit\n")
                w.stdin.flush()
                w.wait(timeout=5)
            except Exception:
                w.kill()
