"""The counter sample on a real GPU: the one-table read of
partitiond_metrics.hpp against the three per-call sources it replaced, and
the sample cache in front of it. Presence of each field is compared, never
its value: activity and power move between two reads."""

import time

import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("gfx_activity_pct", "umc_activity_pct", "vram_used_mb",
          "socket_power_w")


def as_dict(m):
    return {f: getattr(m, f) for f in FIELDS}


@pytest.fixture(scope="module")
def dev():
    from instaslice_amd.smi import _partitiond

    d = _partitiond.Partitiond()
    d.init()
    assert d.num_processors() >= 1
    yield d
    d.shutdown()


def test_table_read_reports_what_the_calls_report(dev):
    by_calls = as_dict(dev.get_metrics_by_calls(0))
    fresh = as_dict(dev.get_metrics(0, max_age_ms=0))
    print(f"\nby calls: {by_calls}\none table: {fresh}")
    for f in FIELDS:
        assert (fresh[f] >= 0) == (by_calls[f] >= 0), f
    # what is absent is exactly -1, in both
    assert all(v >= 0 or v == -1 for v in (*fresh.values(), *by_calls.values()))


def test_default_calls_share_one_sample(dev):
    bound_s = 0.010
    t0 = time.monotonic()
    fresh = as_dict(dev.get_metrics(0, 0))  # read and stored at or after t0
    got = []
    for _ in range(200):
        m = dev.get_metrics(0)
        got.append((time.monotonic(), as_dict(m)))
    # a default call that returned within the bound of t0 saw the stored
    # sample at an age below the bound, so it was handed that sample
    inside = [m for t, m in got if t - t0 < bound_s]
    print(f"\n{len(inside)} of 200 default calls inside {bound_s * 1e3:.0f} ms "
          f"of the read; last returned after {(got[-1][0] - t0) * 1e3:.3f} ms")
    assert all(m == fresh for m in inside)
    # the same with a bound no scheduler delay can outlast
    stored = as_dict(dev.get_metrics(0, 0))
    assert all(as_dict(dev.get_metrics(0, 3_600_000)) == stored
               for _ in range(200))

    after = as_dict(dev.get_metrics(0, max_age_ms=0))
    print(f"fresh read afterwards: {after}")
    assert set(after) == set(FIELDS)
    for f in FIELDS:
        assert (after[f] >= 0) == (fresh[f] >= 0), f


def test_bad_index_still_raises(dev):
    n = dev.num_processors()
    with pytest.raises(IndexError):
        dev.get_metrics(n)
    with pytest.raises(IndexError):
        dev.get_metrics(n, 0)
