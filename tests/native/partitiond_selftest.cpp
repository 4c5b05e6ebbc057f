// Stand-alone self-test of smi/csrc/partitiond_metrics.hpp: the counter
// sample and its cache, against a scripted api that counts its calls.
// No Python, no GPU, no libamd_smi: build with -fsanitize=address,undefined
// and with -fsanitize=thread and run directly
// (tests/test_partitiond_selftest.py does).

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "partitiond_metrics.hpp"

using namespace partitiond;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

// What libamd_smi would answer, set by each case; every call is counted.
struct FakeApi {
  amdsmi_status_t table_status = AMDSMI_STATUS_SUCCESS;
  amdsmi_status_t memory_status = AMDSMI_STATUS_SUCCESS;
  amdsmi_status_t activity_status = AMDSMI_STATUS_SUCCESS;
  amdsmi_status_t power_status = AMDSMI_STATUS_SUCCESS;
  amdsmi_gpu_metrics_t table;
  amdsmi_engine_usage_t usage;
  amdsmi_power_info_t power;
  uint64_t vram_bytes = 3ull << 20;
  int n_table = 0, n_memory = 0, n_activity = 0, n_power = 0;

  FakeApi() {
    // every field "unsupported" unless a case says otherwise
    std::memset(&table, 0xff, sizeof(table));
    std::memset(&usage, 0xff, sizeof(usage));
    std::memset(&power, 0xff, sizeof(power));
    // the table's values and the per-call values differ on purpose, so a
    // test can tell which source a field came from
    table.average_gfx_activity = 11;
    table.average_umc_activity = 12;
    table.current_socket_power = 250;
    table.average_socket_power = 240;
    usage.gfx_activity = 21;
    usage.umc_activity = 22;
    power.socket_power = 350;
    power.current_socket_power = 351;
  }

  amdsmi_status_t metrics_info(amdsmi_processor_handle, amdsmi_gpu_metrics_t* t) {
    ++n_table;
    if (table_status == AMDSMI_STATUS_SUCCESS) *t = table;
    return table_status;
  }
  amdsmi_status_t memory_usage(amdsmi_processor_handle, uint64_t* used) {
    ++n_memory;
    if (memory_status == AMDSMI_STATUS_SUCCESS) *used = vram_bytes;
    return memory_status;
  }
  amdsmi_status_t activity(amdsmi_processor_handle, amdsmi_engine_usage_t* u) {
    ++n_activity;
    if (activity_status == AMDSMI_STATUS_SUCCESS) *u = usage;
    return activity_status;
  }
  amdsmi_status_t power_info(amdsmi_processor_handle, amdsmi_power_info_t* p) {
    ++n_power;
    if (power_status == AMDSMI_STATUS_SUCCESS) *p = power;
    return power_status;
  }
  int calls() const { return n_table + n_memory + n_activity + n_power; }
};

static amdsmi_processor_handle kHandle = nullptr;

static void test_table_fully_valid() {
  FakeApi api;
  Metrics m = read_metrics(kHandle, api);
  CHECK(api.n_table == 1 && api.n_memory == 1 && api.calls() == 2);
  CHECK(m.gfx_activity_pct == 11 && m.umc_activity_pct == 12);
  CHECK(m.socket_power_w == 250 && m.vram_used_mb == 3.0);

  Metrics direct;
  CHECK(metrics_from_table(api.table, direct) == kMetricFromTable);
  CHECK(direct.vram_used_mb == -1);
}

static void test_one_field_unsupported() {
  {  // gfx missing: one activity call, gfx alone from it
    FakeApi api;
    api.table.average_gfx_activity = UINT16_MAX;
    Metrics m = read_metrics(kHandle, api);
    CHECK(api.n_activity == 1 && api.n_power == 0 && api.calls() == 3);
    CHECK(m.gfx_activity_pct == 21);
    CHECK(m.umc_activity_pct == 12 && m.socket_power_w == 250);
  }
  {  // umc missing
    FakeApi api;
    api.table.average_umc_activity = UINT16_MAX;
    Metrics m = read_metrics(kHandle, api);
    CHECK(api.n_activity == 1 && api.n_power == 0 && api.calls() == 3);
    CHECK(m.umc_activity_pct == 22);
    CHECK(m.gfx_activity_pct == 11 && m.socket_power_w == 250);
  }
  {  // power missing in both of the table's fields: one power_info call
    FakeApi api;
    api.table.current_socket_power = UINT16_MAX;
    api.table.average_socket_power = UINT16_MAX;
    Metrics m = read_metrics(kHandle, api);
    CHECK(api.n_activity == 0 && api.n_power == 1 && api.calls() == 3);
    CHECK(m.socket_power_w == 350);
    CHECK(m.gfx_activity_pct == 11 && m.umc_activity_pct == 12);
  }
  {  // the fallback does not report the field either: it stays -1
    FakeApi api;
    api.table.average_gfx_activity = UINT16_MAX;
    api.usage.gfx_activity = UINT32_MAX;
    Metrics m = read_metrics(kHandle, api);
    CHECK(api.n_activity == 1 && m.gfx_activity_pct == -1);
    CHECK(m.umc_activity_pct == 12);
  }
}

static void test_power_preference() {
  {  // current power zero: the average is used, no further call
    FakeApi api;
    api.table.current_socket_power = 0;
    Metrics m = read_metrics(kHandle, api);
    CHECK(m.socket_power_w == 240 && api.calls() == 2);
  }
  {  // current power unsupported (parts before MI300): the average
    FakeApi api;
    api.table.current_socket_power = UINT16_MAX;
    Metrics m = read_metrics(kHandle, api);
    CHECK(m.socket_power_w == 240 && api.calls() == 2);
  }
  {  // power_info: socket_power zero falls to its current_socket_power
    FakeApi api;
    api.power.socket_power = 0;
    Metrics m = read_metrics_by_calls(kHandle, api);
    CHECK(m.socket_power_w == 351);
  }
}

static void test_table_call_fails() {
  FakeApi api;
  api.table_status = AMDSMI_STATUS_NOT_SUPPORTED;
  Metrics m = read_metrics(kHandle, api);
  CHECK(api.n_table == 1 && api.n_memory == 1 && api.n_activity == 1 &&
        api.n_power == 1);
  FakeApi parent;
  Metrics want = read_metrics_by_calls(kHandle, parent);
  CHECK(parent.n_table == 0 && parent.calls() == 3);
  CHECK(want.gfx_activity_pct == 21 && want.umc_activity_pct == 22 &&
        want.socket_power_w == 350 && want.vram_used_mb == 3.0);
  CHECK(m.gfx_activity_pct == want.gfx_activity_pct);
  CHECK(m.umc_activity_pct == want.umc_activity_pct);
  CHECK(m.socket_power_w == want.socket_power_w);
  CHECK(m.vram_used_mb == want.vram_used_mb);
}

static void test_everything_fails() {
  FakeApi api;
  api.table_status = api.memory_status = api.activity_status = api.power_status =
      AMDSMI_STATUS_NOT_SUPPORTED;
  Metrics m = read_metrics(kHandle, api);
  CHECK(api.calls() == 4);
  CHECK(m.gfx_activity_pct == -1 && m.umc_activity_pct == -1);
  CHECK(m.vram_used_mb == -1 && m.socket_power_w == -1);
}

// ---- the cache, on a clock the test sets by hand ---------------------------

struct ManualClock {
  std::atomic<int64_t>* us;
  int64_t operator()() const { return us->load(); }
};

static const int64_t kBoundMs = kMetricsMaxAgeMs;

static void test_cache() {
  std::atomic<int64_t> now{1000000};
  MetricsCache<ManualClock> cache(ManualClock{&now});
  int reads = 0;
  auto reader = [&](double tag) {
    return [&reads, tag] {
      ++reads;
      Metrics m;
      m.gfx_activity_pct = tag;
      return m;
    };
  };

  CHECK(cache.get_or_read(0, kBoundMs, reader(1)).gfx_activity_pct == 1 && reads == 1);
  // hit at age bound - 1 ms, and up to the last microsecond below the bound
  now = 1000000 + (kBoundMs - 1) * 1000;
  CHECK(cache.get_or_read(0, kBoundMs, reader(2)).gfx_activity_pct == 1 && reads == 1);
  now = 1000000 + kBoundMs * 1000 - 1;
  CHECK(cache.get_or_read(0, kBoundMs, reader(2)).gfx_activity_pct == 1 && reads == 1);
  // miss at age == bound; the new sample replaces the old
  now = 1000000 + kBoundMs * 1000;
  CHECK(cache.get_or_read(0, kBoundMs, reader(3)).gfx_activity_pct == 3 && reads == 2);
  CHECK(cache.get_or_read(0, kBoundMs, reader(4)).gfx_activity_pct == 3 && reads == 2);
  // max_age 0 always reads, also at age 0, and what it read is stored
  CHECK(cache.get_or_read(0, 0, reader(5)).gfx_activity_pct == 5 && reads == 3);
  CHECK(cache.get_or_read(0, 0, reader(6)).gfx_activity_pct == 6 && reads == 4);
  CHECK(cache.get_or_read(0, kBoundMs, reader(7)).gfx_activity_pct == 6 && reads == 4);

  // two indices are independent
  CHECK(cache.get_or_read(3, kBoundMs, reader(30)).gfx_activity_pct == 30 && reads == 5);
  CHECK(cache.get_or_read(0, kBoundMs, reader(8)).gfx_activity_pct == 6 && reads == 5);
  CHECK(cache.get_or_read(3, kBoundMs, reader(31)).gfx_activity_pct == 30 && reads == 5);
  // an index between them was never read
  CHECK(cache.get_or_read(1, kBoundMs, reader(10)).gfx_activity_pct == 10 && reads == 6);

  // invalidation empties all indices
  cache.invalidate();
  CHECK(cache.get_or_read(0, kBoundMs, reader(40)).gfx_activity_pct == 40 && reads == 7);
  CHECK(cache.get_or_read(3, kBoundMs, reader(41)).gfx_activity_pct == 41 && reads == 8);

  // a sample whose read began before an invalidation is handed to its
  // caller but not kept
  Metrics stale = cache.get_or_read(0, 0, [&] {
    cache.invalidate();
    Metrics m;
    m.gfx_activity_pct = 50;
    return m;
  });
  CHECK(stale.gfx_activity_pct == 50);
  CHECK(cache.get_or_read(0, kBoundMs, reader(51)).gfx_activity_pct == 51 && reads == 9);

  // a reader that throws stores nothing and leaves the cache usable
  bool threw = false;
  try {
    cache.get_or_read(5, kBoundMs, []() -> Metrics { throw 1; });
  } catch (int) {
    threw = true;
  }
  CHECK(threw);
  CHECK(cache.get_or_read(5, kBoundMs, reader(60)).gfx_activity_pct == 60 && reads == 10);
}

// Callers that ask at once each get a whole Metrics (all four fields from
// one read), with one device read or one per caller; a thread invalidating
// meanwhile changes nothing about that. The ThreadSanitizer build is what
// makes this case worth having.
static void test_cache_threads() {
  std::atomic<int64_t> now{0};
  MetricsCache<ManualClock> cache(ManualClock{&now});
  std::atomic<int> reads{0};
  auto read = [&] {
    double tag = ++reads;
    Metrics m;
    m.gfx_activity_pct = m.umc_activity_pct = m.vram_used_mb = m.socket_power_w = tag;
    return m;
  };
  auto whole = [](const Metrics& m) {
    return m.gfx_activity_pct >= 1 && m.umc_activity_pct == m.gfx_activity_pct &&
           m.vram_used_mb == m.gfx_activity_pct && m.socket_power_w == m.gfx_activity_pct;
  };

  {  // two callers at once on an empty cache, clock standing still
    Metrics a, b;
    std::thread ta([&] { a = cache.get_or_read(0, kBoundMs, read); });
    std::thread tb([&] { b = cache.get_or_read(0, kBoundMs, read); });
    ta.join();
    tb.join();
    CHECK(whole(a) && whole(b));
    CHECK(reads == 1 || reads == 2);
    int before = reads;
    CHECK(whole(cache.get_or_read(0, kBoundMs, read)) && reads == before);
  }

  std::atomic<bool> ok{true};
  std::vector<std::thread> threads;
  for (int t = 0; t < 4; ++t) {
    threads.emplace_back([&, t] {
      for (int i = 0; i < 2000; ++i) {
        Metrics m = cache.get_or_read(t % 2, (i % 5) ? kBoundMs : 0, read);
        if (!whole(m)) ok = false;
      }
    });
  }
  threads.emplace_back([&] {
    for (int i = 0; i < 200; ++i) {
      now += 3000;
      if (i % 10 == 0) cache.invalidate();
      std::this_thread::yield();
    }
  });
  for (auto& th : threads) th.join();
  CHECK(ok);
}

int main() {
  test_table_fully_valid();
  test_one_field_unsupported();
  test_power_preference();
  test_table_call_fails();
  test_everything_fails();
  test_cache();
  test_cache_threads();
  std::printf("partitiond selftest OK\n");
  return 0;
}
