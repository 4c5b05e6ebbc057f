// partitiond: the counter sample (Metrics), without the device.
//
// Everything here is pure: it includes amdsmi.h for its types and calls
// nothing in the library, so tests/native/partitiond_selftest.cpp runs it
// against a scripted api on any machine. partitiond_core.hpp supplies the
// api that forwards to libamd_smi.
//
// A sample used to cost three library calls (activity, memory usage, power
// info). Activity and power info are each built on the driver's gpu_metrics
// table, and power info goes on to read voltages and the power limit that
// Metrics does not keep. read_metrics() fetches the table once and falls
// back to the old calls only for a field the table does not carry
// (profiles/smi_metrics.md has the cost of each call on an MI355X).
// MetricsCache keeps the last sample per processor for callers that ask
// again within a few milliseconds.

#pragma once

#include <amd_smi/amdsmi.h>

#include <chrono>
#include <cstdint>
#include <limits>
#include <mutex>
#include <utility>
#include <vector>

namespace partitiond {

struct Metrics {
  double gfx_activity_pct = -1;
  double umc_activity_pct = -1;
  double vram_used_mb = -1;
  double socket_power_w = -1;
};

// The fields of Metrics that more than one source can supply, as a bit set.
enum : unsigned {
  kMetricGfx = 1u,
  kMetricUmc = 2u,
  kMetricPower = 4u,
  kMetricActivity = kMetricGfx | kMetricUmc,
  kMetricFromTable = kMetricActivity | kMetricPower,
};

// amdsmi marks a field it cannot report with the all-ones value of its type.
template <class T>
inline bool reported(T v) {
  return v != std::numeric_limits<T>::max();
}

// Fills what the gpu_metrics table carries; returns the fields it filled.
inline unsigned metrics_from_table(const amdsmi_gpu_metrics_t& t, Metrics& m) {
  unsigned filled = 0;
  if (reported(t.average_gfx_activity)) {
    m.gfx_activity_pct = t.average_gfx_activity;
    filled |= kMetricGfx;
  }
  if (reported(t.average_umc_activity)) {
    m.umc_activity_pct = t.average_umc_activity;
    filled |= kMetricUmc;
  }
  // current power (MI300 and later) before the average (earlier parts):
  // the order amdsmi_get_power_info itself uses for its socket_power
  if (reported(t.current_socket_power) && t.current_socket_power != 0) {
    m.socket_power_w = t.current_socket_power;
    filled |= kMetricPower;
  } else if (reported(t.average_socket_power)) {
    m.socket_power_w = t.average_socket_power;
    filled |= kMetricPower;
  }
  return filled;
}

// The per-call sources. `want` limits which fields are taken, so a fallback
// for one missing field leaves the ones the table supplied alone.
inline void metrics_from_activity(const amdsmi_engine_usage_t& u, unsigned want,
                                  Metrics& m) {
  if ((want & kMetricGfx) && reported(u.gfx_activity)) m.gfx_activity_pct = u.gfx_activity;
  if ((want & kMetricUmc) && reported(u.umc_activity)) m.umc_activity_pct = u.umc_activity;
}

inline void metrics_from_power_info(const amdsmi_power_info_t& p, Metrics& m) {
  if (reported(p.socket_power) && p.socket_power != 0)
    m.socket_power_w = static_cast<double>(p.socket_power);
  else if (reported(p.current_socket_power))
    m.socket_power_w = p.current_socket_power;
}

template <class Api>
inline void read_vram(amdsmi_processor_handle h, Api& api, Metrics& m) {
  uint64_t used = 0;
  if (api.memory_usage(h, &used) == AMDSMI_STATUS_SUCCESS)
    m.vram_used_mb = static_cast<double>(used) / (1024.0 * 1024.0);
}

template <class Api>
inline void read_by_calls(amdsmi_processor_handle h, Api& api, unsigned want, Metrics& m) {
  if (want & kMetricActivity) {
    amdsmi_engine_usage_t usage;
    if (api.activity(h, &usage) == AMDSMI_STATUS_SUCCESS)
      metrics_from_activity(usage, want, m);
  }
  if (want & kMetricPower) {
    amdsmi_power_info_t power;
    if (api.power_info(h, &power) == AMDSMI_STATUS_SUCCESS)
      metrics_from_power_info(power, m);
  }
}

// One sample: the table and the memory usage, then the per-call source of
// whatever the table left out (everything, when the table call itself fails
// as it does on a secondary partition or a VM guest). `Api` has four
// members, metrics_info / memory_usage / activity / power_info, each taking
// the handle and an out pointer and returning an amdsmi_status_t. A call
// that fails leaves its fields at -1; nothing throws.
template <class Api>
inline Metrics read_metrics(amdsmi_processor_handle h, Api& api) {
  Metrics m;
  unsigned filled = 0;
  amdsmi_gpu_metrics_t table;
  if (api.metrics_info(h, &table) == AMDSMI_STATUS_SUCCESS)
    filled = metrics_from_table(table, m);
  read_vram(h, api, m);
  read_by_calls(h, api, kMetricFromTable & ~filled, m);
  return m;
}

// The same sample by the three per-call sources alone, as it was taken
// before read_metrics: kept callable so a test on the GPU can hold the two
// against each other.
template <class Api>
inline Metrics read_metrics_by_calls(amdsmi_processor_handle h, Api& api) {
  Metrics m;
  read_by_calls(h, api, kMetricActivity, m);
  read_vram(h, api, m);
  read_by_calls(h, api, kMetricPower, m);
  return m;
}

// How old a sample get_metrics hands out by default. A design constant, not
// a measured one: an order of magnitude above the period of the driver's own
// cache of the table, one to two below a reconfigure (100 ms to 1 s) and far
// below the agent's heartbeat. The counters are firmware averages.
constexpr int64_t kMetricsMaxAgeMs = 10;

struct SteadyClockUs {
  int64_t operator()() const {
    return std::chrono::duration_cast<std::chrono::microseconds>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
  }
};

// The last sample per processor index and when it was taken. `NowUs` is a
// callable returning microseconds on a monotonic clock; the self-test passes
// one it sets by hand. Safe to call from any thread: the device read runs
// outside the lock, so two callers that miss together may both read, and
// each gets a whole Metrics.
template <class NowUs = SteadyClockUs>
class MetricsCache {
 public:
  explicit MetricsCache(NowUs now = NowUs()) : now_(std::move(now)) {}

  // The stored sample of `index` if it is younger than max_age_ms, else what
  // `read()` returns, which is then stored. max_age_ms <= 0 always reads.
  template <class Read>
  Metrics get_or_read(uint32_t index, int64_t max_age_ms, Read&& read) {
    int64_t t;
    uint64_t generation;
    {
      std::lock_guard<std::mutex> lk(mu_);
      t = now_();
      if (max_age_ms > 0 && index < slots_.size() && slots_[index].valid &&
          t - slots_[index].taken_us < max_age_ms * 1000)
        return slots_[index].metrics;
      generation = generation_;
    }
    Metrics m = read();
    std::lock_guard<std::mutex> lk(mu_);
    // a sample read before an invalidate() must not outlive it
    if (generation == generation_) {
      if (index >= slots_.size()) slots_.resize(index + 1);
      slots_[index] = Slot{m, t, true};
    }
    return m;
  }

  // Drop every sample: after a mode set the processor population and the
  // load picture are both different.
  void invalidate() {
    std::lock_guard<std::mutex> lk(mu_);
    slots_.clear();
    ++generation_;
  }

 private:
  struct Slot {
    Metrics metrics;
    int64_t taken_us = 0;  // clock at the start of the read: never too young
    bool valid = false;
  };

  NowUs now_;
  std::mutex mu_;
  std::vector<Slot> slots_;
  uint64_t generation_ = 0;
};

}  // namespace partitiond
