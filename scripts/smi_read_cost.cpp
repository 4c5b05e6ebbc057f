// What one counter sample costs in libamd_smi, call by call.
//
// Times amdsmi_get_gpu_activity, amdsmi_get_gpu_memory_usage,
// amdsmi_get_power_info, amdsmi_get_gpu_metrics_info and the three-call
// sequence the device layer used to make per sample, 2000 times each on
// processor 0, and prints median and p99. Opens no HIP context and changes
// no setting. The table it printed on an MI355X is in
// profiles/smi_metrics.md, with the compile command.

#include <amd_smi/amdsmi.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

static const int kReps = 2000;

static amdsmi_processor_handle first_processor() {
  uint32_t nsock = 0;
  if (amdsmi_get_socket_handles(&nsock, nullptr) != AMDSMI_STATUS_SUCCESS || !nsock)
    return nullptr;
  std::vector<amdsmi_socket_handle> socks(nsock);
  if (amdsmi_get_socket_handles(&nsock, socks.data()) != AMDSMI_STATUS_SUCCESS)
    return nullptr;
  uint32_t nproc = 0;
  if (amdsmi_get_processor_handles(socks[0], &nproc, nullptr) != AMDSMI_STATUS_SUCCESS ||
      !nproc)
    return nullptr;
  std::vector<amdsmi_processor_handle> procs(nproc);
  if (amdsmi_get_processor_handles(socks[0], &nproc, procs.data()) != AMDSMI_STATUS_SUCCESS)
    return nullptr;
  return procs[0];
}

template <class F>
static void time_it(const char* name, F&& call) {
  std::vector<double> us(kReps);
  int last = 0;
  for (int i = 0; i < 20; ++i) last = call();  // first calls open sysfs files
  for (int i = 0; i < kReps; ++i) {
    auto t0 = std::chrono::steady_clock::now();
    last = call();
    auto t1 = std::chrono::steady_clock::now();
    us[i] = std::chrono::duration<double, std::micro>(t1 - t0).count();
  }
  std::sort(us.begin(), us.end());
  std::printf("%-34s status %2d  median %8.1f us  p99 %8.1f us\n", name, last,
              us[kReps / 2], us[kReps * 99 / 100]);
}

int main() {
  if (amdsmi_init(AMDSMI_INIT_AMD_GPUS) != AMDSMI_STATUS_SUCCESS) {
    std::fprintf(stderr, "amdsmi_init failed\n");
    return 1;
  }
  amdsmi_processor_handle h = first_processor();
  if (!h) {
    std::fprintf(stderr, "no processor\n");
    amdsmi_shut_down();
    return 1;
  }

  amdsmi_engine_usage_t usage;
  amdsmi_power_info_t power;
  static amdsmi_gpu_metrics_t table;
  uint64_t used = 0;
  std::memset(&usage, 0, sizeof(usage));
  std::memset(&power, 0, sizeof(power));
  std::memset(&table, 0, sizeof(table));

  time_it("amdsmi_get_gpu_activity", [&] { return (int)amdsmi_get_gpu_activity(h, &usage); });
  time_it("amdsmi_get_gpu_memory_usage",
          [&] { return (int)amdsmi_get_gpu_memory_usage(h, AMDSMI_MEM_TYPE_VRAM, &used); });
  time_it("amdsmi_get_power_info", [&] { return (int)amdsmi_get_power_info(h, &power); });
  time_it("amdsmi_get_gpu_metrics_info",
          [&] { return (int)amdsmi_get_gpu_metrics_info(h, &table); });
  time_it("activity + memory_usage + power", [&] {
    int a = amdsmi_get_gpu_activity(h, &usage);
    int b = amdsmi_get_gpu_memory_usage(h, AMDSMI_MEM_TYPE_VRAM, &used);
    int c = amdsmi_get_power_info(h, &power);
    return a ? a : b ? b : c;
  });
  time_it("metrics_info + memory_usage", [&] {
    int a = amdsmi_get_gpu_metrics_info(h, &table);
    int b = amdsmi_get_gpu_memory_usage(h, AMDSMI_MEM_TYPE_VRAM, &used);
    return a ? a : b;
  });

  // what each source reported last, to see which fields the table carries
  std::printf("activity:  gfx %u umc %u\n", usage.gfx_activity, usage.umc_activity);
  std::printf("power:     socket %llu current %u average %u\n",
              (unsigned long long)power.socket_power, power.current_socket_power,
              power.average_socket_power);
  std::printf("table:     gfx %u umc %u current_socket_power %u average_socket_power %u\n",
              table.average_gfx_activity, table.average_umc_activity,
              table.current_socket_power, table.average_socket_power);
  std::printf("vram used: %llu bytes\n", (unsigned long long)used);
  std::printf("sizeof(amdsmi_gpu_metrics_t) = %zu\n", sizeof(table));

  amdsmi_shut_down();
  return 0;
}
