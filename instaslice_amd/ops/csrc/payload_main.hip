// instaslice-payload: standalone workload binary run *inside* partitions.
//
// The MI355X analog of the reference's cuda-vectoradd sample container
// (samples/test-pod.yaml:12): the node agent / e2e tests exec this binary
// with ROCR_VISIBLE_DEVICES set from the pod's ConfigMap, so it exercises
// exactly the device set a real pod would see. Prints one JSON line.
//
//   instaslice-payload info
//   instaslice-payload vecadd [N]             N >= 1 floats, operands derived
//                                             from the element index; exit 1
//                                             unless max_err == 0
//   instaslice-payload membw [BYTES [ITERS [BLOCKS [NT]]]]
//                                             streaming copy, then the
//                                             destination checked against the
//                                             index-derived pattern; exit 1
//                                             iff bad_units != 0
//   instaslice-payload busy [MS]              MS finite, in 0 .. 60000; prints
//                                             the device-side elapsed_ms
//   instaslice-payload census
//   instaslice-payload gemm [M N K [ITERS]]   bf16 MFMA GEMM, exact-checked
//                                             and timed (default 4096 4096
//                                             1024, 10 iters; K <= 1024);
//                                             exit 1 unless max_err == 0
//   instaslice-payload mxgemm [M N K [ITERS]] MXFP8 block-scaled MFMA GEMM
//                                             (e4m3 operands, E8M0 scales per
//                                             32 elements), exact-checked and
//                                             timed (default 4096 4096 2048,
//                                             10 iters; K <= 2048);
//                                             exit 1 unless max_err == 0
//   instaslice-payload mx4gemm [M N K [ITERS]] MXFP4 block-scaled MFMA GEMM
//                                             (e2m1 operands, two to a byte,
//                                             E8M0 scales per 32 elements),
//                                             exact-checked and timed on the
//                                             mxgemm pattern (default 4096
//                                             4096 2048, 10 iters; K <= 2048);
//                                             exit 1 unless max_err == 0
//   instaslice-payload memcheck [BYTES [PASSES [FLIP_OFFSET FLIP_MASK]]]
//                                             moving-inversions memory test
//                                             of one BYTES buffer (default
//                                             1 GiB, 1 pass); FLIP_* corrupt
//                                             one word once (self-test);
//                                             "beyond_llc" says whether BYTES
//                                             exceeds the 256 MiB Infinity
//                                             Cache (below it the run proves
//                                             the kernel, not the HBM);
//                                             exit 1 iff bad_words != 0
//   instaslice-payload attn [B HQ HKV L [ITERS [SPLITS]]]
//                                             KV-cache decode attention (bf16
//                                             MFMA, fp32 online softmax,
//                                             split-KV; head dim 128): the
//                                             self-check at 2 8 2 300 (exact
//                                             pattern and a dense pattern
//                                             against fp64), then a timed run
//                                             (default 32 64 8 4096, 10 iters:
//                                             512 MiB of K and V per step)
//                                             with 16 rows checked exactly;
//                                             SPLITS (0 or absent: auto) fixes
//                                             the KV split count of the timed
//                                             run; exit 1 unless max_err == 0
//                                             and max_rel <= 2^-8
//   instaslice-payload prefill [B HQ HKV L [ITERS [CAUSAL [PATTERN]]]]
//                                             causal prefill attention (bf16
//                                             MFMA, K and V tiles through LDS,
//                                             fp32 online softmax; head dim
//                                             128): the self-check at 2 8 2 300
//                                             (exact pattern and a dense
//                                             pattern against fp64), then a
//                                             timed run on the dense pattern
//                                             (default 8 64 8 4096, 10 iters,
//                                             CAUSAL 1) with 16 rows checked
//                                             against fp64; TFLOP/s counts the
//                                             unmasked pairs only; PATTERN 1
//                                             times the selection pattern
//                                             instead (low-entropy data: a
//                                             flattering rate, for comparison
//                                             only); exit 1 unless max_err ==
//                                             0 and max_rel <= 2^-8
//   instaslice-payload verify [XCDS]          census + vecadd + gemm check +
//                                             membw + timed gemm in one JSON
//                                             line; XCDS (0 or absent: not
//                                             checked) is the XCD count the
//                                             partition should show. Only
//                                             vecadd, gemm, xcds and membw's
//                                             bad_units are judged; rates are
//                                             reported.
//                                             exit 1 iff "failed" is non-empty
//   instaslice-payload serve      (persistent worker: commands on stdin,
//                                  one JSON line per command on stdout —
//                                  HIP init is paid once, so a warm pool
//                                  can run a kernel per pod lifecycle at
//                                  production rate; NOTE the live process
//                                  holds the device, which blocks
//                                  partition mode flips: serve is for
//                                  static-partitioning phases only)
//
// Build: see build_native.py (hipcc --offload-arch=gfx950).

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "payload_core.hpp"

using namespace payload;

// JSON has no inf/nan: an error that is not finite prints as a huge number
static double json_num(double v) { return std::isfinite(v) ? v : 1e300; }

static bool print_vecadd(size_t n) {
  double err = run_vecadd(n);
  std::printf("{\"ok\": %s, \"cmd\": \"vecadd\", \"n\": %zu, \"max_err\": %g}\n",
              err == 0.0 ? "true" : "false", n, json_num(err));
  return err == 0.0;
}

// "nan" and "inf" parse as such and are then rejected by run_busy
static void print_busy(const char* ms_text) {
  double ms = std::strtod(ms_text, nullptr);
  BusyResult r = run_busy(ms);
  std::printf(
      "{\"ok\": true, \"cmd\": \"busy\", \"ms\": %.1f, \"elapsed_ms\": %.3f, "
      "\"iters\": %llu, \"guard_hit\": %s}\n",
      ms, r.elapsed_ms, r.iters, r.guard_hit ? "true" : "false");
}

// one JSON line for a memcheck result; bad_bits is a string because a u64
// does not survive a JSON double
static bool print_memcheck(const MemcheckResult& r) {
  bool ok = r.bad_words == 0;
  std::printf(
      "{\"ok\": %s, \"cmd\": \"memcheck\", \"bytes\": %zu, \"passes\": %d, "
      "\"bad_words\": %llu, \"first_bad_offset\": %lld, \"bad_bits\": \"0x%llx\", "
      "\"fill_gb_per_s\": %.1f, \"check_gb_per_s\": %.1f, \"ms\": %.3f, "
      "\"beyond_llc\": %s}\n",
      ok ? "true" : "false", r.bytes, r.passes,
      static_cast<unsigned long long>(r.bad_words),
      static_cast<long long>(r.first_bad_offset),
      static_cast<unsigned long long>(r.bad_bits), r.fill_gb_s, r.check_gb_s,
      r.ms, r.bytes > kMemcheckLlcBytes ? "true" : "false");
  return ok;
}

// the three GEMM payloads share their verbs' arguments and report lines
struct GemmVerb {
  const char* name;
  GemmResult (*run)(int m, int n, int k, int iters, int device);
  double (*check)(int m, int n, int k, int device);
  int default_k;
};

static const GemmVerb kGemmVerbs[] = {
    {"gemm", run_gemm, run_gemm_check, 1024},
    {"mxgemm", run_mxgemm, run_mxgemm_check, 2048},
    {"mx4gemm", run_mx4gemm, run_mx4gemm_check, 2048},
};

static const GemmVerb* find_gemm_verb(const char* name) {
  for (const GemmVerb& g : kGemmVerbs)
    if (std::strcmp(name, g.name) == 0) return &g;
  return nullptr;
}

// <verb> [M N K [ITERS]]: the timed run
static bool print_timed_gemm(const GemmVerb& g, int argc, char** argv) {
  int m = argc > 4 ? std::atoi(argv[2]) : 4096;
  int n = argc > 4 ? std::atoi(argv[3]) : 4096;
  int k = argc > 4 ? std::atoi(argv[4]) : g.default_k;
  int iters = argc > 5 ? std::atoi(argv[5]) : 10;
  GemmResult r = g.run(m, n, k, iters, 0);
  bool ok = r.max_err == 0.0;
  std::printf(
      "{\"ok\": %s, \"cmd\": \"%s\", \"m\": %d, \"n\": %d, \"k\": %d, "
      "\"iters\": %d, \"tflops\": %.2f, \"max_err\": %g}\n",
      ok ? "true" : "false", g.name, m, n, k, iters, r.tflops, json_num(r.max_err));
  return ok;
}

// serve's <verb> [M N K]: the full check
static void print_gemm_check(const GemmVerb& g, std::istringstream& iss) {
  int m = 96, n = 160, k = 224, tm, tn, tk;
  if (iss >> tm >> tn >> tk) { m = tm; n = tn; k = tk; }
  double err = g.check(m, n, k, 0);
  std::printf(
      "{\"ok\": %s, \"cmd\": \"%s\", \"m\": %d, \"n\": %d, "
      "\"k\": %d, \"max_err\": %g}\n",
      err == 0.0 ? "true" : "false", g.name, m, n, k, json_num(err));
}

// the two attention payloads share their verbs' shape arguments and the head
// of their report lines; a verb starts from its defaults
struct AttnArgs {
  int b, hq, hkv, len;

  // <verb> [B HQ HKV L [...]]: all four or none
  void parse(int argc, char** argv) {
    if (argc > 5)
      *this = {std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]),
               std::atoi(argv[5])};
  }

  // serve's <verb> [B HQ HKV L]
  void parse(std::istringstream& iss) {
    int tb, tq, tk, tl;
    if (iss >> tb >> tq >> tk >> tl) *this = {tb, tq, tk, tl};
  }

  void print_head(const char* cmd, bool ok) const {
    std::printf(
        "{\"ok\": %s, \"cmd\": \"%s\", \"batch\": %d, \"hq\": %d, \"hkv\": %d, "
        "\"len\": %d, ",
        ok ? "true" : "false", cmd, b, hq, hkv, len);
  }
};

// serve's attn / prefill [B HQ HKV L]: the self-check at that shape; `extra`
// goes between the head and the errors
static void print_attn_check(const char* cmd, const AttnArgs& a, const AttnCheck& c,
                             const char* extra) {
  bool ok = c.max_err == 0.0 && c.max_rel <= kAttnRelBound;
  a.print_head(cmd, ok);
  std::printf("%s\"max_err\": %g, \"max_rel\": %g}\n", extra, json_num(c.max_err),
              json_num(c.max_rel));
}

// one census run: the XCDs that ran a workgroup, and the per-XCD counts as the
// elements of a JSON array
struct Census {
  std::vector<unsigned int> per_xcd = run_xcd_census();

  int xcds() const {
    int n = 0;
    for (unsigned v : per_xcd)
      if (v) ++n;
    return n;
  }

  void print_per_xcd() const {
    for (int i = 0; i < 8; ++i) std::printf("%s%u", i ? ", " : "", per_xcd[i]);
  }
};

int main(int argc, char** argv) {
  const char* cmd = argc > 1 ? argv[1] : "info";
  try {
    if (std::strcmp(cmd, "info") == 0) {
      int n = device_count();
      std::printf("{\"ok\": true, \"devices\": %d", n);
      if (n > 0) {
        DeviceInfo i = get_device_info(0);
        std::printf(
            ", \"name\": \"%s\", \"gcn_arch\": \"%s\", \"cu_count\": %d, "
            "\"total_mem_gb\": %.1f, \"xcd_count_visible\": %d",
            i.name.c_str(), i.gcn_arch.c_str(), i.cu_count, i.total_mem_gb,
            i.xcd_count_visible);
      }
      std::printf("}\n");
    } else if (std::strcmp(cmd, "vecadd") == 0) {
      size_t n = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : (1 << 24);
      return print_vecadd(n) ? 0 : 1;
    } else if (std::strcmp(cmd, "membw") == 0) {
      size_t bytes = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : (size_t{1} << 30);
      int iters = argc > 3 ? std::atoi(argv[3]) : 10;
      int blocks = argc > 4 ? std::atoi(argv[4]) : 0;
      bool nt = argc > 5 && std::atoi(argv[5]) != 0;
      MembwResult r = run_membw_check(bytes, iters, 0, blocks, nt);
      bool ok = r.bad_units == 0;
      std::printf(
          "{\"ok\": %s, \"cmd\": \"membw\", \"bytes\": %zu, \"iters\": %d, "
          "\"blocks\": %d, \"nontemporal\": %s, \"gb_per_s\": %.1f, "
          "\"bad_units\": %llu}\n",
          ok ? "true" : "false", bytes, iters, blocks, nt ? "true" : "false", r.gb_s,
          r.bad_units);
      return ok ? 0 : 1;
    } else if (std::strcmp(cmd, "busy") == 0) {
      print_busy(argc > 2 ? argv[2] : "100");
    } else if (std::strcmp(cmd, "census") == 0) {
      Census census;
      std::printf("{\"ok\": true, \"cmd\": \"census\", \"per_xcd\": [");
      census.print_per_xcd();
      std::printf("], \"xcds_visible\": %d}\n", census.xcds());
    } else if (const GemmVerb* g = find_gemm_verb(cmd)) {
      return print_timed_gemm(*g, argc, argv) ? 0 : 1;
    } else if (std::strcmp(cmd, "attn") == 0) {
      AttnArgs a{32, 64, 8, 4096};
      a.parse(argc, argv);
      int iters = argc > 6 ? std::atoi(argv[6]) : 10;
      int splits = argc > 7 ? std::atoi(argv[7]) : 0;
      AttnCheck c = run_attn_check(2, 8, 2, 300);
      AttnResult r = run_attn(a.b, a.hq, a.hkv, a.len, iters, 0, splits);
      double max_err = r.max_err > c.max_err ? r.max_err : c.max_err;
      bool ok = max_err == 0.0 && c.max_rel <= kAttnRelBound;
      a.print_head("attn", ok);
      std::printf(
          "\"iters\": %d, \"kv_gb_per_s\": %.1f, \"steps_per_s\": %.1f, "
          "\"tok_per_s\": %.1f, \"max_err\": %g, \"max_rel\": %g}\n",
          iters, r.kv_gb_s, r.steps_per_s, r.tok_per_s, json_num(max_err),
          json_num(c.max_rel));
      return ok ? 0 : 1;
    } else if (std::strcmp(cmd, "prefill") == 0) {
      AttnArgs a{8, 64, 8, 4096};
      a.parse(argc, argv);
      int iters = argc > 6 ? std::atoi(argv[6]) : 10;
      bool causal = argc > 7 ? std::atoi(argv[7]) != 0 : true;
      int pattern = argc > 8 ? std::atoi(argv[8]) : kPrefillDense;
      AttnCheck c = run_prefill_check(2, 8, 2, 300, causal);
      PrefillResult r = run_prefill(a.b, a.hq, a.hkv, a.len, iters, causal, 0, pattern);
      double max_rel = r.max_rel > c.max_rel ? r.max_rel : c.max_rel;
      if (std::isnan(r.max_rel) || std::isnan(c.max_rel)) max_rel = INFINITY;
      bool ok = c.max_err == 0.0 && max_rel <= kAttnRelBound;
      a.print_head("prefill", ok);
      std::printf(
          "\"iters\": %d, \"causal\": %s, \"tflops\": %.2f, \"tok_per_s\": %.1f, "
          "\"max_err\": %g, \"max_rel\": %g}\n",
          iters, causal ? "true" : "false", r.tflops, r.tok_per_s, json_num(c.max_err),
          json_num(max_rel));
      return ok ? 0 : 1;
    } else if (std::strcmp(cmd, "memcheck") == 0) {
      size_t bytes = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : (size_t{1} << 30);
      int passes = argc > 3 ? std::atoi(argv[3]) : 1;
      int64_t flip_offset = argc > 5 ? std::strtoll(argv[4], nullptr, 10) : -1;
      uint64_t flip_mask = argc > 5 ? std::strtoull(argv[5], nullptr, 0) : 0;
      return print_memcheck(run_memcheck(bytes, passes, 0, 0, flip_offset, flip_mask))
                 ? 0 : 1;
    } else if (std::strcmp(cmd, "verify") == 0) {
      int expected = argc > 2 ? std::atoi(argv[2]) : 0;
      DeviceInfo info = get_device_info(0);
      Census census;
      int xcds = census.xcds();
      double vecadd_err = run_vecadd(1 << 20);
      double gemm_err = run_gemm_check(96, 160, 224);
      MembwResult mb = run_membw_check(size_t{256} << 20, 5);
      double gbs = mb.gb_s;
      GemmResult r = run_gemm(4096, 4096, 1024, 5);
      if (r.max_err > gemm_err) gemm_err = r.max_err;
      bool bad_vecadd = vecadd_err != 0.0;
      bool bad_gemm = gemm_err != 0.0;
      bool bad_xcds = expected > 0 && xcds != expected;
      bool bad_membw = mb.bad_units != 0;
      bool ok = !(bad_vecadd || bad_gemm || bad_xcds || bad_membw);
      std::printf("{\"ok\": %s, \"cmd\": \"verify\", \"xcds_expected\": %d, "
                  "\"xcds_visible\": %d, \"per_xcd\": [",
                  ok ? "true" : "false", expected, xcds);
      census.print_per_xcd();
      int per = xcds > 0 ? xcds : 1;
      std::printf(
          "], \"cu_count\": %d, \"total_mem_gb\": %.1f, \"vecadd_max_err\": %g, "
          "\"gemm_max_err\": %g, \"membw_bad_units\": %llu, \"gb_per_s\": %.1f, "
          "\"tflops\": %.2f, \"gb_per_s_per_xcd\": %.1f, \"tflops_per_xcd\": %.2f, "
          "\"failed\": [",
          info.cu_count, info.total_mem_gb, json_num(vecadd_err),
          json_num(gemm_err), mb.bad_units, gbs, r.tflops, gbs / per, r.tflops / per);
      const char* sep = "";
      if (bad_vecadd) { std::printf("%s\"vecadd\"", sep); sep = ", "; }
      if (bad_gemm) { std::printf("%s\"gemm\"", sep); sep = ", "; }
      if (bad_xcds) { std::printf("%s\"xcds\"", sep); sep = ", "; }
      if (bad_membw) { std::printf("%s\"membw\"", sep); sep = ", "; }
      std::printf("]}\n");
      return ok ? 0 : 1;
    } else if (std::strcmp(cmd, "serve") == 0) {
      // warm-pool worker: one line per request, one JSON line per reply
      //   vecadd <n> | busy <ms> | gemm [M N K] | mxgemm [M N K] |
      //   mx4gemm [M N K] | attn [B HQ HKV L] | prefill [B HQ HKV L] |
      //   memcheck [BYTES] | ping | quit
      std::string line;
      while (std::getline(std::cin, line)) {
        std::istringstream iss(line);
        std::string verb;
        iss >> verb;
        if (verb.empty()) continue;
        try {
          if (verb == "quit") { std::printf("{\"ok\": true}\n"); break; }
          if (verb == "ping") {
            std::printf("{\"ok\": true, \"cmd\": \"ping\"}\n");
          } else if (verb == "vecadd") {
            size_t n = 1 << 20;
            iss >> n;
            print_vecadd(n);
          } else if (const GemmVerb* g = find_gemm_verb(verb.c_str())) {
            print_gemm_check(*g, iss);
          } else if (verb == "attn") {
            AttnArgs a{2, 8, 2, 300};
            a.parse(iss);
            print_attn_check("attn", a, run_attn_check(a.b, a.hq, a.hkv, a.len), "");
          } else if (verb == "prefill") {
            AttnArgs a{1, 4, 2, 200};
            a.parse(iss);
            print_attn_check("prefill", a, run_prefill_check(a.b, a.hq, a.hkv, a.len),
                             "\"causal\": true, ");
          } else if (verb == "memcheck") {
            size_t bytes = size_t{64} << 20;
            iss >> bytes;
            print_memcheck(run_memcheck(bytes));
          } else if (verb == "busy") {
            std::string ms = "10";  // as text: operator>> does not read "nan"
            iss >> ms;
            print_busy(ms.c_str());
          } else {
            std::printf("{\"ok\": false, \"error\": \"unknown verb\"}\n");
          }
        } catch (const std::exception& e) {
          std::printf("{\"ok\": false, \"error\": \"%s\"}\n", e.what());
        }
        std::fflush(stdout);
      }
    } else {
      std::fprintf(stderr, "unknown command: %s\n", cmd);
      return 2;
    }
  } catch (const std::exception& e) {
    std::printf("{\"ok\": false, \"error\": \"%s\"}\n", e.what());
    return 1;
  }
  return 0;
}
