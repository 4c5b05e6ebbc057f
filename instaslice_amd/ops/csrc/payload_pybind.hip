// Python bindings for the gfx950 payload kernels (payload_core.hpp).
// Built in-tree as instaslice_amd/ops/_payload*.so by build_native.py
// (hipcc --offload-arch=gfx950). Fails loudly at call time if no GPU.

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <array>
#include <tuple>

#include "payload_core.hpp"

namespace py = pybind11;

namespace {

// float32 arrays convert through forcecast | c_style: a non-contiguous or
// other-dtype array is copied into a contiguous float32 one, and anything
// that cannot be converted is a TypeError
template <class T>
using c_array = py::array_t<T, py::array::c_style | py::array::forcecast>;
using f32_array = c_array<float>;
using u32_array = c_array<uint32_t>;
using u8_array = c_array<uint8_t>;

// out[i] = f(x[i]): an array of x's shape, any rank
template <class Out, class In>
py::array_t<Out> map_elements(const c_array<In>& x, Out (*f)(In)) {
  py::array_t<Out> out(std::vector<py::ssize_t>(x.shape(), x.shape() + x.ndim()));
  const In* src = x.data();
  Out* dst = out.mutable_data();
  for (py::ssize_t i = 0, n = x.size(); i < n; ++i) dst[i] = f(src[i]);
  return out;
}

// K, the length of the rows of x along its last axis, or ValueError; `what`
// is the argument's name in the message
int last_axis(const char* who, const char* what, const py::array& x) {
  if (x.ndim() < 1)
    throw py::value_error(std::string(who) + ": " + what +
                          " must have at least one axis");
  if (x.shape(x.ndim() - 1) < 1 || x.shape(x.ndim() - 1) > INT32_MAX)
    throw py::value_error(std::string(who) + ": bad length of the last axis");
  return static_cast<int>(x.shape(x.ndim() - 1));
}

// out[..., :] = row(x[..., :]) along the last axis: one uint8 array per width
// in `widths`, shaped like x but that long in the last axis; row(src, dst...)
// is called once per row of K elements with the row's place in each output
template <class In, class... Width, class Row>
auto map_rows(const c_array<In>& x, int K, Row row, Width... widths) {
  std::vector<py::ssize_t> shape(x.shape(), x.shape() + x.ndim());
  auto like = [&shape](py::ssize_t width) {
    shape.back() = width;
    return py::array_t<uint8_t>(shape);
  };
  std::tuple outs{like(widths)...};
  const In* src = x.data();
  for (py::ssize_t r = 0, rows = x.size() / K; r < rows; ++r)
    std::apply(
        [&](auto&... out) {
          row(src + r * K, K, (out.mutable_data() + r * out.shape(out.ndim() - 1))...);
        },
        outs);
  return outs;
}

void no_nan(const char* who, const f32_array& x) {
  const float* src = x.data();
  for (py::ssize_t i = 0, n = x.size(); i < n; ++i)
    if (std::isnan(src[i]))
      throw py::value_error(std::string(who) + ": x has a NaN element (e2m1 has no NaN)");
}

void e2m1_codes(const char* who, const u8_array& codes) {
  const uint8_t* src = codes.data();
  for (py::ssize_t i = 0, n = codes.size(); i < n; ++i)
    if (src[i] > 15)
      throw py::value_error(std::string(who) + ": an e2m1 code must be in 0 .. 15");
}

void any_code(const char*, const u8_array&) {}  // every byte is an e4m3 code

// (codes uint8 [..., K], scales uint8 [..., ceil(K/32)]) of one of the MX
// quantizers along the last axis
using QuantizeRow = void (*)(const float*, int, uint8_t*, uint8_t*);
auto quantize_rows(const f32_array& x, int K, QuantizeRow quantize) {
  const py::ssize_t blocks = (K + payload::kMxBlock - 1) / payload::kMxBlock;
  auto [codes, scales] = map_rows(x, K, quantize, py::ssize_t{K}, blocks);
  return py::make_tuple(codes, scales);
}

// (M, N, K) of an (M,K) x (K,N) product, or ValueError
std::array<int, 3> gemm_dims(const char* who, const py::array& a, const py::array& b) {
  std::string w(who);
  if (a.ndim() != 2 || b.ndim() != 2)
    throw py::value_error(w + ": a and b must be 2-D");
  if (a.shape(1) != b.shape(0))
    throw py::value_error(w + ": a is (M,K) and b is (K,N): K differs");
  if (a.shape(0) < 1 || a.shape(1) < 1 || b.shape(1) < 1)
    throw py::value_error(w + ": empty operand");
  if (a.shape(0) > INT32_MAX || a.shape(1) > INT32_MAX || b.shape(1) > INT32_MAX)
    throw py::value_error(w + ": shape too large");
  return std::array<int, 3>{static_cast<int>(a.shape(0)),
                            static_cast<int>(b.shape(1)),
                            static_cast<int>(a.shape(1))};
}

// C (M,N) of one of the general GEMM entries on float operands
using GemmEntry = void (*)(const float*, const float*, float*, int, int, int, int);
py::array_t<float> gemm_f32(const char* who, GemmEntry entry, const f32_array& a,
                            const f32_array& b, int device) {
  auto [M, N, K] = gemm_dims(who, a, b);
  py::array_t<float> c({static_cast<py::ssize_t>(M), static_cast<py::ssize_t>(N)});
  const float* pa = a.data();
  const float* pb = b.data();
  float* pc = c.mutable_data();
  {
    py::gil_scoped_release rel;
    entry(pa, pb, pc, M, N, K, device);
  }
  return c;
}

// C (M,N) of one of the raw MX GEMM entries; check_codes rejects what is no
// code of the entry's element format
using GemmRawEntry = void (*)(const uint8_t*, const uint8_t*, const uint8_t*,
                              const uint8_t*, float*, int, int, int, int);
py::array_t<float> gemm_raw(const char* who, GemmRawEntry entry,
                            void (*check_codes)(const char*, const u8_array&),
                            const u8_array& a_codes, const u8_array& a_scales,
                            const u8_array& b_codes, const u8_array& b_scales,
                            int device) {
  std::string w(who);
  auto [M, N, K] = gemm_dims(who, a_codes, b_codes);
  const py::ssize_t blocks = (K + payload::kMxBlock - 1) / payload::kMxBlock;
  if (a_scales.ndim() != 2 || a_scales.shape(0) != M || a_scales.shape(1) != blocks)
    throw py::value_error(w + ": a_scales must be (M, ceil(K/32))");
  if (b_scales.ndim() != 2 || b_scales.shape(0) != blocks || b_scales.shape(1) != N)
    throw py::value_error(w + ": b_scales must be (ceil(K/32), N)");
  check_codes(who, a_codes);
  check_codes(who, b_codes);
  py::array_t<float> c({static_cast<py::ssize_t>(M), static_cast<py::ssize_t>(N)});
  const uint8_t* pa = a_codes.data();
  const uint8_t* psa = a_scales.data();
  const uint8_t* pb = b_codes.data();
  const uint8_t* psb = b_scales.data();
  float* pc = c.mutable_data();
  {
    py::gil_scoped_release rel;
    entry(pa, psa, pb, psb, pc, M, N, K, device);
  }
  return c;
}

// the report of one of the timed GEMM runs
using TimedGemm = payload::GemmResult (*)(int, int, int, int, int);
py::dict run_timed_gemm(TimedGemm run, int mm, int n, int k, int iters, int device) {
  payload::GemmResult r;
  {
    py::gil_scoped_release rel;
    r = run(mm, n, k, iters, device);
  }
  py::dict d;
  d["m"] = mm;
  d["n"] = n;
  d["k"] = k;
  d["iters"] = iters;
  d["tflops"] = r.tflops;
  d["max_err"] = r.max_err;
  return d;
}

// the attention entries' q, k and v: q of rank q_rank (q_form in the message),
// k and v (B,Hkv,L,128) and alike, head dim 128, one batch; or ValueError
void attn_operands(const char* who, const f32_array& q, int q_rank, const char* q_form,
                   const f32_array& k, const f32_array& v) {
  std::string w(who);
  if (q.ndim() != q_rank) throw py::value_error(w + ": q must be " + q_form);
  if (k.ndim() != 4 || v.ndim() != 4)
    throw py::value_error(w + ": k and v must be (B,Hkv,L,128)");
  if (q.shape(q_rank - 1) != payload::kAttnD || k.shape(3) != payload::kAttnD)
    throw py::value_error(w + ": head dim must be 128");
  for (int i = 0; i < 4; ++i)
    if (k.shape(i) != v.shape(i)) throw py::value_error(w + ": k and v differ in shape");
  if (k.shape(0) != q.shape(0)) throw py::value_error(w + ": q and k differ in batch");
}

// scale=None is 1/sqrt(128); ValueError on a scale that is not finite
float attn_scale(const char* who, const py::object& scale) {
  if (scale.is_none()) return 1.0f / std::sqrt(static_cast<float>(payload::kAttnD));
  float sc = scale.cast<float>();
  if (!std::isfinite(sc)) throw py::value_error(std::string(who) + ": scale not finite");
  return sc;
}

// ValueError unless every element of q, k and v is finite
void attn_finite(const char* who, const f32_array& q, const f32_array& k,
                 const f32_array& v) {
  const float* pq = q.data();
  const float* pk = k.data();
  const float* pv = v.data();
  for (py::ssize_t i = 0, n = q.size(); i < n; ++i)
    if (!std::isfinite(pq[i]))
      throw py::value_error(std::string(who) + ": q has a non-finite element");
  for (py::ssize_t i = 0, n = k.size(); i < n; ++i)
    if (!std::isfinite(pk[i]) || !std::isfinite(pv[i]))
      throw py::value_error(std::string(who) + ": k or v has a non-finite element");
}

// (q, k, v, expected) of one of the selection patterns: q and expected of
// q_shape, k and v (B,Hkv,L,128), filled by fill(q, k, v, expected)
template <class Fill>
py::tuple attn_pattern_arrays(const std::vector<py::ssize_t>& q_shape, py::ssize_t B,
                              py::ssize_t Hkv, py::ssize_t L, Fill fill) {
  const std::vector<py::ssize_t> kv_shape{B, Hkv, L, payload::kAttnD};
  py::array_t<float> q(q_shape), e(q_shape), k(kv_shape), v(kv_shape);
  fill(q.mutable_data(), k.mutable_data(), v.mutable_data(), e.mutable_data());
  return py::make_tuple(q, k, v, e);
}

// the report of one of the attention self-checks
py::dict attn_check_dict(const payload::AttnCheck& r) {
  py::dict d;
  d["max_err"] = r.max_err;
  d["max_rel"] = r.max_rel;
  return d;
}

// the shape keys that head the report of one of the timed attention runs
py::dict attn_timed_dict(int batch, int hq, int hkv, int length, int iters) {
  py::dict d;
  d["batch"] = batch;
  d["hq"] = hq;
  d["hkv"] = hkv;
  d["len"] = length;
  d["iters"] = iters;
  return d;
}

}  // namespace

PYBIND11_MODULE(_payload, m) {
  m.doc() = "gfx950 HIP payload kernels (vecadd / membw / busy / xcd census / gemm / "
            "mxgemm / mx4gemm / memcheck / attn / prefill)";

  m.def("device_count", &payload::device_count,
        "Number of visible HIP devices (0 if no GPU/driver)");

  m.def(
      "run_vecadd",
      [](size_t n, int device) {
        py::gil_scoped_release rel;
        return payload::run_vecadd(n, device);
      },
      py::arg("n") = (1 << 20), py::arg("device") = 0,
      "c = a + b over n >= 1 floats on `device`, operands derived from the element "
      "index; returns max abs error (expect 0)");

  m.def(
      "run_membw",
      [](size_t bytes, int iters, int device) {
        py::gil_scoped_release rel;
        return payload::run_membw(bytes, iters, device);
      },
      py::arg("bytes") = (size_t{1} << 30), py::arg("iters") = 10,
      py::arg("device") = 0,
      "streaming-copy bandwidth probe; returns GB/s (read+write); RuntimeError if "
      "the copy's destination does not hold the pattern");

  m.def(
      "run_membw_check",
      [](size_t bytes, int iters, int device, int blocks, bool nontemporal) {
        payload::MembwResult r;
        {
          py::gil_scoped_release rel;
          r = payload::run_membw_check(bytes, iters, device, blocks, nontemporal);
        }
        py::dict d;
        d["gb_per_s"] = r.gb_s;
        d["bad_units"] = r.bad_units;
        return d;
      },
      py::arg("bytes") = (size_t{1} << 30), py::arg("iters") = 10,
      py::arg("device") = 0, py::arg("blocks") = 0, py::arg("nontemporal") = false,
      "streaming-copy bandwidth probe with its check: GB/s (read+write) and the "
      "number of 16-byte units of the destination that differ from the "
      "index-derived pattern (expect 0); blocks=0 is the default grid");

  m.def(
      "run_busy",
      [](double ms, int device, unsigned long long max_iters) {
        payload::BusyResult r;
        {
          py::gil_scoped_release rel;
          r = payload::run_busy(ms, device, max_iters);
        }
        py::dict d;
        d["elapsed_ms"] = r.elapsed_ms;
        d["iters"] = r.iters;
        d["guard_hit"] = r.guard_hit;
        return d;
      },
      py::arg("ms") = 100.0, py::arg("device") = 0, py::arg("max_iters") = 0,
      "occupy the device with a bounded spin for ~ms (sleep-pod payload), ms "
      "finite and in 0 .. 60000; max_iters bounds the spin's trips (0: the "
      "built-in bound); returns the device-side elapsed_ms and iters of block "
      "0's first lane and whether the iteration guard ended its spin");

  m.def("grid_for", &payload::grid_for, py::arg("n4"),
        "the default grid for n4 float4s: ceil(n4 / 256) in 1 .. 65535; host only, "
        "no GPU");

  m.def(
      "run_xcd_census",
      [](int device, int blocks) {
        py::gil_scoped_release rel;
        return payload::run_xcd_census(device, blocks);
      },
      py::arg("device") = 0, py::arg("blocks") = 4096,
      "per-XCD workgroup counts: exactly one nonzero in a CPX partition");

  m.def(
      "device_info",
      [](int device) {
        payload::DeviceInfo info;
        {
          py::gil_scoped_release rel;
          info = payload::get_device_info(device);
        }
        py::dict d;
        d["device"] = info.device;
        d["name"] = info.name;
        d["gcn_arch"] = info.gcn_arch;
        d["cu_count"] = info.cu_count;
        d["total_mem_gb"] = info.total_mem_gb;
        d["xcd_count_visible"] = info.xcd_count_visible;
        return d;
      },
      py::arg("device") = 0);

  m.def(
      "vecadd",
      [](f32_array a, f32_array b, int device, int blocks) {
        if (a.ndim() != 1 || b.ndim() != 1)
          throw py::value_error("vecadd: a and b must be 1-D");
        if (a.shape(0) != b.shape(0))
          throw py::value_error("vecadd: a and b differ in length");
        if (a.shape(0) < 1) throw py::value_error("vecadd: empty operand");
        const size_t n = static_cast<size_t>(a.shape(0));
        py::array_t<float> c(static_cast<py::ssize_t>(n));
        const float* pa = a.data();
        const float* pb = b.data();
        float* pc = c.mutable_data();
        size_t guard_changed;
        {
          py::gil_scoped_release rel;
          guard_changed = payload::vecadd(pa, pb, pc, n, device, blocks);
        }
        return py::make_tuple(c, guard_changed);
      },
      py::arg("a"), py::arg("b"), py::arg("device") = 0, py::arg("blocks") = 0,
      "(c, guard_changed): c float32 (n,) = a + b on the vecadd kernel, a and b "
      "1-D float32 of equal length n >= 1, zero-padded to whole float4s; blocks=0 "
      "is the default grid, blocks > 0 forces that grid; guard_changed counts the "
      "bytes the kernel changed in the 4 KiB guards around the destination "
      "(expect 0)");

  m.def(
      "stream_copy",
      [](u32_array x, bool nontemporal, int device, int blocks) {
        if (x.ndim() != 1) throw py::value_error("stream_copy: x must be 1-D");
        if (x.shape(0) < 1) throw py::value_error("stream_copy: empty operand");
        const size_t n = static_cast<size_t>(x.shape(0));
        py::array_t<uint32_t> y(static_cast<py::ssize_t>(n));
        const uint32_t* px = x.data();
        uint32_t* py_ = y.mutable_data();
        size_t guard_changed;
        {
          py::gil_scoped_release rel;
          guard_changed = payload::stream_copy(px, py_, n, nontemporal, device, blocks);
        }
        return py::make_tuple(y, guard_changed);
      },
      py::arg("x"), py::arg("nontemporal") = false, py::arg("device") = 0,
      py::arg("blocks") = 0,
      "(y, guard_changed): y uint32 (n,) = x through the streaming-copy kernel of "
      "the bandwidth probe, or its nontemporal variant; x 1-D uint32 of length n "
      ">= 1 (words, so that every bit pattern survives the binding); blocks and "
      "guard_changed as in vecadd");

  m.def(
      "to_bf16",
      [](f32_array x) { return map_elements(x, payload::to_bf16_rne); },
      py::arg("x"),
      "float32 -> bf16 bits (uint16), round-to-nearest-even; host only, no GPU");

  m.def(
      "gemm_bf16",
      [](f32_array a, f32_array b, int device) {
        return gemm_f32("gemm_bf16", payload::gemm_bf16, a, b, device);
      },
      py::arg("a"), py::arg("b"), py::arg("device") = 0,
      "C (M,N) float32 = bf16(a (M,K)) @ bf16(b (K,N)) on the MFMA kernel");

  m.def(
      "run_gemm_check",
      [](int mm, int n, int k, int device) {
        py::gil_scoped_release rel;
        return payload::run_gemm_check(mm, n, k, device);
      },
      py::arg("m"), py::arg("n"), py::arg("k"), py::arg("device") = 0,
      "integer-pattern GEMM vs host int64 reference; returns max abs error "
      "(expect 0); K <= 1024");

  m.def(
      "run_gemm",
      [](int mm, int n, int k, int iters, int device) {
        return run_timed_gemm(payload::run_gemm, mm, n, k, iters, device);
      },
      py::arg("m") = 4096, py::arg("n") = 4096, py::arg("k") = 1024,
      py::arg("iters") = 10, py::arg("device") = 0,
      "timed bf16 MFMA GEMM, 256 outputs spot-checked exactly; K <= 1024");

  m.def(
      "to_e4m3",
      [](f32_array x) { return map_elements(x, payload::to_e4m3_sat); },
      py::arg("x"),
      "float32 -> OCP e4m3fn byte (uint8), round-to-nearest-even, saturating at "
      "+-448; host only, no GPU");

  m.def(
      "from_e4m3",
      [](u8_array codes) { return map_elements(codes, payload::from_e4m3); },
      py::arg("codes"), "OCP e4m3fn byte (uint8) -> float32; host only, no GPU");

  m.def(
      "mx_quantize",
      [](f32_array x) {
        const int K = last_axis("mx_quantize", "x", x);
        return quantize_rows(x, K, payload::mx_quantize_row);
      },
      py::arg("x"),
      "OCP MX quantization along the last axis: (codes uint8 [..., K], scales "
      "uint8 [..., ceil(K/32)]), e4m3 elements and E8M0 scales; host only, no GPU");

  m.def(
      "gemm_mxfp8",
      [](f32_array a, f32_array b, int device) {
        return gemm_f32("gemm_mxfp8", payload::gemm_mxfp8, a, b, device);
      },
      py::arg("a"), py::arg("b"), py::arg("device") = 0,
      "C (M,N) float32 = mx(a (M,K)) @ mx(b (K,N)): rows of a and columns of b "
      "MX-quantized to e4m3 with E8M0 block scales, on the block-scaled MFMA "
      "kernel; ValueError on a non-finite input");

  m.def(
      "gemm_mxfp8_raw",
      [](u8_array a_codes, u8_array a_scales, u8_array b_codes, u8_array b_scales,
         int device) {
        return gemm_raw("gemm_mxfp8_raw", payload::gemm_mxfp8_raw, any_code, a_codes,
                        a_scales, b_codes, b_scales, device);
      },
      py::arg("a_codes"), py::arg("a_scales"), py::arg("b_codes"),
      py::arg("b_scales"), py::arg("device") = 0,
      "C (M,N) float32 from already quantized operands: e4m3 codes (M,K) and "
      "(K,N), E8M0 scales (M,ceil(K/32)) and (ceil(K/32),N), all uint8");

  m.def(
      "run_mxgemm_check",
      [](int mm, int n, int k, int device) {
        py::gil_scoped_release rel;
        return payload::run_mxgemm_check(mm, n, k, device);
      },
      py::arg("m"), py::arg("n"), py::arg("k"), py::arg("device") = 0,
      "scaled integer-pattern MXFP8 GEMM vs host int64 reference; returns max "
      "abs error (expect 0); K <= 2048");

  m.def(
      "run_mxgemm",
      [](int mm, int n, int k, int iters, int device) {
        return run_timed_gemm(payload::run_mxgemm, mm, n, k, iters, device);
      },
      py::arg("m") = 4096, py::arg("n") = 4096, py::arg("k") = 2048,
      py::arg("iters") = 10, py::arg("device") = 0,
      "timed MXFP8 block-scaled MFMA GEMM, 256 outputs spot-checked exactly; "
      "K <= 2048");

  // ---- MXFP4 ---------------------------------------------------------------

  m.def(
      "to_e2m1",
      [](f32_array x) {
        no_nan("to_e2m1", x);
        return map_elements(x, payload::to_e2m1_sat);
      },
      py::arg("x"),
      "float32 -> OCP e2m1 code (uint8, 0..15, bit 3 the sign), nearest value "
      "with ties to the even code, saturating at +-6; ValueError on NaN; host "
      "only, no GPU");

  m.def(
      "from_e2m1",
      [](u8_array codes) {
        e2m1_codes("from_e2m1", codes);
        return map_elements(codes, payload::from_e2m1);
      },
      py::arg("codes"),
      "OCP e2m1 code (uint8, 0..15) -> float32; ValueError on a code above 15; "
      "host only, no GPU");

  m.def(
      "mx4_quantize",
      [](f32_array x) {
        const int K = last_axis("mx4_quantize", "x", x);
        no_nan("mx4_quantize", x);
        return quantize_rows(x, K, payload::mx4_quantize_row);
      },
      py::arg("x"),
      "OCP MX quantization to e2m1 along the last axis: (codes uint8 [..., K], one "
      "code 0..15 per byte, scales uint8 [..., ceil(K/32)]); ValueError on NaN; "
      "host only, no GPU");

  m.def(
      "pack_fp4",
      [](u8_array codes) {
        const int K = last_axis("pack_fp4", "codes", codes);
        e2m1_codes("pack_fp4", codes);
        return std::get<0>(map_rows(codes, K, payload::pack_fp4, py::ssize_t{(K + 1) / 2}));
      },
      py::arg("codes"),
      "the device byte image of e2m1 codes along the last axis: uint8 [..., "
      "ceil(K/2)], even k in bits 3:0 and odd k in bits 7:4, an odd tail padded "
      "with code 0; ValueError on a code above 15; host only, no GPU");

  m.def(
      "gemm_mxfp4",
      [](f32_array a, f32_array b, int device) {
        return gemm_f32("gemm_mxfp4", payload::gemm_mxfp4, a, b, device);
      },
      py::arg("a"), py::arg("b"), py::arg("device") = 0,
      "C (M,N) float32 = mx4(a (M,K)) @ mx4(b (K,N)): rows of a and columns of b "
      "MX-quantized to e2m1 with E8M0 block scales, on the block-scaled MFMA "
      "kernel; ValueError on a non-finite input");

  m.def(
      "gemm_mxfp4_raw",
      [](u8_array a_codes, u8_array a_scales, u8_array b_codes, u8_array b_scales,
         int device) {
        return gemm_raw("gemm_mxfp4_raw", payload::gemm_mxfp4_raw, e2m1_codes, a_codes,
                        a_scales, b_codes, b_scales, device);
      },
      py::arg("a_codes"), py::arg("a_scales"), py::arg("b_codes"),
      py::arg("b_scales"), py::arg("device") = 0,
      "C (M,N) float32 from already quantized operands: e2m1 codes (M,K) and "
      "(K,N), one code 0..15 per byte, E8M0 scales (M,ceil(K/32)) and "
      "(ceil(K/32),N), all uint8; ValueError on a code above 15");

  m.def(
      "run_mx4gemm_check",
      [](int mm, int n, int k, int device) {
        py::gil_scoped_release rel;
        return payload::run_mx4gemm_check(mm, n, k, device);
      },
      py::arg("m"), py::arg("n"), py::arg("k"), py::arg("device") = 0,
      "scaled integer-pattern MXFP4 GEMM vs host int64 reference; returns max "
      "abs error (expect 0); K <= 2048");

  m.def(
      "run_mx4gemm",
      [](int mm, int n, int k, int iters, int device) {
        return run_timed_gemm(payload::run_mx4gemm, mm, n, k, iters, device);
      },
      py::arg("m") = 4096, py::arg("n") = 4096, py::arg("k") = 2048,
      py::arg("iters") = 10, py::arg("device") = 0,
      "timed MXFP4 block-scaled MFMA GEMM, 256 outputs spot-checked exactly; "
      "K <= 2048");

  m.def(
      "memcheck_pattern",
      [](uint64_t first_word, size_t n_words, uint64_t seed) {
        py::array_t<uint64_t> out(static_cast<py::ssize_t>(n_words));
        payload::memcheck_pattern(out.mutable_data(), first_word, n_words, seed);
        return out;
      },
      py::arg("first_word"), py::arg("n_words"), py::arg("seed") = 0,
      "the memcheck pattern's 64-bit words first_word .. first_word+n_words-1 "
      "(uint64); host only, no GPU");

  m.def(
      "memcheck_fill",
      [](size_t bytes, uint64_t seed, uint64_t base_unit, bool invert, int device,
         int blocks) {
        if (bytes < payload::kMemcheckUnit)
          throw py::value_error("memcheck_fill: bytes must be >= 16");
        py::array_t<uint64_t> out(
            static_cast<py::ssize_t>(bytes / payload::kMemcheckUnit * 2));
        uint64_t* dst = out.mutable_data();
        {
          py::gil_scoped_release rel;
          payload::memcheck_fill(dst, bytes, seed, base_unit, invert, device, blocks);
        }
        return out;
      },
      py::arg("bytes"), py::arg("seed") = 0, py::arg("base_unit") = 0,
      py::arg("invert") = false, py::arg("device") = 0, py::arg("blocks") = 0,
      "run the memcheck fill kernel alone on a fresh buffer and return its "
      "bytes // 16 * 2 words (uint64); base_unit is the pattern index of unit 0");

  m.def(
      "run_memcheck",
      [](size_t bytes, int passes, int device, int blocks, int64_t flip_offset,
         uint64_t flip_mask) {
        payload::MemcheckResult r;
        {
          py::gil_scoped_release rel;
          r = payload::run_memcheck(bytes, passes, device, blocks, flip_offset,
                                    flip_mask);
        }
        py::dict d;
        d["bytes"] = r.bytes;
        d["passes"] = r.passes;
        d["bad_words"] = r.bad_words;
        d["first_bad_offset"] = r.first_bad_offset;
        d["bad_bits"] = py::int_(r.bad_bits);
        d["fill_gb_s"] = r.fill_gb_s;
        d["check_gb_s"] = r.check_gb_s;
        d["ms"] = r.ms;
        return d;
      },
      py::arg("bytes") = (size_t{1} << 30), py::arg("passes") = 1,
      py::arg("device") = 0, py::arg("blocks") = 0, py::arg("flip_offset") = -1,
      py::arg("flip_mask") = 0,
      "moving-inversions memory test of one buffer: fill, check + invert, "
      "check, per pass; flip_offset / flip_mask corrupt one word once (self-test). "
      "Buffers of 256 MiB or less can be served from the Infinity Cache");

  // ---- decode attention ----------------------------------------------------

  // lengths: None, or B integers in 1 .. L; ValueError otherwise
  auto attn_lengths = [](const char* who, const py::object& lengths, py::ssize_t B,
                         py::ssize_t L) {
    std::vector<int> lens;
    if (lengths.is_none()) return lens;
    std::string w(who);
    py::array_t<int64_t, py::array::c_style | py::array::forcecast> arr;
    try {
      arr = py::array_t<int64_t, py::array::c_style | py::array::forcecast>::ensure(
          lengths);
    } catch (const py::error_already_set&) {
      arr = py::array_t<int64_t, py::array::c_style | py::array::forcecast>();
    }
    if (!arr) {
      PyErr_Clear();
      throw py::value_error(w + ": lengths must be integers");
    }
    if (arr.ndim() != 1 || arr.shape(0) != B)
      throw py::value_error(w + ": lengths must have shape (B,)");
    for (py::ssize_t b = 0; b < B; ++b) {
      int64_t v = arr.data()[b];
      if (v < 1 || v > L) throw py::value_error(w + ": lengths must be in 1 .. L");
      lens.push_back(static_cast<int>(v));
    }
    return lens;
  };

  // A shape's limits are the headers': attn_decode_shape and attn_prefill_shape
  // throw std::invalid_argument, which pybind11 raises as ValueError. Every
  // entry calls its check first, before it allocates or releases the GIL.

  m.def(
      "attn_decode",
      [attn_lengths](f32_array q, f32_array k, f32_array v, py::object lengths,
                     py::object scale, int splits, int device) {
        const char* who = "attn_decode";
        attn_operands(who, q, 3, "(B,Hq,128)", k, v);
        const py::ssize_t B = q.shape(0), Hq = q.shape(1), Hkv = k.shape(1),
                          L = k.shape(2);
        payload::attn_decode_shape(B, Hq, Hkv, L, splits);
        std::vector<int> lens = attn_lengths(who, lengths, B, L);
        const float sc = attn_scale(who, scale);
        attn_finite(who, q, k, v);
        const float* pq = q.data();
        const float* pk = k.data();
        const float* pv = v.data();
        py::array_t<float> o({B, Hq, static_cast<py::ssize_t>(payload::kAttnD)});
        float* po = o.mutable_data();
        {
          py::gil_scoped_release rel;
          payload::attn_decode(pq, pk, pv, lens.empty() ? nullptr : lens.data(), po,
                               static_cast<int>(B), static_cast<int>(Hq),
                               static_cast<int>(Hkv), static_cast<int>(L), sc, splits,
                               device);
        }
        return o;
      },
      py::arg("q"), py::arg("k"), py::arg("v"), py::arg("lengths") = py::none(),
      py::arg("scale") = py::none(), py::arg("splits") = 0, py::arg("device") = 0,
      "o (B,Hq,128) float32 = softmax(scale q.k) v over the first lengths[b] keys: "
      "single-token grouped-query attention over a KV cache, q (B,Hq,128), k and "
      "v (B,Hkv,L,128) rounded to bf16, on the MFMA split-KV kernel; scale=None "
      "is 1/sqrt(128), splits=0 is auto; ValueError on an unsupported shape, "
      "length, split count or a non-finite input");

  m.def(
      "attn_check_pattern",
      [attn_lengths](int batch, int hq, int hkv, int length, py::object lengths) {
        payload::attn_decode_shape(batch, hq, hkv, length);
        std::vector<int> lens = attn_lengths("attn_check_pattern", lengths, batch, length);
        return attn_pattern_arrays(
            {batch, hq, payload::kAttnD}, batch, hkv, length,
            [&](float* q, float* k, float* v, float* e) {
              payload::attn_check_pattern(q, k, v, e, batch, hq, hkv, length,
                                          lens.empty() ? nullptr : lens.data());
            });
      },
      py::arg("batch"), py::arg("hq"), py::arg("hkv"), py::arg("length"),
      py::arg("lengths") = py::none(),
      "(q, k, v, expected) of the exact selection pattern: small integers, K zero "
      "at min(32, largest power of two <= len) selected keys per (sequence, kv "
      "head) and <= -16 elsewhere, expected = mean of v over the selected keys; "
      "host only, no GPU");

  m.def(
      "run_attn_check",
      [](int batch, int hq, int hkv, int length, int splits, int device) {
        payload::attn_decode_shape(batch, hq, hkv, length, splits);
        payload::AttnCheck r;
        {
          py::gil_scoped_release rel;
          r = payload::run_attn_check(batch, hq, hkv, length, splits, device);
        }
        return attn_check_dict(r);
      },
      py::arg("batch"), py::arg("hq"), py::arg("hkv"), py::arg("length"),
      py::arg("splits") = 0, py::arg("device") = 0,
      "decode attention self-check at full lengths: max_err of the selection "
      "pattern (expect exactly 0) and max_rel = max |o - fp64 ref| / max |v| of a "
      "dense pattern (expect <= 2^-8)");

  m.def(
      "run_attn",
      [](int batch, int hq, int hkv, int length, int iters, int device) {
        payload::attn_decode_shape(batch, hq, hkv, length);
        payload::AttnResult r;
        {
          py::gil_scoped_release rel;
          r = payload::run_attn(batch, hq, hkv, length, iters, device);
        }
        py::dict d = attn_timed_dict(batch, hq, hkv, length, iters);
        d["kv_gb_per_s"] = r.kv_gb_s;
        d["steps_per_s"] = r.steps_per_s;
        d["tok_per_s"] = r.tok_per_s;
        d["max_err"] = r.max_err;
        return d;
      },
      py::arg("batch") = 32, py::arg("hq") = 64, py::arg("hkv") = 8,
      py::arg("length") = 4096, py::arg("iters") = 10, py::arg("device") = 0,
      "timed decode attention on the selection pattern (device-filled cache, "
      "512 MiB of K and V at the default shape), 16 output rows checked exactly");

  // ---- prefill attention -----------------------------------------------------

  m.attr("PREFILL_ROWS") = payload::kPrefillRows;
  m.attr("PREFILL_KEYS") = payload::kPrefillKeys;

  m.def(
      "attn_prefill",
      [](f32_array q, f32_array k, f32_array v, bool causal, py::object scale,
         int device) {
        const char* who = "attn_prefill";
        attn_operands(who, q, 4, "(B,Hq,L,128)", k, v);
        if (k.shape(2) != q.shape(2))
          throw py::value_error("attn_prefill: q and k differ in length");
        const py::ssize_t B = q.shape(0), Hq = q.shape(1), Hkv = k.shape(1),
                          L = q.shape(2);
        payload::attn_prefill_shape(B, Hq, Hkv, L);
        const float sc = attn_scale(who, scale);
        attn_finite(who, q, k, v);
        const float* pq = q.data();
        const float* pk = k.data();
        const float* pv = v.data();
        py::array_t<float> o({B, Hq, L, static_cast<py::ssize_t>(payload::kAttnD)});
        float* po = o.mutable_data();
        {
          py::gil_scoped_release rel;
          payload::attn_prefill(pq, pk, pv, po, static_cast<int>(B),
                                static_cast<int>(Hq), static_cast<int>(Hkv),
                                static_cast<int>(L), causal, sc, device);
        }
        return o;
      },
      py::arg("q"), py::arg("k"), py::arg("v"), py::arg("causal") = true,
      py::arg("scale") = py::none(), py::arg("device") = 0,
      "o (B,Hq,L,128) float32 = softmax(scale q.k) v over the keys t <= i (causal) "
      "or all L keys: grouped-query self-attention over a whole prompt, q "
      "(B,Hq,L,128), k and v (B,Hkv,L,128) rounded to bf16, on the MFMA flash "
      "kernel with K and V tiles staged through LDS; scale=None is 1/sqrt(128); "
      "ValueError on an unsupported shape or a non-finite input or scale");

  m.def(
      "prefill_check_pattern",
      [](int batch, int hq, int hkv, int length, bool causal) {
        payload::attn_prefill_shape(batch, hq, hkv, length);
        return attn_pattern_arrays(
            {batch, hq, length, payload::kAttnD}, batch, hkv, length,
            [&](float* q, float* k, float* v, float* e) {
              payload::prefill_check_pattern(q, k, v, e, batch, hq, hkv, length, causal);
            });
      },
      py::arg("batch"), py::arg("hq"), py::arg("hkv"), py::arg("length"),
      py::arg("causal") = true,
      "(q, k, v, expected) of the exact selection pattern: small integers, K zero "
      "at the selected keys of a (sequence, kv head) (key 0 and every t with (t + "
      "b + 2 g) % 5 == 0) and <= -16 elsewhere, expected = mean of v over the "
      "selected keys a row sees; host only, no GPU");

  m.def(
      "run_prefill_check",
      [](int batch, int hq, int hkv, int length, bool causal, int device) {
        payload::attn_prefill_shape(batch, hq, hkv, length);
        payload::AttnCheck r;
        {
          py::gil_scoped_release rel;
          r = payload::run_prefill_check(batch, hq, hkv, length, causal, device);
        }
        return attn_check_dict(r);
      },
      py::arg("batch"), py::arg("hq"), py::arg("hkv"), py::arg("length"),
      py::arg("causal") = true, py::arg("device") = 0,
      "prefill attention self-check: max_err of the selection pattern (expect "
      "exactly 0) and max_rel = max |o - fp64 ref| / max |v| of a dense pattern "
      "(expect <= 2^-8)");

  m.def(
      "run_prefill",
      [](int batch, int hq, int hkv, int length, int iters, bool causal, int device,
         int pattern) {
        payload::attn_prefill_shape(batch, hq, hkv, length);
        payload::PrefillResult r;
        {
          py::gil_scoped_release rel;
          r = payload::run_prefill(batch, hq, hkv, length, iters, causal, device,
                                   pattern);
        }
        py::dict d = attn_timed_dict(batch, hq, hkv, length, iters);
        d["causal"] = causal;
        d["tflops"] = r.tflops;
        d["tok_per_s"] = r.tok_per_s;
        d["max_rel"] = r.max_rel;
        return d;
      },
      py::arg("batch") = 8, py::arg("hq") = 64, py::arg("hkv") = 8,
      py::arg("length") = 4096, py::arg("iters") = 10, py::arg("causal") = true,
      py::arg("device") = 0, py::arg("pattern") = 0,
      "timed prefill attention on the dense hash pattern (device-filled; pattern=1 "
      "times the low-entropy selection pattern instead), TFLOP/s over the unmasked "
      "pairs only, 16 spread output rows checked against fp64");
}
