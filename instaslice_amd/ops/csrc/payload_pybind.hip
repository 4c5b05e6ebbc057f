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
using f64_array = c_array<double>;
using u32_array = c_array<uint32_t>;
using u8_array = c_array<uint8_t>;
using i8_array = c_array<int8_t>;

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

// C (M,N) of one of the general GEMM entries on operands of element type T
// (float, or double for gemm_f64)
template <class T>
using GemmEntry = void (*)(const T*, const T*, T*, int, int, int, int);
template <class T>
py::array_t<T> gemm_dense(const char* who, GemmEntry<T> entry, const c_array<T>& a,
                          const c_array<T>& b, int device) {
  auto [M, N, K] = gemm_dims(who, a, b);
  py::array_t<T> c({static_cast<py::ssize_t>(M), static_cast<py::ssize_t>(N)});
  const T* pa = a.data();
  const T* pb = b.data();
  T* pc = c.mutable_data();
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

// an int8 operand of the INT8 GEMM entries as a contiguous array. Another
// integer dtype is not cast: a value outside int8 would wrap silently, so it
// is a TypeError
i8_array int8_operand(const char* who, const char* what, const py::object& x) {
  if (!py::isinstance<py::array>(x) ||
      !py::reinterpret_borrow<py::array>(x).dtype().is(py::dtype::of<int8_t>()))
    throw py::type_error(std::string(who) + ": " + what + " must be an int8 array");
  return i8_array::ensure(x);
}

// a pool of e4m3 codes of the fp8 attention entry: uint8 and nothing else, for
// the same reason
u8_array uint8_operand(const char* who, const char* what, const py::object& x) {
  if (!py::isinstance<py::array>(x) ||
      !py::reinterpret_borrow<py::array>(x).dtype().is(py::dtype::of<uint8_t>()))
    throw py::type_error(std::string(who) + ": " + what + " must be a uint8 array");
  return u8_array::ensure(x);
}

// (M, N, K) of the INT8 GEMM entries: gemm_dims plus the K limit
std::array<int, 3> igemm_dims(const char* who, const i8_array& a, const i8_array& b) {
  auto dims = gemm_dims(who, a, b);
  if (dims[2] > payload::kIgemmMaxK)
    throw py::value_error(std::string(who) + ": K must be <= 131071");
  return dims;
}

// a W8A8 scale vector: `n` floats
void scale_vector(const char* who, const char* what, const f32_array& s, int n) {
  if (s.ndim() != 1 || s.shape(0) != n)
    throw py::value_error(std::string(who) + ": " + what + " has the wrong length");
}

// the (T, topk) ids of the routed entries as ints. A floating array is a
// TypeError, not a cast: a cast would hide a wrong value. An id beyond int is
// passed on as -1, which the host layer refuses like any id outside [0, E)
std::vector<int> moe_ids(const char* who, const py::object& ids_) {
  std::string w(who);
  if (!py::isinstance<py::array>(ids_))
    throw py::type_error(w + ": ids must be an integer array");
  const char kind = py::reinterpret_borrow<py::array>(ids_).dtype().kind();
  if (kind != 'i' && kind != 'u')
    throw py::type_error(w + ": ids must be an integer array");
  auto ids = c_array<int64_t>::ensure(ids_);
  if (!ids) throw py::type_error(w + ": ids must be an integer array");
  if (ids.ndim() != 2 || ids.shape(0) < 1 || ids.shape(1) < 1 ||
      ids.shape(0) > INT32_MAX || ids.shape(1) > payload::kMoeMaxTopk)
    throw py::value_error(w + ": ids must be (T, topk), T >= 1 and 1 <= topk <= 8");
  std::vector<int> out(ids.size());
  const int64_t* src = ids.data();
  for (size_t i = 0; i < out.size(); ++i)
    out[i] = src[i] < 0 || src[i] > INT32_MAX ? -1 : static_cast<int>(src[i]);
  return out;
}

// an integer argument of the paged attention entries (the table, the lengths)
// as int64 of rank `rank`. Anything floating is a TypeError, not a cast.
c_array<int64_t> paged_ints(const char* who, const char* what, const py::object& x,
                            int rank) {
  const std::string w = std::string(who) + ": " + what;
  py::array any = py::array::ensure(x);
  if (!any) {
    PyErr_Clear();
    throw py::type_error(w + " must be an integer array");
  }
  const char kind = any.dtype().kind();
  if (kind != 'i' && kind != 'u') throw py::type_error(w + " must be an integer array");
  auto arr = c_array<int64_t>::ensure(any);
  if (!arr) throw py::type_error(w + " must be an integer array");
  if (arr.ndim() != rank) throw py::value_error(w + " has the wrong rank");
  return arr;
}

// narrowed to int; what does not fit becomes -1, which no check admits
std::vector<int> paged_narrow(const c_array<int64_t>& x) {
  std::vector<int> out(static_cast<size_t>(x.size()));
  const int64_t* src = x.data();
  for (size_t i = 0; i < out.size(); ++i)
    out[i] = src[i] < 0 || src[i] > INT32_MAX ? -1 : static_cast<int>(src[i]);
  return out;
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

// the report of one of the timed paged runs; r8: what the fp8 one adds
py::dict paged_timed_dict(int batch, int hq, int hkv, int length, int iters, int page,
                          bool ragged, const payload::AttnPagedResult& r,
                          const payload::AttnPaged8Result* r8 = nullptr) {
  py::dict d = attn_timed_dict(batch, hq, hkv, length, iters);
  d["page"] = page;
  d["ragged"] = ragged;
  d["items"] = r.items;
  if (r8) {
    d["us"] = r8->us;
    d["bf16_us"] = r8->bf16_us;
  }
  d["kv_gb_per_s"] = r.kv_gb_s;
  d["steps_per_s"] = r.steps_per_s;
  d["tok_per_s"] = r.tok_per_s;
  if (r8) d["quant_rel"] = r8->quant_rel;
  d["max_err"] = r.max_err;
  return d;
}

// The operands of the two paged entries: q (B,Hq,128), the two pools
// (P,Hkv,page,128) and alike (`pools` names them in the messages), table (B,W)
// and lens (B,) integer, narrowed. TypeError or ValueError, in the order the
// entries always raised them; the shape limits are the caller's and come after.
// Narrowing here, ahead of them, raises nothing (paged_narrow cannot): it only
// copies a table once that the limits may then reject.
struct PagedOperands {
  py::ssize_t B, Hq, Hkv, page, W, P;
  std::vector<int> tab, lens;
};
template <class Pool>
PagedOperands paged_operands(const char* who, const char* pools, const f32_array& q,
                             const Pool& k, const Pool& v, const py::object& table_,
                             const py::object& lens_) {
  const std::string w(who), kv(pools);
  auto table = paged_ints(who, "table", table_, 2);
  auto lens_arr = paged_ints(who, "lens", lens_, 1);
  if (q.ndim() != 3) throw py::value_error(w + ": q must be (B,Hq,128)");
  if (k.ndim() != 4 || v.ndim() != 4)
    throw py::value_error(w + ": " + kv + " must be (P,Hkv,page,128)");
  if (q.shape(2) != payload::kAttnD || k.shape(3) != payload::kAttnD)
    throw py::value_error(w + ": head dim must be 128");
  for (int i = 0; i < 4; ++i)
    if (k.shape(i) != v.shape(i)) throw py::value_error(w + ": " + kv + " differ in shape");
  if (table.shape(0) != q.shape(0) || lens_arr.shape(0) != q.shape(0))
    throw py::value_error(w + ": table must be (B,W) and lens (B,)");
  return {q.shape(0), q.shape(1), k.shape(1), k.shape(2), table.shape(1), k.shape(0),
          paged_narrow(table), paged_narrow(lens_arr)};
}

}  // namespace

PYBIND11_MODULE(_payload, m) {
  m.doc() = "gfx950 HIP payload kernels (vecadd / membw / busy / xcd census / gemm / "
            "dgemm / igemm / mxgemm / mx4gemm / moe / memcheck / attn / paged / paged8 / "
            "prefill / extend)";

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
        return gemm_dense<float>("gemm_bf16", payload::gemm_bf16, a, b, device);
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
      "gemm_f64",
      [](f64_array a, f64_array b, int device) {
        return gemm_dense<double>("gemm_f64", payload::gemm_f64, a, b, device);
      },
      py::arg("a"), py::arg("b"), py::arg("device") = 0,
      "C (M,N) float64 = a (M,K) @ b (K,N) with fp64 operands and accumulation on "
      "the FP64 MFMA kernel; ValueError on a non-finite input");

  m.def(
      "run_dgemm_check",
      [](int mm, int n, int k, int device) {
        py::gil_scoped_release rel;
        return payload::run_dgemm_check(mm, n, k, device);
      },
      py::arg("m"), py::arg("n"), py::arg("k"), py::arg("device") = 0,
      "FP64 GEMM on an integer pattern scaled by 2^-16 (46-bit results at K = "
      "1024) vs host int64 reference; returns max abs error (expect 0); "
      "K <= 65536");

  m.def(
      "run_dgemm",
      [](int mm, int n, int k, int iters, int device) {
        return run_timed_gemm(payload::run_dgemm, mm, n, k, iters, device);
      },
      py::arg("m") = 4096, py::arg("n") = 4096, py::arg("k") = 1024,
      py::arg("iters") = 10, py::arg("device") = 0,
      "timed FP64 MFMA GEMM, 256 outputs spot-checked exactly; K <= 65536");

  // ---- INT8 -----------------------------------------------------------------

  m.def(
      "gemm_i8",
      [](py::object a_, py::object b_, int device) {
        const char* who = "gemm_i8";
        i8_array a = int8_operand(who, "a", a_), b = int8_operand(who, "b", b_);
        auto [M, N, K] = igemm_dims(who, a, b);
        py::array_t<int32_t> c({static_cast<py::ssize_t>(M), static_cast<py::ssize_t>(N)});
        const int8_t* pa = a.data();
        const int8_t* pb = b.data();
        int32_t* pc = c.mutable_data();
        {
          py::gil_scoped_release rel;
          payload::gemm_i8(pa, pb, pc, M, N, K, device);
        }
        return c;
      },
      py::arg("a"), py::arg("b"), py::arg("device") = 0,
      "C (M,N) int32 = a (M,K) @ b (K,N), int8 operands and int32 accumulation on "
      "the INT8 MFMA kernel; TypeError unless both are int8 arrays, ValueError on "
      "K > 131071 (beyond it an int32 sum could wrap)");

  m.def(
      "gemm_w8a8",
      [](py::object a_, py::object b_, f32_array sa, f32_array sb, int device) {
        const char* who = "gemm_w8a8";
        i8_array a = int8_operand(who, "a", a_), b = int8_operand(who, "b", b_);
        auto [M, N, K] = igemm_dims(who, a, b);
        scale_vector(who, "sa", sa, M);
        scale_vector(who, "sb", sb, N);
        py::array_t<float> c({static_cast<py::ssize_t>(M), static_cast<py::ssize_t>(N)});
        const int8_t* pa = a.data();
        const int8_t* pb = b.data();
        const float* psa = sa.data();
        const float* psb = sb.data();
        float* pc = c.mutable_data();
        {
          py::gil_scoped_release rel;
          payload::gemm_w8a8(pa, pb, psa, psb, pc, M, N, K, device);
        }
        return c;
      },
      py::arg("a"), py::arg("b"), py::arg("sa"), py::arg("sb"), py::arg("device") = 0,
      "C (M,N) float32 = (float32(a (M,K) @ b (K,N)) * sa[:, None]) * sb[None, :]: "
      "the int32 product of int8 operands scaled per row (sa, M floats) and per "
      "column (sb, N floats) in the kernel's epilogue, in fp32 and in that order; "
      "TypeError unless a and b are int8 arrays, ValueError on K > 131071, a scale "
      "vector of the wrong length or a non-finite scale");

  m.def(
      "quantize_i8",
      [](f32_array x) {
        const int K = last_axis("quantize_i8", "x", x);
        std::vector<py::ssize_t> shape(x.shape(), x.shape() + x.ndim());
        py::array_t<int8_t> codes(shape);
        shape.pop_back();
        py::array_t<float> scales(shape);
        const float* src = x.data();
        int8_t* pc = codes.mutable_data();
        float* ps = scales.mutable_data();
        for (py::ssize_t r = 0, rows = x.size() / K; r < rows; ++r)
          payload::quantize_i8_row(src + r * K, K, pc + r * K, ps + r);
        return py::make_tuple(codes, scales);
      },
      py::arg("x"),
      "symmetric int8 quantization along the last axis: (codes int8 [..., K], "
      "scales float32 [...]), scale = absmax / 127 (1 for an all-zero row), code = "
      "round-to-nearest-even of x / scale in -127 .. 127; ValueError on a "
      "non-finite element; host only, no GPU");

  m.def(
      "run_igemm_check",
      [](int mm, int n, int k, int device) {
        py::gil_scoped_release rel;
        return payload::run_igemm_check(mm, n, k, device);
      },
      py::arg("m"), py::arg("n"), py::arg("k"), py::arg("device") = 0,
      "INT8 GEMM (int32 result) on a pattern over the whole int8 range vs host "
      "int64 reference; returns max abs error (expect 0); K <= 131071");

  m.def(
      "run_igemm",
      [](int mm, int n, int k, int iters, int device) {
        return run_timed_gemm(payload::run_igemm, mm, n, k, iters, device);
      },
      py::arg("m") = 4096, py::arg("n") = 4096, py::arg("k") = 4096,
      py::arg("iters") = 10, py::arg("device") = 0,
      "timed INT8 MFMA GEMM, 256 outputs spot-checked exactly; \"tflops\" is "
      "10^12 integer operations per second (2 M N K per launch); K <= 131071");

  // ---- routed mixture of experts ---------------------------------------------

  m.def(
      "moe_gemm",
      [](f32_array x, f32_array w, py::object ids_, py::object gates_, int bm,
         int device) {
        const std::string who = "moe_gemm";
        if (x.ndim() != 2 || w.ndim() != 3)
          throw py::value_error(who + ": x must be (T,K) and w (E,K,N)");
        std::vector<int> ids = moe_ids("moe_gemm", ids_);
        const py::array_t<int64_t> shape_of = c_array<int64_t>::ensure(ids_);
        const py::ssize_t T = x.shape(0), K = x.shape(1), topk = shape_of.shape(1);
        if (shape_of.shape(0) != T)
          throw py::value_error(who + ": x is (T,K) and ids is (T,topk): T differs");
        if (w.shape(1) != K)
          throw py::value_error(who + ": x is (T,K) and w is (E,K,N): K differs");
        if (K < 1 || w.shape(0) < 1 || w.shape(2) < 1)
          throw py::value_error(who + ": empty operand");
        if (K > INT32_MAX || w.shape(0) > INT32_MAX || w.shape(2) > INT32_MAX)
          throw py::value_error(who + ": shape too large");
        f32_array gates;
        if (!gates_.is_none()) {
          gates = f32_array::ensure(gates_);
          if (!gates) throw py::type_error(who + ": gates must be a float array or None");
          if (gates.ndim() != 2 || gates.shape(0) != T || gates.shape(1) != topk)
            throw py::value_error(who + ": gates must be (T, topk) like ids");
        }
        const int E = static_cast<int>(w.shape(0)), N = static_cast<int>(w.shape(2));
        py::array_t<float> y({T, static_cast<py::ssize_t>(N)});
        const float* px = x.data();
        const float* pw = w.data();
        const float* pg = gates_.is_none() ? nullptr : gates.data();
        float* py_ = y.mutable_data();
        {
          py::gil_scoped_release rel;
          payload::moe_gemm(px, pw, ids.data(), pg, py_, static_cast<int>(T), N,
                            static_cast<int>(K), E, static_cast<int>(topk), bm, device);
        }
        return y;
      },
      py::arg("x"), py::arg("w"), py::arg("ids"), py::arg("gates") = py::none(),
      py::arg("bm") = 0, py::arg("device") = 0,
      "y (T,N) float32: y[t] = sum_j gates[t,j] * (bf16(x[t]) @ bf16(w[ids[t,j]])), "
      "the routed mixture-of-experts layer on the grouped MFMA GEMM: x (T,K), w "
      "(E,K,N), ids (T,topk) integer with a token's experts all different, gates "
      "(T,topk) or None (all ones); routing on the device, fp32 accumulation, the "
      "gate applied in fp32, the top-k rows added in the order of j; bm 0 (the "
      "host's choice), 32 or 128 picks the tile height; TypeError on floating ids, "
      "ValueError on a bad shape, E > 256, topk > min(E, 8), an id outside [0, E), "
      "a repeated expert, a non-finite element or another bm");

  m.def(
      "moe_route",
      [](py::object ids_, int experts, int device) {
        std::vector<int> ids = moe_ids("moe_route", ids_);
        const py::array_t<int64_t> shape_of = c_array<int64_t>::ensure(ids_);
        const int T = static_cast<int>(shape_of.shape(0));
        const int topk = static_cast<int>(shape_of.shape(1));
        if (experts < 1 || experts > payload::kMoeMaxExperts)
          throw py::value_error("moe_route: experts must be in 1 .. 256");
        py::array_t<int32_t> perm(static_cast<py::ssize_t>(ids.size()));
        py::array_t<int32_t> seg(static_cast<py::ssize_t>(experts) + 1);
        int* pp = perm.mutable_data();
        int* ps = seg.mutable_data();
        {
          py::gil_scoped_release rel;
          payload::moe_route(ids.data(), T, topk, experts, pp, ps, device);
        }
        return py::make_tuple(perm, seg);
      },
      py::arg("ids"), py::arg("experts"), py::arg("device") = 0,
      "the routing kernels alone on ids (T,topk): (perm int32 (T*topk,), the slot "
      "t*topk+j at each row of the expert-sorted order, seg int32 (experts+1,), "
      "the start of each expert's run); the order inside a run is not fixed");

  m.def(
      "run_moe_check",
      [](int tokens, int n, int k, int experts, int topk, int bm, int device) {
        py::gil_scoped_release rel;
        return payload::run_moe_check(tokens, n, k, experts, topk, bm, device);
      },
      py::arg("tokens"), py::arg("n"), py::arg("k"), py::arg("experts"),
      py::arg("topk"), py::arg("bm") = 0, py::arg("device") = 0,
      "routed grouped GEMM on an integer pattern with an empty expert vs host "
      "int64 reference; returns max abs error (expect 0); K <= 1024");

  m.def(
      "run_moe",
      [](int tokens, int n, int k, int experts, int topk, int iters, int bm,
         int device) {
        payload::MoeResult r;
        {
          py::gil_scoped_release rel;
          r = payload::run_moe(tokens, n, k, experts, topk, iters, bm, device);
        }
        py::dict d;
        d["tokens"] = tokens;
        d["n"] = n;
        d["k"] = k;
        d["experts"] = experts;
        d["topk"] = topk;
        d["bm"] = r.bm;
        d["iters"] = iters;
        d["tflops"] = r.tflops;
        d["tokens_per_s"] = r.tokens_per_s;
        d["max_err"] = r.max_err;
        return d;
      },
      py::arg("tokens") = 8192, py::arg("n") = 4096, py::arg("k") = 1024,
      py::arg("experts") = 32, py::arg("topk") = 4, py::arg("iters") = 10,
      py::arg("bm") = 0, py::arg("device") = 0,
      "timed routed grouped GEMM (route, GEMM and combine per launch), 256 outputs "
      "spot-checked exactly; tflops counts 2 T topk N K per launch; K <= 1024");

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
        return gemm_dense<float>("gemm_mxfp8", payload::gemm_mxfp8, a, b, device);
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
        return gemm_dense<float>("gemm_mxfp4", payload::gemm_mxfp4, a, b, device);
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

  // ---- paged decode attention ------------------------------------------------

  m.def(
      "attn_paged_decode",
      [](f32_array q, f32_array k_pages, f32_array v_pages, py::object table_,
         py::object lens_, py::object scale, int workgroups, int device) {
        const char* who = "attn_paged_decode";
        const PagedOperands a =
            paged_operands(who, "k_pages and v_pages", q, k_pages, v_pages, table_, lens_);
        const py::ssize_t B = a.B, Hq = a.Hq, Hkv = a.Hkv, page = a.page, W = a.W, P = a.P;
        payload::attn_paged_shape(B, Hq, Hkv, page, W, P, workgroups);
        const float sc = attn_scale(who, scale);
        const float* pq = q.data();
        const float* pk = k_pages.data();
        const float* pv = v_pages.data();
        py::array_t<float> o({B, Hq, static_cast<py::ssize_t>(payload::kAttnD)});
        float* po = o.mutable_data();
        {
          py::gil_scoped_release rel;
          payload::attn_paged_decode(pq, pk, pv, a.tab.data(), a.lens.data(), po,
                                     static_cast<int>(B), static_cast<int>(Hq),
                                     static_cast<int>(Hkv), static_cast<int>(page),
                                     static_cast<int>(W), static_cast<int>(P), sc,
                                     workgroups, device);
        }
        return o;
      },
      py::arg("q"), py::arg("k_pages"), py::arg("v_pages"), py::arg("table"),
      py::arg("lens"), py::arg("scale") = py::none(), py::arg("workgroups") = 0,
      py::arg("device") = 0,
      "o (B,Hq,128) float32: single-token grouped-query attention over a paged KV "
      "cache. q (B,Hq,128); k_pages and v_pages (P,Hkv,page,128), page 32, 64, 128 "
      "or 256, rounded to bf16; table (B,W) integer names the physical page of each "
      "logical page of a sequence, lens (B,) integer in 1 .. W*page. Only table "
      "entries below ceil(lens[b]/page) are read and must be in 0 .. P-1; only the "
      "chunks below ceil(lens[b]/32) are read and must be finite; a page may serve "
      "several sequences. The split into work items is planned on the device from "
      "lens; workgroups (0 = auto, at most 4096) is the item count it aims at; "
      "scale=None is 1/sqrt(128). TypeError on a floating table or lens, ValueError "
      "on an unsupported shape, length, table entry or a non-finite input, all "
      "before any device work");

  m.def(
      "attn_paged_plan",
      [](py::object lens_, int target, int chunk) {
        auto arr = paged_ints("attn_paged_plan", "lens", lens_, 1);
        if (arr.shape(0) < 1 || arr.shape(0) > 65535)
          throw py::value_error("attn_paged_plan: lens must hold 1 .. 65535 lengths");
        const std::vector<int> lens = paged_narrow(arr);
        const payload::AttnPagedPlan plan = payload::attn_paged_plan(
            lens.data(), static_cast<int>(lens.size()), target, chunk);
        py::array_t<int32_t> items({static_cast<py::ssize_t>(plan.items.size() / 3),
                                    py::ssize_t{3}});
        py::array_t<int32_t> seq({static_cast<py::ssize_t>(lens.size()), py::ssize_t{2}});
        std::copy(plan.items.begin(), plan.items.end(), items.mutable_data());
        std::copy(plan.seq.begin(), plan.seq.end(), seq.mutable_data());
        return py::make_tuple(items, seq);
      },
      py::arg("lens"), py::arg("target"), py::arg("chunk") = payload::kAttnChunk,
      "the work plan of the paged decode kernels, computed on the host with the "
      "arithmetic of the device's plan kernel: (items int32 (n,3) of (sequence, "
      "chunk_begin, chunk_end) over chunks of `chunk` keys, 32 for the bf16 cache "
      "and 64 for the fp8 one, seq int32 (B,2) of (first partial, partials) per "
      "sequence); n <= target + B, target in 1 .. 4096; host only, no GPU");

  m.def(
      "run_attn_paged_check",
      [](int batch, int hq, int hkv, int length, int page, int workgroups, int device) {
        payload::attn_paged_shape(batch, hq, hkv, page, 1, 1, workgroups);
        if (length < 1 || length > (1 << 24))
          throw py::value_error("run_attn_paged_check: length must be in 1 .. 2^24");
        payload::AttnCheck r;
        {
          py::gil_scoped_release rel;
          r = payload::run_attn_paged_check(batch, hq, hkv, length, page, workgroups,
                                            device);
        }
        return attn_check_dict(r);
      },
      py::arg("batch"), py::arg("hq"), py::arg("hkv"), py::arg("length"),
      py::arg("page") = 64, py::arg("workgroups") = 0, py::arg("device") = 0,
      "paged decode attention self-check on ragged lengths derived from `length` "
      "(the length itself, 1, a multiple of 32, a multiple of page plus one) under "
      "a scrambled table with NaN in the unreferenced pages: max_err of the "
      "selection pattern (expect exactly 0) and max_rel = max |o - fp64 ref| / max "
      "|v| of a dense pattern (expect <= 2^-8)");

  m.def(
      "run_attn_paged",
      [](int batch, int hq, int hkv, int length, int page, int iters, bool ragged,
         int workgroups, int device, bool contiguous) {
        payload::attn_paged_shape(batch, hq, hkv, page, 1, 1, workgroups);
        if (iters < 1) throw py::value_error("run_attn_paged: iters must be >= 1");
        payload::AttnPagedResult r;
        {
          py::gil_scoped_release rel;
          r = payload::run_attn_paged(batch, hq, hkv, length, page, iters, ragged,
                                      workgroups, device, contiguous);
        }
        return paged_timed_dict(batch, hq, hkv, length, iters, page, ragged, r);
      },
      py::arg("batch") = 32, py::arg("hq") = 64, py::arg("hkv") = 8,
      py::arg("length") = 4096, py::arg("page") = 64, py::arg("iters") = 10,
      py::arg("ragged") = false, py::arg("workgroups") = 0, py::arg("device") = 0,
      py::arg("contiguous") = false,
      "timed paged decode attention on the selection pattern (pool filled on the "
      "device through a fixed scrambled table; plan, decode and combine per "
      "launch), 16 output rows checked exactly; ragged=True gives every eighth "
      "sequence `length` keys and the rest length/8; kv_gb_per_s counts the keys "
      "below the lengths; items is the plan's item count; contiguous=True times "
      "the contiguous kernel on the same lengths and data instead (length a "
      "multiple of page), for comparison");

  // ---- paged decode attention over an fp8 cache ------------------------------

  m.def(
      "attn_paged_decode_fp8",
      [](f32_array q, py::object k_codes_, py::object v_codes_, f32_array k_scale,
         f32_array v_scale, py::object table_, py::object lens_, py::object scale,
         int workgroups, int device) {
        const char* who = "attn_paged_decode_fp8";
        auto k_codes = uint8_operand(who, "k_codes", k_codes_);
        auto v_codes = uint8_operand(who, "v_codes", v_codes_);
        const PagedOperands a =
            paged_operands(who, "k_codes and v_codes", q, k_codes, v_codes, table_, lens_);
        const py::ssize_t B = a.B, Hq = a.Hq, Hkv = a.Hkv, page = a.page, W = a.W, P = a.P;
        scale_vector(who, "k_scale", k_scale, static_cast<int>(Hkv));
        scale_vector(who, "v_scale", v_scale, static_cast<int>(Hkv));
        payload::attn_paged_fp8_shape(B, Hq, Hkv, page, W, P, workgroups);
        const float sc = attn_scale(who, scale);
        const float* pq = q.data();
        const uint8_t* pk = k_codes.data();
        const uint8_t* pv = v_codes.data();
        const float* pks = k_scale.data();
        const float* pvs = v_scale.data();
        py::array_t<float> o({B, Hq, static_cast<py::ssize_t>(payload::kAttnD)});
        float* po = o.mutable_data();
        {
          py::gil_scoped_release rel;
          payload::attn_paged_decode_fp8(pq, pk, pv, pks, pvs, a.tab.data(), a.lens.data(),
                                         po, static_cast<int>(B), static_cast<int>(Hq),
                                         static_cast<int>(Hkv), static_cast<int>(page),
                                         static_cast<int>(W), static_cast<int>(P), sc,
                                         workgroups, device);
        }
        return o;
      },
      py::arg("q"), py::arg("k_codes"), py::arg("v_codes"), py::arg("k_scale"),
      py::arg("v_scale"), py::arg("table"), py::arg("lens"),
      py::arg("scale") = py::none(), py::arg("workgroups") = 0, py::arg("device") = 0,
      "o (B,Hq,128) float32: attn_paged_decode over an FP8 cache. k_codes and "
      "v_codes (P,Hkv,page,128) uint8 hold OCP e4m3 codes (to_e4m3(x / s)), page "
      "64, 128 or 256; k_scale and v_scale (Hkv,) float32, finite and > 0, are the "
      "scales s per kv head: K = k_scale[g] * e4m3(k_codes), likewise V. The codes "
      "are widened to bf16 exactly, in registers, in front of the bf16 MFMA; the "
      "scales are folded into the score factor and the output. Only the 64-key "
      "chunks below ceil(lens[b]/64) are read; they must hold no NaN code (0x7F, "
      "0xFF). table, lens, scale and workgroups as in attn_paged_decode. TypeError "
      "on pools that are not uint8 or a floating table or lens, ValueError on an "
      "unsupported shape, scale, length, table entry, NaN code or non-finite q, "
      "all before any device work");

  m.def(
      "run_attn_paged_fp8_check",
      [](int batch, int hq, int hkv, int length, int page, int workgroups, bool ragged,
         int device) {
        payload::attn_paged_fp8_shape(batch, hq, hkv, page, 1, 1, workgroups);
        if (length < 1 || length > (1 << 24))
          throw py::value_error("run_attn_paged_fp8_check: length must be in 1 .. 2^24");
        payload::AttnCheck r;
        {
          py::gil_scoped_release rel;
          r = payload::run_attn_paged_fp8_check(batch, hq, hkv, length, page, workgroups,
                                                ragged, device);
        }
        return attn_check_dict(r);
      },
      py::arg("batch"), py::arg("hq"), py::arg("hkv"), py::arg("length"),
      py::arg("page") = 64, py::arg("workgroups") = 0, py::arg("ragged") = true,
      py::arg("device") = 0,
      "fp8 paged decode attention self-check. ragged=True: sequence b takes entry b "
      "% 8 of (length, 1, 33, 63, 64, 65, 2 page + 1, a multiple of 64), each at "
      "most `length`; otherwise every sequence has `length` keys. Scrambled table, "
      "NaN codes in everything that must not be read, 448 at the stale keys of a "
      "read chunk: max_err of the e4m3 selection pattern (expect exactly 0) and "
      "max_rel = max |o - fp64 ref on the dequantised values| / max |v| of a dense "
      "pattern (expect <= 2^-8)");

  m.def(
      "run_attn_paged_fp8",
      [](int batch, int hq, int hkv, int length, int page, int iters, bool ragged,
         int workgroups, int device) {
        payload::attn_paged_fp8_shape(batch, hq, hkv, page, 1, 1, workgroups);
        if (iters < 1) throw py::value_error("run_attn_paged_fp8: iters must be >= 1");
        payload::AttnPaged8Result r;
        {
          py::gil_scoped_release rel;
          r = payload::run_attn_paged_fp8(batch, hq, hkv, length, page, iters, ragged,
                                          workgroups, device);
        }
        return paged_timed_dict(batch, hq, hkv, length, iters, page, ragged, r, &r);
      },
      py::arg("batch") = 32, py::arg("hq") = 64, py::arg("hkv") = 8,
      py::arg("length") = 4096, py::arg("page") = 64, py::arg("iters") = 10,
      py::arg("ragged") = false, py::arg("workgroups") = 0, py::arg("device") = 0,
      "timed fp8 paged decode attention on the e4m3 selection pattern (pool filled "
      "on the device; plan, decode and combine per launch), 16 output rows checked "
      "exactly; us is the time of a step, kv_gb_per_s counts one byte per element "
      "of the keys below the lengths; bf16_us is run_attn_paged on the same "
      "arguments in the same process; quant_rel is the error against fp64 on "
      "unquantised dense data, a property of the format that is never judged");

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

  // ---- paged chunked-prefill (extend) attention --------------------------------

  m.def(
      "attn_paged_extend",
      [](f32_array q, f32_array k_pages, f32_array v_pages, py::object table_,
         py::object lens_, py::object qlens_, py::object scale, int device) {
        const char* who = "attn_paged_extend";
        const std::string w(who);
        auto table = paged_ints(who, "table", table_, 2);
        auto lens_arr = paged_ints(who, "lens", lens_, 1);
        auto qlens_arr = paged_ints(who, "qlens", qlens_, 1);
        if (q.ndim() != 3) throw py::value_error(w + ": q must be (Tq,Hq,128)");
        if (k_pages.ndim() != 4 || v_pages.ndim() != 4)
          throw py::value_error(w + ": k_pages and v_pages must be (P,Hkv,page,128)");
        if (q.shape(2) != payload::kAttnD || k_pages.shape(3) != payload::kAttnD)
          throw py::value_error(w + ": head dim must be 128");
        for (int i = 0; i < 4; ++i)
          if (k_pages.shape(i) != v_pages.shape(i))
            throw py::value_error(w + ": k_pages and v_pages differ in shape");
        const py::ssize_t B = table.shape(0), W = table.shape(1), Tq = q.shape(0),
                          Hq = q.shape(1), P = k_pages.shape(0), Hkv = k_pages.shape(1),
                          page = k_pages.shape(2);
        if (lens_arr.shape(0) != B || qlens_arr.shape(0) != B)
          throw py::value_error(w + ": table must be (B,W), lens and qlens (B,)");
        payload::attn_extend_shape(B, Hq, Hkv, page, W, P, Tq);
        const float sc = attn_scale(who, scale);
        const std::vector<int> tab = paged_narrow(table), lens = paged_narrow(lens_arr),
                               qlens = paged_narrow(qlens_arr);
        const float* pq = q.data();
        const float* pk = k_pages.data();
        const float* pv = v_pages.data();
        py::array_t<float> o({Tq, Hq, static_cast<py::ssize_t>(payload::kAttnD)});
        float* po = o.mutable_data();
        {
          py::gil_scoped_release rel;
          payload::attn_paged_extend(pq, pk, pv, tab.data(), lens.data(), qlens.data(), po,
                                     static_cast<int>(B), static_cast<int>(Hq),
                                     static_cast<int>(Hkv), static_cast<int>(page),
                                     static_cast<int>(W), static_cast<int>(P),
                                     static_cast<int>(Tq), sc, device);
        }
        return o;
      },
      py::arg("q"), py::arg("k_pages"), py::arg("v_pages"), py::arg("table"),
      py::arg("lens"), py::arg("qlens"), py::arg("scale") = py::none(),
      py::arg("device") = 0,
      "o (Tq,Hq,128) float32: chunked-prefill (extend) attention over a paged KV "
      "cache. The last qlens[b] of the lens[b] keys of sequence b are new tokens; q "
      "(Tq,Hq,128) packs their queries, sequence after sequence, Tq = sum(qlens). "
      "Token i of sequence b attends to the keys t <= lens[b] - qlens[b] + i. "
      "k_pages, v_pages, table and lens as in attn_paged_decode (the new tokens' "
      "keys are in the pool already); qlens (B,) integer in 1 .. lens[b]. "
      "scale=None is 1/sqrt(128). TypeError on a floating table, lens or qlens, "
      "ValueError on an unsupported shape, length, table entry, qlens that do not "
      "sum to Tq or a non-finite input, all before any device work");

  m.def(
      "attn_extend_plan",
      [](py::object qlens_, int group) {
        auto arr = paged_ints("attn_extend_plan", "qlens", qlens_, 1);
        if (arr.shape(0) < 1 || arr.shape(0) > 65535)
          throw py::value_error("attn_extend_plan: qlens must hold 1 .. 65535 lengths");
        const std::vector<int> qlens = paged_narrow(arr);
        const payload::AttnExtendPlan plan = payload::attn_extend_plan(
            qlens.data(), static_cast<int>(qlens.size()), group);
        py::array_t<int32_t> items({static_cast<py::ssize_t>(plan.items.size() / 2),
                                    py::ssize_t{2}});
        py::array_t<int32_t> cu(static_cast<py::ssize_t>(qlens.size()));
        std::copy(plan.items.begin(), plan.items.end(), items.mutable_data());
        std::copy(plan.cu.begin(), plan.cu.end(), cu.mutable_data());
        return py::make_tuple(items, cu);
      },
      py::arg("qlens"), py::arg("group"),
      "the work plan of the extend kernel, computed on the host with the arithmetic "
      "of the device's plan kernel: (items int32 (n,2) of (sequence, first column) "
      "over blocks of 128 of a sequence's qlens[b] * group (token, head) columns, "
      "cu int32 (B,) of a sequence's first token in the packed q); n <= "
      "ceil(sum(qlens) * group / 128) + B, group in 1 .. 16; host only, no GPU");

  m.def(
      "run_attn_extend_check",
      [](int batch, int hq, int hkv, int length, int page, int device) {
        payload::attn_paged_shape(batch, hq, hkv, page, 1, 1);
        if (length < 1 || length > payload::kExtendMaxLen)
          throw py::value_error("run_attn_extend_check: length must be in 1 .. 2^24");
        payload::AttnCheck r;
        {
          py::gil_scoped_release rel;
          r = payload::run_attn_extend_check(batch, hq, hkv, length, page, device);
        }
        return attn_check_dict(r);
      },
      py::arg("batch"), py::arg("hq"), py::arg("hkv"), py::arg("length"),
      py::arg("page") = 64, py::arg("device") = 0,
      "extend attention self-check on the ragged lengths of run_attn_paged_check and "
      "runs of new tokens that cycle through (1, the whole length, 17, an odd "
      "prefix), under a scrambled table with NaN in the unreferenced pages: max_err "
      "of prefill's selection pattern (expect exactly 0) and max_rel = max |o - fp64 "
      "ref| / max |v| of a dense pattern (expect <= 2^-8)");

  m.def(
      "run_attn_extend",
      [](int batch, int hq, int hkv, int length, int new_tokens, int page, int iters,
         bool ragged, int device) {
        payload::attn_paged_shape(batch, hq, hkv, page, 1, 1);
        if (iters < 1) throw py::value_error("run_attn_extend: iters must be >= 1");
        payload::AttnExtendResult r;
        {
          py::gil_scoped_release rel;
          r = payload::run_attn_extend(batch, hq, hkv, length, new_tokens, page, iters,
                                       ragged, device);
        }
        py::dict d = attn_timed_dict(batch, hq, hkv, length, iters);
        d["new"] = new_tokens;
        d["page"] = page;
        d["ragged"] = ragged;
        d["items"] = r.items;
        d["tflops"] = r.tflops;
        d["tok_per_s"] = r.tok_per_s;
        d["max_rel"] = r.max_rel;
        return d;
      },
      py::arg("batch") = 8, py::arg("hq") = 64, py::arg("hkv") = 8,
      py::arg("length") = 4096, py::arg("new_tokens") = 1024, py::arg("page") = 64,
      py::arg("iters") = 10, py::arg("ragged") = false, py::arg("device") = 0,
      "timed extend attention: the last min(new_tokens, len) keys of every sequence "
      "are new tokens; pool and q filled on the device with the dense hash pattern "
      "through a fixed scrambled table; plan and extend per launch; TFLOP/s over "
      "the unmasked pairs only, tok_per_s over the new tokens, 16 spread output "
      "rows checked against fp64; ragged=True gives every eighth sequence `length` "
      "keys and the rest length/8; items is the plan's item count");
}
