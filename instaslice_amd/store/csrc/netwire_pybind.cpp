// _netwire: pybind11 layer over netwire_core.hpp (see there for the design).
//
// The GIL is held only where Python objects are touched: call()/send()/
// close() release it around everything that can block, and the reader
// thread takes it only to run on_frame / on_closed.

#include <pybind11/pybind11.h>

#include <memory>
#include <string>

#include "netwire_core.hpp"

namespace py = pybind11;

namespace {

bool finalizing() {
#if PY_VERSION_HEX >= 0x030D0000
  return Py_IsFinalizing();
#else
  return _Py_IsFinalizing();
#endif
}

// a Python callable owned from C++: released under the GIL whichever thread
// drops the last reference (never while the interpreter is going down)
std::shared_ptr<py::object> hold(py::object o) {
  return std::shared_ptr<py::object>(
      new py::object(std::move(o)), [](py::object* p) {
        if (finalizing()) {
          p->release();  // leak: no interpreter left to free it in
        } else {
          py::gil_scoped_acquire gil;
          p->dec_ref();
          p->release();
        }
        delete p;
      });
}

void report_unraisable(py::error_already_set& e, const py::object& ctx) {
  e.restore();
  PyErr_WriteUnraisable(ctx.ptr());
}

class PyWire {
 public:
  // `owner` (the socket object the fd belongs to) is only kept alive: the
  // fd must outlive the reader whatever order the garbage collector takes
  // a dropped client apart in
  PyWire(int fd, py::object on_frame, py::object on_closed, py::object owner)
      : owner_(std::move(owner)) {
    auto frame_cb = hold(std::move(on_frame));
    auto closed_cb = hold(std::move(on_closed));
    py::gil_scoped_release nogil;  // create() starts the reader thread
    wire_ = netwire::Wire::create(
        fd,
        [frame_cb](const char* p, size_t n) {
          if (finalizing()) return;
          py::gil_scoped_acquire gil;
          try {
            (*frame_cb)(py::bytes(p, n));
          } catch (py::error_already_set& e) {
            // a consumer bug must not kill the reader
            report_unraisable(e, *frame_cb);
          }
        },
        [closed_cb]() {
          if (finalizing()) return;
          py::gil_scoped_acquire gil;
          try {
            (*closed_cb)();
          } catch (py::error_already_set& e) {
            report_unraisable(e, *closed_cb);
          }
        });
  }

  ~PyWire() { close(); }

  void send(const py::bytes& data) {
    char* p;
    Py_ssize_t n;
    if (PyBytes_AsStringAndSize(data.ptr(), &p, &n) != 0)
      throw py::error_already_set();
    bool ok;
    {
      py::gil_scoped_release nogil;
      ok = wire_->send(p, static_cast<size_t>(n));
    }
    if (!ok) raise(PyExc_ConnectionError, "netstore send failed");
  }

  py::bytes call(int64_t rid, const py::bytes& req, double timeout_s) {
    char* p;
    Py_ssize_t n;
    if (PyBytes_AsStringAndSize(req.ptr(), &p, &n) != 0)
      throw py::error_already_set();
    std::string out;
    netwire::CallStatus st;
    {
      py::gil_scoped_release nogil;  // `req` is kept alive by our caller
      st = wire_->call(rid, p, static_cast<size_t>(n), timeout_s, out);
    }
    switch (st) {
      case netwire::CallStatus::Ok:
        return py::bytes(out);
      case netwire::CallStatus::Timeout:
        raise(PyExc_TimeoutError, "netstore call timed out");
      case netwire::CallStatus::SendFailed:
        raise(PyExc_ConnectionError, "netstore send failed");
      case netwire::CallStatus::Lost:
        break;
    }
    raise(PyExc_ConnectionError, "connection lost");
  }

  void close() {
    // the reader may be waiting for the GIL inside a callback: let it finish
    py::gil_scoped_release nogil;
    wire_->close();
  }

  bool alive() const { return wire_->alive(); }

 private:
  [[noreturn]] static void raise(PyObject* type, const char* msg) {
    PyErr_SetString(type, msg);
    throw py::error_already_set();
  }

  std::shared_ptr<netwire::Wire> wire_;
  py::object owner_;
};

}  // namespace

PYBIND11_MODULE(_netwire, m) {
  m.doc() = "native store wire: framing, response demultiplexing and the "
            "reader thread of a NetStoreClient, off the GIL";
  py::class_<PyWire>(m, "Wire")
      .def(py::init<int, py::object, py::object, py::object>(),
           py::arg("fd"), py::arg("on_frame"), py::arg("on_closed"),
           py::arg("owner") = py::none())
      .def("send", &PyWire::send)
      .def("call", &PyWire::call, py::arg("rid"), py::arg("request"),
           py::arg("timeout_s"))
      .def("close", &PyWire::close)
      .def("alive", &PyWire::alive);
}
