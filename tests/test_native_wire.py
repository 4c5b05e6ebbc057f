"""NetStoreClient over the native wire (store/_netwire) and over the
pure-Python wire: the same battery against both store servers, so the two
paths cannot drift apart. CPU tier; every case takes at most a few seconds."""

import socket
import threading
import time

import pytest

from instaslice_amd.store import AlreadyExists, Conflict, NotFound
from instaslice_amd.store import netstore
from instaslice_amd.store.native import NativeStoreServer, stored_available
from instaslice_amd.store.netstore import NetStoreClient, StoreServer

if netstore._netwire is None:
    pytest.skip("the _netwire extension is not built", allow_module_level=True)


def _start_stored():
    # the daemon is this project's own build product: missing, it fails the
    # case, it does not quietly halve the battery
    assert stored_available(), "instaslice-stored is not built"
    return NativeStoreServer().start()


@pytest.fixture(params=[
    pytest.param(lambda: StoreServer().start(), id="pyserver"),
    pytest.param(_start_stored, id="stored"),
])
def server(request):
    srv = request.param()
    yield srv
    srv.stop()


@pytest.fixture(params=["wire", "pywire"])
def wire_mode(request, monkeypatch):
    monkeypatch.setenv("INSTASLICE_NATIVE_WIRE",
                       "1" if request.param == "wire" else "0")
    return request.param


@pytest.fixture
def client(server, wire_mode):
    c = NetStoreClient("127.0.0.1", server.port)
    assert (c._wire is not None) == (wire_mode == "wire")
    yield c
    c.close()


def _obj(name, kind="Thing", ns="", **extra):
    return {"apiVersion": "v1", "kind": kind,
            "metadata": {"name": name, "namespace": ns}, **extra}


def _rv(obj):
    return int(obj["metadata"]["resourceVersion"])


# -- verbs and errors ---------------------------------------------------------

def test_verbs_and_errors_roundtrip(client):
    c = client
    assert c._call("ping") == "pong"
    created = c.create(_obj("a", spec={"v": 1}))
    assert created["spec"] == {"v": 1}
    with pytest.raises(AlreadyExists):
        c.create(_obj("a"))
    assert c.get("Thing", "a")["metadata"]["name"] == "a"
    assert [o["metadata"]["name"] for o in c.list("Thing")] == ["a"]
    stale = c.get("Thing", "a")
    fresh = dict(stale, spec={"v": 2})
    assert c.update(fresh)["spec"] == {"v": 2}
    with pytest.raises(Conflict):
        c.update(stale)
    patched = c.patch("Thing", "a", "",
                      [{"op": "set", "path": ["spec", "v"], "value": 3}])
    assert patched["spec"]["v"] == 3
    assert c.patch("Thing", "a", "",
                   [{"op": "set", "path": ["spec", "v"], "value": 4}],
                   quiet=True) is None
    res = c.batch([
        {"verb": "create", "obj": _obj("b")},
        {"verb": "get", "kind": "Thing", "name": "nope", "namespace": ""},
    ])
    assert res[0]["ok"] and not res[1]["ok"]
    assert res[1]["error"]["type"] == "NotFound"
    c.delete("Thing", "a")
    with pytest.raises(NotFound):
        c.get("Thing", "a")
    with pytest.raises(NotFound):
        c.delete("Thing", "a")


# -- event order ----------------------------------------------------------------

N_PATCHES = 1000


def _patch_n(c, n):
    for i in range(n):
        c.patch("Thing", "hot", "",
                [{"op": "set", "path": ["spec", "i"], "value": i}], quiet=True)


def _assert_in_order(events, n):
    assert len(events) == n, f"{len(events)} events, wanted {n}"
    rvs = [_rv(o) for _, o in events]
    assert rvs == sorted(rvs) and len(set(rvs)) == n
    assert [o["spec"]["i"] for _, o in events] == list(range(n))


def test_event_order_queue_mode(client):
    client.create(_obj("hot", spec={"i": -1}))
    w = client.watch("Thing", replay=False)
    _patch_n(client, N_PATCHES)
    got = []
    while len(got) < N_PATCHES:
        ev = w.next(timeout=5)
        assert ev is not None, f"stalled after {len(got)} events"
        got.append(ev)
    _assert_in_order(got, N_PATCHES)


def test_event_order_callback_mode(client):
    client.create(_obj("hot", spec={"i": -1}))
    w = client.watch("Thing", replay=False)
    # the first events land in the queue, set_callback drains them, the rest
    # arrive on the reader: one ordered sequence across the switch
    _patch_n(client, N_PATCHES // 2)
    got, done = [], threading.Event()

    def cb(et, obj):
        got.append((et, obj))
        if len(got) == N_PATCHES:
            done.set()

    w.set_callback(cb)
    for i in range(N_PATCHES // 2, N_PATCHES):
        client.patch("Thing", "hot", "",
                     [{"op": "set", "path": ["spec", "i"], "value": i}],
                     quiet=True)
    assert done.wait(10), f"only {len(got)} events"
    _assert_in_order(got, N_PATCHES)


def test_events_before_watch_registers_are_delivered_in_order(client,
                                                              monkeypatch):
    """The orphan path: hold watch() between the subscribe response and the
    registration of its id while events stream in."""
    for i in range(50):
        client.create(_obj(f"o{i:02d}"))
    real_call = client._call
    wid_seen = {}

    def slow_call(verb, **kw):
        res = real_call(verb, **kw)
        if verb == "watch":
            # replay events are on the wire right behind the response: wait
            # until the reader has parked all of them as orphans
            deadline = time.monotonic() + 5
            wid = res["watch_id"]
            while time.monotonic() < deadline:
                with client._watch_reg_lock:
                    if len(client._orphan_events.get(wid, [])) >= 50:
                        break
                time.sleep(0.001)
            wid_seen["n"] = len(client._orphan_events.get(wid, []))
        return res

    monkeypatch.setattr(client, "_call", slow_call)
    w = client.watch("Thing", replay=True)
    assert wid_seen["n"] == 50, "events did not arrive ahead of registration"
    names = []
    for _ in range(50):
        ev = w.next(timeout=5)
        assert ev is not None
        names.append(ev[1]["metadata"]["name"])
    assert names == [f"o{i:02d}" for i in range(50)]
    assert not client._orphan_events


# -- concurrency and framing ------------------------------------------------------

def test_concurrent_calls_match_their_requests(client):
    for t in range(8):
        client.create(_obj(f"t{t}", spec={"owner": t}))
    errors = []

    def worker(t):
        try:
            for i in range(200):
                got = client.patch(
                    "Thing", f"t{t}", "",
                    [{"op": "set", "path": ["spec", "i"], "value": i}])
                assert got["metadata"]["name"] == f"t{t}"
                assert got["spec"] == {"owner": t, "i": i}
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(30)
    assert not any(th.is_alive() for th in threads), "a call never returned"
    assert not errors, errors


def test_large_response_over_partial_reads(client):
    pad = "x" * 300
    client.batch([{"verb": "create", "obj": _obj(f"big{i:03d}", spec={"pad": pad, "i": i})}
                  for i in range(300)], quiet=True)
    got = client.list("Thing")  # > 64 KB in one frame
    assert [o["spec"]["i"] for o in got] == list(range(300))
    assert all(o["spec"]["pad"] == pad for o in got)


# -- failure and shutdown ---------------------------------------------------------

class _MuteServer:
    """Accepts one connection and never answers; stop() severs it."""

    def __init__(self):
        self._lsock = socket.socket()
        self._lsock.bind(("127.0.0.1", 0))
        self._lsock.listen(1)
        self.port = self._lsock.getsockname()[1]
        self.conn = None
        self.got_request = threading.Event()
        self._t = threading.Thread(target=self._run, daemon=True)
        self._t.start()

    def _run(self):
        self.conn, _ = self._lsock.accept()
        try:
            if self.conn.recv(4):
                self.got_request.set()
        except OSError:
            pass

    def flood(self, frame: bytes) -> threading.Thread:
        """Send `frame` over and over until the connection is gone."""
        def run():
            try:
                while True:
                    self.conn.sendall(frame)
            except OSError:
                pass

        t = threading.Thread(target=run, daemon=True)
        t.start()
        return t

    def kill(self):
        try:
            self.conn.shutdown(socket.SHUT_RDWR)
        except OSError:
            pass  # the client went first
        self.conn.close()

    def stop(self):
        self._lsock.close()


def test_server_death_fails_the_call_and_stops_watches(wire_mode):
    """The server goes away while a call is waiting for its answer (a
    stand-in server, so that the call is certainly in flight when it dies;
    the next test kills the real daemon)."""
    mute = _MuteServer()
    c = NetStoreClient("127.0.0.1", mute.port)
    try:
        # a watch object registered by hand: the mute server cannot subscribe
        w = netstore._ClientWatch()
        c._watches[1] = w
        failed = {}

        def call():
            t0 = time.monotonic()
            try:
                c.get("Thing", "a")
            except Exception as e:  # noqa: BLE001 - inspected below
                failed["exc"] = e
            failed["dt"] = time.monotonic() - t0

        th = threading.Thread(target=call)
        th.start()
        assert mute.got_request.wait(5)
        mute.kill()
        th.join(10)
        assert not th.is_alive()
        assert isinstance(failed["exc"], ConnectionError), failed
        assert failed["dt"] < 5.0
        deadline = time.monotonic() + 5
        while not w._stopped and time.monotonic() < deadline:
            time.sleep(0.005)
        assert w._stopped
        with pytest.raises(ConnectionError):
            c.get("Thing", "a")
    finally:
        c.close()
        mute.stop()


def test_real_server_death_is_a_connection_error(wire_mode):
    """Same, against the daemon itself being killed."""
    srv = _start_stored()
    c = NetStoreClient("127.0.0.1", srv.port)
    try:
        w = c.watch("Thing")
        c.create(_obj("a"))
        assert w.next(timeout=5)[0] == "ADDED"
        srv.stop()
        t0 = time.monotonic()
        with pytest.raises(ConnectionError):
            for _ in range(100):  # the first call may still race the FIN
                c.get("Thing", "a")
        assert time.monotonic() - t0 < 5.0
        deadline = time.monotonic() + 5
        while not w._stopped and time.monotonic() < deadline:
            time.sleep(0.005)
        assert w._stopped
    finally:
        c.close()
        srv.stop()


def test_close_with_call_in_flight(wire_mode):
    """close() with a call waiting and events streaming in: it returns at
    once, the call fails, and no callback runs once it has returned."""
    mute = _MuteServer()
    c = NetStoreClient("127.0.0.1", mute.port)
    fired = []  # per callback: had close() already returned?
    closed = threading.Event()
    w = netstore._ClientWatch()
    w.set_callback(lambda et, obj: fired.append(closed.is_set()))
    c._watches[1] = w
    failed = {}

    def call():
        try:
            c.get("Thing", "a")
        except Exception as e:  # noqa: BLE001 - inspected below
            failed["exc"] = e

    th = threading.Thread(target=call)
    th.start()
    flooder = None
    try:
        assert mute.got_request.wait(5)
        # events keep arriving right up to, and past, the close
        flooder = mute.flood(netstore._pack(
            {"watch_id": 1, "event": ["ADDED", _obj("e")]}))
        deadline = time.monotonic() + 5
        while len(fired) < 100 and time.monotonic() < deadline:
            time.sleep(0.001)
        assert len(fired) >= 100, "the callback path never was live"
        t0 = time.monotonic()
        c.close()
        closed.set()
        assert time.monotonic() - t0 < 1.0
        if wire_mode == "wire":
            assert not c._wire.alive()  # the native reader is joined
            th.join(5)
            assert not th.is_alive()
            assert isinstance(failed.get("exc"), ConnectionError), failed
            seen = len(fired)
            flooder.join(5)  # the server has noticed the closed socket
            assert len(fired) == seen and True not in fired
        with pytest.raises(ConnectionError):
            c.get("Thing", "a")
    finally:
        mute.kill()
        th.join(5)
        if flooder is not None:
            flooder.join(5)
        mute.stop()
    assert not th.is_alive()


def test_dropped_client_is_collected_without_close(server, monkeypatch):
    import gc
    import weakref

    monkeypatch.delenv("INSTASLICE_NATIVE_WIRE", raising=False)
    c = NetStoreClient("127.0.0.1", server.port)
    c.create(_obj("a"))
    wire = c._wire
    ref = weakref.ref(c)
    del c
    gc.collect()
    assert ref() is None, "the wire's callbacks pin the client"
    del wire  # the last reference: the destructor joins the reader


# -- fallback selection -----------------------------------------------------------

def test_env_selects_python_path(server, monkeypatch):
    monkeypatch.setenv("INSTASLICE_NATIVE_WIRE", "0")
    c = NetStoreClient("127.0.0.1", server.port)
    try:
        assert c._wire is None and c._reader.is_alive()
        assert c._call("ping") == "pong"
    finally:
        c.close()
    monkeypatch.delenv("INSTASLICE_NATIVE_WIRE")
    c = NetStoreClient("127.0.0.1", server.port)
    try:
        assert c._wire is not None and c._reader is None
        assert c._call("ping") == "pong"
    finally:
        c.close()


def test_reconnect_selects_python_path(server, monkeypatch):
    monkeypatch.delenv("INSTASLICE_NATIVE_WIRE", raising=False)
    c = NetStoreClient("127.0.0.1", server.port, reconnect=True)
    try:
        assert c._wire is None and c._reader.is_alive()
        assert c._call("ping") == "pong"
    finally:
        c.close()
