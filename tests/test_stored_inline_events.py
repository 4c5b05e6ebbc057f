"""instaslice-stored sends a watch event from the thread that made the
mutation (store/csrc/stored_core.hpp, Conn::flush_inline). What must not
change with that: event order per connection, writers never waiting for a
slow watcher, the outbox cap, and the subscribe response coming first."""

import socket
import threading
import time

import pytest

from instaslice_amd.store import netstore
from instaslice_amd.store.native import NativeStoreServer, stored_available
from instaslice_amd.store.netstore import NetStoreClient

K_MAX_OUTBOX = 65536  # Conn::kMaxOutbox


@pytest.fixture
def stored():
    assert stored_available(), "instaslice-stored is not built"
    srv = NativeStoreServer().start()
    yield srv
    srv.stop()


def _obj(name, **extra):
    return {"apiVersion": "v1", "kind": "Thing",
            "metadata": {"name": name, "namespace": ""}, **extra}


def _patch_req(name, i):
    return {"verb": "patch", "kind": "Thing", "name": name, "namespace": "",
            "ops": [{"op": "set", "path": ["spec", "i"], "value": i}]}


class _RawConn:
    """The protocol by hand, for a peer that reads only when told to."""

    def __init__(self, port, rcvbuf=None):
        self.sock = socket.socket()
        if rcvbuf is not None:  # before connect: it sizes the TCP window
            self.sock.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, rcvbuf)
        self.sock.connect(("127.0.0.1", port))
        self.sock.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
        self.rfile = self.sock.makefile("rb")

    def send(self, obj):
        self.sock.sendall(netstore._pack(obj))

    def read(self):
        return netstore._read_msg(self.rfile)

    def close(self):
        self.rfile.close()
        self.sock.close()


def test_event_order_under_contention(stored):
    """8 writer connections hammer one object; a watcher on a ninth sees
    every event, strictly in resourceVersion order."""
    writers, per_writer = 8, 300
    watcher = NetStoreClient("127.0.0.1", stored.port)
    clients = [NetStoreClient("127.0.0.1", stored.port)
               for _ in range(writers)]
    try:
        first = clients[0].create(_obj("hot", spec={"i": 0}))
        w = watcher.watch("Thing", replay=False)
        errors = []

        def hammer(c, t):
            try:
                for i in range(per_writer):
                    c.patch("Thing", "hot", "",
                            _patch_req("hot", t * per_writer + i)["ops"],
                            quiet=True)
            except Exception as e:  # noqa: BLE001 - reported below
                errors.append(repr(e))

        threads = [threading.Thread(target=hammer, args=(c, t))
                   for t, c in enumerate(clients)]
        for th in threads:
            th.start()
        total = writers * per_writer
        rvs = []
        while len(rvs) < total:
            ev = w.next(timeout=10)
            assert ev is not None, f"stalled after {len(rvs)} of {total}"
            rvs.append(int(ev[1]["metadata"]["resourceVersion"]))
        for th in threads:
            th.join(10)
        assert not errors, errors
        # nothing else mutates the store: the revisions are consecutive, so
        # "in order" and "none missing" are one comparison
        base = int(first["metadata"]["resourceVersion"])
        assert rvs == list(range(base + 1, base + 1 + total))
        assert w.next(timeout=0.05) is None
    finally:
        watcher.close()
        for c in clients:
            c.close()


def test_stalled_watcher_neither_slows_writers_nor_outlives_the_cap(stored):
    batch, timed_batches = 500, 20
    c = NetStoreClient("127.0.0.1", stored.port)
    stalled = None
    try:
        c.create(_obj("hot", spec={"i": 0, "pad": "p" * 200}))
        sent = 0

        def push(n_batches):
            nonlocal sent
            t0 = time.perf_counter()
            for _ in range(n_batches):
                res = c.batch([_patch_req("hot", sent + k)
                               for k in range(batch)], quiet=True)
                assert all(r["ok"] for r in res)
                sent += batch
            return n_batches * batch / (time.perf_counter() - t0)

        push(2)  # warm
        rate_alone = push(timed_batches)

        # a watcher that subscribes and then never reads again; the small
        # receive buffer keeps what TCP itself can park for it small
        stalled = _RawConn(stored.port, rcvbuf=4096)
        stalled.send({"id": 1, "verb": "watch", "kind": "Thing",
                      "replay": False})
        assert stalled.read()["ok"]
        sent_before_stall = sent
        rate_stalled = push(timed_batches)
        print(f"writer rate alone {rate_alone:.0f}/s, "
              f"with a stalled watcher {rate_stalled:.0f}/s")
        # the same order of magnitude: a writer that waited for the stalled
        # socket even once would not finish at all
        assert rate_stalled >= rate_alone / 10.0

        # past the cap the daemon drops the watcher: kMaxOutbox queued events
        # on top of whatever the socket buffers took (at ~0.4 KB an event,
        # the 4 MiB the kernel allows a send buffer hold ~10k)
        while sent - sent_before_stall < K_MAX_OUTBOX + 30000:
            push(10)
        assert c._call("ping") == "pong"
        stalled.sock.settimeout(10)
        received = 0
        while True:
            msg = stalled.read()  # None: the daemon closed the connection
            if msg is None:
                break
            received += 1
        assert received < sent - sent_before_stall - K_MAX_OUTBOX // 2, (
            f"{received} of {sent - sent_before_stall} events were served: "
            "the watcher was not cut off at the cap")
    finally:
        if stalled is not None:
            stalled.close()
        c.close()


def test_subscribe_response_precedes_first_event(stored):
    """With writers mutating matching objects all the while, the first frame
    on a fresh connection that subscribes is the subscribe response, and its
    watch's events follow — replayed ones first, in name order."""
    c = NetStoreClient("127.0.0.1", stored.port)
    stop = threading.Event()
    try:
        for i in range(20):
            c.create(_obj(f"o{i:02d}", spec={"i": 0}))

        def churn():
            i = 0
            w = NetStoreClient("127.0.0.1", stored.port)
            try:
                while not stop.is_set():
                    i += 1
                    w.patch("Thing", "o00", "", _patch_req("o00", i)["ops"],
                            quiet=True)
            finally:
                w.close()

        th = threading.Thread(target=churn)
        th.start()
        for round_ in range(25):
            raw = _RawConn(stored.port)
            try:
                raw.send({"id": 7, "verb": "watch", "kind": "Thing",
                          "replay": True})
                first = raw.read()
                assert first.get("id") == 7 and first["ok"], first
                wid = first["result"]["watch_id"]
                names = []
                for _ in range(20):
                    ev = raw.read()
                    assert ev["watch_id"] == wid
                    assert ev["event"][0] == "ADDED"
                    names.append(ev["event"][1]["metadata"]["name"])
                assert names == [f"o{i:02d}" for i in range(20)]
                # live events after the replay: never older than the replay
                ev = raw.read()
                assert ev["watch_id"] == wid and ev["event"][0] == "MODIFIED"
                assert (int(ev["event"][1]["metadata"]["resourceVersion"])
                        > first["result"]["rev"])
            finally:
                raw.close()
        stop.set()
        th.join(10)
    finally:
        stop.set()
        c.close()
