"""Host-side thread contract of the Python layer (nets.py / engine.py; include/d3d.h "Threads"), on a stub engine: no GPU needed.

- range tickets posted inside deferred_range_checks() stay with the thread that opened the block;
- two threads that ask for one device's engine at the same time get ONE Engine and one upload of the weights;
- a DataParallel replica may ask for a second device (one RuntimeWarning), a model that is no replica may not (D3DError);
- guard counters survive concurrent read-modify-writes, and the guard object copies / pickles without its locks."""
import copy
import pickle
import threading
import warnings

import pytest
import torch

import diff3dhpe_amd as d3d
from diff3dhpe_amd import _lib, nets
from host_helpers import create_host_engine, engine_info

JOIN = 30.0


class StubEngine:
    """What nets.py needs of an engine: precision, lock, load_weights, set_option, release_workspace, post_range / take_range."""
    built = []                      # every instance, in construction order
    gate = None                     # an Event the constructor waits on (slows construction down without sleeping)
    entered = None                  # set when a constructor has been entered
    describe_range_flags = staticmethod(nets.Engine.describe_range_flags)

    def __init__(self, cfg, precision="fp32", device=None):
        if StubEngine.entered is not None:
            StubEngine.entered.set()
        if StubEngine.gate is not None:
            assert StubEngine.gate.wait(JOIN)
        self.cfg, self.precision, self.device = cfg, precision, device
        self.lock = threading.RLock()
        self.loads = 0
        self.posts, self.takes = [], []          # (thread id, ticket[, block])
        self.flags = 0
        StubEngine.built.append(self)

    def load_weights(self, sd):
        with self.lock:
            self.loads += 1

    def set_option(self, key, value):
        pass

    def release_workspace(self):
        pass

    def post_range(self):
        with self.lock:
            self.posts.append((threading.get_ident(), len(self.posts)))
            return len(self.posts) - 1

    def take_range(self, ticket, block=True):
        with self.lock:
            self.takes.append((threading.get_ident(), ticket, block))
            return self.flags


@pytest.fixture()
def stub(monkeypatch):
    StubEngine.built, StubEngine.gate, StubEngine.entered = [], None, None
    monkeypatch.setattr(nets, "Engine", StubEngine)
    yield StubEngine
    StubEngine.built, StubEngine.gate, StubEngine.entered = [], None, None


def _net(precision="f16x3"):
    net = d3d.HPE_model(d3d.S2S_NAME)(num_frame=9, embed_dim=32, depth=1)
    net.precision = precision
    net.range_check = True
    net.allow_multi_device = False
    return net


def _replica(net):
    """A replica as torch.nn.parallel.replicate() leaves it: _replicate_for_data_parallel(), then the module's own parameters as
    plain tensors (the broadcast copies there; the tensors themselves here -- no device is touched)."""
    rep = net._replicate_for_data_parallel()
    for key, p in net._parameters.items():
        setattr(rep, key, p.detach())
    return rep


def _run(*targets):
    """Start one thread per target, join each with a time limit; exceptions of the threads are re-raised here."""
    errs = []

    def wrap(fn):
        def go():
            try:
                fn()
            except BaseException as e:      # noqa: BLE001  (reported below)
                errs.append(e)
        return go
    ts = [threading.Thread(target=wrap(fn), daemon=True) for fn in targets]
    for t in ts:
        t.start()
    for t in ts:
        t.join(JOIN)
        assert not t.is_alive(), "a worker thread did not finish"
    if errs:
        raise errs[0]


def test_deferred_tickets_stay_with_their_thread(stub):
    net = _net()
    dev = torch.device("cuda", 0)
    opened, release = threading.Event(), threading.Event()
    seen = {}

    def t1():
        with net.deferred_range_checks() as box:
            opened.set()
            assert release.wait(JOIN)
            seen["items"] = list(box.items)
            seen["resolved"] = box.resolve()

    def t2():
        assert opened.wait(JOIN)
        try:
            seen["t2"] = threading.get_ident()
            seen["out"] = net._guarded(lambda fb: net.engine_for(dev, fb), lambda eng: "ran", "stub call")
        finally:
            release.set()

    _run(t1, t2)
    eng, = stub.built
    assert seen["out"] == "ran"
    assert seen["items"] == [] and seen["resolved"] is False            # thread 1's box never saw thread 2's ticket ...
    assert eng.posts == [(seen["t2"], 0)]
    assert eng.takes == [(seen["t2"], 0, True)]                         # ... which was read at once, waiting, by its own thread
    assert net._guard["posted"] == 1 and net._guard["flagged"] == 0


def test_a_deferred_block_still_collects_its_own_threads_tickets(stub):
    net = _net()
    dev = torch.device("cuda", 0)
    with net.deferred_range_checks() as box:
        net._guarded(lambda fb: net.engine_for(dev, fb), lambda eng: None, "a")
        net._guarded(lambda fb: net.engine_for(dev, fb), lambda eng: None, "b")
        eng, = stub.built
        assert len(box.items) == 2 and eng.takes == []
        assert box.resolve() is False
    assert [t[1:] for t in eng.takes] == [(0, True), (1, True)]
    net._guarded(lambda fb: net.engine_for(dev, fb), lambda eng: None, "c")     # block closed: read at once again
    assert eng.takes[-1][1:] == (2, True) and net._guard["posted"] == 3


def test_the_engine_lock_is_held_from_the_launch_to_the_posted_ticket(stub):
    net = _net()
    dev = torch.device("cuda", 0)
    eng = net.engine_for(dev)
    held = []
    real_post = eng.post_range

    def another_thread_cannot_take_it():
        got = []

        def probe():
            ok = eng.lock.acquire(blocking=False)
            got.append(ok)
            if ok:
                eng.lock.release()
        _run(probe)
        return not got[0]

    def post():
        held.append(another_thread_cannot_take_it())
        return real_post()
    eng.post_range = post
    net._guarded(lambda fb: net.engine_for(dev, fb), lambda e: held.append(another_thread_cannot_take_it()), "call")
    assert held == [True, True]
    assert not another_thread_cannot_take_it()


def test_one_engine_per_device_under_contention(stub):
    net = _net()
    dev = torch.device("cuda", 0)
    stub.gate, stub.entered = threading.Event(), threading.Event()
    got = []
    second_started = threading.Event()

    def first():
        got.append(net.engine_for(dev))

    def second():
        assert stub.entered.wait(JOIN)          # the first thread is inside the (slowed) constructor, holding the guard's engines lock
        second_started.set()
        got.append(net.engine_for(dev))

    def opener():
        assert second_started.wait(JOIN)
        stub.gate.set()

    _run(first, second, opener)
    assert len(stub.built) == 1 and got[0] is got[1] is stub.built[0]
    assert stub.built[0].loads == 1


def test_the_refusal_rule(stub):
    net = _net()
    rep = _replica(net)
    assert rep._src_sig is not None and rep._guard is net._guard and rep._engines is net._engines
    rep.engine_for(torch.device("cuda", 0))
    with warnings.catch_warnings(record=True) as wlog:
        warnings.simplefilter("always")
        e1 = rep.engine_for(torch.device("cuda", 1))
    assert len(wlog) == 1 and issubclass(wlog[0].category, RuntimeWarning)
    assert ("several devices in one process: host-side concurrency is tested on one device, the multi-device run itself is "
            "unmeasured on hardware") in str(wlog[0].message)
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # once per model: neither the same replica nor a later one warns again
        assert rep.engine_for(torch.device("cuda", 1)) is e1
        _replica(net).engine_for(torch.device("cuda", 2))
    assert sorted(net._engines) == [0, 1, 2]

    plain = _net()                              # no replica, not moved: today's refusal
    plain.engine_for(torch.device("cuda", 0))
    with pytest.raises(_lib.D3DError, match="ONE device per process"):
        plain.engine_for(torch.device("cuda", 1))
    assert list(plain._engines) == [0]

    quiet = _net()                              # the opt-in keeps its meaning and silences the warning
    quiet.allow_multi_device = True
    qrep = _replica(quiet)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        qrep.engine_for(torch.device("cuda", 0))
        qrep.engine_for(torch.device("cuda", 1))
        quiet.engine_for(torch.device("cuda", 2))


def test_fallback_decision_is_shared_and_warns_once(stub):
    """Two replicas' threads read a range flag at the same time: one warning, one fallback signature, both counted."""
    net = _net("auto")
    dev = torch.device("cuda", 0)
    reps = [_replica(net) for _ in range(2)]
    net.engine_for(dev).flags = _lib.RANGE_ACT
    barrier = threading.Barrier(2, timeout=JOIN)
    ran = []

    def call(rep):
        def go():
            barrier.wait()
            rep._guarded(lambda fb: rep.engine_for(dev, fb), lambda eng: ran.append(eng.precision), "stub call")
        return go

    with warnings.catch_warnings(record=True) as wlog:
        warnings.simplefilter("always")
        _run(call(reps[0]), call(reps[1]))
        reps[0]._guarded(lambda fb: reps[0].engine_for(dev, fb), lambda eng: ran.append(eng.precision), "later call")
    fired = [w for w in wlog if "range guard fired" in str(w.message)]
    assert len(fired) == 1
    g = net._guard
    assert g["fallback"] == reps[0]._src_sig and reps[1]._on_fallback()
    assert ran[-1] == "fp32" and 1 <= g["flagged"] <= 2 and g["flagged"] == g["reruns"]     # (the second thread may already start on fp32)
    assert len(stub.built) == 2                 # the F16X3 engine and ONE fp32 engine


def test_guard_counters_under_contention_and_guard_copies(stub):
    net = _net()
    dev = torch.device("cuda", 0)
    net.engine_for(dev)
    n = 300
    barrier = threading.Barrier(2, timeout=JOIN)

    def many():
        barrier.wait()
        for _ in range(n):
            net._guarded(lambda fb: net.engine_for(dev, fb), lambda eng: None, "call")
    _run(many, many)
    assert net._guard["posted"] == 2 * n and len(stub.built[0].posts) == 2 * n and stub.built[0].loads == 1
    g2 = copy.deepcopy(net._guard)
    g3 = pickle.loads(pickle.dumps(net._guard))
    assert dict(g2) == dict(g3) == dict(net._guard) and g2.lock is not net._guard.lock and g3.mine.deferred is None


# ---------------------------------------------------------------------------------------- the C ABI itself (host-only engines)
def test_deep_stages_is_a_field_of_the_engine():
    """ "deep_stages" on an engine is that engine's own setting; with a NULL engine it is the process-wide default, which only engines
    without a value of their own follow (include/d3d.h, version 133)."""
    L = _lib.lib()
    assert L.d3d_version() >= 133
    a, b = (create_host_engine("f16x3", num_frame=27, embed_dim=512, depth=2) for _ in range(2))
    try:
        assert engine_info(L, a, "deep_stages") == (0, 1) and engine_info(L, b, "deep_stages") == (0, 1)            # the default stays
        assert L.d3d_engine_set_option(a, b"deep_stages", 0) == 0
        assert engine_info(L, a, "deep_stages") == (0, 0) and engine_info(L, b, "deep_stages") == (0, 1)            # ... and no longer leaks to another engine
        assert L.d3d_engine_set_option(None, b"deep_stages", 0) == 0
        assert engine_info(L, b, "deep_stages") == (0, 0)                                                 # b follows the process default
        assert L.d3d_engine_set_option(a, b"deep_stages", 1) == 0
        assert engine_info(L, a, "deep_stages") == (0, 1) and engine_info(L, b, "deep_stages") == (0, 0)
    finally:
        assert L.d3d_engine_set_option(None, b"deep_stages", 1) == 0
        L.d3d_engine_destroy(a)
        L.d3d_engine_destroy(b)
    assert L.d3d_engine_set_option(None, b"latency_mode", 1) != 0                              # still the only key a NULL engine takes


def test_distinct_engines_from_distinct_threads_at_the_abi():
    """Two threads, an engine each: create, options, info, weights tables and failing calls interleave freely (ctypes releases the
    GIL in every call); d3d_last_error() is the calling thread's own message."""
    L = _lib.lib()
    barrier = threading.Barrier(2, timeout=JOIN)
    seen = [[], []]

    def worker(i):
        def go():
            barrier.wait()
            for k in range(50):
                h = create_host_engine("f16x3", num_frame=27, embed_dim=512, depth=2)
                try:
                    assert L.d3d_engine_set_option(h, b"deep_stages", (i + k) & 1) == 0
                    assert L.d3d_engine_set_option(h, b"latency_mode", i) == 0
                    assert L.d3d_engine_set_option(h, f"no_such_key_{i}".encode(), 1) != 0
                    seen[i].append(L.d3d_last_error().decode())
                    assert engine_info(L, h, "deep_stages") == (0, (i + k) & 1) and engine_info(L, h, "latency_mode") == (0, i)
                    assert L.d3d_engine_num_weights(h) > 0 and L.d3d_workspace_bytes(h, 1 + i) > 0
                finally:
                    L.d3d_engine_destroy(h)
        return go
    _run(worker(0), worker(1))
    for i in range(2):
        assert len(seen[i]) == 50 and all(f"no_such_key_{i}" in m for m in seen[i]), seen[i][:3]
