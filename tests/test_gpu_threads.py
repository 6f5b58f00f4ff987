"""Concurrent host threads on ONE device (include/d3d.h "Threads"; nets.py _Guard; engine.py Engine.lock): what nn.DataParallel's
parallel_apply (RUN:216-218), a thread pool or a server does to this library -- two engines driven at once, replicas that share guard
state, one engine reached from two threads.  One device is where two threads can collide at all; the multi-device run itself is not
claimed here.  F16X3 through precision "auto", synthetic weights, depth 2, D = 512, 8 heads, J = 17, S = 3 DDIM steps, at the two
fused-temporal tile forms: T = 27 (grouped joints) and T = 243 (one joint per tile).  Every result is compared bit for bit with the
same model's serial result.  At most two extra threads; every join carries a time limit, and a thread that misses it ends the session
(nothing more is started on the GPU)."""
import threading
import warnings

import pytest
import torch

from diff3dhpe_amd.spec import DenoiserConfig
from helpers import build_product, dev, xy

pytestmark = pytest.mark.gpu

JOIN = 30.0
S = 3
ITERS = 20
SHAPES = [(27, 3), (243, 1)]


def _product(T, seed, precision="auto"):   # this module's model: D = 512, depth 2, S sampling steps, the default precision
    return build_product(DenoiserConfig(num_frame=T, embed_dim=512, depth=2), seed, sampling=S, precision=precision)


def _sample(diff, x2d, nz):   # through the diffusion object's forward(), which is what the threads call
    return diff(clean_3d_pose=torch.zeros_like(nz), noisy_2d_pose=x2d, output_loss=False, init_noise=nz)[1]


def _run(*targets):
    """One thread per target (at most two), joined with a time limit; a thread's exception is re-raised here."""
    assert len(targets) <= 2
    errs = []

    def wrap(fn):
        def go():
            try:
                fn()
            except BaseException as e:      # noqa: BLE001  (re-raised below)
                errs.append(e)
        return go
    ts = [threading.Thread(target=wrap(fn), daemon=True) for fn in targets]
    for t in ts:
        t.start()
    for t in ts:
        t.join(JOIN)
        if t.is_alive():
            pytest.exit("a worker thread did not return within its time limit: nothing more is started on the GPU", returncode=1)
    if errs:
        raise errs[0]


@pytest.mark.parametrize("T,B", SHAPES)
def test_lock_is_held_during_a_call(T, B):
    """While another thread holds the engine's lock a call on that engine does not start; released, it runs and gives the serial bits."""
    net, _ = _product(T, 5)
    x2d, nz = xy(B, T, 31)
    xcat = torch.cat([x2d, nz], dim=-1)
    t = torch.arange(B, device="cuda") * 300 + 7
    serial = net.forward_denoise(xcat, t)
    eng = net.engine_for(dev())
    assert isinstance(eng.lock, type(threading.RLock()))
    out, done = {}, threading.Event()

    def worker():
        out["y"] = net.forward_denoise(xcat, t)
        done.set()

    th = threading.Thread(target=worker, daemon=True)
    with eng.lock:
        th.start()
        returned_early = done.wait(0.5)
    th.join(JOIN)
    if th.is_alive():
        pytest.exit("the worker did not return after the lock was released: nothing more is started on the GPU", returncode=1)
    assert not returned_early
    assert torch.equal(out["y"], serial)
    assert net._guard["posted"] == 2 and net._guard["flagged"] == 0


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "hipgraph"])
@pytest.mark.parametrize("T,B", SHAPES)
def test_two_models_two_threads(T, B, graph):
    """Each thread owns a model and its engine (different weights): 20 samplings each, side by side, every one the serial bits."""
    prods = [_product(T, seed) for seed in (5, 6)]
    data = [xy(B, T, seed) for seed in (41, 42)]
    engs = [net.engine_for(dev()) for net, _ in prods]
    assert engs[0] is not engs[1]
    serial = [_sample(diff, *xn).clone() for (_, diff), xn in zip(prods, data)]      # eager, one thread
    assert not torch.equal(serial[0], serial[1])
    outs = [[], []]
    start = threading.Barrier(2, timeout=JOIN)

    def worker(i):
        def go():
            start.wait()
            for _ in range(ITERS):
                outs[i].append(_sample(prods[i][1], *data[i]))
        return go

    for eng in engs:
        eng.set_graph_mode(graph)
    try:
        _run(worker(0), worker(1))
    finally:
        for eng in engs:
            eng.set_graph_mode(False)
    torch.cuda.synchronize()
    for i in range(2):
        assert len(outs[i]) == ITERS
        bad = [k for k, y in enumerate(outs[i]) if not torch.equal(y, serial[i])]
        assert not bad, (i, bad)
        assert prods[i][0]._guard["posted"] == 1 + ITERS and prods[i][0]._guard["flagged"] == 0
    if graph:
        assert all(eng.info("graphs_captured") >= 1 for eng in engs)


@pytest.mark.parametrize("T", [27, 243])
def test_one_model_two_replicas_two_threads(T):
    """What parallel_apply runs: two replicas of one module (torch.nn.parallel.replicate -> _replicate_for_data_parallel), one thread
    each, each sampling its half of a batch of 4 -- ONE engine, one upload, calls serialised by its lock; the halves put together are
    the serial full-batch bits (a row does not depend on the batch it is computed in), and every guarded call posted one ticket."""
    net, diff = _product(T, 7)
    x2d, nz = xy(4, T, 51)
    serial = _sample(diff, x2d, nz).clone()
    idx = torch.cuda.current_device()
    reps = [torch.nn.parallel.replicate(diff, [idx])[0] for _ in range(2)]
    assert all(r.model._src_sig is not None and r.model._guard is net._guard and r.model._engines is net._engines for r in reps)
    halves = [slice(0, 2), slice(2, 4)]
    outs = [[], []]
    start = threading.Barrier(2, timeout=JOIN)

    def worker(i):
        def go():
            start.wait()
            for _ in range(ITERS):
                outs[i].append(_sample(reps[i], x2d[halves[i]].contiguous(), nz[halves[i]].contiguous()))
        return go

    with warnings.catch_warnings(record=True) as wlog:
        warnings.simplefilter("always")
        _run(worker(0), worker(1))
    assert not [str(w.message) for w in wlog if "diff3dhpe_amd" in str(w.message)]      # one device: nothing to warn about
    torch.cuda.synchronize()
    for k in range(ITERS):
        assert torch.equal(torch.cat([outs[0][k], outs[1][k]], dim=0), serial), k
    g = net._guard
    assert g["posted"] == 1 + 2 * ITERS and g["flagged"] == 0 and g["reruns"] == 0
    assert list(net._engines) == [idx] and not net._engines_fb


def test_one_engine_two_threads_on_two_streams():
    """A thread pool with a stream per worker on ONE model: the lock orders the host calls, and a call that arrives on another stream
    than the previous one waits for that stream first -- the one workspace is never written by two calls at once."""
    T, B = 27, 3
    net, _ = _product(T, 8)
    t = torch.arange(B, device="cuda") * 250 + 3
    xs = [torch.cat(xy(B, T, seed), dim=-1) for seed in (61, 62)]
    serial = [net.forward_denoise(x, t).clone() for x in xs]
    assert not torch.equal(serial[0], serial[1])
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [[], []]
    start = threading.Barrier(2, timeout=JOIN)

    def worker(i):
        def go():
            with torch.cuda.stream(streams[i]):
                start.wait()
                for _ in range(ITERS):
                    outs[i].append(net.forward_denoise(xs[i], t))
                streams[i].synchronize()
        return go

    _run(worker(0), worker(1))
    torch.cuda.synchronize()
    for i in range(2):
        bad = [k for k, y in enumerate(outs[i]) if not torch.equal(y, serial[i])]
        assert not bad, (i, bad)
    assert len(net._engines) == 1 and net._guard["posted"] == 2 + 2 * ITERS


@pytest.mark.parametrize("T,B", SHAPES)
def test_deferred_block_beside_a_plain_call(T, B):
    """deferred_range_checks() open in this thread; a guarded call made meanwhile by another thread is read at once and never lands in
    this thread's box; this thread's own call does."""
    net, diff = _product(T, 9)
    x2d, nz = xy(B, T, 71)
    serial = _sample(diff, x2d, nz).clone()
    eng = net.engine_for(dev())
    takes = []
    real_take = eng.take_range

    def take(ticket, block=True):
        takes.append((threading.get_ident(), block))
        return real_take(ticket, block)
    eng.take_range = take
    out = {}

    def worker():
        out["tid"] = threading.get_ident()
        out["y"] = _sample(diff, x2d, nz)

    with net.deferred_range_checks() as box:
        _run(worker)
        assert box.items == []
        assert takes == [(out["tid"], True)]
        mine = _sample(diff, x2d, nz)
        assert len(box.items) == 1 and len(takes) == 1
        assert box.resolve() is False
    assert torch.equal(out["y"], serial) and torch.equal(mine, serial)
    assert net._guard["posted"] == 3 and net._guard["flagged"] == 0


def test_fallback_decision_is_shared():
    """precision "auto": a call of one replica's thread leaves the F16X3 range (input scaled past |x| = 8188) -- repeated on the fp32
    engine, ONE warning; the other replica's thread then runs its next call on the fp32 engine directly."""
    T, B = 27, 3
    net, _ = _product(T, 10)
    net32, _ = _product(T, 10, precision="fp32")
    x2d, nz = xy(B, T, 81)
    xcat = torch.cat([x2d, nz], dim=-1)
    t = torch.arange(B, device="cuda") * 300 + 11
    want = net32.forward_denoise(xcat, t).clone()
    big = torch.cat([x2d * 1.0e6, nz], dim=-1)
    want_big = net32.forward_denoise(big, t).clone()
    idx = torch.cuda.current_device()
    reps = [torch.nn.parallel.replicate(net, [idx])[0] for _ in range(2)]
    tripped = threading.Event()
    out = {}

    def first():
        try:
            out["big"] = reps[0].forward_denoise(big, t)
        finally:
            tripped.set()

    def second():
        assert tripped.wait(JOIN)
        out["on_fallback"] = reps[1]._on_fallback()
        out["y"] = reps[1].forward_denoise(xcat, t)

    with warnings.catch_warnings(record=True) as wlog:
        warnings.simplefilter("always")
        _run(first, second)
    ours = [w for w in wlog if issubclass(w.category, RuntimeWarning)]
    assert len(ours) == 1 and "range guard fired" in str(ours[0].message), [str(w.message) for w in wlog]
    g = net._guard
    assert g["flagged"] == 1 and g["reruns"] == 1 and out["on_fallback"] and net._on_fallback()
    assert list(net._engines_fb) == [idx]
    assert torch.equal(out["big"], want_big)                   # the flagged call itself: repeated on the fp32 engine
    assert torch.equal(out["y"], want)                         # the other thread: the fp32 engine directly
    reps[1].flush_range_checks()                               # (the calling thread's own lazy tickets: none here, nothing raised)
    assert g["posted"] == 2
