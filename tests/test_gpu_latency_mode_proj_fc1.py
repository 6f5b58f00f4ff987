"""proj and fc1 of the opt-in "latency_mode" on the MI355X: the split-K x split-N GEMM plus the ordered reduce kernels k_splitk_residual /
k_splitk_gelu (include/d3d.h "proj_split" / "fc1_split").  Op-level accuracy against fp64, golden parity at the project's gate,
determinism inside the mode, no leakage into the default path, range guard, switching the options between calls."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import diff3dhpe_amd as d3d
from conftest import gold
from helpers import hashed, torch_sd, maxabs, inputs, cfg_full, build_product, _tol
from helpers import dev as _dev          # tests here hold the device in a local named dev
from diff3dhpe_amd.spec import DenoiserConfig

pytestmark = pytest.mark.gpu

GATE = 1e-4


def _force(eng, proj, fc1):
    eng.set_option("proj_split", proj)
    eng.set_option("fc1_split", fc1)


def _splits(eng):
    return eng.info("proj_split_last"), eng.info("fc1_split_last")


# ---------------------------------------------------------------------------------------------------------------- 1. op level
# (the bounds: helpers._tol)
@pytest.mark.parametrize("M", [130, 459, 1377])
@pytest.mark.parametrize("S", [2, 4])
def test_splitk_residual_matches_fp64(S, M):
    from diff3dhpe_amd import engine as E
    N, K = 512, 512
    A = hashed(f"skA{M}", (M, K), 21, 2.0).cuda()
    W = hashed(f"skW{K}", (N, K), 22, 1.0 / np.sqrt(K)).cuda()
    b = hashed("skb", (N,), 23, 0.5).cuda()
    R = (hashed(f"skR{M}", (M, N), 24, 1.5) + 0.3).cuda()
    ref = R.double() + A.double() @ W.double().t() + b.double()
    x, st, _ = E.op_linear_splitk_residual(A, W, b, R, S=S, with_stats=True)
    e = maxabs(x, ref.cpu())
    blocks = ref.view(M, N // 64, 64)
    es, eq = maxabs(st[:, :, 0], blocks.sum(2).cpu()), maxabs(st[:, :, 1], (blocks * blocks).sum(2).cpu())
    x0, _, _ = E.op_linear_splitk_residual(A, W, b, R, S=0)
    print(f"splitk residual S={S} M={M}: planes {e:.3e} (tol {_tol(K) + 2e-6:.3e}); stats {es:.3e} {eq:.3e}; "
          f"default kernel {maxabs(x0, ref.cpu()):.3e}, split vs default {maxabs(x, x0.cpu()):.3e}")
    assert e < _tol(K) + 2e-6
    assert es < 2e-3 and eq < 1e-2
    # a row depends on S alone: bit-equal in the full matrix and in a slice of it, and from one call to the next
    lo, hi = (100, 229) if M > 229 else (31, M)
    part, pst, _ = E.op_linear_splitk_residual(A[lo:hi].contiguous(), W, b, R[lo:hi].contiguous(), S=S, with_stats=True)
    assert torch.equal(part, x[lo:hi]) and torch.equal(pst, st[lo:hi])
    again, ast, _ = E.op_linear_splitk_residual(A, W, b, R, S=S, with_stats=True)
    assert torch.equal(again, x) and torch.equal(ast, st)


@pytest.mark.parametrize("M", [130, 459, 1377])
@pytest.mark.parametrize("S", [2, 4])
def test_splitk_gelu_matches_fp64(S, M):
    from diff3dhpe_amd import engine as E
    N, K = 1024, 512
    X = hashed(f"skA{M}", (M, K), 21, 2.0).cuda()
    W = hashed(f"skW1{K}", (N, K), 22, 1.0 / np.sqrt(K)).cuda()
    b = hashed("skb1", (N,), 23, 0.5).cuda()
    g = (1 + 0.2 * hashed("skg", (K,), 25)).cuda()
    be = (0.2 * hashed("skbe", (K,), 26)).cuda()
    ref = F.gelu(F.layer_norm(X.double(), (K,), g.double(), be.double(), 1e-6) @ W.double().t() + b.double())
    h, _ = E.op_linear_splitk_gelu(X, W, b, g, be, 1e-6, S=S)
    e = maxabs(h, ref.cpu())
    h0, _ = E.op_linear_splitk_gelu(X, W, b, g, be, 1e-6, S=0)
    print(f"splitk gelu S={S} M={M}: planes {e:.3e} (tol {_tol(K) + 2e-6:.3e}); default kernel {maxabs(h0, ref.cpu()):.3e}, "
          f"split vs default {maxabs(h, h0.cpu()):.3e}")
    assert e < _tol(K) + 2e-6
    lo, hi = (100, 229) if M > 229 else (31, M)
    part, _ = E.op_linear_splitk_gelu(X[lo:hi].contiguous(), W, b, g, be, 1e-6, S=S)
    assert torch.equal(part, h[lo:hi])
    again, _ = E.op_linear_splitk_gelu(X, W, b, g, be, 1e-6, S=S)
    assert torch.equal(again, h)


def test_op_hooks_reject_other_shapes():
    from diff3dhpe_amd import engine as E
    z = lambda *s: torch.zeros(*s).cuda()
    with pytest.raises(d3d.D3DError):
        E.op_linear_splitk_residual(z(64, 512), z(512, 512), z(512), z(64, 512), S=3)
    with pytest.raises(d3d.D3DError):
        E.op_linear_splitk_residual(z(64, 128), z(512, 128), z(512), z(64, 512), S=2)          # 4 k-tiles / 2 < 4
    with pytest.raises(d3d.D3DError):
        E.op_linear_splitk_gelu(z(64, 512), z(1024, 512), z(1024), z(512), z(512), S=8)
    with pytest.raises(d3d.D3DError):
        E.op_linear_splitk_gelu(z(64, 512), z(256, 512), z(256), z(512), z(512), S=2)          # width outside the predicate


# ------------------------------------------------------------------------------------------------------------ 2. golden parity
_NETS = {}


def _product(tag, cfg, seed, sampling):   # cached per golden tag: the mode-on and mode-off tests of one golden share a product
    """One latency-mode product per fixture, shared by the three S settings."""
    key = (tag, sampling)
    if key not in _NETS:
        net, diff = build_product(cfg, seed, sampling=sampling, precision="f16x3")
        net.latency_mode = True
        _NETS[key] = (net, diff)
    return _NETS[key]


MODES = [("forced2", 2), ("forced4", 4), ("rule", -1)]


@pytest.mark.parametrize("mode,S", MODES, ids=[m for m, _ in MODES])
@pytest.mark.parametrize("tag,cfg", [("s2f_T27", cfg_full(27, seq2frame=True)), ("full_T81", cfg_full(81))], ids=["s2f_T27", "full_T81"])
def test_golden_parity_denoise(tag, cfg, mode, S):
    """forward_denoise of the fixture's sequences, one at a time (B = 1), option on: <= 1e-4 against the fixture."""
    g = gold("denoise_" + tag)
    B = int(g["B"])
    net, _ = _product("denoise_" + tag, cfg, int(g["seed"]), 9)
    eng = net.engine_for(_dev())
    _force(eng, S, S)
    inp = inputs(B, cfg.num_frame, int(g["input_seed"]))
    xcat = torch.cat([inp["x2d"], inp["noise"] * float(g["y_scale"])], dim=-1).cuda()
    cases = [(f"t{t}", torch.full((B,), t, dtype=torch.long, device="cuda")) for t in (999, 443, 0)]
    cases.append(("tmixed", torch.from_numpy(g["tmixed_t"]).long().cuda()))
    worst, seen = 0.0, set()
    for key, t in cases:
        for i in range(B):
            o1 = net.forward_denoise(xcat[i:i + 1].contiguous(), t[i:i + 1].contiguous())
            seen.add(_splits(eng))
            if S >= 0:
                assert _splits(eng) == (S, S), (tag, key, i)
            worst = max(worst, maxabs(o1, g[key][i:i + 1]))
    print(f"denoise {tag} [latency_mode, {mode}]: max-abs {worst:.3e}; (proj, fc1) split = {sorted(seen)}, fc2 {eng.info('fc2_split_last')}")
    assert len(seen) == 1 and all(s in (0, 2, 4) for s in next(iter(seen)))
    assert worst <= GATE


@pytest.mark.parametrize("mode,S", MODES, ids=[m for m, _ in MODES])
@pytest.mark.parametrize("tag,cfg,traj", [("s2f_T27_S9", cfg_full(27, seq2frame=True), True), ("full_T81_S9", cfg_full(81), False)],
                         ids=["s2f_T27_S9", "full_T81_S9"])
def test_golden_parity_ddim(tag, cfg, traj, mode, S):
    """The 9-step DDIM loop of the fixture, one sequence at a time (B = 1), option on: <= 1e-4 against the fixture."""
    g = gold("ddim_" + tag)
    B, steps = int(g["B"]), int(g["S"])
    net, diff = _product("ddim_" + tag, cfg, int(g["seed"]), steps)
    eng = net.engine_for(_dev())
    _force(eng, S, S)
    inp = inputs(B, cfg.num_frame, int(g["input_seed"]))
    noise = inp["noise"][:, :1].contiguous() if cfg.seq2frame else inp["noise"]
    worst, seen = 0.0, set()
    keys = ("y0", "x_reverse_diffusion", "x_start_est") if traj else ("y0",)
    for i in range(B):
        nz, x2d = noise[i:i + 1].contiguous().cuda(), inp["x2d"][i:i + 1].contiguous().cuda()
        clean = torch.zeros_like(nz)
        if traj:
            res = diff(clean, x2d, None, True, False, init_noise=nz)[1:]
        else:
            res = diff(clean_3d_pose=clean, noisy_2d_pose=x2d, output_loss=False, init_noise=nz)[1:]
        seen.add(_splits(eng))
        if S >= 0:
            assert _splits(eng) == (S, S), (tag, i)
        worst = max(worst, max(maxabs(r, g[k][i:i + 1]) for r, k in zip(res, keys)))
    print(f"ddim {tag} [latency_mode, {mode}]: max-abs {worst:.3e}; (proj, fc1) split = {sorted(seen)}, fc2 {eng.info('fc2_split_last')}")
    assert len(seen) == 1 and all(s in (0, 2, 4) for s in next(iter(seen)))
    assert worst <= GATE


# ------------------------------------------------------------------------------------------- 3.-6.: one D = 512 model per module
T27 = DenoiserConfig(num_frame=27, embed_dim=512, depth=2)


@pytest.fixture(scope="module")
def pair27():
    """(latency-mode product, default product) with the same seeded weights; T = 27, width 512, 2 x 2 blocks."""
    on = build_product(T27, 41, sampling=3, precision="f16x3")
    on[0].latency_mode = True
    off = build_product(T27, 41, sampling=3, precision="f16x3")
    return on, off


def _xcat(B, T, seed):
    inp = inputs(B, T, seed)
    return torch.cat([inp["x2d"], inp["noise"]], dim=-1).cuda()


def _sample(diff, x2d, nz):   # through the diffusion object's forward()
    return diff(clean_3d_pose=torch.zeros_like(nz), noisy_2d_pose=x2d, output_loss=False, init_noise=nz)[1]


@pytest.mark.parametrize("S", [2, 4])
def test_determinism_inside_the_mode(pair27, S):
    (net, diff), _ = pair27
    eng = net.engine_for(_dev())
    _force(eng, S, S)
    try:
        x3 = _xcat(3, 27, 81)
        t3 = torch.tensor([700, 30, 999], device="cuda")
        a, b = net.forward_denoise(x3, t3), net.forward_denoise(x3, t3)
        s3 = _splits(eng) + (eng.info("fc2_split_last"),)
        assert s3[:2] == (S, S) and torch.equal(a, b)                                          # two runs of one call
        one = net.forward_denoise(x3[:1].contiguous(), t3[:1].contiguous())
        s1 = _splits(eng) + (eng.info("fc2_split_last"),)
        assert s1[:2] == (S, S)
        if s1 == s3:   # (fc2's own rule decides its S: equal at 256 CUs)
            assert torch.equal(one, a[:1]), f"sequence 0 alone vs row 0 of B = 3, splits {s1}"
        else:
            assert maxabs(one, a[:1].cpu()) <= GATE
        inp = inputs(1, 27, 82)
        x2d, nz = inp["x2d"].cuda(), inp["noise"].cuda()
        eng.set_graph_mode(False)
        eager = _sample(diff, x2d, nz)
        assert _splits(eng) == (S, S)
        eng.set_graph_mode(True)
        try:
            for rep in range(3):
                assert torch.equal(_sample(diff, x2d, nz), eager), rep                         # eager launches vs hipGraph replay
                assert _splits(eng) == (S, S)
            # a sampling of three sequences runs as two half-batches on two streams, each with its own partials
            inp3 = inputs(3, 27, 83)
            y3 = _sample(diff, inp3["x2d"].cuda(), inp3["noise"].cuda())
            y1 = _sample(diff, inp3["x2d"][2:3].contiguous().cuda(), inp3["noise"][2:3].contiguous().cuda())
            assert torch.equal(y3, _sample(diff, inp3["x2d"].cuda(), inp3["noise"].cuda()))
            assert torch.equal(y1, y3[2:3]) or s1 != s3
        finally:
            eng.set_graph_mode(False)
    finally:
        _force(eng, -1, -1)


def test_no_leakage_into_the_default_path(pair27):
    (net, diff), (ref_net, ref_diff) = pair27
    dev = _dev()
    inp = inputs(1, 27, 84)
    x2d, nz = inp["x2d"].cuda(), inp["noise"].cuda()
    want = _sample(ref_diff, x2d, nz)
    ref_eng = ref_net.engine_for(dev)
    assert ref_eng.info("latency_mode") == 0 and _splits(ref_eng) == (0, 0)
    eng = net.engine_for(dev)
    try:
        # the option keys alone change nothing: they are read only while the mode is on
        net.latency_mode = False
        net.engine_for(dev)
        _force(eng, 4, 4)
        off = _sample(diff, x2d, nz)
        assert eng.info("latency_mode") == 0 and _splits(eng) == (0, 0) and eng.info("fc2_split_last") == 0
        assert torch.equal(off, want)
        xc = _xcat(1, 27, 85)
        t = torch.tensor([500], device="cuda")
        assert torch.equal(net.forward_denoise(xc, t), ref_net.forward_denoise(xc, t)) and _splits(eng) == (0, 0)
        # the mode on with the split forced, then off again: the default bits come back
        net.latency_mode = True
        on = _sample(diff, x2d, nz)
        assert _splits(eng) == (4, 4) and maxabs(on, want.cpu()) <= GATE
        net.latency_mode = False
        assert torch.equal(_sample(diff, x2d, nz), want) and _splits(eng) == (0, 0)
    finally:
        net.latency_mode = True
        net.engine_for(dev)
        _force(eng, -1, -1)


def test_large_call_keeps_the_default_kernels():
    cfg = DenoiserConfig(num_frame=27, embed_dim=512, depth=1)
    net, _ = build_product(cfg, 43, precision="f16x3")
    ref_net, _ = build_product(cfg, 43, precision="f16x3")
    net.latency_mode = True
    x = _xcat(64, 27, 86)
    t = torch.full((64,), 500, dtype=torch.long, device="cuda")
    out = net.forward_denoise(x, t)
    eng = net.engine_for(_dev())
    assert eng.info("latency_mode") == 1 and _splits(eng) == (0, 0) and eng.info("fc2_split_last") == 0
    assert torch.equal(out, ref_net.forward_denoise(x, t))


@pytest.mark.parametrize("S", [2, 4])
def test_nan_filled_workspace_gives_the_same_bits(pair27, S):
    (net, diff), _ = pair27
    eng = net.engine_for(_dev())
    _force(eng, S, S)
    try:
        xc = _xcat(1, 27, 87)
        t = torch.tensor([321], device="cuda")
        eng._workspace(1).zero_()
        a = net.forward_denoise(xc, t)
        eng._workspace(1).view(torch.float32).fill_(float("nan"))
        b = net.forward_denoise(xc, t)
        assert _splits(eng) == (S, S)
        assert torch.isfinite(b).all() and torch.equal(a, b)
    finally:
        _force(eng, -1, -1)


def _big_proj_bias(sd):
    sd["STEblocks.0.attn.proj.bias"] += 1.0e4      # large and finite: the proj output of block 0 passes |x| = 8188


def _range_model(precision, latency):
    cfg = DenoiserConfig(num_frame=27, embed_dim=512, depth=1)
    sd = torch_sd(cfg, 8)
    _big_proj_bias(sd)
    net = d3d.HPE_model(d3d.S2S_NAME)(num_frame=27, embed_dim=512, depth=1)
    net.load_state_dict(sd)
    net.precision = precision
    net.latency_mode = latency
    return net.cuda()


def test_range_guard_through_the_proj_reduce():
    from diff3dhpe_amd import _lib
    dev = _dev()
    xc = _xcat(1, 27, 88)
    t = torch.tensor([500], device="cuda")
    net = _range_model("f16x3", True)
    net.range_check = False
    eng = net.engine_for(dev)
    _force(eng, 4, 4)
    eng.range_flags(clear=True)
    net.forward_denoise(xc, t)
    assert _splits(eng) == (4, 4)
    f = eng.range_flags()
    assert f & _lib.RANGE_ACT and not (f & _lib.RANGE_WEIGHT)
    # "auto": the flagged call is repeated on the fp32 engine, as with the default kernels
    auto = _range_model("auto", True)
    auto.engine_for(dev)
    _force(auto.engine_for(dev), 4, 4)
    with warnings.catch_warnings(record=True) as wlog:
        warnings.simplefilter("always")
        out = auto.forward_denoise(xc, t)
    assert any("range guard fired" in str(w.message) for w in wlog)
    assert auto._guard["flagged"] == 1 and auto._guard["reruns"] == 1 and auto._on_fallback()
    assert torch.equal(out, _range_model("fp32", False).forward_denoise(xc, t))


def test_switching_proj_split_between_graph_calls(pair27):
    (net, diff), _ = pair27
    eng = net.engine_for(_dev())
    inp = inputs(1, 27, 89)
    x2d, nz = inp["x2d"].cuda(), inp["noise"].cuda()
    eng.set_graph_mode(True)
    try:
        _force(eng, 2, 0)
        a = _sample(diff, x2d, nz)
        assert _splits(eng) == (2, 0) and eng.info("graphs_cached") >= 1
        eng.set_option("proj_split", 4)
        assert eng.info("graphs_cached") == 0                                   # the change dropped the captured graphs
        b = _sample(diff, x2d, nz)
        assert _splits(eng) == (4, 0)
        eng.set_option("proj_split", 0)
        c = _sample(diff, x2d, nz)
        assert _splits(eng) == (0, 0)
        assert maxabs(a, b.cpu()) <= GATE and maxabs(a, c.cpu()) <= GATE
        eng.set_option("proj_split", 2)
        assert torch.equal(_sample(diff, x2d, nz), a)
    finally:
        eng.set_graph_mode(False)
        _force(eng, -1, -1)
