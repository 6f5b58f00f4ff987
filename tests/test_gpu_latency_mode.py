"""The opt-in "latency_mode" of the F16X3 engine on the MI355X: fc2 + post-norm of a small call as a split-K x split-N GEMM plus an
ordered reduce / post-norm row kernel (include/d3d.h).  Op-level accuracy against fp64, golden parity at the project's gate, determinism
inside the mode, no leakage into the default path, large calls untouched, range guard alive."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import diff3dhpe_amd as d3d
from conftest import gold
from helpers import hashed, torch_sd, maxabs, inputs, cfg_small, cfg_full, build_product, cu_count
from helpers import dev as _dev          # tests here hold the device in a local named dev
from diff3dhpe_amd.spec import DenoiserConfig

pytestmark = pytest.mark.gpu

GATE = 1e-4


def policy_split(M, D, Dm, n_cu):
    """The rule of include/d3d.h / d3d_kernels.h (fc2_splitk_choose), restated: S in {2, 4}, or 0 where the default kernel runs."""
    if D != 512 or Dm % 32 or (M + 63) // 64 >= n_cu:
        return 0
    nk, tiles = Dm // 32, ((M + 127) // 128) * (D // 128)
    best, best_cost = 0, None
    for S in (1, 2, 4):
        if nk % S or nk // S < 4:
            continue
        W = tiles * S
        if W > 2 * n_cu:
            continue
        cost = (nk // S) * (1.0 if W <= n_cu else 1.45)
        if best_cost is None or cost < best_cost:
            best, best_cost = S, cost
    return best if best >= 2 else 0


def test_policy_examples_of_the_rule():
    """The worked examples of the rule at 256 CUs (no device arithmetic: the restatement above must be the rule the tests below rely on)."""
    assert policy_split(4131, 512, 1024, 256) == 2      # B = 1, T = 243: 132 tiles, 264 workgroups, 23.2 against 32
    assert policy_split(1377, 512, 1024, 256) == 4      # T = 81
    assert policy_split(2754, 512, 1024, 256) == 4      # T = 81, B = 2
    assert policy_split(8262, 512, 1024, 256) == 0      # B = 2, T = 243: S = 1, the mode stays off
    assert policy_split(64 * 243 * 17, 512, 1024, 256) == 0
    assert policy_split(1377, 32, 64, 256) == 0         # no fused post-norm tile at this width


# ---------------------------------------------------------------------------------------------------------------- 1. op level
@pytest.mark.parametrize("mode", ["plain", "all"])
@pytest.mark.parametrize("M", [4131, 1377, 459, 130])
@pytest.mark.parametrize("S", [2, 4])
def test_splitk_postnorm_matches_fp64(S, M, mode):
    """The kernel pair alone against fp64 math, built the way test_linear_postnorm_matches_fp64 builds its reference, with that test's
    bounds: 3e-6 sqrt(K/32) + 2e-6 for the fp32 output, 2e-6 more for the planes (22 bits of y), 2e-3 / 1e-2 for the row statistics.
    A row must come out bit-equal in the full matrix and in a slice of it (fixed S)."""
    from diff3dhpe_amd import engine as E
    N, K = 512, 1024
    A = hashed(f"skA{M}", (M, K), 21, 2.0).cuda()
    W = hashed(f"skW{K}", (N, K), 22, 1.0 / np.sqrt(K)).cuda()
    b = hashed("skb", (N,), 23, 0.5).cuda()
    R = (hashed(f"skR{M}", (M, N), 24, 1.5) + 0.3).cuda()
    g = (1 + 0.2 * hashed("skg", (N,), 25)).cuda()
    be = (0.2 * hashed("skbe", (N,), 26)).cuda()
    rows = torch.arange(M, device="cuda")
    kw, add = {}, torch.zeros((M, N), dtype=torch.float64, device="cuda")
    if mode == "all":
        pos = hashed("skpos", (9, N), 27, 0.5).cuda()
        rpb = 51
        tv = hashed("sktvr", ((M + rpb - 1) // rpb, N), 29, 0.5).cuda()
        kw.update(pos=pos, pos_div=17, tvec=tv, rows_per_batch=rpb)
        add += pos.double()[(rows // 17) % 9] + tv.double()[rows // rpb]
    ref = F.layer_norm(R.double() + A.double() @ W.double().t() + b.double(), (N,), g.double(), be.double(), 1e-6) + add
    tol = 3e-6 * np.sqrt(K / 32) + 2e-6
    y32, _, _ = E.op_linear_splitk_postnorm(A, W, b, R, g, be, 1e-6, S=S, **kw)
    e32 = maxabs(y32, ref.cpu())
    yp, st, _ = E.op_linear_splitk_postnorm(A, W, b, R, g, be, 1e-6, S=S, with_stats=True, **kw)
    ep, epp = maxabs(yp, ref.cpu()), maxabs(yp, y32.cpu())
    es, eq = maxabs(st[:, 0], ref.sum(1).cpu()), maxabs(st[:, 1], (ref * ref).sum(1).cpu())
    print(f"splitk postnorm S={S} M={M} [{mode}]: fp32 {e32:.3e} planes {ep:.3e} (vs fp32 form {epp:.3e}) stats {es:.3e} {eq:.3e}; tol {tol:.3e}")
    assert e32 < tol
    assert ep < tol + 2e-6
    assert epp < 2e-6
    assert es < 2e-3 and eq < 1e-2
    lo, hi = (100, 229) if M > 229 else (31, M)
    full0 = y32 if not kw else E.op_linear_splitk_postnorm(A, W, b, R, g, be, 1e-6, S=S)[0]
    part0, _, _ = E.op_linear_splitk_postnorm(A[lo:hi].contiguous(), W, b, R[lo:hi].contiguous(), g, be, 1e-6, S=S)
    assert torch.equal(part0, full0[lo:hi])
    again, _, _ = E.op_linear_splitk_postnorm(A, W, b, R, g, be, 1e-6, S=S, **kw)
    assert torch.equal(again, y32)


def test_splitk_postnorm_rejects_other_shapes():
    from diff3dhpe_amd import engine as E
    z = lambda *s: torch.zeros(*s).cuda()
    with pytest.raises(d3d.D3DError):
        E.op_linear_splitk_postnorm(z(64, 64), z(256, 64), z(256), z(64, 256), z(256), z(256), S=2)       # width without the tile shape
    with pytest.raises(d3d.D3DError):
        E.op_linear_splitk_postnorm(z(64, 128), z(512, 128), z(512), z(64, 512), z(512), z(512), S=3)     # S not in {2, 4}


# ------------------------------------------------------------------------------------------------------------ 2. golden parity
DENOISE = [("small_T81", cfg_small(81)), ("full_T27", cfg_full(27)), ("full_T81", cfg_full(81)),
           ("full_T243", cfg_full(243)), ("s2f_T27", cfg_full(27, seq2frame=True)),
           ("notemb_T27", cfg_full(27, with_time_emb=False)), ("small_s2f_T27", cfg_small(27, seq2frame=True))]
DDIM = [("small_T81_S5", cfg_small(81), True, True), ("full_T81_S9", cfg_full(81), False, True),
        ("full_T243_S9", cfg_full(243), False, True), ("full_T243_S50", cfg_full(243), False, True),
        ("s2f_T27_S9", cfg_full(27, seq2frame=True), True, True),
        ("full_T27_S7_notemb", cfg_full(27, with_time_emb=False), False, True),
        ("small_T81_S5_noclip", cfg_small(81), True, False)]
if not os.environ.get("D3D_SLOW_TESTS"):
    DDIM = [d for d in DDIM if d[0] != "full_T243_S50"]


def _rows(cfg, B):
    return B * cfg.num_frame * cfg.num_joints


def _expected_split(cfg, B):
    return policy_split(_rows(cfg, B), cfg.embed_dim, cfg.mlp_hidden, cu_count())


def test_golden_parity_denoise_with_the_mode_on():
    """Every denoise_* fixture of the F16X3 parity test, option on: <= 1e-4 against the fixture (the project's gate) and the split the
    rule predicts.  Each fixture runs at its own batch size AND one sequence at a time (rows of a batch are independent sequences):
    the fixtures hold two sequences, and at T = 243 only a single sequence is small enough for the rule (M = 8262 gives S = 1), so the
    per-sequence leg is what puts denoise_full_T243 through the split kernels.  Fixtures without a fused post-norm tile (width 32)
    must report 0 and stay bit-equal to the default engine."""
    split_set = set()
    for tag, cfg in DENOISE:
        g = gold("denoise_" + tag)
        B = int(g["B"])
        net, _ = build_product(cfg, int(g["seed"]), precision="f16x3")
        net.latency_mode = True
        eng = net.engine_for(_dev())
        assert eng.info("latency_mode") == 1
        inp = inputs(B, cfg.num_frame, int(g["input_seed"]))
        xcat = torch.cat([inp["x2d"], inp["noise"] * float(g["y_scale"])], dim=-1).cuda()
        cases = [(f"t{t}", torch.full((B,), t, dtype=torch.long, device="cuda")) for t in (999, 443, 0)]
        cases.append(("tmixed", torch.from_numpy(g["tmixed_t"]).long().cuda()))
        worst, outs = 0.0, {}
        for key, t in cases:
            out = net.forward_denoise(xcat, t)
            assert eng.info("fc2_split_last") == _expected_split(cfg, B), (tag, key)
            worst = max(worst, maxabs(out, g[key]))
            outs[key] = out
            for i in range(B):      # one sequence at a time
                o1 = net.forward_denoise(xcat[i:i + 1].contiguous(), t[i:i + 1].contiguous())
                assert eng.info("fc2_split_last") == _expected_split(cfg, 1), (tag, key, i)
                worst = max(worst, maxabs(o1, g[key][i:i + 1]))
        if _expected_split(cfg, B) >= 2 or _expected_split(cfg, 1) >= 2:
            split_set.add("denoise_" + tag)
        print(f"denoise {tag} [f16x3, latency_mode]: max-abs {worst:.3e}; S = {_expected_split(cfg, B)} at B = {B}, {_expected_split(cfg, 1)} at B = 1")
        assert worst <= GATE, tag
        if cfg.embed_dim != 512:
            assert _expected_split(cfg, B) == 0 and _expected_split(cfg, 1) == 0
            ref_net, _ = build_product(cfg, int(g["seed"]), precision="f16x3")
            for key, t in cases:
                assert torch.equal(ref_net.forward_denoise(xcat, t), outs[key]), (tag, key)
    assert split_set and "denoise_full_T243" in split_set, split_set


def test_golden_parity_ddim_with_the_mode_on():
    """Every ddim_* fixture of the F16X3 parity test (the 50-step one only with D3D_SLOW_TESTS), option on: <= 1e-4 against the fixture.
    A sampling of B >= 2 runs as two half-batches: the reported split is the first half's."""
    split_set = set()
    for tag, cfg, traj, clip in DDIM:
        g = gold("ddim_" + tag)
        B, S = int(g["B"]), int(g["S"])
        net, diff = build_product(cfg, int(g["seed"]), sampling=S, clip=clip, precision="f16x3")
        net.latency_mode = True
        inp = inputs(B, cfg.num_frame, int(g["input_seed"]))
        noise = inp["noise"][:, :1].contiguous() if cfg.seq2frame else inp["noise"]
        clean, x2d = torch.zeros_like(noise).cuda(), inp["x2d"].cuda()

        def run(d):
            if traj:
                _, y0, rev, x0s = d(clean, x2d, None, True, False, init_noise=noise.cuda())
                return y0, rev, x0s
            return d(clean_3d_pose=clean, noisy_2d_pose=x2d, output_loss=False, init_noise=noise.cuda())[1:]
        res = run(diff)
        eng = net.engine_for(_dev())
        want = _expected_split(cfg, (B + 1) // 2 if (B >= 2 and eng.info("streams") == 2) else B)
        assert eng.info("latency_mode") == 1 and eng.info("fc2_split_last") == want, tag
        keys = ("y0", "x_reverse_diffusion", "x_start_est") if traj else ("y0",)
        e = max(maxabs(r, g[k]) for r, k in zip(res, keys))
        print(f"ddim {tag} [f16x3, latency_mode]: max-abs {e:.3e}; S = {want}")
        assert e <= GATE, tag
        if want >= 2:
            split_set.add("ddim_" + tag)
        if cfg.embed_dim != 512:
            assert want == 0
            _, ref_diff = build_product(cfg, int(g["seed"]), sampling=S, clip=clip, precision="f16x3")
            for a, b_ in zip(run(ref_diff), res):
                assert torch.equal(a, b_), tag
    assert split_set and "ddim_full_T243_S9" in split_set, split_set


# ------------------------------------------------------------------------------------------- 3.-6.: one D = 512 model per module
T81 = DenoiserConfig(num_frame=81, embed_dim=512, depth=2)


@pytest.fixture(scope="module")
def pair81():
    """(latency-mode product, default product) with the same seeded weights; T = 81, width 512, 2 x 2 blocks."""
    on = build_product(T81, 31, sampling=3, precision="f16x3")
    on[0].latency_mode = True
    off = build_product(T81, 31, sampling=3, precision="f16x3")
    return on, off


def _xcat(B, T, seed):
    inp = inputs(B, T, seed)
    return torch.cat([inp["x2d"], inp["noise"]], dim=-1).cuda()


def test_determinism_inside_the_mode(pair81):
    (net, diff), _ = pair81
    eng = net.engine_for(_dev())
    x2 = _xcat(2, 81, 71)
    t2 = torch.tensor([700, 30], device="cuda")
    a, b = net.forward_denoise(x2, t2), net.forward_denoise(x2, t2)
    s2 = eng.info("fc2_split_last")
    assert s2 >= 2 and torch.equal(a, b)                                    # two runs of one call
    one = net.forward_denoise(x2[:1].contiguous(), t2[:1].contiguous())
    s1 = eng.info("fc2_split_last")
    assert s1 >= 2
    if s1 == s2:   # (256 CUs: S = 4 at M = 1377 and at M = 2754)
        assert torch.equal(one, a[:1]), f"sequence 0 alone vs row 0 of B = 2, both S = {s1}"
    else:
        e = maxabs(one, a[:1].cpu())
        assert e <= GATE, f"S differs ({s1} alone, {s2} at B = 2): not bit-equal by design, max-abs {e:.3e} must stay inside the gate"
    # eager launches vs hipGraph replay
    inp = inputs(1, 81, 72)
    x2d, nz = inp["x2d"].cuda(), inp["noise"].cuda()
    z = torch.zeros_like(nz)
    eng.set_graph_mode(False)
    _, eager = diff(clean_3d_pose=z, noisy_2d_pose=x2d, output_loss=False, init_noise=nz)
    s_eager = eng.info("fc2_split_last")
    eng.set_graph_mode(True)
    try:
        for rep in range(3):
            _, gr = diff(clean_3d_pose=z, noisy_2d_pose=x2d, output_loss=False, init_noise=nz)
            assert torch.equal(gr, eager), rep
            assert eng.info("fc2_split_last") == s_eager >= 2
    finally:
        eng.set_graph_mode(False)


def test_no_leakage_into_the_default_path(pair81):
    (net, diff), (ref_net, ref_diff) = pair81
    dev = _dev()
    inp = inputs(1, 81, 73)
    x2d, nz = inp["x2d"].cuda(), inp["noise"].cuda()
    z = torch.zeros_like(nz)
    run = lambda d: d(clean_3d_pose=z, noisy_2d_pose=x2d, output_loss=False, init_noise=nz)[1]
    want = run(ref_diff)
    ref_eng = ref_net.engine_for(dev)
    assert ref_eng.info("latency_mode") == 0 and ref_eng.info("fc2_split_last") == 0
    eng = net.engine_for(dev)
    eng.set_graph_mode(True)
    try:
        net.latency_mode = True
        on = run(diff)
        assert eng.info("fc2_split_last") >= 2 and eng.info("graphs_cached") >= 1
        assert maxabs(on, want.cpu()) <= GATE
        net.latency_mode = False
        assert net.engine_for(dev) is eng
        assert eng.info("latency_mode") == 0 and eng.info("graphs_cached") == 0          # the change dropped the captured graphs
        off = run(diff)
        assert eng.info("fc2_split_last") == 0 and eng.info("graphs_cached") >= 1
        assert torch.equal(off, want)                                                    # the default path, bit for bit
        net.latency_mode = True
        net.engine_for(dev)
        assert eng.info("latency_mode") == 1 and eng.info("graphs_cached") == 0
        assert torch.equal(run(diff), on)
    finally:
        eng.set_graph_mode(False)
        net.latency_mode = True


def test_large_call_keeps_the_default_kernels():
    cfg = DenoiserConfig(num_frame=243, embed_dim=512, depth=1)
    net, _ = build_product(cfg, 33, precision="f16x3")
    ref_net, _ = build_product(cfg, 33, precision="f16x3")
    net.latency_mode = True
    x = _xcat(64, 243, 74)
    t = torch.full((64,), 500, dtype=torch.long, device="cuda")
    out = net.forward_denoise(x, t)
    eng = net.engine_for(_dev())
    assert eng.info("latency_mode") == 1 and eng.info("fc2_split_last") == 0
    assert torch.equal(out, ref_net.forward_denoise(x, t))


def test_range_guard_with_the_mode_on():
    """The construction of test_f16x3_range_guard (residual stream ~1e4: |8 x| > 65504): the flag must rise with the option on as it
    does on the default engine."""
    from diff3dhpe_amd import _lib
    cfg = DenoiserConfig(num_frame=27, embed_dim=512, depth=1)
    inp = inputs(2, 27, 3)
    x2d, nz = inp["x2d"].cuda(), inp["noise"].cuda()
    dev = _dev()

    def run(mutate, latency):
        sd = torch_sd(cfg, 8)
        mutate(sd)
        net = d3d.HPE_model(d3d.S2S_NAME)(num_frame=27, embed_dim=512, depth=1)
        net.load_state_dict(sd)
        net.precision = "f16x3"
        net.latency_mode = latency
        net.range_check = False
        diff = d3d.GaussianDiffusion(model=net, timesteps=1000, sampling_timesteps=2, clip_denoised=True).eval().to(dev)
        eng = diff._engine(dev)
        eng.range_flags(clear=True)
        diff(clean_3d_pose=torch.zeros_like(nz), noisy_2d_pose=x2d, output_loss=False, init_noise=nz)
        return eng

    def big_x(sd):
        sd["fusion_layer.bias"] += 1.0e4
    assert run(big_x, False).range_flags() & _lib.RANGE_ACT
    eng = run(big_x, True)
    assert eng.info("fc2_split_last") >= 2
    f = eng.range_flags()
    assert f & _lib.RANGE_ACT and not (f & _lib.RANGE_WEIGHT)
    eng = run(lambda sd: None, True)
    assert eng.info("fc2_split_last") >= 2 and eng.range_flags() == 0          # healthy model: nothing rises
