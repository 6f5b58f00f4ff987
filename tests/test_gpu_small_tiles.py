""""small_tiles" under "latency_mode" on the MI355X: the fused qkv + attention step of the F16X3 folded flow on 128-row tiles
(kernels_qkv_attn_x3_small.hip; include/d3d.h).  D = 512, 8 heads, depth 1 unless said otherwise, trained-like weights.

The contract is BIT-IDENTITY with the two-kernel flow (folded qkv GEMM -> [M][3 D] hi / lo planes in HBM -> launch_attn_temporal_x3): the
same MFMA products in the same k order, the same epilogue, the same softmax arithmetic.  So the comparisons between the two flows are
torch.equal.  Both legs keep "latency_mode" on (the same split-K launches elsewhere in the block); only the two launches that open a block
differ.  Block 0 is the only spatial block of a depth-1 model and keeps its direct form (whose values are not the K = 512 GEMM's), so
every case runs twice, "block0_direct" = 1 and 0 in BOTH legs: with 0, block 0 goes through the small spatial kernel's k-loop and the
reference through the qkv GEMM.

The shapes (T, B, J) are the smallest that hit each regime of the row map: see CASES.  Where a test states the expected "small_tiles_last"
as a number, it is the rule's value at the 256 CUs of the MI355X (expected_small restates the rule)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import diff3dhpe_amd as d3d
from conftest import gold
from helpers import hashed, maxabs, inputs, cfg_full, build_product, dev, cu_count
from diff3dhpe_amd.engine import op_layernorm, op_linear, op_attention, op_qkv_attn_x3_small
from diff3dhpe_amd.spec import DenoiserConfig
from diff3dhpe_amd.synth import synth_inputs, synth_state_dict

pytestmark = pytest.mark.gpu
GATE = 1e-4
D, H = 512, 8


def expected_small(T, B, J, n_cu):
    """The rule of include/d3d.h, restated: a block type takes the small tiles where its present fused launch runs fewer workgroups than the
    device has CUs and the small-tile launch -- ceil(groups / (127 // N)) tiles x 8 heads -- at most 5/8 as many.  Present launches: spatial
    (15 .. 17 joints) ceil(B T / 15) tiles (16 frames at 15 / 16 joints) x 8 heads; temporal (2 <= T <= 127) B ceil(J / min(255 // T, J))
    tiles x 8 heads.  Bit 0 spatial, bit 1 temporal."""
    small = lambda groups, N: (groups + 127 // N - 1) // (127 // N) * 8
    sp = tp = False
    if J in (15, 16, 17):
        fpt = 15 if J == 17 else 16
        sp = (B * T + fpt - 1) // fpt * 8 < n_cu and 8 * small(B * T, J) <= 5 * n_cu
    if 2 <= T <= 127:
        g = min(255 // T, J)
        tp = B * ((J + g - 1) // g) * 8 < n_cu and 8 * small(B * J, T) <= 5 * n_cu
    return int(sp) | 2 * int(tp)


def test_the_restated_rule_at_256_cus():
    assert expected_small(81, 1, 17, 256) == 3 and expected_small(27, 4, 17, 256) == 3
    assert expected_small(243, 1, 17, 256) == 0       # T = 243: 35 x 8 spatial small-tile workgroups; no temporal small form
    assert expected_small(128, 1, 17, 256) == 1       # 19 x 8 = 152 <= 160
    assert expected_small(81, 8, 17, 256) == 0        # 44 x 8 spatial, 8 x 6 x 8 temporal workgroups
    assert expected_small(81, 2, 17, 256) == 0        # 24 x 8 = 192 spatial, 34 x 8 = 272 temporal small-tile workgroups: more than 160
    assert expected_small(27, 8, 17, 256) == 0 and expected_small(27, 4, 17, 256) == 3      # 31 x 8 and 34 x 8 / 16 x 8 and 17 x 8
    assert expected_small(81, 4, 17, 256) == 0        # 47 x 8 spatial small-tile workgroups
    assert expected_small(27, 4, 17, 256) == 3 and expected_small(9, 3, 17, 256) == 3 and expected_small(2, 2, 17, 256) == 3
    assert expected_small(27, 1, 21, 256) == 2


# ------------------------------------------------------------------------------------------------ models, built once per module
_MODELS = {}


def _model(T, J=17, prec="f16x3", sharp=1.0, depth=1):
    """(net, diff, engine): D = 512, trained-like weights; sharp: the q and k rows of every qkv weight times sqrt(sharp) (logits x sharp)."""
    key = (T, J, prec, sharp, depth)
    if key not in _MODELS:
        cfg = DenoiserConfig(num_frame=T, num_joints=J, embed_dim=D, depth=depth)
        sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 11, family="trainedlike").items()}
        if sharp != 1.0:
            for k in sd:
                if k.endswith("attn.qkv.weight") or k.endswith("attn.qkv.bias"):
                    sd[k] = sd[k].clone()
                    sd[k][:2 * D] *= float(np.sqrt(sharp))
        net = d3d.HPE_model(d3d.S2S_NAME)(num_frame=T, num_joints=J, in_chans=2, embed_dim=D, depth=depth, num_heads=H, mlp_ratio=2.0,
                                          drop_path_rate=0.1, with_time_emb=True)
        net.load_state_dict(sd, strict=True)
        net.precision = prec
        net.range_check = False
        diff = d3d.GaussianDiffusion(model=net, timesteps=1000, sampling_timesteps=2, loss_type="l2", clip_denoised=True,
                                     beta_schedule="cosine", ddim_sampling_eta=0.0, clipLoss=True).eval().cuda()
        _MODELS[key] = (net, diff, diff._engine(dev()))
    return _MODELS[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_models():
    yield
    _MODELS.clear()


def _flow(net, small, fused=None, direct=None):
    """latency_mode on; small tiles on / off; the fused kernels and block 0's direct form on (default) or off.  Returns the engine."""
    net.latency_mode = True
    net.latency_small_tiles = bool(small)
    eng = net.engine_for(dev())
    fused = small if fused is None else fused
    direct = small if direct is None else direct
    eng.set_option("fused_spatial", int(fused))
    eng.set_option("fused_temporal", int(fused))
    eng.set_option("block0_direct", int(direct))
    return eng


def _restore(net):
    eng = _flow(net, False, fused=True, direct=True)
    eng.set_option("streams", 2)
    eng.set_graph_mode(False)
    net.latency_mode = False
    net.engine_for(dev())


def _xt(T, B, J, seed):
    inp = synth_inputs(B, T, J, seed=seed)
    x = torch.cat([torch.from_numpy(inp["x2d"]), torch.from_numpy(inp["noise"]) * 0.7], dim=-1).cuda()
    t = torch.tensor([(431 * i + 77) % 1000 for i in range(B)], dtype=torch.long).cuda()
    return x, t


# ------------------------------------------------------------------------------------------------ 1. bit identity
# (27, 1, 17): temporal 4 joints per tile with a last tile of one group, spatial 7 frames per tile with a last tile of 6
# (81, 2, 17): spatial tiles across the batch boundary (81 = 11 x 7 + 4), temporal one group per tile -- at 256 CUs both launches (192 / 272
#               workgroups) are beyond the rule's 160, so this case shows the PRESENT kernels running with the key on; (81, 1, 17) carries the
#               one-group-per-tile regime, (9, 3, 17) and the 15 / 16-joint cases tiles across a batch boundary
# (127, 1, 17): one pad key in the last of four key tiles
# (9, 3, 17): temporal 14 groups per tile, groups of several batch elements in one tile
# (2, 2, 17): 63 temporal groups per tile
# (27, 2, 15), (27, 2, 16): spatial groups of 15 / 16 joints (8 / 7 frames per tile)
CASES = [(27, 1, 17), (81, 2, 17), (81, 1, 17), (127, 1, 17), (9, 3, 17), (2, 2, 17), (27, 2, 15), (27, 2, 16)]


@pytest.mark.parametrize("T,B,J", CASES)
def test_small_tiles_equal_the_two_kernel_flow_bit_for_bit(T, B, J):
    net, _, _ = _model(T, J)
    x, t = _xt(T, B, J, 500 + T + J)
    try:
        bits = expected_small(T, B, J, cu_count())
        assert bits == (0 if (T, B) == (81, 2) else 3), (T, B, J, bits)
        for direct in (True, False):              # False: block 0 through the small spatial kernel's k-loop
            eng = _flow(net, False, direct=direct)
            if not bits & 1:                      # a block type the rule leaves alone keeps its present kernel in both legs (the grouped
                eng.set_option("fused_spatial", 1)   # temporal one is not bit-identical to two kernels)
            if not bits & 2:
                eng.set_option("fused_temporal", 1)
            want = net.forward_denoise(x, t).clone()
            assert eng.info("small_tiles_last") == 0 and eng.info("fused_spatial_last") == (0 if bits & 1 else 1)
            assert torch.isfinite(want).all()
            eng = _flow(net, True, direct=direct)
            got = net.forward_denoise(x, t).clone()
            assert eng.info("small_tiles") == 1 and eng.info("latency_mode") == 1
            assert eng.info("small_tiles_last") == bits, (T, B, J)
            assert eng.info("block0_direct_last") == int(direct)
            assert torch.equal(got, want), f"block0_direct {int(direct)}: max-abs {maxabs(got, want.cpu()):.3e}"
    finally:
        _restore(net)


def test_deeper_model_and_sampling_bit_for_bit():
    """Depth 2 (a spatial block behind block 0: row statistics from a GEMM epilogue) through a whole 2-step sampling."""
    net, _, eng = _model(27, 17, depth=2)
    inp = synth_inputs(2, 27, 17, seed=77)
    x2d, nz = torch.from_numpy(inp["x2d"]).cuda(), torch.from_numpy(inp["noise"]).cuda()
    try:
        eng = _flow(net, False, direct=True)
        eng.set_option("streams", 1)
        want = eng.ddim_sample(x2d, nz).clone()
        eng = _flow(net, True)
        got = eng.ddim_sample(x2d, nz).clone()
        assert eng.info("small_tiles_last") == 3
        assert torch.equal(got, want) and torch.isfinite(got).all()
    finally:
        _restore(net)


# ------------------------------------------------------------------------------------------------ 2. op level
def _fp64_attention(x, W, b, g, be, eps, groups, N, stride):
    """fp64 math of the op: LayerNorm, qkv GEMM, (softmax(q k^T / 8) - I) v per (group, head).  Group u holds rows
    (u // stride) N stride + u % stride + t stride."""
    xn = F.layer_norm(x.double(), (D,), g.double(), be.double(), eps)
    qkv = xn @ W.double().T + b.double()
    u, tt = torch.arange(groups), torch.arange(N)
    idx = ((u // stride) * N * stride + u % stride)[:, None] + tt[None, :] * stride
    x3 = qkv[idx]
    q, k, v = [x3[..., i * D:(i + 1) * D].reshape(groups, N, H, 64).transpose(1, 2) for i in range(3)]
    p = ((q * 0.125) @ k.transpose(-1, -2)).softmax(-1) - torch.eye(N, dtype=torch.float64)
    out = torch.empty(groups * N, D, dtype=torch.float64)
    out[idx] = (p @ v).transpose(1, 2).reshape(groups, N, D)
    return out


# (N, stride, groups): 20 frames of 17 joints (7 + 7 + 6 per tile); the frames of 17 / 17 / 5 joints
OP_CASES = [(17, 1, 20), (27, 17, 17), (81, 17, 17), (127, 5, 5)]


@pytest.mark.parametrize("N,stride,groups", OP_CASES)
def test_op_matches_fp64_as_well_as_the_two_kernel_ops(N, stride, groups):
    """The fused kernel alone against fp64 math (fold + GEMM + attention) on hashed inputs at scale 2.0.  Bound: 1.5 x the error of the
    existing two-kernel ops (op_layernorm, op_linear and op_attention in F16X3) on the same input."""
    rows = groups * N
    x = hashed(f"stx{N}", (rows, D), 41, 2.0)
    W = hashed("stW", (3 * D, D), 42, 1.0 / np.sqrt(D))
    b = hashed("stb", (3 * D,), 43, 0.5)
    g = 1 + 0.2 * hashed("stg", (D,), 44)
    be = 0.2 * hashed("stbe", (D,), 45)
    ref = _fp64_attention(x, W, b, g, be, 1e-6, groups, N, stride)
    temporal = stride != 1
    got = op_qkv_attn_x3_small(x.cuda(), W.cuda(), b.cuda(), g.cuda(), be.cuda(), 1e-6, groups, N, stride, H, temporal)
    qkv = op_linear(op_layernorm(x.cuda(), g.cuda(), be.cuda(), 1e-6), W.cuda(), b.cuda(), epi="none", precision="f16x3")
    two = op_attention(qkv, groups // stride, N, stride, H, True, precision="f16x3")
    e_small, e_two = maxabs(got, ref), maxabs(two, ref)
    print(f"op qkv+attention N={N} stride={stride} groups={groups}: small tiles {e_small:.3e}, two-kernel ops {e_two:.3e} "
          f"(|ref| max {ref.abs().max():.2f})")
    assert torch.isfinite(got).all()
    assert e_small <= 1.5 * e_two, (e_small, e_two)
    again = op_qkv_attn_x3_small(x.cuda(), W.cuda(), b.cuda(), g.cuda(), be.cuda(), 1e-6, groups, N, stride, H, temporal)
    assert torch.equal(again, got)


# ------------------------------------------------------------------------------------------------ 3. sharp softmax
@pytest.mark.parametrize("T,B", [(27, 2), (81, 1)])
def test_sharp_softmax_is_finite_and_bit_equal(T, B):
    """Logits scaled by 9 (q and k rows of every qkv weight times 3): near one-hot rows, exp2 underflow on most keys."""
    net, _, _ = _model(T, 17, sharp=9.0)
    x, t = _xt(T, B, 17, 610 + T)
    try:
        for direct in (True, False):
            _flow(net, False, direct=direct)
            want = net.forward_denoise(x, t).clone()
            eng = _flow(net, True, direct=direct)
            got = net.forward_denoise(x, t).clone()
            assert eng.info("small_tiles_last") == 3
            assert torch.isfinite(got).all() and torch.equal(got, want), direct
    finally:
        _restore(net)


# ------------------------------------------------------------------------------------------------ 4. row isolation
@pytest.mark.parametrize("T", [9, 27])
def test_a_nan_batch_element_does_not_reach_its_tile_neighbours(T):
    """B = 2, element 1 NaN: at T = 9 and 27 spatial tiles (7 frames) and temporal tiles (14 / 4 joints of 17) hold rows of both elements.
    The clean element is finite and bit-equal to its run alone -- where that run takes the same split-K forms of latency mode (each is a
    function of the row count), else to its rows in a batch with another clean element."""
    net, _, _ = _model(T, 17)
    x, t = _xt(T, 2, 17, 700 + T)
    bad = x.clone()
    bad[1] = float("nan")
    splits = lambda e: tuple(e.info(k) for k in ("fc2_split_last", "proj_split_last", "fc1_split_last"))
    try:
        for direct in (True, False):
            eng = _flow(net, True, direct=direct)
            got = eng.denoise(bad[..., :2], bad[..., 2:], t).clone()
            assert eng.info("small_tiles_last") == 3
            s2 = splits(eng)
            assert torch.isfinite(got[0]).all() and not torch.isfinite(got[1]).any()
            alone = eng.denoise(x[:1, ..., :2].contiguous(), x[:1, ..., 2:].contiguous(), t[:1].contiguous()).clone()
            assert eng.info("small_tiles_last") == 3
            if splits(eng) == s2:
                assert torch.equal(got[:1], alone), direct
            clean = eng.denoise(x[..., :2], x[..., 2:], t).clone()
            assert torch.equal(got[0], clean[0]), direct
    finally:
        _restore(net)


# ------------------------------------------------------------------------------------------------ 5. independence
def test_workspace_contents_streams_and_graph_replay():
    T = 27
    net, _, _ = _model(T, 17)
    inp = synth_inputs(2, T, 17, seed=811)
    x2d, nz = torch.from_numpy(inp["x2d"]).cuda(), torch.from_numpy(inp["noise"]).cuda()
    try:
        eng = _flow(net, True)
        eng.set_option("streams", 1)
        want = eng.ddim_sample(x2d, nz).clone()
        assert eng.info("small_tiles_last") == 3
        eng._workspace(2).view(torch.float32).fill_(float("nan"))                 # a stale read of the workspace shows
        assert torch.equal(eng.ddim_sample(x2d, nz), want)
        eng.set_option("streams", 2)                                             # two half-batches of one sequence each
        assert torch.equal(eng.ddim_sample(x2d, nz), want)
        assert eng.info("small_tiles_last") == 3
        eng.set_graph_mode(True)
        assert torch.equal(eng.ddim_sample(x2d, nz), want) and torch.equal(eng.ddim_sample(x2d, nz), want)   # capture, then replay
        assert eng.info("graphs_cached") >= 1 and eng.info("small_tiles_last") == 3
        eng.set_option("small_tiles", 0)                                         # the option drops the captured graphs
        assert eng.info("graphs_cached") == 0
        eng.set_option("small_tiles", 1)
        assert torch.equal(eng.ddim_sample(x2d, nz), want)
    finally:
        _restore(net)


# ------------------------------------------------------------------------------------------------ 6. proof of the path
@pytest.mark.parametrize("T,J", [(128, 17), (243, 17), (27, 21)])
def test_shapes_outside_the_predicate_keep_their_kernels(T, J):
    """T = 128 (no fused temporal kernel) and T = 243 (the one-joint fused kernel) keep their temporal launches, 21 joints their
    two-kernel spatial flow: the bit reads 0 and the result is that of the two-kernel flow -- to which the kernels that keep running
    there are bit-identical."""
    net, _, _ = _model(T, J)
    x, t = _xt(T, 1, J, 900 + T + J)
    want_bits = expected_small(T, 1, J, cu_count())
    assert want_bits == {(128, 17): 1, (243, 17): 0, (27, 21): 2}[(T, J)]     # (256 CUs; T = 243: 35 x 8 small spatial workgroups > 160)
    try:
        _flow(net, False, direct=True)
        want = net.forward_denoise(x, t).clone()
        eng = _flow(net, True)
        got = net.forward_denoise(x, t).clone()
        assert eng.info("small_tiles_last") == want_bits
        assert torch.equal(got, want)
        eng = _flow(net, False, fused=True, direct=True)                          # latency mode alone
        off = net.forward_denoise(x, t).clone()
        assert eng.info("small_tiles_last") == 0
        if J == 17:      # the 256-row spatial kernel is bit-identical to the two-kernel flow as well
            assert torch.equal(off, got)
        else:            # the grouped temporal kernel is not: inside the gate
            assert maxabs(off, got.cpu()) <= GATE
    finally:
        _restore(net)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_other_precisions_ignore_the_key(prec):
    net, _, eng = _model(27, 17, prec=prec)
    x, t = _xt(27, 1, 17, 950)
    want = net.forward_denoise(x, t).clone()
    assert eng.info("small_tiles_last") == 0
    try:
        eng.set_option("latency_mode", 1)
        eng.set_option("small_tiles", 1)
        got = net.forward_denoise(x, t).clone()
        assert eng.info("small_tiles") == 1 and eng.info("small_tiles_last") == 0
        assert torch.equal(got, want)
    finally:
        eng.set_option("small_tiles", 0)
        eng.set_option("latency_mode", 0)


def test_without_latency_mode_the_key_is_inert():
    net, _, eng = _model(81, 17)
    x, t = _xt(81, 1, 17, 960)
    net.latency_mode = False
    net.latency_small_tiles = False
    eng = net.engine_for(dev())
    want = net.forward_denoise(x, t).clone()
    try:
        net.latency_small_tiles = True
        assert net.engine_for(dev()) is eng
        got = net.forward_denoise(x, t).clone()
        assert eng.info("small_tiles") == 1 and eng.info("latency_mode") == 0 and eng.info("small_tiles_last") == 0
        assert torch.equal(got, want)
        net.latency_mode = True                                                  # with the mode on the same key selects the kernel
        net.forward_denoise(x, t)
        assert eng.info("small_tiles_last") == 3
    finally:
        _restore(net)
        net.latency_small_tiles = False
        net.engine_for(dev())


# ------------------------------------------------------------------------------------------------ 7. golden parity
@pytest.mark.parametrize("tag,cfg", [("full_T81", cfg_full(81)), ("s2f_T27", cfg_full(27, seq2frame=True))])
def test_golden_parity_with_the_option_on(tag, cfg):
    """The depth-8 fixtures of the F16X3 parity test, one sequence at a time (B = 1), latency mode and small tiles on: <= 1e-4, the
    project's gate."""
    g = gold("denoise_" + tag)
    B = int(g["B"])
    net, _ = build_product(cfg, int(g["seed"]), precision="f16x3")
    net.latency_mode = True
    net.latency_small_tiles = True
    eng = net.engine_for(dev())
    inp = inputs(B, cfg.num_frame, int(g["input_seed"]))
    xcat = torch.cat([inp["x2d"], inp["noise"] * float(g["y_scale"])], dim=-1).cuda()
    worst = 0.0
    for key, tv in (("t999", 999), ("t443", 443), ("t0", 0)):
        for i in range(B):
            out = net.forward_denoise(xcat[i:i + 1].contiguous(), torch.full((1,), tv, dtype=torch.long, device="cuda"))
            assert eng.info("small_tiles_last") == 3 and eng.info("latency_mode") == 1, (tag, key, i)
            worst = max(worst, maxabs(out, g[key][i:i + 1]))
    print(f"denoise {tag} [f16x3, latency_mode, small_tiles], B = 1: max-abs {worst:.3e}")
    assert worst <= GATE, tag
