""""fused_narrow" on the MI355X: the LayerNorm-folded qkv GEMM and the GRAND attention of an F16X3 engine with heads of 32 columns in pairs
(embed_dim 256, 8 heads) or 16 columns in quads (embed_dim 128, 8 heads) as ONE kernel, q / k / v in LDS (the narrow forms of
kernels_qkv_attn_x3_small.hip; include/d3d.h).

The contract is BIT-IDENTITY with the two launches it replaces -- the folded qkv GEMM, its [M][3 D] hi / lo planes in HBM, then
launch_attn_x3_h32 / launch_attn_x3_h16: the same MFMA products in the same k order, the same epilogue, the same per-head softmax.  So
key on against key off is torch.equal, at op level and through the engine.

  1. op level: fp64 math, the existing two-kernel ops, determinism;
  2. op level: a NaN head does not reach the other heads of its 64-column segment, a NaN group does not reach its tile neighbours;
  3. engine level: key on == key off bit for bit, both inside the 1e-4 gate of the fp64 oracle, the path proven by "fused_narrow_last" and
     the per-kernel trace, the range word equal;
  4. engine level: a NaN batch element, workspace contents, streams, graph replay; engines outside the predicate ignore the key."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import hashed, maxabs, torch_sd, product_with_engine, dev
from diff3dhpe_amd import engine as E
from diff3dhpe_amd.spec import DenoiserConfig
from diff3dhpe_amd.synth import synth_inputs

pytestmark = pytest.mark.gpu
GATE = 1e-4
EPS = 1e-6
WIDTHS = [(256, 8), (128, 8)]      # (embed_dim, heads): heads of 32 columns in pairs, of 16 columns in quads


# ------------------------------------------------------------------------------------------------ 1. op level
# (N, stride, groups):
#   (17, 1, 20)   spatial, tiles of 7 + 7 + 6 groups          (21, 1, 8)    another joint count (6 + 2 groups)
#   (1, 1, 5)     one-token groups                            (27, 17, 17)  temporal, 4 joints per tile, a last tile of one
#   (33, 2, 4)    two key tiles, the 31 pad keys of a group are the next group's rows
#   (81, 17, 17)  three key tiles, one group per tile         (127, 5, 5)   four key tiles, one pad key
OP_CASES = [(17, 1, 20), (21, 1, 8), (1, 1, 5), (27, 17, 17), (33, 2, 4), (81, 17, 17), (127, 5, 5)]
_OPS = {}


def _operands(D, N, stride, groups):
    rows = groups * N
    x = hashed(f"fnx{N}_{D}", (rows, D), 41, 2.0)
    W = hashed(f"fnW{D}", (3 * D, D), 42, 1.0 / np.sqrt(D))
    b = hashed(f"fnb{D}", (3 * D,), 43, 0.5)
    g = 1 + 0.2 * hashed(f"fng{D}", (D,), 44)
    be = 0.2 * hashed(f"fnbe{D}", (D,), 45)
    return x, W, b, g, be


def _group_rows(N, stride, groups):
    """(groups, N) row indices: group u holds rows (u // stride) N stride + u % stride + t stride."""
    u, tt = torch.arange(groups), torch.arange(N)
    return ((u // stride) * N * stride + u % stride)[:, None] + tt[None, :] * stride


def _fp64_attention(x, W, b, g, be, H, groups, N, stride):
    """fp64 math of the op: LayerNorm, qkv GEMM, (softmax(q k^T / sqrt(dh)) - I) v per (group, head)."""
    D = x.shape[1]
    dh = D // H
    xn = F.layer_norm(x.double(), (D,), g.double(), be.double(), EPS)
    qkv = xn @ W.double().T + b.double()
    idx = _group_rows(N, stride, groups)
    x3 = qkv[idx]
    q, k, v = [x3[..., i * D:(i + 1) * D].reshape(groups, N, H, dh).transpose(1, 2) for i in range(3)]
    p = ((q * dh ** -0.5) @ k.transpose(-1, -2)).softmax(-1) - torch.eye(N, dtype=torch.float64)
    out = torch.empty(groups * N, D, dtype=torch.float64)
    out[idx] = (p @ v).transpose(1, 2).reshape(groups, N, D)
    return out


def _narrow(x, W, b, g, be, H, N, stride, groups):
    return E.op_qkv_attn_x3_narrow(x.cuda(), W.cuda(), b.cuda(), g.cuda(), be.cuda(), EPS, groups, N, stride, H, stride != 1)


def _width_attention(qkv, H, N, stride, groups):
    """The stand-alone attention op of the width on fp32 q / k / v rows."""
    op = E.op_attention_h32 if qkv.shape[1] // 3 // H == 32 else E.op_attention_h16
    if stride == 1:
        return op(qkv, 1, groups, N, H, False)
    return op(qkv, groups // stride, N, stride, H, True)


def _clean(D, H, case):
    """(operands, fp64 reference, the fused op's result) of a case, computed once."""
    key = (D, H) + case
    if key not in _OPS:
        N, stride, groups = case
        ops = _operands(D, N, stride, groups)
        _OPS[key] = (ops, _fp64_attention(*ops, H, groups, N, stride), _narrow(*ops, H, N, stride, groups))
    return _OPS[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _OPS.clear()
    _MODELS.clear()


@pytest.mark.parametrize("D,H", WIDTHS)
@pytest.mark.parametrize("N,stride,groups", OP_CASES)
def test_op_matches_fp64_as_well_as_the_two_kernel_ops(N, stride, groups, D, H):
    """Bound: 1.5 x the error of the existing two-kernel F16X3 ops (op_layernorm, op_linear, then the width's attention op) on the same
    input, the rule of tests/test_gpu_small_tiles.py.  The same call twice gives the same bits."""
    (x, W, b, g, be), ref, got = _clean(D, H, (N, stride, groups))
    qkv = E.op_linear(E.op_layernorm(x.cuda(), g.cuda(), be.cuda(), EPS), W.cuda(), b.cuda(), epi="none", precision="f16x3")
    two = _width_attention(qkv, H, N, stride, groups)
    e_fused, e_two = maxabs(got, ref), maxabs(two, ref)
    print(f"op qkv+attention D={D} N={N} stride={stride} groups={groups}: fused {e_fused:.3e}, two-kernel ops {e_two:.3e} "
          f"(|ref| max {ref.abs().max():.2f})")
    assert torch.isfinite(got).all()
    assert e_fused <= 1.5 * e_two, (e_fused, e_two)
    assert torch.equal(_narrow(x, W, b, g, be, H, N, stride, groups), got)


# No existing hook composes the fused kernel's arithmetic bit for bit: d3d_op_linear_folded returns the hi / lo planes the kernel keeps in
# LDS, but the width's attention op takes fp32 rows and splits them again, and that split is not the identity on a (hi, lo) pair -- where
# the remainder behind hi is one fp16 half-ulp short of the midpoint, lo rounds up to the midpoint, hi + lo is an exact tie and the second
# split may pick the other neighbour as hi (about one element in 8000; same value, other planes, other MFMA roundings: 2.4e-7 apart at
# D = 256).  The bit-for-bit comparison with the two launches is the engine-level one below, on the planes themselves.


# ------------------------------------------------------------------------------------------------ 2. isolation
@pytest.mark.parametrize("D,H,heads", [(256, 8, (1, 0)), (128, 8, (1, 0, 2, 3, 6))])
@pytest.mark.parametrize("N,stride,groups", [(17, 1, 20), (33, 2, 4), (127, 5, 5)])
def test_a_nan_head_does_not_reach_the_other_heads_of_its_segment(N, stride, groups, D, H, heads):
    """A NaN bias on one head's q, k and v rows (its own output is whatever the output clamp makes of NaN): every other head -- its pair /
    quad neighbours, whose K, V and accumulator tiles share its LDS rows, included -- is finite and keeps its bits.  Width 16: each head
    of a quad in turn."""
    (x, W, b, g, be), _, clean = _clean(D, H, (N, stride, groups))
    dh = D // H
    for hd in heads:
        bad = b.clone()
        for part in range(3):
            bad[part * D + hd * dh:part * D + (hd + 1) * dh] = float("nan")
        got = _narrow(x, W, bad, g, be, H, N, stride, groups)
        others = [c for c in range(D) if c // dh != hd]
        assert torch.isfinite(got[:, others]).all(), hd
        assert torch.equal(got[:, others], clean[:, others]), hd


@pytest.mark.parametrize("D,H", WIDTHS)
@pytest.mark.parametrize("N,stride,groups", [(17, 1, 20), (33, 2, 4), (27, 17, 17)])
def test_a_nan_group_does_not_reach_its_tile_neighbours(N, stride, groups, D, H):
    """Every odd group's rows NaN: the planes are compact, so the pad keys of an even group ARE the next (NaN) group's rows -- (33, 2, 4):
    31 of the 64 keys of group 0 and group 2.  The even groups are finite and keep their bits."""
    (x, W, b, g, be), _, clean = _clean(D, H, (N, stride, groups))
    idx = _group_rows(N, stride, groups)
    bad = x.clone()
    bad[idx[1::2].reshape(-1)] = float("nan")
    got = _narrow(bad, W, b, g, be, H, N, stride, groups)
    even = idx[0::2].reshape(-1)
    assert torch.isfinite(got[even]).all()
    assert torch.equal(got[even], clean[even])


# ------------------------------------------------------------------------------------------------ 3. engine level
_MODELS = {}


def _model(T, J, D, H=8, prec="f16x3", depth=1):
    """(net, diff, engine, state dict): trained-like weights, seed 11."""
    key = (T, J, D, H, prec, depth)
    if key not in _MODELS:
        cfg = DenoiserConfig(num_frame=T, num_joints=J, embed_dim=D, depth=depth, num_heads=H)
        net, diff, eng = product_with_engine(cfg, 11, prec, 2, family="trainedlike")
        net.range_check = False
        _MODELS[key] = (net, diff, eng, torch_sd(cfg, 11, family="trainedlike"))
    return _MODELS[key]


def _xt(T, B, J, seed):
    inp = synth_inputs(B, T, J, seed=seed)
    x = torch.cat([torch.from_numpy(inp["x2d"]), torch.from_numpy(inp["noise"]) * 0.7], dim=-1)
    t = torch.tensor([(431 * i + 77) % 1000 for i in range(B)], dtype=torch.long)
    return x, t


def _expected_last(T, J):
    return (1 if J <= 127 else 0) | (2 if T <= 127 else 0)


def _traced(net, eng, x, t):
    """(output, trace, range word) of one forward_denoise with the per-kernel trace on."""
    eng.range_flags(clear=True)
    eng.set_trace(64)
    try:
        out = net.forward_denoise(x, t).clone()
        tr = eng.trace_read()
    finally:
        eng.set_trace(0)
    return out, tr, eng.range_flags(clear=True)


# (T, B, J).  (27, 1, 17): temporal 4 joints per tile, spatial 7 frames per tile | (81, 2, 17): spatial tiles across the batch boundary,
# three key tiles | (127, 1, 17): four key tiles, one pad key | (9, 3, 17): 14 temporal groups per tile, several batch elements in a tile |
# (2, 2, 17): 63 temporal groups per tile | (27, 2, 15), (27, 2, 21): other joint counts | (128, 1, 17), (243, 1, 17): the temporal blocks
# keep the resident kernel of the width | (300, 1, 17): ... the key-streaming one
ENGINE_CASES = [(27, 1, 17), (81, 2, 17), (127, 1, 17), (9, 3, 17), (2, 2, 17), (27, 2, 15), (27, 2, 21), (128, 1, 17), (243, 1, 17),
                (300, 1, 17)]


@pytest.mark.parametrize("D,H", WIDTHS)
@pytest.mark.parametrize("T,B,J", ENGINE_CASES)
def test_key_on_equals_key_off_bit_for_bit_inside_the_gate(T, B, J, D, H):
    """forward_denoise, depth 1, per-row t.  Key on is torch.equal to key off; "fused_narrow_last" and the trace prove the path -- the
    fused blocks write no q / k / v planes (trace kernel 2) and the attention outputs (kernel 3) have the same checksums in both legs;
    the range word is the same; against oracle/d3d_oracle.py in fp64 both legs sit inside the 1e-4 gate."""
    from oracle import d3d_oracle as orc
    net, _, eng, sd = _model(T, J, D, H)
    x, t = _xt(T, B, J, 500 + T + J)
    ref32 = orc.forward_denoise(sd, x, t, depth=1)
    torch.set_default_dtype(torch.float64)      # (the oracle's sinusoid and identity follow the default dtype)
    try:
        ref64 = orc.forward_denoise({k: v.double() for k, v in sd.items()}, x.double(), t, depth=1)
    finally:
        torch.set_default_dtype(torch.float32)
    assert ref64.dtype == torch.float64
    floor = (ref32.double() - ref64).abs().max().item()
    want_last = _expected_last(T, J)
    kernels = lambda tr, blk: sorted({(tag >> 4) & 0xF for tag, _ in tr if (tag >> 8) & 0xFF == blk})
    attn = lambda tr: [(tag & 0xFFFF, s) for tag, s in tr if (tag >> 4) & 0xF == 3]
    try:
        eng.set_option("fused_narrow", 0)
        off, tr_off, rw_off = _traced(net, eng, x.cuda(), t.cuda())
        assert eng.info("fused_narrow_last") == 0
        assert 2 in kernels(tr_off, 0) and 2 in kernels(tr_off, 1)
        eng.set_option("fused_narrow", 1)
        on, tr_on, rw_on = _traced(net, eng, x.cuda(), t.cuda())
        assert eng.info("fused_narrow") == 1 and eng.info("fused_narrow_last") == want_last, (T, B, J)
    finally:
        eng.set_option("fused_narrow", 0)
    assert 2 not in kernels(tr_on, 0) and 3 in kernels(tr_on, 0)                  # block 0 included: no q / k / v plane write
    assert (2 in kernels(tr_on, 1)) == (T > 127) and 3 in kernels(tr_on, 1)
    assert attn(tr_on) == attn(tr_off)
    e_on, e_off = (on.cpu().double() - ref64).abs().max().item(), (off.cpu().double() - ref64).abs().max().item()
    print(f"fused_narrow D={D} T={T} B={B} J={J}: err_on {e_on:.3e} err_off {e_off:.3e} oracle fp32 floor {floor:.3e} "
          f"last {want_last} range {rw_on}/{rw_off}")
    assert torch.isfinite(on).all()
    assert torch.equal(on, off), f"max-abs {maxabs(on, off.cpu()):.3e}"
    assert rw_on == rw_off
    assert e_on <= GATE and e_off <= GATE


@pytest.mark.parametrize("D,H", WIDTHS)
def test_deeper_model_and_sampling_bit_for_bit(D, H):
    """Depth 2 (blocks behind block 0 take their row statistics from the post-norm row kernel) through a whole 2-step sampling; the key
    set through the model class attribute."""
    T, B = 27, 2
    net, _, eng, _ = _model(T, 17, D, H, depth=2)
    inp = synth_inputs(B, T, 17, seed=77)
    x2d, nz = torch.from_numpy(inp["x2d"]).cuda(), torch.from_numpy(inp["noise"]).cuda()
    try:
        want = eng.ddim_sample(x2d, nz).clone()
        assert eng.info("fused_narrow_last") == 0
        net.fused_narrow = True
        assert net.engine_for(dev()) is eng and eng.info("fused_narrow") == 1
        got = eng.ddim_sample(x2d, nz).clone()
        assert eng.info("fused_narrow_last") == 3
        assert torch.isfinite(got).all() and torch.equal(got, want)
    finally:
        net.fused_narrow = False
        net.engine_for(dev())
    assert eng.info("fused_narrow") == 0


# ------------------------------------------------------------------------------------------------ 4. isolation and independence
@pytest.mark.parametrize("D,H", WIDTHS)
@pytest.mark.parametrize("T", [9, 27])
def test_a_nan_batch_element_does_not_reach_its_tile_neighbours(T, D, H):
    """B = 2, element 1 NaN: spatial tiles (7 frames) and temporal tiles (14 / 4 joints of 17) hold rows of both elements.  Element 0 is
    finite and keeps the bits it has in the clean batch."""
    net, _, eng, _ = _model(T, 17, D, H)
    x, t = _xt(T, 2, 17, 700 + T)
    x, t = x.cuda(), t.cuda()
    bad = x.clone()
    bad[1] = float("nan")
    try:
        eng.set_option("fused_narrow", 1)
        clean = eng.denoise(x[..., :2], x[..., 2:], t).clone()
        got = eng.denoise(bad[..., :2], bad[..., 2:], t).clone()
        assert eng.info("fused_narrow_last") == 3
    finally:
        eng.set_option("fused_narrow", 0)
    assert torch.isfinite(got[0]).all() and not torch.isfinite(got[1]).any()
    assert torch.equal(got[0], clean[0])


@pytest.mark.parametrize("D,H", WIDTHS)
def test_workspace_contents_streams_and_graph_replay(D, H):
    T = 27
    net, _, eng, _ = _model(T, 17, D, H)
    inp = synth_inputs(2, T, 17, seed=811)
    x2d, nz = torch.from_numpy(inp["x2d"]).cuda(), torch.from_numpy(inp["noise"]).cuda()
    try:
        eng.set_option("fused_narrow", 1)
        eng.set_option("streams", 1)
        want = eng.ddim_sample(x2d, nz).clone()
        assert eng.info("fused_narrow_last") == 3
        eng._workspace(2).view(torch.float32).fill_(float("nan"))                 # a stale read of the workspace shows
        assert torch.equal(eng.ddim_sample(x2d, nz), want)
        eng.set_option("streams", 2)                                             # two half-batches of one sequence each
        assert torch.equal(eng.ddim_sample(x2d, nz), want)
        assert eng.info("fused_narrow_last") == 3
        eng.set_graph_mode(True)
        assert torch.equal(eng.ddim_sample(x2d, nz), want) and torch.equal(eng.ddim_sample(x2d, nz), want)   # capture, then replay
        assert eng.info("graphs_cached") >= 1 and eng.info("fused_narrow_last") == 3
        eng.set_option("fused_narrow", 0)                                        # the option drops the captured graphs
        assert eng.info("graphs_cached") == 0
        assert torch.equal(eng.ddim_sample(x2d, nz), want) and eng.info("fused_narrow_last") == 0
    finally:
        eng.set_graph_mode(False)
        eng.set_option("streams", 2)
        eng.set_option("fused_narrow", 0)


def test_the_decision_does_not_read_latency_mode():
    net, _, eng, _ = _model(27, 17, 256)
    x, t = _xt(27, 1, 17, 960)
    try:
        eng.set_option("fused_narrow", 1)
        for lat in (1, 0):
            eng.set_option("latency_mode", lat)
            net.forward_denoise(x.cuda(), t.cuda())
            assert eng.info("fused_narrow_last") == 3, lat
    finally:
        eng.set_option("latency_mode", 0)
        eng.set_option("fused_narrow", 0)


@pytest.mark.parametrize("D,H,prec", [(256, 8, "fp32"), (128, 8, "fp32"), (512, 8, "bf16"), (512, 8, "f16x3"), (384, 8, "f16x3"),
                                      (256, 4, "f16x3"), (96, 6, "f16x3")])
def test_engines_outside_the_predicate_ignore_the_key(D, H, prec):
    """FP32 and BF16 engines, heads of 64 and 48 columns, and six heads of 16 columns (no whole quads)."""
    T = 27
    net, _, eng, _ = _model(T, 17, D, H, prec=prec)
    x, t = _xt(T, 1, 17, 950)
    want = net.forward_denoise(x.cuda(), t.cuda()).clone()
    assert eng.info("fused_narrow_last") == 0
    try:
        eng.set_option("fused_narrow", 1)
        got = net.forward_denoise(x.cuda(), t.cuda()).clone()
        assert eng.info("fused_narrow") == 1 and eng.info("fused_narrow_last") == 0
        assert torch.equal(got, want)
    finally:
        eng.set_option("fused_narrow", 0)
