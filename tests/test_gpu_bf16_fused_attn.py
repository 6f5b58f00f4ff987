"""BF16 mode: the fused qkv GEMM + attention kernels (kernels_qkv_attn_bf16.hip; "fused_spatial" / "fused_temporal" on a bf16 engine).

The contract is BIT-IDENTITY with the two-kernel flow (qkv GEMM -> [M][3 D] bf16 in HBM -> attention): the same MFMA products in the
same k order into each accumulator element, the same rounding points, the same softmax arithmetic.  So every comparison between the two
flows here is torch.equal; the loose emulation gates of tests/test_gpu_bf16.py are not leaned on.

Shapes.  helpers.cfg_small (embed_dim 32: head width 4) is not a shape the bf16 engine accepts at all (head width 64 only), so the
small engine-level model here is embed_dim 256 / 4 heads / depth 2.  The refused shape is embed_dim 192 / 3 heads: the bf16 engine
takes it, the fused predicates (D % 128 == 0) do not -- the two-kernel flow must run there with both flags 0."""
import numpy as np
import pytest
import torch

from conftest import gold
from helpers import cfg_full, inputs, build_product, maxabs
from diff3dhpe_amd.engine import op_linear, op_attention, op_qkv_attn_bf16
from diff3dhpe_amd.spec import DenoiserConfig
from diff3dhpe_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu
D, H = 512, 8


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float64)


def _qkv_weights(family):
    sd = synth_state_dict(cfg_full(27), 11, family=family)
    kw = [k for k in sd if k.endswith("attn.qkv.weight")][2]
    return torch.from_numpy(sd[kw]), torch.from_numpy(sd[kw.replace("weight", "bias")])


def _rows(M, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=g) * (1.0 + 0.1 * torch.randn(D, generator=g))   # a LayerNorm output with gains
    return x + 0.1 * torch.randn(D, generator=g)


# (B, T, J, temporal): M never a multiple of 255; the larger ones give a workgroup more than one tile (persistent walk)
OP_CASES = [(1, 31, 17, False), (1, 607, 17, False), (2, 27, 17, True), (2, 81, 17, True), (2, 243, 17, True), (3, 100, 5, True)]


@pytest.mark.parametrize("family", ["uniform", "trainedlike"])
@pytest.mark.parametrize("B,T,J,temporal", OP_CASES)
def test_op_fused_equals_linear_then_attention_bit_for_bit(B, T, J, temporal, family):
    W, b = _qkv_weights(family)
    A = _rows(B * T * J, B * T + J).cuda()
    qkv = op_linear(A, W.cuda(), b.cuda(), epi="none", precision="bf16")
    want = op_attention(qkv, B, T, J, H, temporal, precision="bf16")
    groups, N, stride = (B * J, T, J) if temporal else (B * T, J, 1)
    got = op_qkv_attn_bf16(A, W.cuda(), b.cuda(), groups, N, stride, H, temporal)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want), f"max-abs {maxabs(got, want.cpu()):.3e}"


@pytest.mark.parametrize("B,T,J,temporal", [(1, 31, 17, False), (2, 81, 17, True), (1, 243, 17, True)])
def test_op_fused_matches_rounded_operand_math(B, T, J, temporal):
    """The one reference here that shares no code with the kernels: fp64 math with the bf16 rounding points of the oracle's
    operand_rounding(torch.bfloat16) emulation, hand-rolled as the op tests of tests/test_gpu_bf16.py hand-roll them (the emulation
    itself works on whole models, not on one op), in two stages with those tests' own bound forms:
      * GEMM stage: op_linear (bf16) -- bit for bit the q / k / v the fused kernel keeps in LDS, by the torch.equal tests above --
        against fp64 on the rounded operands: per-element one-ulp bound and >= 99.8 % round-to-nearest-even of the exact value
        (test_bf16_linear_matches_rounded_operand_math);
      * attention stage: the fused kernel's output against fp64 attention on THOSE bf16 q / k / v (q third x 2^-3: exact), so that only
        the attention arithmetic differs: max-abs <= 3e-2 max(1, |ref| / 4) AND >= 99.8 % of the outputs equal RNE(exact)
        (test_bf16_attention_matches_rounded_operand_math).  A wrong key mask, diagonal or bias column fails the second half."""
    W, b = _qkv_weights("uniform")
    A = _rows(B * T * J, 7 * T + J)
    groups, N, stride = (B * J, T, J) if temporal else (B * T, J, 1)
    out = op_qkv_attn_bf16(A.cuda(), W.cuda(), b.cuda(), groups, N, stride, H, temporal).cpu().double()
    qkv = op_linear(A.cuda(), W.cuda(), b.cuda(), epi="none", precision="bf16").cpu().double()
    lin = _bf(A) @ _bf(W).T + b.double()
    ulp = torch.maximum(lin.abs(), torch.tensor(2.0 ** -120, dtype=torch.float64)) * 2.0 ** -8
    assert ((qkv - lin).abs() <= ulp + 2e-5).all() and torch.equal(qkv, _bf(qkv.float()))
    lin_exact = (qkv == _bf(lin.float())).float().mean().item()
    qkv = qkv.clone()
    qkv[:, :D] *= 0.125
    x = qkv.view(B, T, J, 3, H, 64)
    x = x.permute(3, 0, 2, 4, 1, 5) if temporal else x.permute(3, 0, 1, 4, 2, 5)
    q, k, v = x[0], x[1], x[2]
    a = q @ k.transpose(-2, -1)
    p = a.softmax(-1) - torch.eye(a.shape[-1], dtype=torch.float64)
    o = _bf(_bf(p.float()) @ v)
    o = o.permute(0, 3, 1, 2, 4) if temporal else o.permute(0, 1, 3, 2, 4)
    ref = o.reshape(B * T * J, D)
    err = (out - ref).abs().max().item()
    exact = (out == ref).float().mean().item()
    print(f"fused bf16 qkv+attention B={B} T={T} J={J} temporal={temporal}: q/k/v {100 * lin_exact:.3f} % RNE(exact); output max-abs vs fp64 "
          f"on the same q/k/v {err:.3e} (|out| max {ref.abs().max():.2f}), {100 * exact:.3f} % equal RNE(exact)")
    assert lin_exact >= 0.998, lin_exact
    assert err <= 3e-2 * max(1.0, ref.abs().max().item() / 4) and exact >= 0.998, (err, exact)


@pytest.mark.parametrize("B,T,J,temporal", [(1, 31, 17, False), (2, 81, 17, True), (2, 27, 17, True)])
def test_op_a_non_finite_group_stays_in_its_own_rows(B, T, J, temporal):
    """The pad keys of a group are the NEXT group's rows in the tile (another frame, joint or batch element): their V values are
    replaced by zeros before the second product, so NaN / Inf rows of one group change no other group's output -- as in the two-kernel
    flow, whose pad rows are zeros."""
    W, b = _qkv_weights("uniform")
    A = _rows(B * T * J, 3 * T + J)
    groups, N, stride = (B * J, T, J) if temporal else (B * T, J, 1)
    clean = op_qkv_attn_bf16(A.cuda(), W.cuda(), b.cuda(), groups, N, stride, H, temporal).view(B, T, J, D)
    bad = A.clone().view(B, T, J, D)
    if temporal:
        bad[0, :, 1] = float("nan"); bad[B - 1, :, 5] = float("inf")           # two joints
        keep = torch.ones(B, T, J, dtype=torch.bool); keep[0, :, 1] = False; keep[B - 1, :, 5] = False
    else:
        bad[0, 1] = float("nan"); bad[0, 16] = float("inf")                    # two frames (one at a tile's start)
        keep = torch.ones(B, T, J, dtype=torch.bool); keep[0, 1] = False; keep[0, 16] = False
    got = op_qkv_attn_bf16(bad.reshape(-1, D).cuda(), W.cuda(), b.cuda(), groups, N, stride, H, temporal).view(B, T, J, D)
    assert not torch.isfinite(got[~keep.cuda()]).any()                    # the poisoned groups' own rows: every value non-finite
    assert torch.equal(got[keep.cuda()], clean[keep.cuda()])


# ------------------------------------------------------------------------------------------------ engine level
def _small(T):
    return DenoiserConfig(num_frame=T, embed_dim=256, depth=2, num_heads=4)


_MODELS = {}


def _model(kind, T, prec="bf16"):
    """(net, diff, engine) built once per module."""
    key = (kind, T, prec)
    if key not in _MODELS:
        cfg = {"full": cfg_full, "small": _small, "refused": lambda t: DenoiserConfig(num_frame=t, embed_dim=192, depth=2, num_heads=3)}[kind](T)
        net, diff = build_product(cfg, 21, sampling=9, precision=prec)
        _MODELS[key] = (net, diff, diff._engine(torch.device("cuda", torch.cuda.current_device())))
    return _MODELS[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_models():
    yield
    _MODELS.clear()


def _set(eng, on):
    eng.set_option("fused_spatial", int(on))
    eng.set_option("fused_temporal", int(on))


def _run(net, eng, T, B=3, seed=310):
    inp = inputs(B, T, seed)
    xcat = torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1).cuda()
    t = torch.tensor([(431 * i + 77) % 1000 for i in range(B)], dtype=torch.long).cuda()
    den = net.forward_denoise(xcat, t).clone()
    return den, eng.ddim_sample(inp["x2d"].cuda(), inp["noise"].cuda()).clone()


@pytest.mark.parametrize("kind,T", [("full", 27), ("full", 81), ("full", 243), ("small", 27), ("small", 81), ("small", 243)])
def test_engine_fused_equals_two_kernel_flow_bit_for_bit(kind, T):
    net, _, eng = _model(kind, T)
    try:
        _set(eng, False)
        den0, y0 = _run(net, eng, T)
        assert (eng.info("bf16_fused_spatial_last"), eng.info("bf16_fused_temporal_last")) == (0, 0)
        _set(eng, True)
        den1, y1 = _run(net, eng, T)
        assert (eng.info("bf16_fused_spatial_last"), eng.info("bf16_fused_temporal_last")) == (1, 1)
        assert torch.equal(den1, den0) and torch.equal(y1, y0)
        assert torch.isfinite(y1).all()
        eng.set_option("fused_spatial", 0)                       # one block type at a time
        den2, y2 = _run(net, eng, T)
        assert (eng.info("bf16_fused_spatial_last"), eng.info("bf16_fused_temporal_last")) == (0, 1)
        assert torch.equal(den2, den0) and torch.equal(y2, y0)
    finally:
        _set(eng, True)


def test_refused_shape_keeps_the_two_kernel_flow():
    """embed_dim 192 / 3 heads: accepted by the bf16 engine, refused by the fused predicates: flags 0 whatever the options say, the
    result that of the options off, and the emulation gate of tests/test_gpu_bf16.py green."""
    from oracle import d3d_oracle as orc
    from helpers import torch_sd
    from test_gpu_bf16 import _emulations, _mpjpe, GATE_MAXABS, GATE_MPJPE
    T = 27
    net, _, eng = _model("refused", T)
    _set(eng, True)
    den1, y1 = _run(net, eng, T, B=2)
    assert (eng.info("bf16_fused_spatial_last"), eng.info("bf16_fused_temporal_last")) == (0, 0)
    _set(eng, False)
    den0, y0 = _run(net, eng, T, B=2)
    _set(eng, True)
    assert torch.equal(den1, den0) and torch.equal(y1, y0)
    cfg = DenoiserConfig(num_frame=T, embed_dim=192, depth=2, num_heads=3)
    inp = inputs(2, T, 310)
    xcat = torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1)
    t = torch.tensor([77, 508], dtype=torch.long)
    out = net.forward_denoise(xcat.cuda(), t.cuda())
    e32, e64, _ = _emulations(orc.forward_denoise, torch_sd(cfg, 21), xcat, t, depth=cfg.depth, heads=3)
    assert maxabs(out, e32) <= GATE_MAXABS and _mpjpe(out, e32) <= max(1.5 * _mpjpe(e32, e64), GATE_MPJPE)
    assert torch.isfinite(y1).all() and y1.abs().max().item() <= 1.0


def test_batch_independence_streams_graph_and_garbage_workspace():
    T = 81
    net, _, eng = _model("full", T)
    _set(eng, True)
    inp = inputs(3, T, 310)
    x2d, nz = inp["x2d"].cuda(), inp["noise"].cuda()
    eng.set_option("streams", 1)
    try:
        want = eng.ddim_sample(x2d, nz).clone()
        assert eng.info("bf16_fused_spatial_last") == 1 and eng.info("bf16_fused_temporal_last") == 1
        assert torch.equal(eng.ddim_sample(x2d[:1].contiguous(), nz[:1].contiguous()), want[:1])     # sequence 0 of B = 3 == the B = 1 call
        eng.set_option("streams", 2)
        assert torch.equal(eng.ddim_sample(x2d, nz), want)                                           # two streams == one
        eng._workspace(3).view(torch.float32).fill_(float("nan"))                                    # a stale read of w.QKV / pad rows shows
        assert torch.equal(eng.ddim_sample(x2d, nz), want)
        eng.set_graph_mode(True)
        assert torch.equal(eng.ddim_sample(x2d, nz), want) and torch.equal(eng.ddim_sample(x2d, nz), want)   # capture, then replay
        assert eng.info("graphs_cached") >= 1
        eng.set_option("fused_spatial", 0)                                                           # a flow switch drops the captured graphs
        assert eng.info("graphs_cached") == 0
        assert torch.equal(eng.ddim_sample(x2d, nz), want)
        assert eng.info("bf16_fused_spatial_last") == 0 and eng.info("graphs_cached") >= 1
    finally:
        eng.set_graph_mode(False)
        eng.set_option("streams", 2)
        _set(eng, True)


def test_f16x3_engine_is_untouched():
    """The two info keys stay 0 on an F16X3 engine and its outputs are the goldens' (the gate of tests/test_gpu_parity.py)."""
    g = gold("denoise_full_T27")
    net, diff = build_product(cfg_full(27), int(g["seed"]), precision="f16x3")
    eng = diff._engine(torch.device("cuda", torch.cuda.current_device()))
    inp = inputs(2, 27, int(g["input_seed"]))
    xcat = torch.cat([inp["x2d"], inp["noise"] * float(g["y_scale"])], dim=-1).cuda()
    for t in (999, 0):
        out = net.forward_denoise(xcat, torch.full((2,), t, dtype=torch.long, device="cuda"))
        assert maxabs(out, g[f"t{t}"]) <= 1e-4
    assert (eng.info("bf16_fused_spatial_last"), eng.info("bf16_fused_temporal_last")) == (0, 0)
