"""F16X3 attention for heads of 32 columns on the MI355X ("attn_h32", kernels_attn_x3_h32.hip k_attn_x3_h32): embed_dim 256 with the
runner's 8 heads.  Two adjacent heads share the 128-byte LDS rows of the 64-wide kernels; each has its own scores, softmax and sum.
  * op level against fp64 math: every key-tile count of the ladder, pad keys, one head pair, spatial and temporal groups;
  * sharp softmax; launch forms bit-identical; a NaN batch element does not reach its neighbour; refusals;
  * engine level against the fp64 oracle with the option on and off, invariances, proof of the path through info("attn_h32_last")."""
import pytest
import torch

from helpers import hashed, inputs, maxabs, attn_ref, torch_sd, product_with_engine, xy
from diff3dhpe_amd._lib import D3DError
from diff3dhpe_amd.spec import DenoiserConfig

pytestmark = pytest.mark.gpu
GATE = 1e-4
DEPTH = 1


def _eng():
    from diff3dhpe_amd import engine
    return engine


# ------------------------------------------------------------------------------------------------ 1. op level against fp64
# temporal: 1 / 1 / 1 / 2 / 3 / 5 / 8 / 8 key tiles (31, 5, 0, 31, 15, 0, 13, 0 pad keys in the last); spatial: 1 key tile.  With
# test_launch_forms_agree (the multi-unit form) and the T = 100 / 180 / 200 cases (4, 6, 7 key tiles) every form of the ladder is reached.
CASES = [(1, 1, 17, 256, 8, True), (2, 27, 3, 256, 8, True), (1, 32, 2, 64, 2, True), (1, 33, 2, 64, 2, True), (2, 81, 3, 256, 8, True),
         (1, 160, 1, 256, 8, True), (1, 243, 2, 256, 8, True), (1, 256, 1, 256, 8, True),
         (2, 5, 17, 256, 8, False), (3, 23, 15, 256, 8, False), (2, 5, 16, 64, 2, False),
         (1, 100, 1, 256, 8, True), (1, 180, 1, 256, 8, True), (1, 200, 1, 256, 8, True)]


@pytest.mark.parametrize("B,T,J,D,H,temporal", CASES)
def test_op_matches_fp64(B, T, J, D, H, temporal):
    """5e-6, the bound of tests/test_gpu_long_temporal.py; where a shape misses it, 1.5 x the error of the generic fp32 kernel on the same
    input in the same run."""
    E = _eng()
    qkv = hashed(f"qkv{T}_{J}_{D}", (B * T * J, 3 * D), 21, 2.0).cuda()
    ref = attn_ref(qkv, B, T, J, H, temporal).cpu()
    got = E.op_attention_h32(qkv, B, T, J, H, temporal)
    err = maxabs(got, ref)
    err32 = maxabs(E.op_attention(qkv, B, T, J, H, temporal, force_generic=True), ref)
    print(f"attention_h32 B={B} T={T} J={J} D={D} H={H} temporal={int(temporal)}: max-abs {err:.3e}; generic fp32 {err32:.3e}")
    assert torch.isfinite(got).all()
    assert err < (5e-6 if err < 5e-6 else 1.5 * err32)


# ------------------------------------------------------------------------------------------------ 2. sharp softmax
@pytest.mark.parametrize("B,T,J,temporal", [(2, 7, 17, False), (1, 243, 3, True)])
def test_sharp_softmax(B, T, J, temporal):
    """Logits up to ~100 (near one-hot rows): the bound of tests/test_gpu_ops.py::test_attention_fast_kernels_agree_with_generic_on_sharp_softmax."""
    E = _eng()
    qkv = hashed(f"sharp{T}", (B * T * J, 3 * 256), 22, 9.0).cuda()
    ref = attn_ref(qkv, B, T, J, 8, temporal).cpu()
    a = E.op_attention_h32(qkv, B, T, J, 8, temporal)
    b = E.op_attention(qkv, B, T, J, 8, temporal, force_generic=True)
    print(f"attention_h32 sharp T={T} J={J}: h32 {maxabs(a, ref):.3e} generic {maxabs(b, ref):.3e} apart {maxabs(a, b.cpu()):.3e}")
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert maxabs(a, ref) < 2e-3 and maxabs(b, ref) < 2e-3
    assert maxabs(a, b.cpu()) < 2e-3


# ------------------------------------------------------------------------------------------------ 3. launch forms
def test_launch_forms_agree():
    """Spatial, 1031 groups of 17 joints x 4 head pairs = 4124 units: eight units per workgroup (from 4096 units on), the last workgroup
    with surplus waves.  Its first and last groups, run as launches of one unit per workgroup, give the same bits."""
    E = _eng()
    G, J, D, H = 1031, 17, 256, 8
    qkv = hashed(f"forms{G}_{J}_{D}", (G * J, 3 * D), 21, 2.0).cuda()
    big = E.op_attention_h32(qkv, 1, G, J, H, False)
    assert torch.isfinite(big).all()
    for lo, hi in ((0, 2), (G - 3, G)):
        small = E.op_attention_h32(qkv[lo * J:hi * J].contiguous(), 1, hi - lo, J, H, False)
        assert torch.equal(small, big[lo * J:hi * J])
    err = maxabs(big[:4 * J], attn_ref(qkv[:4 * J], 1, 4, J, H, False).cpu())
    assert err < 5e-6, err


# ------------------------------------------------------------------------------------------------ 4. isolation
@pytest.mark.parametrize("T,J,temporal", [(243, 2, True), (5, 17, False)])
def test_a_nan_batch_element_does_not_reach_its_neighbour(T, J, temporal):
    E = _eng()
    B, D, H = 2, 256, 8
    qkv = hashed(f"isoqkv{T}_{J}_{D}_{B}", (B * T * J, 3 * D), 21, 2.0).cuda()
    bad = qkv.clone()
    bad[T * J:] = float("nan")
    alone = E.op_attention_h32(qkv[:T * J].contiguous(), 1, T, J, H, temporal)
    both = E.op_attention_h32(bad, B, T, J, H, temporal)
    assert torch.isfinite(both[:T * J]).all()
    assert torch.equal(both[:T * J], alone)


# ------------------------------------------------------------------------------------------------ 5. refusal
@pytest.mark.parametrize("T,D,H", [(27, 512, 8), (27, 96, 3), (257, 256, 8)])
def test_refuses_other_widths_odd_head_counts_and_long_windows(T, D, H):
    qkv = torch.zeros((T * 2, 3 * D), device="cuda")
    with pytest.raises(D3DError, match="head_dim 32"):
        _eng().op_attention_h32(qkv, 1, T, 2, H, True)


# ------------------------------------------------------------------------------------------------ 6. - 8. engine level
def _cfg(T, D=256, H=8):
    return DenoiserConfig(num_frame=T, embed_dim=D, depth=DEPTH, num_heads=H)


def _sd(cfg, seed=11):   # this module's weights: seed 11 of the trained-like family
    return torch_sd(cfg, seed, family="trainedlike")


def _product(cfg, seed=11, prec="f16x3", sampling=2):   # this module's defaults; the weights of _sd
    return product_with_engine(cfg, seed, prec, sampling, family="trainedlike")


def _sample(eng, x2d, nz):   # reads this feature's proof-of-path key, "attn_h32_last"
    out = eng.ddim_sample(x2d, nz).clone()
    return out, eng.info("attn_h32_last")


@pytest.mark.parametrize("T", [27, 243])
def test_forward_denoise_against_the_oracle_with_the_option_on_and_off(T):
    """forward_denoise at B = 2, trained-like weights, depth 1, per-row t, against oracle/d3d_oracle.py in fp64: the folded flow with the
    head-width-32 attention and the plain row-kernel flow both inside the project's 1e-4 gate."""
    from oracle import d3d_oracle as orc
    cfg = _cfg(T)
    net, _, eng = _product(cfg)
    sd = _sd(cfg)
    inp = inputs(2, T, 500)
    xcat = torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1)
    t = torch.tensor([905, 17], dtype=torch.long)
    ref32 = orc.forward_denoise(sd, xcat, t, depth=DEPTH)
    torch.set_default_dtype(torch.float64)      # (the oracle's sinusoid and identity follow the default dtype)
    try:
        ref64 = orc.forward_denoise({k: v.double() for k, v in sd.items()}, xcat.double(), t, depth=DEPTH)
    finally:
        torch.set_default_dtype(torch.float32)
    assert ref64.dtype == torch.float64
    floor = (ref32.double() - ref64).abs().max().item()
    default = eng.info("attn_h32")
    eng.range_flags(clear=True)
    err = {}
    try:
        for opt in (1, 0):
            eng.set_option("attn_h32", opt)
            out = net.forward_denoise(xcat.cuda(), t.cuda())
            assert eng.info("attn_h32_last") == opt
            err[opt] = (out.cpu().double() - ref64).abs().max().item()
    finally:
        eng.set_option("attn_h32", default)
    print(f"attn_h32 T={T} B=2: err_on {err[1]:.3e} err_off {err[0]:.3e} oracle fp32 floor {floor:.3e}")
    assert eng.range_flags() == 0
    assert err[1] <= GATE and err[0] <= GATE


def test_rows_do_not_depend_on_batch_streams_workspace_contents_or_graph_replay():
    T, B = 27, 3
    _, _, eng = _product(_cfg(T))
    eng.set_option("attn_h32", 1)
    x2d, nz = xy(B, T, 80)
    eng.set_option("streams", 2)
    whole, last = _sample(eng, x2d, nz)
    assert last == 1 and torch.isfinite(whole).all()
    for b in range(B):
        one, last = _sample(eng, x2d[b:b + 1].contiguous(), nz[b:b + 1].contiguous())
        assert last == 1 and torch.equal(one, whole[b:b + 1])
    eng.set_option("streams", 1)
    assert torch.equal(_sample(eng, x2d, nz)[0], whole)
    eng.set_option("streams", 2)
    eng._workspace(B).view(torch.float32).fill_(float("nan"))
    assert torch.equal(_sample(eng, x2d, nz)[0], whole)
    eng.set_graph_mode(True)
    try:
        first, l1 = _sample(eng, x2d, nz)          # eager warm-up pass + capture + replay
        again = eng.ddim_sample(x2d, nz).clone()   # replay of the cached graph
        assert eng.info("graphs_cached") >= 1
    finally:
        eng.set_graph_mode(False)
    assert l1 == 1
    assert torch.equal(first, whole) and torch.equal(again, whole)


@pytest.mark.parametrize("T,D,H,prec", [(27, 512, 8, "f16x3"), (27, 256, 4, "f16x3"), (300, 256, 8, "f16x3"), (27, 256, 8, "fp32")])
def test_other_engines_never_take_the_kernel(T, D, H, prec):
    """Heads of 64 columns, windows of more than 256 frames at this width (still the plain flow) and FP32 engines, with the option on."""
    _, _, eng = _product(_cfg(T, D, H), prec=prec)
    eng.set_option("attn_h32", 1)
    assert eng.info("attn_h32_last") == 0              # before any forward
    x2d, nz = xy(1, T, 83)
    out, last = _sample(eng, x2d, nz)
    assert last == 0 and torch.isfinite(out).all()
