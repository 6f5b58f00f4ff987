"""FP32 windows of more than 256 frames with heads of 32 columns on the MI355X ("long_temporal_f32_h32", kernels_attn_f32_h32_long.hip
k_attn_f32_stream3<32>): embed_dim 256 with the runner's 8 heads on an FP32 engine -- the exact mode, and the engine a precision-"auto"
model falls back to.  The keys of a unit stream through LDS in chunks of 256 frames, three passes (maximum, sum, normalised product), the
arithmetic of k_attn_temporal_f32_h32 in the same order.
  * op level: bit for bit op_attention_f32_h32 wherever that runs (T <= 256: every wave count, an odd head count, sharp softmax);
  * op level: windows of 257 .. 513 frames against fp64 math, bound max(5e-6, 2 e32) with e32 the generic kernel's error on the same input
    (the rule of tests/test_gpu_attn_f32_h32.py); sharp softmax; a NaN batch element does not reach its neighbour; refusals;
  * engine level against the fp64 oracle with the option on and off, invariances, graph replay, proof of the path through
    info("long_temporal_f32_h32_last"), a precision-"auto" model at this shape.

Measured (MI355X), max-abs against fp64 (e32, the generic kernel on the same input, in brackets): T = 257 8.1e-7 (3.3e-6), 288 7.4e-7
(4.2e-6), 300 1.06e-6 (4.1e-6), 512 1.31e-6 (4.9e-6), 513 7.4e-7 (4.9e-6), D = 64 8.1e-7 (2.9e-6), B = 3 x 17 joints 1.74e-6 (4.1e-6);
sharp softmax 9.1e-5 (1.1e-4, 1.3e-4 apart); engine against the oracle at T = 300, option on / off: 3.26e-6 / 3.18e-6 (oracle fp32 floor
1.56e-6)."""
import pytest
import torch

from helpers import hashed, inputs, maxabs, attn_ref, torch_sd, product_with_engine, xy
from diff3dhpe_amd._lib import D3DError
from diff3dhpe_amd.spec import DenoiserConfig

pytestmark = pytest.mark.gpu
GATE = 1e-4
FLOOR = 5e-6          # test_attention_core's bound for hashed qkv at scale 2.0
DEPTH = 1
KEY, LAST = "long_temporal_f32_h32", "long_temporal_f32_h32_last"


def _eng():
    from diff3dhpe_amd import engine
    return engine


# ------------------------------------------------------------------------------------------------ 1. op level, bit identity
# 8 / 8 / 3 / 2 / 1 / 5 waves; 13, 0, 15, 31, 31, 0 pad keys in the last tile; an odd head count
SAME = [(1, 243, 2, 256, 8), (1, 256, 1, 256, 8), (2, 81, 3, 256, 8), (1, 33, 2, 64, 2), (1, 1, 17, 256, 8), (1, 160, 1, 256, 8),
        (2, 27, 3, 96, 3)]


@pytest.mark.parametrize("B,T,J,D,H", SAME)
def test_bit_identical_to_the_resident_kernel(B, T, J, D, H):
    E = _eng()
    qkv = hashed(f"qkv{T}_{J}_{D}", (B * T * J, 3 * D), 21, 2.0).cuda()
    want = E.op_attention_f32_h32(qkv, B, T, J, H, True)
    got = E.op_attention_long_f32_h32(qkv, B, T, J, H)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)


def test_bit_identical_on_sharp_softmax():
    """Logits up to ~100 (near one-hot rows): the maximum of pass 1 and the -inf key mask."""
    E = _eng()
    B, T, J = 1, 243, 3
    qkv = hashed(f"sharp{T}", (B * T * J, 3 * 256), 22, 9.0).cuda()
    want = E.op_attention_f32_h32(qkv, B, T, J, 8, True)
    got = E.op_attention_long_f32_h32(qkv, B, T, J, 8)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ 2. op level, long windows vs fp64
LONG = [(1, 257, 2, 256, 8),    # one key in the second chunk, one query in the second block (2 x 5 waves of 160)
        (1, 288, 2, 256, 8),    # a full last key tile
        (1, 300, 2, 256, 8),
        (1, 512, 2, 256, 8),    # two full chunks, no mask, two full query blocks
        (1, 513, 2, 256, 8),    # a third chunk and a third query block
        (1, 300, 2, 64, 2),
        (3, 300, 17, 256, 8)]


@pytest.mark.parametrize("B,T,J,D,H", LONG)
def test_long_windows_match_fp64(B, T, J, D, H):
    """err <= max(5e-6, 2 e32), e32 the error of the generic one-thread-per-row fp32 kernel on the same input in the same run."""
    E = _eng()
    qkv = hashed(f"qkv{T}_{J}_{D}", (B * T * J, 3 * D), 21, 2.0).cuda()
    ref = attn_ref(qkv, B, T, J, H, True).cpu()
    got = E.op_attention_long_f32_h32(qkv, B, T, J, H)
    err = maxabs(got, ref)
    e32 = maxabs(E.op_attention(qkv, B, T, J, H, True, precision="fp32", force_generic=True), ref)
    print(f"attention_long_f32_h32 B={B} T={T} J={J} D={D}: max-abs {err:.3e}; generic fp32 {e32:.3e}")
    assert torch.isfinite(got).all()
    assert err <= max(FLOOR, 2 * e32)


def test_sharp_softmax_on_a_long_window():
    """Logits up to ~100: the bound of tests/test_gpu_ops.py::test_attention_fast_kernels_agree_with_generic_on_sharp_softmax."""
    E = _eng()
    B, T, J, D, H = 1, 300, 3, 256, 8
    qkv = hashed(f"sharp{T}", (B * T * J, 3 * D), 22, 9.0).cuda()
    ref = attn_ref(qkv, B, T, J, H, True).cpu()
    a = E.op_attention_long_f32_h32(qkv, B, T, J, H)
    b = E.op_attention(qkv, B, T, J, H, True, precision="fp32", force_generic=True)
    print(f"attention_long_f32_h32 sharp T={T}: new {maxabs(a, ref):.3e} generic {maxabs(b, ref):.3e} apart {maxabs(a, b.cpu()):.3e}")
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert maxabs(a, ref) < 2e-3 and maxabs(b, ref) < 2e-3
    assert maxabs(a, b.cpu()) < 2e-3


# ------------------------------------------------------------------------------------------------ 3. op level, isolation and refusals
def test_a_nan_batch_element_does_not_reach_its_neighbour():
    E = _eng()
    B, T, J, D, H = 2, 300, 2, 256, 8
    qkv = hashed(f"isoqkv{T}_{J}_{D}_{B}", (B * T * J, 3 * D), 21, 2.0).cuda()
    bad = qkv.clone()
    bad[T * J:] = float("nan")
    alone = E.op_attention_long_f32_h32(qkv[:T * J].contiguous(), 1, T, J, H)
    both = E.op_attention_long_f32_h32(bad, B, T, J, H)
    assert torch.isfinite(both[:T * J]).all()
    assert torch.equal(both[:T * J], alone)


@pytest.mark.parametrize("D,H", [(512, 8), (256, 4)])
def test_refuses_other_widths(D, H):
    T = 27
    qkv = torch.zeros((T * 2, 3 * D), device="cuda")
    with pytest.raises(D3DError, match="head_dim 32"):
        _eng().op_attention_long_f32_h32(qkv, 1, T, 2, H)


# ------------------------------------------------------------------------------------------------ 4. engine level
def _cfg(T, D=256, J=17):
    return DenoiserConfig(num_frame=T, num_joints=J, embed_dim=D, depth=DEPTH, num_heads=8)


def _sd(cfg, seed=11):   # this module's weights: seed 11 of the trained-like family
    return torch_sd(cfg, seed, family="trainedlike")


def _product(cfg, seed=11, prec="fp32", sampling=2):   # this module's defaults; the weights of _sd
    return product_with_engine(cfg, seed, prec, sampling, family="trainedlike")


def _sample(eng, x2d, nz, opt=1):   # toggles the option, reads the proof-of-path key and puts the option back
    default = eng.info(KEY)
    eng.set_option(KEY, opt)
    try:
        out = eng.ddim_sample(x2d, nz).clone()
        last = eng.info(LAST)
    finally:
        eng.set_option(KEY, default)
    return out, last


def test_forward_denoise_against_the_oracle_with_the_option_on_and_off():
    """forward_denoise of an FP32 engine at T = 300, B = 2, trained-like weights, depth 1, per-row t, against oracle/d3d_oracle.py in
    fp64: the key-streaming kernel of this width and the generic kernel both inside the project's 1e-4 gate."""
    from oracle import d3d_oracle as orc
    T = 300
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
    default = eng.info(KEY)
    err = {}
    try:
        for opt in (1, 0):
            eng.set_option(KEY, opt)
            out = net.forward_denoise(xcat.cuda(), t.cuda())
            assert eng.info(LAST) == opt
            assert eng.info("attn_f32_h32_last") == 1      # the spatial blocks (17 joints) alone
            err[opt] = (out.cpu().double() - ref64).abs().max().item()
    finally:
        eng.set_option(KEY, default)
    print(f"long_temporal_f32_h32 T={T} B=2: err_on {err[1]:.3e} err_off {err[0]:.3e} oracle fp32 floor {floor:.3e}")
    assert err[1] <= GATE and err[0] <= GATE


def test_rows_do_not_depend_on_batch_streams_workspace_contents_or_graph_replay():
    T, B = 257, 3
    _, _, eng = _product(_cfg(T))
    default = eng.info(KEY)
    eng.set_option(KEY, 1)
    try:
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
            first = eng.ddim_sample(x2d, nz).clone()   # eager warm-up pass + capture + replay
            l1 = eng.info(LAST)
            again = eng.ddim_sample(x2d, nz).clone()   # replay of the cached graph
            assert eng.info("graphs_cached") >= 1
        finally:
            eng.set_graph_mode(False)
        assert l1 == 1
        assert torch.equal(first, whole) and torch.equal(again, whole)
    finally:
        eng.set_option(KEY, default)


# ------------------------------------------------------------------------------------------------ 5. path selection
def test_other_joint_counts_leave_the_spatial_blocks_on_the_generic_kernel():
    T, J = 300, 21
    _, _, eng = _product(_cfg(T, J=J))
    assert eng.info(LAST) == 0                         # before any forward
    out, last = _sample(eng, *xy(1, T, 83, J))
    assert last == 1 and eng.info("attn_f32_h32_last") == 0 and torch.isfinite(out).all()


def test_windows_up_to_256_never_take_the_long_kernel_and_ignore_the_option():
    T = 243
    _, _, eng = _product(_cfg(T))
    x2d, nz = xy(2, T, 82)
    on, l_on = _sample(eng, x2d, nz, 1)
    off, l_off = _sample(eng, x2d, nz, 0)
    assert (l_on, l_off) == (0, 0)
    assert torch.isfinite(on).all() and torch.equal(on, off)


def test_heads_of_64_columns_keep_their_own_long_kernel():
    T = 300
    _, _, eng = _product(_cfg(T, D=512))
    out, last = _sample(eng, *xy(1, T, 83))
    assert last == 0 and eng.info("long_temporal_f32_last") == 1 and torch.isfinite(out).all()


def test_an_auto_model_samples_on_its_f16x3_engine():
    """precision "auto" at T = 300, embed_dim 256 with ordinary weights and inputs: the guard stays quiet, the model stays on its F16X3
    engine, and that engine's temporal blocks run the key-streaming F16X3 kernel of this width."""
    T = 300
    cfg = _cfg(T)
    net, diff, eng = _product(cfg, prec="auto")
    default = eng.info("long_temporal_h32")
    eng.set_option("long_temporal_h32", 1)             # (whatever the default is)
    try:
        x2d, nz = xy(1, T, 81)
        out = diff.ddim_sample_loop(x2d, tuple(nz.shape), init_noise=nz)
        assert out.shape == nz.shape and torch.isfinite(out).all()
        assert not net._on_fallback()
        assert eng.info("long_temporal_h32_last") == 1 and eng.info(LAST) == 0
    finally:
        eng.set_option("long_temporal_h32", default)
