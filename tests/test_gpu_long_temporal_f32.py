"""FP32 windows of more than 256 frames on the MI355X ("long_temporal_f32", kernels_attn_f32_long.hip k_attn_f32_stream3<64>): the keys of a
unit stream through LDS in chunks of 256 frames, the queries are cut into balanced blocks of at most 8 waves, and the arithmetic is that of
k_attn_temporal_f32 (v_mfma_f32_32x32x2_f32, softmax normalised before the second product) in the same order, in three passes.
  * op level: bit for bit the resident kernel wherever that runs (T <= 256: one chunk, one query block, every wave count);
  * op level: windows of 257 .. 513 frames against fp64 math (one key in the second chunk, full and ragged last tiles, two full chunks,
    a third chunk; two and three query blocks of uneven fill);
  * row isolation at op and engine level; graph replay == eager;
  * engine level against the fp64 oracle with the option on and off; proof of the path through info("long_temporal_f32_last");
  * the default precision ("auto") reaches the kernel through its fp32 fallback engine."""
import warnings

import pytest
import torch

from helpers import hashed, inputs, maxabs, attn_ref, torch_sd, build_net, product_with_engine, xy
from diff3dhpe_amd.spec import DenoiserConfig

pytestmark = pytest.mark.gpu
GATE = 1e-4
DEPTH = 1
KEY, LAST = "long_temporal_f32", "long_temporal_f32_last"


def _eng():
    from diff3dhpe_amd import engine
    return engine


# ------------------------------------------------------------------------------------------------ 1. op level, bit identity
# 8 / 8 / 3 / 2 / 1 / 5 waves; 13, 0, 15, 31, 31, 0 pad keys in the last tile
SAME = [(1, 243, 2, 512, 8), (1, 256, 1, 512, 8), (2, 81, 3, 512, 8), (1, 33, 2, 128, 2), (1, 1, 17, 512, 8), (1, 160, 1, 512, 8)]


@pytest.mark.parametrize("B,T,J,D,H", SAME)
def test_bit_identical_to_the_resident_kernel(B, T, J, D, H):
    E = _eng()
    qkv = hashed(f"qkv{T}_{J}_{D}", (B * T * J, 3 * D), 21, 2.0).cuda()
    want = E.op_attention(qkv, B, T, J, H, True)
    got = E.op_attention_long_f32(qkv, B, T, J, H)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)


def test_bit_identical_on_sharp_softmax():
    """Logits up to ~100 (near one-hot rows): the maximum of pass 1 and the -inf key mask."""
    E = _eng()
    B, T, J = 1, 243, 3
    qkv = hashed(f"sharp{T}", (B * T * J, 3 * 512), 22, 9.0).cuda()
    want = E.op_attention(qkv, B, T, J, 8, True)
    got = E.op_attention_long_f32(qkv, B, T, J, 8)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ 2. op level, long windows vs fp64
LONG = [(1, 257, 2, 512, 8),    # one key in the second chunk, one query in the second block (2 x 5 waves of 160)
        (1, 288, 2, 512, 8),    # a full last key tile
        (1, 300, 2, 512, 8),
        (1, 512, 2, 512, 8),    # two full chunks, no mask, two full query blocks
        (1, 513, 2, 512, 8),    # a third chunk and a third query block
        (1, 300, 2, 128, 2),
        (3, 300, 17, 512, 8)]


@pytest.mark.parametrize("B,T,J,D,H", LONG)
def test_long_windows_match_fp64(B, T, J, D, H):
    """5e-6: the bound tests/test_gpu_ops.py::test_attention_core holds the resident fp32 kernel to on the same input family.  Plain fp32
    attention already differs from fp64 by 3.4 - 4.4e-6 on these inputs, so where a long shape misses 5e-6 the bound of that shape is
    1.5 x the error of the generic fp32 kernel (existing code, an equally ordered fp32 sum) on the same input."""
    E = _eng()
    qkv = hashed(f"qkv{T}_{J}_{D}", (B * T * J, 3 * D), 21, 2.0).cuda()
    ref = attn_ref(qkv, B, T, J, H, True).cpu()
    got = E.op_attention_long_f32(qkv, B, T, J, H)
    err = maxabs(got, ref)
    err32 = maxabs(E.op_attention(qkv, B, T, J, H, True, force_generic=True), ref)
    print(f"attention_long_f32 B={B} T={T} J={J} D={D}: max-abs {err:.3e}; generic fp32 {err32:.3e}")
    assert torch.isfinite(got).all()
    assert err < (5e-6 if err < 5e-6 else 1.5 * err32)


# ------------------------------------------------------------------------------------------------ 3. op level, isolation
def test_a_nan_batch_element_does_not_reach_its_neighbour():
    E = _eng()
    B, T, J, D, H = 2, 300, 2, 512, 8
    qkv = hashed(f"isoqkv{T}_{J}_{D}_{B}", (B * T * J, 3 * D), 21, 2.0).cuda()
    bad = qkv.clone()
    bad[T * J:] = float("nan")
    alone = E.op_attention_long_f32(qkv[:T * J].contiguous(), 1, T, J, H)
    both = E.op_attention_long_f32(bad, B, T, J, H)
    assert torch.isfinite(both[:T * J]).all()
    assert torch.equal(both[:T * J], alone)


# ------------------------------------------------------------------------------------------------ 4. engine level
def _cfg(T):
    return DenoiserConfig(num_frame=T, embed_dim=512, depth=DEPTH)


def _sd(cfg, seed=11):   # this module's weights: seed 11 of the trained-like family
    return torch_sd(cfg, seed, family="trainedlike")


def _net(cfg, seed=11, prec="fp32"):
    return build_net(cfg, seed, prec, family="trainedlike")


def _product(cfg, seed=11, prec="fp32", sampling=2):   # this module's defaults; the weights of _sd
    return product_with_engine(cfg, seed, prec, sampling, family="trainedlike")


def _sample(eng, x2d, nz, long=1):   # toggles this feature's option KEY and reads LAST
    eng.set_option(KEY, long)
    out = eng.ddim_sample(x2d, nz).clone()
    last = eng.info(LAST)
    eng.set_option(KEY, 1)
    return out, last


@pytest.mark.parametrize("T", [257, 300])
def test_forward_denoise_against_the_oracle_with_the_option_on_and_off(T):
    """forward_denoise of an FP32 engine at B = 2, trained-like weights, depth 1, per-row t, against oracle/d3d_oracle.py in fp64: the
    key-streaming attention and the generic kernel both inside the project's 1e-4 gate."""
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
    err = {}
    for opt in (1, 0):
        eng.set_option(KEY, opt)
        out = net.forward_denoise(xcat.cuda(), t.cuda())
        assert eng.info(LAST) == opt
        assert eng.info("long_temporal_last") == 0
        err[opt] = (out.cpu().double() - ref64).abs().max().item()
    eng.set_option(KEY, 1)
    print(f"long_temporal_f32 T={T} B=2: err_on {err[1]:.3e} err_off {err[0]:.3e} oracle fp32 floor {floor:.3e}")
    assert err[1] <= GATE and err[0] <= GATE


# ------------------------------------------------------------------------------------------------ 5. independence
def test_rows_do_not_depend_on_batch_streams_workspace_contents_or_graph_replay():
    T, B = 257, 3
    _, _, eng = _product(_cfg(T))
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


# ------------------------------------------------------------------------------------------------ 6. path proof
def test_windows_up_to_256_never_take_the_long_kernel_and_ignore_the_option():
    T = 243
    _, _, eng = _product(_cfg(T))
    x2d, nz = xy(2, T, 82)
    on, l_on = _sample(eng, x2d, nz, long=1)
    off, l_off = _sample(eng, x2d, nz, long=0)
    assert (l_on, l_off) == (0, 0)
    assert torch.isfinite(on).all() and torch.equal(on, off)


def test_f16x3_engines_are_left_alone():
    """Neither flow of an F16X3 engine at T = 300 -- the folded one on the key-streaming F16X3 kernel, the plain one "long_temporal" = 0
    selects -- takes the fp32 long kernel."""
    T = 300
    _, _, e3 = _product(_cfg(T), prec="f16x3")
    x2d, nz = xy(1, T, 83)
    assert e3.info(KEY) == 1 and e3.info(LAST) == 0
    for flow in (1, 0):
        e3.set_option("long_temporal", flow)
        out = e3.ddim_sample(x2d, nz)
        assert torch.isfinite(out).all()
        assert e3.info("long_temporal_last") == flow and e3.info(LAST) == 0
    e3.set_option("long_temporal", 1)


# ------------------------------------------------------------------------------------------------ 7. the default precision
def test_the_auto_fallback_engine_runs_the_long_kernel():
    """precision "auto" at T = 300: an input scaled past the plane range raises the F16X3 guard, the call is repeated on the exact-fp32
    engine -- ONE warning, the fp32 model's result bit for bit, and that engine's temporal blocks on the key-streaming fp32 kernel."""
    T, B = 300, 2
    cfg = _cfg(T)
    net = _net(cfg, prec="auto").cuda()
    net32 = _net(cfg, prec="fp32").cuda()
    x2d, nz = xy(B, T, 81)
    big = torch.cat([x2d * 1.0e6, nz], dim=-1)
    t = torch.arange(B, device="cuda") * 300 + 11
    want = net32.forward_denoise(big, t).clone()
    with warnings.catch_warnings(record=True) as wlog:
        warnings.simplefilter("always")
        got = net.forward_denoise(big, t).clone()
    ours = [w for w in wlog if issubclass(w.category, RuntimeWarning)]
    assert len(ours) == 1 and "range guard fired" in str(ours[0].message), [str(w.message) for w in wlog]
    assert torch.equal(got, want)
    dev = torch.device("cuda", torch.cuda.current_device())
    assert net._on_fallback()
    assert net.engine_for(dev, True).info(LAST) == 1
    assert net32.engine_for(dev).info(LAST) == 1
