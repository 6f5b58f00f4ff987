"""Windows of more than 128 frames with heads of 128 columns on the MI355X ("attn_h128", kernels_attn_x3_long.hip k_attn_x3_stream<128, 4>):
embed_dim 1024 with the runner's 8 heads.  The keys of a head stream through LDS in chunks of 128 frames, the queries are cut into
balanced blocks of at most 8 waves, and the arithmetic is k_attn_x3_h128's in the same order.
  * op level: bit for bit op_attention_h128 wherever that runs (T <= 128: one chunk, one query block);
  * op level: windows of 129 .. 385 frames against fp64 math (one key in the second chunk, full and ragged last tiles, two full chunks,
    a third and a fourth chunk, two query blocks), every window length 1 .. 300, sharp softmax, isolation, refusal;
  * engine level against the fp64 oracle with the option on and off at the flagship window T = 243; the launches large enough for the
    dedicated fc1 and proj kernels at K = 1024; proof of the path through info("attn_h128_last").

Measured (MI355X), max-abs against fp64 (the generic fp32 kernel on the same input in brackets): T = 129 8.1e-7 (2.5e-6), 160 8.4e-7
(2.7e-6), 243 1.16e-6 (3.5e-6), 256 7.3e-7 (3.1e-6), 257 9.0e-7 (3.5e-6), 300 1.07e-6 (3.7e-6), 385 at two heads 7.4e-7 (4.2e-6); every
T = 1 .. 300: worst 9.6e-7 at T = 297; sharp softmax 1.4e-4 (2.2e-4, 2.5e-4 apart); engine against the oracle at T = 243, option on /
off: 3.8e-6 / 5.0e-6 (oracle fp32 floor 3.7e-6); B = 6: 3.3e-6."""
import pytest
import torch

from helpers import hashed, inputs, maxabs, attn_ref, torch_sd, product_with_engine, xy
from diff3dhpe_amd._lib import D3DError
from diff3dhpe_amd.spec import DenoiserConfig

pytestmark = pytest.mark.gpu
GATE = 1e-4
DEPTH = 1
KEY, LAST = "attn_h128", "attn_h128_last"


def _eng():
    from diff3dhpe_amd import engine
    return engine


def _bound_ok(err, err32):
    """The project's rule for an MFMA attention kernel: 5e-6, else 1.5 x the generic fp32 kernel's error on the same input."""
    return err < (5e-6 if err < 5e-6 else 1.5 * err32)


# ------------------------------------------------------------------------------------------------ 1. op level, bit identity
@pytest.mark.parametrize("B,T,J,D,H", [(1, 1, 17, 1024, 8), (2, 27, 3, 1024, 8), (1, 33, 2, 256, 2), (2, 81, 3, 1024, 8), (1, 128, 1, 1024, 8)])
def test_bit_identical_to_the_resident_kernel(B, T, J, D, H):
    E = _eng()
    qkv = hashed(f"qkv{T}_{J}_{D}", (B * T * J, 3 * D), 21, 2.0).cuda()
    want = E.op_attention_h128(qkv, B, T, J, H, True)
    got = E.op_attention_long_h128(qkv, B, T, J, H)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ 2. op level, long windows vs fp64
LONG = [(1, 129, 2, 1024, 8),   # one key in the second chunk
        (1, 160, 2, 1024, 8),   # a full last key tile
        (1, 243, 2, 1024, 8),   # the flagship window: 13 pad keys
        (1, 256, 2, 1024, 8),   # two full chunks, no mask, one full query block
        (1, 257, 2, 1024, 8),   # a third chunk of one key, a second query block (2 x 5 waves)
        (1, 300, 2, 1024, 8),
        (1, 385, 2, 256, 2)]    # a fourth chunk of one key, two heads


@pytest.mark.parametrize("B,T,J,D,H", LONG)
def test_long_windows_match_fp64(B, T, J, D, H):
    E = _eng()
    qkv = hashed(f"qkv{T}_{J}_{D}", (B * T * J, 3 * D), 21, 2.0).cuda()
    ref = attn_ref(qkv, B, T, J, H, True).cpu()
    got = E.op_attention_long_h128(qkv, B, T, J, H)
    err = maxabs(got, ref)
    err32 = maxabs(E.op_attention(qkv, B, T, J, H, True, force_generic=True), ref)
    print(f"attention_long_h128 B={B} T={T} J={J} D={D}: max-abs {err:.3e}; generic fp32 {err32:.3e}")
    assert torch.isfinite(got).all()
    assert _bound_ok(err, err32)


def test_every_window_length():
    """B = 1, one joint, one head: every T = 1 .. 300, so every pad-key count, chunk count and query-block split up to three chunks."""
    E = _eng()
    D, H = 128, 1
    full = hashed("everyN_300", (300, 3 * D), 21, 2.0).cuda()
    worst = (0.0, 0, 0.0)
    for N in range(1, 301):
        qkv = full[:N].contiguous()
        ref = attn_ref(qkv, 1, N, 1, H, True).cpu()
        got = E.op_attention_long_h128(qkv, 1, N, 1, H)
        assert torch.isfinite(got).all(), N
        err = maxabs(got, ref)
        err32 = maxabs(E.op_attention(qkv, 1, N, 1, H, True, force_generic=True), ref) if err >= 5e-6 else float("nan")
        if err > worst[0]:
            worst = (err, N, err32)
        assert _bound_ok(err, err32), (N, err, err32)
    print(f"attention_long_h128 every T = 1 .. 300: worst max-abs {worst[0]:.3e} at T = {worst[1]} (generic fp32 there: {worst[2]:.3e})")


def test_sharp_softmax_on_the_flagship_window():
    """Logits up to ~100: the bound of tests/test_gpu_ops.py::test_attention_fast_kernels_agree_with_generic_on_sharp_softmax."""
    E = _eng()
    B, T, J, D, H = 1, 243, 3, 1024, 8
    qkv = hashed(f"sharp{T}", (B * T * J, 3 * D), 22, 9.0).cuda()
    ref = attn_ref(qkv, B, T, J, H, True).cpu()
    a = E.op_attention_long_h128(qkv, B, T, J, H)
    b = E.op_attention(qkv, B, T, J, H, True, force_generic=True)
    print(f"attention_long_h128 sharp T={T}: new {maxabs(a, ref):.3e} generic {maxabs(b, ref):.3e} apart {maxabs(a, b.cpu()):.3e}")
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert maxabs(a, ref) < 2e-3 and maxabs(b, ref) < 2e-3
    assert maxabs(a, b.cpu()) < 2e-3


# ------------------------------------------------------------------------------------------------ 3. op level, isolation and refusal
@pytest.mark.parametrize("T", [243, 100])
def test_a_nan_batch_element_does_not_reach_its_neighbour(T):
    E = _eng()
    B, J, D, H = 2, 2, 1024, 8
    qkv = hashed(f"isoqkv{T}_{J}_{D}_{B}", (B * T * J, 3 * D), 21, 2.0).cuda()
    bad = qkv.clone()
    bad[T * J:] = float("nan")
    alone = E.op_attention_long_h128(qkv[:T * J].contiguous(), 1, T, J, H)
    both = E.op_attention_long_h128(bad, B, T, J, H)
    assert torch.isfinite(both[:T * J]).all()
    assert torch.equal(both[:T * J], alone)


def test_refuses_other_widths():
    T, D, H = 27, 512, 8
    qkv = torch.zeros((T * 2, 3 * D), device="cuda")
    with pytest.raises(D3DError, match="head_dim 128"):
        _eng().op_attention_long_h128(qkv, 1, T, 2, H)


# ------------------------------------------------------------------------------------------------ 4. engine level
def _cfg(T):
    return DenoiserConfig(num_frame=T, embed_dim=1024, depth=DEPTH, num_heads=8)


def _sd(cfg, seed=11):   # this module's weights: seed 11 of the trained-like family
    return torch_sd(cfg, seed, family="trainedlike")


def _product(cfg, seed=11, prec="f16x3", sampling=2):   # this module's defaults; the weights of _sd
    return product_with_engine(cfg, seed, prec, sampling, family="trainedlike")


def _oracle64(cfg, xcat, t):
    """(fp64 oracle output, max-abs distance of the fp32 oracle from it)."""
    from oracle import d3d_oracle as orc
    sd = _sd(cfg)
    ref32 = orc.forward_denoise(sd, xcat, t, depth=DEPTH)
    torch.set_default_dtype(torch.float64)      # (the oracle's sinusoid and identity follow the default dtype)
    try:
        ref64 = orc.forward_denoise({k: v.double() for k, v in sd.items()}, xcat.double(), t, depth=DEPTH)
    finally:
        torch.set_default_dtype(torch.float32)
    assert ref64.dtype == torch.float64
    return ref64, (ref32.double() - ref64).abs().max().item()


def test_forward_denoise_against_the_oracle_with_the_option_on_and_off():
    """forward_denoise at the flagship window T = 243, B = 2, trained-like weights, depth 1, per-row t, against oracle/d3d_oracle.py in
    fp64: the folded flow (spatial blocks resident, temporal blocks streaming: bits 0 and 2) and the plain row-kernel flow both inside the
    project's 1e-4 gate."""
    T = 243
    cfg = _cfg(T)
    net, _, eng = _product(cfg)
    inp = inputs(2, T, 500)
    xcat = torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1)
    t = torch.tensor([905, 17], dtype=torch.long)
    ref64, floor = _oracle64(cfg, xcat, t)
    default = eng.info(KEY)
    eng.range_flags(clear=True)
    err = {}
    try:
        for opt in (1, 0):
            eng.set_option(KEY, opt)
            out = net.forward_denoise(xcat.cuda(), t.cuda())
            assert eng.info(LAST) == (5 if opt else 0)
            err[opt] = (out.cpu().double() - ref64).abs().max().item()
    finally:
        eng.set_option(KEY, default)
    print(f"attn_h128 T={T} B=2: err_on {err[1]:.3e} err_off {err[0]:.3e} oracle fp32 floor {floor:.3e}")
    assert eng.range_flags() == 0
    assert err[1] <= GATE and err[0] <= GATE


def test_a_launch_large_enough_for_the_dedicated_fc1_and_proj_kernels():
    """B = 6 at T = 243: M = 24786 rows, 129 whole 192-row tiles x 4 column tiles = 516 >= 512, so proj runs kernels_proj_x3.hip and fc1
    kernels_fc1_x3.hip with K = 1024 (their only shapes so far: K = 512 and 256).  Finite, and the first batch element within the gate
    of the oracle's one-element forward."""
    T, B = 243, 6
    cfg = _cfg(T)
    net, _, eng = _product(cfg)
    assert (B * T * 17 // 192) * (1024 // 256) >= 512
    inp = inputs(B, T, 500)
    xcat = torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1)
    t = torch.tensor([905, 17, 444, 3, 999, 250], dtype=torch.long)
    ref64, floor = _oracle64(cfg, xcat[:1], t[:1])
    eng.set_option(KEY, 1)
    eng.range_flags(clear=True)
    out = net.forward_denoise(xcat.cuda(), t.cuda())
    assert eng.info(LAST) == 5
    assert torch.isfinite(out).all()
    err = (out[:1].cpu().double() - ref64).abs().max().item()
    print(f"attn_h128 T={T} B={B}: err of element 0 {err:.3e} oracle fp32 floor {floor:.3e}")
    assert eng.range_flags() == 0
    assert err <= GATE


def test_the_same_plan_beyond_256_frames():
    """T = 300 at B = 5 (132 whole 192-row tiles x 4 = 528): two query blocks, three chunks; bits 0 and 2."""
    T, B = 300, 5
    _, _, eng = _product(_cfg(T))
    assert (B * T * 17 // 192) * (1024 // 256) >= 512
    eng.set_option(KEY, 1)
    assert eng.info(LAST) == 0                         # before any forward
    out = eng.ddim_sample(*xy(B, T, 84))
    assert eng.info(LAST) == 5
    assert torch.isfinite(out).all()
    assert eng.range_flags() == 0
