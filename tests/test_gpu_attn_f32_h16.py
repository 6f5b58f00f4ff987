"""Head width 16 on the MI355X, op level, exact fp32 (v_mfma_f32_32x32x2_f32): the DH = 16 walks of kernels_attn_f32_hx.hip --
k_attn_f32_hx<16, NKT> for groups of up to 256 tokens and the two-pass key-streaming k_attn_f32_hx_stream<16>, any head count.  The one
32 x 32 accumulator tile of O^T is half used: its upper 16 rows span the NEXT head's columns, whose V must never be staged (the LDS rows
hold zeros there) and which must never be stored.
  * the resident kernel against fp64 math: key-tile counts 1, 2, 3, 8, pad keys, 1 / 3 / 8 heads, spatial and temporal groups, every
    group length N = 1 .. 256;
  * a NaN head between two clean ones (resident and streaming), a NaN batch element, sharp softmax, refusals;
  * the streaming kernel against fp64 math beyond 256 frames, and bit for bit the resident kernel up to 256.
The engines of this width are in tests/test_gpu_attn_h16_engine.py.

Measured (MI355X), max-abs against fp64 (the generic fp32 kernel on the same input in brackets): the resident kernel 0 (T = 1) ..
6.6e-7 over its eight shapes (worst at T = 81: generic 1.9e-6; T = 256, one head: 4.1e-7 against 2.6e-6); every N = 1 .. 256: worst
6.2e-7 at N = 240; sharp softmax 5.5e-5 / 8.3e-5 (generic 4.3e-5 / 6.2e-5, up to 7.8e-5 apart); the streaming kernel 3.2e-7 .. 6.5e-7
over T = 257, 300, 513 and 300 at 8 heads (2.5e-6 .. 4.0e-6).  The module's 33 cases: 1.4 s."""
import pytest
import torch

from helpers import hashed, maxabs, attn_ref
from diff3dhpe_amd._lib import D3DError

pytestmark = pytest.mark.gpu
DH = 16


def _eng():
    from diff3dhpe_amd import engine
    return engine


def _bound_ok(err, err32):
    """The project's rule for an MFMA attention kernel (tests/test_gpu_attn_hx.py): 5e-6, else 1.5 x the generic fp32 kernel's error on
    the same input."""
    return err < (5e-6 if err < 5e-6 else 1.5 * err32)


# ------------------------------------------------------------------------------------------------ 1. resident kernel against fp64
# the cases of tests/test_gpu_attn_h16.py with head counts 8, 3 and 1: key tiles 1 / 1 / 1 / 2 / 3 / 8; spatial: one key tile
CASES = [(1, 1, 17, 128, 8, True), (2, 27, 3, 128, 8, True), (1, 32, 2, 48, 3, True), (1, 33, 2, 48, 3, True), (2, 81, 3, 128, 8, True),
         (1, 256, 1, 16, 1, True), (2, 5, 17, 128, 8, False), (3, 23, 15, 16, 1, False)]


@pytest.mark.parametrize("B,T,J,D,H,temporal", CASES)
def test_op_matches_fp64(B, T, J, D, H, temporal):
    E = _eng()
    qkv = hashed(f"qkv{T}_{J}_{D}", (B * T * J, 3 * D), 21, 2.0).cuda()
    ref = attn_ref(qkv, B, T, J, H, temporal).cpu()
    got = E.op_attention_f32_h16(qkv, B, T, J, H, temporal)
    generic = E.op_attention(qkv, B, T, J, H, temporal, force_generic=True)
    err, err32 = maxabs(got, ref), maxabs(generic, ref)
    print(f"attention_f32_h16 B={B} T={T} J={J} D={D} H={H} temporal={int(temporal)}: max-abs {err:.3e}; generic fp32 {err32:.3e}")
    assert torch.isfinite(got).all()
    assert _bound_ok(err, err32)


def test_every_group_length():
    """B = 1, one joint, one head: every N = 1 .. 256, so every pad-key count of every key-tile count."""
    E = _eng()
    D, H, NMAX = DH, 1, 256
    full = hashed(f"everyN_{NMAX}_{DH}", (NMAX, 3 * D), 21, 2.0).cuda()
    worst = (0.0, 0, 0.0)
    for N in range(1, NMAX + 1):
        qkv = full[:N].contiguous()
        ref = attn_ref(qkv, 1, N, 1, H, True).cpu()
        got = E.op_attention_f32_h16(qkv, 1, N, 1, H, True)
        assert torch.isfinite(got).all(), N
        err = maxabs(got, ref)
        err32 = maxabs(E.op_attention(qkv, 1, N, 1, H, True, force_generic=True), ref) if err >= 5e-6 else float("nan")
        if err > worst[0]:
            worst = (err, N, err32)
        assert _bound_ok(err, err32), (N, err, err32)
    print(f"attention_f32_h16 every N = 1 .. {NMAX}: worst max-abs {worst[0]:.3e} at N = {worst[1]} (generic fp32 there: {worst[2]:.3e})")


# ------------------------------------------------------------------------------------------------ 2. isolation
def _ops():
    E = _eng()
    return {"resident": lambda q, B, T, J, H: E.op_attention_f32_h16(q, B, T, J, H, True), "streaming": E.op_attention_long_f32_h16}


@pytest.mark.parametrize("op", ["resident", "streaming"])
def test_a_nan_head_does_not_reach_its_neighbours(op):
    """Three heads (D = 48), head 1's q, k and v columns NaN.  The upper half of head 0's accumulator tile spans head 1's columns: the
    kernel stages zeros there and never stores those rows.  Heads 0 and 2 must be finite and carry the bits of the clean run."""
    B, T, J, H = 1, 40, 2, 3
    D = DH * H
    run = _ops()[op]
    qkv = hashed(f"headiso_f32_{DH}", (B * T * J, 3 * D), 21, 2.0).cuda()
    bad = qkv.clone()
    for third in range(3):
        bad[:, third * D + DH:third * D + 2 * DH] = float("nan")
    clean, got = run(qkv, B, T, J, H), run(bad, B, T, J, H)
    ref = attn_ref(qkv, B, T, J, H, True).cpu()
    assert maxabs(clean, ref) < 5e-6
    for hd in (0, 2):
        cols = slice(hd * DH, (hd + 1) * DH)
        assert torch.isfinite(got[:, cols]).all(), hd
        assert torch.equal(got[:, cols], clean[:, cols]), hd


@pytest.mark.parametrize("T,J,temporal", [(100, 2, True), (5, 17, False)])
def test_a_nan_batch_element_does_not_reach_its_neighbour(T, J, temporal):
    E = _eng()
    B, H = 2, 8
    D = DH * H
    qkv = hashed(f"isoqkv{T}_{J}_{D}_{B}", (B * T * J, 3 * D), 21, 2.0).cuda()
    bad = qkv.clone()
    bad[T * J:] = float("nan")
    alone = E.op_attention_f32_h16(qkv[:T * J].contiguous(), 1, T, J, H, temporal)
    both = E.op_attention_f32_h16(bad, B, T, J, H, temporal)
    assert torch.isfinite(both[:T * J]).all()
    assert torch.equal(both[:T * J], alone)


# ------------------------------------------------------------------------------------------------ 3. sharp softmax
@pytest.mark.parametrize("B,T,J,temporal", [(2, 7, 17, False), (1, 100, 3, True)])
def test_sharp_softmax(B, T, J, temporal):
    """The scaling and the bound of tests/test_gpu_attn_hx.py::test_sharp_softmax."""
    E = _eng()
    qkv = hashed(f"sharp{T}", (B * T * J, 3 * DH * 8), 22, 9.0).cuda()
    ref = attn_ref(qkv, B, T, J, 8, temporal).cpu()
    a = E.op_attention_f32_h16(qkv, B, T, J, 8, temporal)
    b = E.op_attention(qkv, B, T, J, 8, temporal, force_generic=True)
    print(f"attention_f32_h16 sharp T={T} J={J}: h16 {maxabs(a, ref):.3e} generic {maxabs(b, ref):.3e} apart {maxabs(a, b.cpu()):.3e}")
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert maxabs(a, ref) < 2e-3 and maxabs(b, ref) < 2e-3
    assert maxabs(a, b.cpu()) < 2e-3


# ------------------------------------------------------------------------------------------------ 4. refusal
@pytest.mark.parametrize("T,D,H", [(27, 256, 8), (27, 384, 8), (27, 512, 8), (257, 128, 8)])
def test_resident_op_refuses_other_widths_and_long_windows(T, D, H):
    qkv = torch.zeros((T * 2, 3 * D), device="cuda")
    with pytest.raises(D3DError, match="head_dim 16"):
        _eng().op_attention_f32_h16(qkv, 1, T, 2, H, True)


@pytest.mark.parametrize("D,H", [(256, 8), (384, 8), (512, 8)])
def test_streaming_op_refuses_other_widths(D, H):
    qkv = torch.zeros((27 * 2, 3 * D), device="cuda")
    with pytest.raises(D3DError, match="head_dim 16"):
        _eng().op_attention_long_f32_h16(qkv, 1, 27, 2, H)


# ------------------------------------------------------------------------------------------------ 5. streaming kernel
# chunks of 256 frames: one key in the second chunk, a ragged second chunk and two query blocks, one key in the third chunk; 8 heads
LONG = [(1, 257, 1, 16, 1), (1, 300, 1, 48, 3), (1, 513, 1, 16, 1), (1, 300, 2, 128, 8)]


@pytest.mark.parametrize("B,T,J,D,H", LONG)
def test_long_windows_match_fp64(B, T, J, D, H):
    E = _eng()
    qkv = hashed(f"qkv{T}_{J}_{D}", (B * T * J, 3 * D), 21, 2.0).cuda()
    ref = attn_ref(qkv, B, T, J, H, True).cpu()
    got = E.op_attention_long_f32_h16(qkv, B, T, J, H)
    err = maxabs(got, ref)
    err32 = maxabs(E.op_attention(qkv, B, T, J, H, True, force_generic=True), ref)
    print(f"attention_long_f32_h16 B={B} T={T} J={J} D={D}: max-abs {err:.3e}; generic fp32 {err32:.3e}")
    assert torch.isfinite(got).all()
    assert _bound_ok(err, err32)


@pytest.mark.parametrize("T", [1, 31, 32, 33, 100, 255, 256])
def test_streaming_is_bit_identical_to_the_resident_kernel(T):
    E = _eng()
    B, J, H = 2, 3, 3
    qkv = hashed(f"qkv{T}_{J}_{DH * H}", (B * T * J, 3 * DH * H), 21, 2.0).cuda()
    want = E.op_attention_f32_h16(qkv, B, T, J, H, True)
    got = E.op_attention_long_f32_h16(qkv, B, T, J, H)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)
