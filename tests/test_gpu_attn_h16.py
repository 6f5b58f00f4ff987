"""Head width 16 on the MI355X (embed_dim 128 with the runner's 8 heads), op level, F16X3: the resident kernel
(kernels_attn_x3_h16.hip k_attn_x3_h16) and the key-streaming kernel at that width (kernels_attn_x3_long.hip k_attn_x3_stream<16, 8>).
Four adjacent heads share one 128-byte LDS row; two of them share a 32-column line of the PV product, so each head's accumulator tile
also holds the line neighbour's V times this head's numerators in its other 16 rows, which must never be stored.
  * the resident kernel against fp64 math: key-tile counts 1, 2, 3, 8, pad keys, 1 and 2 quads, spatial and temporal groups, every group
    length N = 1 .. 256;
  * head isolation: each head of a quad in turn NaN in q, k and v changes no bit of the other three (resident and streaming); a NaN batch
    element does not reach its neighbour; sharp softmax; launch forms bit-identical; refusals;
  * the streaming kernel against fp64 math beyond 256 frames, and bit for bit the resident kernel up to 256.
The engines of this width are in tests/test_gpu_attn_h16_engine.py, the fp32 kernels in tests/test_gpu_attn_f32_h16.py.

Measured (MI355X), max-abs against fp64 (the generic fp32 kernel on the same input in brackets): the resident kernel 2.4e-7 .. 7.3e-7 over
its eight shapes (worst at T = 81: generic 1.9e-6; T = 256: 5.9e-7 against 2.4e-6); every N = 1 .. 256: worst 7.1e-7 at N = 71; sharp
softmax 3.2e-5 / 3.8e-5 (generic 4.3e-5 / 6.2e-5, up to 6.1e-5 apart); the streaming kernel 4.4e-7 .. 6.3e-7 over T = 257, 300, 513 and
300 at 8 heads (2.6e-6 .. 3.5e-6).  The module's 59 cases: 1.4 s."""
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
# key tiles 1 / 1 / 1 / 2 / 3 / 8 with 31, 5, 0, 31, 15, 0 pad keys in the last; two quads (D = 128) and one (D = 64); spatial: one key tile
CASES = [(1, 1, 17, 128, 8, True), (2, 27, 3, 128, 8, True), (1, 32, 2, 64, 4, True), (1, 33, 2, 64, 4, True), (2, 81, 3, 128, 8, True),
         (1, 256, 1, 64, 4, True), (2, 5, 17, 128, 8, False), (3, 23, 15, 64, 4, False)]


@pytest.mark.parametrize("B,T,J,D,H,temporal", CASES)
def test_op_matches_fp64(B, T, J, D, H, temporal):
    E = _eng()
    qkv = hashed(f"qkv{T}_{J}_{D}", (B * T * J, 3 * D), 21, 2.0).cuda()
    ref = attn_ref(qkv, B, T, J, H, temporal).cpu()
    got = E.op_attention_h16(qkv, B, T, J, H, temporal)
    err = maxabs(got, ref)
    err32 = maxabs(E.op_attention(qkv, B, T, J, H, temporal, force_generic=True), ref)
    print(f"attention_h16 B={B} T={T} J={J} D={D} H={H} temporal={int(temporal)}: max-abs {err:.3e}; generic fp32 {err32:.3e}")
    assert torch.isfinite(got).all()
    assert _bound_ok(err, err32)


def test_every_group_length():
    """B = 1, one joint, one quad: every N = 1 .. 256, so every pad-key count of every key-tile count."""
    E = _eng()
    D, H, NMAX = 4 * DH, 4, 256
    full = hashed(f"everyN_{NMAX}_{DH}", (NMAX, 3 * D), 21, 2.0).cuda()
    worst = (0.0, 0, 0.0)
    for N in range(1, NMAX + 1):
        qkv = full[:N].contiguous()
        ref = attn_ref(qkv, 1, N, 1, H, True).cpu()
        got = E.op_attention_h16(qkv, 1, N, 1, H, True)
        assert torch.isfinite(got).all(), N
        err = maxabs(got, ref)
        err32 = maxabs(E.op_attention(qkv, 1, N, 1, H, True, force_generic=True), ref) if err >= 5e-6 else float("nan")
        if err > worst[0]:
            worst = (err, N, err32)
        assert _bound_ok(err, err32), (N, err, err32)
    print(f"attention_h16 every N = 1 .. {NMAX}: worst max-abs {worst[0]:.3e} at N = {worst[1]} (generic fp32 there: {worst[2]:.3e})")


# ------------------------------------------------------------------------------------------------ 2. isolation
def _ops():
    E = _eng()
    return {"resident": lambda q, B, T, J, H: E.op_attention_h16(q, B, T, J, H, True), "streaming": E.op_attention_long_h16}


@pytest.mark.parametrize("op", ["resident", "streaming"])
@pytest.mark.parametrize("k", range(4))
def test_a_nan_head_does_not_reach_the_rest_of_its_quad(k, op):
    """One quad (D = 64), head k's q, k and v columns NaN.  The other three lie in the same 128-byte LDS rows, and one of them shares
    head k's PV line: its accumulator tile takes head k's V in the 16 rows that are not its own.  They must be finite and carry the bits
    of the clean run."""
    B, T, J, H = 1, 40, 2, 4
    D = DH * H
    run = _ops()[op]
    qkv = hashed(f"headiso{DH}", (B * T * J, 3 * D), 21, 2.0).cuda()
    bad = qkv.clone()
    for third in range(3):
        bad[:, third * D + k * DH:third * D + (k + 1) * DH] = float("nan")
    clean, got = run(qkv, B, T, J, H), run(bad, B, T, J, H)
    ref = attn_ref(qkv, B, T, J, H, True).cpu()
    assert maxabs(clean, ref) < 5e-6
    for hd in range(4):
        if hd == k:
            continue
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
    alone = E.op_attention_h16(qkv[:T * J].contiguous(), 1, T, J, H, temporal)
    both = E.op_attention_h16(bad, B, T, J, H, temporal)
    assert torch.isfinite(both[:T * J]).all()
    assert torch.equal(both[:T * J], alone)


# ------------------------------------------------------------------------------------------------ 3. sharp softmax
@pytest.mark.parametrize("B,T,J,temporal", [(2, 7, 17, False), (1, 100, 3, True)])
def test_sharp_softmax(B, T, J, temporal):
    """The scaling of tests/test_gpu_attn_hx.py (hashed inputs at scale 9.0: near one-hot rows) and its bound, that of
    tests/test_gpu_ops.py::test_attention_fast_kernels_agree_with_generic_on_sharp_softmax."""
    E = _eng()
    qkv = hashed(f"sharp{T}", (B * T * J, 3 * DH * 8), 22, 9.0).cuda()
    ref = attn_ref(qkv, B, T, J, 8, temporal).cpu()
    a = E.op_attention_h16(qkv, B, T, J, 8, temporal)
    b = E.op_attention(qkv, B, T, J, 8, temporal, force_generic=True)
    print(f"attention_h16 sharp T={T} J={J}: h16 {maxabs(a, ref):.3e} generic {maxabs(b, ref):.3e} apart {maxabs(a, b.cpu()):.3e}")
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert maxabs(a, ref) < 2e-3 and maxabs(b, ref) < 2e-3
    assert maxabs(a, b.cpu()) < 2e-3


# ------------------------------------------------------------------------------------------------ 4. launch forms
def test_launch_forms_agree():
    """Spatial, 4097 groups of 17 joints x 1 quad = 4097 units: eight units per workgroup (from 4096 units on), the last workgroup with
    surplus waves.  Its first and last groups, run as launches of one unit per workgroup, give the same bits.  (The forms of 1 .. 8 key
    tiles: the next test.)"""
    E = _eng()
    G, J, D, H = 4097, 17, 4 * DH, 4
    qkv = hashed(f"forms{G}_{J}_{D}", (G * J, 3 * D), 21, 2.0).cuda()
    big = E.op_attention_h16(qkv, 1, G, J, H, False)
    assert torch.isfinite(big).all()
    for lo, hi in ((0, 2), (G - 3, G)):
        small = E.op_attention_h16(qkv[lo * J:hi * J].contiguous(), 1, hi - lo, J, H, False)
        assert torch.equal(small, big[lo * J:hi * J])
    err = maxabs(big[:4 * J], attn_ref(qkv[:4 * J], 1, 4, J, H, False).cpu())
    assert err < 5e-6, err


@pytest.mark.parametrize("nkt", range(1, 9))
def test_every_key_tile_form_of_the_ladder_gives_the_streaming_kernels_bits(nkt):
    """One input of 256 frames x 2 joints x 2 quads; its first 32 nkt - 5 frames take the resident form of nkt key tiles.  The streaming
    kernel is ONE form whatever T is, so agreeing with it bit for bit at every nkt ties the eight forms of the ladder to each other."""
    E = _eng()
    J, H, T = 2, 8, 32 * nkt - 5
    full = hashed(f"ladder_{DH}", (256 * J, 3 * DH * H), 21, 2.0).cuda()
    qkv = full[:T * J].contiguous()
    want = E.op_attention_long_h16(qkv, 1, T, J, H)
    got = E.op_attention_h16(qkv, 1, T, J, H, True)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ 5. refusal
@pytest.mark.parametrize("T,D,H", [(27, 256, 8), (27, 384, 8), (27, 512, 8), (27, 32, 2), (27, 96, 6), (257, 128, 8)])
def test_resident_op_refuses_other_widths_head_counts_and_long_windows(T, D, H):
    qkv = torch.zeros((T * 2, 3 * D), device="cuda")
    with pytest.raises(D3DError, match="head_dim 16"):
        _eng().op_attention_h16(qkv, 1, T, 2, H, True)


@pytest.mark.parametrize("D,H", [(256, 8), (384, 8), (512, 8), (32, 2), (96, 6)])
def test_streaming_op_refuses_other_widths_and_head_counts(D, H):
    qkv = torch.zeros((27 * 2, 3 * D), device="cuda")
    with pytest.raises(D3DError, match="head_dim 16"):
        _eng().op_attention_long_h16(qkv, 1, 27, 2, H)


# ------------------------------------------------------------------------------------------------ 6. streaming kernel
# chunks of 256 frames: one key in the second chunk, a ragged second chunk and two query blocks, one key in the third chunk; two quads
LONG = [(1, 257, 1, 64, 4), (1, 300, 1, 64, 4), (1, 513, 1, 64, 4), (1, 300, 2, 128, 8)]


@pytest.mark.parametrize("B,T,J,D,H", LONG)
def test_long_windows_match_fp64(B, T, J, D, H):
    E = _eng()
    qkv = hashed(f"qkv{T}_{J}_{D}", (B * T * J, 3 * D), 21, 2.0).cuda()
    ref = attn_ref(qkv, B, T, J, H, True).cpu()
    got = E.op_attention_long_h16(qkv, B, T, J, H)
    err = maxabs(got, ref)
    err32 = maxabs(E.op_attention(qkv, B, T, J, H, True, force_generic=True), ref)
    print(f"attention_long_h16 B={B} T={T} J={J} D={D}: max-abs {err:.3e}; generic fp32 {err32:.3e}")
    assert torch.isfinite(got).all()
    assert _bound_ok(err, err32)


@pytest.mark.parametrize("T", [1, 31, 32, 33, 255, 256])
def test_streaming_is_bit_identical_to_the_resident_kernel(T):
    E = _eng()
    B, J, H = 2, 3, 8
    qkv = hashed(f"qkv{T}_{J}_{DH * H}", (B * T * J, 3 * DH * H), 21, 2.0).cuda()
    want = E.op_attention_h16(qkv, B, T, J, H, True)
    got = E.op_attention_long_h16(qkv, B, T, J, H)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)
