"""Head widths 48 and 96 on the MI355X (embed_dim 384 / 768 with the runner's 8 heads), op level: the generic kernel's DH = 48 / 96
instances, the resident F16X3 kernel (kernels_attn_x3_hx.hip k_attn_x3_hx) and the key-streaming kernel at these widths
(kernels_attn_x3_long.hip k_attn_x3_stream<48, 8> / <96, 4>).  A head is 48 or 96 adjacent plane columns from column hd DH on: it does
not coincide with the 64-column LDS rows, so the columns behind it in its last LDS row must be zeros (or never read), never the next head.
  * the generic instances against fp64 math, bounded by torch's own fp32 evaluation of the same input;
  * the resident kernel against fp64 math: every key-tile count, pad keys, 1 / 2 / 8 heads, spatial and temporal groups, every group length;
  * head isolation: a NaN head between two clean ones changes no bit of them (resident and streaming); a NaN batch element does not
    reach its neighbour; sharp softmax; launch forms bit-identical; refusals;
  * the streaming kernel against fp64 math beyond the resident limits, and bit for bit the resident kernel below them.
The engines of these widths are in tests/test_gpu_attn_hx_engine.py.

Measured (MI355X), max-abs against fp64 (the generic fp32 kernel on the same input in brackets): the generic instances 1.23e-6 (dh 48)
and 1.49e-6 (dh 96), torch fp32 1.23e-6 / 1.37e-6; the resident kernel at width 48 2.4e-7 .. 8.2e-7 over its eight shapes (worst at
T = 81: generic 1.9e-6), at width 96 2.4e-7 .. 1.0e-6 over its six (worst spatial, 17 joints: 1.5e-6); every N = 1 .. 256 at width 48:
worst 7.4e-7 at N = 81, every N = 1 .. 128 at width 96: worst 8.4e-7 at N = 43; sharp softmax 4.5e-5 .. 1.2e-4 (generic 5.9e-5 .. 2.6e-4,
up to 2.5e-4 apart); the streaming kernel at width 48 5.6e-7 .. 6.5e-7 over T = 257, 300, 513 and 300 at 8 heads (2.4e-6 .. 3.5e-6),
at width 96 6.2e-7 .. 9.5e-7 over T = 129, 243, 300 and 150 at 8 heads (1.9e-6 .. 3.0e-6)."""
import pytest
import torch

from helpers import hashed, maxabs, attn_ref
from diff3dhpe_amd._lib import D3DError

pytestmark = pytest.mark.gpu
WIDTHS = (48, 96)
RESIDENT = {48: 256, 96: 128}      # the longest resident group of a width


def _eng():
    from diff3dhpe_amd import engine
    return engine


def _bound_ok(err, err32):
    """The project's rule for an MFMA attention kernel: 5e-6, else 1.5 x the generic fp32 kernel's error on the same input."""
    return err < (5e-6 if err < 5e-6 else 1.5 * err32)


# ------------------------------------------------------------------------------------------------ 1. the generic DH = 48 / 96 instances
@pytest.mark.parametrize("B,T,J,D,H,temporal", [(2, 27, 3, 384, 8, True), (2, 5, 17, 768, 8, False)])
def test_generic_kernel_matches_fp64(B, T, J, D, H, temporal):
    """max(5e-6, 3 e32), the rule of tests/test_gpu_attn_h128.py: 5e-6 is the op-level bound, e32 the error of torch's own fp32
    evaluation of the same input; the factor 3 because the kernel sums the columns and the keys sequentially where torch sums blocked."""
    E = _eng()
    qkv = hashed(f"qkv{T}_{J}_{D}", (B * T * J, 3 * D), 21, 2.0)
    ref = attn_ref(qkv, B, T, J, H, temporal)
    e32 = maxabs(attn_ref(qkv, B, T, J, H, temporal, dtype=torch.float32), ref)
    got = E.op_attention(qkv.cuda(), B, T, J, H, temporal, force_generic=True)
    err = maxabs(got, ref)
    print(f"attention generic dh={D // H} B={B} T={T} J={J} temporal={int(temporal)}: max-abs {err:.3e}; torch fp32 {e32:.3e}")
    assert torch.isfinite(got).all()
    assert err < max(5e-6, 3 * e32)


# ------------------------------------------------------------------------------------------------ 2. resident kernel against fp64
# width 48: key tiles 1 / 1 / 1 / 2 / 3 / 8 with 31, 5, 0, 31, 15, 0 pad keys in the last; 8, 2 and 1 heads (D = 48: an output row pitch
# of 64 columns); spatial: one key tile.  Width 96: key tiles 1 / 1 / 2 / 3 / 4
CASES = [(1, 1, 17, 384, 8, True), (2, 27, 3, 384, 8, True), (1, 32, 2, 96, 2, True), (1, 33, 2, 96, 2, True), (2, 81, 3, 384, 8, True),
         (1, 256, 1, 48, 1, True), (2, 5, 17, 384, 8, False), (3, 23, 15, 48, 1, False),
         (1, 1, 17, 768, 8, True), (1, 32, 2, 192, 2, True), (1, 33, 2, 192, 2, True), (2, 81, 3, 768, 8, True), (1, 128, 1, 96, 1, True),
         (2, 5, 17, 768, 8, False)]


@pytest.mark.parametrize("B,T,J,D,H,temporal", CASES)
def test_op_matches_fp64(B, T, J, D, H, temporal):
    E = _eng()
    qkv = hashed(f"qkv{T}_{J}_{D}", (B * T * J, 3 * D), 21, 2.0).cuda()
    ref = attn_ref(qkv, B, T, J, H, temporal).cpu()
    got = E.op_attention_hx(qkv, B, T, J, H, temporal)
    err = maxabs(got, ref)
    err32 = maxabs(E.op_attention(qkv, B, T, J, H, temporal, force_generic=True), ref)
    print(f"attention_hx dh={D // H} B={B} T={T} J={J} D={D} H={H} temporal={int(temporal)}: max-abs {err:.3e}; generic fp32 {err32:.3e}")
    assert torch.isfinite(got).all()
    assert _bound_ok(err, err32)


@pytest.mark.parametrize("DH", WIDTHS)
def test_every_group_length(DH):
    """B = 1, one joint, one head: every N = 1 .. 256 (width 48) / 1 .. 128 (width 96), so every pad-key count of every key-tile count."""
    E = _eng()
    D, H, NMAX = DH, 1, RESIDENT[DH]
    full = hashed(f"everyN_{NMAX}_{DH}", (NMAX, 3 * D), 21, 2.0).cuda()
    worst = (0.0, 0, 0.0)
    for N in range(1, NMAX + 1):
        qkv = full[:N].contiguous()
        ref = attn_ref(qkv, 1, N, 1, H, True).cpu()
        got = E.op_attention_hx(qkv, 1, N, 1, H, True)
        assert torch.isfinite(got).all(), N
        err = maxabs(got, ref)
        err32 = maxabs(E.op_attention(qkv, 1, N, 1, H, True, force_generic=True), ref) if err >= 5e-6 else float("nan")
        if err > worst[0]:
            worst = (err, N, err32)
        assert _bound_ok(err, err32), (N, err, err32)
    print(f"attention_hx dh={DH} every N = 1 .. {NMAX}: worst max-abs {worst[0]:.3e} at N = {worst[1]} (generic fp32 there: {worst[2]:.3e})")


# ------------------------------------------------------------------------------------------------ 3. isolation
def _ops():
    E = _eng()
    return {"resident": lambda q, B, T, J, H: E.op_attention_hx(q, B, T, J, H, True), "streaming": E.op_attention_long_hx}


@pytest.mark.parametrize("op", ["resident", "streaming"])
@pytest.mark.parametrize("DH", WIDTHS)
def test_a_nan_head_does_not_reach_its_neighbours(DH, op):
    """Three heads (D = 144 / 288), head 1's q, k and v columns NaN.  Head 0 ends and head 2 starts inside an LDS row whose other columns
    are head 1's in the planes: staged as they lie there, the NaN would enter the score chain (d-steps behind the head) or the PV
    product.  Heads 0 and 2 must be finite and carry the bits of the clean run."""
    B, T, J, H = 1, 40, 2, 3
    D = DH * H
    run = _ops()[op]
    qkv = hashed(f"headiso{DH}", (B * T * J, 3 * D), 21, 2.0).cuda()
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
@pytest.mark.parametrize("DH", WIDTHS)
def test_a_nan_batch_element_does_not_reach_its_neighbour(DH, T, J, temporal):
    E = _eng()
    B, H = 2, 8
    D = DH * H
    qkv = hashed(f"isoqkv{T}_{J}_{D}_{B}", (B * T * J, 3 * D), 21, 2.0).cuda()
    bad = qkv.clone()
    bad[T * J:] = float("nan")
    alone = E.op_attention_hx(qkv[:T * J].contiguous(), 1, T, J, H, temporal)
    both = E.op_attention_hx(bad, B, T, J, H, temporal)
    assert torch.isfinite(both[:T * J]).all()
    assert torch.equal(both[:T * J], alone)


# ------------------------------------------------------------------------------------------------ 4. sharp softmax
@pytest.mark.parametrize("B,T,J,temporal", [(2, 7, 17, False), (1, 100, 3, True)])
@pytest.mark.parametrize("DH", WIDTHS)
def test_sharp_softmax(DH, B, T, J, temporal):
    """Logits up to ~100 (near one-hot rows): the bound of tests/test_gpu_ops.py::test_attention_fast_kernels_agree_with_generic_on_sharp_softmax."""
    E = _eng()
    qkv = hashed(f"sharp{T}", (B * T * J, 3 * DH * 8), 22, 9.0).cuda()
    ref = attn_ref(qkv, B, T, J, 8, temporal).cpu()
    a = E.op_attention_hx(qkv, B, T, J, 8, temporal)
    b = E.op_attention(qkv, B, T, J, 8, temporal, force_generic=True)
    print(f"attention_hx dh={DH} sharp T={T} J={J}: hx {maxabs(a, ref):.3e} generic {maxabs(b, ref):.3e} apart {maxabs(a, b.cpu()):.3e}")
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert maxabs(a, ref) < 2e-3 and maxabs(b, ref) < 2e-3
    assert maxabs(a, b.cpu()) < 2e-3


# ------------------------------------------------------------------------------------------------ 5. launch forms
@pytest.mark.parametrize("DH", WIDTHS)
def test_launch_forms_agree(DH):
    """Spatial, 4097 groups of 17 joints x 1 head = 4097 units: eight (width 48) / four (width 96) units per workgroup (from 4096 units
    on), the last workgroup with surplus waves.  Its first and last groups, run as launches of one unit per workgroup, give the same bits."""
    E = _eng()
    G, J, D, H = 4097, 17, DH, 1
    qkv = hashed(f"forms{G}_{J}_{D}", (G * J, 3 * D), 21, 2.0).cuda()
    big = E.op_attention_hx(qkv, 1, G, J, H, False)
    assert torch.isfinite(big).all()
    for lo, hi in ((0, 2), (G - 3, G)):
        small = E.op_attention_hx(qkv[lo * J:hi * J].contiguous(), 1, hi - lo, J, H, False)
        assert torch.equal(small, big[lo * J:hi * J])
    err = maxabs(big[:4 * J], attn_ref(qkv[:4 * J], 1, 4, J, H, False).cpu())
    assert err < 5e-6, err


# ------------------------------------------------------------------------------------------------ 6. refusal
@pytest.mark.parametrize("T,D,H", [(27, 256, 8), (27, 512, 8), (27, 1024, 8), (257, 384, 8), (129, 768, 8)])
def test_resident_op_refuses_other_widths_and_long_windows(T, D, H):
    qkv = torch.zeros((T * 2, 3 * D), device="cuda")
    with pytest.raises(D3DError, match="head_dim 48 or 96"):
        _eng().op_attention_hx(qkv, 1, T, 2, H, True)


@pytest.mark.parametrize("D,H", [(256, 8), (512, 8), (1024, 8)])
def test_streaming_op_refuses_other_widths(D, H):
    qkv = torch.zeros((27 * 2, 3 * D), device="cuda")
    with pytest.raises(D3DError, match="head_dim 48 or 96"):
        _eng().op_attention_long_hx(qkv, 1, 27, 2, H)


# ------------------------------------------------------------------------------------------------ 7. streaming kernel
# width 48 (chunks of 256 frames): one key in the second chunk, a ragged second chunk and two query blocks, one key in the third chunk; 8
# heads.  Width 96 (chunks of 128): one key in the second chunk, a ragged second chunk, a third chunk and two query blocks; 8 heads
LONG = [(1, 257, 1, 48, 1), (1, 300, 1, 48, 1), (1, 513, 1, 48, 1), (1, 300, 2, 384, 8),
        (1, 129, 1, 96, 1), (1, 243, 1, 96, 1), (1, 300, 1, 96, 1), (1, 150, 2, 768, 8)]


@pytest.mark.parametrize("B,T,J,D,H", LONG)
def test_long_windows_match_fp64(B, T, J, D, H):
    E = _eng()
    qkv = hashed(f"qkv{T}_{J}_{D}", (B * T * J, 3 * D), 21, 2.0).cuda()
    ref = attn_ref(qkv, B, T, J, H, True).cpu()
    got = E.op_attention_long_hx(qkv, B, T, J, H)
    err = maxabs(got, ref)
    err32 = maxabs(E.op_attention(qkv, B, T, J, H, True, force_generic=True), ref)
    print(f"attention_long_hx dh={D // H} B={B} T={T} J={J} D={D}: max-abs {err:.3e}; generic fp32 {err32:.3e}")
    assert torch.isfinite(got).all()
    assert _bound_ok(err, err32)


@pytest.mark.parametrize("DH,T", [(48, 27), (48, 100), (48, 256), (96, 27), (96, 100), (96, 128)])
def test_streaming_is_bit_identical_to_the_resident_kernel(DH, T):
    E = _eng()
    B, J, H = 2, 3, 8
    qkv = hashed(f"qkv{T}_{J}_{DH * H}", (B * T * J, 3 * DH * H), 21, 2.0).cuda()
    want = E.op_attention_hx(qkv, B, T, J, H, True)
    got = E.op_attention_long_hx(qkv, B, T, J, H)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)
