"""Head width 128 on the MI355X (embed_dim 1024 with the runner's 8 heads): the generic kernel's DH = 128 instance, the resident F16X3
kernel ("attn_h128", kernels_attn_x3_h128.hip k_attn_x3_h128) and the engines of that width.  A head is two 64-column halves of the plane
rows: one score chain over both, one softmax, four 32-column output quarters.
  * the generic instance against fp64 math, bounded by torch's own fp32 evaluation of the same input;
  * the resident kernel against fp64 math: every key-tile count, pad keys, 1 / 2 / 8 heads, spatial and temporal groups, every group length;
  * sharp softmax; launch forms bit-identical; a NaN batch element does not reach its neighbour; refusals;
  * engine level against the fp64 oracle with the option on and off (F16X3) and in FP32, invariances, proof of the path through
    info("attn_h128_last").  The windows of more than 128 frames are in tests/test_gpu_long_h128.py.

Measured (MI355X), max-abs against fp64: the generic instance 1.6e-6 / 3.5e-6 / 1.4e-6 at its three shapes (torch fp32: 1.5e-6 / 2.3e-6 /
1.4e-6); the resident kernel 2.4e-7 .. 1.24e-6 over its ten shapes (generic fp32 on the same inputs: up to 2.6e-6), every N = 1 .. 128:
worst 9.1e-7 at N = 90; sharp softmax 8.3e-5 spatial (generic 1.6e-4, 1.6e-4 apart); engine against the oracle at T = 27, option on /
off: 3.2e-6 / 3.9e-6 (oracle fp32 floor 3.6e-6), FP32 engine 3.6e-6."""
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


# ------------------------------------------------------------------------------------------------ 1. the generic DH = 128 instance
@pytest.mark.parametrize("B,T,J,D,H,temporal", [(2, 27, 3, 1024, 8, True), (1, 243, 2, 1024, 8, True), (2, 5, 17, 1024, 8, False)])
def test_generic_kernel_matches_fp64(B, T, J, D, H, temporal):
    """max(5e-6, 3 e32): 5e-6 is the op-level bound of tests/test_gpu_long_temporal.py, e32 the error of torch's own fp32 evaluation of the
    same input; the factor 3 because the kernel sums 128 columns and N keys sequentially where torch sums blocked."""
    E = _eng()
    qkv = hashed(f"qkv{T}_{J}_{D}", (B * T * J, 3 * D), 21, 2.0)
    ref = attn_ref(qkv, B, T, J, H, temporal)
    e32 = maxabs(attn_ref(qkv, B, T, J, H, temporal, dtype=torch.float32), ref)
    got = E.op_attention(qkv.cuda(), B, T, J, H, temporal, force_generic=True)
    err = maxabs(got, ref)
    print(f"attention generic dh=128 B={B} T={T} J={J} temporal={int(temporal)}: max-abs {err:.3e}; torch fp32 {e32:.3e}")
    assert torch.isfinite(got).all()
    assert err < max(5e-6, 3 * e32)


# ------------------------------------------------------------------------------------------------ 2. resident kernel against fp64
# key tiles 1 / 1 / 1 / 2 / 3 / 4 / 4 with 31, 5, 0, 31, 15, 28, 0 pad keys in the last; 8, 2 and 1 heads; spatial: one key tile
CASES = [(1, 1, 17, 1024, 8, True), (2, 27, 3, 1024, 8, True), (1, 32, 2, 256, 2, True), (1, 33, 2, 256, 2, True), (2, 81, 3, 1024, 8, True),
         (1, 100, 1, 128, 1, True), (1, 128, 1, 1024, 8, True),
         (2, 5, 17, 1024, 8, False), (3, 23, 15, 1024, 8, False), (2, 5, 16, 128, 1, False)]


@pytest.mark.parametrize("B,T,J,D,H,temporal", CASES)
def test_op_matches_fp64(B, T, J, D, H, temporal):
    E = _eng()
    qkv = hashed(f"qkv{T}_{J}_{D}", (B * T * J, 3 * D), 21, 2.0).cuda()
    ref = attn_ref(qkv, B, T, J, H, temporal).cpu()
    got = E.op_attention_h128(qkv, B, T, J, H, temporal)
    err = maxabs(got, ref)
    err32 = maxabs(E.op_attention(qkv, B, T, J, H, temporal, force_generic=True), ref)
    print(f"attention_h128 B={B} T={T} J={J} D={D} H={H} temporal={int(temporal)}: max-abs {err:.3e}; generic fp32 {err32:.3e}")
    assert torch.isfinite(got).all()
    assert _bound_ok(err, err32)


def test_every_group_length():
    """B = 1, one joint, one head: every N = 1 .. 128, so every pad-key count of every key-tile count."""
    E = _eng()
    D, H = 128, 1
    full = hashed("everyN_128", (128, 3 * D), 21, 2.0).cuda()
    worst = (0.0, 0, 0.0)
    for N in range(1, 129):
        qkv = full[:N].contiguous()
        ref = attn_ref(qkv, 1, N, 1, H, True).cpu()
        got = E.op_attention_h128(qkv, 1, N, 1, H, True)
        assert torch.isfinite(got).all(), N
        err = maxabs(got, ref)
        err32 = maxabs(E.op_attention(qkv, 1, N, 1, H, True, force_generic=True), ref) if err >= 5e-6 else float("nan")
        if err > worst[0]:
            worst = (err, N, err32)
        assert _bound_ok(err, err32), (N, err, err32)
    print(f"attention_h128 every N = 1 .. 128: worst max-abs {worst[0]:.3e} at N = {worst[1]} (generic fp32 there: {worst[2]:.3e})")


# ------------------------------------------------------------------------------------------------ 3. sharp softmax
@pytest.mark.parametrize("B,T,J,temporal", [(2, 7, 17, False), (1, 100, 3, True)])
def test_sharp_softmax(B, T, J, temporal):
    """Logits up to ~100 (near one-hot rows): the bound of tests/test_gpu_ops.py::test_attention_fast_kernels_agree_with_generic_on_sharp_softmax.
    (The T = 243 input of this family is the streaming kernel's: tests/test_gpu_long_h128.py.)"""
    E = _eng()
    qkv = hashed(f"sharp{T}", (B * T * J, 3 * 1024), 22, 9.0).cuda()
    ref = attn_ref(qkv, B, T, J, 8, temporal).cpu()
    a = E.op_attention_h128(qkv, B, T, J, 8, temporal)
    b = E.op_attention(qkv, B, T, J, 8, temporal, force_generic=True)
    print(f"attention_h128 sharp T={T} J={J}: h128 {maxabs(a, ref):.3e} generic {maxabs(b, ref):.3e} apart {maxabs(a, b.cpu()):.3e}")
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert maxabs(a, ref) < 2e-3 and maxabs(b, ref) < 2e-3
    assert maxabs(a, b.cpu()) < 2e-3


# ------------------------------------------------------------------------------------------------ 4. launch forms
def test_launch_forms_agree():
    """Spatial, 4097 groups of 17 joints x 1 head = 4097 units: four units per workgroup (from 4096 units on), the last workgroup with
    three surplus waves.  Its first and last groups, run as launches of one unit per workgroup, give the same bits."""
    E = _eng()
    G, J, D, H = 4097, 17, 128, 1
    qkv = hashed(f"forms{G}_{J}_{D}", (G * J, 3 * D), 21, 2.0).cuda()
    big = E.op_attention_h128(qkv, 1, G, J, H, False)
    assert torch.isfinite(big).all()
    for lo, hi in ((0, 2), (G - 3, G)):
        small = E.op_attention_h128(qkv[lo * J:hi * J].contiguous(), 1, hi - lo, J, H, False)
        assert torch.equal(small, big[lo * J:hi * J])
    err = maxabs(big[:4 * J], attn_ref(qkv[:4 * J], 1, 4, J, H, False).cpu())
    assert err < 5e-6, err


# ------------------------------------------------------------------------------------------------ 5. isolation
@pytest.mark.parametrize("T,J,temporal", [(100, 2, True), (5, 17, False)])
def test_a_nan_batch_element_does_not_reach_its_neighbour(T, J, temporal):
    E = _eng()
    B, D, H = 2, 1024, 8
    qkv = hashed(f"isoqkv{T}_{J}_{D}_{B}", (B * T * J, 3 * D), 21, 2.0).cuda()
    bad = qkv.clone()
    bad[T * J:] = float("nan")
    alone = E.op_attention_h128(qkv[:T * J].contiguous(), 1, T, J, H, temporal)
    both = E.op_attention_h128(bad, B, T, J, H, temporal)
    assert torch.isfinite(both[:T * J]).all()
    assert torch.equal(both[:T * J], alone)


# ------------------------------------------------------------------------------------------------ 6. refusal
@pytest.mark.parametrize("T,D,H", [(27, 512, 8), (27, 96, 3), (129, 1024, 8)])
def test_refuses_other_widths_and_long_windows(T, D, H):
    qkv = torch.zeros((T * 2, 3 * D), device="cuda")
    with pytest.raises(D3DError, match="head_dim 128"):
        _eng().op_attention_h128(qkv, 1, T, 2, H, True)


# ------------------------------------------------------------------------------------------------ 7. - 9. engine level
def _cfg(T, D=1024, H=8):
    return DenoiserConfig(num_frame=T, embed_dim=D, depth=DEPTH, num_heads=H)


def _sd(cfg, seed=11):   # this module's weights: seed 11 of the trained-like family
    return torch_sd(cfg, seed, family="trainedlike")


def _product(cfg, seed=11, prec="f16x3", sampling=2):   # this module's defaults; the weights of _sd
    return product_with_engine(cfg, seed, prec, sampling, family="trainedlike")


def _sample(eng, x2d, nz):   # reads this feature's proof-of-path key
    out = eng.ddim_sample(x2d, nz).clone()
    return out, eng.info(LAST)


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
    """forward_denoise at T = 27, B = 2, trained-like weights, depth 1, per-row t, against oracle/d3d_oracle.py in fp64: the folded flow
    with the head-width-128 attention (spatial and temporal blocks resident: bits 0 and 1) and the plain row-kernel flow both inside
    the project's 1e-4 gate."""
    T = 27
    cfg = _cfg(T)
    net, _, eng = _product(cfg)
    inp = inputs(2, T, 500)
    xcat = torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1)
    t = torch.tensor([905, 17], dtype=torch.long)
    ref64, floor = _oracle64(cfg, xcat, t)
    default = eng.info(KEY)
    assert eng.info(LAST) == 0                         # before any forward
    eng.range_flags(clear=True)
    err = {}
    try:
        for opt in (1, 0):
            eng.set_option(KEY, opt)
            out = net.forward_denoise(xcat.cuda(), t.cuda())
            assert eng.info(LAST) == (3 if opt else 0)
            err[opt] = (out.cpu().double() - ref64).abs().max().item()
    finally:
        eng.set_option(KEY, default)
    print(f"attn_h128 T={T} B=2: err_on {err[1]:.3e} err_off {err[0]:.3e} oracle fp32 floor {floor:.3e}")
    assert eng.range_flags() == 0
    assert err[1] <= GATE and err[0] <= GATE


def test_fp32_engine_against_the_oracle():
    """An FP32 engine of this width runs the generic kernel in both block types: the same gate, attn_h128_last == 0."""
    T = 27
    cfg = _cfg(T)
    net, _, eng = _product(cfg, prec="fp32")
    inp = inputs(2, T, 500)
    xcat = torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1)
    t = torch.tensor([905, 17], dtype=torch.long)
    ref64, floor = _oracle64(cfg, xcat, t)
    eng.set_option(KEY, 1)
    out = net.forward_denoise(xcat.cuda(), t.cuda())
    err = (out.cpu().double() - ref64).abs().max().item()
    print(f"attn_h128 fp32 engine T={T} B=2: err {err:.3e} oracle fp32 floor {floor:.3e}")
    assert eng.info(LAST) == 0
    assert err <= GATE


def test_rows_do_not_depend_on_batch_streams_workspace_contents_or_graph_replay():
    T, B = 27, 3
    _, _, eng = _product(_cfg(T))
    eng.set_option(KEY, 1)
    x2d, nz = xy(B, T, 80)
    eng.set_option("streams", 2)
    whole, last = _sample(eng, x2d, nz)
    assert last == 3 and torch.isfinite(whole).all()
    for b in range(B):
        one, last = _sample(eng, x2d[b:b + 1].contiguous(), nz[b:b + 1].contiguous())
        assert last == 3 and torch.equal(one, whole[b:b + 1])
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
    assert l1 == 3
    assert eng.range_flags() == 0
    assert torch.equal(first, whole) and torch.equal(again, whole)


@pytest.mark.parametrize("D,H", [(512, 8), (256, 8), (256, 4)])
def test_other_widths_never_take_the_kernels(D, H):
    """Heads of 64 and 32 columns with the option on."""
    T = 27
    _, _, eng = _product(_cfg(T, D, H))
    eng.set_option(KEY, 1)
    assert eng.info(LAST) == 0                         # before any forward
    out, last = _sample(eng, *xy(1, T, 83))
    assert last == 0 and torch.isfinite(out).all()
