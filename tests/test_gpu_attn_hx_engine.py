"""Engines with heads of 48 and 96 columns on the MI355X (embed_dim 384 / 768 with the runner's 8 heads; option "attn_hx"): the folded
F16X3 flow with the attention of kernels_attn_x3_hx.hip and kernels_attn_x3_long.hip, the plain row-kernel flow with the generic kernel
(option off), and FP32 engines (the generic kernel) -- forward_denoise against the fp64 oracle, proof of the path through
info("attn_hx_last") (bit 0: spatial blocks, bit 1: temporal blocks resident, bit 2: temporal blocks streaming), the invariances of a
sampling, one long-window sampling per width.  The kernels alone are in tests/test_gpu_attn_hx.py; every GEMM and row kernel of these
engines at its new widths in tests/test_gpu_widths_384_768.py.

Measured (MI355X), max-abs against the fp64 oracle (oracle fp32 floor in brackets): T = 27, B = 2, option on / off: D = 384 1.9e-6 /
2.2e-6 (3.2e-6), D = 768 2.6e-6 / 2.9e-6 (3.3e-6); FP32 engines 3.4e-6 / 3.2e-6; long windows, B = 1, on / off: D = 384, T = 300 2.3e-6 /
4.6e-6 (4.4e-6), D = 768, T = 150 3.4e-6 / 3.0e-6 (3.5e-6); the 2-step sampling of those windows against the fp32 oracle 4.4e-6 / 2.1e-6."""
import pytest
import torch

from helpers import inputs, torch_sd, product_with_engine, xy
from diff3dhpe_amd.spec import DenoiserConfig

pytestmark = pytest.mark.gpu
GATE = 1e-4
DEPTH = 1
KEY, LAST = "attn_hx", "attn_hx_last"
WIDTHS = [384, 768]
LONG_T = {384: 300, 768: 150}      # the shortest windows of the issue beyond the resident limit (256 / 128 frames)


def _cfg(T, D):
    return DenoiserConfig(num_frame=T, embed_dim=D, depth=DEPTH, num_heads=8)


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


def _denoise_inputs(B, T):
    inp = inputs(B, T, 500)
    return torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1), torch.tensor([905, 17, 444][:B], dtype=torch.long)


@pytest.mark.parametrize("D", WIDTHS)
def test_forward_denoise_against_the_oracle_with_the_option_on_and_off(D):
    """forward_denoise at T = 27, B = 2, trained-like weights, depth 1, per-row t, against oracle/d3d_oracle.py in fp64: the folded flow
    with the attention of these widths (spatial and temporal blocks resident: bits 0 and 1) and the plain row-kernel flow with the generic
    kernel both inside the project's 1e-4 gate."""
    T = 27
    cfg = _cfg(T, D)
    net, _, eng = _product(cfg)
    xcat, t = _denoise_inputs(2, T)
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
    print(f"attn_hx D={D} T={T} B=2: err_on {err[1]:.3e} err_off {err[0]:.3e} oracle fp32 floor {floor:.3e}")
    assert eng.range_flags() == 0
    assert err[1] <= GATE and err[0] <= GATE


@pytest.mark.parametrize("D", WIDTHS)
def test_fp32_engine_against_the_oracle(D):
    """An FP32 engine of these widths runs the generic kernel in both block types: the same gate, attn_hx_last == 0."""
    T = 27
    cfg = _cfg(T, D)
    net, _, eng = _product(cfg, prec="fp32")
    xcat, t = _denoise_inputs(2, T)
    ref64, floor = _oracle64(cfg, xcat, t)
    eng.set_option(KEY, 1)
    eng.range_flags(clear=True)
    out = net.forward_denoise(xcat.cuda(), t.cuda())
    err = (out.cpu().double() - ref64).abs().max().item()
    print(f"attn_hx fp32 engine D={D} T={T} B=2: err {err:.3e} oracle fp32 floor {floor:.3e}")
    assert eng.info(LAST) == 0
    assert eng.range_flags() == 0
    assert err <= GATE


def test_one_head_of_48_columns_runs_the_fp32_kernels():
    """embed_dim 48 with one head: no multiple of 32, so the fp16 plane forms (pair layout, 32-deep k-tiles) do not exist there.  The
    engine is admitted in both precisions and runs the FP32 kernels in both -- the fp32 GEMM with a zero-filled last k-tile of 16, the
    generic attention kernel: inside the gate of the fp64 oracle, the same bits from an "fp32" and an "f16x3" model, attn_hx_last 0."""
    T = 27
    cfg = DenoiserConfig(num_frame=T, embed_dim=48, depth=DEPTH, num_heads=1)
    xcat, t = _denoise_inputs(2, T)
    from oracle import d3d_oracle as orc
    sd = _sd(cfg)
    torch.set_default_dtype(torch.float64)
    try:
        ref64 = orc.forward_denoise({k: v.double() for k, v in sd.items()}, xcat.double(), t, depth=DEPTH, heads=1)
    finally:
        torch.set_default_dtype(torch.float32)
    outs = {}
    for prec in ("fp32", "f16x3"):
        net, _, eng = _product(cfg, prec=prec)
        eng.range_flags(clear=True)
        outs[prec] = net.forward_denoise(xcat.cuda(), t.cuda()).cpu()
        assert eng.info(LAST) == 0 and eng.range_flags() == 0
        err = (outs[prec].double() - ref64).abs().max().item()
        print(f"embed_dim 48, one head [{prec}] T={T} B=2: err {err:.3e}")
        assert err <= GATE
    assert torch.equal(outs["fp32"], outs["f16x3"])


@pytest.mark.parametrize("D", WIDTHS)
def test_long_windows_stream_the_temporal_blocks(D):
    """T = 300 (D = 384) / 150 (D = 768), B = 1: the spatial blocks resident, the temporal blocks on the key-streaming kernel (bits 0 and
    2), 0 with the option off; a forward and a 2-step sampling against the oracle inside the gate."""
    T = LONG_T[D]
    cfg = _cfg(T, D)
    net, diff, eng = _product(cfg)
    xcat, t = _denoise_inputs(1, T)
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
        eng.set_option(KEY, 1)
        x2d, nz = xy(1, T, 84)
        got, last = _sample(eng, x2d, nz)
    finally:
        eng.set_option(KEY, default)
    assert last == 5 and torch.isfinite(got).all()
    from oracle import d3d_oracle as orc
    want = orc.ddim_sample_loop(_sd(cfg), orc.diffusion_tables("cosine", 1000), x2d.cpu(), nz.cpu(), num_timesteps=1000, sampling_timesteps=2,
                                depth=DEPTH)
    serr = (got.cpu().double() - want.double()).abs().max().item()
    print(f"attn_hx D={D} T={T} B=1: forward err_on {err[1]:.3e} err_off {err[0]:.3e} oracle fp32 floor {floor:.3e}; sampling {serr:.3e}")
    assert eng.range_flags() == 0
    assert err[1] <= GATE and err[0] <= GATE
    assert serr <= GATE


@pytest.mark.parametrize("D", WIDTHS)
def test_rows_do_not_depend_on_batch_streams_workspace_contents_or_graph_replay(D):
    T, B = 9, 3
    _, _, eng = _product(_cfg(T, D))
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
