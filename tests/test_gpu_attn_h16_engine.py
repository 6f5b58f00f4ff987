"""Engines with heads of 16 columns on the MI355X (embed_dim 128 with the runner's 8 heads), depth 1: the folded F16X3 flow with the
attention of kernels_attn_x3_h16.hip and kernels_attn_x3_long.hip (option "attn_h16"), FP32 engines on the DH = 16 walks of
kernels_attn_f32_hx.hip (option "attn_f32_h16"), and both with their option off (the generic kernel) -- forward_denoise against the fp64
oracle, proof of the path through info("attn_h16_last") / info("attn_f32_h16_last") (bit 0: spatial blocks, bit 1: temporal blocks
resident, bit 2: temporal blocks streaming), the invariances of a sampling, long windows, the fallback engine of precision "auto",
embed_dim 32 with 2 heads (no quad: the F16X3 engine keeps its flow), and the plan rows of these engines.  The kernels alone are in
tests/test_gpu_attn_h16.py and tests/test_gpu_attn_f32_h16.py.

Measured (MI355X), max-abs against the fp64 oracle, option on / off (oracle fp32 floor in brackets): T = 27, B = 2: F16X3 1.0e-6 /
2.1e-6, FP32 1.9e-6 / 2.3e-6 (2.0e-6); T = 300, B = 1: F16X3 3.9e-6 / 2.4e-6, FP32 2.6e-6 / 3.2e-6 (4.4e-6); embed_dim 32 with 2 heads:
F16X3 8.2e-7 / 8.2e-7 (the same flow), FP32 9.8e-7 / 8.8e-7 (8.2e-7).  The 2-step sampling at T = 300 is 0 from the fp32 oracle in both
precisions: with these weights the clipped x0 of the last step sits on the clip bounds, so that comparison shows a finished sampling and
little more; the forward comparison is the sharp one.  The module's 13 cases: 1.7 s."""
import warnings

import pytest
import torch

from helpers import inputs, torch_sd, build_net, product_with_engine, xy
from diff3dhpe_amd.spec import DenoiserConfig

pytestmark = pytest.mark.gpu
GATE = 1e-4
DEPTH = 1
# precision -> (option, info key)
KEYS = {"f16x3": ("attn_h16", "attn_h16_last"), "fp32": ("attn_f32_h16", "attn_f32_h16_last")}
PRECS = sorted(KEYS)


def _cfg(T, D=128, H=8):
    return DenoiserConfig(num_frame=T, embed_dim=D, depth=DEPTH, num_heads=H)


def _sd(cfg, seed=11):   # this module's weights: seed 11 of the trained-like family
    return torch_sd(cfg, seed, family="trainedlike")


def _product(cfg, seed=11, prec="f16x3", sampling=2):   # this module's defaults; the weights of _sd
    return product_with_engine(cfg, seed, prec, sampling, family="trainedlike")


def _oracle64(cfg, xcat, t):
    """(fp64 oracle output, max-abs distance of the fp32 oracle from it)."""
    from oracle import d3d_oracle as orc
    sd = _sd(cfg)
    kw = {} if cfg.num_heads == 8 else {"heads": cfg.num_heads}
    ref32 = orc.forward_denoise(sd, xcat, t, depth=DEPTH, **kw)
    torch.set_default_dtype(torch.float64)      # (the oracle's sinusoid and identity follow the default dtype)
    try:
        ref64 = orc.forward_denoise({k: v.double() for k, v in sd.items()}, xcat.double(), t, depth=DEPTH, **kw)
    finally:
        torch.set_default_dtype(torch.float32)
    assert ref64.dtype == torch.float64
    return ref64, (ref32.double() - ref64).abs().max().item()


def _denoise_inputs(B, T):
    inp = inputs(B, T, 500)
    return torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1), torch.tensor([905, 17, 444][:B], dtype=torch.long)


def _forward_on_and_off(net, eng, key, last, xcat, t, ref64, want):
    """max-abs error of forward_denoise with the option on and off; the info key reads `want` / 0."""
    default = eng.info(key)
    assert eng.info(last) == 0                         # before any forward
    eng.range_flags(clear=True)
    err = {}
    try:
        for opt in (1, 0):
            eng.set_option(key, opt)
            out = net.forward_denoise(xcat.cuda(), t.cuda())
            assert eng.info(last) == (want if opt else 0)
            err[opt] = (out.cpu().double() - ref64).abs().max().item()
    finally:
        eng.set_option(key, default)
    return err


# ------------------------------------------------------------------------------------------------ 1. / 2. T = 27 against the oracle
@pytest.mark.parametrize("prec", PRECS)
def test_forward_denoise_against_the_oracle_with_the_option_on_and_off(prec):
    """forward_denoise at T = 27, B = 2, trained-like weights, per-row t, against oracle/d3d_oracle.py in fp64: the kernels of this
    width in both block types (bits 0 and 1) and the generic kernel (option off) both inside the project's 1e-4 gate."""
    T = 27
    key, last = KEYS[prec]
    cfg = _cfg(T)
    net, _, eng = _product(cfg, prec=prec)
    xcat, t = _denoise_inputs(2, T)
    ref64, floor = _oracle64(cfg, xcat, t)
    err = _forward_on_and_off(net, eng, key, last, xcat, t, ref64, 3)
    print(f"{key} T={T} B=2: err_on {err[1]:.3e} err_off {err[0]:.3e} oracle fp32 floor {floor:.3e}")
    assert eng.range_flags() == 0
    assert err[1] <= GATE and err[0] <= GATE


# ------------------------------------------------------------------------------------------------ 3. long windows
@pytest.mark.parametrize("prec", PRECS)
def test_long_windows_stream_the_temporal_blocks(prec):
    """T = 300, B = 1: the spatial blocks resident, the temporal blocks on the key-streaming kernel (bits 0 and 2), 0 with the option
    off; a forward against the fp64 oracle and a 2-step sampling against the oracle inside the gate."""
    T = 300
    key, last = KEYS[prec]
    cfg = _cfg(T)
    net, diff, eng = _product(cfg, prec=prec)
    xcat, t = _denoise_inputs(1, T)
    ref64, floor = _oracle64(cfg, xcat, t)
    default = eng.info(key)
    err = _forward_on_and_off(net, eng, key, last, xcat, t, ref64, 5)
    try:
        eng.set_option(key, 1)
        x2d, nz = xy(1, T, 84)
        got = eng.ddim_sample(x2d, nz).clone()
        ran = eng.info(last)
    finally:
        eng.set_option(key, default)
    assert ran == 5 and torch.isfinite(got).all()
    from oracle import d3d_oracle as orc
    want = orc.ddim_sample_loop(_sd(cfg), orc.diffusion_tables("cosine", 1000), x2d.cpu(), nz.cpu(), num_timesteps=1000, sampling_timesteps=2,
                                depth=DEPTH)
    serr = (got.cpu().double() - want.double()).abs().max().item()
    print(f"{key} T={T} B=1: forward err_on {err[1]:.3e} err_off {err[0]:.3e} oracle fp32 floor {floor:.3e}; sampling {serr:.3e}")
    assert eng.range_flags() == 0
    assert err[1] <= GATE and err[0] <= GATE
    assert serr <= GATE


# ------------------------------------------------------------------------------------------------ 4. invariances
@pytest.mark.parametrize("prec", PRECS)
def test_rows_do_not_depend_on_batch_streams_or_graph_replay(prec):
    T, B = 9, 3
    key, last = KEYS[prec]
    _, _, eng = _product(_cfg(T), prec=prec)
    eng.set_option(key, 1)
    x2d, nz = xy(B, T, 80)

    def sample(x, n):
        out = eng.ddim_sample(x, n).clone()
        return out, eng.info(last)

    eng.set_option("streams", 2)
    whole, ran = sample(x2d, nz)
    assert ran == 3 and torch.isfinite(whole).all()
    for b in range(B):
        one, ran = sample(x2d[b:b + 1].contiguous(), nz[b:b + 1].contiguous())
        assert ran == 3 and torch.equal(one, whole[b:b + 1])
    eng.set_option("streams", 1)
    assert torch.equal(sample(x2d, nz)[0], whole)
    eng.set_option("streams", 2)
    eng.set_graph_mode(True)
    try:
        first, l1 = sample(x2d, nz)                # eager warm-up pass + capture + replay
        again = eng.ddim_sample(x2d, nz).clone()   # replay of the cached graph
        assert eng.info("graphs_cached") >= 1
    finally:
        eng.set_graph_mode(False)
    assert l1 == 3
    assert eng.range_flags() == 0
    assert torch.equal(first, whole) and torch.equal(again, whole)


# ------------------------------------------------------------------------------------------------ 5. precision "auto"
def test_the_auto_fallback_engine_runs_the_kernels():
    """precision "auto" at T = 27, embed_dim 128: an input scaled past the plane range raises the F16X3 guard, the call is repeated on the
    exact-fp32 engine -- ONE warning, the fp32 model's result bit for bit, and that engine's blocks on the fp32 kernels for heads of 16
    columns (the pattern of tests/test_gpu_attn_f32_hx.py)."""
    T, Bn = 27, 2
    key, last = KEYS["fp32"]
    cfg = _cfg(T)
    net = build_net(cfg, 11, "auto", family="trainedlike").cuda()
    net32 = build_net(cfg, 11, "fp32", family="trainedlike").cuda()
    dev = torch.device("cuda", torch.cuda.current_device())
    net.engine_for(dev, True).set_option(key, 1)       # (whatever the default is)
    net32.engine_for(dev).set_option(key, 1)
    x2d, nz = xy(Bn, T, 81)
    big = torch.cat([x2d * 1.0e6, nz], dim=-1)
    t = torch.arange(Bn, device="cuda") * 300 + 11
    want = net32.forward_denoise(big, t).clone()
    with warnings.catch_warnings(record=True) as wlog:
        warnings.simplefilter("always")
        got = net.forward_denoise(big, t).clone()
    ours = [w for w in wlog if issubclass(w.category, RuntimeWarning)]
    assert len(ours) == 1 and "range guard fired" in str(ours[0].message), [str(w.message) for w in wlog]
    assert torch.equal(got, want)
    assert net._on_fallback()
    assert net.engine_for(dev, True).info(last) == 3
    assert net32.engine_for(dev).info(last) == 3


# ------------------------------------------------------------------------------------------------ 6. heads that are no quad
@pytest.mark.parametrize("prec", PRECS)
def test_two_heads_of_16_columns(prec):
    """embed_dim 32 with 2 heads: the F16X3 kernels take quads of heads, so that engine keeps the flow it had whatever the option says
    (attn_h16_last 0 with the option on and off); the FP32 engine runs the fp32 kernels of the width (3 / 0).  Both inside the gate."""
    T = 27
    key, last = KEYS[prec]
    cfg = _cfg(T, 32, 2)
    net, _, eng = _product(cfg, prec=prec)
    xcat, t = _denoise_inputs(2, T)
    ref64, floor = _oracle64(cfg, xcat, t)
    err = _forward_on_and_off(net, eng, key, last, xcat, t, ref64, 3 if prec == "fp32" else 0)
    print(f"{key} embed_dim 32, 2 heads, T={T} B=2: err_on {err[1]:.3e} err_off {err[0]:.3e} oracle fp32 floor {floor:.3e}")
    assert eng.range_flags() == 0
    assert err[1] <= GATE and err[0] <= GATE


# ------------------------------------------------------------------------------------------------ 7. the plan
# The keys of tests/test_gpu_attention_plan.py, which all read 0 at this width, and the two of this width.  Options: the new ones on
# (whatever their default), every other at its default.
OTHER_KEYS = ("long_temporal_last", "attn_h32_last", "long_temporal_h32_last", "attn_h128_last", "long_temporal_f32_last", "attn_f32_h32_last",
              "long_temporal_f32_h32_last")
NEW_KEYS = ("attn_h16_last", "attn_f32_h16_last")
# (precision, embed_dim, heads, frames): the keys that are not 0
PLANS = [
    ("f16x3", 128, 8, 243, {"attn_h16_last": 3}),        # bit 0 spatial, bit 1 resident temporal
    ("f16x3", 128, 8, 300, {"attn_h16_last": 5}),        # bit 0 spatial, bit 2 streaming temporal
    ("fp32", 128, 8, 243, {"attn_f32_h16_last": 3}),
    ("fp32", 128, 8, 300, {"attn_f32_h16_last": 5}),
]


@pytest.mark.parametrize("prec,D,H,T,expected", PLANS, ids=[f"{p}_D{d}_T{t}" for p, d, _, t, _ in PLANS])
def test_the_plan_of_an_engine_of_this_width(prec, D, H, T, expected):
    cfg = DenoiserConfig(num_frame=T, embed_dim=D, depth=1, num_heads=H)
    net, _, eng = product_with_engine(cfg, 3, prec, sampling=2)
    keys = OTHER_KEYS + NEW_KEYS
    eng.set_option("attn_h16", 1)
    eng.set_option("attn_f32_h16", 1)
    assert {k: eng.info(k) for k in keys} == dict.fromkeys(keys, 0)      # before any forward
    inp = inputs(1, T, 500)
    out = net.forward_denoise(torch.cat([inp["x2d"], inp["noise"]], dim=-1).cuda(), torch.tensor([500]).cuda())
    assert torch.isfinite(out).all()
    assert {k: eng.info(k) for k in keys} == {**dict.fromkeys(keys, 0), **expected}
