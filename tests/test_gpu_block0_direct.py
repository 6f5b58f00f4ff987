"""Block 0 of the F16X3 folded flow from the raw input channels ("block0_direct", kernels_qkv_sattn.hip k_qkv_sattn_direct): its input rows
are W_e u + b_e + spos[j] + tv[b] with u the in_chans + 3 channels of a token, so Wg x0 = G u + P[j] + Q[b] -- commit-time tables and one
time row per forward instead of the K = 512 qkv GEMM.  D = 512, small T and B: the shapes where the 15-frame tile geometry can go wrong
(tiles that hold rows of two to five batch elements, ragged last tiles, one and several tiles).
  * accuracy against the oracle with the option on and off, the option's cost bounded by the oracle's own fp32 floor;
  * bit-identity of the fused kernel and the plane-writing kernel (the property the project keeps for every block);
  * row isolation: batch position, stream count, workspace contents;
  * graph replay == eager;
  * proof of the path through info("block0_direct_last")."""
from functools import partial

import pytest
import torch

from helpers import inputs, torch_sd, product_with_engine, xy
from diff3dhpe_amd.spec import DenoiserConfig

pytestmark = pytest.mark.gpu
GATE = 1e-4
DEPTH = 1            # one spatial + one temporal block: the smallest depth the config accepts; block 0 is what changes


def _cfg(T, **kw):
    return DenoiserConfig(num_frame=T, embed_dim=512, depth=DEPTH, **kw)


def _product(cfg, seed=11, prec="f16x3", sampling=2, family="trainedlike", **ctor):   # this module's defaults
    return product_with_engine(cfg, seed, prec, sampling, family, **ctor)


def _cfg_xy(cfg, B, seed):
    """xy() at the config's frame and joint counts; a seq2frame model takes the noise of one frame."""
    x2d, nz = xy(B, cfg.num_frame, seed, cfg.num_joints)
    return x2d, (nz[:, :1].contiguous() if cfg.seq2frame else nz)


def _sample(eng, x2d, nz, direct=1, fused=1):   # toggles "block0_direct" and "fused_spatial", reads "block0_direct_last"
    eng.set_option("block0_direct", direct)
    eng.set_option("fused_spatial", fused)
    out = eng.ddim_sample(x2d, nz).clone()
    last = eng.info("block0_direct_last")
    eng.set_option("block0_direct", 1)
    eng.set_option("fused_spatial", 1)
    return out, last


# ------------------------------------------------------------------------------------------------ 1 (+ 6). accuracy, on and off
VARIANTS = {"default": {}, "nobias_qkscale_eps1e-3": dict(qkv_bias=False, qk_scale=0.2, norm_layer=partial(torch.nn.LayerNorm, eps=1e-3))}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_forward_denoise_against_the_oracle_with_the_option_on_and_off(variant):
    """forward_denoise at T = 27, B = 2, trained-like weights, depth 1, per-row t, against oracle/d3d_oracle.py in fp64: both settings
    inside the project's 1e-4 gate, and the direct form no worse than the GEMM by more than the oracle's own fp32 floor (the distance
    between the oracle in fp32 and in fp64 on these inputs).  The second variant builds the tables from a model with qkv_bias=False, a
    qk_scale and LayerNorm eps = 1e-3 (the table builder needs the device, so its check against an fp64 evaluation is this one)."""
    from oracle import d3d_oracle as orc
    ctor = VARIANTS[variant]
    cfg = _cfg(27)
    net, _, eng = _product(cfg, **ctor)
    sd = torch_sd(cfg, 11, "trainedlike", ctor.get("qkv_bias", True))
    inp = inputs(2, 27, 500)
    xcat = torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1)
    t = torch.tensor([905, 17], dtype=torch.long)
    okw = dict(depth=DEPTH, qk_scale=ctor.get("qk_scale"), norm_eps=1e-3 if "norm_layer" in ctor else 1e-6)
    ref32 = orc.forward_denoise(sd, xcat, t, **okw)
    torch.set_default_dtype(torch.float64)      # (the oracle's sinusoid and identity follow the default dtype)
    try:
        ref64 = orc.forward_denoise({k: v.double() for k, v in sd.items()}, xcat.double(), t, **okw)
    finally:
        torch.set_default_dtype(torch.float32)
    assert ref64.dtype == torch.float64
    floor = (ref32.double() - ref64).abs().max().item()
    eng.range_flags(clear=True)
    err = {}
    for opt in (1, 0):
        eng.set_option("block0_direct", opt)
        out = net.forward_denoise(xcat.cuda(), t.cuda())
        assert eng.info("block0_direct_last") == opt
        err[opt] = (out.cpu().double() - ref64).abs().max().item()
    eng.set_option("block0_direct", 1)
    print(f"block0_direct [{variant}] T=27 B=2: err_on {err[1]:.3e} err_off {err[0]:.3e} oracle fp32 floor {floor:.3e}")
    assert eng.range_flags() == 0
    assert err[1] <= GATE and err[0] <= GATE
    assert err[1] <= err[0] + floor


# ------------------------------------------------------------------------------------------------ 2. fused == plane-writing kernel
# 9, 27, 54, 135 frames: below / multiples of / not multiples of the 15-frame tile; at T = 9 a tile holds rows of two batch elements, at
# T = 3 (21 frames) the first tile holds five whole batch elements and the second the other two
SHAPES = [(9, 1), (9, 3), (27, 2), (27, 5), (3, 7)]


@pytest.mark.parametrize("T,B", SHAPES)
def test_fused_and_two_kernel_flow_are_bit_identical_in_a_sampling(T, B):
    cfg = _cfg(T)
    _, _, eng = _product(cfg)
    x2d, nz = _cfg_xy(cfg, B, 77)
    eng.range_flags(clear=True)
    fused, l1 = _sample(eng, x2d, nz, fused=1)
    plain, l0 = _sample(eng, x2d, nz, fused=0)
    assert l1 == 1 and l0 == 1
    assert torch.isfinite(fused).all() and eng.range_flags() == 0
    assert torch.equal(fused, plain)


@pytest.mark.parametrize("T,B", SHAPES)
def test_fused_and_two_kernel_flow_are_bit_identical_with_a_time_per_row(T, B):
    cfg = _cfg(T)
    net, _, eng = _product(cfg)
    inp = inputs(B, T, 78)
    xcat = torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1).cuda()
    t = torch.tensor([905, 17, 443, 0, 999, 250, 611][:B], dtype=torch.long).cuda()
    outs = []
    for fused in (1, 0):
        eng.set_option("fused_spatial", fused)
        outs.append(net.forward_denoise(xcat, t).clone())
        assert eng.info("block0_direct_last") == 1
    eng.set_option("fused_spatial", 1)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    if B > 1:      # the rows carry their own t: row 1 alone, with its own time, is row 1 of the batch
        assert torch.equal(net.forward_denoise(xcat[1:2].contiguous(), t[1:2]), outs[0][1:2])


@pytest.mark.parametrize("kind", ["no_time_emb", "seq2frame"])
def test_fused_and_two_kernel_flow_are_bit_identical_without_time_rows_and_with_broadcast_y(kind):
    cfg = _cfg(27, with_time_emb=False) if kind == "no_time_emb" else _cfg(27, seq2frame=True)
    _, _, eng = _product(cfg, family="uniform", seed=5)
    x2d, nz = _cfg_xy(cfg, 3, 79)
    fused, l1 = _sample(eng, x2d, nz, fused=1)
    plain, l0 = _sample(eng, x2d, nz, fused=0)
    assert l1 == 1 and l0 == 1 and torch.isfinite(fused).all()
    assert torch.equal(fused, plain)


# ------------------------------------------------------------------------------------------------ 3. row isolation
def test_rows_do_not_depend_on_batch_streams_or_workspace_contents():
    cfg = _cfg(9)               # 9 frames per batch element: each 15-frame tile of a B = 3 call holds rows of two of them
    _, _, eng = _product(cfg)
    x2d, nz = _cfg_xy(cfg, 3, 80)
    eng.set_option("streams", 2)
    whole, last = _sample(eng, x2d, nz)
    assert last == 1
    for b in range(3):
        one, last = _sample(eng, x2d[b:b + 1].contiguous(), nz[b:b + 1].contiguous())
        assert last == 1 and torch.equal(one, whole[b:b + 1])
    eng.set_option("streams", 1)
    assert torch.equal(_sample(eng, x2d, nz)[0], whole)
    eng.set_option("streams", 2)
    eng._workspace(3).view(torch.float32).fill_(float("nan"))
    assert torch.equal(_sample(eng, x2d, nz)[0], whole)


# ------------------------------------------------------------------------------------------------ 4. graph replay
def test_graph_replay_equals_eager():
    cfg = _cfg(9)
    _, _, eng = _product(cfg)
    x2d, nz = _cfg_xy(cfg, 2, 81)
    eager, last = _sample(eng, x2d, nz)
    eng.set_graph_mode(True)
    try:
        first, l1 = _sample(eng, x2d, nz)          # eager warm-up pass + capture + replay
        again = eng.ddim_sample(x2d, nz).clone()   # replay of the cached graph
        assert eng.info("graphs_cached") >= 1
    finally:
        eng.set_graph_mode(False)
    assert last == 1 and l1 == 1
    assert torch.equal(first, eager) and torch.equal(again, eager)


# ------------------------------------------------------------------------------------------------ 5. path proof
def test_option_off_is_the_gemm_flow_and_other_precisions_never_take_the_direct_form():
    cfg = _cfg(27)
    _, _, eng = _product(cfg)
    x2d, nz = _cfg_xy(cfg, 2, 82)
    on, l_on = _sample(eng, x2d, nz, direct=1)
    off_fused, l_off1 = _sample(eng, x2d, nz, direct=0, fused=1)
    off_plain, l_off0 = _sample(eng, x2d, nz, direct=0, fused=0)
    assert (l_on, l_off1, l_off0) == (1, 0, 0)
    assert torch.equal(off_fused, off_plain)                  # the parent's arithmetic: its own bit-identity holds
    assert torch.isfinite(on).all()
    for prec in ("bf16", "fp32"):
        _, _, e2 = _product(cfg, prec=prec)
        _, last = _sample(e2, x2d, nz)
        assert last == 0, prec
