"""Skeletons of 15 and 16 joints on the fused spatial path of the F16X3 flow (kernels_qkv_sattn.hip: k_qkv_sattn<J> and
k_qkv_sattn_direct<J, ..>, a tile of 16 whole frames x one head) and on the fp32 spatial kernel (k_attn_spatial_f32<J>).  D = 512, 8 heads,
depth 1 unless said otherwise, trained-like weights, inputs from synth_inputs(B, T, J, seed).  The (T, B) shapes are the smallest that hit
each regime of the 16-frame tile: 9 frames (less than a tile), 16 (exactly one, two batch elements), 17 (one frame into a second tile),
54 (not a multiple of 16), 21 frames of 7 batch elements (several batch elements per tile: the direct form's Q rows).
  1. proof of the path: info("fused_spatial_last") / info("block0_direct_last");
  2. bit-identity of the fused kernel and the two-kernel flow (k-loop form), of the fused and the plane-writing direct form;
  3. accuracy against oracle/d3d_oracle.py in fp64, the direct form's cost bounded by the oracle's own fp32 floor;
  4. independence: batch position, workspace contents, graph replay, stream count, non-finite neighbours;
  5. the fp32 kernel against fp64 math, beside the generic kernel."""
import pytest
import torch

from helpers import hashed, maxabs, attn_ref, torch_sd, product_with_engine, xy
from diff3dhpe_amd import _lib
from diff3dhpe_amd.spec import DenoiserConfig
from diff3dhpe_amd.synth import synth_inputs

pytestmark = pytest.mark.gpu
GATE = 1e-4
JOINTS = (15, 16)
SHAPES = [(9, 1), (8, 2), (17, 1), (27, 2), (3, 7)]


def _cfg(T, J, depth=1, **kw):
    return DenoiserConfig(num_frame=T, num_joints=J, embed_dim=512, depth=depth, **kw)


def _sd(cfg, seed=11, family="trainedlike"):   # this module's default weights: seed 11 of the trained-like family
    return torch_sd(cfg, seed, family)


def _product(cfg, seed=11, prec="f16x3", sampling=2, family="trainedlike"):   # this module's defaults; the weights of _sd
    return product_with_engine(cfg, seed, prec, sampling, family)


def _inputs(cfg, B, seed):
    return {k: torch.from_numpy(v) for k, v in synth_inputs(B, cfg.num_frame, cfg.num_joints, seed=seed).items()}


def _cfg_xy(cfg, B, seed):
    """xy() at the config's frame and joint counts; a seq2frame model takes the noise of one frame."""
    x2d, nz = xy(B, cfg.num_frame, seed, cfg.num_joints)
    return x2d, (nz[:, :1].contiguous() if cfg.seq2frame else nz)


def _sample(eng, x2d, nz, direct=1, fused=1):   # toggles "block0_direct" and "fused_spatial", reads both *_last keys
    """(output, (fused_spatial_last, block0_direct_last)) of one sampling with the two options set, defaults restored."""
    eng.set_option("block0_direct", direct)
    eng.set_option("fused_spatial", fused)
    out = eng.ddim_sample(x2d, nz).clone()
    last = (eng.info("fused_spatial_last"), eng.info("block0_direct_last"))
    eng.set_option("block0_direct", 1)
    eng.set_option("fused_spatial", 1)
    return out, last


# ------------------------------------------------------------------------------------------------ 1. proof of the path
@pytest.mark.parametrize("J,want", [(15, (1, 1)), (16, (1, 1)), (17, (1, 1)), (21, (0, 0))])
def test_the_info_keys_report_the_path_a_sampling_took(J, want):
    cfg = _cfg(9, J)
    _, _, eng = _product(cfg)
    assert (eng.info("fused_spatial_last"), eng.info("block0_direct_last")) == (0, 0)       # before any forward
    x2d, nz = _cfg_xy(cfg, 2, 70 + J)
    out, last = _sample(eng, x2d, nz)
    assert last == want and torch.isfinite(out).all()
    _, last = _sample(eng, x2d, nz, direct=0, fused=0)
    assert last == (0, 0)
    if want == (1, 1):
        assert _sample(eng, x2d, nz, direct=1, fused=0)[1] == (0, 1)
        assert _sample(eng, x2d, nz, direct=0, fused=1)[1] == (1, 0)
        assert eng.info("bf16_fused_spatial_last") == 0


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_the_key_stays_zero_on_other_precisions(prec):
    cfg = _cfg(9, 16)
    _, _, eng = _product(cfg, prec=prec)
    x2d, nz = _cfg_xy(cfg, 2, 69)
    _, last = _sample(eng, x2d, nz)
    assert last == (0, 0)


# ------------------------------------------------------------------------------------------------ 2. bit-identity
@pytest.mark.parametrize("T,B", SHAPES)
@pytest.mark.parametrize("J", JOINTS)
def test_fused_kernel_and_two_kernel_flow_are_bit_identical(J, T, B):
    """"block0_direct" = 0: every spatial block on k_qkv_sattn<J> against the folded qkv GEMM + k_attn_temporal_x3*; "block0_direct" = 1:
    block 0 on k_qkv_sattn_direct<J, 2, false> against its plane-writing form + the attention kernel."""
    cfg = _cfg(T, J)
    _, _, eng = _product(cfg)
    x2d, nz = _cfg_xy(cfg, B, 77)
    eng.range_flags(clear=True)
    for direct in (0, 1):
        fused, l1 = _sample(eng, x2d, nz, direct=direct, fused=1)
        plain, l0 = _sample(eng, x2d, nz, direct=direct, fused=0)
        assert l1 == (1, direct) and l0 == (0, direct)
        assert torch.isfinite(fused).all() and eng.range_flags() == 0
        assert torch.equal(fused, plain), (direct, maxabs(fused, plain))


@pytest.mark.parametrize("J", JOINTS)
def test_bit_identity_at_depth_2_with_a_time_per_row(J):
    T, B = 17, 3
    cfg = _cfg(T, J, depth=2)
    net, _, eng = _product(cfg)
    inp = _inputs(cfg, B, 78)
    xcat = torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1).cuda()
    t = torch.tensor([905, 17, 443], dtype=torch.long).cuda()
    for direct in (0, 1):
        eng.set_option("block0_direct", direct)
        outs = []
        for fused in (1, 0):
            eng.set_option("fused_spatial", fused)
            outs.append(net.forward_denoise(xcat, t).clone())
            assert (eng.info("fused_spatial_last"), eng.info("block0_direct_last")) == (fused, direct)
        assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1]), direct
        # the rows carry their own t: row 1 alone, with its own time, is row 1 of the batch
        eng.set_option("fused_spatial", 1)
        assert torch.equal(net.forward_denoise(xcat[1:2].contiguous(), t[1:2]), outs[0][1:2])
    eng.set_option("block0_direct", 1)


@pytest.mark.parametrize("kind", ["no_time_emb", "seq2frame"])
@pytest.mark.parametrize("J", JOINTS)
def test_bit_identity_without_time_rows_and_with_broadcast_y(J, kind):
    cfg = _cfg(27, J, with_time_emb=False) if kind == "no_time_emb" else _cfg(27, J, seq2frame=True)
    _, _, eng = _product(cfg, family="uniform", seed=5)
    x2d, nz = _cfg_xy(cfg, 3, 79)
    for direct in (0, 1):
        fused, l1 = _sample(eng, x2d, nz, direct=direct, fused=1)
        plain, l0 = _sample(eng, x2d, nz, direct=direct, fused=0)
        assert l1 == (1, direct) and l0 == (0, direct) and torch.isfinite(fused).all()
        assert torch.equal(fused, plain), direct


# ------------------------------------------------------------------------------------------------ 3. accuracy against the oracle
@pytest.mark.parametrize("J", JOINTS)
def test_forward_denoise_against_the_oracle_with_block0_direct_on_and_off(J):
    """forward_denoise at T = 27, B = 2, per-row t, against oracle/d3d_oracle.py in fp64 (the construction of
    test_gpu_block0_direct.py): both settings inside the 1e-4 gate, the direct form no worse than the GEMM by more than the oracle's own
    fp32 floor.  Measured on an MI355X: see DESIGN.md section 3."""
    from oracle import d3d_oracle as orc
    cfg = _cfg(27, J)
    net, _, eng = _product(cfg)
    sd = _sd(cfg)
    inp = _inputs(cfg, 2, 500)
    xcat = torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1)
    t = torch.tensor([905, 17], dtype=torch.long)
    ref32 = orc.forward_denoise(sd, xcat, t, depth=1)
    torch.set_default_dtype(torch.float64)      # (the oracle's sinusoid and identity follow the default dtype)
    try:
        ref64 = orc.forward_denoise({k: v.double() for k, v in sd.items()}, xcat.double(), t, depth=1)
    finally:
        torch.set_default_dtype(torch.float32)
    assert ref64.dtype == torch.float64 and tuple(ref64.shape)[-2] == J
    floor = (ref32.double() - ref64).abs().max().item()
    eng.range_flags(clear=True)
    err = {}
    for opt in (1, 0):
        eng.set_option("block0_direct", opt)
        out = net.forward_denoise(xcat.cuda(), t.cuda())
        assert (eng.info("fused_spatial_last"), eng.info("block0_direct_last")) == (1, opt)
        err[opt] = (out.cpu().double() - ref64).abs().max().item()
    eng.set_option("block0_direct", 1)
    print(f"spatial joints J={J} T=27 B=2: err_on {err[1]:.3e} err_off {err[0]:.3e} oracle fp32 floor {floor:.3e}")
    assert eng.range_flags() == 0
    assert err[1] <= GATE and err[0] <= GATE
    assert err[1] <= err[0] + floor


# ------------------------------------------------------------------------------------------------ 4. independence
@pytest.fixture(scope="module")
def indep():
    """J = 15, T = 9, B = 3: 27 frames, so the 16 trailing rows of the first tile (rows 240..255) belong to batch element 1 and the
    second tile holds the end of element 1 and element 2.  One engine, one clean sampling and one clean denoise for the tests below."""
    cfg = _cfg(9, 15)
    _, _, eng = _product(cfg)
    x2d, nz = _cfg_xy(cfg, 3, 80)
    t = torch.tensor([508.0, 77.0, 939.0], device="cuda")
    eng.set_option("streams", 2)
    eng.range_flags(clear=True)
    whole, last = _sample(eng, x2d, nz)
    den = eng.denoise(x2d, nz, t).clone()
    assert last == (1, 1) and torch.isfinite(whole).all() and torch.isfinite(den).all() and eng.range_flags(clear=True) == 0
    return eng, x2d, nz, t, whole, den


def test_every_batch_element_equals_the_element_sampled_alone(indep):
    eng, x2d, nz, _, whole, _ = indep
    for b in range(3):
        one, last = _sample(eng, x2d[b:b + 1].contiguous(), nz[b:b + 1].contiguous())
        assert last == (1, 1) and torch.equal(one, whole[b:b + 1]), b


def test_streams_and_workspace_contents_do_not_matter(indep):
    eng, x2d, nz, _, whole, _ = indep
    eng.set_option("streams", 1)
    try:
        assert torch.equal(_sample(eng, x2d, nz)[0], whole)
    finally:
        eng.set_option("streams", 2)
    eng._workspace(3).view(torch.float32).fill_(float("nan"))
    assert torch.equal(_sample(eng, x2d, nz)[0], whole)
    for direct, fused in ((0, 1), (1, 0)):          # the k-loop form reads the stream's pad rows, the plane form the q / k / v region
        a = _sample(eng, x2d, nz, direct=direct, fused=fused)[0]
        eng._workspace(3).view(torch.float32).fill_(float("nan"))
        assert torch.equal(_sample(eng, x2d, nz, direct=direct, fused=fused)[0], a), (direct, fused)


def test_graph_replay_equals_eager(indep):
    eng, x2d, nz, _, whole, _ = indep
    eng.set_graph_mode(True)
    try:
        first, l1 = _sample(eng, x2d, nz)          # eager warm-up pass + capture + replay
        again = eng.ddim_sample(x2d, nz).clone()   # replay of the cached graph
        assert eng.info("graphs_cached") >= 1
    finally:
        eng.set_graph_mode(False)
    assert l1 == (1, 1)
    assert torch.equal(first, whole) and torch.equal(again, whole)


@pytest.mark.parametrize("poison", ["x2d_one_nan", "x2d_all_inf", "y_one_nan"])
@pytest.mark.parametrize("direct", [1, 0])
def test_a_non_finite_batch_element_stays_alone(indep, poison, direct):
    """Batch element 1 non-finite (the pattern of tests/test_gpu_isolation.py part B): elements 0 and 2 are bit-equal to the clean run,
    and element 1 never comes back finite with a clean guard word.  Both forms: the direct fill and the k-loop."""
    eng, x2d, nz, t, _, _ = indep
    bx, by = x2d.clone(), nz.clone()
    if poison == "x2d_one_nan":
        bx[1, 3, 5, 0] = float("nan")
    elif poison == "x2d_all_inf":
        bx[1] = float("inf")
    else:
        by[1, 3, 5, 0] = float("nan")
    clean = torch.tensor([True, False, True], device="cuda")
    eng.set_option("block0_direct", direct)
    try:
        eng.range_flags(clear=True)
        den0 = eng.denoise(x2d, nz, t).clone()
        ddim0 = eng.ddim_sample(x2d, nz).clone()
        assert (eng.info("fused_spatial_last"), eng.info("block0_direct_last")) == (1, direct)
        assert torch.isfinite(den0).all() and torch.isfinite(ddim0).all() and eng.range_flags(clear=True) == 0
        den = eng.denoise(bx, by, t)
        flags = eng.range_flags(clear=True)
        assert torch.equal(den[clean], den0[clean])
        finite = torch.isfinite(den[~clean])
        assert not finite.any() or flags & _lib.RANGE_PRECISION, f"SILENT: {int(finite.sum())} finite values, guard word {flags:#x}"
        out = eng.ddim_sample(bx, by)
        assert torch.equal(out[clean], ddim0[clean])
    finally:
        eng.range_flags(clear=True)
        eng.set_option("block0_direct", 1)


# ------------------------------------------------------------------------------------------------ 5. fp32
@pytest.mark.parametrize("B,T,J", [(2, 5, 15), (2, 5, 16), (3, 23, 15)])
def test_fp32_spatial_attention_against_fp64(B, T, J):
    """k_attn_spatial_f32<15> / <16> (four units per wave; at 15 joints four idle lanes, at (3, 23, 15) a ragged last block) to the bound
    test_attention_core holds 17 joints to, the generic kernel beside it."""
    from diff3dhpe_amd import engine as E
    qkv = hashed(f"qkv{T}_{J}_512", (B * T * J, 3 * 512), 21, 2.0).cuda()
    ref = attn_ref(qkv, B, T, J, 8, False).cpu()
    fast = E.op_attention(qkv, B, T, J, 8, False)
    gen = E.op_attention(qkv, B, T, J, 8, False, force_generic=True)
    print(f"fp32 spatial attention J={J} B={B} T={T}: fast {maxabs(fast, ref):.3e} generic {maxabs(gen, ref):.3e}")
    assert maxabs(fast, ref) < 5e-6 and maxabs(gen, ref) < 5e-6


@pytest.mark.parametrize("J", JOINTS)
def test_fp32_spatial_attention_on_a_sharp_softmax(J):
    from diff3dhpe_amd import engine as E
    B, T = 2, 7
    qkv = hashed(f"sharp{T}_{J}", (B * T * J, 3 * 512), 22, 9.0).cuda()
    ref = attn_ref(qkv, B, T, J, 8, False).cpu()
    a = E.op_attention(qkv, B, T, J, 8, False)
    b = E.op_attention(qkv, B, T, J, 8, False, force_generic=True)
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert maxabs(a, ref) < 2e-3 and maxabs(b, ref) < 2e-3 and maxabs(a, b.cpu()) < 2e-3


def test_fp32_engine_sampling_at_16_joints_against_the_oracle():
    from oracle import d3d_oracle as orc
    cfg = _cfg(27, 16)
    _, diff, _ = _product(cfg, seed=33, prec="fp32", family="uniform")
    inp = _inputs(cfg, 2, 346)
    _, y0 = diff(clean_3d_pose=torch.zeros_like(inp["noise"]).cuda(), noisy_2d_pose=inp["x2d"].cuda(), output_loss=False,
                 init_noise=inp["noise"].cuda())
    ref = orc.ddim_sample_loop(_sd(cfg, 33, "uniform"), orc.diffusion_tables("cosine", 1000), inp["x2d"], inp["noise"],
                               num_timesteps=1000, sampling_timesteps=2, depth=cfg.depth)
    assert tuple(y0.shape) == (2, 27, 16, 3) and maxabs(y0, ref) <= GATE, maxabs(y0, ref)
