"""Round-4 evidence on the MI355X, through the product API / the C ABI:
  * the fixtures VERDICT r03 found missing: seq2frame without time embedding (the reference's 3DHP command lines), the trained-like
    family on the seq2frame model, the trained-like family in the bf16 operand mode,
  * `python bench.py --gpus 2` with NO launcher (bench.py starts its rank processes itself), two ranks on ONE device over gloo; on a
    box with two devices also over RCCL, and nn.DataParallel over two devices with allow_multi_device,
  * a repeated two-process sampling as the run-time cross-check of the head kernel on a shared GPU,
  * the F16X3 range-guard word per ENGINE, the hipGraph cache bound (LRU of 4), graph warm-up from staged inputs,
  * p_losses' weighted loss and the repeat_n tiling / hypothesis mean as engine kernels (d3d_weighted_loss, d3d_repeat_batch,
    d3d_hypothesis_mean) against their host-framework formulas, bit for bit,
  * a module moved with .to() between devices / engines."""
import numpy as np
import pytest
import torch

from conftest import gold
from helpers import cfg_full, cfg_small, inputs, build_product, product, maxabs, torch_sd, bench_subprocess, clean_env
import diff3dhpe_amd as d3d
from diff3dhpe_amd import _lib
from diff3dhpe_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu
GATE = 1e-4
PRECS = ["fp32", "f16x3"]


# ------------------------------------------------------------------------------------------------ the missing fixtures
CASES = [("s2f_notemb_T27", cfg_full(27, seq2frame=True, with_time_emb=False), "uniform"),
         ("trainedlike_s2f_T27", cfg_full(27, seq2frame=True), "trainedlike")]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tag,cfg,family", CASES, ids=[c[0] for c in CASES])
def test_forward_denoise_golden_round4(tag, cfg, family, prec):
    g = gold("denoise_" + tag)
    net, diff = product(cfg, int(g["seed"]), prec, family=family)
    eng = diff._engine(torch.device("cuda", torch.cuda.current_device()))
    eng.range_flags(clear=True)
    inp = inputs(2, 27, int(g["input_seed"]))
    xcat = torch.cat([inp["x2d"], inp["noise"] * float(g["y_scale"])], dim=-1).cuda()
    worst = 0.0
    for t in (999, 443, 0):
        out = net.forward_denoise(xcat, torch.full((2,), t, dtype=torch.long, device="cuda"))
        assert out.shape == g[f"t{t}"].shape == (2, 1, 17, 3)
        worst = max(worst, maxabs(out, g[f"t{t}"]))
    worst = max(worst, maxabs(net.forward_denoise(xcat, torch.from_numpy(g["tmixed_t"]).long().cuda()), g["tmixed"]))
    print(f"denoise {tag} [{prec}]: max-abs {worst:.3e}")
    assert eng.range_flags() == 0 and worst <= GATE


@pytest.mark.parametrize("prec", PRECS)
def test_ddim_loop_golden_seq2frame_without_time_embedding(prec):
    """The 3DHP command line (Experiments.sh:15-17): ...S2F... model, with_time_emb False, 7 DDIM steps, (B, 1, J, 3) targets."""
    g = gold("ddim_s2f_notemb_T27_S7")
    cfg = cfg_full(27, seq2frame=True, with_time_emb=False)
    _, diff = product(cfg, int(g["seed"]), prec, sampling=int(g["S"]))
    inp = inputs(int(g["B"]), 27, int(g["input_seed"]))
    noise = inp["noise"][:, :1].contiguous()
    loss, y0 = diff(clean_3d_pose=torch.zeros_like(noise).cuda(), noisy_2d_pose=inp["x2d"].cuda(), output_loss=False, init_noise=noise.cuda())
    e = maxabs(y0, g["y0"])
    print(f"ddim s2f notemb T=27 S=7 [{prec}]: max-abs {e:.3e}")
    assert loss is None and y0.shape == g["y0"].shape and e <= GATE and y0.abs().max().item() <= 1.0


def test_bf16_mode_on_the_trainedlike_family():
    """Second-class bf16 operand mode on heavy-tailed weights / wide LayerNorm gains: gated like tests/test_gpu_bf16.py, against the
    oracle's bf16-operand emulation (same rounding points) at 1.5x the emulation's own fp32-vs-fp64-accumulation distance."""
    from oracle import d3d_oracle as orc
    from test_gpu_bf16 import _emulations, _mpjpe, GATE_MAXABS, GATE_MPJPE
    cfg = cfg_full(27)
    net, _ = product(cfg, 11, "bf16", family="trainedlike")
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 11, family="trainedlike").items()}
    inp = inputs(2, 27, 500)
    xcat = torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1)
    t = torch.tensor([905, 17], dtype=torch.long)
    out = net.forward_denoise(xcat.cuda(), t.cuda())
    e32, e64, f32 = _emulations(orc.forward_denoise, sd, xcat, t, depth=8)
    e1, m1, self_m, self_e = maxabs(out, e32), _mpjpe(out, e32), _mpjpe(e32, e64), maxabs(e32, e64)
    print(f"bf16 trained-like denoise T=27: engine vs emulation max-abs {e1:.3e} MPJPE {m1:.3e} | emulation self-distance max-abs {self_e:.3e} "
          f"MPJPE {self_m:.3e} | engine vs fp32 oracle MPJPE {_mpjpe(out, f32):.3e}")
    assert torch.isfinite(out).all()
    assert e1 <= max(GATE_MAXABS, 1.5 * self_e) and m1 <= max(1.5 * self_m, GATE_MPJPE)


# ------------------------------------------------------------------------------------------------ multi-process / multi-device
COMMON = ["--steps", "1", "--warmup", "0", "--frames", "27", "--sampling", "3", "--no-cpu-baseline", "--no-extras"]


def test_bench_dump_outputs_is_the_timed_result_and_repeats(tmp_path):
    """bench.py --dump-outputs: two runs with the same arguments write the same files, bit for bit; --steps sets the timed steps; the
    dumped sums are the ones behind the line's MPJPE, and the dumped prediction is the batch's (B, T, J, 3) poses."""
    args = ["--gpus", "1", "--batch", "4", "--steps", "2", "--warmup", "1", "--frames", "27", "--sampling", "3", "--no-cpu-baseline",
            "--no-extras", "--profile-steps", "0"]
    lines = [bench_subprocess(args + ["--dump-outputs", str(tmp_path / f"run{i}")], clean_env()) for i in range(2)]
    assert all(l["steps"] == 2 and l["ms_per_step"] > 0 for l in lines)
    pred = [np.load(tmp_path / f"run{i}" / "pred.npy") for i in range(2)]
    sums = [np.load(tmp_path / f"run{i}" / "mpjpe_sums.npy") for i in range(2)]
    assert pred[0].dtype == np.float32 and pred[0].shape == (4, 27, 17, 3) and np.isfinite(pred[0]).all()
    assert np.array_equal(pred[0], pred[1]) and np.array_equal(sums[0], sums[1])
    assert lines[0]["mpjpe_vs_synthetic_gt"] == round(sums[0][0] / sums[0][1], 6)


def test_bench_self_launch_two_ranks_on_one_device():
    """`python bench.py --gpus 2` -- NO torchrun in the command: bench.py starts its two rank processes itself (before torch or HIP
    are touched), they share cuda:0 through gloo (D3D_BENCH_ONE_DEVICE=1), rank 0's single JSON line is relayed, and the gathered
    MPJPE equals the one-process value for the same global batch."""
    two = bench_subprocess(["--gpus", "2", "--batch", "3"] + COMMON, clean_env(D3D_BENCH_ONE_DEVICE="1", D3D_DIST_BACKEND="gloo"))
    one = bench_subprocess(["--gpus", "1", "--batch", "6"] + COMMON, clean_env())
    assert two["n_gpus"] == 2 and two["config"]["global_batch"] == 6 == one["config"]["global_batch"]
    assert two["mpjpe_vs_synthetic_gt"] == one["mpjpe_vs_synthetic_gt"]
    assert two["dist"]["launcher"] == "self" and two["dist"]["world_size"] == 2 and two["dist"]["backend"] == "gloo"
    assert two["ranks"]["allgather_bytes_per_rank"] == 3 * 27 * 17 * 3 * 4 and "dist" not in one


def test_two_ranks_on_one_device_repeat():
    """Run-time cross-check of the head kernel on a GPU shared by two processes (its deviation showed in ~1 launch of 60 with the
    compiler's free instruction stream; the kept stream is pinned by tests/test_abi_host.py, the mechanism is open): five two-rank
    runs at T = 81 (2 samplings x 9 steps x 2 ranks each = 180 head launches beside the other rank's GEMMs) must all report the same
    MPJPE, bit for bit.  The 20-run T = 243 form stays opt-in (tests/test_gpu_parity.py, D3D_SLOW_TESTS=1)."""
    env = clean_env(D3D_BENCH_ONE_DEVICE="1", D3D_DIST_BACKEND="gloo")
    seen = set()
    for i in range(5):
        line = bench_subprocess(["--gpus", "2", "--batch", "2", "--steps", "2", "--warmup", "0", "--frames", "81", "--sampling", "9",
                            "--no-cpu-baseline", "--no-extras", "--no-selfcheck", "--profile-steps", "0"], env)
        seen.add(line["mpjpe_vs_synthetic_gt"])
    assert len(seen) == 1, seen


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two HIP devices")
def test_bench_self_launch_two_ranks_on_two_devices_rccl():
    """Plain `python bench.py --gpus 2`, backend nccl (RCCL), one process per GPU: MPJPE == the one-rank value for the same batch."""
    two = bench_subprocess(["--gpus", "2", "--batch", "3"] + COMMON, clean_env(HSA_ENABLE_IPC_MODE_LEGACY="0"))
    one = bench_subprocess(["--gpus", "1", "--batch", "6"] + COMMON, clean_env())
    assert two["dist"]["backend"] == "nccl" and two["dist"]["world_size"] == 2 and two["dist"]["one_process_per_gpu"]
    assert two["mpjpe_vs_synthetic_gt"] == one["mpjpe_vs_synthetic_gt"]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two HIP devices")
def test_data_parallel_over_two_devices_with_allow_multi_device():
    """The reference's own multi-device form (RUN:216-218, `--gpu_id 0,1`): nn.DataParallel over two devices in ONE process, behind
    the explicit allow_multi_device switch -- one engine per device, driven from DataParallel's worker threads.  Without the switch
    the second device is refused loudly; with it the wrapped result equals the bare module's."""
    cfg = cfg_full(27)
    net, diff = build_product(cfg, 5, sampling=3, precision="f16x3")
    inp = inputs(4, 27, 31)
    x2d, nz = inp["x2d"].cuda(0), inp["noise"].cuda(0)
    z = torch.zeros_like(nz)
    _, bare = diff(clean_3d_pose=z, noisy_2d_pose=x2d, output_loss=False, init_noise=nz)
    dp = torch.nn.DataParallel(diff, device_ids=[0, 1])
    with pytest.raises(Exception, match="ONE device per process"):
        dp(clean_3d_pose=z, noisy_2d_pose=x2d, output_loss=False, init_noise=nz)
    type(net).allow_multi_device = True
    try:
        _, wrapped = dp(clean_3d_pose=z, noisy_2d_pose=x2d, output_loss=False, init_noise=nz)
    finally:
        type(net).allow_multi_device = False
    assert wrapped.shape == bare.shape and torch.equal(wrapped.cpu(), bare.cpu())


def test_module_moved_between_engines_keeps_working():
    """A model that ran, is moved with .to() (here: to the CPU and back -- on a two-device box also to cuda:1), and runs again: the stale
    engine is released instead of raising 'ONE device per process' (ADVICE r03)."""
    cfg = cfg_small(27)
    net, diff = build_product(cfg, 5, sampling=2, precision="fp32")
    inp = inputs(2, 27, 31)
    z = torch.zeros_like(inp["noise"])
    _, a = diff(clean_3d_pose=z.cuda(), noisy_2d_pose=inp["x2d"].cuda(), output_loss=False, init_noise=inp["noise"].cuda())
    diff.cpu()
    diff.cuda()
    _, b = diff(clean_3d_pose=z.cuda(), noisy_2d_pose=inp["x2d"].cuda(), output_loss=False, init_noise=inp["noise"].cuda())
    assert torch.equal(a, b)
    if torch.cuda.device_count() >= 2:
        diff.to("cuda:1")
        _, c = diff(clean_3d_pose=z.to("cuda:1"), noisy_2d_pose=inp["x2d"].to("cuda:1"), output_loss=False, init_noise=inp["noise"].to("cuda:1"))
        assert c.device.index == 1 and torch.equal(c.cpu(), a.cpu()) and list(net._engines) == [1]


# ------------------------------------------------------------------------------------------------ engine state
def test_range_guard_word_belongs_to_the_engine():
    """Two engines on one device: the one that meets an out-of-range activation raises ITS flag; the healthy engine beside it reads
    0 before and after, and its read does not consume the other's flag (the word used to be per device, cleared on read)."""
    cfg = cfg_full(27)
    cfg1 = type(cfg)(num_frame=27, embed_dim=512, depth=1)
    inp = inputs(2, 27, 3)
    x2d, nz = inp["x2d"].cuda(), inp["noise"].cuda()
    dev = torch.device("cuda", torch.cuda.current_device())

    def make(mutate):
        sd = torch_sd(cfg1, 8)
        mutate(sd)
        net = d3d.HPE_model(d3d.S2S_NAME)(num_frame=27, embed_dim=512, depth=1)
        net.load_state_dict(sd)
        net.precision = "f16x3"
        net.range_check = False          # raw words are read below (the default reading: tests/test_gpu_round5.py)
        diff = d3d.GaussianDiffusion(model=net, timesteps=1000, sampling_timesteps=2, clip_denoised=True).eval().to(dev)
        return diff, diff._engine(dev)

    def big_x(sd):
        sd["fusion_layer.bias"] += 1.0e4
    good, eg = make(lambda sd: None)
    bad, eb = make(big_x)
    for d in (good, bad, good):
        d(clean_3d_pose=torch.zeros_like(nz), noisy_2d_pose=x2d, output_loss=False, init_noise=nz)
    assert eg.range_flags() == 0                              # the healthy engine saw nothing -- and consumed nothing:
    assert eb.range_flags(clear=False) & _lib.RANGE_ACT
    assert eg.range_flags() == 0
    with pytest.raises(_lib.D3DError, match="range"):
        eb.check_range()
    assert eb.range_flags() == 0                              # cleared by its own check
    # both internal streams of one call report to the same word (B >= 2 runs as two half-batches on two streams)
    eb.set_option("streams", 2)
    bad(clean_3d_pose=torch.zeros_like(nz), noisy_2d_pose=x2d, output_loss=False, init_noise=nz)
    assert eb.range_flags() & _lib.RANGE_ACT and eg.range_flags() == 0


def test_hipgraph_cache_is_bounded_and_the_first_replay_is_clean():
    """d3d_engine_set_graph_mode keeps at most four captured graphs (least recently used evicted): a caller that re-allocates its
    workspace per batch does not accumulate graphs.  The capture's eager warm-up pass runs on the STAGED inputs, so a workspace
    full of large finite garbage cannot set the sticky range words (D3D_CHECK_RANGE=1 would raise a spurious error)."""
    cfg = cfg_full(27)
    cfgd = type(cfg)(num_frame=27, embed_dim=512, depth=1)
    _, diff = build_product(cfgd, 5, sampling=2, precision="f16x3")
    dev = torch.device("cuda", torch.cuda.current_device())
    eng = diff._engine(dev)
    inp = inputs(7, 27, 77)
    x2d, nz = inp["x2d"].cuda(), inp["noise"].cuda()
    eager = {B: eng.ddim_sample(x2d[:B].contiguous(), nz[:B].contiguous()).clone() for B in range(1, 8)}
    eng.set_graph_mode(True)
    try:
        eng.range_flags(clear=True)
        eng._ws = None
        eng._workspace(7).view(torch.float32).fill_(3.0e4)     # |8 x| > 65504 if the warm-up pass read it
        assert torch.equal(eng.ddim_sample(x2d, nz), eager[7])
        assert eng.range_flags() == 0
        for B in (1, 2, 3, 4, 5, 6):                           # seven distinct (B, workspace) pairs in all
            assert torch.equal(eng.ddim_sample(x2d[:B].contiguous(), nz[:B].contiguous()), eager[B])
        assert eng.info("graphs_captured") == 7 and eng.info("graphs_cached") == 4
        n = eng.info("graphs_captured")
        assert torch.equal(eng.ddim_sample(x2d[:6].contiguous(), nz[:6].contiguous()), eager[6])     # most recent: still cached
        assert eng.info("graphs_captured") == n
        assert torch.equal(eng.ddim_sample(x2d, nz), eager[7])                                     # evicted long ago: re-captured
        assert eng.info("graphs_captured") == n + 1 and eng.info("graphs_cached") == 4
    finally:
        eng.set_graph_mode(False)
    assert eng.info("graphs_cached") == 0


# ------------------------------------------------------------------------------------------------ f2 / f3 arithmetic in the engine
@pytest.mark.parametrize("loss_type,clip", [("l2", True), ("l2", False), ("l1", True)])
def test_weighted_loss_kernel_matches_the_host_formula_bit_for_bit(loss_type, clip):
    """d3d_weighted_loss (DIFF:411-418): loss_fn(model_out, target, 'none') * (1 + ac[t] / sqrt(1 - ac)[t]).clamp(max=3) -- the same
    fp32 operations in the same order as the host framework's ops, so equality is exact."""
    import torch.nn.functional as F
    cfg = cfg_small(27)
    _, diff = build_product(cfg, 5, sampling=2, precision="fp32")
    diff.loss_type, diff.clipLoss = loss_type, clip
    eng = diff._engine(torch.device("cuda", torch.cuda.current_device()))
    g = torch.Generator().manual_seed(3)
    mo, tg = torch.randn(9, 27, 17, 3, generator=g).cuda(), torch.randn(9, 27, 17, 3, generator=g).cuda()
    t = torch.tensor([0, 1, 110, 443, 700, 887, 950, 998, 999]).cuda()
    got = eng.weighted_loss(mo, tg, t, loss_type, clip)
    ac, so = diff.alphas_cumprod, diff.sqrt_one_minus_alphas_cumprod
    coef = 1.0 + ac[t].view(-1, 1, 1, 1) / so[t].view(-1, 1, 1, 1)
    if clip:
        coef = torch.clamp(coef, max=3.0)
    ref = (F.mse_loss if loss_type == "l2" else F.l1_loss)(mo, tg, reduction="none") * coef
    assert torch.equal(got, ref)
    assert (coef.max().item() == 3.0) == clip                   # the clamp is active in this set of timesteps


def test_repeat_and_hypothesis_mean_kernels():
    from diff3dhpe_amd.engine import hypothesis_mean, repeat_batch
    g = torch.Generator().manual_seed(5)
    x = torch.randn(5, 27, 17, 2, generator=g).cuda()
    assert torch.equal(repeat_batch(x, 3), x.repeat(3, 1, 1, 1)) and repeat_batch(x, 1) is x
    p = torch.randn(15, 27, 17, 3, generator=g).cuda()
    ref = torch.mean(p.view(3, 5, 27, 17, -1), dim=0, keepdim=True).squeeze(0)
    got = hypothesis_mean(p, 3)
    assert got.shape == ref.shape and (got - ref).abs().max().item() <= 2.4e-7     # (sum order of a 3-term fp32 mean)
    pc = p.cpu()                     # the pinned reference is the CPU path: sum in hypothesis order, then a true division
    seq = (pc[:5] + pc[5:10] + pc[10:]) / 3.0          # (the host framework's GPU kernels multiply by 1/R instead: 1 ulp apart)
    assert torch.equal(got.cpu(), seq)


def test_repeat_n_with_cpu_inputs_returns_on_the_inputs_device():
    """forward(repeat_n = R) with CPU tensors in: tiling and hypothesis mean run as engine kernels, the prediction comes back on the
    inputs' device, and equals the golden made by the imported reference (the GPU-input form of this golden: test_gpu_parity.py;
    p_losses through d3d_weighted_loss: test_p_losses_and_q_sample there and at D = 512 in test_gpu_round3.py)."""
    from helpers import hashed
    g = gold("ddim_small_T27_S4_eta05_rep3")
    cfg = cfg_small(27)
    B, S, R = int(g["B"]), int(g["S"]), int(g["R"])
    _, diff = build_product(cfg, int(g["seed"]), sampling=S, eta=0.5, precision="fp32")
    inp = inputs(B * R, 27, int(g["input_seed"]))
    step_noise = torch.stack([hashed(f"eta_noise/{i}", tuple(inp["noise"].shape), 6) for i in range(S)])
    _, y0 = diff(clean_3d_pose=torch.zeros(B, 27, 17, 3), noisy_2d_pose=inp["x2d"][:B], output_loss=False,
                 repeat_n=R, init_noise=inp["noise"], step_noise=step_noise)
    assert y0.shape == (B, 27, 17, 3) and not y0.is_cuda
    assert maxabs(y0, g["y0"]) <= GATE


# ------------------------------------------------------------------------------------------------ fused spatial blocks
@pytest.mark.parametrize("T,B,family", [(27, 2, "uniform"), (81, 3, "uniform"), (27, 5, "trainedlike"), (243, 9, "uniform"), (9, 1, "uniform")])
def test_fused_spatial_blocks_are_bit_identical_to_the_two_kernel_flow(T, B, family):
    """"fused_spatial" (default): the spatial blocks' LayerNorm-folded qkv GEMM and 17-key attention as one kernel (q / k / v stay in
    LDS: kernels_qkv_sattn.hip).  Same MFMAs in the same order per element, same epilogue and attention arithmetic: the sampling is
    bit for bit the one of the two-kernel flow -- whose parity against the reference the golden tests establish.  Frame counts
    that are / are not multiples of the 15-frame tile, one to many tiles per workgroup, both weight families, the range guard silent."""
    cfg = cfg_full(T)
    _, diff = product(cfg, 11 if family == "trainedlike" else 5, "f16x3", sampling=2, family=family)
    eng = diff._engine(torch.device("cuda", torch.cuda.current_device()))
    inp = inputs(B, T, 77)
    x2d, nz = inp["x2d"].cuda(), inp["noise"].cuda()
    eng.range_flags(clear=True)
    eng.set_option("fused_spatial", 1)
    fused = eng.ddim_sample(x2d, nz).clone()
    eng.set_option("fused_spatial", 0)
    plain = eng.ddim_sample(x2d, nz).clone()
    eng.set_option("fused_spatial", 1)
    assert torch.isfinite(fused).all() and eng.range_flags() == 0
    assert torch.equal(fused, plain)


def test_fused_spatial_blocks_with_garbage_workspace_and_large_batch():
    """The fused spatial kernel stages rows beyond the matrix (its 255-row tiles over a 256-row padded stream), the fused temporal one
    repeats a group's last frame in its pad rows: neither may let them reach a stored value: workspace filled with NaN, B = 32 at
    T = 243 (30 / 17 tiles per workgroup, ragged last M-tile), two streams."""
    cfg = cfg_full(243)
    _, diff = product(cfg, 5, "f16x3", sampling=1)
    eng = diff._engine(torch.device("cuda", torch.cuda.current_device()))
    inp = inputs(32, 243, 78)
    x2d, nz = inp["x2d"].cuda(), inp["noise"].cuda()
    eng.set_option("fused_spatial", 0)
    eng.set_option("fused_temporal", 0)                          # (both block types as two kernels: the flow the goldens pinned first)
    plain = eng.ddim_sample(x2d, nz).clone()
    eng.set_option("fused_spatial", 1)
    eng.set_option("fused_temporal", 1)
    eng._workspace(32).view(torch.float32).fill_(float("nan"))
    fused = eng.ddim_sample(x2d, nz)
    assert torch.equal(fused, plain)
    for lo in (0, 13):                                           # and batch-size independent, as every kernel of the engine
        assert torch.equal(eng.ddim_sample(x2d[lo:lo + 13].contiguous(), nz[lo:lo + 13].contiguous()), plain[lo:lo + 13])


# ------------------------------------------------------------------------------------------------ machine probes
def test_machine_probes_report_plausible_ceilings():
    """d3d_probe_machine (bench.py's "machine_probes"): the sustained fp16 MFMA rate lies under the nominal 2.5 PFLOP/s and above the
    rate the GEMM class itself reaches; the staging stream from L2 runs well above what HBM could deliver; bad arguments are refused."""
    from diff3dhpe_amd.engine import probe_machine
    pm = probe_machine(ms_target=40.0)
    assert 1100.0 < pm["mfma_f16_tflops"] < 2500.0, pm
    assert 8000.0 < pm["l2_to_lds_gbps"] < 60000.0, pm
    import ctypes as C
    r = C.c_float(0.0)
    L = _lib.lib()
    assert L.d3d_probe_machine(2, 10.0, C.byref(r), None) == -1
    assert L.d3d_probe_machine(0, 0.0, C.byref(r), None) == -1
    assert L.d3d_probe_machine(0, 10.0, None, None) == -1


# ------------------------------------------------------------------------------------------------ fused temporal blocks
@pytest.mark.parametrize("T,B,family", [(243, 2, "uniform"), (243, 9, "trainedlike"), (200, 3, "uniform"), (255, 1, "uniform"), (193, 2, "trainedlike")])
def test_fused_temporal_blocks_are_bit_identical_to_the_two_kernel_flow(T, B, family):
    """"fused_temporal": the temporal blocks' LayerNorm-folded qkv GEMM and T-key attention as one kernel where the frames of a joint fit
    one 256-row tile (kernels_qkv_tattn.hip: K / V planes and the query exchange in LDS).  Same MFMAs in the same order per element, the
    epilogue arithmetic of the qkv GEMM and the attention arithmetic of k_attn_temporal_x3s: the sampling is bit for bit the one of
    the two-kernel flow.  Frame counts with and without pad rows in the tile, few and many groups per workgroup, both weight families."""
    cfg = cfg_full(T)
    _, diff = product(cfg, 11 if family == "trainedlike" else 5, "f16x3", sampling=2, family=family)
    eng = diff._engine(torch.device("cuda", torch.cuda.current_device()))
    inp = inputs(B, T, 78)
    x2d, nz = inp["x2d"].cuda(), inp["noise"].cuda()
    eng.range_flags(clear=True)
    eng.set_option("fused_temporal", 1)
    fused = eng.ddim_sample(x2d, nz).clone()
    eng.set_option("fused_temporal", 0)
    plain = eng.ddim_sample(x2d, nz).clone()
    eng.set_option("fused_temporal", 1)
    again = eng.ddim_sample(x2d, nz).clone()
    assert torch.isfinite(fused).all() and eng.range_flags() == 0
    assert torch.equal(fused, plain) and torch.equal(fused, again)


def test_fused_temporal_blocks_with_another_joint_count():
    """The fused temporal kernel walks a group's frames by the joint stride: 21 joints (the spatial blocks then take the two-kernel
    flow -- their fusion needs 17), T = 200, depth 2: against the CPU oracle inside the gate, and bit for bit the two-kernel flow."""
    from oracle import d3d_oracle as orc
    from diff3dhpe_amd.spec import DenoiserConfig
    from diff3dhpe_amd.synth import synth_inputs
    J, T = 21, 200
    cfg = DenoiserConfig(num_frame=T, num_joints=J, embed_dim=512, depth=2)
    net, diff = build_product(cfg, 34, sampling=2, precision="f16x3")
    inp = {k: torch.from_numpy(v) for k, v in synth_inputs(2, T, J, seed=351).items()}
    eng = diff._engine(torch.device("cuda", torch.cuda.current_device()))
    x2d, nz = inp["x2d"].cuda(), inp["noise"].cuda()
    eng.set_option("fused_temporal", 1)
    fused = eng.ddim_sample(x2d, nz).clone()
    eng.set_option("fused_temporal", 0)
    plain = eng.ddim_sample(x2d, nz).clone()
    eng.set_option("fused_temporal", 1)
    ref = orc.ddim_sample_loop(torch_sd(cfg, 34), orc.diffusion_tables("cosine", 1000), inp["x2d"], inp["noise"], num_timesteps=1000,
                               sampling_timesteps=2, depth=cfg.depth)
    assert torch.equal(fused, plain)
    assert maxabs(fused, ref) <= GATE, maxabs(fused, ref)


@pytest.mark.parametrize("T,B,family,s2f", [(81, 5, "uniform", False), (81, 3, "trainedlike", False), (27, 7, "uniform", True), (27, 4, "trainedlike", False),
                                            (100, 2, "uniform", False), (9, 3, "uniform", False)])
def test_fused_temporal_blocks_grouped_form_for_short_sequences(T, B, family, s2f):
    """T <= 127: the fused temporal kernel takes the frames of 255 / T joints of ONE batch element per tile (k_qkv_tattn<true>): a query sees
    the keys of its own joint only, and only the key tiles that hold them are computed.  Its softmax sums and key-tile products are
    grouped differently from the stand-alone attention kernels, so it is NOT bit-identical to the two-kernel flow: within 2e-5 of it
    (both are ~2e-6 from the oracle), inside the gate against the CPU oracle, deterministic, NaN-filled workspace, and -- which joints
    share a tile depends on the joint index alone -- every batch element's result bit for bit the one it has when sampled alone."""
    from oracle import d3d_oracle as orc
    cfg = cfg_full(T, seq2frame=s2f)
    seed = 11 if family == "trainedlike" else 5
    _, diff = product(cfg, seed, "f16x3", sampling=2, family=family)
    eng = diff._engine(torch.device("cuda", torch.cuda.current_device()))
    inp = inputs(B, T, 83)
    x2d = inp["x2d"].cuda()
    nz = (inp["noise"][:, :1] if s2f else inp["noise"]).contiguous().cuda()
    eng.range_flags(clear=True)
    eng.set_option("fused_temporal", 1)
    eng._workspace(B).view(torch.float32).fill_(float("nan"))
    fused = eng.ddim_sample(x2d, nz).clone()
    again = eng.ddim_sample(x2d, nz).clone()
    alone = torch.cat([eng.ddim_sample(x2d[i:i + 1].contiguous(), nz[i:i + 1].contiguous()).clone() for i in range(B)])
    eng.set_option("fused_temporal", 0)
    plain = eng.ddim_sample(x2d, nz).clone()
    eng.set_option("fused_temporal", 1)
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, seed, family=family).items()}
    ref = orc.ddim_sample_loop(sd, orc.diffusion_tables("cosine", 1000), inp["x2d"], nz.cpu(), num_timesteps=1000, sampling_timesteps=2,
                               depth=cfg.depth, seq2frame=s2f)
    e_plain, e_ref = maxabs(fused, plain.cpu()), maxabs(fused, ref)
    print(f"grouped fused temporal T={T} B={B} [{family}{', s2f' if s2f else ''}]: vs two-kernel flow {e_plain:.3e}, vs oracle {e_ref:.3e}")
    assert torch.isfinite(fused).all() and eng.range_flags() == 0
    assert torch.equal(fused, again) and torch.equal(fused, alone)
    assert e_plain <= 2e-5 and e_ref <= GATE


def test_fused_temporal_grouped_form_with_another_joint_count():
    """21 joints at T = 27: 9 joints per tile, three tiles per batch element, the last with three joints (six joint slots of pad rows)."""
    from oracle import d3d_oracle as orc
    from diff3dhpe_amd.spec import DenoiserConfig
    from diff3dhpe_amd.synth import synth_inputs
    J, T = 21, 27
    cfg = DenoiserConfig(num_frame=T, num_joints=J, embed_dim=512, depth=2)
    net, diff = build_product(cfg, 35, sampling=2, precision="f16x3")
    inp = {k: torch.from_numpy(v) for k, v in synth_inputs(3, T, J, seed=352).items()}
    eng = diff._engine(torch.device("cuda", torch.cuda.current_device()))
    x2d, nz = inp["x2d"].cuda(), inp["noise"].cuda()
    eng.set_option("fused_temporal", 1)
    fused = eng.ddim_sample(x2d, nz).clone()
    eng.set_option("fused_temporal", 0)
    plain = eng.ddim_sample(x2d, nz).clone()
    eng.set_option("fused_temporal", 1)
    ref = orc.ddim_sample_loop(torch_sd(cfg, 35), orc.diffusion_tables("cosine", 1000), inp["x2d"], inp["noise"], num_timesteps=1000,
                               sampling_timesteps=2, depth=cfg.depth)
    assert maxabs(fused, plain.cpu()) <= 2e-5 and maxabs(fused, ref) <= GATE, (maxabs(fused, plain.cpu()), maxabs(fused, ref))


# ------------------------------------------------------------------------------------------------ dedicated fc1 kernel
@pytest.mark.parametrize("T,B,family", [(243, 32, "uniform"), (243, 33, "trainedlike"), (81, 96, "uniform")])
def test_fc1_kernel_is_bit_identical_to_the_template_form(T, B, family):
    """"fc1_kernel" (default): fc1 on its own kernel (kernels_fc1_x3.hip: the hand-specialised k-loop of the fused kernels, whole 256-row
    tiles over padded buffers) from two rounds of tiles on; same MFMAs in the same order and the template's own epilogue function: bit
    for bit the token GEMM's LN-folded GELU form.  Ragged last M-tile (rows beyond the matrix are staged and multiplied, never read
    back), NaN-filled workspace, the range guard silent."""
    cfg = cfg_full(T)
    _, diff = product(cfg, 11 if family == "trainedlike" else 5, "f16x3", sampling=1, family=family)
    eng = diff._engine(torch.device("cuda", torch.cuda.current_device()))
    inp = inputs(B, T, 79)
    x2d, nz = inp["x2d"].cuda(), inp["noise"].cuda()
    eng.set_option("fc1_kernel", 0)
    plain = eng.ddim_sample(x2d, nz).clone()
    eng.set_option("fc1_kernel", 1)
    eng._workspace(B).view(torch.float32).fill_(float("nan"))
    eng.range_flags(clear=True)
    own = eng.ddim_sample(x2d, nz).clone()
    assert torch.isfinite(own).all() and eng.range_flags() == 0
    assert torch.equal(own, plain)


@pytest.mark.parametrize("T,B,family", [(243, 32, "uniform"), (243, 33, "trainedlike"), (81, 97, "uniform")])
def test_proj_kernel_is_bit_identical_to_the_template_form(T, B, family):
    """"proj_kernel" (default): proj on its own kernel (kernels_proj_x3.hip: whole 192-row tiles on the hand-specialised k-loop, the
    template's own epilogue function; the rows behind the last whole tile through the template's checked forms): bit for bit the
    token GEMM's plane-residual + row-statistics form.  Token counts that are and are not multiples of 192, NaN-filled workspace."""
    cfg = cfg_full(T)
    _, diff = product(cfg, 11 if family == "trainedlike" else 5, "f16x3", sampling=1, family=family)
    eng = diff._engine(torch.device("cuda", torch.cuda.current_device()))
    inp = inputs(B, T, 80)
    x2d, nz = inp["x2d"].cuda(), inp["noise"].cuda()
    eng.set_option("proj_kernel", 0)
    plain = eng.ddim_sample(x2d, nz).clone()
    eng.set_option("proj_kernel", 1)
    eng._workspace(B).view(torch.float32).fill_(float("nan"))
    eng.range_flags(clear=True)
    own = eng.ddim_sample(x2d, nz).clone()
    assert torch.isfinite(own).all() and eng.range_flags() == 0
    assert torch.equal(own, plain)
