#!/usr/bin/env python3
"""Skeletons of 15 and 16 joints on an F16X3 engine: the fused spatial kernels ("fused_spatial" = 1, "block0_direct" = 1: k_qkv_sattn<J> and
k_qkv_sattn_direct<J, ..>, kernels_qkv_sattn.hip) against both options at 0 -- the folded qkv GEMM + k_attn_temporal_x3* in every spatial
block, launch for launch what the tree before the 16-frame tile ran at these joint counts.  J in {15, 16} x (T, B) in {(243, 64),
(243, 1), (81, 128)}, depth 8, D = 512, 9 steps, hipGraph replay.

Two engines hold the same weights in ONE process, one per setting; the legs alternate for REPEATS rounds of N samplings each, every
sampling timed from the host around a device synchronise.  A leg's figure is the median of its round medians, the off leg's spread is
max - min of its round medians; "ahead_in_every_round" says whether the on leg beat the off leg by more than that spread in every
alternation (the condition for shipping the path on by default at these joint counts).  A profiling pass (eager launches, one stream, HIP
events around every kernel) gives the per-launch times of the spatial kernels in both modes.  Writes profiles/spatial_joints.json (or the
path given with --out).

--fp32: the fp32 spatial attention kernel k_attn_spatial_f32<J> against the generic one-thread-per-row kernel (d3d_op_attention with
force_generic, what an FP32 engine launched at these joint counts before), per launch at the same token counts, into the same file's
"fp32" list.

    python experiments/spatial_joints.py [--fp32] [--out FILE] [--samples 5] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import diff3dhpe_amd as d3d  # noqa: E402
from diff3dhpe_amd.spec import DenoiserConfig  # noqa: E402
from diff3dhpe_amd.synth import synth_state_dict, synth_inputs, hash_uniform  # noqa: E402

STEPS = 9
SHAPES = [(243, 64), (243, 1), (81, 128)]


def product(T, J, sd, on):
    net = d3d.HPE_model(d3d.S2S_NAME)(num_frame=T, num_joints=J, embed_dim=512, depth=8)
    net.load_state_dict(sd)
    net.precision = "f16x3"
    diff = d3d.GaussianDiffusion(model=net, timesteps=1000, sampling_timesteps=STEPS, loss_type="l2", clip_denoised=True).eval().cuda()
    eng = diff._engine(torch.device("cuda", torch.cuda.current_device()))
    eng.set_option("fused_spatial", int(on))
    eng.set_option("block0_direct", int(on))
    return eng, net, diff   # (the engine lives as long as its model)


def samplings_ms(eng, x2d, nz, n):
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.ddim_sample(x2d, nz)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def per_launch(eng, x2d, nz):
    """us per launch of the kernels of the spatial blocks, from the profiling API (one stream, eager)."""
    eng.set_graph_mode(False)
    eng.set_option("streams", 1)
    eng.set_profiling(True)
    eng.ddim_sample(x2d, nz)
    torch.cuda.synchronize()
    eng.profile_reset()
    eng.ddim_sample(x2d, nz)
    torch.cuda.synchronize()
    p = eng.profile_read()
    eng.set_profiling(False)
    eng.set_option("streams", 2)
    eng.set_graph_mode(True)
    out = {}
    for c in ("qkv_sattn", "attn_spatial", "linear_qkv"):
        if p.get(c, {}).get("launches"):
            out[c + "_us"] = 1e3 * p[c]["ms"] / p[c]["launches"]
            out[c + "_launches"] = p[c]["launches"]
    out["spatial_ms"] = sum(p[c]["ms"] for c in ("qkv_sattn", "attn_spatial", "linear_qkv") if c in p)
    return out


def fp32_cells(joints, samples):
    from diff3dhpe_amd import engine as E
    cells = []
    for J in joints:
        for T, B in SHAPES:
            B = min(B, 16)      # (B T J, 3 D) fp32 rows: 16 sequences of 243 frames are 0.36 GB
            n = B * T * J * 3 * 512
            qkv = torch.from_numpy(hash_uniform(f"sj{J}_{T}", n, 3).astype("float32").reshape(B * T * J, 3 * 512) * 2.0).cuda()
            us = {}
            for name, generic in (("fast", False), ("generic", True)):
                E.op_attention(qkv, B, T, J, 8, False, force_generic=generic)
                ts = []
                for _ in range(samples):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = E.op_attention(qkv, B, T, J, 8, False, force_generic=generic)
                    e1.record()
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1) * 1e3)
                us[name] = statistics.median(ts)
                us[name + "_out"] = out
            cell = {"J": J, "T": T, "B": B, "fast_us": us["fast"], "generic_us": us["generic"],
                    "max_abs_between": (us["fast_out"] - us["generic_out"]).abs().max().item()}
            cells.append(cell)
            print(f"fp32 J={J} T={T} B={B}: k_attn_spatial_f32 {cell['fast_us']:.1f} us, generic {cell['generic_us']:.1f} us", flush=True)
    return cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fp32", action="store_true", help="the fp32 spatial attention kernel against the generic one, per launch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial_joints.json"))
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--joints", type=int, nargs="*", default=[15, 16])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.setdefault("device", torch.cuda.get_device_name(0))
    res.setdefault("cus", torch.cuda.get_device_properties(0).multi_processor_count)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)

    if a.fp32:
        res["fp32_what"] = (f"d3d_op_attention, spatial, fp32, D = 512, 8 heads: k_attn_spatial_f32<J> against force_generic (k_attn_generic), us per "
                            f"launch, median of {a.samples} (HIP events)")
        res["fp32"] = fp32_cells(a.joints, a.samples)
        save()
        print(a.out)
        return
    res["what"] = (f"{STEPS}-step DDIM sampling, F16X3, depth 8, D = 512, hipGraph replay, (fused_spatial, block0_direct) = (1, 1) (on) vs (0, 0) (off: "
                   f"the launches of the tree before the 16-frame tile), two engines with the same weights alternating in one process; ms are "
                   f"medians of {a.repeats} round medians of {a.samples} samplings; spread = max - min of the off leg's round medians")
    res["cells"] = []
    for J in a.joints:
        for T, B in SHAPES:
            cfg = DenoiserConfig(num_frame=T, num_joints=J, embed_dim=512, depth=8)
            sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 0).items()}
            legs = {"on": product(T, J, sd, True), "off": product(T, J, sd, False)}
            inp = synth_inputs(B, T, J, seed=1)
            x2d, nz = torch.from_numpy(inp["x2d"]).cuda(), torch.from_numpy(inp["noise"]).cuda()
            outs, ran = {}, {}
            for name, (eng, _, _) in legs.items():      # warm-up: eager pass + capture + replays
                eng.set_graph_mode(True)
                for _ in range(2):
                    outs[name] = eng.ddim_sample(x2d, nz).clone()
                ran[name] = (eng.info("fused_spatial_last"), eng.info("block0_direct_last"))
            torch.cuda.synchronize()
            assert ran == {"on": (1, 1), "off": (0, 0)}, ran
            med = {"on": [], "off": []}
            for _ in range(a.repeats):
                for name, (eng, _, _) in legs.items():
                    med[name].append(statistics.median(samplings_ms(eng, x2d, nz, a.samples)))
            spread = max(med["off"]) - min(med["off"])
            cell = {"J": J, "B": B, "T": T, "on_ms": statistics.median(med["on"]), "off_ms": statistics.median(med["off"]), "off_spread_ms": spread,
                    "on_round_medians_ms": med["on"], "off_round_medians_ms": med["off"],
                    "ahead_in_every_round": bool(all(off - on > spread for on, off in zip(med["on"], med["off"]))),
                    "max_abs_between_modes": (outs["on"] - outs["off"]).abs().max().item(),
                    "per_launch": {name: per_launch(eng, x2d, nz) for name, (eng, _, _) in legs.items()}}
            cell["gain_ms"] = cell["off_ms"] - cell["on_ms"]
            res["cells"].append(cell)
            pl = cell["per_launch"]
            print(f"J={J} T={T} B={B}: on {cell['on_ms']:.3f} ms, off {cell['off_ms']:.3f} ms (spread {spread:.3f}), gain {cell['gain_ms']:+.3f} ms, "
                  f"ahead in every round: {cell['ahead_in_every_round']}; max-abs between modes {cell['max_abs_between_modes']:.3e}; spatial "
                  f"kernels {pl['off']['spatial_ms']:.2f} -> {pl['on']['spatial_ms']:.2f} ms per sampling", flush=True)
            save()
            del legs
    print(a.out)


if __name__ == "__main__":
    main()
