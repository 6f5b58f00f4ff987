#!/usr/bin/env python3
"""Heads of 48 and 96 columns (embed_dim 384 / 768 with the runner's 8 heads) on an FP32 engine: the attention of the spatial and temporal
blocks on kernels_attn_f32_hx.hip ("attn_f32_hx" = 1, include/d3d.h) against the generic one-thread-per-row kernel ("attn_f32_hx" = 0:
launch for launch what the tree before the option ran).  Per width (T, B) in {(27, 1), (27, 64), (243, 1), (243, 16)}, depth 8, 9 steps,
hipGraph replay.  T = 243 streams the temporal blocks at width 96 (243 > 192 frames) and keeps them resident at width 48.

Two engines hold the same weights in ONE process, one with the option on and one with it off; the legs alternate for REPEATS rounds of N
samplings each, every sampling timed from the host around a device synchronise.  A leg's figure is the median of its round medians, the
off leg's spread is max - min of its round medians; "ahead_in_every_round" says whether the on leg beat the off leg by more than that
spread in every alternation (the condition for shipping the option on by default).  An op-level pass times the kernels alone against
op_attention(..., force_generic=True) on the qkv shape of one forward: HIP events around each launch, median of OP_LAUNCHES.  Writes
profiles/attn_f32_hx.json (or the path given with --out).

    python experiments/attn_f32_hx.py [--out FILE] [--samples 5] [--repeats 5] [--widths 384 768] [--cells 27x1 27x64 243x1 243x16]
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
from diff3dhpe_amd import engine as E  # noqa: E402
from diff3dhpe_amd.spec import DenoiserConfig  # noqa: E402
from diff3dhpe_amd.synth import synth_state_dict, synth_inputs, hash_uniform  # noqa: E402

STEPS = 9
KEY = "attn_f32_hx"
HEADS, DEPTH, JOINTS = 8, 8, 17
RESIDENT_MAX = {48: 256, 96: 192}
OP_LAUNCHES = 21


def product(T, width, sd, on):
    net = d3d.HPE_model(d3d.S2S_NAME)(num_frame=T, embed_dim=width, depth=DEPTH, num_heads=HEADS)
    net.load_state_dict(sd)
    net.precision = "fp32"
    diff = d3d.GaussianDiffusion(model=net, timesteps=1000, sampling_timesteps=STEPS, loss_type="l2", clip_denoised=True).eval().cuda()
    eng = diff._engine(torch.device("cuda", torch.cuda.current_device()))
    eng.set_option(KEY, int(on))
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


def op_median_us(fn):
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(OP_LAUNCHES):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return statistics.median(us)


def per_launch(B, T, width):
    """Median us per launch of each block type's attention alone, new kernel and generic kernel, on the qkv rows of one forward of B."""
    rows = B * T * JOINTS
    resident = T <= RESIDENT_MAX[width // HEADS]
    qkv = torch.from_numpy(hash_uniform("expqkv", rows * 3 * width, 21).astype("float32").reshape(rows, 3 * width) * 2.0).cuda()
    temporal_op = (lambda: E.op_attention_f32_hx(qkv, B, T, JOINTS, HEADS, True)) if resident else \
                  (lambda: E.op_attention_long_f32_hx(qkv, B, T, JOINTS, HEADS))
    out = {"temporal_kernel": "resident" if resident else "streaming"}
    for name, fn, temporal in (("spatial", lambda: E.op_attention_f32_hx(qkv, B, T, JOINTS, HEADS, False), False),
                               ("temporal", temporal_op, True)):
        out[name + "_us"] = op_median_us(fn)
        out[name + "_generic_us"] = op_median_us(lambda: E.op_attention(qkv, B, T, JOINTS, HEADS, temporal, force_generic=True))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", KEY + ".json"))
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--widths", nargs="*", type=int, default=[384, 768])
    ap.add_argument("--cells", nargs="*", default=["27x1", "27x64", "243x1", "243x16"], help="TxB")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    res = {"what": f"{STEPS}-step DDIM sampling, FP32, depth {DEPTH}, {HEADS} heads, hipGraph replay, {KEY} 1 (on) vs 0 (off: the launches of "
                   f"the tree before the option), two engines with the same weights alternating in one process; ms are medians of "
                   f"{a.repeats} round medians of {a.samples} samplings; spread = max - min of the off leg's round medians; per_launch: "
                   f"median of {OP_LAUNCHES} event-timed launches of the op hooks",
           "device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count, "cells": []}
    for width in a.widths:
        for T, B in (tuple(int(v) for v in c.split("x")) for c in a.cells):
            cfg = DenoiserConfig(num_frame=T, embed_dim=width, depth=DEPTH, num_heads=HEADS)
            sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 0).items()}
            legs = {"off": product(T, width, sd, False), "on": product(T, width, sd, True)}
            inp = synth_inputs(B, T, seed=1)
            x2d, nz = torch.from_numpy(inp["x2d"]).cuda(), torch.from_numpy(inp["noise"]).cuda()
            outs, ran = {}, {}
            for name, (eng, _, _) in legs.items():      # warm-up: eager pass + capture + replays
                eng.set_graph_mode(True)
                for _ in range(2):
                    outs[name] = eng.ddim_sample(x2d, nz).clone()
                ran[name] = eng.info(KEY + "_last")
            torch.cuda.synchronize()
            assert ran == {"on": 3 if T <= RESIDENT_MAX[width // HEADS] else 5, "off": 0}, ran
            med = {"on": [], "off": []}
            for _ in range(a.repeats):
                for name, (eng, _, _) in legs.items():
                    med[name].append(statistics.median(samplings_ms(eng, x2d, nz, a.samples)))
            spread = max(med["off"]) - min(med["off"])
            cell = {"D": width, "B": B, "T": T, "last": ran["on"], "on_ms": statistics.median(med["on"]),
                    "off_ms": statistics.median(med["off"]), "off_spread_ms": spread,
                    "on_round_medians_ms": med["on"], "off_round_medians_ms": med["off"],
                    "ahead_in_every_round": bool(all(off - on > spread for on, off in zip(med["on"], med["off"]))),
                    "smallest_lead_ms": min(off - on for on, off in zip(med["on"], med["off"])),
                    "max_abs_between_modes": (outs["on"] - outs["off"]).abs().max().item(),
                    "per_launch": per_launch(B, T, width)}
            cell["gain_ms"] = cell["off_ms"] - cell["on_ms"]
            res["cells"].append(cell)
            pl = cell["per_launch"]
            print(f"D={width} T={T} B={B}: on {cell['on_ms']:.3f} ms, off {cell['off_ms']:.3f} ms (spread {spread:.3f}), gain "
                  f"{cell['gain_ms']:+.3f} ms, smallest lead {cell['smallest_lead_ms']:+.3f} ms, ahead in every round: "
                  f"{cell['ahead_in_every_round']}; max-abs between modes {cell['max_abs_between_modes']:.3e}; spatial attention "
                  f"{pl['spatial_generic_us']:.1f} -> {pl['spatial_us']:.1f}, temporal ({pl['temporal_kernel']}) "
                  f"{pl['temporal_generic_us']:.1f} -> {pl['temporal_us']:.1f} us per launch", flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(res, open(a.out, "w"), indent=1)
            del legs
    print(a.out)


if __name__ == "__main__":
    main()
