#!/usr/bin/env python3
"""Heads of 32 columns (embed_dim 256 with the runner's 8 heads) on an F16X3 engine: the folded flow with the attention of every block on
kernels_attn_x3_h32.hip ("attn_h32" = 1, include/d3d.h) against the plain row-kernel flow with the generic fp32 attention ("attn_h32" = 0:
launch for launch what the tree before the option ran).  (T, B) in {27, 81, 243} x {1, 64}, depth 8, 9 steps, hipGraph replay.

Two engines hold the same weights in ONE process, one with the option on and one with it off; the legs alternate for REPEATS rounds of N
samplings each, every sampling timed from the host around a device synchronise.  A leg's figure is the median of its round medians, the
off leg's spread is max - min of its round medians; "ahead_in_every_round" says whether the on leg beat the off leg by more than that
spread in every alternation (the condition for shipping the option on by default).  A profiling pass (eager launches, one stream, HIP
events around every kernel) gives the per-launch time of the spatial and the temporal attention in both modes.  Writes
profiles/attn_h32.json (or the path given with --out).

    python experiments/attn_h32.py [--out FILE] [--samples 5] [--repeats 5] [--frames 27 81 243] [--batches 1 64]
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
from diff3dhpe_amd.synth import synth_state_dict, synth_inputs  # noqa: E402

STEPS = 9
KEY = "attn_h32"
WIDTH, HEADS, DEPTH = 256, 8, 8


def product(T, sd, on):
    net = d3d.HPE_model(d3d.S2S_NAME)(num_frame=T, embed_dim=WIDTH, depth=DEPTH, num_heads=HEADS)
    net.load_state_dict(sd)
    net.precision = "f16x3"
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


def per_launch(eng, x2d, nz):
    """us per launch of the two attention kernels from the profiling API (one stream, eager), and the sum over all kernel classes."""
    eng.set_graph_mode(False)
    eng.set_profiling(True)
    eng.ddim_sample(x2d, nz)
    torch.cuda.synchronize()
    eng.profile_reset()
    eng.ddim_sample(x2d, nz)
    torch.cuda.synchronize()
    p = eng.profile_read()
    eng.set_profiling(False)
    eng.set_graph_mode(True)
    us = lambda c: (1e3 * p[c]["ms"] / p[c]["launches"]) if p.get(c, {}).get("launches") else None
    return {"attn_spatial_us": us("attn_spatial"), "attn_spatial_launches": p.get("attn_spatial", {}).get("launches"),
            "attn_temporal_us": us("attn_temporal"), "attn_temporal_launches": p.get("attn_temporal", {}).get("launches"),
            "total_ms": sum(v["ms"] for k, v in p.items() if not k.startswith("linear_"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", KEY + ".json"))
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="*", default=[27, 81, 243])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    res = {"what": f"{STEPS}-step DDIM sampling, F16X3, depth {DEPTH}, D = {WIDTH}, {HEADS} heads, hipGraph replay, {KEY} 1 (on) vs 0 (off: the "
                   f"launches of the tree before the option), two engines with the same weights alternating in one process; ms are medians of "
                   f"{a.repeats} round medians of {a.samples} samplings; spread = max - min of the off leg's round medians",
           "device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count, "cells": []}
    for T in a.frames:
        cfg = DenoiserConfig(num_frame=T, embed_dim=WIDTH, depth=DEPTH, num_heads=HEADS)
        sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 0).items()}
        legs = {"on": product(T, sd, True), "off": product(T, sd, False)}
        for B in a.batches:
            inp = synth_inputs(B, T, seed=1)
            x2d, nz = torch.from_numpy(inp["x2d"]).cuda(), torch.from_numpy(inp["noise"]).cuda()
            outs, ran = {}, {}
            for name, (eng, _, _) in legs.items():      # warm-up: eager pass + capture + replays
                eng.set_graph_mode(True)
                for _ in range(2):
                    outs[name] = eng.ddim_sample(x2d, nz).clone()
                ran[name] = eng.info(KEY + "_last")
            torch.cuda.synchronize()
            assert ran == {"on": 1, "off": 0}, ran
            med = {"on": [], "off": []}
            for _ in range(a.repeats):
                for name, (eng, _, _) in legs.items():
                    med[name].append(statistics.median(samplings_ms(eng, x2d, nz, a.samples)))
            spread = max(med["off"]) - min(med["off"])
            cell = {"B": B, "T": T, "on_ms": statistics.median(med["on"]), "off_ms": statistics.median(med["off"]), "off_spread_ms": spread,
                    "on_round_medians_ms": med["on"], "off_round_medians_ms": med["off"],
                    "ahead_in_every_round": bool(all(off - on > spread for on, off in zip(med["on"], med["off"]))),
                    "max_abs_between_modes": (outs["on"] - outs["off"]).abs().max().item(),
                    "per_launch": {name: per_launch(eng, x2d, nz) for name, (eng, _, _) in legs.items()}}
            cell["gain_ms"] = cell["off_ms"] - cell["on_ms"]
            res["cells"].append(cell)
            pl = cell["per_launch"]
            print(f"T={T} B={B}: on {cell['on_ms']:.3f} ms, off {cell['off_ms']:.3f} ms (spread {spread:.3f}), gain {cell['gain_ms']:+.3f} ms, ahead in "
                  f"every round: {cell['ahead_in_every_round']}; max-abs between modes {cell['max_abs_between_modes']:.3e}; spatial attention "
                  f"{pl['off']['attn_spatial_us']:.1f} -> {pl['on']['attn_spatial_us']:.1f}, temporal {pl['off']['attn_temporal_us']:.1f} -> "
                  f"{pl['on']['attn_temporal_us']:.1f} us per launch", flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(res, open(a.out, "w"), indent=1)
        del legs
    print(a.out)


if __name__ == "__main__":
    main()
