#!/usr/bin/env python3
"""Default path against "latency_mode" (include/d3d.h) for small calls: B in {1, 2, 4} x T in {27, 81, 243}, 9 steps, F16X3, hipGraph replay.

Both legs run in ONE process, interleaved: REPEATS rounds of (default: N samplings, latency mode: N samplings), each sampling timed from
the host around a device synchronise; a leg's figure is the median of its round medians, the default leg's spread is max - min of its round
medians.  A profiling pass (eager launches, one stream, HIP events around every kernel) then gives the per-launch time of fc2 and of the
row kernel in both modes.  Writes profiles/latency_mode.json (or the path given with --out).

    python experiments/latency_mode.py [--out FILE] [--samples 20] [--repeats 5]
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


def product(T, latency):
    cfg = DenoiserConfig(num_frame=T, embed_dim=512, depth=8)
    net = d3d.HPE_model(d3d.S2S_NAME)(num_frame=T, embed_dim=512, depth=8)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 0).items()})
    net.precision = "f16x3"
    net.latency_mode = latency
    diff = d3d.GaussianDiffusion(model=net, timesteps=1000, sampling_timesteps=STEPS, loss_type="l2", clip_denoised=True).eval().cuda()
    return diff._engine(torch.device("cuda", torch.cuda.current_device())), net, diff   # (the engine lives as long as its model)


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
    """us per launch of fc2 (+ post-norm, default path) / of the split GEMM, and of the row kernels, from the profiling API."""
    eng.set_graph_mode(False)
    eng.set_profiling(True)
    eng.ddim_sample(x2d, nz)
    torch.cuda.synchronize()
    eng.profile_reset()
    eng.ddim_sample(x2d, nz)
    torch.cuda.synchronize()
    p = eng.profile_read()
    split = eng.info("fc2_split_last")   # (profiling runs the whole batch on one stream: for B >= 2 not the replay's half-batches)
    eng.set_profiling(False)
    eng.set_graph_mode(True)
    us = lambda c: (1e3 * p[c]["ms"] / p[c]["launches"]) if p[c]["launches"] else None
    return {"S_profiled": split, "fc2_us": us("linear_fc2"), "fc2_launches": p["linear_fc2"]["launches"],
            "row_kernel_us": us("layernorm"), "row_kernel_launches": p["layernorm"]["launches"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latency_mode.json"))
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="*", default=[27, 81, 243])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 2, 4])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    res = {"what": f"{STEPS}-step DDIM sampling, F16X3, hipGraph replay, default path vs latency_mode, interleaved in one process; ms are medians "
                   f"of {a.repeats} round medians of {a.samples} samplings; spread = max - min of the default leg's round medians",
           "device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count, "cells": []}
    for T in a.frames:
        legs = {"default": product(T, False), "latency": product(T, True)}
        for B in a.batches:
            inp = synth_inputs(B, T, seed=1)
            x2d, nz = torch.from_numpy(inp["x2d"]).cuda(), torch.from_numpy(inp["noise"]).cuda()
            outs, split = {}, {}
            for name, (eng, _, _) in legs.items():      # warm-up: eager pass + capture + replays
                eng.set_graph_mode(True)
                for _ in range(3):
                    outs[name] = eng.ddim_sample(x2d, nz)
                split[name] = eng.info("fc2_split_last")
            torch.cuda.synchronize()
            med = {"default": [], "latency": []}
            for _ in range(a.repeats):
                for name, (eng, _, _) in legs.items():
                    med[name].append(statistics.median(samplings_ms(eng, x2d, nz, a.samples)))
            cell = {"B": B, "T": T, "S": split["latency"],
                    "default_ms": statistics.median(med["default"]), "latency_ms": statistics.median(med["latency"]),
                    "default_spread_ms": max(med["default"]) - min(med["default"]),
                    "default_round_medians_ms": med["default"], "latency_round_medians_ms": med["latency"],
                    "max_abs_between_modes": (outs["default"] - outs["latency"]).abs().max().item(),
                    "per_launch": {name: per_launch(eng, x2d, nz) for name, (eng, _, _) in legs.items()}}
            cell["gain_ms"] = cell["default_ms"] - cell["latency_ms"]
            res["cells"].append(cell)
            print(f"T={T:3d} B={B} S={cell['S']}: default {cell['default_ms']:.3f} ms (spread {cell['default_spread_ms']:.3f}), latency mode "
                  f"{cell['latency_ms']:.3f} ms, gain {cell['gain_ms']:+.3f} ms; fc2 {cell['per_launch']['default']['fc2_us']:.1f} -> "
                  f"{cell['per_launch']['latency']['fc2_us']:.1f} us, row kernels {cell['per_launch']['latency']['row_kernel_us']} us",
                  flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(res, open(a.out, "w"), indent=1)
        del legs
    print(a.out)


if __name__ == "__main__":
    main()
