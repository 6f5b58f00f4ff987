#!/usr/bin/env python3
"""The fp16 operand mode (D3D_PREC_F16) beside bf16 and F16X3: throughput and distance to the F16X3 result, same weights, same inputs.

ONE process holds a bf16, an f16 and an f16x3 engine per shape and alternates them: --repeats rounds of (bf16, f16, f16x3), each leg of
a round --samples samplings (9-step DDIM, hipGraph replay, timed from the host around a device synchronise).  A leg's figure is the
median of its round medians as pose-seq/s (B / seconds per sampling); its spread is (max - min) of its round figures.  The expectation
under test: f16 lies within the bf16 leg's own round-to-round spread.  Shapes: BASELINE configs[1] (T = 81, B = 128) and T = 243, B = 64.
Per leg also MPJPE / max-abs of its sampling to the f16x3 leg's.  Writes profiles/f16_mode.json (or --out).

    python experiments/f16_mode.py [--out FILE] [--samples 10] [--repeats 5] [--shapes 81:128 243:64]
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
LEGS = ("bf16", "f16", "f16x3")


def product(T, prec):
    cfg = DenoiserConfig(num_frame=T, embed_dim=512, depth=8)
    net = d3d.HPE_model(d3d.S2S_NAME)(num_frame=T, embed_dim=512, depth=8)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 0).items()})
    net.precision = prec
    diff = d3d.GaussianDiffusion(model=net, timesteps=1000, sampling_timesteps=STEPS, loss_type="l2", clip_denoised=True).eval().cuda()
    return diff._engine(torch.device("cuda", torch.cuda.current_device())), net, diff   # (the engine lives as long as its model)


def samplings_s(eng, x2d, nz, n):
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.ddim_sample(x2d, nz)
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_mode.json"))
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=["81:128", "243:64"], help="T:B")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    assert a.repeats >= 5, "at least five rounds per leg"
    res = {"what": f"{STEPS}-step DDIM sampling, depth 8, embed_dim 512, hipGraph replay; bf16 / f16 / f16x3 engines alternating in one process; "
                   f"pose-seq/s = B / (median of {a.repeats} round medians of {a.samples} samplings); spread = max - min of the leg's round figures",
           "device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count, "cells": []}
    for shape in a.shapes:
        T, B = (int(v) for v in shape.split(":"))
        legs = {p: product(T, p) for p in LEGS}
        inp = synth_inputs(B, T, seed=1)
        x2d, nz = torch.from_numpy(inp["x2d"]).cuda(), torch.from_numpy(inp["noise"]).cuda()
        outs = {}
        for p, (eng, _, _) in legs.items():      # warm-up: eager pass + capture + replays
            eng.set_graph_mode(True)
            for _ in range(3):
                outs[p] = eng.ddim_sample(x2d, nz).clone()
        torch.cuda.synchronize()
        rate = {p: [] for p in LEGS}
        for _ in range(a.repeats):
            for p in LEGS:
                rate[p].append(B / statistics.median(samplings_s(legs[p][0], x2d, nz, a.samples)))
        ref = outs["f16x3"].double()
        cell = {"T": T, "B": B}
        for p in LEGS:
            d = outs[p].double() - ref
            cell[p] = {"pose_seq_per_s": statistics.median(rate[p]), "spread": max(rate[p]) - min(rate[p]), "rounds": rate[p],
                       "mpjpe_to_f16x3": d.norm(dim=-1).mean().item(), "max_abs_to_f16x3": d.abs().max().item(),
                       "finite": bool(torch.isfinite(outs[p]).all())}
        cell["f16_minus_bf16"] = cell["f16"]["pose_seq_per_s"] - cell["bf16"]["pose_seq_per_s"]
        cell["f16_within_bf16_spread"] = bool(abs(cell["f16_minus_bf16"]) <= cell["bf16"]["spread"])
        res["cells"].append(cell)
        print(f"T={T} B={B}: " + "; ".join(f"{p} {cell[p]['pose_seq_per_s']:.1f} pose-seq/s (spread {cell[p]['spread']:.1f}), to f16x3 MPJPE "
                                          f"{cell[p]['mpjpe_to_f16x3']:.3e} max-abs {cell[p]['max_abs_to_f16x3']:.3e}" for p in LEGS)
              + f"; f16 - bf16 {cell['f16_minus_bf16']:+.1f}, within the bf16 spread: {cell['f16_within_bf16_spread']}", flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
        del legs
    print(a.out)


if __name__ == "__main__":
    main()
