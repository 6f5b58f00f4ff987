#!/usr/bin/env python3
"""Heads of 32 columns (embed_dim 256 with the runner's 8 heads) beyond 256 frames: the key-streaming attention kernels of that width
against what the tree before them ran.

  f16x3   "long_temporal_h32" = 1: the folded flow, temporal blocks on kernels_attn_x3_long.hip (width 32), spatial blocks on
          kernels_attn_x3_h32.hip / 0: the plain row-kernel flow with the generic fp32 attention in all 16 blocks
  fp32    "long_temporal_f32_h32" = 1: the temporal blocks on kernels_attn_f32_h32_long.hip / 0: the generic kernel there

(T, B) in {300, 513} x {1, 64}, depth 8, 9 steps, hipGraph replay.  Two engines hold the same weights in ONE process, one with the option
on and one with it off; the legs alternate for REPEATS rounds of N samplings each, every sampling timed from the host around a device
synchronise.  A leg's figure is the median of its round medians, the off leg's spread is max - min of its round medians;
"ahead_in_every_round" says whether the on leg beat the off leg by more than that spread in every alternation (the condition DESIGN.md
states for shipping such an option on by default).  An op-level pass times the new launch alone (through its single-op hook, so the
F16X3 figure includes the plane split and merge around the kernel) against op_attention(..., force_generic=True) at B J = 17 and 64 x 17
groups.  Writes profiles/long_h32.json (or the path given with --out).

    python experiments/long_h32.py [--out FILE] [--samples 5] [--repeats 5] [--frames 300 513] [--batches 1 64] [--precisions f16x3 fp32]
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
KEYS = {"f16x3": "long_temporal_h32", "fp32": "long_temporal_f32_h32"}
OPS = {"f16x3": E.op_attention_long_h32, "fp32": E.op_attention_long_f32_h32}
WIDTH, HEADS, DEPTH, JOINTS = 256, 8, 8, 17


def product(T, sd, prec, on):
    net = d3d.HPE_model(d3d.S2S_NAME)(num_frame=T, embed_dim=WIDTH, depth=DEPTH, num_heads=HEADS)
    net.load_state_dict(sd)
    net.precision = prec
    diff = d3d.GaussianDiffusion(model=net, timesteps=1000, sampling_timesteps=STEPS, loss_type="l2", clip_denoised=True).eval().cuda()
    eng = diff._engine(torch.device("cuda", torch.cuda.current_device()))
    eng.set_option(KEYS[prec], int(on))
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


def op_ms(fn, n=5):
    """Median of n host-timed calls of fn() around a device synchronise, after one warm-up call."""
    fn()
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def op_level(prec, T, B):
    rows = B * T * JOINTS
    qkv = torch.from_numpy((2.0 * hash_uniform(f"oplong{T}", rows * 3 * WIDTH, 21)).astype("float32").reshape(rows, 3 * WIDTH)).cuda()
    new = op_ms(lambda: OPS[prec](qkv, B, T, JOINTS, HEADS))
    old = op_ms(lambda: E.op_attention(qkv, B, T, JOINTS, HEADS, True, precision="fp32", force_generic=True))
    return {"new_ms": new, "generic_ms": old}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_h32.json"))
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="*", default=[300, 513])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
    ap.add_argument("--precisions", nargs="*", default=["f16x3", "fp32"], choices=sorted(KEYS))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    res = {"what": f"{STEPS}-step DDIM sampling, depth {DEPTH}, D = {WIDTH}, {HEADS} heads, hipGraph replay, option 1 (on) vs 0 (off: the launches "
                   f"of the tree before the option), two engines with the same weights alternating in one process; ms are medians of "
                   f"{a.repeats} round medians of {a.samples} samplings; spread = max - min of the off leg's round medians; op: the new "
                   f"launch through its single-op hook against op_attention(force_generic), median of 5 calls",
           "device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count, "cells": []}
    for prec in a.precisions:
        key = KEYS[prec]
        for T in a.frames:
            cfg = DenoiserConfig(num_frame=T, embed_dim=WIDTH, depth=DEPTH, num_heads=HEADS)
            sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 0).items()}
            legs = {"on": product(T, sd, prec, True), "off": product(T, sd, prec, False)}
            for B in a.batches:
                inp = synth_inputs(B, T, seed=1)
                x2d, nz = torch.from_numpy(inp["x2d"]).cuda(), torch.from_numpy(inp["noise"]).cuda()
                outs, ran = {}, {}
                for name, (eng, _, _) in legs.items():      # warm-up: eager pass + capture + replays
                    eng.set_graph_mode(True)
                    for _ in range(2):
                        outs[name] = eng.ddim_sample(x2d, nz).clone()
                    ran[name] = eng.info(key + "_last")
                torch.cuda.synchronize()
                assert ran == {"on": 1, "off": 0}, ran
                med = {"on": [], "off": []}
                for _ in range(a.repeats):
                    for name, (eng, _, _) in legs.items():
                        med[name].append(statistics.median(samplings_ms(eng, x2d, nz, a.samples)))
                spread = max(med["off"]) - min(med["off"])
                cell = {"precision": prec, "key": key, "B": B, "T": T, "on_ms": statistics.median(med["on"]),
                        "off_ms": statistics.median(med["off"]), "off_spread_ms": spread,
                        "on_round_medians_ms": med["on"], "off_round_medians_ms": med["off"],
                        "ahead_in_every_round": bool(all(off - on > spread for on, off in zip(med["on"], med["off"]))),
                        "max_abs_between_modes": (outs["on"] - outs["off"]).abs().max().item(),
                        "op": op_level(prec, T, B)}
                cell["gain_ms"] = cell["off_ms"] - cell["on_ms"]
                res["cells"].append(cell)
                print(f"{prec} T={T} B={B}: on {cell['on_ms']:.3f} ms, off {cell['off_ms']:.3f} ms (spread {spread:.3f}), gain "
                      f"{cell['gain_ms']:+.3f} ms, ahead in every round: {cell['ahead_in_every_round']}; max-abs between modes "
                      f"{cell['max_abs_between_modes']:.3e}; op {cell['op']['generic_ms']:.3f} -> {cell['op']['new_ms']:.3f} ms", flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                json.dump(res, open(a.out, "w"), indent=1)
            del legs
    print(a.out)


if __name__ == "__main__":
    main()
