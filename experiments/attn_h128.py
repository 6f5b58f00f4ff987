#!/usr/bin/env python3
"""Heads of 128 columns (embed_dim 1024 with the runner's 8 heads): the F16X3 attention kernels of that width against the plain flow.

  "attn_h128" = 1: the folded flow, spatial blocks and temporal blocks of up to 128 frames on kernels_attn_x3_h128.hip, temporal blocks
                   of more than 128 frames on kernels_attn_x3_long.hip (width 128)
              / 0: the plain row-kernel flow with the generic fp32 attention in all 16 blocks

The tree before the option refuses this width, so it cannot be a leg; the off leg stands for what a bare admission would have run.

(T, B) in {27, 243, 300} x {1, 64}, depth 8, 9 steps, hipGraph replay.  Two engines hold the same weights in ONE process, one with the
option on and one with it off; the legs alternate for REPEATS rounds of N samplings each, every sampling timed from the host around a
device synchronise.  A leg's figure is the median of its round medians, the off leg's spread is max - min of its round medians;
"ahead_in_every_round" says whether the on leg beat the off leg by more than that spread in every alternation (the condition DESIGN.md
states for shipping such an option on by default).  An op-level pass times the two launches alone (through their single-op hooks, so the
figures include the plane split and merge around the kernel) against op_attention(..., force_generic=True): the temporal kernel the
engine takes at that T on B x 17 groups of T frames, the resident kernel on B x T spatial groups of 17 joints.  Writes
profiles/attn_h128.json (or the path given with --out).

    python experiments/attn_h128.py [--out FILE] [--samples 5] [--repeats 5] [--frames 27 243 300] [--batches 1 64]
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
KEY = "attn_h128"
WIDTH, HEADS, DEPTH, JOINTS = 1024, 8, 8, 17


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


def op_level(T, B):
    rows = B * T * JOINTS
    qkv = torch.from_numpy((2.0 * hash_uniform(f"op128_{T}", rows * 3 * WIDTH, 21)).astype("float32").reshape(rows, 3 * WIDTH)).cuda()
    if T <= 128:
        tp = op_ms(lambda: E.op_attention_h128(qkv, B, T, JOINTS, HEADS, True))
    else:
        tp = op_ms(lambda: E.op_attention_long_h128(qkv, B, T, JOINTS, HEADS))
    tp_old = op_ms(lambda: E.op_attention(qkv, B, T, JOINTS, HEADS, True, precision="fp32", force_generic=True))
    sp = op_ms(lambda: E.op_attention_h128(qkv, B, T, JOINTS, HEADS, False))
    sp_old = op_ms(lambda: E.op_attention(qkv, B, T, JOINTS, HEADS, False, precision="fp32", force_generic=True))
    return {"temporal_kernel": "resident" if T <= 128 else "streaming", "temporal_new_ms": tp, "temporal_generic_ms": tp_old,
            "spatial_new_ms": sp, "spatial_generic_ms": sp_old}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_h128.json"))
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="*", default=[27, 243, 300])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    res = {"what": f"{STEPS}-step DDIM sampling, depth {DEPTH}, D = {WIDTH}, {HEADS} heads, hipGraph replay, F16X3, option 1 (on) vs 0 (off: the plain flow "
                   f"with the generic attention kernel), two engines with the same weights alternating in one process; ms are medians of "
                   f"{a.repeats} round medians of {a.samples} samplings; spread = max - min of the off leg's round medians; op: the new "
                   f"launches through their single-op hooks against op_attention(force_generic), median of 5 calls",
           "device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count, "cells": []}
    for T in a.frames:
        cfg = DenoiserConfig(num_frame=T, embed_dim=WIDTH, depth=DEPTH, num_heads=HEADS)
        sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 0).items()}
        legs = {"on": product(T, sd, True), "off": product(T, sd, False)}
        want = 3 if T <= 128 else 5
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
            assert ran == {"on": want, "off": 0}, ran
            med = {"on": [], "off": []}
            for rnd in range(a.repeats):
                for name, (eng, _, _) in legs.items():
                    med[name].append(statistics.median(samplings_ms(eng, x2d, nz, a.samples)))
                print(f"  T={T} B={B} round {rnd}: on {med['on'][-1]:.3f} ms, off {med['off'][-1]:.3f} ms", flush=True)
            spread = max(med["off"]) - min(med["off"])
            cell = {"key": KEY, "B": B, "T": T, "attn_h128_last": want, "on_ms": statistics.median(med["on"]),
                    "off_ms": statistics.median(med["off"]), "off_spread_ms": spread,
                    "on_round_medians_ms": med["on"], "off_round_medians_ms": med["off"],
                    "ahead_in_every_round": bool(all(off - on > spread for on, off in zip(med["on"], med["off"]))),
                    "max_abs_between_modes": (outs["on"] - outs["off"]).abs().max().item(),
                    "op": op_level(T, B)}
            cell["gain_ms"] = cell["off_ms"] - cell["on_ms"]
            res["cells"].append(cell)
            op = cell["op"]
            print(f"T={T} B={B}: on {cell['on_ms']:.3f} ms, off {cell['off_ms']:.3f} ms (spread {spread:.3f}), gain "
                  f"{cell['gain_ms']:+.3f} ms, ahead in every round: {cell['ahead_in_every_round']}; max-abs between modes "
                  f"{cell['max_abs_between_modes']:.3e}; op temporal ({op['temporal_kernel']}) {op['temporal_generic_ms']:.3f} -> "
                  f"{op['temporal_new_ms']:.3f} ms, spatial {op['spatial_generic_ms']:.3f} -> {op['spatial_new_ms']:.3f} ms", flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(res, open(a.out, "w"), indent=1)
        del legs
    print(a.out)


if __name__ == "__main__":
    main()
