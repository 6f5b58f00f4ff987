#!/usr/bin/env python3
"""Heads of 16 columns (embed_dim 128 with the runner's 8 heads): the attention kernels of that width against the flow such an engine ran
before them.

  "attn_h16" = 1 (F16X3): the folded flow, spatial blocks and temporal blocks of up to 256 frames on kernels_attn_x3_h16.hip, longer
                  temporal blocks on kernels_attn_x3_long.hip at that width
             / 0: the plain row-kernel flow with the generic fp32 attention in all 16 blocks
  "attn_f32_h16" = 1 (FP32, --fp32): every block's attention on kernels_attn_f32_hx.hip at DH = 16 (resident up to 256 tokens, streaming
                  beyond) / 0: the generic one-thread-per-row kernel

The off leg launches exactly the kernels of the tree before the options: it is the reference leg.

D = 128; (T, B) in {27, 243} x {1, 64} and (300, 1); depth 8, 9 steps, hipGraph replay.  Two engines hold the same weights in ONE process,
one with the option on and one with it off; the legs alternate for REPEATS rounds of N samplings each, every sampling timed from the host
around a device synchronise.  A leg's figure is the median of its round medians, the off leg's spread is max - min of its round medians;
"ahead_in_every_round" says whether the on leg beat the off leg by more than that spread in every alternation (the condition DESIGN.md
states for shipping such an option on by default).  Writes profiles/attn_h16.json (or the path given with --out; a run with --fp32 adds
its cells to the file's F16X3 cells and the other way round) and prints the rows of the DESIGN.md section 5 table.

    python experiments/attn_h16.py [--fp32] [--out FILE] [--samples 5] [--repeats 5] [--cells 27x1 27x64 243x1 243x64 300x1]
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
D, HEADS, DEPTH = 128, 8, 8
RESIDENT = 256     # the longest window whose temporal blocks stay resident


def product(T, sd, key, prec, on):
    net = d3d.HPE_model(d3d.S2S_NAME)(num_frame=T, embed_dim=D, depth=DEPTH, num_heads=HEADS)
    net.load_state_dict(sd)
    net.precision = prec
    diff = d3d.GaussianDiffusion(model=net, timesteps=1000, sampling_timesteps=STEPS, loss_type="l2", clip_denoised=True).eval().cuda()
    eng = diff._engine(torch.device("cuda", torch.cuda.current_device()))
    eng.set_option(key, int(on))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_h16.json"))
    ap.add_argument("--fp32", action="store_true", help='the FP32 engines and "attn_f32_h16" instead of F16X3 and "attn_h16"')
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cells", nargs="*", default=["27x1", "27x64", "243x1", "243x64", "300x1"], help="TxB")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    key, prec = ("attn_f32_h16", "fp32") if a.fp32 else ("attn_h16", "f16x3")
    cells = [tuple(int(v) for v in c.split("x")) for c in a.cells]
    res = {"what": f"{STEPS}-step DDIM sampling, embed_dim {D}, depth {DEPTH}, {HEADS} heads, hipGraph replay, option 1 (on) vs 0 (off: the "
                   f"generic attention kernel in every block, the kernels of the tree before the option), two engines with the same weights "
                   f"alternating in one process; ms are medians of round medians of samplings timed from the host; spread = max - min of "
                   f"the off leg's round medians",
           "cells": []}
    if os.path.exists(a.out):      # keep the other precision's cells
        old = json.load(open(a.out))
        res["cells"] = [c for c in old.get("cells", []) if c.get("key") != key]
    res["device"] = torch.cuda.get_device_name(0)
    res["cus"] = torch.cuda.get_device_properties(0).multi_processor_count
    mine = []
    for T in sorted({t for t, _ in cells}):
        cfg = DenoiserConfig(num_frame=T, embed_dim=D, depth=DEPTH, num_heads=HEADS)
        sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 0).items()}
        legs = {"on": product(T, sd, key, prec, True), "off": product(T, sd, key, prec, False)}
        want = 3 if T <= RESIDENT else 5
        for B in [b for t, b in cells if t == T]:
            inp = synth_inputs(B, T, seed=1)
            x2d, nz = torch.from_numpy(inp["x2d"]).cuda(), torch.from_numpy(inp["noise"]).cuda()
            outs, ran = {}, {}
            for name, (eng, _, _) in legs.items():      # warm-up: eager pass + capture + replays
                eng.set_graph_mode(True)
                for _ in range(2):
                    outs[name] = eng.ddim_sample(x2d, nz).clone()
                ran[name] = eng.info(key + "_last")
            torch.cuda.synchronize()
            assert ran == {"on": want, "off": 0}, ran
            assert all(torch.isfinite(o).all() for o in outs.values())
            med = {"on": [], "off": []}
            for rnd in range(a.repeats):
                for name, (eng, _, _) in legs.items():
                    med[name].append(statistics.median(samplings_ms(eng, x2d, nz, a.samples)))
                print(f"  {prec} T={T} B={B} round {rnd}: on {med['on'][-1]:.3f} ms, off {med['off'][-1]:.3f} ms", flush=True)
            spread = max(med["off"]) - min(med["off"])
            cell = {"key": key, "precision": prec, "D": D, "B": B, "T": T, key + "_last": want, "samples": a.samples, "repeats": a.repeats,
                    "on_ms": statistics.median(med["on"]), "off_ms": statistics.median(med["off"]), "off_spread_ms": spread,
                    "on_round_medians_ms": med["on"], "off_round_medians_ms": med["off"],
                    "ahead_in_every_round": bool(all(off - on > spread for on, off in zip(med["on"], med["off"]))),
                    "max_abs_between_modes": (outs["on"] - outs["off"]).abs().max().item()}
            cell["gain_ms"] = cell["off_ms"] - cell["on_ms"]
            mine.append(cell)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump({**res, "cells": res["cells"] + mine}, open(a.out, "w"), indent=1)
        del legs
    print(f"| precision | T | B | {key}_last | off ms | on ms | off spread ms | ahead in every round | max-abs between modes |")
    print("|---|---|---|---|---|---|---|---|---|")
    for c in mine:
        print(f"| {c['precision']} | {c['T']} | {c['B']} | {c[key + '_last']} | {c['off_ms']:.1f} | {c['on_ms']:.1f} | {c['off_spread_ms']:.2f} | "
              f"{'yes' if c['ahead_in_every_round'] else 'no'} | {c['max_abs_between_modes']:.1e} |")
    print(a.out)


if __name__ == "__main__":
    main()
