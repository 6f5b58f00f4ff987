#!/usr/bin/env python3
"""Heads of 32 and 16 columns (embed_dim 256 / 128 with the runner's 8 heads) on an F16X3 engine: the qkv GEMM and the attention of a block
as ONE kernel ("fused_narrow" = 1, include/d3d.h: the narrow forms of kernels_qkv_attn_x3_small.hip) against the two launches with the
q / k / v planes in HBM ("fused_narrow" = 0).  (T, B) in {27, 81, 243} x {1, 64}, depth 8, 9 steps, hipGraph replay.

Two engines hold the same weights in ONE process, one with the key on and one with it off; the legs alternate for REPEATS rounds of N
samplings each, every sampling timed from the host around a device synchronise.  A leg's figure is the median of its round medians, the
off leg's spread is max - min of its round medians; "ahead_in_every_round" says whether the on leg beat the off leg by more than that
spread in every alternation.  A profiling pass (eager launches, one stream, HIP events around every kernel) gives the per-launch times of
the spatial and the temporal step: qkv GEMM + attention with the key off, the fused kernel with it on.

The baseline is a build of the PARENT commit: run this script once more with --package-root pointing at a checkout of it and --legs
plain (an engine whose options are not touched: the parent has no such key), in the same session on the same device, and give its output
to the main run with --parent-json; each cell then carries "parent_ms" beside the off leg, which is launch for launch the parent's flow.

    python experiments/fused_narrow.py --package-root ../parent --legs plain --out /tmp/parent.json
    python experiments/fused_narrow.py --parent-json /tmp/parent.json [--out profiles/fused_narrow.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 9
KEY = "fused_narrow"
HEADS, DEPTH = 8, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=HERE, help="the checkout whose diff3dhpe_amd is measured")
    ap.add_argument("--legs", nargs="*", default=["on", "off"], choices=["on", "off", "plain"])
    ap.add_argument("--parent-json", default=None, help="the output of a --legs plain run on the parent commit")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", KEY + ".json"))
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--widths", type=int, nargs="*", default=[256, 128])
    ap.add_argument("--frames", type=int, nargs="*", default=[27, 81, 243])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    import diff3dhpe_amd as d3d
    from diff3dhpe_amd.spec import DenoiserConfig
    from diff3dhpe_amd.synth import synth_state_dict, synth_inputs
    assert torch.cuda.is_available(), "needs the GPU"
    assert os.path.abspath(d3d.__file__).startswith(os.path.abspath(a.package_root)), d3d.__file__

    def product(T, D, sd, leg):
        net = d3d.HPE_model(d3d.S2S_NAME)(num_frame=T, embed_dim=D, depth=DEPTH, num_heads=HEADS)
        net.load_state_dict(sd)
        net.precision = "f16x3"
        diff = d3d.GaussianDiffusion(model=net, timesteps=1000, sampling_timesteps=STEPS, loss_type="l2", clip_denoised=True).eval().cuda()
        eng = diff._engine(torch.device("cuda", torch.cuda.current_device()))
        if leg != "plain":
            eng.set_option(KEY, int(leg == "on"))
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
        """us per launch from the profiling API (one stream, eager): the qkv GEMM, the two attention kernels, the two fused classes."""
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
        out = {}
        for c in ("linear_qkv", "attn_spatial", "attn_temporal", "qkv_sattn", "qkv_tattn"):
            n = p.get(c, {}).get("launches")
            out[c + "_us"], out[c + "_launches"] = (1e3 * p[c]["ms"] / n if n else None), n
        out["total_ms"] = sum(v["ms"] for k, v in p.items() if not k.startswith("linear_"))
        return out

    parent = {}
    if a.parent_json:
        for c in json.load(open(a.parent_json))["cells"]:
            parent[(c["D"], c["T"], c["B"])] = c
    res = {"what": f"{STEPS}-step DDIM sampling, F16X3, depth {DEPTH}, {HEADS} heads, hipGraph replay; legs {a.legs}: on / off = {KEY} 1 / 0, two "
                   f"engines with the same weights alternating in one process; plain = an engine whose options are untouched; ms are medians "
                   f"of {a.repeats} round medians of {a.samples} samplings; spread = max - min of a leg's round medians; parent_ms: the "
                   f"plain leg of a build of the parent commit, run in the same session on the same device (not alternating with these legs)",
           "version": d3d._lib.lib().d3d_version(),
           "device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count, "cells": []}
    for D in a.widths:
        for T in a.frames:
            cfg = DenoiserConfig(num_frame=T, embed_dim=D, depth=DEPTH, num_heads=HEADS)
            sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 0).items()}
            legs = {leg: product(T, D, sd, leg) for leg in a.legs}
            for B in a.batches:
                inp = synth_inputs(B, T, seed=1)
                x2d, nz = torch.from_numpy(inp["x2d"]).cuda(), torch.from_numpy(inp["noise"]).cuda()
                outs, ran = {}, {}
                for name, (eng, _, _) in legs.items():      # warm-up: eager pass + capture + replays
                    eng.set_graph_mode(True)
                    for _ in range(2):
                        outs[name] = eng.ddim_sample(x2d, nz).clone()
                    ran[name] = eng.info(KEY + "_last") if name != "plain" else None
                torch.cuda.synchronize()
                med = {name: [] for name in legs}
                for _ in range(a.repeats):
                    for name, (eng, _, _) in legs.items():
                        med[name].append(statistics.median(samplings_ms(eng, x2d, nz, a.samples)))
                cell = {"D": D, "T": T, "B": B, "last": ran}
                for name in legs:
                    cell[name + "_ms"] = statistics.median(med[name])
                    cell[name + "_spread_ms"] = max(med[name]) - min(med[name])
                    cell[name + "_round_medians_ms"] = med[name]
                cell["per_launch"] = {name: per_launch(eng, x2d, nz) for name, (eng, _, _) in legs.items()}
                line = f"D={D} T={T} B={B}: " + ", ".join(f"{n} {cell[n + '_ms']:.3f} ms (spread {cell[n + '_spread_ms']:.3f})" for n in legs)
                if "on" in legs and "off" in legs:
                    spread = cell["off_spread_ms"]
                    cell["gain_ms"] = cell["off_ms"] - cell["on_ms"]
                    cell["ahead_in_every_round"] = bool(all(off - on > spread for on, off in zip(med["on"], med["off"])))
                    cell["bit_identical"] = bool(torch.equal(outs["on"], outs["off"]))
                    pl = cell["per_launch"]
                    f = lambda v: "-" if v is None else f"{v:.1f}"
                    line += (f", gain {cell['gain_ms']:+.3f} ms, ahead in every round: {cell['ahead_in_every_round']}, bit-identical: "
                             f"{cell['bit_identical']}, last {ran['on']}; per launch us: qkv GEMM {f(pl['off']['linear_qkv_us'])} + attention "
                             f"{f(pl['off']['attn_spatial_us'])} / {f(pl['off']['attn_temporal_us'])} -> fused {f(pl['on']['qkv_sattn_us'])} / "
                             f"{f(pl['on']['qkv_tattn_us'])} (on leg's remaining attention {f(pl['on']['attn_temporal_us'])})")
                if (D, T, B) in parent:
                    cell["parent_ms"] = parent[(D, T, B)]["plain_ms"]
                    cell["parent_spread_ms"] = parent[(D, T, B)]["plain_spread_ms"]
                    line += f"; parent build {cell['parent_ms']:.3f} ms (spread {cell['parent_spread_ms']:.3f})"
                res["cells"].append(cell)
                print(line, flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                json.dump(res, open(a.out, "w"), indent=1)
            del legs
    print(a.out)


if __name__ == "__main__":
    main()
