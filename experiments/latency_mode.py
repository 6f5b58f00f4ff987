#!/usr/bin/env python3
"""Default path against "latency_mode" (include/d3d.h) for small calls: B in {1, 2, 4} x T in {27, 81, 243}, 9 steps, F16X3, hipGraph replay.

Both legs run in ONE process, interleaved: REPEATS rounds of (default: N samplings, latency mode: N samplings), each sampling timed from
the host around a device synchronise; a leg's figure is the median of its round medians, the default leg's spread is max - min of its round
medians.  A profiling pass (eager launches, one stream, HIP events around every kernel) then gives the per-launch time of fc2 and of the
row kernel in both modes.  Writes profiles/latency_mode.json (or the path given with --out).

    python experiments/latency_mode.py [--out FILE] [--samples 20] [--repeats 5]

--proj-fc1: the table behind the proj / fc1 rules (d3d_kernels.h proj_splitk_choose / fc1_splitk_choose), written to
profiles/latency_mode_proj_fc1.json.  Two legs with the mode ON, interleaved the same way: "base" -- "proj_split" = "fc1_split" = 0,
launch for launch what the tree before those rules ran with the mode on -- and "rule" -- both keys at -1.  With --parent DIR (a built
checkout of that earlier tree) the base leg is run from DIR in a child process per round instead, alternating with this tree's.  Per
cell: both medians, the base leg's spread (max - min of its round medians), and one-stream per-launch times of proj and fc1 with S forced
to 0, 2 and 4 (profiling API; the split GEMM under its class, the reduce among the row kernels).

--small-tiles: the table behind the "small_tiles" rule (engine.hip plan_blocks), written to profiles/latency_small_tiles.json.  Two
engines with the same weights, the mode ON in both, "small_tiles" 1 ("on") / 0 ("off": launch for launch latency mode without the key),
alternating for --repeats rounds of --samples samplings.  Per cell: both medians, the off leg's spread, whether the on leg leads in every
round, what "small_tiles_last" reported, and one-stream per-launch times of the two fused qkv + attention classes in both legs.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("D3D_TREE") or ROOT)   # (D3D_TREE: the --parent leg imports the package of another checkout)
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


def per_launch_forced(eng, x2d, nz):
    """us per launch of proj / fc1 (split GEMM or present kernel) and of all row kernels, with both S forced to 0, 2, 4 in turn."""
    out = {}
    eng.set_graph_mode(False)
    for S in (0, 2, 4):
        eng.set_option("proj_split", S)
        eng.set_option("fc1_split", S)
        eng.set_profiling(True)
        eng.ddim_sample(x2d, nz)
        torch.cuda.synchronize()
        eng.profile_reset()
        eng.ddim_sample(x2d, nz)
        torch.cuda.synchronize()
        p = eng.profile_read()
        eng.set_profiling(False)
        us = lambda c: (1e3 * p[c]["ms"] / p[c]["launches"]) if p[c]["launches"] else None
        out[f"S{S}"] = {"ran": [eng.info("proj_split_last"), eng.info("fc1_split_last")], "proj_us": us("linear_proj"), "fc1_us": us("linear_fc1"),
                        "row_kernel_us": us("layernorm"), "row_kernel_launches": p["layernorm"]["launches"],
                        "proj_launches": p["linear_proj"]["launches"]}
    eng.set_option("proj_split", -1)
    eng.set_option("fc1_split", -1)
    eng.set_graph_mode(True)
    return out


def child_round(T, B, samples):
    """One round's median of this tree with the mode on (the --parent leg runs this function from the parent checkout)."""
    eng, net, diff = product(T, True)
    inp = synth_inputs(B, T, seed=1)
    x2d, nz = torch.from_numpy(inp["x2d"]).cuda(), torch.from_numpy(inp["noise"]).cuda()
    eng.set_graph_mode(True)
    for _ in range(3):
        eng.ddim_sample(x2d, nz)
    print(json.dumps({"median_ms": statistics.median(samplings_ms(eng, x2d, nz, samples))}))


def proj_fc1_table(a):
    import subprocess
    out = a.out if a.out_given else os.path.join(ROOT, "profiles", "latency_mode_proj_fc1.json")
    res = {"what": f"{STEPS}-step DDIM sampling, F16X3, hipGraph replay, latency_mode ON in both legs: base = proj_split / fc1_split 0 (the launches "
                   f"of the tree before the proj / fc1 rules" + (", run from a checkout of it" if a.parent else "") + "), rule = both -1; ms are medians of "
                   f"{a.repeats} round medians of {a.samples} samplings; spread = max - min of the base leg's round medians; per_launch: one stream, "
                   "eager, HIP events, both S forced",
           "device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count, "cells": []}
    for T in a.frames:
        base, rule = product(T, True), product(T, True)
        base[0].set_option("proj_split", 0)
        base[0].set_option("fc1_split", 0)
        legs = {"base": base, "rule": rule}
        for B in a.batches:
            inp = synth_inputs(B, T, seed=1)
            x2d, nz = torch.from_numpy(inp["x2d"]).cuda(), torch.from_numpy(inp["noise"]).cuda()
            outs = {}
            for name, (eng, _, _) in legs.items():
                eng.set_graph_mode(True)
                for _ in range(3):
                    outs[name] = eng.ddim_sample(x2d, nz)
            ran = [rule[0].info("proj_split_last"), rule[0].info("fc1_split_last"), rule[0].info("fc2_split_last")]
            torch.cuda.synchronize()
            med = {"base": [], "rule": []}
            for _ in range(a.repeats):
                for name, (eng, _, _) in legs.items():
                    if name == "base" and a.parent:
                        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(T), str(B), "--samples", str(a.samples)],
                                           check=True, capture_output=True, text=True, env=dict(os.environ, D3D_TREE=os.path.abspath(a.parent)))
                        med[name].append(json.loads(r.stdout.strip().splitlines()[-1])["median_ms"])
                    else:
                        med[name].append(statistics.median(samplings_ms(eng, x2d, nz, a.samples)))
            cell = {"B": B, "T": T, "S_proj_fc1_fc2": ran, "base_ms": statistics.median(med["base"]), "rule_ms": statistics.median(med["rule"]),
                    "base_spread_ms": max(med["base"]) - min(med["base"]), "base_round_medians_ms": med["base"],
                    "rule_round_medians_ms": med["rule"], "max_abs_between_legs": (outs["base"] - outs["rule"]).abs().max().item(),
                    "per_launch": per_launch_forced(rule[0], x2d, nz)}
            cell["gain_ms"] = cell["base_ms"] - cell["rule_ms"]
            cell["ahead_by_more_than_spread"] = bool(cell["gain_ms"] > cell["base_spread_ms"])
            res["cells"].append(cell)
            pl = cell["per_launch"]
            print(f"T={T:3d} B={B} S(proj, fc1, fc2)={ran}: base {cell['base_ms']:.3f} ms (spread {cell['base_spread_ms']:.3f}), rule "
                  f"{cell['rule_ms']:.3f} ms, gain {cell['gain_ms']:+.3f}; per launch S=0/2/4: proj "
                  + "/".join(f"{pl[k]['proj_us']:.1f}" for k in ("S0", "S2", "S4")) + " us, fc1 "
                  + "/".join(f"{pl[k]['fc1_us']:.1f}" for k in ("S0", "S2", "S4")) + " us, row kernels "
                  + "/".join(f"{pl[k]['row_kernel_us']:.1f}x{pl[k]['row_kernel_launches']}" for k in ("S0", "S2", "S4")), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            json.dump(res, open(out, "w"), indent=1)
        del legs, base, rule
    print(out)


def per_launch_qkv_attn(eng, x2d, nz):
    """us per launch of the fused qkv + attention classes (spatial: block 0's direct launches included) from the profiling API."""
    eng.set_graph_mode(False)
    eng.set_profiling(True)
    eng.ddim_sample(x2d, nz)
    torch.cuda.synchronize()
    eng.profile_reset()
    eng.ddim_sample(x2d, nz)
    torch.cuda.synchronize()
    p = eng.profile_read()
    ran = eng.info("small_tiles_last")   # (profiling runs the whole batch on one stream: for B >= 2 not the replay's half-batches)
    eng.set_profiling(False)
    eng.set_graph_mode(True)
    us = lambda c: (1e3 * p[c]["ms"] / p[c]["launches"]) if p[c]["launches"] else None
    return {"small_tiles_profiled": ran, "qkv_sattn_us": us("qkv_sattn"), "qkv_sattn_launches": p["qkv_sattn"]["launches"],
            "qkv_tattn_us": us("qkv_tattn"), "qkv_tattn_launches": p["qkv_tattn"]["launches"]}


def small_tiles_table(a):
    out = a.out if a.out_given else os.path.join(ROOT, "profiles", "latency_small_tiles.json")
    res = {"what": f"{STEPS}-step DDIM sampling, depth 8, F16X3, hipGraph replay, latency_mode ON in both legs: off = small_tiles 0 (launch for "
                   f"launch latency mode without the key), on = small_tiles 1; alternating in one process; ms are medians of {a.repeats} round "
                   f"medians of {a.samples} samplings; spread = max - min of the off leg's round medians; per_launch: one stream, eager, HIP "
                   "events, the whole batch in one forward (a replay of B >= 2 runs two half-batches on two streams)",
           "device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count, "cells": []}
    for T in a.frames:
        legs = {"off": product(T, True), "on": product(T, True)}
        legs["on"][0].set_option("small_tiles", 1)
        for B in a.batches:
            inp = synth_inputs(B, T, seed=1)
            x2d, nz = torch.from_numpy(inp["x2d"]).cuda(), torch.from_numpy(inp["noise"]).cuda()
            outs, ran = {}, {}
            for name, (eng, _, _) in legs.items():      # warm-up: eager pass + capture + replays
                eng.set_graph_mode(True)
                for _ in range(3):
                    outs[name] = eng.ddim_sample(x2d, nz)
                ran[name] = eng.info("small_tiles_last")
            torch.cuda.synchronize()
            med = {"off": [], "on": []}
            for _ in range(a.repeats):
                for name in ("on", "off"):
                    med[name].append(statistics.median(samplings_ms(legs[name][0], x2d, nz, a.samples)))
            cell = {"B": B, "T": T, "small_tiles_last": ran["on"], "small_tiles_last_off": ran["off"],
                    "off_ms": statistics.median(med["off"]), "on_ms": statistics.median(med["on"]),
                    "off_spread_ms": max(med["off"]) - min(med["off"]), "off_round_medians_ms": med["off"], "on_round_medians_ms": med["on"],
                    "on_leads_in_every_round": all(x < y for x, y in zip(med["on"], med["off"])),
                    "max_abs_between_legs": (outs["off"] - outs["on"]).abs().max().item(),
                    "per_launch": {name: per_launch_qkv_attn(eng, x2d, nz) for name, (eng, _, _) in legs.items()}}
            cell["gain_ms"] = cell["off_ms"] - cell["on_ms"]
            cell["ahead_by_more_than_spread"] = bool(cell["gain_ms"] > cell["off_spread_ms"])
            res["cells"].append(cell)
            pl = cell["per_launch"]
            print(f"T={T:3d} B={B} small_tiles_last={ran['on']}: off {cell['off_ms']:.3f} ms (spread {cell['off_spread_ms']:.3f}), on "
                  f"{cell['on_ms']:.3f} ms, gain {cell['gain_ms']:+.3f}, on leads in every round: {cell['on_leads_in_every_round']}; per launch "
                  f"off -> on: spatial {pl['off']['qkv_sattn_us']:.1f} -> {pl['on']['qkv_sattn_us']:.1f} us, temporal "
                  f"{pl['off']['qkv_tattn_us']:.1f} -> {pl['on']['qkv_tattn_us']:.1f} us (profiled small_tiles_last {pl['on']['small_tiles_profiled']})",
                  flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            json.dump(res, open(out, "w"), indent=1)
        del legs
    print(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proj-fc1", action="store_true", help="the proj / fc1 table (profiles/latency_mode_proj_fc1.json)")
    ap.add_argument("--small-tiles", action="store_true", help='the "small_tiles" table (profiles/latency_small_tiles.json)')
    ap.add_argument("--parent", default=None, help="with --proj-fc1: a built checkout of the tree before the proj / fc1 rules")
    ap.add_argument("--child", nargs=2, type=int, default=None, metavar=("T", "B"), help="internal: one round of the mode-on leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latency_mode.json"))
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="*", default=[27, 81, 243])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 2, 4])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    a.out_given = any(x == "--out" or x.startswith("--out=") for x in sys.argv[1:])
    if a.child:
        return child_round(a.child[0], a.child[1], a.samples)
    if a.proj_fc1:
        return proj_fc1_table(a)
    if a.small_tiles:
        return small_tiles_table(a)
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
