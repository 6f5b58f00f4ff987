#!/usr/bin/env python3
"""Per-launch times of the attention kernels built on a shared tile header, for A/B runs of two builds of the library
(experiments/attn_x3_tile_ab.sh swaps the .so between processes, the pattern of ab_libs.sh).

    python experiments/attn_x3_tile_ab.py leg TABLE NAME OUT.json      one process = one leg: every shape of TABLE with the library in place
    python experiments/attn_x3_tile_ab.py collect OUT.json LEG.json...   medians, spreads and the criterion per kernel

TABLE: x3_tile (the four F16X3 kernels on csrc/attn_x3_tile.h, D = 512) or f32_tile (the six exact-fp32 MFMA kernels on
csrc/attn_f32_tile.h, head widths 64, 32 and 128 on FP32 engines).

Each shape runs a depth-1 engine of its precision and width with the options that route the block to the kernel in question, eager
launches on one stream with the profiling API (HIP events around every kernel); the figure is the class's event time / launches over
ITERS forwards.  The path is asserted with the engine's *_last info keys.

Criterion (per kernel): median of the new build's legs <= median of the parent's legs + the parent's own spread (max - min of its legs)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ITERS = 10

# name: (T, B, embed_dim, precision, options, latency mode + small tiles, {info key: (mask, value)}, profiling classes read)
TABLES = {
    "x3_tile": {
        "x3p<3> T=81 B=128": (81, 128, 512, "f16x3", {"fused_temporal": 0}, False, {}, ("attn_temporal",)),
        "x3p<1,8> spatial T=243 B=64": (243, 64, 512, "f16x3", {"fused_spatial": 0, "block0_direct": 0}, False, {}, ("attn_spatial",)),
        "base<5,1> T=160 B=8": (160, 8, 512, "f16x3", {"fused_temporal": 0}, False, {}, ("attn_temporal",)),
        "long T=300 B=8": (300, 8, 512, "f16x3", {}, False, {"long_temporal_last": (1, 1)}, ("attn_temporal",)),
        "small T=81 B=1": (81, 1, 512, "f16x3", {"block0_direct": 0}, True, {"small_tiles_last": (~0, 3)}, ("qkv_sattn", "qkv_tattn")),
    },
    "f32_tile": {
        # (the 64-wide resident kernel has no info key of its own: the assertion only says that the streaming kernel did not run; the
        # generic kernel would pass it too, and is ruled out by plan_blocks' rule for D = 64 H, T <= 256 alone)
        "w64 resident<8> T=243 B=16": (243, 16, 512, "fp32", {}, False, {"long_temporal_f32_last": (1, 0)}, ("attn_temporal",)),
        "w64 stream3 T=300 B=8": (300, 8, 512, "fp32", {}, False, {"long_temporal_f32_last": (1, 1)}, ("attn_temporal",)),
        "w32 resident<8> T=243 B=16": (243, 16, 256, "fp32", {}, False, {"attn_f32_h32_last": (2, 2)}, ("attn_temporal",)),
        "w32 stream3 T=300 B=8": (300, 8, 256, "fp32", {}, False, {"long_temporal_f32_h32_last": (1, 1)}, ("attn_temporal",)),
        "w128 resident T=81 B=16": (81, 16, 1024, "fp32", {}, False, {"attn_f32_h128_last": (7, 3)}, ("attn_spatial", "attn_temporal")),
        "w128 stream T=243 B=8": (243, 8, 1024, "fp32", {}, False, {"attn_f32_h128_last": (4, 4)}, ("attn_temporal",)),
    },
}


def leg(table, name, out):
    import torch
    import diff3dhpe_amd as d3d
    from diff3dhpe_amd.spec import DenoiserConfig
    from diff3dhpe_amd.synth import synth_state_dict, synth_inputs
    dev = torch.device("cuda", 0)
    res = {"leg": name, "table": table, "device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "iters": ITERS,
           "us_per_launch": {}}
    for shape, (T, B, E, prec, opts, small, last, classes) in TABLES[table].items():
        cfg = DenoiserConfig(num_frame=T, embed_dim=E, depth=1)
        net = d3d.HPE_model(d3d.S2S_NAME)(num_frame=T, embed_dim=E, depth=1)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 0).items()})
        net.precision = prec
        net.range_check = False
        net.latency_mode = small
        net.latency_small_tiles = small
        diff = d3d.GaussianDiffusion(model=net, timesteps=1000, sampling_timesteps=2, loss_type="l2", clip_denoised=True).eval().cuda()
        eng = net.engine_for(dev)
        for k, v in opts.items():
            eng.set_option(k, v)
        eng.set_option("streams", 1)
        eng.set_graph_mode(False)
        inp = synth_inputs(B, T, seed=1)
        x2d, y = torch.from_numpy(inp["x2d"]).cuda(), torch.from_numpy(inp["noise"]).cuda()
        t = torch.full((B,), 500, dtype=torch.long, device=dev)
        eng.set_profiling(True)
        for _ in range(2):
            eng.denoise(x2d, y, t)
        torch.cuda.synchronize()
        for key, (mask, want) in last.items():
            assert eng.info(key) & mask == want, (shape, key, eng.info(key))
        eng.profile_reset()
        for _ in range(ITERS):
            eng.denoise(x2d, y, t)
        torch.cuda.synchronize()
        p = eng.profile_read()
        eng.set_profiling(False)
        for c in classes:
            assert p[c]["launches"] >= ITERS, (shape, c, p[c])
            key = shape if len(classes) == 1 else f"{shape} {c}"
            res["us_per_launch"][key] = 1e3 * p[c]["ms"] / p[c]["launches"]
            print(f"{name:8s} {key:40s} {res['us_per_launch'][key]:9.2f} us", flush=True)
        del eng, diff, net
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def collect(out, files):
    legs = [json.load(open(f)) for f in files]
    res = {"what": f"us per launch (HIP events, eager, one stream, depth-1 engines) of the attention kernels of table {legs[0]['table']} "
                   "(experiments/attn_x3_tile_ab.py); legs alternate parent / new in one session on one device, one process per leg; "
                   "criterion: new median <= parent median + parent spread (max - min over its legs)",
           "device": legs[0]["device"], "rocm": legs[0]["rocm"], "iters_per_leg": legs[0]["iters"], "order": [l["leg"] for l in legs], "kernels": {}}
    for key in legs[0]["us_per_launch"]:
        runs = {n: [l["us_per_launch"][key] for l in legs if l["leg"] == n] for n in ("parent", "new")}
        pm, nm = statistics.median(runs["parent"]), statistics.median(runs["new"])
        spread = max(runs["parent"]) - min(runs["parent"])
        res["kernels"][key] = {"parent_us": runs["parent"], "new_us": runs["new"], "parent_median_us": pm, "new_median_us": nm,
                               "parent_spread_us": spread, "criterion_met": bool(nm <= pm + spread)}
        print(f"{key:40s} parent {pm:9.2f} us (spread {spread:6.2f})  new {nm:9.2f} us  {'ok' if nm <= pm + spread else 'MISSED'}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if sys.argv[1] == "leg":
        leg(sys.argv[2], sys.argv[3], sys.argv[4])
    else:
        collect(sys.argv[2], sys.argv[3:])
