#!/usr/bin/env python3
"""The key-streaming F16X3 attention kernels (kernels_attn_x3_long.hip) of two builds of the library against each other: the library
of the tree ("new") and one built from another commit to a second path ("parent").  For a refactor of those kernels: the parent is the
yardstick and its own spread is the margin.

  op        the three single-op hooks (op_attention_long, op_attention_long_h32, op_attention_long_h128: plane split, kernel, merge)
            at (T, B J) = (300, 17), (513, 17), (300, 64 x 17); D = 512 / 256 / 1024, 8 heads
  sampling  one 9-step depth-8 DDIM sampling per width at T = 300, B = 1 and B = 64, hipGraph replay, timed as experiments/long_h32.py
            does (from the host around a device synchronise)

One process per leg and round (a process loads ONE library), the legs alternating parent, new, parent, new, ...; a round's figure per cell
is the median of its samples, a leg's the median of its round medians, the spread max - min of the PARENT leg's round medians.  The
condition per cell: the new median is not slower than the parent's by more than that spread.  Writes
profiles/attn_x3_stream_refactor.json (or --out).  A leg that fails ends the run: nothing more is started on the device.

    python experiments/attn_x3_stream_ab.py --parent-lib PATH [--rounds 5] [--samples 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WIDTHS = {64: 512, 32: 256, 128: 1024}       # head width -> embed_dim at 8 heads
HEADS, DEPTH, JOINTS, STEPS = 8, 8, 17, 9
OP_SHAPES = [(300, 1), (513, 1), (300, 64)]  # (T, B) at 17 joints
SAMPLING = [(300, 1), (300, 64)]


def leg(lib_path, samples):
    """One leg in this process: every cell once, {cell name: median ms of `samples`}."""
    from diff3dhpe_amd import _lib
    _lib.LIB_PATH = lib_path                 # before the first use: the process binds this library and no other
    import torch
    import diff3dhpe_amd as d3d
    from diff3dhpe_amd import engine as E
    from diff3dhpe_amd.spec import DenoiserConfig
    from diff3dhpe_amd.synth import synth_state_dict, synth_inputs, hash_uniform
    assert _lib.lib()._name == lib_path
    ops = {64: E.op_attention_long, 32: E.op_attention_long_h32, 128: E.op_attention_long_h128}

    def timed(fn, n, warm):
        for _ in range(warm):
            fn()
        out = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out)

    res = {}
    for dh, D in WIDTHS.items():
        for T, B in OP_SHAPES:
            rows = B * T * JOINTS
            qkv = torch.from_numpy((2.0 * hash_uniform(f"abq{T}", rows * 3 * D, 21)).astype("float32").reshape(rows, 3 * D)).cuda()
            res[f"op_h{dh}_T{T}_BJ{B * JOINTS}"] = timed(lambda: ops[dh](qkv, B, T, JOINTS, HEADS), samples, 2)
            del qkv
        T = SAMPLING[0][0]
        cfg = DenoiserConfig(num_frame=T, embed_dim=D, depth=DEPTH, num_heads=HEADS)
        net = d3d.HPE_model(d3d.S2S_NAME)(num_frame=T, embed_dim=D, depth=DEPTH, num_heads=HEADS)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 0).items()})
        net.precision = "f16x3"
        diff = d3d.GaussianDiffusion(model=net, timesteps=1000, sampling_timesteps=STEPS, loss_type="l2", clip_denoised=True).eval().cuda()
        eng = diff._engine(torch.device("cuda", torch.cuda.current_device()))
        eng.set_graph_mode(True)
        for T, B in SAMPLING:
            inp = synth_inputs(B, T, seed=1)
            x2d, nz = torch.from_numpy(inp["x2d"]).cuda(), torch.from_numpy(inp["noise"]).cuda()
            res[f"sampling_h{dh}_T{T}_B{B}"] = timed(lambda: eng.ddim_sample(x2d, nz), samples, 2)   # warm-up: eager pass + capture, a replay
        ran = {k: eng.info(k) for k in ("long_temporal_last", "long_temporal_h32_last", "attn_h128_last")}
        assert ran == {"long_temporal_last": int(dh == 64), "long_temporal_h32_last": int(dh == 32), "attn_h128_last": 5 * int(dh == 128)}, ran
        del eng, diff, net
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libd3d_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_x3_stream_refactor.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--leg-lib", help="(child) run one leg with this library and print its cells as JSON")
    a = ap.parse_args()
    if a.leg_lib:
        print("LEG " + json.dumps(leg(os.path.abspath(a.leg_lib), a.samples)), flush=True)
        return
    from diff3dhpe_amd import _lib
    libs = {"parent": os.path.abspath(a.parent_lib), "new": _lib.LIB_PATH}
    assert os.path.exists(libs["parent"]) and os.path.exists(libs["new"]) and libs["parent"] != libs["new"], libs
    rounds = {"parent": [], "new": []}
    for r in range(a.rounds):
        for name, path in libs.items():
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg-lib", path, "--samples", str(a.samples)], capture_output=True,
                               text=True, timeout=600)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG ")]
            if p.returncode != 0 or not lines:
                sys.exit(f"round {r} leg {name}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            rounds[name].append(json.loads(lines[-1][4:]))
            print(f"round {r} {name}: " + " ".join(f"{k}={v:.3f}" for k, v in rounds[name][-1].items()), flush=True)
    cells = []
    for k in rounds["parent"][0]:
        par, new = [x[k] for x in rounds["parent"]], [x[k] for x in rounds["new"]]
        spread = max(par) - min(par)
        cells.append({"cell": k, "parent_ms": statistics.median(par), "new_ms": statistics.median(new), "parent_spread_ms": spread,
                      "parent_round_medians_ms": par, "new_round_medians_ms": new,
                      "not_slower_than_parent_by_more_than_its_spread": bool(statistics.median(new) - statistics.median(par) <= spread)})
        c = cells[-1]
        print(f"{k}: parent {c['parent_ms']:.3f} ms, new {c['new_ms']:.3f} ms, parent spread {spread:.3f} ms -> "
              f"{'ok' if c['not_slower_than_parent_by_more_than_its_spread'] else 'SLOWER'}")
    res = {"what": f"key-streaming F16X3 attention, library of the tree (new) against the library of {a.parent_commit or 'the parent commit'} "
                   f"(parent): one process per leg and round, legs alternating, {a.rounds} rounds of {a.samples} samples; ms are medians of round "
                   f"medians, spread = max - min of the parent leg's round medians; op: the single-op hooks (split, kernel, merge), sampling: "
                   f"{STEPS}-step DDIM sampling, depth {DEPTH}, 8 heads, hipGraph replay",
           "cells": cells, "all_ok": all(c["not_slower_than_parent_by_more_than_its_spread"] for c in cells)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(a.out, "all ok" if res["all_ok"] else "NOT all ok")


if __name__ == "__main__":
    main()
