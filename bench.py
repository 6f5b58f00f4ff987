#!/usr/bin/env python3
"""Headline benchmark: pose-sequences/sec of the DDIM sampling hot path (BASELINE.json metric).

One "step" = one full S-step `d3d_ddim_sample` over one resident batch of synthetic CPN-style windows (plus the
flip-free evaluate() tail: all-gather of the predicted sequences when N > 1 and the MPJPE reduction kernel).
Default workload = the per-GPU shard of BASELINE.json configs[2]: T=243, J=17, D=512, depth=8, 9 DDIM steps,
B=64 sequences per GPU (weak scaling: the 8-GPU run is the full B=512 of that config).

    python bench.py --gpus 1 --steps 3 --warmup 1
    python bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR   (also writes the last timed step's outputs: dump_outputs())
    python bench.py --gpus 1 --steps 3 --warmup 1 --full               (also everything beyond the headline, see below)
    python bench.py --gpus N ...            (no launcher: bench.py starts its N rank processes itself, self_launch())
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Prints ONE JSON line on rank 0 (contract in the task statement).  The timed region runs the engine exactly as a user gets
it (per-kernel event timing OFF; `headline_under` names the launch mode: eager / graph / 2-stream).  A plain run does only what
the headline needs: set-up, warm-up, the timed steps, --dump-outputs, the line; its `roofline` is the whole-path figure of the
timed region.  --full adds, after the timed region: a separate profiled pass behind the per-kernel `roofline` (same batch, ONE
stream, HIP events around every kernel on the launch stream), the batch-vs-pair self-check, and on one GPU the companion legs
(companion_legs()), `machine_probes` and `cpu_baseline`, the CPU oracle (a port of the reference's op sequence) timed on this
node's host cores on a bounded sample.  --profile-steps, --no-selfcheck, --no-extras and --no-cpu-baseline trim a --full run.
"""
import argparse
import json
import os
import sys
import time

_T_IMPORT = time.time()      # (startup_s: process creation -> first sampling done; the creation time itself comes from psutil)

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# dense MFMA peaks (MI355X_MICROARCH.md): fp32 157.3, fp16/bf16 2500 TFLOP/s.  F16X3 issues 3 fp16 MFMAs per
# algorithmic product, so its ceiling in ALGORITHMIC (fp32-equivalent) flops is 2500/3.
PEAK_TFLOPS = {"fp32": 157.3, "f16x3": 2500.0 / 3.0, "bf16": 2500.0}
DTYPE_NAME = {"fp32": "f32", "f16x3": "f16x3", "bf16": "bf16"}   # f16x3: fp16 hi/lo operand pairs, 3 MFMAs per product, fp32 accumulate


def flops_per_seq_step(T, D=512, J=17):
    return J * T * (256 * D * D + 544 * D + 32 * T * D)       # F(T)


def usable_cpus():
    """(CPUs this process may run on, CPUs its cgroup's CFS quota pays for or None): a GPU box of the pool shows every host CPU in
    the affinity mask while its container is paid a fraction of them -- more runnable threads than the quota only get throttled."""
    try:
        aff = len(os.sched_getaffinity(0))
    except AttributeError:
        aff = os.cpu_count() or 1
    quota = None
    cands = ["/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"]
    try:
        for ln in open("/proc/self/cgroup").read().splitlines():
            _, ctrl, path = ln.split(":", 2)
            if ctrl == "":
                cands.insert(0, "/sys/fs/cgroup" + path.rstrip("/") + "/cpu.max")
            elif "cpu" in ctrl.split(","):
                cands.insert(0, "/sys/fs/cgroup/cpu" + path.rstrip("/") + "/cpu.cfs_quota_us")
    except Exception:
        pass
    for c in cands:
        try:
            txt = open(c).read().split()
            if c.endswith("cpu.max"):
                q = None if txt[0] == "max" else float(txt[0]) / float(txt[1])
            else:
                per = float(open(c.replace("cfs_quota_us", "cfs_period_us")).read())
                q = None if float(txt[0]) <= 0 else float(txt[0]) / per
            if q is not None:
                quota = q if quota is None else min(quota, q)
        except Exception:
            continue
    return aff, quota


def cpu_baseline(T, S, seed, budget_s=40.0):
    """The oracle (port of the reference's eager op sequence) on the host cores, bounded to ~budget_s of CPU work.

    Every DDIM step costs the same, so throughput is measured on whole steps and scaled to S steps where the budget does not
    allow all of them: (1) thread-count sweep on one step at B=1 (big hosts are much slower with one thread per logical CPU
    than with a few dozen); (2) one step at each B in {1, 2, 4, 8} -- a larger B is skipped, and
    reported as skipped, when its projected time does not fit the budget (the reference's CPU path gets slower per sequence
    as B grows); (3) the best B is timed three times on as many of the S steps as fit (all S when
    they do): the minimum is reported, with the max/min spread of the three."""
    import torch
    from oracle import d3d_oracle as orc
    from diff3dhpe_amd.spec import DenoiserConfig
    from diff3dhpe_amd.synth import synth_state_dict, synth_inputs
    avail, quota = usable_cpus()
    cfg = DenoiserConfig(num_frame=T, embed_dim=512, depth=8)
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, seed).items()}
    tabs = orc.diffusion_tables("cosine", 1000)

    def run(B, steps):
        inp = synth_inputs(B, T, seed=42)
        t0 = time.time()
        orc.ddim_sample_loop(sd, tabs, torch.from_numpy(inp["x2d"]), torch.from_numpy(inp["noise"]), num_timesteps=1000,
                             sampling_timesteps=steps, depth=8)
        return time.time() - t0

    t_start = time.time()
    left = lambda: budget_s - (time.time() - t_start)
    sweep = {}
    for th in sorted({t for t in (8, 16, 32, 64) if t <= avail} | ({avail} if avail <= 64 else set())):
        torch.set_num_threads(th)
        sweep[th] = run(1, 1)
        if left() < budget_s * 0.75:
            break
    best_th = min(sweep, key=sweep.get)
    torch.set_num_threads(best_th)
    per_step = {1: sweep[best_th]}          # seconds per DDIM step, by B
    skipped = []
    for B in (2, 4, 8):
        proj = per_step[max(per_step)] * (B / max(per_step)) * 1.5      # at least linear in B on this path
        if proj > left() * 0.35:
            skipped.append(B)
            continue
        per_step[B] = run(B, 1)
    bestB = min(per_step, key=lambda b: per_step[b] / b)
    n = max(1, min(S, int(left() / 3.0 / per_step[bestB])))
    reps = [run(bestB, n) / n for _ in range(3)]
    d = min(reps)
    return {"value": round(bestB / (d * S), 4), "unit": "pose-seq/s", "cores": best_th, "kind": "port",
            "spread_max_over_min": round(max(reps) / d, 3),
            "host_cpus": {"affinity": avail, "cgroup_quota": quota},
            "all_cores_concurrent": cpu_baseline_concurrent(T, S, seed, best_th, avail, per_step[1], quota=quota),
            "sample": f"fp32 eager CPU oracle (port of the reference op sequence; cross-timed against the imported reference in the "
                      f"build container: profiles/r02_cpu_oracle_vs_reference.json), T={T}: thread sweep on 1 DDIM step at B=1 "
                      f"{ {k: round(v, 2) for k, v in sweep.items()} } s; 1 step at B in {sorted(per_step)}: "
                      f"{ {b: round(v, 2) for b, v in per_step.items()} } s (B {skipped} skipped: projected beyond the "
                      f"{budget_s:.0f} s budget); best B={bestB} timed 3x on {n} of {S} steps "
                      f"({', '.join(f'{r:.2f}' for r in reps)} s/step; min reported, scaled to {S} steps); "
                      f"host has {avail} usable CPUs"}


def cpu_worker(T, seed, threads, run_s):
    """Child of cpu_baseline_concurrent (`bench.py --cpu-worker T,seed,threads,seconds`; never touches the GPU): build the oracle's
    inputs, say "ready", wait for "go" on stdin, run whole DDIM steps at B=1 for ~run_s seconds, print {"steps", "seconds"}."""
    import torch
    from oracle import d3d_oracle as orc
    from diff3dhpe_amd.spec import DenoiserConfig
    from diff3dhpe_amd.synth import synth_state_dict, synth_inputs
    torch.set_num_threads(threads)
    cfg = DenoiserConfig(num_frame=T, embed_dim=512, depth=8)
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, seed).items()}
    tabs = orc.diffusion_tables("cosine", 1000)
    inp = synth_inputs(1, T, seed=42)
    x2d, nz = torch.from_numpy(inp["x2d"]), torch.from_numpy(inp["noise"])
    one = lambda: orc.ddim_sample_loop(sd, tabs, x2d, nz, num_timesteps=1000, sampling_timesteps=1, depth=8)
    print("ready", flush=True)
    if sys.stdin.readline().strip() != "go":
        return
    t0, n = time.time(), 0
    while n == 0 or time.time() - t0 < run_s:
        one()
        n += 1
    print(json.dumps({"steps": n, "seconds": time.time() - t0}), flush=True)


def cpu_baseline_concurrent(T, S, seed, best_th, avail, step_s_alone, run_s=8.0, max_procs=16, quota=None):
    """The same oracle on ALL of this node's usable cores at once: k = usable CPUs // best_th processes (capped), each a B=1
    sampling loop on best_th threads, started together; throughput = whole DDIM steps finished by all of them / wall / S.  This is
    the figure "the node's own host cores" can deliver for independent windows -- the single-process number above is the
    reference's own form (one Python process, RUN).  Children are fresh processes that never touch the GPU."""
    import subprocess
    eff = avail if not quota else max(1, min(avail, int(quota)))        # CPUs this container is PAID for (cgroup CFS quota), not just shown
    k = max(1, min(max_procs, eff // max(best_th, 1)))
    if k == 1:     # the quota (or the mask) holds one such process: the concurrent figure IS the single-process one -- nothing to run
        return {"value": None, "processes": 1, "threads_per_process": best_th, "cgroup_cpu_quota": quota, "equal_to_single_process": True,
                "note": f"{avail} CPUs in the affinity mask, cgroup CFS quota {quota}: this container is paid for {eff} CPUs, which hold ONE oracle "
                        f"process at its best thread count ({best_th}); more processes are only throttled (measured once on this pool: 16 x 16 "
                        "threads under a 16-CPU quota took 43x longer per step).  The all-cores figure of this container equals the single-process one"}
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-worker", f"{T},{seed},{best_th},{run_s}"]
    env = dict(os.environ, OMP_NUM_THREADS=str(best_th), HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    procs = []
    try:
        for _ in range(k):
            procs.append(subprocess.Popen(cmd, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True))
        for p in procs:
            if p.stdout.readline().strip() != "ready":
                raise RuntimeError("cpu worker did not come up")
        t0 = time.time()
        for p in procs:
            p.stdin.write("go\n")
            p.stdin.flush()
        outs = [json.loads(p.stdout.readline()) for p in procs]
        wall = time.time() - t0
        for p in procs:
            p.wait(timeout=30)
        steps = sum(o["steps"] for o in outs)
        return {"value": round(steps / wall / S, 4), "unit": "pose-seq/s", "processes": k, "threads_per_process": best_th,
                "cores": k * best_th, "steps_finished": steps, "wall_s": round(wall, 2),
                "one_process_alone_s_per_step": round(step_s_alone, 3), "cgroup_cpu_quota": quota,
                "s_per_step_under_load": round(max(o["seconds"] / o["steps"] for o in outs), 3),
                "note": f"{k} concurrent B=1 oracle processes x {best_th} threads for ~{run_s:.0f} s each, whole DDIM steps counted, scaled to "
                        f"{S} steps per sequence; {avail} CPUs in the affinity mask, cgroup CFS quota {quota} (a quota below processes x threads "
                        "throttles them: the figure is what THIS container is given, not what the bare node could do)"}
    except Exception as ex:
        return {"value": None, "error": str(ex)[:200], "processes": k}
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()


def companion_legs(a, diff, net, eng, x2d, noise, gt, dev, T, S, Bl):
    """Short legs after the timed region, so that the numbers DESIGN.md quotes beside the headline are observed by whoever
    runs bench.py --full (single GPU only; each leg: 1 warm call, then 2 timed calls between device synchronisations):
      graph_vs_eager              the same sampling with profiling off, as eager launches and as ONE hipGraph replay of the whole
                                  S-step loop (BASELINE configs[3]: d3d_engine_set_graph_mode), outputs compared bit for bit
      evaluate_equiv_frames_per_s the reference evaluate() unit (RUN:575-621): two samplings per window (flip-TTA) + un-flip /
                                  average + masked MPJPE, frames of the batch per wall second
      fp32_mode                   the exact-fp32 engine (v_mfma_f32_32x32x2_f32) on the same batch: value and MFMA roofline fraction"""
    import torch
    from diff3dhpe_amd.evaluate import evaluate
    out = {}

    def timed(fn, n=2):
        fn()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            r = fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / n, r

    modes, ref, same = {}, None, True
    for name, st, gr in (("eager_1stream", 1, False), ("eager_2stream", 2, False), ("graph_2stream", 2, True)):
        eng.set_option("streams", st)
        eng.set_graph_mode(gr)
        t, y = timed(lambda: eng.ddim_sample(x2d, noise))
        modes[name] = round(t * 1e3, 3)
        ref = y if ref is None else ref
        same = same and bool(torch.equal(y, ref))
    eng.set_graph_mode(False)
    eng.set_option("streams", a.streams)
    out["launch_modes"] = {"ms_per_sampling": modes, "bit_identical_across_modes": same,
                           "note": "the same sampling (profiling off) as eager launches / as ONE hipGraph replay of the whole S-step loop "
                                   "(d3d_engine_set_graph_mode), on one stream / as two half-batches on two streams (\"streams\" option)"}
    out["graph_vs_eager"] = {"eager_ms": modes["eager_2stream"], "graph_ms": modes["graph_2stream"],
                             "graph_over_eager": round(modes["graph_2stream"] / modes["eager_2stream"], 4), "bit_identical": same,
                             "under": "two streams (the default)"}
    # serving latency of small batches (visualisation scripts: B = 1; the ragged last batch of evaluate()): ms per S-step sampling
    small = {}
    for b in (1, 4):
        if b < x2d.shape[0]:
            xs, ns = x2d[:b].contiguous(), noise[:b].contiguous()
            t, _ = timed(lambda: eng.ddim_sample(xs, ns), n=3)
            small[str(b)] = round(t * 1e3, 3)
    if small:
        out["small_batch_latency_ms"] = dict(small, note="ms per sampling at B = 1 / B = 4 on this engine (eager launches, default streams)")
    if (T, S, Bl) == (243, 9, 64) and a.precision == "f16x3" and not a.seq2frame and a.scaling == "weak":
        # BASELINE configs[2] EXACTLY (B = 512) on this one GPU, so that a driver-timed figure exists for the configuration as written;
        # the headline stays the B = 64 per-GPU shard (comparable with rounds 1-5)
        try:
            from diff3dhpe_amd.synth import synth_inputs_rows
            big = synth_inputs_rows(0, 512, T, seed=42)
            xb, nb = torch.from_numpy(big["x2d"]).to(dev), torch.from_numpy(big["noise"]).to(dev)
            tb512, yb512 = timed(lambda: eng.ddim_sample(xb, nb), n=2)
            out["strong_B512_N1"] = {"value": round(512 / tb512, 3), "unit": "pose-seq/s", "ms_per_step": round(tb512 * 1e3, 2),
                                     "finite": bool(torch.isfinite(yb512).all()),
                                     "first_64_rows_equal_the_headline_batch": bool(torch.equal(yb512[:x2d.shape[0]], eng.ddim_sample(x2d, noise))),
                                     "note": "BASELINE configs[2] as written (global batch 512) on ONE GPU: 2 timed samplings after 1 warm one"}
            del xb, nb, yb512
        except Exception as ex:          # (e.g. a smaller-memory device) never fails the run
            out["strong_B512_N1"] = {"error": str(ex)[:200]}
    if a.precision == "f16x3":
        # cost of reading the range guard the way the Python layer does by default: one one-lane snapshot kernel behind the call + a
        # wait on ITS event (never the device) -- timed back to back on an idle stream, i.e. with nothing to hide behind
        torch.cuda.synchronize(dev)
        n_rt = 200
        t0 = time.perf_counter()
        for _ in range(n_rt):
            eng.take_range(eng.post_range(), block=True)
        us = (time.perf_counter() - t0) / n_rt * 1e6
        out["range_guard_read"] = {"us_per_call_post_plus_wait_idle_stream": round(us, 1),
                                   "frac_of_one_sampling": round(us * 1e-3 / max(modes["eager_2stream"], 1e-9), 6),
                                   "note": "d3d_engine_range_post + d3d_engine_range_take(block) per call; the timed region above posts "
                                           "one ticket per sampling and reads it behind the step's own synchronisation"}
    batch = {"inputs_2d": x2d, "inputs_3d": gt[:x2d.shape[0]], "init_noise": noise, "init_noise_flip": noise}
    tv, res = timed(lambda: evaluate(diff, [batch], scale=1.0, device=dev, verbose=False), n=1)
    To = gt.shape[1]                               # target frames per window: T, or 1 for a seq2frame model
    out["evaluate_equiv_frames_per_s"] = {"value": round(Bl * To / tv, 1), "unit": "frames/s", "windows_per_s": round(Bl / tv, 3),
                                          "mpjpe_mm_vs_synthetic_gt": round(res["mpjpe_mm"], 3),
                                          "note": "evaluate(): 2 DDIM samplings per window (normal + flipped 2D) + merge + MPJPE (RUN:575-621; "
                                                  "a seq2frame model -- the 3DHP runner's form -- predicts ONE frame per window)"}
    if a.precision != "fp32":
        net.precision = "fp32"
        e32 = diff._engine(dev)
        t32, _ = timed(lambda: e32.ddim_sample(x2d, noise), n=1)
        net.precision = a.precision
        v32 = Bl / t32
        out["fp32_mode"] = {"value": round(v32, 3), "unit": "pose-seq/s", "ms_per_step": round(t32 * 1e3, 3),
                            "whole_step_tflops": round(flops_per_seq_step(T) * S * v32 / 1e12, 2),
                            "frac_of_fp32_mfma_peak": round(flops_per_seq_step(T) * S * v32 / 1e12 / PEAK_TFLOPS["fp32"], 4),
                            "note": "exact-fp32 companion (D3D_PREC_FP32), whole path against the 157.3 TFLOP/s fp32 MFMA peak"}
    if a.precision == "f16x3":
        # bf16 operand mode (BASELINE configs[1] names it): SECOND-CLASS -- narrower than the reference's fp32, it cannot meet the
        # 1e-4 gate and is never the headline; reported with its distance to the default precision on this very batch
        y_ref = eng.ddim_sample(x2d, noise)
        net.precision = "bf16"
        eb = diff._engine(dev)
        eb.set_option("streams", a.streams)
        tb, yb = timed(lambda: eb.ddim_sample(x2d, noise), n=2)
        eb.set_option("streams", 1)
        eb.profile_reset()
        eb.set_profiling(True)
        eb.ddim_sample(x2d, noise)
        torch.cuda.synchronize(dev)
        eb.set_profiling(False)
        pb = eb.profile_read()
        net.precision = a.precision
        vb = Bl / tb
        lin = pb["linear"]
        out["bf16_mode"] = {"value": round(vb, 3), "unit": "pose-seq/s", "ms_per_step": round(tb * 1e3, 3),
                            "whole_step_tflops": round(flops_per_seq_step(T) * S * vb / 1e12, 2),
                            "frac_of_bf16_mfma_peak": round(flops_per_seq_step(T) * S * vb / 1e12 / PEAK_TFLOPS["bf16"], 4),
                            "gemm_tflops": round(lin["flops"] / (lin["ms"] * 1e-3) / 1e12, 1) if lin["ms"] else None,
                            "by_kernel_ms_per_step": {k: round(v["ms"], 3) for k, v in pb.items() if v["launches"] and not k.startswith("linear_")},
                            "by_gemm_avg_launch_ms": {k[7:]: round(v["ms"] / v["launches"], 4) for k, v in pb.items() if k.startswith("linear_") and v["launches"]},
                            "vs_default_precision_on_this_batch": {
                                "max_abs": round(float((yb - y_ref).abs().max()), 5),
                                "mpjpe_normalised": round(float((yb - y_ref).norm(dim=-1).mean()), 6)},
                            "note": "D3D_PREC_BF16: bf16 operands for the block GEMMs and both attention products (one MFMA per product), "
                                    "fp32 residual stream / LayerNorm / softmax / DDIM update; second-class precision -- gated against the "
                                    "oracle's bf16-operand emulation (tests/test_gpu_bf16.py), NOT against the 1e-4 gate; never the headline"}
    return out


class PowerSampler:
    """Socket power / shader clock of THIS rank's card while the timed region runs, read from the amdgpu hwmon files (sysfs; no GPU call, no
    privilege, ~20 samples a second on a daemon thread): the bench line then says by itself whether the path ran at the board's power cap
    (DESIGN section 5).  The card is matched by PCI address; every failure mode (no sysfs, no match) gives None, never an error."""

    def __init__(self, pci_bus_id, root="/sys/class/drm"):
        import glob
        self.files = None
        self.rows = []
        self._stop = None
        try:
            want = (pci_bus_id or "").lower()
            for dev in sorted(glob.glob(os.path.join(root, "card[0-9]*", "device"))):
                real = os.path.realpath(dev).lower()
                if not want or not real.endswith(want):
                    continue
                hw = sorted(glob.glob(os.path.join(dev, "hwmon", "hwmon*")))
                if not hw:
                    continue
                pw = next((q for q in (os.path.join(hw[0], "power1_input"), os.path.join(hw[0], "power1_average")) if os.path.exists(q)), None)
                fq = os.path.join(hw[0], "freq1_input")
                if pw:
                    self.files = {"power": pw, "sclk": fq if os.path.exists(fq) else None, "cap": os.path.join(hw[0], "power1_cap"), "card": dev}
                break
        except Exception:
            self.files = None

    @staticmethod
    def _num(path):
        try:
            with open(path) as f:
                return float(f.read().strip())
        except Exception:
            return None

    def start(self):
        if not self.files:
            return
        import threading
        self._stop = threading.Event()

        def loop():
            while not self._stop.is_set():
                self.rows.append((self._num(self.files["power"]), self._num(self.files["sclk"]) if self.files["sclk"] else None))
                time.sleep(0.05)
        self._th = threading.Thread(target=loop, daemon=True)
        self._th.start()

    def stop(self):
        if not self.files or self._stop is None:
            return None
        self._stop.set()
        self._th.join(timeout=1.0)

        def st(xs, scale):
            xs = sorted(x / scale for x in xs if x is not None)
            if not xs:
                return None
            return {"p50": round(xs[len(xs) // 2], 1), "mean": round(sum(xs) / len(xs), 1), "p95": round(xs[min(len(xs) - 1, int(0.95 * len(xs)))], 1)}
        cap = self._num(self.files["cap"])
        pw = st([r[0] for r in self.rows], 1e6)
        out = {"socket_power_W": pw, "power_cap_W": cap / 1e6 if cap else None, "sclk_MHz": st([r[1] for r in self.rows], 1e6), "samples": len(self.rows),
               "source": "amdgpu hwmon (power1_input, freq1_input) of this rank's card, ~20 samples/s over the timed region, no GPU call"}
        if pw and cap:
            out["frac_of_cap_p50"] = round(pw["p50"] / (cap / 1e6), 4)
        return out


def _mark_ready():
    """Tell the self-launcher's watchdog that this rank's first sampling is done (a file in D3D_BENCH_READY_DIR; no-op elsewhere)."""
    d = os.environ.get("D3D_BENCH_READY_DIR")
    if d:
        try:
            open(os.path.join(d, "rank_" + os.environ.get("RANK", "0")), "w").close()
        except OSError:
            pass


def self_launch(n: int) -> int:
    """`python bench.py --gpus N` without a launcher: start N fresh rank processes (one per GPU) and relay rank 0's JSON line.

    The parent never imports torch and never touches HIP -- it only spawns `sys.executable bench.py <same argv>` N times with
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set (never an exec of a process that has initialised the GPU),
    waits for all of them and returns the first non-zero exit code.  Rank 0's stdout is relayed unchanged (the ONE JSON line);
    the other ranks' stdout goes to stderr.  The torchrun form (WORLD_SIZE already set) does not come through here."""
    import socket
    import subprocess
    port = os.environ.get("MASTER_PORT")
    if not port:
        with socket.socket() as sk:           # a free port on the loopback interface
            sk.bind(("127.0.0.1", 0))
            port = str(sk.getsockname()[1])
    import signal
    import tempfile
    procs = []
    # Watchdog: every rank touches <ready_dir>/rank_<r> when its first sampling (and reduction) is done; a rank that
    # has not done so `startup_timeout_s` after its start (D3D_BENCH_STARTUP_TIMEOUT_S, default 120: imports + weight commit + rendezvous +
    # code-object loads take 5 ... 20 s) is named, every rank is ended and the launcher exits non-zero -- a hung rendezvous does not
    # sit until the harness's own limit
    startup_timeout_s = float(os.environ.get("D3D_BENCH_STARTUP_TIMEOUT_S", "120"))
    ready_dir = tempfile.mkdtemp(prefix="d3d_bench_ready_")

    def end_children(grace=5.0):
        """terminate() every live child (its whole session: start_new_session below), wait briefly, then kill()."""
        live = [p for p in procs if p.poll() is None]
        for p in live:
            try:
                os.killpg(p.pid, signal.SIGTERM)
            except (ProcessLookupError, PermissionError):
                p.terminate()
        t_end = time.time() + grace
        for p in live:
            try:
                p.wait(timeout=max(0.0, t_end - time.time()))
            except subprocess.TimeoutExpired:
                try:
                    os.killpg(p.pid, signal.SIGKILL)
                except (ProcessLookupError, PermissionError):
                    p.kill()
                p.wait()

    def on_term(signum, frame):       # a harness that ends only the launcher must not leave ranks waiting in a collective
        raise KeyboardInterrupt(f"signal {signum}")
    old_handlers = {sg: signal.signal(sg, on_term) for sg in (signal.SIGTERM, signal.SIGHUP)}
    first_bad = None
    with tempfile.TemporaryFile() as out0:
        try:
            for r in range(n):
                env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                           MASTER_ADDR=os.environ.get("MASTER_ADDR", "127.0.0.1"), MASTER_PORT=port, D3D_BENCH_LAUNCHER="self",
                           D3D_BENCH_READY_DIR=ready_dir)
                env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC (RCCL across processes on this driver)
                procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                              stdout=out0 if r == 0 else sys.stderr, start_new_session=True))
            t_start = time.time()
            watchdog_done = startup_timeout_s <= 0
            while any([p.poll() is None for p in procs]):     # (a list: every child is polled each round)
                for r, p in enumerate(procs):
                    if first_bad is None and p.returncode not in (None, 0):
                        first_bad = (r, p.returncode)
                        end_children()         # a dead rank leaves the others waiting in a collective: end exactly our children
                if not watchdog_done and first_bad is None:
                    ready = [os.path.exists(os.path.join(ready_dir, f"rank_{r}")) for r in range(n)]
                    if all(ready):
                        watchdog_done = True
                    elif time.time() - t_start > startup_timeout_s:
                        slow = [r for r in range(n) if not ready[r]]
                        print(f"bench.py self-launch: rank(s) {slow} had not finished a first sampling {startup_timeout_s:.0f} s after the "
                              f"start (D3D_BENCH_STARTUP_TIMEOUT_S); ending all ranks", file=sys.stderr)
                        first_bad = (slow[0], 124)
                        end_children()
                time.sleep(0.05)
        except KeyboardInterrupt as ex:
            print(f"bench.py self-launch: interrupted ({ex or 'SIGINT'}); ending the rank processes", file=sys.stderr)
            first_bad = first_bad or (-1, 130)
        finally:
            end_children()                     # whatever ends the launcher -- Ctrl-C, SIGTERM, an exception -- no rank outlives it
            for sg, h in old_handlers.items():
                signal.signal(sg, h)
            import shutil
            shutil.rmtree(ready_dir, ignore_errors=True)
        out0.seek(0)
        sys.stdout.write(out0.read().decode(errors="replace"))
        sys.stdout.flush()
    if first_bad is None:
        first_bad = next(((r, p.returncode) for r, p in enumerate(procs) if p.returncode != 0), None)
    if first_bad is not None:
        if first_bad[0] >= 0:
            print(f"bench.py self-launch: rank {first_bad[0]} failed with exit code {first_bad[1]}", file=sys.stderr)
        return first_bad[1] if 0 < first_bad[1] < 256 else 1
    return 0


DUMP_LIMIT_BYTES = 64 * 1000 * 1000      # --dump-outputs: all files together, .npy headers included


def dump_outputs(out_dir, pred, err, cnt, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: what the last timed step returned to its caller, as <out_dir>/<name>.npy.

    pred.npy         float32 (B, F, J, 3): the sampled poses of the (gathered) batch -- every sequence, or, when they would not fit
                     in `limit`, a fixed sample of sequences (seeded, so equal arguments give equal rows; listed in the returned dict)
    mpjpe_sums.npy   float64 (2,): the two sums of the MPJPE reduction (error sum, joint count)
    The inputs are a pure function of the arguments (synth_state_dict / synth_inputs_rows), so two builds run with the same
    arguments can be compared file for file.  Returns a small dict for the JSON line."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    p = pred.detach().float().cpu().numpy()
    sums = np.array([err, cnt], dtype=np.float64)
    rows = None
    budget = limit - sums.nbytes - 2 * 4096                      # (room for the two .npy headers)
    row_bytes = max(p[:1].nbytes, 1)
    if p.nbytes > budget:
        k = max(budget // row_bytes, 0)
        rows = np.sort(np.random.default_rng(0).choice(p.shape[0], size=k, replace=False))
        p = p[rows]
    np.save(os.path.join(out_dir, "pred.npy"), np.ascontiguousarray(p, dtype=np.float32))
    np.save(os.path.join(out_dir, "mpjpe_sums.npy"), sums)
    return {"dir": out_dir, "files": {"pred": list(p.shape), "mpjpe_sums": list(sums.shape)},
            "pred_rows": "all" if rows is None else rows.tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=64, help="sequences per GPU (weak scaling: the global batch is --batch x --gpus)")
    ap.add_argument("--global-batch", type=int, default=None,
                    help="global batch, split over the ranks by parallel.shard_bounds (ragged allowed; overrides --batch)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak (default): --batch sequences per GPU; strong: the global batch is fixed -- 512 = BASELINE configs[2] exactly "
                         "unless --global-batch says otherwise -- and split over the ranks (legal at N=1: 34 GB of workspace)")
    ap.add_argument("--cpu-worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--frames", type=int, default=243)
    ap.add_argument("--sampling", type=int, default=9)
    ap.add_argument("--precision", default="f16x3", choices=["fp32", "f16x3", "bf16"],
                    help="f16x3: fp32-accurate GEMMs from 3 fp16 MFMAs (default; passes the same 1e-4 parity gate); fp32: fp32 MFMA; "
                         "bf16: bf16 MFMA operands, second-class (cannot meet the 1e-4 gate: never the headline)")
    ap.add_argument("--streams", type=int, default=2, choices=[1, 2],
                    help="2 (default): the sampling runs as two half-batches on two HIP streams inside the engine (bit-identical, "
                         "fills the partly idle kernel tails); 1: one stream")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also run the profiled pass, the self-check and (one GPU) the companion legs, machine "
                         "probes and CPU baseline; a plain run does only what the headline needs")
    ap.add_argument("--profile-steps", type=int, default=2,
                    help="with --full: samplings of the separate profiled pass behind the roofline object (0: none)")
    ap.add_argument("--option", action="append", default=[], metavar="KEY=VALUE",
                    help="d3d_engine_set_option switch for A/B runs (experiments/ab_option.sh), e.g. fused_postnorm=0")
    ap.add_argument("--seq2frame", action="store_true", help="BASELINE configs[4]: ...S2F... model, (B,1,J,3) targets")
    ap.add_argument("--no-time-emb", action="store_true", help="with_time_emb=False (3DHP command lines)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the cpu_baseline leg")
    ap.add_argument("--cpu-budget", type=float, default=40.0, help="seconds of CPU work for the cpu_baseline leg")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the companion legs after the timed region (fp32 mode, hipGraph replay, evaluate()-equivalent) "
                         "and the machine probes")
    ap.add_argument("--graph", action="store_true",
                    help="time the main leg with hipGraph replay of the whole S-step loop (BASELINE configs[3]); per-kernel event "
                         "timing is off then, so the roofline object carries the whole-path figure only")
    ap.add_argument("--no-selfcheck", action="store_true", help="with --full: skip the bitwise batch-vs-pair check (profiling passes: keeps the kernel tables to the timed workload)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step returned as DIR/<name>.npy (rank 0; see dump_outputs())")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.warmup < 0:
        ap.error("--warmup must not be negative")

    if a.cpu_worker:                 # child of cpu_baseline_concurrent: CPU only
        T_, seed_, th_, run_ = a.cpu_worker.split(",")
        cpu_worker(int(T_), int(seed_), int(th_), float(run_))
        return
    if os.environ.get("D3D_BENCH_LAUNCHER") == "self":
        try:                         # a rank of self_launch(): end with the launcher even if that one is SIGKILLed (PR_SET_PDEATHSIG)
            import ctypes
            import signal
            ctypes.CDLL("libc.so.6", use_errno=True).prctl(1, int(signal.SIGTERM))
        except Exception:
            pass
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: this process becomes the launcher (before torch or HIP are touched)
        sys.exit(self_launch(a.gpus))
    if int(os.environ.get("WORLD_SIZE", "1")) != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={os.environ.get('WORLD_SIZE')} (run `python bench.py --gpus N` "
                         f"plain, or torchrun with --nproc-per-node equal to --gpus)")
    if os.environ.get("D3D_BENCH_LAUNCH_CHECK"):
        # launcher self-test (tests/test_compat_and_dist.py, no GPU): report the rank environment and leave; the rank named by
        # D3D_BENCH_LAUNCH_CHECK_FAIL exits non-zero instead (the launcher must propagate it and end the other ranks)
        r = int(os.environ.get("RANK", "0"))
        if os.environ.get("D3D_BENCH_LAUNCH_CHECK_HANG") == str(r):
            time.sleep(60)                     # (a rank stuck before its first sampling: the launcher's watchdog has to end it)
            return
        _mark_ready()
        if os.environ.get("D3D_BENCH_LAUNCH_CHECK_HANG"):
            time.sleep(60)                     # (the others would sit in a collective waiting for it)
            return
        if os.environ.get("D3D_BENCH_LAUNCH_CHECK_FAIL") == str(r):
            sys.exit(7)
        if os.environ.get("D3D_BENCH_LAUNCH_CHECK_FAIL"):
            time.sleep(30)                     # (a surviving rank would sit in a collective: the launcher has to end it)
        print(json.dumps({"launch_check": True, "rank": r, "local_rank": int(os.environ.get("LOCAL_RANK", "0")),
                          "world_size": int(os.environ.get("WORLD_SIZE", "1")), "master_addr": os.environ.get("MASTER_ADDR"),
                          "master_port": os.environ.get("MASTER_PORT"), "launcher": os.environ.get("D3D_BENCH_LAUNCHER", "none")}),
              file=sys.stdout if r == 0 else sys.stderr, flush=True)
        return

    import torch
    import torch.distributed as dist
    import diff3dhpe_amd as d3d
    from diff3dhpe_amd import parallel
    from diff3dhpe_amd.engine import tta_mpjpe
    from diff3dhpe_amd.spec import DenoiserConfig
    from diff3dhpe_amd.synth import synth_state_dict, synth_inputs_rows

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # D3D_BENCH_ONE_DEVICE=1 + D3D_DIST_BACKEND=gloo: functional test of the N>1 code path with all ranks on cuda:0
    backend = os.environ.get("D3D_DIST_BACKEND", "nccl")
    if os.environ.get("D3D_BENCH_ONE_DEVICE"):
        local = 0
    # D3D_FORCE_DIST=1: form the process group even at world size 1, so that `torchrun --nproc-per-node 1 bench.py --gpus 1`
    # executes init_process_group("nccl", device_id=...), all_gather_into_tensor, all_reduce(MAX) and barrier on a one-rank
    # RCCL communicator -- the N > 1 code path on a one-GPU box (tests/test_gpu_parity.py)
    force_dist = bool(os.environ.get("D3D_FORCE_DIST"))
    use_dist = world > 1 or force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)

    T, S = a.frames, a.sampling
    Bg = a.global_batch if a.global_batch is not None else (512 if a.scaling == "strong" else a.batch * world)
    lo, hi = parallel.shard_bounds(Bg, rank, world)
    Bl = hi - lo                                    # this rank's shard: ranks differ by one row when Bg % world != 0, and a rank
    if Bg < 1:                                      # beyond a tiny global batch holds NO row (it still joins the collective)
        raise SystemExit("bench.py: the global batch must hold at least one sequence")
    cfg = DenoiserConfig(num_frame=T, embed_dim=512, depth=8, seq2frame=a.seq2frame, with_time_emb=not a.no_time_emb)
    net = d3d.HPE_model(d3d.S2F_NAME if a.seq2frame else d3d.S2S_NAME)(
        num_frame=T, num_joints=17, in_chans=2, embed_dim=512, depth=8, num_heads=8, mlp_ratio=2., qkv_bias=True,
        qk_scale=None, drop_path_rate=0.1, with_time_emb=not a.no_time_emb)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 0).items()})
    net.precision = a.precision
    diff = d3d.GaussianDiffusion(model=net, timesteps=1000, sampling_timesteps=S, loss_type="l2", clip_denoised=True,
                                 beta_schedule="cosine", ddim_sampling_eta=0.0, clipLoss=True).eval().to(dev)

    # synthetic batch: every rank builds ONLY its contiguous shard (row i of the global batch is a function of i alone:
    # synth.synth_inputs_rows) and keeps it resident in HBM before the timed region; the ground truth every rank needs for the
    # reduction over the gathered predictions is assembled ONCE, before the timed region, by the same all-gather the path uses
    inp = synth_inputs_rows(lo, hi, T, seed=42)
    x2d = torch.from_numpy(inp["x2d"]).to(dev)
    noise = torch.from_numpy(inp["noise"]).to(dev)
    gt_local = torch.from_numpy(inp["gt3d"]).to(dev)
    if a.seq2frame:   # one target frame per window (DIFF-S2F): noise / ground truth of the centre frame
        noise, gt_local = noise[:, :1].contiguous(), gt_local[:, T // 2:T // 2 + 1].contiguous()
    gt = parallel.all_gather_pred(gt_local, Bg) if world > 1 else gt_local
    census = None
    if use_dist:
        # what the communicator itself saw: its rank count and the number of DISTINCT devices behind those ranks,
        # from the devices' UUIDs gathered over it -- "RCCL saw N ranks on N devices" is then in the line, not an assumption
        try:
            uu = str(getattr(torch.cuda.get_device_properties(dev), "uuid", "")) or f"cuda:{local}@{os.uname().nodename}"
            mine = torch.zeros(64, dtype=torch.uint8)
            raw = uu.encode()[:64]
            mine[:len(raw)] = torch.tensor(list(raw), dtype=torch.uint8)
            mine = mine.to(dev if backend == "nccl" else "cpu")
            allu = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(allu, mine)
            census = {"world": dist.get_world_size(), "distinct_devices": len({bytes(u.cpu().tolist()) for u in allu})}
        except Exception as ex:
            census = {"world": dist.get_world_size(), "distinct_devices": None, "error": str(ex)[:120]}
    eng = diff._engine(dev)
    eng.set_option("streams", a.streams)
    for kv in a.option:
        k, v = kv.split("=", 1)
        eng.set_option(k, int(v))
    ag_events = []                                # (start, end) event pairs around the exchange step of every timed step

    first_done = []                               # wall-clock time at which this rank's first sampling + reduction had completed
    tickets = []                                  # one F16X3 range-guard ticket per sampling: posted behind it, READ after the
                                                  # step's own synchronisation (the read-back of the MPJPE sums) -- never a wait of its own
    guard_on = a.precision == "f16x3"
    seen_flags = [0]                              # OR of the flags read so far

    def step(record=False):
        pred = eng.ddim_sample(x2d, noise)
        if guard_on:
            tickets.append(eng.post_range())
        if record and use_dist:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        pred = parallel.all_gather_pred(pred, Bg, force=force_dist)          # RCCL all-gather (no-op at N=1 unless forced)
        if record and use_dist:
            e1.record()                           # (the current stream waits for the collective before anything behind it)
            ag_events.append((e0, e1))
        res = tta_mpjpe(pred, None, gt, None, 1.0, [], [])          # (reads the two sums back: the step's synchronisation)
        while tickets:                            # ... behind which this sampling's snapshot has run: its flags are there, no wait
            seen_flags[0] |= eng.take_range(tickets.pop(), block=True) or 0
        if not first_done:
            first_done.append(time.time())
            _mark_ready()
        return res, pred

    def fence():
        torch.cuda.synchronize(dev)
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize(dev)

    if a.graph:
        eng.set_graph_mode(True)
    for _ in range(a.warmup):
        step()
    seen_flags[0] = 0                             # (the timed samplings' flags only)
    # ---- timed region: the engine as a user gets it -- per-kernel event timing OFF
    try:
        pr = torch.cuda.get_device_properties(dev)
        pci = "%04x:%02x:%02x.0" % (int(getattr(pr, "pci_domain_id", 0)), int(pr.pci_bus_id), int(pr.pci_device_id))
    except Exception:
        pci = None
    power = PowerSampler(pci) if pci else None
    fence()
    if power:
        power.start()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        (err, cnt), last_pred = step(record=True)
    fence()
    elapsed = time.perf_counter() - t0
    power_stats = power.stop() if power else None
    dumped = dump_outputs(a.dump_outputs, last_pred, err, cnt) if (a.dump_outputs and rank == 0) else None
    rank_ms = elapsed / a.steps * 1e3
    try:                                          # process creation -> first sampling (and its reduction) done on this rank
        import psutil
        t_created = psutil.Process().create_time()
    except Exception:
        t_created = _T_IMPORT
    startup_s = (first_done[0] - t_created) if first_done else None
    range_flags = seen_flags[0]                   # the timed samplings' range flags (read inside step(), behind each step's own sync)
    rank_stats = None
    if use_dist:
        cdev = dev if backend == "nccl" else "cpu"
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=cdev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        tmin = torch.tensor([elapsed], dtype=torch.float64, device=cdev)
        dist.all_reduce(tmin, op=dist.ReduceOp.MIN)
        ag_ms = sum(e0.elapsed_time(e1) for e0, e1 in ag_events) / max(len(ag_events), 1)
        agt = torch.tensor([ag_ms, float(startup_s or 0.0), float(range_flags)], dtype=torch.float64, device=cdev)
        dist.all_reduce(agt, op=dist.ReduceOp.MAX)       # (flags: the max over ranks is non-zero iff any rank saw one)
        range_flags_any = int(agt[2])
        rank_stats = {"ms_per_step_min_over_ranks": round(float(tmin[0]) / a.steps * 1e3, 3),
                      "ms_per_step_max_over_ranks": round(float(tmax[0]) / a.steps * 1e3, 3),
                      "this_rank_ms_per_step": round(rank_ms, 3),
                      "allgather_ms_per_step_max_over_ranks": round(float(agt[0]), 4),
                      "allgather_frac_of_step": round(float(agt[0]) / max(float(tmax[0]) / a.steps * 1e3, 1e-9), 5),
                      "allgather_bytes_per_rank": int(noise.numel() * 4),
                      "rccl_world": (census or {}).get("world") if backend == "nccl" else None,
                      "comm_world": (census or {}).get("world"),
                      "distinct_devices": (census or {}).get("distinct_devices"),
                      "startup_s_max_over_ranks": round(float(agt[1]), 2),
                      "startup_note": "process creation -> this rank's first sampling + reduction done (imports, weight commit, rendezvous, "
                                      "first-launch code-object loads); max over ranks",
                      "range_flags": range_flags_any,
                      "local_batch_min_max": [Bg // world, Bg // world + (1 if Bg % world else 0)],
                      "data_built_per_rank": "its own shard only (synth_inputs_rows); the ground truth of the gathered batch is assembled once, "
                                             "before the timed region, by the path's own all-gather",
                      "allgather_note": "event-timed on the launch stream around parallel.all_gather_pred (includes waiting for the slowest rank's sampling)"}
        elapsed = float(tmax[0])
    if a.graph:
        eng.set_graph_mode(False)
    # ---- profiled pass (--full; outside the timed region): same batch, ONE stream, HIP events around every kernel
    profile_steps = a.profile_steps if a.full else 0
    eng.profile_reset()
    if profile_steps > 0:
        eng.set_option("streams", 1)
        eng.set_profiling(True)
        for _ in range(profile_steps):
            eng.ddim_sample(x2d, noise)
        torch.cuda.synchronize(dev)
        eng.set_profiling(False)
        eng.set_option("streams", a.streams)
    prof = eng.profile_read()
    psteps = max(profile_steps, 1)
    # self-check of the timed configuration (--full; no oracle runs at this size): the first two sequences of the batch, sampled
    # again as a batch of two (the small-problem kernels the golden-vector tests cover), must come out bit-identical
    selfcheck = None
    if a.full and not a.no_selfcheck and Bl >= 2:
        pred_big = eng.ddim_sample(x2d, noise)
        pred_two = eng.ddim_sample(x2d[:2].contiguous(), noise[:2].contiguous())
        selfcheck = bool(torch.equal(pred_big[:2], pred_two)) and bool(torch.isfinite(pred_big).all())

    if rank == 0:
        value = Bg * a.steps / elapsed
        gemm_kinds = {k: v for k, v in prof.items() if k.startswith("linear_")}     # sub-classes of "linear": not added to the total
        prof = {k: v for k, v in prof.items() if not k.startswith("linear_")}
        tot_ms = sum(v["ms"] for v in prof.values()) or 1.0
        # The GEMM-bearing kernels of the F16X3 flow are ONE family -- the x3q k-loop with different epilogues: the plain forms ("linear":
        # proj, fc1, fc2, and the qkv GEMMs of the shapes the fusions do not serve) and the two forms whose epilogue is the block's attention
        # ("qkv_sattn", "qkv_tattn": their time and flops include it).  Since round 4 the qkv GEMMs -- the form closest to the MFMA bound -- live
        # in the fused kernels, so the dominant kernel class priced against the MFMA roofline is the family, not "linear" alone (which is
        # still reported: by_kernel_ms_per_step, by_gemm, and the two fused entries below).
        fam = [k for k in ("linear", "qkv_sattn", "qkv_tattn") if prof.get(k, {}).get("launches")]
        if len(fam) > 1:
            prof_fam = {"ms": sum(prof[k]["ms"] for k in fam), "launches": sum(prof[k]["launches"] for k in fam),
                        "flops": sum(prof[k]["flops"] for k in fam), "bytes": sum(prof[k]["bytes"] for k in fam)}
        else:
            prof_fam = None
        dom = max(prof, key=lambda k: prof[k]["ms"])
        d = prof[dom]
        dom_name = dom
        if prof_fam and dom in fam:
            d, dom_name = prof_fam, "gemm family: " + " + ".join(fam)
            dom = "linear"
        if not d["ms"]:                         # no profiled pass: no per-kernel events; the whole-path figures are filled in below
            roof = {"bound": "mfma", "achieved": None, "peak": round(PEAK_TFLOPS[a.precision], 1), "unit": "TFLOP/s", "frac": None}
        elif dom == "linear" or dom == "attn_temporal":
            ach = d["flops"] / (d["ms"] * 1e-3) / 1e12
            peak = PEAK_TFLOPS[a.precision]
            roof = {"bound": "mfma", "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(ach / peak, 4)}
            if a.precision == "f16x3":
                roof["note"] = ("achieved = algorithmic (fp32-equivalent) flops; the kernel issues 3 fp16 MFMAs per product, "
                                f"i.e. {ach * 3:.0f} TFLOP/s of fp16 MFMA work against the 2500 TFLOP/s dense fp16 peak")
            if prof_fam and d is prof_fam:
                # what the family figure counts: the GEMMs' 2 M N K AND, for the two fused kernels, the attention products
                # 4 M keys D they run in the same launch -- both on the fp16 matrix pipe as three MFMAs per product, so the x3 of
                # `machine_probes.roofline_frac_of_sustained_mfma` applies to all of it; the GEMM-only figure (attention flops left out,
                # time unchanged: a LOWER bound on the GEMM rate) is given beside it for comparison with earlier rounds' "linear"
                Mrows, Dw = Bl * T * 17, 512
                gemm_fl = (prof["linear"]["flops"] + sum(prof[k]["launches"] * 2.0 * Mrows * 3 * Dw * Dw for k in ("qkv_sattn", "qkv_tattn")
                                                            if prof.get(k, {}).get("launches")))
                roof["frac_definition"] = ("family = plain GEMM launches + the two fused qkv/attention kernels; flops = GEMM 2MNK + the fused "
                                           "kernels' attention products (4 M keys D), all issued as 3 fp16 MFMAs per product; "
                                           "peak = 2500/3 TFLOP/s")
                roof["gemm_only"] = {"flops_share": round(gemm_fl / d["flops"], 4),
                                     "frac_lower_bound": round(gemm_fl / (d["ms"] * 1e-3) / 1e12 / peak, 4)}
        else:
            ach = d["bytes"] / (d["ms"] * 1e-3) / 1e9
            roof = {"bound": "hbm", "achieved": round(ach, 1), "peak": 8000.0, "unit": "GB/s", "frac": round(ach / 8000.0, 4)}
        roof.update({"kernel": dom_name, "launches": d["launches"], "avg_launch_ms": round(d["ms"] / max(d["launches"], 1), 4),
                     "share_of_gpu_time": round(d["ms"] / tot_ms, 4), "traffic": None,
                     "timed_in": f"separate profiled pass of {profile_steps} samplings right after the timed region (one stream, HIP events "
                                 "around every kernel on the launch stream)",
                     "by_kernel_ms_per_step": {k: round(v["ms"] / psteps, 3) for k, v in prof.items() if v["launches"]}})
        if prof.get("qkv_sattn", {}).get("launches"):   # spatial blocks: qkv GEMM + 17-key attention in one kernel ("fused_spatial")
            v = prof["qkv_sattn"]
            roof["qkv_sattn"] = {"avg_launch_ms": round(v["ms"] / v["launches"], 4),
                                 "frac": round(v["flops"] / (v["ms"] * 1e-3) / 1e12 / PEAK_TFLOPS[a.precision], 4),
                                 "note": "qkv GEMM (LayerNorm-folded) + spatial attention of a 15-frame group in one kernel; its launches "
                                         "are in neither 'linear' nor 'attn_spatial'"}
        if prof.get("qkv_tattn", {}).get("launches"):   # temporal blocks likewise ("fused_temporal")
            v = prof["qkv_tattn"]
            roof["qkv_tattn"] = {"avg_launch_ms": round(v["ms"] / v["launches"], 4),
                                 "frac": round(v["flops"] / (v["ms"] * 1e-3) / 1e12 / PEAK_TFLOPS[a.precision], 4),
                                 "note": "qkv GEMM (LayerNorm-folded) + temporal attention of one (batch, joint) group in one kernel; its launches "
                                         "are in neither 'linear' nor 'attn_temporal'"}
        if any(v["launches"] for v in gemm_kinds.values()):
            pk = PEAK_TFLOPS[a.precision]
            roof["by_gemm"] = {k[7:]: {"avg_launch_ms": round(v["ms"] / v["launches"], 4),
                                       "frac": round(v["flops"] / (v["ms"] * 1e-3) / 1e12 / pk, 4)}
                               for k, v in gemm_kinds.items() if v["launches"]}
        # HBM bytes per launch cannot be counted from inside the process: they come from the separate rocprofv3 --pmc passes of
        # profiles/collect.sh (FETCH_SIZE doubled per the gfx950 correction + WRITE_SIZE) and are labelled as such
        tfile = os.path.join(ROOT, "profiles", "hbm_traffic.json")
        if d["ms"] and os.path.exists(tfile):
            try:
                tj = json.load(open(tfile))
                key = f"{dom}:T{T}:B{Bl}:{a.precision}"
                roof["traffic"] = tj.get(key)
                if prof_fam and dom_name != dom:      # the family: launch-weighted mean over its classes
                    per = [(tj.get(f"{k}:T{T}:B{Bl}:{a.precision}"), prof[k]["launches"]) for k in fam]
                    roof["traffic"] = (round(sum(b * n for b, n in per) / sum(n for _, n in per)) if all(b is not None for b, _ in per) else None)
                if roof["traffic"] is not None:
                    # the file carries the hash of the library it was collected with (profiles/collect.sh): a kernel change since then
                    # makes the figure stale -- said here instead of silently kept
                    import hashlib
                    from diff3dhpe_amd import _lib as _l
                    sha = hashlib.sha256(open(_l.LIB_PATH, "rb").read()).hexdigest()
                    roof["traffic_stale"] = ((tj.get("_lib_sha256") or {}).get(f"T{T}:B{Bl}:{a.precision}") != sha)
                    roof["traffic_source"] = ("profiles/hbm_traffic.json: mean bytes per launch of this kernel class from the "
                                              f"rocprofv3 --pmc passes of profiles/collect.sh ({tj.get('_collected', 'date not recorded')}), "
                                              "NOT measured in this run")
            except Exception:
                pass
        whole = flops_per_seq_step(T) * S * value / 1e12
        line = {
            "metric": "pose_sequences_per_sec", "value": round(value, 3), "unit": "pose-seq/s", "n_gpus": world,
            "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(elapsed / a.steps * 1e3, 3),
            "higher_is_better": True, "scaling": a.scaling, "vs_baseline": None, "dtype": DTYPE_NAME[a.precision],
            "data": "synthetic",
            "config": {"workload": f"H36M-CPN-shape 2D windows T={T} J=17, MixSTE{'-S2F' if a.seq2frame else ''} D=512 depth=8 "
                                   f"random-init, {S} DDIM steps, "
                                   + (f"B={Bl}/GPU" if Bg == Bl * world else f"global B={Bg} over {world} GPU(s) (this rank {Bl})")
                                   + (" (BASELINE configs[2] per-GPU shard)" if (T, S, Bl) == (243, 9, 64) and Bg == 64 * world and not a.seq2frame else "")
                                   + (" (BASELINE configs[2] exactly: B=512)" if (T, S, Bg) == (243, 9, 512) and not a.seq2frame else "")
                                   + f", eta=0, clip_denoised, {a.scaling} scaling",
                       "global_batch": Bg, "frames": T, "sampling_timesteps": S, "parallelism": f"dp{world}",
                       "precision": a.precision},
            "whole_step_tflops": round(whole, 2),
            "mpjpe_vs_synthetic_gt": round(err / max(cnt, 1), 6),
            "selfcheck_batch_vs_pair_bit_identical": selfcheck,
            # F16X3 range guard over the timed samplings (OR over steps, max over ranks): must be 0 -- a non-zero word means the timed
            # results were NOT fp32-accurate (include/d3d.h D3D_RANGE_*); null for precisions without the guard
            "range_flags": (range_flags_any if use_dist else range_flags) if guard_on else None,
            "startup_s": round(startup_s, 2) if startup_s is not None else None,
            "headline_under": ("2-stream" if (a.streams == 2 and Bl >= 2) else "eager") + ("+graph" if a.graph else ""),
            "roofline": roof,
        }
        if power_stats:
            # rank 0's card over the timed region: at the cap, time is energy (J per pose-sequence = W x s / sequences of THIS rank)
            power_stats["joules_per_pose_sequence"] = (round(power_stats["socket_power_W"]["mean"] * (elapsed / a.steps) / max(Bl, 1), 2)
                                                       if power_stats.get("socket_power_W") else None)
            line["power"] = power_stats
        if rank_stats:
            line["ranks"] = rank_stats
        if a.precision == "f16x3":
            line["precision_note"] = ("f16x3 = fp32-accurate arithmetic from three fp16 MFMAs per product (same 1e-4 parity gate as fp32): "
                                      "the headline precision.  BASELINE configs[1]'s bf16 exists as a second-class mode (--precision bf16, "
                                      "'bf16_mode' companion object): it cannot meet the 1e-4 gate (SURVEY appendix B) and is never the headline")
        if a.precision == "bf16":
            line["precision_note"] = ("bf16 = SECOND-CLASS precision, narrower than the reference's fp32: bf16 operands for the block GEMMs and "
                                      "attention products; fails the 1e-4 parity gate by design (gated against the oracle's bf16-operand "
                                      "emulation instead).  Not a headline number.")
        if a.graph:
            line["graph_replay"] = True
        if dumped:
            line["dump_outputs"] = dumped
        if not d["ms"]:
            roof["note"] = ("no profiled pass (a plain run, or --full --profile-steps 0): 'achieved' is the whole-path figure of the "
                            "timed region")
            roof.update({"kernel": "whole path", "achieved": round(whole, 2), "frac": round(whole / PEAK_TFLOPS[a.precision], 4),
                         "launches": a.steps, "avg_launch_ms": round(elapsed / a.steps * 1e3, 3), "share_of_gpu_time": 1.0,
                         "by_kernel_ms_per_step": {}, "traffic": None, "timed_in": "the timed region (whole path)"})
        if use_dist:
            try:
                rccl = ".".join(str(v) for v in torch.cuda.nccl.version()) if backend == "nccl" else None
            except Exception:
                rccl = None
            line["dist"] = {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "forced_single_rank_group": force_dist,
                            "rccl_version": rccl,
                            "launcher": os.environ.get("D3D_BENCH_LAUNCHER", "torchrun" if "TORCHELASTIC_RUN_ID" in os.environ else "external"),
                            "one_process_per_gpu": not bool(os.environ.get("D3D_BENCH_ONE_DEVICE")),
                            "collectives": ["barrier", "all_gather_into_tensor", "all_reduce(MAX)"]}
    extras = None
    if world == 1 and a.full and not a.no_extras:
        extras = companion_legs(a, diff, net, eng, x2d, noise, gt, dev, T, S, Bl)
    if rank == 0:
        if extras:
            line.update(extras)
        if world == 1 and a.full and not a.no_extras:
            # what THIS chip sustains today for the two resources that co-limit the F16X3 / bf16 GEMM k-loop (d3d_probe_machine): fp16
            # MFMA work in register loops at the power-limited clock, and the k-loop's L2 -> LDS staging stream alone.  Beside the
            # nominal peaks, not instead of them: roofline.frac stays against MI355X_MICROARCH.md's 2.5 PFLOP/s.
            try:
                from diff3dhpe_amd.engine import probe_machine
                pm = probe_machine(dev, ms_target=150.0)
                mp = {"mfma_f16_tflops_sustained": round(pm["mfma_f16_tflops"], 1),
                      "mfma_f16_frac_of_nominal": round(pm["mfma_f16_tflops"] / 2500.0, 4),
                      "l2_to_lds_staging_gbps_chip": round(pm["l2_to_lds_gbps"], 1),
                      "note": "register-only fp16 MFMA loops (2 waves per SIMD, operands with real hi / lo statistics) and the k-loop's LDS-DMA "
                              "stream alone (64 KiB stages from L2-resident rows, no MFMA), each ~150 ms on this device right after the bench"}
                if a.precision in ("f16x3", "bf16") and roof.get("achieved") and roof.get("bound") == "mfma":
                    issued = roof["achieved"] * (3.0 if a.precision == "f16x3" else 1.0)
                    mp["roofline_frac_of_sustained_mfma"] = round(issued / pm["mfma_f16_tflops"], 4)
                line["machine_probes"] = mp
            except Exception as ex:      # a probe never fails a bench run
                line["machine_probes"] = {"error": str(ex)[:200]}
        if world == 1 and a.full and not a.no_cpu_baseline:
            line["cpu_baseline"] = cb = cpu_baseline(T, S, 0, a.cpu_budget)
            acc = cb.get("all_cores_concurrent") or {}
            allc = cb["value"] if acc.get("equal_to_single_process") else acc.get("value")
            line["speedup_vs_cpu_baseline"] = {
                "vs_single_process": round(value / max(cb["value"], 1e-9), 1),
                "vs_all_cores_concurrent": round(value / allc, 1) if allc else None,
                "note": "single process = the reference's own form (one Python process, its best thread count); all cores = as many "
                        "concurrent B=1 oracle processes as the node's usable CPUs hold.  A baseline statement, not a kernel-quality claim"}
        print(json.dumps(line), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
