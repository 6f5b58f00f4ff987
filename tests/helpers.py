"""Shared test helpers: seeded weights/inputs (never the reference; never shipped vectors of weights)."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

from diff3dhpe_amd.spec import DenoiserConfig
from diff3dhpe_amd.synth import synth_state_dict, synth_inputs, hash_uniform


def cfg_small(T=81, **kw):
    return DenoiserConfig(num_frame=T, embed_dim=32, depth=4, **kw)


def cfg_full(T, **kw):
    return DenoiserConfig(num_frame=T, embed_dim=512, depth=8, **kw)


def torch_sd(cfg, seed, family="uniform", qkv_bias=True):
    """The seeded state dict of `family` as torch tensors; qkv_bias=False drops the attention qkv biases (a model built without them)."""
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, seed, family=family).items()}
    if not qkv_bias:
        sd = {k: v for k, v in sd.items() if not k.endswith("attn.qkv.bias")}
    return sd


def inputs(B, T, seed):
    d = synth_inputs(B, T, seed=seed)
    return {k: torch.from_numpy(v) for k, v in d.items()}


def xy(B, T, seed, J=17):
    """(x2d, noise) of the seeded inputs, on the GPU."""
    inp = synth_inputs(B, T, J, seed=seed)
    return torch.from_numpy(inp["x2d"]).cuda(), torch.from_numpy(inp["noise"]).cuda()


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def cu_count():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


# Row counts that put a launcher on a given branch of its ladder depend on the device's CU count: named here, resolved inside the test
# (collection does not touch the GPU).
_ROWS = {"walk256": lambda cu: 256 * 2 * cu + 100,    # 256 x 256 tiles: the persistent walk (>= 4 rounds) with a ragged last round
         "rows128": lambda cu: 128 * cu + 77,         # whole-row tiles: more 128-row tiles than CUs, one tile per workgroup
         "rowswalk": lambda cu: 128 * 4 * cu + 77}    # whole-row tiles: the persistent walk


def _rows(M):
    return _ROWS[M](cu_count()) if isinstance(M, str) else M


# The bounds of tests/test_gpu_latency_mode.py::test_splitk_postnorm_matches_fp64: 3e-6 sqrt(K / 32) + 2e-6 for the GEMM part, 2e-6 more
# for a result read back from planes (22 bits), 2e-3 / 1e-2 for sums / sums of squares.  Operands from the same generators.
def _tol(K):
    return 3e-6 * np.sqrt(K / 32) + 2e-6


def hashed(name, shape, seed, scale=1.0):
    n = int(np.prod(shape))
    return torch.from_numpy((scale * hash_uniform(name, n, seed)).astype(np.float32).reshape(shape))


def build_net(cfg, seed, precision="fp32", family="uniform", sd=None, **ctor):
    """HPE_model of the product with the seeded weights of `family` (or the state dict `sd`), on the CPU.  `ctor` overrides constructor
    arguments (qkv_bias, qk_scale, norm_layer, ...); precision=None leaves the net's default."""
    import diff3dhpe_amd as d3d
    name = d3d.S2F_NAME if cfg.seq2frame else d3d.S2S_NAME
    args = dict(num_frame=cfg.num_frame, num_joints=cfg.num_joints, in_chans=cfg.in_chans,
                embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio,
                qkv_bias=True, qk_scale=None, drop_path_rate=0.1, with_time_emb=cfg.with_time_emb)
    args.update(ctor)
    net = d3d.HPE_model(name)(**args)
    net.load_state_dict(torch_sd(cfg, seed, family, args["qkv_bias"]) if sd is None else sd, strict=True)
    if precision is not None:
        net.precision = precision
    return net


def build_product(cfg, seed, sampling=9, eta=0.0, clip=True, device="cuda", precision="fp32", family="uniform", sd=None, **ctor):
    """build_net + GaussianDiffusion of the product, on `device`."""
    import diff3dhpe_amd as d3d
    net = build_net(cfg, seed, precision, family, sd, **ctor)
    diff = d3d.GaussianDiffusion(model=net, timesteps=1000, sampling_timesteps=sampling, loss_type="l2",
                                 clip_denoised=clip, beta_schedule="cosine", ddim_sampling_eta=eta, clipLoss=True).eval()
    if device != "cpu":
        diff = diff.to(device)
    return net, diff


def product(cfg, seed, prec, sampling=9, family="uniform", **kw):
    """build_product in the argument order of the kernel-option tests: (cfg, seed, precision, sampling steps, weight family)."""
    return build_product(cfg, seed, sampling=sampling, precision=prec, family=family, **kw)


def product_with_engine(cfg, seed, prec, sampling=9, family="uniform", **kw):
    """(net, diff, eng): product() and the engine of the current device."""
    net, diff = product(cfg, seed, prec, sampling, family, **kw)
    return net, diff, diff._engine(dev())


def attn_ref(qkv, B, T, J, H, temporal, dtype=torch.float64):
    """(softmax(q k^T / sqrt(dh)) - I) v in `dtype`: the reference of the GRAND attention core over spatial (b, t) or temporal (b, j) groups."""
    D = qkv.shape[-1] // 3
    dh = D // H
    x = qkv.to(dtype).reshape(B, T, J, 3, H, dh)
    if temporal:
        x = x.permute(0, 2, 1, 3, 4, 5)            # (B, J, T, 3, H, dh): groups are joints
    q, k, v = (x[..., i, :, :].transpose(-3, -2) for i in range(3))   # (.., H, N, dh)
    a = (q @ k.transpose(-2, -1)) * dh ** -0.5
    a = a.softmax(-1)
    N = a.shape[-1]
    o = (a - torch.eye(N, dtype=a.dtype, device=a.device)) @ v          # (B, G2, H, N, dh)
    o = o.transpose(-3, -2)                                             # (B, G2, N, H, dh)
    if temporal:
        o = o.permute(0, 2, 1, 3, 4)                                    # (B, T, J, H, dh)
    return o.reshape(B * T * J, D)


# ------------------------------------------------------------------------------------------------ bench.py as a child process
_RANK_ENV = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "D3D_FORCE_DIST", "D3D_BENCH_ONE_DEVICE", "D3D_DIST_BACKEND")


def clean_env(**extra):
    """The environment without a launcher's rank variables and the benchmark's own switches, plus `extra`."""
    env = {k: v for k, v in os.environ.items() if k not in _RANK_ENV}
    env.update(extra)
    return env


def bench_subprocess(args, env, timeout=900):
    """Runs bench.py with `args`; asserts exit code 0 and exactly one JSON line on stdout, and returns it parsed."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args, capture_output=True, text=True, env=env, cwd=root,
                         timeout=timeout)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = [l for l in run.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, run.stdout[-2000:]
    return json.loads(lines[0])


def maxabs(a, b):
    return (a.detach().cpu().double() - torch.as_tensor(b).double()).abs().max().item()


# ------------------------------------------------------------------------------------------------ row isolation / guard bands
BAND_BYTES = 4096
BAND_PATTERN = 0x7FC5A5A5      # a quiet NaN as fp32; as int32 it is positive, so fill_ takes it


def _pattern_bytes(lo, hi, device):
    """The bytes lo .. hi-1 of a buffer filled with the little-endian int32 BAND_PATTERN from byte 0 on."""
    pat = torch.tensor([(BAND_PATTERN >> (8 * i)) & 0xFF for i in range(4)], dtype=torch.uint8, device=device)
    return pat[torch.arange(lo, hi, device=device) % 4]


def banded(shape, dtype=torch.float32, device="cuda"):
    """(view, check): a tensor of `shape` that starts BAND_BYTES into one uint8 buffer of BAND_BYTES + its bytes rounded up to BAND_BYTES +
    BAND_BYTES, every 32-bit word of which -- the view's own included -- holds BAND_PATTERN.  check() asserts that every byte in front of
    the view and behind it still does (the back band starts at the first byte behind the view: the padding up to the next multiple of
    BAND_BYTES is part of it); untouched(view) counts the words of the view itself that do."""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    inner = (nbytes + BAND_BYTES - 1) // BAND_BYTES * BAND_BYTES
    total = BAND_BYTES + inner + BAND_BYTES
    buf = torch.empty(total, dtype=torch.uint8, device=device)
    buf.view(torch.int32).fill_(BAND_PATTERN)
    view = buf[BAND_BYTES:BAND_BYTES + nbytes].view(dtype).view(shape)

    def check():
        for name, lo, hi in (("front", 0, BAND_BYTES), ("back", BAND_BYTES + nbytes, total)):
            bad = (buf[lo:hi] != _pattern_bytes(lo, hi, buf.device)).nonzero()
            assert bad.numel() == 0, (f"{name} band: {bad.numel()} bytes changed, the first {int(bad[0]) + lo - BAND_BYTES} bytes from the "
                                      f"view's start (the view holds {nbytes})")
    return view, check


def untouched(view):
    """How many whole 32-bit words of a banded view still hold BAND_PATTERN."""
    assert view.is_contiguous(), "untouched() counts the words of the memory the launch wrote: a contiguous view"
    b = view.reshape(-1).view(torch.uint8)
    return int((b[:b.numel() // 4 * 4].view(torch.int32) == BAND_PATTERN).sum())


def group_index(B, T, J, temporal):
    """The attention group of every token row m = (b T + t) J + j: temporal groups are (b, j) -> b J + j, spatial ones (b, t) -> b T + t."""
    m = torch.arange(B * T * J)
    return (m // (T * J)) * J + m % J if temporal else m // J


def poison_groups(x, group_index, kinds=("nan", "inf"), cols=None):
    """(poisoned copy of x, keep mask over its rows).  Every row of an odd-numbered group becomes non-finite -- kinds[0] for groups = 1
    mod 4, kinds[1] for groups = 3 mod 4 -- in all its columns, or in `cols` (a slice) only; even groups are untouched, so in any tile
    packing every clean group has poisoned neighbours on both sides."""
    value = {"nan": float("nan"), "inf": float("inf"), "-inf": float("-inf")}
    g = torch.as_tensor(group_index).to(x.device).long()
    assert g.shape == (x.shape[0],), (g.shape, x.shape)
    bad = x.clone()
    sl = slice(None) if cols is None else cols
    for rem, kind in ((1, kinds[0]), (3, kinds[1])):
        rows = (g % 4 == rem).nonzero().flatten()
        sub = bad[rows]
        sub[:, sl] = value[kind]
        bad[rows] = sub
    return bad, g % 2 == 0
