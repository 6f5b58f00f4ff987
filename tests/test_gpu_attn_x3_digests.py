"""Recorded output digests of the four compiler-scheduled F16X3 attention kernels that share csrc/attn_x3_tile.h: k_attn_temporal_x3,
k_attn_temporal_x3p, k_attn_x3_stream<64, 8> and the attention step of k_qkv_attn_x3_small.  The "form A torch.equal form B" tests compare
kernels that are built from the same pieces, so a change to a shared piece moves both sides together; these digests pin every touched
instantiation to the bits of the hand-written bodies the header replaced.

tests/golden/attn_x3_digests.json holds one SHA-256 of the output bytes per case, with the ROCm version and the commit it was recorded
on.  It was written ONCE, by experiments/attn_x3_digests.py, from the commit before the kernels were rewritten on the header; it is the
project's own recorded result, not the output of the code under test, and no change to these kernels regenerates it.  A toolchain change
that moves the digests (another contraction or instruction selection in the compiler) means re-recording them -- after the fp64 and the
form-equality tests (test_attention_core, test_attention_persistent_kernels, test_gpu_long_temporal.py, test_gpu_small_tiles.py) pass
on the new toolchain.

Inputs are hashed(...) at scale 2.0 (sharp cases: 9.0), D = 512, 8 heads, through the op hooks.  The cases are the smallest shapes that
reach every instantiation (launch_attn_temporal_x3's rules: units = B J H)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLD
from helpers import hashed
from diff3dhpe_amd.engine import op_attention, op_attention_long, op_qkv_attn_x3_small

pytestmark = pytest.mark.gpu
D, H = 512, 8
DIGESTS = os.path.join(GOLD, "attn_x3_digests.json")


def _qkv(T, B, J, scale):
    return hashed(f"dgqkv{T}_{B}_{J}", (B * T * J, 3 * D), 61, scale).cuda()


def _resident(T, B, J, scale=2.0):
    return lambda: op_attention(_qkv(T, B, J, scale), B, T, J, H, True, precision="f16x3")


def _long(T, B, J, scale=2.0):
    return lambda: op_attention_long(_qkv(T, B, J, scale), B, T, J, H)


def _small(N, stride, groups, sharp=1.0):
    """The inputs of tests/test_gpu_small_tiles.py's op test; sharp: q and k rows of the weight and bias times sqrt(sharp) (the LayerNorm
    in front of the GEMM undoes a scale of x)."""
    def run():
        x = hashed(f"stx{N}", (groups * N, D), 41, 2.0)
        W = hashed("stW", (3 * D, D), 42, 1.0 / np.sqrt(D))
        b = hashed("stb", (3 * D,), 43, 0.5)
        g = 1 + 0.2 * hashed("stg", (D,), 44)
        be = 0.2 * hashed("stbe", (D,), 45)
        W[:2 * D] *= float(np.sqrt(sharp))
        b[:2 * D] *= float(np.sqrt(sharp))
        return op_qkv_attn_x3_small(x.cuda(), W.cuda(), b.cuda(), g.cuda(), be.cuda(), 1e-6, groups, N, stride, H, stride != 1)
    return run


CASES = {}
# base kernel <NKT, 1>, NKT = 1 .. 8, with and without pad keys in the last tile (16 units: never the persistent forms)
for _T in (17, 33, 81, 100, 160, 161, 200, 243, 256):
    CASES[f"base_T{_T}"] = _resident(_T, 1, 2)
# 512 groups = 4096 units: base <1, 8> (the wave-private forms do not fit 160 KiB at 31 rows), x3p <1, 8>, x3p <1, 6, 4>
CASES["base_mu8_T31"] = _resident(31, 32, 16)
CASES["x3p_mu8_T17"] = _resident(17, 32, 16)
CASES["x3p_mu6_T27"] = _resident(27, 32, 16)
CASES["x3p_nkt3_T81"] = _resident(81, 8, 16)          # B J = 128: 1024 units
for _T in (100, 257, 300, 513):
    CASES[f"long_T{_T}"] = _long(_T, 1, 2)
CASES["long_T300_B3_J17"] = _long(300, 3, 17)
for _N, _stride, _groups in ((17, 1, 20), (27, 17, 17), (81, 17, 17), (127, 5, 5)):      # OP_CASES of tests/test_gpu_small_tiles.py
    CASES[f"small_N{_N}"] = _small(_N, _stride, _groups)
# sharp softmax: near one-hot rows, exp2 underflow on most keys
CASES["sharp_base_T81"] = _resident(81, 1, 2, 9.0)
CASES["sharp_x3p_nkt3_T81"] = _resident(81, 8, 16, 9.0)
CASES["sharp_long_T300"] = _long(300, 1, 2, 9.0)
CASES["sharp_small_N27"] = _small(27, 17, 17, 9.0)


def digest(name):
    out = CASES[name]()
    assert torch.isfinite(out).all(), name
    return hashlib.sha256(out.cpu().contiguous().numpy().tobytes()).hexdigest()


def test_every_case_is_recorded():
    with open(DIGESTS) as f:
        assert sorted(json.load(f)["sha256"]) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_output_bits_are_the_recorded_ones(name):
    with open(DIGESTS) as f:
        rec = json.load(f)
    assert digest(name) == rec["sha256"][name], (name, "recorded on", rec["commit"], "ROCm", rec["rocm"])
