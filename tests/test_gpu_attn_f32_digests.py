"""Recorded output digests of the six exact-fp32 MFMA attention kernels that share csrc/attn_f32_tile.h: k_attn_temporal_f32<NKT>,
k_attn_temporal_f32_h32<NKT>, k_attn_f32_h128<NKT> and their key-streaming forms k_attn_f32_stream3<64>, k_attn_f32_stream3<32> and
k_attn_f32_h128_stream.  The "streaming torch.equal resident" tests compare kernels that are built from the same pieces, so a change to
a shared piece moves both sides together; these digests pin every touched instantiation to the bits of the hand-written bodies the
header replaced.

tests/golden/attn_f32_digests.json holds one SHA-256 of the output bytes per case, with the ROCm version and the commit it was recorded
on.  It was written ONCE, by experiments/attn_x3_digests.py --cases test_gpu_attn_f32_digests, from the commit before the kernels were
rewritten on the header; it is the project's own recorded result, not the output of the code under test, and no change to these kernels
regenerates it.  A toolchain change that moves the digests (another contraction or instruction selection in the compiler) means
re-recording them -- after the fp64 and the form-equality tests (test_gpu_long_temporal_f32.py, test_gpu_long_f32_h32.py,
test_gpu_attn_f32_h32.py, test_gpu_attn_f32_h128.py, test_gpu_group_lengths.py) pass on the new toolchain.

Inputs are hashed(...) at scale 2.0 (sharp cases: 9.0), two heads (D = 2 DH), B = 1 and J = 2 unless the case says otherwise, through
the op hooks.  The cases are the smallest shapes that reach every instantiation and every branch: NKT = 1 .. 8 (1 .. 4 at width 128) with
full and ragged last key tiles, one spatial grouping at width 128; streaming: one chunk, one key in the second chunk, a full last tile,
two query blocks of 5 waves, three chunks with three blocks of 6 waves (chunks of 256 keys, 128 at width 128)."""
import hashlib
import json
import os

import pytest
import torch

from conftest import GOLD
from helpers import hashed
from diff3dhpe_amd.engine import (op_attention, op_attention_f32_h32, op_attention_f32_h128, op_attention_long_f32,
                                  op_attention_long_f32_h32, op_attention_long_f32_h128)

pytestmark = pytest.mark.gpu
H = 2
DIGESTS = os.path.join(GOLD, "attn_f32_digests.json")


def _qkv(DH, T, B, J, scale):
    return hashed(f"dgf32qkv{DH}_{T}_{B}_{J}", (B * T * J, 3 * H * DH), 67, scale).cuda()


def _resident(DH, T, B=1, J=2, scale=2.0, temporal=True):
    def run():
        qkv = _qkv(DH, T, B, J, scale)
        if DH == 64:
            return op_attention(qkv, B, T, J, H, temporal)
        return {32: op_attention_f32_h32, 128: op_attention_f32_h128}[DH](qkv, B, T, J, H, temporal)
    return run


def _long(DH, T, B=1, J=2, scale=2.0):
    op = {64: op_attention_long_f32, 32: op_attention_long_f32_h32, 128: op_attention_long_f32_h128}[DH]
    return lambda: op(_qkv(DH, T, B, J, scale), B, T, J, H)


CASES = {}
for _DH in (32, 64):
    # resident <NKT>, NKT = 1 .. 8: ragged last tiles, and full ones at T = 64 and 256 (width 32: the rounded-product form without a pad key)
    for _T in (17, 33, 64, 81, 100, 160, 161, 200, 243, 256):
        CASES[f"w{_DH}_T{_T}"] = _resident(_DH, _T)
    for _T in (100, 256, 257, 288, 300, 513):
        CASES[f"w{_DH}_long_T{_T}"] = _long(_DH, _T)
    CASES[f"w{_DH}_long_T300_B3_J17"] = _long(_DH, 300, 3, 17)
    # sharp softmax: near one-hot rows, expf underflow on most keys
    CASES[f"sharp_w{_DH}_T243"] = _resident(_DH, 243, scale=9.0)
    CASES[f"sharp_w{_DH}_long_T300"] = _long(_DH, 300, scale=9.0)
for _T in (17, 33, 64, 81, 100, 128):
    CASES[f"w128_T{_T}"] = _resident(128, _T)
CASES["w128_spatial_B2_T5_J17"] = _resident(128, 5, 2, 17, temporal=False)
for _T in (100, 128, 129, 257, 300, 513):
    CASES[f"w128_long_T{_T}"] = _long(128, _T)
CASES["w128_long_T300_B3_J17"] = _long(128, 300, 3, 17)
CASES["sharp_w128_T100"] = _resident(128, 100, scale=9.0)
CASES["sharp_w128_long_T300"] = _long(128, 300, scale=9.0)


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
