"""Recorded output digests of the key-streaming F16X3 attention at head widths 32 and 128 (csrc/kernels_attn_x3_long.hip), beyond the
window lengths their resident twins reach: test_gpu_long_h32.py and test_gpu_long_h128.py pin them bit for bit to k_attn_x3_h32 up to
256 frames and to k_attn_x3_h128 up to 128, and check longer windows against fp64 within a tolerance, which a reordered sum would pass.
The 64-wide streaming kernel has its digests in test_gpu_attn_x3_digests.py.

tests/golden/attn_x3_width_digests.json holds one SHA-256 of the output bytes per case, with the ROCm version and the commit it was
recorded on.  It was written ONCE, by experiments/attn_x3_digests.py --cases test_gpu_attn_x3_width_digests, from the commit before the
three streaming kernels became one template; it is the project's own recorded result, not the output of the code under test, and no
change to these kernels regenerates it.  A toolchain change that moves the digests (another contraction or instruction selection in the
compiler) means re-recording them -- after the fp64 and the form-equality tests (test_gpu_long_h32.py, test_gpu_long_h128.py) pass on
the new toolchain.

Inputs are hashed(...) at scale 2.0 (sharp cases: 9.0), through the op hooks.  The cases are the smallest shapes that reach each regime:
width 32 at D = 256 with 8 heads (four head pairs, chunks of 256 keys), width 128 at D = 256 with 2 heads (chunks of 128 keys) and once
at D = 1024 with 8; a query block is at most 256 queries."""
import hashlib
import json
import os

import pytest
import torch

from conftest import GOLD
from helpers import hashed
from diff3dhpe_amd.engine import op_attention_long_h32, op_attention_long_h128

pytestmark = pytest.mark.gpu
DIGESTS = os.path.join(GOLD, "attn_x3_width_digests.json")


def _case(op, D, H, T, B, J, scale=2.0):
    return lambda: op(hashed(f"wdqkv{D}_{T}_{B}_{J}", (B * T * J, 3 * D), 61, scale).cuda(), B, T, J, H)


CASES = {}
# width 32: 257 = a second chunk of one key and a second query block, 513 = three query blocks and a third chunk
for _T in (100, 257, 300, 513):
    CASES[f"h32_T{_T}"] = _case(op_attention_long_h32, 256, 8, _T, 1, 2)
CASES["h32_T300_B3_J17"] = _case(op_attention_long_h32, 256, 8, 300, 3, 17)
CASES["sharp_h32_T300"] = _case(op_attention_long_h32, 256, 8, 300, 1, 2, 9.0)
# width 128: 129 = one key in the second chunk, 257 = a third chunk and a second query block, 513 = a fifth chunk and three query blocks
for _T in (100, 129, 257, 300, 513):
    CASES[f"h128_T{_T}"] = _case(op_attention_long_h128, 256, 2, _T, 1, 2)
CASES["h128_T300_B3_J17"] = _case(op_attention_long_h128, 256, 2, 300, 3, 17)
CASES["h128_D1024_T300"] = _case(op_attention_long_h128, 1024, 8, 300, 1, 2)
CASES["sharp_h128_T300"] = _case(op_attention_long_h128, 256, 2, 300, 1, 2, 9.0)


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
