"""The attention kernel a forward runs in its spatial and in its temporal blocks, as the twelve "*_last" info keys report it: one
depth-1 engine per row of a literal table (B = 1, 17 joints, every option at its default), one forward_denoise, every key read and
compared.  The per-feature tests (test_gpu_long_temporal.py, test_gpu_attn_h32.py, test_gpu_long_h32.py, test_gpu_attn_h128.py,
test_gpu_long_h128.py) switch one option on and off; this table pins the whole plan -- every key of every row, the zeros included -- so
a change to the attention choice (csrc/attn_dispatch.hip) that moves one precedence shows here.  The values of the first ten rows were
read off plan_blocks as it stood when the plan still held one flag per feature; the library of that commit reports the same table.
Every row is also compared, in all twelve keys, with what the library reported at that shape before the plan became a table: the
recorded grid of tests/test_attention_plan_host.py (tests/golden/attention_plan_grid.npz, J = 17, default options)."""
import os

import numpy as np
import pytest
import torch

from helpers import inputs, product_with_engine
from diff3dhpe_amd.spec import DenoiserConfig

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_plan_grid.npz"))
KEYS = tuple(G["key_names"].tolist())
# (precision, embed_dim, heads, frames): the keys that are not 0.  None: the row states no values of its own, the recorded grid alone does
PLANS = [
    ("f16x3", 512, 8, 243, {}),
    ("f16x3", 512, 8, 300, {"long_temporal_last": 1}),
    ("f16x3", 256, 8, 243, {"attn_h32_last": 1}),
    ("f16x3", 256, 8, 300, {"long_temporal_h32_last": 1}),
    ("f16x3", 1024, 8, 81, {"attn_h128_last": 3}),       # bit 0 spatial, bit 1 resident temporal
    ("f16x3", 1024, 8, 243, {"attn_h128_last": 5}),      # bit 0 spatial, bit 2 streaming temporal
    ("fp32", 512, 8, 300, {"long_temporal_f32_last": 1}),
    ("fp32", 256, 8, 243, {"attn_f32_h32_last": 3}),     # bit 0 spatial, bit 1 temporal
    ("fp32", 256, 8, 300, {"attn_f32_h32_last": 1, "long_temporal_f32_h32_last": 1}),
    ("fp32", 1024, 8, 243, {"attn_f32_h128_last": 5}),   # (a key this table did not read while it held seven)
] + [(p, D, 8, T, None) for D in (384, 768, 128) for T in (27, 300) for p in ("f16x3", "fp32")] + [("fp32", 1024, 8, 300, None)]


def recorded(prec, D, H, T):
    """The twelve keys of the recorded grid at (precision, D, H, T), 17 joints, every option at its default."""
    a = G["engines"].tolist().index([{"fp32": 0, "f16x3": 1}[prec], D, H])
    o = G["optsets"].tolist().index([(1 << 12) - 1, 1])
    return dict(zip(KEYS, G["keys"][a, G["T"].tolist().index(T), G["J"].tolist().index(17), o].tolist()))


@pytest.mark.parametrize("prec,D,H,T,expected", PLANS, ids=[f"{p}_D{d}_T{t}" for p, d, _, t, _ in PLANS])
def test_the_plan_of_a_default_engine(prec, D, H, T, expected):
    want = recorded(prec, D, H, T)
    if expected is not None:                       # the literal row and the recorded grid say the same
        assert want == {**dict.fromkeys(KEYS, 0), **expected}
    cfg = DenoiserConfig(num_frame=T, embed_dim=D, depth=1, num_heads=H)
    net, _, eng = product_with_engine(cfg, 3, prec, sampling=2)
    assert {k: eng.info(k) for k in KEYS} == dict.fromkeys(KEYS, 0)      # before any forward
    inp = inputs(1, T, 500)
    out = net.forward_denoise(torch.cat([inp["x2d"], inp["noise"]], dim=-1).cuda(), torch.tensor([500]).cuda())
    assert torch.isfinite(out).all()
    assert {k: eng.info(k) for k in KEYS} == want
