"""The attention kernel a forward runs in its spatial and in its temporal blocks, as the seven "*_last" info keys report it: one
depth-1 engine per row of a literal table (B = 1, 17 joints, every option at its default), one forward_denoise, every key read and
compared.  The per-feature tests (test_gpu_long_temporal.py, test_gpu_attn_h32.py, test_gpu_long_h32.py, test_gpu_attn_h128.py,
test_gpu_long_h128.py) switch one option on and off; this table pins the whole plan -- every key of every row, the zeros included -- so
a change to plan_blocks (csrc/engine.hip) that moves one precedence shows here.  The values were read off plan_blocks as it stood when
the plan still held one flag per feature; the library of that commit reports the same table."""
import pytest
import torch

from helpers import inputs, product_with_engine
from diff3dhpe_amd.spec import DenoiserConfig

pytestmark = pytest.mark.gpu
KEYS = ("long_temporal_last", "attn_h32_last", "long_temporal_h32_last", "attn_h128_last", "long_temporal_f32_last", "attn_f32_h32_last",
        "long_temporal_f32_h32_last")
# (precision, embed_dim, heads, frames): the keys that are not 0
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
    ("fp32", 1024, 8, 243, {}),
]


@pytest.mark.parametrize("prec,D,H,T,expected", PLANS, ids=[f"{p}_D{d}_T{t}" for p, d, _, t, _ in PLANS])
def test_the_plan_of_a_default_engine(prec, D, H, T, expected):
    cfg = DenoiserConfig(num_frame=T, embed_dim=D, depth=1, num_heads=H)
    net, _, eng = product_with_engine(cfg, 3, prec, sampling=2)
    assert {k: eng.info(k) for k in KEYS} == dict.fromkeys(KEYS, 0)      # before any forward
    inp = inputs(1, T, 500)
    out = net.forward_denoise(torch.cat([inp["x2d"], inp["noise"]], dim=-1).cuda(), torch.tensor([500]).cuda())
    assert torch.isfinite(out).all()
    assert {k: eng.info(k) for k in KEYS} == {**dict.fromkeys(KEYS, 0), **expected}
