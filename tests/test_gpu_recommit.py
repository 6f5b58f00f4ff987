"""Re-commit: loading a second state dict into a module whose engine has already run frees and rebuilds every resident weight image of
that engine (d3d_engine_commit_weights on a committed engine).  The engine must then compute exactly what a fresh engine built from the
second state dict computes, and keep no captured graph of the first."""
import pytest
import torch

from diff3dhpe_amd.spec import DenoiserConfig
from helpers import build_product, inputs, torch_sd

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("precision", ["f16x3", "bf16", "fp32"])
def test_recommit_equals_a_fresh_engine_and_drops_the_graphs(precision):
    # D = 512, H = 8, J = 17, T = 9, one spatial + one temporal block: in F16X3 both tile-order copies and the block-0 tables exist
    cfg = DenoiserConfig(num_frame=9, embed_dim=512, depth=1)
    dev = torch.device("cuda", torch.cuda.current_device())
    inp = inputs(1, 9, 31)
    x2d, nz = inp["x2d"].cuda(), inp["noise"].cuda()
    net, diff = build_product(cfg, 5, sampling=2, precision=precision)
    eng = diff._engine(dev)
    eng.set_graph_mode(True)
    try:
        ya = eng.ddim_sample(x2d, nz).clone()
        assert eng.info("graphs_cached") >= 1
        net.load_state_dict(torch_sd(cfg, 6), strict=True)
        assert diff._engine(dev) is eng                      # the same engine, committed again
        assert eng.info("graphs_cached") == 0
        yb = eng.ddim_sample(x2d, nz).clone()
    finally:
        eng.set_graph_mode(False)
    _, fresh = build_product(cfg, 6, sampling=2, precision=precision)
    yf = fresh._engine(dev).ddim_sample(x2d, nz)
    assert torch.equal(yb, yf)
    assert not torch.equal(ya, yb)                           # (the two state dicts do differ)
    assert torch.equal(eng.ddim_sample(x2d, nz), yf)         # and eagerly, on the re-committed engine
