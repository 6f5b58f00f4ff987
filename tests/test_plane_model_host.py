"""The plane model of tests/plane_model.py against itself, on the CPU: the floor a weight exponent k puts under an F16X3 GEMM (the numbers
the GPU tolerances of tests/test_gpu_weight_exponent.py are built from, and the justification of F16X3_MIN_WEIGHT_EXP in weight_pack.h),
and the exact scaling identity the GPU tests rely on."""
import numpy as np
import pytest

import plane_model as pm
from diff3dhpe_amd.synth import hash_uniform

# (outlier, the exponent it forces): the table of DESIGN section 4.1
TABLE = [(None, 12), (100.0, 9), (5.0e3, 3), (7.0e4, -1), (1.0e6, -4), (1.0e9, -14)]


def _operands(K, M=96, N=64):
    A = (2.0 * hash_uniform(f"pmA{K}", M * K, 31)).astype(np.float32).reshape(M, K)
    W = (hash_uniform(f"pmW{K}", N * K, 32) / np.sqrt(K)).astype(np.float32).reshape(N, K)
    return A, W


def floor_table(K):
    """{k: floor} for the table's outliers: a ~ U(-2, 2), w ~ U(+-1 / sqrt(K)), one outlier entry; max-abs distance of the three-product
    model from the exact product on the output columns that do not hold the outlier."""
    A, W0 = _operands(K)
    out = {}
    for outlier, k in TABLE:
        W = W0.copy()
        if outlier is not None:
            W[5, 7] = outlier
        assert pm.weight_exp(W) == k, (outlier, pm.weight_exp(W), k)
        out[k] = pm.floor(A, W, skip_cols=(5,))
    return out


@pytest.mark.parametrize("K", [32, 512, 2048])
def test_floor_table(K):
    t = floor_table(K)
    print(f"plane-model floor, K = {K}: " + ", ".join(f"k={k}: {v:.2e}" for k, v in t.items()))
    ks = [k for _, k in TABLE]                      # descending
    # Monotone: a lower exponent only moves more of the ordinary entries' lo halves (and then hi halves) into fp16 subnormals.  Each entry's
    # split error is bounded by max(2^-22 |w|, 2^-25 2^-k); the second term doubles with every step of k.  While the first term rules
    # (k >= 9 here) two exponents may differ either way by the luck of single roundings, far below the floor itself: 1 % slack.
    for hi_k, lo_k in zip(ks, ks[1:]):
        assert t[lo_k] >= 0.99 * t[hi_k], (hi_k, lo_k, t)
    if K == 512:
        for k in ks:
            if k >= 3:
                assert t[k] <= 3e-7, (k, t[k])
    # the bottom of the admitted range is far outside anything an "fp32-accurate" engine may return in silence
    assert t[-14] > 1e-3 * np.sqrt(K / 512)
    # the bound behind the numbers: per entry 2^-25 2^-k, K entries of |a| <= 2 (random signs: sqrt(K) growth; K as the hard bound)
    for k in ks:
        assert t[k] <= 2.0 * K * max(2.0 ** -25 * 2.0 ** -k, 2.0 ** -22 / np.sqrt(K)) + 2.0 ** -20, (k, t[k])


def test_min_weight_exp_is_the_header_constant_and_what_the_floor_allows():
    """F16X3_MIN_WEIGHT_EXP (weight_pack.h) is the model's MIN_WEIGHT_EXP, and it is the lowest exponent at which the floor stays within a
    quarter of the fp32 rounding bound the suite holds a GEMM to at k = 12, 2e-6 sqrt(K / 32) (tests/test_gpu_ops.py), at the two depths
    the engine's GEMMs have (K = embed_dim = 512 and K = mlp_hidden = 1024; a block chains four GEMMs)."""
    import os
    import re
    from diff3dhpe_amd import build as B
    m = re.search(r"constexpr int F16X3_MIN_WEIGHT_EXP\s*=\s*(-?\d+)\s*;", open(os.path.join(B.CSRC, "weight_pack.h")).read())
    assert m and int(m.group(1)) == pm.MIN_WEIGHT_EXP
    for K in (512, 1024):
        A, W0 = _operands(K)
        budget = 0.25 * 2e-6 * np.sqrt(K / 32)
        fl = {}
        for k in (pm.MIN_WEIGHT_EXP, pm.MIN_WEIGHT_EXP - 1):
            W = W0.copy()
            W[5, 7] = pm.outlier_for(k)
            assert pm.weight_exp(W) == k
            fl[k] = pm.floor(A, W, skip_cols=(5,))
        print(f"K = {K}: floor at k = {pm.MIN_WEIGHT_EXP}: {fl[pm.MIN_WEIGHT_EXP]:.2e}, one below: {fl[pm.MIN_WEIGHT_EXP - 1]:.2e}, budget {budget:.2e}")
        assert fl[pm.MIN_WEIGHT_EXP] <= budget < fl[pm.MIN_WEIGHT_EXP - 1]


def test_weight_exp_boundaries():
    for k in range(12, -15, -1):
        amax = np.float32(65504.0 * 2.0 ** -k)
        assert pm.weight_exp(np.array([0.25, -amax], dtype=np.float32)) == k
        above = np.nextafter(amax, np.float32(np.inf), dtype=np.float32)
        assert pm.weight_exp(np.array([above], dtype=np.float32)) == max(k - 1, -14)
        assert pm.weight_exp(np.array([pm.outlier_for(k)], dtype=np.float32)) == k
    assert pm.weight_exp(np.array([0.0, np.inf, np.nan, 1.0], dtype=np.float32)) == 12      # non-finite entries do not take part
    assert pm.weight_exp(np.zeros(4, dtype=np.float32)) == 12


@pytest.mark.parametrize("j", list(range(1, 27)))
def test_scaling_identity(j):
    """split(2^j W) at its own exponent 12 - j equals split(W) at 12 plane for plane: what makes op(A, 2^j W) == 2^j op(A, W) an exact
    statement about a kernel.  W holds one entry that pins amax inside (7.995, 15.99], so weight_exp(2^j W) is exactly 12 - j."""
    W = (hash_uniform("pmscale", 48 * 64, 33) / 8.0).astype(np.float32).reshape(48, 64)
    W[::5] *= np.float32(2.0 ** -17)                # lo (and hi) halves in fp16 subnormals
    W[3, 9] = -12.5
    assert pm.weight_exp(W) == 12
    Wj = (W * np.float32(2.0 ** j)).astype(np.float32)
    assert pm.weight_exp(Wj) == 12 - j
    h0, l0, _ = pm.split_weight(W)
    h1, l1, k1 = pm.split_weight(Wj)
    assert k1 == 12 - j and np.array_equal(h0, h1) and np.array_equal(l0, l1)
    A = (2.0 * hash_uniform("pmscaleA", 8 * 64, 34)).astype(np.float32).reshape(8, 64)
    assert np.array_equal(pm.gemm(A, W), pm.gemm(A, Wj))
    assert np.array_equal(pm.product(A, Wj), pm.product(A, W) * 2.0 ** j)


def test_split_planes_and_clamp():
    x = np.array([0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -12, -3.0e5, 3.0e5, 2.0 ** -26], dtype=np.float32)
    hi, lo = pm.split(x, 1.0)
    assert hi[1] == 1.0 and lo[1] == 0.0
    assert hi[2] == 1.0 and lo[2] == 2.0 ** -11          # a tie rounds to even; the rest is the lo plane's
    assert hi[3] == 1.0 and lo[3] == 2.0 ** -12
    assert hi[4] == -65504.0 and hi[5] == 65504.0 and lo[4] == 0.0 and lo[5] == 0.0
    assert hi[6] == 0.0 and lo[6] == 0.0                 # below half the smallest subnormal: gone
    hi, lo = pm.split(x[:4], 8.0)
    assert np.array_equal(hi + lo, 8.0 * x[:4].astype(np.float64))


def test_torch_form_equals_numpy_form():
    import torch
    A, W = _operands(64, M=24, N=16)
    A[3, 5] = 9000.0                     # clamped activation plane
    for outlier in (None, 5.0e3, 1.0e6, 1.0e9):
        Wk = W.copy()
        if outlier is not None:
            Wk[2, 3] = outlier
        pt, k = pm.product_t(torch.from_numpy(A), torch.from_numpy(Wk))
        assert k == pm.weight_exp(Wk)
        for a, b in zip(pm.split_t(torch.from_numpy(Wk), 2.0 ** k), pm.split(Wk, 2.0 ** k)):     # the planes: bit for bit
            assert np.array_equal(a.numpy(), b)
        assert np.allclose(pt.numpy(), pm.product(A, Wk), rtol=1e-13, atol=1e-13)               # (two BLAS: the fp64 sums' order)
    b = np.linspace(-0.5, 0.5, 16, dtype=np.float32)
    g = np.linspace(0.5, 1.5, 64, dtype=np.float32)
    be = np.linspace(-0.2, 0.2, 64, dtype=np.float32)
    ft, kt = pm.folded_linear_t(*(torch.from_numpy(v) for v in (A, W, b, g, be)), 1e-6)
    fn, kn = pm.folded_linear(A, W, b, g, be, 1e-6)
    assert kt == kn and np.abs(ft.numpy() - fn).max() <= 1e-12 * np.abs(fn).max()


def test_fold_matches_its_definition():
    N, K = 40, 64
    W = (hash_uniform("pmfW", N * K, 35) / 8.0).astype(np.float32).reshape(N, K)
    b = (0.5 * hash_uniform("pmfb", N, 36)).astype(np.float32)
    g = (1.0 + 0.5 * hash_uniform("pmfg", K, 37)).astype(np.float32)
    be = (0.3 * hash_uniform("pmfbe", K, 38)).astype(np.float32)
    x = (1.5 * hash_uniform("pmfx", 9 * K, 39) + 0.2).astype(np.float32).reshape(9, K)
    wg, csum, fb = pm.fold_layernorm(W, b, g, be)
    assert wg.dtype == np.float32 and csum.dtype == np.float32 and fb.dtype == np.float32
    assert np.array_equal(wg, W * g[None, :])
    xd = x.astype(np.float64)
    ln = (xd - xd.mean(1, keepdims=True)) / np.sqrt(xd.var(1, keepdims=True) + 1e-6) * g.astype(np.float64) + be.astype(np.float64)
    ref = ln @ W.astype(np.float64).T + b.astype(np.float64)
    got, k = pm.folded_linear(x, W, b, g, be, 1e-6)
    assert k == 12
    assert np.abs(got - ref).max() < 2e-6
