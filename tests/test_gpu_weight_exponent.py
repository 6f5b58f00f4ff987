"""The per-matrix weight exponent of the F16X3 planes (split_weight_f16x3: planes of 2^k w, k = 12 for |w| <= 15.99, lower for larger weights,
down to -14) through every GEMM launcher that takes it, on the MI355X.  Each kernel undoes the exponent with out_scale = 2^-(3 + k); every
other test of the suite runs at k = 12 (9 .. 11 for the folded matrices of the trained-like family).

  (a) exact scaling      op(A, 2^j W, 2^j b, 2^j R) == 2^j op(A, W, b, R), torch.equal: the planes of 2^j W are those of W (only k moves) and a
                         power of two commutes with every rounding of a linear epilogue.  Catches a wrong exponent, a scaled bias / residual.
  (b) dead input         A[:, k0] = 0 and W[n0, k0] = an outlier that forces k: the exact result does not contain the outlier, only k changes.
                         Against the plane model (tests/plane_model.py) at the tolerance the k = 12 test of that hook uses, whatever k -- the
                         kernel has to follow its model --, and against fp64 at that tolerance plus the model's own floor at this k.
  (c) live outliers      A[:, k0] not zeroed: the outlier's column relative to its own size, the other columns as in (b).  The product of the
                         outlier and an activation has to stay below the activation guard (8188) where it lands in planes again, which limits
                         these cases to k >= 5: the outlier of k = 3 is 6141, times any activation above 1.33.
  engine                 depth 1, forward_denoise against oracle/d3d_oracle.py in fp64 on doctored checkpoints, every flow of the block loop.

Exponents under test: 12, 11, 9, 5, 3, 0, -4, -14.  Below F16X3_MIN_WEIGHT_EXP the commit refuses a matrix (D3D_RANGE_WEIGHT): the op hooks,
which do not go through the commit, still run every exponent, the engine cases run the admitted ones and pin the refusal of the others."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import plane_model as pm
from helpers import hashed, inputs
from test_gpu_ops import _rows          # (row counts per launcher rung from its _ROWS table, resolved by CU count)
from diff3dhpe_amd.spec import DenoiserConfig
from diff3dhpe_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu

GATE = 1e-4
EXPS = (12, 11, 9, 5, 3, 0, -4, -14)
LIVE_EXPS = (12, 11, 9, 5)
MIN_EXP = pm.MIN_WEIGHT_EXP      # F16X3_MIN_WEIGHT_EXP of weight_pack.h (pinned to the header by tests/test_plane_model_host.py)


def _E():
    from diff3dhpe_amd import engine
    return engine


def _lib():
    from diff3dhpe_amd import _lib
    return _lib


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _d(a, b):
    """max |a - b| in fp64 on a's device (helpers.maxabs goes through the host: seconds for the 10^5-row rungs)."""
    return (a.double() - torch.as_tensor(b).to(a.device).double()).abs().max().item()


def _errs_clear():
    """The hooks leave no error state: the device has no pending error and the stream is idle."""
    torch.cuda.synchronize()


_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _CACHE.clear()


def _operands(M, N, K):
    """A at scale 2, W at 1 / sqrt(K), b at 0.5, R at 1 from `hashed`, as tests/test_gpu_ops.py; cached per shape (the big ones take seconds)."""
    key = (M, N, K)
    if key not in _CACHE:
        _CACHE[key] = (hashed(f"weA{M}_{K}", (M, K), 11, 2.0).cuda(), hashed(f"weW{N}_{K}", (N, K), 12, 1.0 / np.sqrt(K)).cuda(),
                       hashed(f"web{N}", (N,), 13, 0.5).cuda(), hashed(f"weR{M}_{N}", (M, N), 14, 1.0).cuda())
    return _CACHE[key]


def _wexp(W):
    return pm.weight_exp(W.detach().cpu().numpy())


# ================================================================================================ (a) exact scaling
# (name, M, N, K, variant): variant 4 = 256 x 128 tiles, 13 = 256 x 256 tiles, one workgroup per tile; 0 = the launcher's own ladder
LINEAR_FORMS = [("variant4", 129, 132, 96, 4), ("variant13", 300, 256, 64, 13), ("auto_128x128", 128, 128, 32, 0),
                ("auto_256x128_ragged", 300, 96, 32, 0), ("auto_256x128_ragged3", 129, 132, 96, 0), ("auto_walk", "walk256", 512, 512, 0),
                ("auto_big_odd_ktiles", "walk256", 512, 96, 0)]


def _pinned(W):
    """W with one entry at -12.5: amax inside (7.995, 15.99], so 2^j W has exponent exactly 12 - j."""
    W = W.clone()
    W[W.shape[0] // 3, W.shape[1] // 2] = -12.5
    return W


@pytest.mark.parametrize("name,M,N,K,variant", LINEAR_FORMS, ids=[f[0] for f in LINEAR_FORMS])
def test_exact_scaling_linear(name, M, N, K, variant):
    E = _E()
    M = _rows(M)
    A, W, b, R = _operands(M, N, K)
    W = _pinned(W)
    assert _wexp(W) == 12

    def run(W, b, R, epi):
        kw = dict(bias=b if epi != "none" else None, residual=R if epi == "residual" else None, epi="residual" if epi == "residual" else "none",
                  precision="f16x3")
        return E.op_linear(A, W, **kw) if variant == 0 else E.op_linear_bench(A, W, variant=variant, reps=1, **kw)[0]
    for epi in ("none", "bias", "residual"):
        base = run(W, b, R, epi)
        ref = A.double() @ W.double().t() + (b.double() if epi != "none" else 0) + (R.double() if epi == "residual" else 0)
        e = _d(base, ref)
        print(f"exact scaling [{name}] M={M} N={N} K={K} {epi}: k=12 vs fp64 {e:.3e}")
        assert e < 2e-6 * np.sqrt(K / 32) + 3e-6 * 12.5 * 2, e          # (the pinned entry's column is O(25): its relative share on top)
        for k in EXPS[1:]:
            s = 2.0 ** (12 - k)
            Wk = W * s
            assert _wexp(Wk) == k
            got = run(Wk, b * s, R * s, epi)
            assert torch.equal(got, base * s), (name, epi, k, _d(got / s, base))
    _errs_clear()


def _splitk_partials(kind, A, W, b, R, S, g=None, be=None):
    """The fp32 partials [S][M][N] the split-K GEMM of a hook hands back, through the C ABI (the Python wrappers keep the buffer)."""
    L, lib = _lib().lib(), _lib()
    M, K = A.shape
    N = W.shape[0]
    part = torch.full((S, M, N), float("nan"), device="cuda")
    y = torch.empty((M, N), device="cuda")
    ms = C.c_float(0.0)
    if kind == "residual":
        lib.check(L.d3d_op_linear_splitk_residual(_p(A), _p(W), _p(b), _p(R), _p(y), None, M, N, K, S, _p(part), 1, C.byref(ms), _st()))
    else:
        lib.check(L.d3d_op_linear_splitk_postnorm(_p(A), _p(W), _p(b), _p(R), _p(g), _p(be), 1e-6, None, 1, 1, None, 0, 1, _p(y), None, M, N, K, S,
                                                  _p(part), 1, C.byref(ms), _st()))
    return part, y


@pytest.mark.parametrize("M", [17, 128, 300])
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("kind", ["residual", "postnorm"])
def test_exact_scaling_splitk_partials(kind, S, M):
    N, K = 512, 512
    A, W, b, R = _operands(M, N, K)
    W = _pinned(W)
    g, be = (1 + 0.2 * hashed("weg", (N,), 25)).cuda(), (0.2 * hashed("webe", (N,), 26)).cuda()
    base, _ = _splitk_partials(kind, A, W, b, R, S, g, be)
    assert torch.isfinite(base).all()
    e = _d(base.double().sum(0), (A.double() @ W.double().t()))
    print(f"split-K partials [{kind}] S={S} M={M}: sum of the partials vs fp64 {e:.3e}")
    assert e < 3e-6 * np.sqrt(K / 32) + 3e-6 * 25, e
    for k in EXPS[1:]:
        s = 2.0 ** (12 - k)
        got, _ = _splitk_partials(kind, A, W * s, b * s, R * s, S, g, be)
        assert torch.equal(got, base * s), (kind, S, M, k)
    _errs_clear()


def test_on_the_fly_kernel_refuses_other_exponents():
    """N % 4 != 0 goes to the on-the-fly kernel, whose un-scaling is the constant 2^-15: an error for k != 12, numbers for k = 12."""
    from diff3dhpe_amd import D3DError
    E = _E()
    A, W, b, _ = _operands(129, 130, 96)
    ref = A.double() @ W.double().t() + b.double()
    assert _d(E.op_linear(A, W, b, precision="f16x3"), ref) < 2e-6 * np.sqrt(96 / 32)
    for k in EXPS[1:]:
        Wk = W.clone()
        Wk[7, 9] = pm.outlier_for(k)
        assert _wexp(Wk) == k
        with pytest.raises(D3DError):
            E.op_linear(A, Wk, b, precision="f16x3")
    _errs_clear()


# ================================================================================================ (b) dead input
def _dead(A, W, k, n0, k0, live=False):
    """(A, W) with W[n0, k0] = the outlier of exponent k and, unless live, A[:, k0] = 0."""
    A, W = A.clone(), W.clone()
    if not live:
        A[:, k0] = 0.0
    W[n0, k0] = pm.outlier_for(k)
    assert _wexp(W) == k
    return A, W


def _two_sided(got, model, exact, tol, what):
    """The two assertions of (b): the kernel follows its model at the k = 12 tolerance; fp64 is within that plus the model's own floor."""
    d_model, d_exact, floor = _d(got, model), _d(got, exact), _d(model, exact)
    print(f"{what}: vs plane model {d_model:.3e} (tol {tol:.3e}), vs fp64 {d_exact:.3e} (tol + model floor {floor:.3e})")
    assert d_model < tol, (what, d_model, tol)
    assert d_exact < tol + floor, (what, d_exact, tol, floor)
    return d_model, d_exact, floor


@pytest.mark.parametrize("M,N,K", [(129, 132, 96), (300, 512, 512), ("walk256", 512, 512)])
def test_dead_input_linear_gelu(M, N, K):
    E = _E()
    M = _rows(M)
    A0, W0, b, _ = _operands(M, N, K)
    tol = 2e-6 * np.sqrt(K / 32)                               # test_linear_matches_fp64
    for k in EXPS:
        A, W = _dead(A0, W0, k, N // 3, K // 2)
        model, km = pm.product_t(A, W)
        assert km == k
        exact = A.double() @ W.double().t()
        got = E.op_linear(A, W, b, epi="gelu", precision="f16x3")
        _two_sided(got, F.gelu(model + b.double()), F.gelu(exact + b.double()), tol, f"dead input, linear + gelu M={M} N={N} K={K} k={k}")
    _errs_clear()


def _row_classes(M, N, mode):
    rows = torch.arange(M, device="cuda")
    kw, add = {}, torch.zeros((M, N), dtype=torch.float64, device="cuda")
    if mode in ("pos", "all"):
        pos = hashed("wepos", (9, N), 27, 0.5).cuda()
        kw.update(pos=pos, pos_div=17)
        add += pos.double()[(rows // 17) % 9]
    if mode in ("tvecrows", "all"):
        rpb = 51
        tv = hashed("wetvr", ((M + rpb - 1) // rpb, N), 29, 0.5).cuda()
        kw.update(tvec=tv, rows_per_batch=rpb)
        add += tv.double()[rows // rpb] if tv.shape[0] > 1 else tv.double()[0]
    return kw, add


def _postnorm_operands(M, K):
    N = 512
    A, W, b, _ = _operands(M, N, K)
    key = ("pn", M)
    if key not in _CACHE:
        _CACHE[key] = (hashed(f"wepnR{M}", (M, N), 24, 1.5) + 0.3).cuda()
    g, be = (1 + 0.2 * hashed("weg", (N,), 25)).cuda(), (0.2 * hashed("webe", (N,), 26)).cuda()
    return A, W, b, _CACHE[key], g, be


# the 64-row tiles, the 128-row one-tile-per-workgroup form, the persistent walk; K = 32 and 2048; pos and per-row tvec
POSTNORM_CASES = [(17, 512, "all"), ("rows128", 512, "plain"), ("rowswalk", 512, "tvecrows"), (17, 32, "all"), (128, 2048, "plain"), (300, 512, "pos")]


@pytest.mark.parametrize("M,K,mode", POSTNORM_CASES)
def test_dead_input_postnorm(M, K, mode):
    E = _E()
    N = 512
    M = _rows(M)
    A0, W0, b, R, g, be = _postnorm_operands(M, K)
    kw, add = _row_classes(M, N, mode)
    tol = 3e-6 * np.sqrt(K / 32) + 2e-6                        # test_linear_postnorm_matches_fp64
    ln = lambda acc: F.layer_norm(R.double() + acc + b.double(), (N,), g.double(), be.double(), 1e-6) + add
    for k in EXPS:
        A, W = _dead(A0, W0, k, N // 3, K // 2)
        model, km = pm.product_t(A, W)
        assert km == k
        ym, ye = ln(model), ln(A.double() @ W.double().t())
        what = f"dead input, post-norm M={M} K={K} [{mode}] k={k}"
        y32, _, _ = E.op_linear_postnorm(A, W, b, R, g, be, 1e-6, **kw)
        _two_sided(y32, ym, ye, tol, what + " fp32 form")
        yp, st, _ = E.op_linear_postnorm(A, W, b, R, g, be, 1e-6, with_stats=True, **kw)
        _two_sided(yp, ym, ye, tol + 2e-6, what + " plane form")                     # planes hold 22 bits of y
        assert _d(yp, y32) < 2e-6
        es, eq = _d(st[:, 0], ym.sum(1)), _d(st[:, 1], (ym * ym).sum(1))
        print(f"{what}: stats vs model {es:.3e} {eq:.3e}")
        assert es < 2e-3 and eq < 1e-2
    _errs_clear()


@pytest.mark.parametrize("M", [17, 300])
@pytest.mark.parametrize("S", [2, 4])
def test_dead_input_splitk_postnorm(S, M):
    E = _E()
    N, K = 512, 1024
    A0, W0, b, R, g, be = _postnorm_operands(M, K)
    kw, add = _row_classes(M, N, "all")
    tol = 3e-6 * np.sqrt(K / 32) + 2e-6                        # test_splitk_postnorm_matches_fp64
    ln = lambda acc: F.layer_norm(R.double() + acc + b.double(), (N,), g.double(), be.double(), 1e-6) + add
    for k in EXPS:
        A, W = _dead(A0, W0, k, N // 3, K // 2)
        model, _ = pm.product_t(A, W)
        ym, ye = ln(model), ln(A.double() @ W.double().t())
        what = f"dead input, split-K post-norm S={S} M={M} k={k}"
        y32, _, _ = E.op_linear_splitk_postnorm(A, W, b, R, g, be, 1e-6, S=S, **kw)
        _two_sided(y32, ym, ye, tol, what + " fp32 form")
        yp, st, _ = E.op_linear_splitk_postnorm(A, W, b, R, g, be, 1e-6, S=S, with_stats=True, **kw)
        _two_sided(yp, ym, ye, tol + 2e-6, what + " plane form")
        es, eq = _d(st[:, 0], ym.sum(1)), _d(st[:, 1], (ym * ym).sum(1))
        assert es < 2e-3 and eq < 1e-2, (what, es, eq)
    _errs_clear()


@pytest.mark.parametrize("M", [17, 300])
@pytest.mark.parametrize("S", [0, 2, 4])
def test_dead_input_splitk_residual(S, M):
    E = _E()
    N, K = 512, 512
    A0, W0, b, R, _, _ = _postnorm_operands(M, K)
    tol = 3e-6 * np.sqrt(K / 32) + 2e-6 + 2e-6                 # test_splitk_residual_matches_fp64 (planes)
    for k in EXPS:
        A, W = _dead(A0, W0, k, N // 3, K // 2)
        model, _ = pm.product_t(A, W)
        xm, xe = R.double() + model + b.double(), R.double() + A.double() @ W.double().t() + b.double()
        x, st, _ = E.op_linear_splitk_residual(A, W, b, R, S=S, with_stats=True)
        _two_sided(x, xm, xe, tol, f"dead input, split-K residual S={S} M={M} k={k}")
        blocks = xm.view(M, N // 64, 64)
        es, eq = _d(st[:, :, 0], blocks.sum(2)), _d(st[:, :, 1], (blocks * blocks).sum(2))
        assert es < 2e-3 and eq < 1e-2, (S, M, k, es, eq)
    _errs_clear()


# ================================================================================================ (c) live outliers
def _outlier_column(got, exact, n0, what, floor=2e-8):
    scale = exact[:, n0].abs().max().item()
    e = _d(got[:, n0], exact[:, n0])
    print(f"{what}: outlier column |max| {scale:.3e}, error {e:.3e} (bound {3e-6 * scale + floor:.3e})")
    assert e < 3e-6 * scale + floor, (what, e, scale)           # the rule of test_linear_f16x3_dynamic_range


@pytest.mark.parametrize("M,N,K", [(300, 512, 512), (129, 132, 96)])
def test_live_outlier_linear(M, N, K):
    E = _E()
    A0, W0, b, _ = _operands(M, N, K)
    n0 = N // 3
    others = [n for n in range(N) if n != n0]
    tol = 2e-6 * np.sqrt(K / 32)
    for k in LIVE_EXPS:
        A, W = _dead(A0, W0, k, n0, K // 2, live=True)
        assert (A[:, K // 2].abs().max() * pm.outlier_for(k)).item() < 8188
        model, _ = pm.product_t(A, W)
        exact = A.double() @ W.double().t()
        got = E.op_linear(A, W, None, precision="f16x3")
        what = f"live outlier, linear M={M} N={N} K={K} k={k}"
        _outlier_column(got, exact, n0, what)
        _two_sided(got[:, others], model[:, others], exact[:, others], tol, what + " other columns")
    _errs_clear()


@pytest.mark.parametrize("where", ["W", "gamma"])
@pytest.mark.parametrize("S", [0, 2, 4])
def test_live_outlier_folded_gelu(S, where):
    """fc1 with the LayerNorm folded in: the planes are those of W diag(gamma), so an outlier of gamma raises a whole column of them."""
    E = _E()
    M, N, K = 300, 1024, 512
    X, W0, b, _ = _operands(M, N, K)
    g0, be = (1 + 0.2 * hashed("wefg", (K,), 25)).cuda(), (0.2 * hashed("wefbe", (K,), 26)).cuda()
    n0, k0 = N // 3, K // 2
    tol = 3e-6 * np.sqrt(K / 32) + 2e-6 + 2e-6                 # test_splitk_gelu_matches_fp64
    for k in LIVE_EXPS:
        W, g = W0.clone(), g0.clone()
        if where == "W":
            W[n0, k0] = pm.outlier_for(k) / g[k0].item()
        else:
            g[k0] = pm.outlier_for(k) / W[:, k0].abs().max().item()
        model, km = pm.folded_linear_t(X, W, b, g, be, 1e-6)
        assert km == k, (km, k)
        pre = F.layer_norm(X.double(), (K,), g.double(), be.double(), 1e-6) @ W.double().t() + b.double()
        assert pre.abs().max().item() < 8188                    # the hidden activation's planes stay inside the guard
        exact, hm = F.gelu(pre), F.gelu(model)
        h, _ = E.op_linear_splitk_gelu(X, W, b, g, be, 1e-6, S=S)
        what = f"live outlier in {where}, folded fc1 S={S} k={k}"
        if where == "W":
            others = [n for n in range(N) if n != n0]
            _outlier_column(h, exact, n0, what, floor=tol)
            _two_sided(h[:, others], hm[:, others], exact[:, others], tol, what + " other columns")
        else:                                                   # every column holds the outlier
            scale = exact.abs().max().item()
            e = _d(h, exact)
            print(f"{what}: |max| {scale:.3e}, error {e:.3e} (bound {3e-6 * scale + tol:.3e}), vs plane model {_d(h, hm):.3e}")
            assert e < 3e-6 * scale + tol, (what, e)
    _errs_clear()


def _fp64_qkv_attention(x, W, b, g, be, eps, groups, N, stride, H=8):
    D = x.shape[1]
    qkv = F.layer_norm(x.double(), (D,), g.double(), be.double(), eps) @ W.double().t() + b.double()
    u, tt = torch.arange(groups), torch.arange(N)
    idx = ((u // stride) * N * stride + u % stride)[:, None] + tt[None, :] * stride
    x3 = qkv[idx]
    q, k, v = [x3[..., i * D:(i + 1) * D].reshape(groups, N, H, D // H).transpose(1, 2) for i in range(3)]
    p = ((q * (D // H) ** -0.5) @ k.transpose(-1, -2)).softmax(-1) - torch.eye(N, dtype=torch.float64)
    out = torch.empty(groups * N, D, dtype=torch.float64)
    out[idx] = (p @ v).transpose(1, 2).reshape(groups, N, D)
    return out, qkv


@pytest.mark.parametrize("N,stride,groups", [(17, 1, 20), (27, 3, 6)])
def test_live_outlier_qkv_attention_small(N, stride, groups):
    """The fused qkv + attention kernel of "small_tiles" (folded qkv planes in tile order, their exponent from tile_order_copy): the outlier
    sits in a V row, so the logits -- and the softmax -- are those of the clean weights and one output column carries it.  The other
    columns by the rule of tests/test_gpu_small_tiles.py (1.5 x the error of the two-kernel ops on the same input), which at k < 12 the
    clean input sets: those columns' exact values do not change."""
    E = _E()
    D, H = 512, 8
    rows = groups * N
    temporal = stride != 1
    x = hashed(f"wesx{N}", (rows, D), 41, 2.0)
    W0 = hashed("wesW", (3 * D, D), 42, 1.0 / np.sqrt(D))
    b = hashed("wesb", (3 * D,), 43, 0.5)
    g = 1 + 0.2 * hashed("wesg", (D,), 44)
    be = 0.2 * hashed("wesbe", (D,), 45)
    c0, q0 = 150, 260
    others = [n for n in range(D) if n != c0]
    e_two_clean = None
    for k in LIVE_EXPS:
        W = W0.clone()
        W[2 * D + c0, q0] = pm.outlier_for(k) / g[q0].item()
        assert pm.weight_exp((W * g[None, :]).numpy()) == k
        ref, qkv = _fp64_qkv_attention(x, W, b, g, be, 1e-6, groups, N, stride)
        assert 2 * qkv.abs().max().item() < 8188                # v and (softmax - I) v stay inside the activation guard
        got = E.op_qkv_attn_x3_small(x.cuda(), W.cuda(), b.cuda(), g.cuda(), be.cuda(), 1e-6, groups, N, stride, H, temporal)
        two = E.op_attention(E.op_linear(E.op_layernorm(x.cuda(), g.cuda(), be.cuda(), 1e-6), W.cuda(), b.cuda(), precision="f16x3"),
                             groups // stride, N, stride, H, True, precision="f16x3")
        e_small, e_two = _d(got[:, others], ref[:, others]), _d(two[:, others], ref[:, others])
        if k == 12:
            e_two_clean = e_two
        what = f"live outlier in a V row, small-tile qkv + attention N={N} stride={stride} k={k}"
        print(f"{what}: other columns {e_small:.3e}, two-kernel ops {e_two:.3e} (at k = 12: {e_two_clean:.3e})")
        assert torch.isfinite(got).all()
        assert e_small <= 1.5 * e_two_clean, (what, e_small, e_two_clean)
        _outlier_column(got, ref, c0, what, floor=5e-6)         # 5e-6: test_attention_core's absolute bound
    _errs_clear()


# ================================================================================================ engine level
PFX = ("STEblocks.0", "TTEblocks.0")
MATS = ("qkv_e", "proj_e", "fc1_e", "fc2_e", "qkv_fe", "fc1_fe")


def _sd(cfg, seed=8):   # clones: _doctor writes into the tensors, and numpy's buffers behind torch_sd are shared
    return {k: torch.from_numpy(v).clone() for k, v in synth_state_dict(cfg, seed).items()}


def _doctor(sd, D, Dm, dead=None, live=None):
    """The checkpoint with the inputs of the outlier entries made exactly zero (always: the "clean" model is this with no outlier), the dead
    outliers {matrix: k} and the live ones {matrix: k} placed, in the spatial and in the temporal block.
      proj_e   a proj column <- the matching V row of qkv.weight / qkv.bias zeroed: that attention output channel is (softmax - I) 0
      fc2_e    an fc2 column <- the fc1 row zeroed, its bias -40: GELU gives 0
      qkv_e    a qkv column  <- gamma = beta = 0 at that channel of norm1 (the plain flow's LayerNorm output is 0 there; folded, the entry is 0)
      fc1_e    an fc1 column <- the same in norm2
      qkv_fe   (live) a V row entry; the proj column of that channel zeroed, so the large channel ends there
      fc1_fe   (live) an fc1 row entry; the fc2 column of that hidden unit zeroed"""
    dead, live = dead or {}, live or {}
    cp, hf, cq, cf, cv, qv, hl, ql = 37 % D, 55 % Dm, 200 % D, 211 % D, 150 % D, 101 % D, 300 % Dm, 33 % D
    for p in PFX:
        qw, qb, pw = sd[p + ".attn.qkv.weight"], sd[p + ".attn.qkv.bias"], sd[p + ".attn.proj.weight"]
        f1w, f1b, f2w = sd[p + ".mlp.fc1.weight"], sd[p + ".mlp.fc1.bias"], sd[p + ".mlp.fc2.weight"]
        qw[2 * D + cp, :] = 0.0; qb[2 * D + cp] = 0.0
        f1w[hf, :] = 0.0; f1b[hf] = -40.0
        for n, c in ((".norm1", cq), (".norm2", cf)):
            sd[p + n + ".weight"][c] = 0.0; sd[p + n + ".bias"][c] = 0.0
        pw[:, cv] = 0.0
        f2w[:, hl] = 0.0
        pw[101 % D, cp] = pm.outlier_for(dead["proj_e"]) if "proj_e" in dead else 0.0
        f2w[77 % D, hf] = -pm.outlier_for(dead["fc2_e"]) if "fc2_e" in dead else 0.0
        qw[D + 7, cq] = pm.outlier_for(dead["qkv_e"]) if "qkv_e" in dead else 0.0
        f1w[600 % Dm, cf] = -pm.outlier_for(dead["fc1_e"]) if "fc1_e" in dead else 0.0
        # live: the lower end of the exponent's interval of amax (1.02 x), on the folded value W gamma
        if "qkv_fe" in live:
            qw[2 * D + cv, qv] = 1.02 * 0.5 * 65504.0 * 2.0 ** -live["qkv_fe"] / sd[p + ".norm1.weight"][qv].item()
        if "fc1_fe" in live:
            f1w[hl, ql] = 1.02 * 0.5 * 65504.0 * 2.0 ** -live["fc1_fe"] / sd[p + ".norm2.weight"][ql].item()
    return sd


def _expected_exponents(sd, p):
    n = lambda t: t.numpy()
    qw, f1w = n(sd[p + ".attn.qkv.weight"]), n(sd[p + ".mlp.fc1.weight"])
    return {"qkv_e": pm.weight_exp(qw), "proj_e": pm.weight_exp(n(sd[p + ".attn.proj.weight"])), "fc1_e": pm.weight_exp(f1w),
            "fc2_e": pm.weight_exp(n(sd[p + ".mlp.fc2.weight"])),
            "qkv_fe": pm.weight_exp(pm.fold_layernorm(qw, n(sd[p + ".attn.qkv.bias"]), n(sd[p + ".norm1.weight"]), n(sd[p + ".norm1.bias"]))[0]),
            "fc1_fe": pm.weight_exp(pm.fold_layernorm(f1w, n(sd[p + ".mlp.fc1.bias"]), n(sd[p + ".norm2.weight"]), n(sd[p + ".norm2.bias"]))[0])}


def _engine(cfg, sd, opts=()):
    from diff3dhpe_amd.engine import Engine
    from oracle import d3d_oracle as orc
    eng = Engine(cfg, precision="f16x3")
    eng.load_weights(sd)
    tabs = orc.diffusion_tables("cosine", 1000)
    eng.set_schedule(tabs["alphas_cumprod"], tabs["sqrt_one_minus_alphas_cumprod"], 2, 0.0, True)
    for key, v in opts:
        eng.set_option(key, v)
    return eng


def _oracle(sd, xcat, t, depth=1):
    """(fp64 result, the oracle's own fp32-vs-fp64 distance) on this checkpoint and input."""
    from oracle import d3d_oracle as orc
    heads = 8
    ref32 = orc.forward_denoise(sd, xcat, t, depth=depth, heads=heads)
    torch.set_default_dtype(torch.float64)      # (the oracle's sinusoid and identity follow the default dtype)
    try:
        ref64 = orc.forward_denoise({k: v.double() for k, v in sd.items()}, xcat.double(), t, depth=depth, heads=heads)
    finally:
        torch.set_default_dtype(torch.float32)
    assert ref64.dtype == torch.float64
    return ref64, (ref32.double() - ref64).abs().max().item()


def _traced(eng, call):
    """(result, {(block, kernel, buffer)}) of one forward under the per-kernel trace (include/d3d.h)."""
    eng.set_trace(4096, 1)
    try:
        out = call().clone()
        tags = [t for t, _ in eng.trace_read()]
    finally:
        eng.set_trace(0)
    return out, {((t >> 8) & 0xFF, (t >> 4) & 0xF, t & 0xF) for t in tags}


def _proof_default(eng, tr):
    assert eng.info("fused_spatial_last") == 1 and eng.info("block0_direct_last") == 1 and eng.info("long_temporal_last") == 0
    assert (0, 6, 0) in tr and (0, 7, 0) not in tr and (1, 3, 0) in tr


def _proof_unfused(eng, tr):
    assert eng.info("fused_spatial_last") == 0 and (0, 2, 0) in tr and (1, 2, 0) in tr      # q / k / v planes written by the qkv GEMM / direct form


def _proof_no_direct(eng, tr):
    assert eng.info("block0_direct_last") == 0 and eng.info("fused_spatial_last") == 1


def _proof_plain(eng, tr):      # not the folded flow: none of its plan words is set
    assert eng.info("fused_spatial_last") == 0 and eng.info("block0_direct_last") == 0 and eng.info("attn_h32_last") == 0


def _proof_row_postnorm(eng, tr):
    assert eng.info("fc2_split_last") == 0 and (0, 7, 0) in tr and (1, 7, 0) in tr


def _proof_latency(S):
    def proof(eng, tr):
        assert (eng.info("proj_split_last"), eng.info("fc1_split_last")) == (S, S) and eng.info("fc2_split_last") in (2, 4)
        assert (0, 4, 2) in tr and (1, 5, 2) in tr and (1, 7, 0) in tr
    return proof


def _proof_small(eng, tr):
    assert eng.info("small_tiles_last") == 3


def _proof_h32(eng, tr):
    assert eng.info("attn_h32_last") == 1 and (0, 7, 0) in tr                               # fc2 without the post-norm epilogue


def _proof_long(eng, tr):
    assert eng.info("long_temporal_last") == 1 and (1, 2, 0) in tr


# (name, T, embed_dim, B, options, proof)
LAT = (("latency_mode", 1),)
PATHS = [
    ("default_T27", 27, 512, 2, (), _proof_default),
    ("default_T81", 81, 512, 1, (), _proof_default),
    ("default_T243", 243, 512, 1, (), _proof_default),
    ("unfused", 27, 512, 2, (("fused_spatial", 0), ("fused_temporal", 0)), _proof_unfused),
    ("no_block0_direct", 27, 512, 2, (("block0_direct", 0),), _proof_no_direct),
    ("plain_flow", 27, 512, 2, (("fold_layernorm", 0),), _proof_plain),
    ("row_postnorm", 27, 512, 2, (("fused_postnorm", 0),), _proof_row_postnorm),
    ("latency_split2", 27, 512, 2, LAT + (("proj_split", 2), ("fc1_split", 2)), _proof_latency(2)),
    ("latency_split4", 27, 512, 2, LAT + (("proj_split", 4), ("fc1_split", 4)), _proof_latency(4)),
    ("small_tiles", 27, 512, 2, LAT + (("small_tiles", 1), ("block0_direct", 0)), _proof_small),
    ("embed256_h32", 27, 256, 2, (), _proof_h32),
    ("long_temporal_T257", 257, 512, 1, (), _proof_long),
]
# six different admitted exponents, one per matrix: crossed plumbing between any two shows.  The live ones (folded flow) stay >= 5.
MIXED_DEAD = {"qkv_e": 3, "proj_e": 6, "fc1_e": 4, "fc2_e": 8}
MIXED_LIVE = {"qkv_fe": 7, "fc1_fe": 5}


def _inputs(B, T, seed=500):
    inp = inputs(B, T, seed)
    t = torch.tensor([905, 17, 443, 0][:B], dtype=torch.long)
    return inp["x2d"], inp["noise"] * 0.7, t


def _engine_errors(cfg, B, opts, proof, models):
    """{model name: (error vs the fp64 oracle, oracle fp32 floor)} for the checkpoints in `models`, each on an engine of its own."""
    x2d, y, t = _inputs(B, cfg.num_frame)
    xcat = torch.cat([x2d, y], dim=-1)
    res = {}
    for name, sd in models.items():
        ref64, floor = _oracle(sd, xcat, t, cfg.depth)
        eng = _engine(cfg, sd, opts)
        eng.range_flags(clear=True)
        call = lambda: eng.denoise(x2d.cuda(), y.cuda(), t.float().cuda())
        out = call().clone()
        flags = eng.range_flags()
        assert torch.isfinite(out).all() and flags == 0, (name, eng.describe_range_flags(flags))
        traced, tr = _traced(eng, call)
        assert torch.equal(traced, out)
        if proof is not None:
            proof(eng, tr)
        res[name] = ((out.cpu().double() - ref64).abs().max().item(), floor)
    return res


@pytest.mark.parametrize("name,T,D,B,opts,proof", PATHS, ids=[p[0] for p in PATHS])
def test_engine_paths(name, T, D, B, opts, proof):
    """Every flow of the block loop on three checkpoints: clean (inputs zeroed, no outlier), dead (the four un-folded matrices at the lowest
    admitted exponent, their inputs exactly zero) and mixed (six different exponents; the folded ones live).  Dead: no worse than the clean
    checkpoint by more than the oracle's own fp32 floor (the rule of tests/test_gpu_block0_direct.py).  Live: within twice that floor + 2e-6.
    Everything inside the 1e-4 gate, the range word 0, the path proven from the plan's info keys and the trace."""
    cfg = DenoiserConfig(num_frame=T, embed_dim=D, depth=1)
    Dm = cfg.mlp_hidden
    models = {"clean": _doctor(_sd(cfg), D, Dm),
              "dead": _doctor(_sd(cfg), D, Dm, dead={m: MIN_EXP for m in MATS[:4]}),
              "mixed": _doctor(_sd(cfg), D, Dm, dead=MIXED_DEAD, live=MIXED_LIVE)}
    for p in PFX:
        assert _expected_exponents(models["clean"], p) == {m: 12 for m in MATS}
        assert _expected_exponents(models["dead"], p) == {**{m: MIN_EXP for m in MATS[:4]}, "qkv_fe": 12, "fc1_fe": 12}
        mixed = _expected_exponents(models["mixed"], p)
        assert mixed == {**MIXED_DEAD, **MIXED_LIVE} and len(set(mixed.values())) == 6, mixed
    res = _engine_errors(cfg, B, opts, proof, models)
    (e_clean, floor), (e_dead, _), (e_mixed, floor_m) = res["clean"], res["dead"], res["mixed"]
    print(f"engine [{name}] T={T} D={D} B={B}: clean {e_clean:.3e}, dead k={MIN_EXP} {e_dead:.3e} (oracle fp32 floor {floor:.3e}), "
          f"mixed {sorted({**MIXED_DEAD, **MIXED_LIVE}.items())} {e_mixed:.3e} (floor {floor_m:.3e})")
    assert max(e_clean, e_dead, e_mixed) <= GATE
    assert e_dead <= e_clean + floor, (e_dead, e_clean, floor)
    assert e_mixed <= 2 * floor_m + 2e-6, (e_mixed, floor_m)


@pytest.mark.parametrize("k", [k for k in EXPS if k >= MIN_EXP])
def test_engine_dead_exponent_sweep(k):
    """The default folded flow (proj_e, fc2_e) and the plain flow (qkv_e, fc1_e too) at every admitted exponent under test."""
    cfg = DenoiserConfig(num_frame=27, embed_dim=512, depth=1)
    models = {"clean": _doctor(_sd(cfg), 512, cfg.mlp_hidden), "dead": _doctor(_sd(cfg), 512, cfg.mlp_hidden, dead={m: k for m in MATS[:4]})}
    for opts, proof, flow in (((), _proof_default, "folded"), ((("fold_layernorm", 0),), _proof_plain, "plain")):
        res = _engine_errors(cfg, 2, opts, proof, models)
        (e_clean, floor), (e_dead, _) = res["clean"], res["dead"]
        print(f"engine dead sweep k={k} [{flow} flow]: clean {e_clean:.3e}, dead {e_dead:.3e}, oracle fp32 floor {floor:.3e}")
        assert e_dead <= GATE and e_dead <= e_clean + floor, (k, flow, e_dead, e_clean, floor)


@pytest.mark.parametrize("k", [k for k in EXPS if k < MIN_EXP])
def test_engine_refuses_exponents_below_the_line(k):
    """Below F16X3_MIN_WEIGHT_EXP the planes of a matrix's ordinary entries lose more than the engine may lose in silence (DESIGN section
    4.1): the commit raises D3D_RANGE_WEIGHT, sticky, as for a non-finite weight."""
    cfg = DenoiserConfig(num_frame=27, embed_dim=512, depth=1)
    lib = _lib()
    for m in MATS[:4]:
        eng = _engine(cfg, _doctor(_sd(cfg), 512, cfg.mlp_hidden, dead={m: k}))
        assert eng.range_flags(clear=False) & lib.RANGE_WEIGHT, (m, k)
        with pytest.raises(lib.D3DError, match="range"):
            eng.check_range()


def test_engine_own_fc1_and_proj_kernels():
    """launch_fc1_x3 and launch_proj_x3 (from two rounds of tiles on: B = 32, T = 243) on the mixed checkpoint: bit for bit the template forms
    ("fc1_kernel" / "proj_kernel" = 0), as tests/test_gpu_round4.py asserts at k = 12, and the first two sequences against the oracle."""
    cfg = DenoiserConfig(num_frame=243, embed_dim=512, depth=1)
    B = 32
    sd = _doctor(_sd(cfg), 512, cfg.mlp_hidden, dead=MIXED_DEAD, live=MIXED_LIVE)
    inp = inputs(B, 243, 79)
    x2d, y = inp["x2d"], inp["noise"] * 0.7
    t = torch.tensor([(431 * i + 77) % 1000 for i in range(B)], dtype=torch.long)
    eng = _engine(cfg, sd)
    call = lambda: eng.denoise(x2d.cuda(), y.cuda(), t.float().cuda()).clone()
    eng.range_flags(clear=True)
    own = call()
    assert torch.isfinite(own).all() and eng.range_flags() == 0
    for key in ("fc1_kernel", "proj_kernel"):
        eng.set_option(key, 0)
        assert torch.equal(call(), own), key
        eng.set_option(key, 1)
    ref64, floor = _oracle(sd, torch.cat([x2d[:2], y[:2]], dim=-1), t[:2])
    e = (own[:2].cpu().double() - ref64).abs().max().item()
    print(f"engine [own fc1 / proj kernels] T=243 B={B}: mixed {e:.3e} (oracle fp32 floor {floor:.3e})")
    assert e <= GATE and e <= 2 * floor + 2e-6
