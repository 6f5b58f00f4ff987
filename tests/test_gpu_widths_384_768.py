"""The GEMMs and the row kernel at embed_dim 384 and 768 (heads of 48 and 96 columns) on the MI355X: every N and K an engine of these
widths runs -- {384, 768, 1152, 1536, 2304} -- in the folded, plane-residual and plain F16X3 forms and in the fp32 kernel, and the row
kernel at D = 384 and 768 with pair-layout outputs.  N = 384 and 1152 are no multiple of 256: the 256-column tile shapes and the walks refuse them, the 128-column ones must take them.  Operands,
helpers and bounds are those of tests/test_gpu_folded_forms.py (each form's own test there) and tests/test_gpu_ops.py.

Measured (MI355X), max-abs against fp64, worst of each form's cases (its bound in brackets): qkv form q columns 0.14 of the per-value
bound, k / v columns 2.5e-6 (1.9e-5); fc1 form 2.4e-6 (1.9e-5); proj form planes 2.6e-6 (1.9e-5), statistics 8.9e-6 / 2.9e-5 (2e-3 / 1e-2);
fc2-to-fp32 form 3.5e-6 (2.3e-5); op_linear F16X3 4.4e-6 and fp32 7.3e-6 at K = 1536 (1.4e-5); row kernel post-norm 5.6e-7, second
LayerNorm 6.7e-7 (3e-6), planes at 1.00 of the quantum.  Launch shapes reached: 128 x 128 tiles ("small") and 256 x 128 tiles ("mid")."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import hashed, maxabs, _tol
from test_gpu_folded_forms import (EPS, LN_TOL, ST_SUM, ST_SQ, _E, _m, _launch_shape, _mat, _weights, _affine, _partials, _folded_ref,
                                   _qkv_errors, _residual_operands, _plane_quantum, _ln_inputs)

pytestmark = pytest.mark.gpu
ROWS = ["small", "mid"]


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("N,K", [(1152, 384), (2304, 768)])
def test_qkv_form_matches_fp64(N, K, rows):
    """(FX_LNF, EPI_NONE, outsplit 1) at the qkv shapes: the bounds of test_gpu_folded_forms.py::test_qkv_form_matches_fp64."""
    M, qcols = _m(rows, N), K
    X = _mat("ffXq", M, K, 31, 2.0, 0.3)
    (W, b), (g, be) = _weights("q", N, K), _affine("q", K)
    ref = _folded_ref(X, W, b, g, be, False)
    for st_np in (1, K // 64):
        hi, lo = _E().op_linear_folded(X, W, b, g, be, _partials(X, st_np), EPS, "none", qcols)
        ratio, eq, ekv, tkv = _qkv_errors(hi, lo, ref, qcols, K)
        print(f"qkv form {rows} ({_launch_shape(M, N, K)}) M={M} N={N} K={K} st_np={st_np}: q columns {eq:.3e} ({ratio:.2f} of the per-value "
              f"bound), k/v columns {ekv:.3e} (tol {tkv:.3e})")
        assert ratio < 1.0
        assert ekv < tkv


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("N,K", [(768, 384), (1536, 768)])
def test_fc1_form_matches_fp64(N, K, rows):
    """(FX_LNF, EPI_GELU, outsplit 2) at the fc1 shapes: the bound of test_gpu_folded_forms.py::test_fc1_form_matches_fp64."""
    M = _m(rows, N)
    X = _mat("ffXf", M, K, 41, 2.0, 0.3)
    (W, b), (g, be) = _weights("f", N, K), _affine("f", K)
    ref = _folded_ref(X, W, b, g, be, True)
    for st_np in (1, K // 64):
        h = _E().op_linear_folded(X, W, b, g, be, _partials(X, st_np), EPS, "gelu")
        e = (h.double() - ref).abs().max().item()
        print(f"fc1 form {rows} ({_launch_shape(M, N, K)}) M={M} N={N} K={K} st_np={st_np}: {e:.3e} (tol {_tol(K) + 2e-6:.3e})")
        assert e < _tol(K) + 2e-6


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("D", [384, 768])
def test_proj_form_matches_fp64(D, rows):
    """(FX_RP | FX_SO, EPI_RESIDUAL, outsplit 2) at N = K = D: 6 and 12 statistics partials per row; the bounds of
    test_gpu_folded_forms.py::test_proj_form_matches_fp64, and the same bits from a slice of the rows."""
    N = K = D
    M = _m(rows, N)
    A, W, b, R, ref = _residual_operands("p", M, N, K)
    x, st = _E().op_linear_plane_residual(A, W, b, R)
    assert st.shape == (M, N // 64, 2)
    e = (x.double() - ref).abs().max().item()
    blocks = ref.view(M, N // 64, 64)
    es = (st[:, :, 0].double() - blocks.sum(2)).abs().max().item()
    esq = (st[:, :, 1].double() - (blocks * blocks).sum(2)).abs().max().item()
    print(f"proj form {rows} ({_launch_shape(M, N, K, proj=True)}) M={M} N=K={D}: planes {e:.3e} (tol {_tol(K) + 2e-6:.3e}); statistics "
          f"{es:.3e} {esq:.3e} (tol {ST_SUM:.0e} {ST_SQ:.0e})")
    assert e < _tol(K) + 2e-6
    assert es < ST_SUM and esq < ST_SQ
    part, pst = _E().op_linear_plane_residual(A[100:229].contiguous(), W, b, R[100:229].contiguous())
    assert torch.equal(part, x[100:229]) and torch.equal(pst, st[100:229])


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("N,K", [(384, 768), (768, 1536)])
def test_fc2_fp32_form_matches_fp64(N, K, rows):
    """(FX_RP, EPI_RESIDUAL, outsplit 0) at the fc2 shapes: the bound of test_gpu_folded_forms.py::test_fc2_fp32_form_matches_fp64."""
    M = _m(rows, N)
    A, W, b, R, ref = _residual_operands("c", M, N, K)
    y, st = _E().op_linear_plane_residual(A, W, b, R, with_stats=False)
    assert st is None
    e = (y.double() - ref).abs().max().item()
    print(f"fc2-to-fp32 form {rows} ({_launch_shape(M, N, K)}) M={M} N={N} K={K}: {e:.3e} (tol {_tol(K):.3e})")
    assert e < _tol(K)


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("N,K", [(1152, 384), (2304, 768), (768, 384), (1536, 768), (384, 384), (768, 768), (384, 768), (768, 1536)])
def test_plain_linear_matches_fp64(N, K, rows, prec):
    """op_linear in every epilogue, operands and bound (2e-6 sqrt(K / 32)) of tests/test_gpu_ops.py::test_linear_matches_fp64."""
    E = _E()
    M = _m(rows, N)
    A = hashed(f"A{M}", (M, K), 11, 2.0).cuda()
    W = hashed(f"W{N}", (N, K), 12, 1.0 / np.sqrt(K)).cuda()
    b = hashed(f"b{N}", (N,), 13, 0.5).cuda()
    R = hashed(f"R{M}", (M, N), 14, 1.0).cuda()
    ref = A.double() @ W.double().t() + b.double()
    tol = 2e-6 * np.sqrt(K / 32)
    errs = (maxabs(E.op_linear(A, W, b, precision=prec), ref.cpu()),
            maxabs(E.op_linear(A, W, None, precision=prec), (ref - b.double()).cpu()),
            maxabs(E.op_linear(A, W, b, epi="gelu", precision=prec), F.gelu(ref).cpu()),
            maxabs(E.op_linear(A, W, b, residual=R, epi="residual", precision=prec), (ref + R.double()).cpu()))
    print(f"linear {prec} {rows} M={M} N={N} K={K}: bias {errs[0]:.3e} none {errs[1]:.3e} gelu {errs[2]:.3e} residual {errs[3]:.3e} (tol {tol:.3e})")
    assert max(errs) < tol


@pytest.mark.parametrize("M,N,K", [(129, 144, 48), (459, 48, 48), (300, 96, 48), (459, 48, 96), (129, 130, 144), (7, 48, 16)])
def test_fp32_linear_with_a_last_k_tile_of_16_columns(M, N, K):
    """The fp32 GEMM at K % 32 == 16 -- the shapes of an engine with one head of 48 columns (embed_dim 48: qkv 144 x 48, proj 48 x 48,
    fc1 96 x 48, fc2 48 x 96), three heads (K = 144) and a single half tile: the last k-tile's columns behind K are zero-filled.  Every
    epilogue, operands and bound (2e-6 sqrt(K / 32), K rounded up to whole tiles) of tests/test_gpu_ops.py::test_linear_matches_fp64; the
    F16X3 form goes on refusing such a K."""
    E = _E()
    A = hashed(f"A{M}", (M, K), 11, 2.0).cuda()
    W = hashed(f"W{N}", (N, K), 12, 1.0 / np.sqrt(K)).cuda()
    b = hashed(f"b{N}", (N,), 13, 0.5).cuda()
    R = hashed(f"R{M}", (M, N), 14, 1.0).cuda()
    ref = A.double() @ W.double().t() + b.double()
    tol = 2e-6 * np.sqrt(-(-K // 32))
    errs = (maxabs(E.op_linear(A, W, b, precision="fp32"), ref.cpu()),
            maxabs(E.op_linear(A, W, None, precision="fp32"), (ref - b.double()).cpu()),
            maxabs(E.op_linear(A, W, b, epi="gelu", precision="fp32"), F.gelu(ref).cpu()),
            maxabs(E.op_linear(A, W, b, residual=R, epi="residual", precision="fp32"), (ref + R.double()).cpu()))
    print(f"linear fp32 M={M} N={N} K={K}: bias {errs[0]:.3e} none {errs[1]:.3e} gelu {errs[2]:.3e} residual {errs[3]:.3e} (tol {tol:.3e})")
    assert max(errs) < tol
    if K % 32:
        from diff3dhpe_amd._lib import D3DError
        with pytest.raises(D3DError, match="multiple of 32"):
            E.op_linear(A, W, b, precision="f16x3")


@pytest.mark.parametrize("rows", [3, 333])
@pytest.mark.parametrize("D", [384, 768])
def test_row_kernel_forms_with_pair_layout_outputs(D, rows):
    """The stream entry (skip_ln1), the post-norm form and the second LayerNorm at D = 384 and 768 -- 12 and 24 pair groups of 32 columns
    per row -- as fp32, as planes and with statistics: the checks and bounds of
    test_gpu_folded_forms.py::test_row_kernel_stream_entry_and_postnorm_forms and ::test_row_kernel_second_layernorm_forms."""
    E = _E()
    x, g, b, pos, tv, add = _ln_inputs(rows, D)
    xd = x.double()
    o = E.op_layernorm_forms(x, skip_ln1=True, outputs=("y", "y_x3", "stats"))
    assert torch.equal(o["y"], x)
    assert ((o["y_x3"] - x).abs() <= _plane_quantum(x)).all()
    es, esq = maxabs(o["stats"][:, 0], xd.sum(1).cpu()), maxabs(o["stats"][:, 1], (xd * xd).sum(1).cpu())
    ref = F.layer_norm(xd, (D,), g.double(), b.double(), EPS) + add
    p = E.op_layernorm_forms(x, g, b, EPS, pos=pos, pos_div=17, tvec=tv, rows_per_batch=51, outputs=("y", "y_x3", "stats"))
    e = (p["y"].double() - ref).abs().max().item()
    ps, psq = maxabs(p["stats"][:, 0], ref.sum(1).cpu()), maxabs(p["stats"][:, 1], (ref * ref).sum(1).cpu())
    plane = ((p["y_x3"] - p["y"]).abs() / _plane_quantum(p["y"])).max().item()
    g2 = (1 + 0.2 * hashed("lng2", (D,), 6)).cuda()
    b2 = (0.2 * hashed("lnb2", (D,), 7)).cuda()
    kw = dict(pos=pos, pos_div=17, tvec=tv, rows_per_batch=51, gamma2=g2, beta2=b2, eps2=1e-5)
    a = E.op_layernorm_forms(x, g, b, EPS, outputs=("y", "h"), **kw)
    own = (a["h"].double() - F.layer_norm(a["y"].double(), (D,), g2.double(), b2.double(), 1e-5)).abs().max().item()
    c = E.op_layernorm_forms(x, g, b, EPS, outputs=("y_x3", "stats", "h_x3"), **kw)
    hplane = ((c["h_x3"] - a["h"]).abs() / _plane_quantum(a["h"])).max().item()
    print(f"row kernel D={D} rows={rows}: entry statistics {es:.3e} {esq:.3e}; post-norm y {e:.3e} (tol {LN_TOL:.0e}), planes vs y "
          f"{plane:.2f} of the quantum, statistics {ps:.3e} {psq:.3e} (tol {ST_SUM:.0e} {ST_SQ:.0e}); LN2 h {own:.3e}, h planes {hplane:.2f}")
    assert es < ST_SUM and esq < ST_SQ
    assert e < LN_TOL
    assert plane <= 1.0
    assert ps < ST_SUM and psq < ST_SQ
    assert own < LN_TOL
    assert hplane <= 1.0
    assert torch.equal(a["y"], p["y"]) and ((c["y_x3"] - a["y"]).abs() <= _plane_quantum(a["y"])).all()
