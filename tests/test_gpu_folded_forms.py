"""The four folded forms of the F16X3 tile template (D3D_X3_FORMS in csrc/kernels_gemm_x3p.hip: qkv, proj, fc1, fc2-to-fp32) and the
output forms of the LayerNorm row kernel, each alone through its single-op hook (d3d_op_linear_folded, d3d_op_linear_plane_residual,
d3d_op_layernorm_forms) against plain fp64 torch of the same operation -- at every embedding width the engine runs them at and in
every launch shape launch_x3q_auto chooses: 128 x 128 tiles, 256 x 128 tiles, 256 x 256 tiles (one workgroup per tile, odd k-tile
count), the 256-row persistent walk (statistics staged by LDS-DMA up to 8 partials per row, loaded in the kernel beyond) and the
192-row walk of proj.  Everything hand-specialised (launch_fc1_x3, launch_proj_x3, the fused qkv + attention kernels) is pinned bit
for bit to these forms elsewhere; here the forms themselves meet fp64.

Bounds (the project's own, helpers._tol): an fp32 output of a K-deep product 3e-6 sqrt(K / 32) + 2e-6; 2e-6 more for a value read
back from planes of 8 y (22 bits of |8 y| <= ~40); statistics 2e-3 on sums, 1e-2 on sums of squares.  The q third of a qkv output is
stored at scale 1: a value v is the fp16 pair hi = fp16(v), lo = fp16(v - hi); hi keeps 11 bits, lo 11 bits of the rest, so the pair
is within 2^-22 |v| of v, unless lo falls below the smallest normal fp16 (2^-14), where its quantum is 2^-24: an error of at most
2^-25.  Hence max(2^-22 |v|, 2^-25) per value on top of _tol(K), checked per element against the fp64 value."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import hashed, maxabs, cu_count, _ROWS, _rows, _tol

pytestmark = pytest.mark.gpu

EPS = 1e-6
ST_SUM, ST_SQ = 2e-3, 1e-2      # the statistics bounds of tests/test_gpu_latency_mode_proj_fc1.py
assert "walk256" in _ROWS


def _E():
    from diff3dhpe_amd import engine
    return engine


# ---------------------------------------------------------------------------------------------------------------- rows and launch shapes
def _m(rows, N):
    """The row count of a named case: ragged in M, resolved from the CU count inside the test."""
    if rows == "small":
        return 129                                               # two 128-row tiles per 128 columns, each on a CU of its own
    if rows == "mid":
        return 128 * (cu_count() // (N // 128) + 1) + 77        # more 128 x 128 tiles than CUs, far below 1024 tiles of 256 x 256
    return _rows(rows)


def _launch_shape(M, N, K, proj=False):
    """launch_x3q_auto's ladder (csrc/kernels_gemm_x3p.hip), restated: the case names must mean the launch shapes they are named for."""
    big = N % 256 == 0 and -(-M // 256) * -(-N // 256) >= 4 * 256
    if big and (K // 32) % 2 == 0:
        return "walk192" if proj else "walk256"
    if big:
        return "tile256x256"
    if N % 128 == 0 and -(-M // 128) * -(-N // 128) <= cu_count():
        return "tile128x128"
    return "tile256x128"


_SHAPE_OF = {"small": "tile128x128", "mid": "tile256x128"}


def _expect_shape(rows, M, N, K, proj=False):
    want = _SHAPE_OF.get(rows) or ("tile256x256" if (K // 32) % 2 else ("walk192" if proj else "walk256"))
    got = _launch_shape(M, N, K, proj)
    assert got == want, f"{rows}: M = {M}, N = {N}, K = {K} on {cu_count()} CUs launches {got}, the case is meant for {want}"
    return got


# ---------------------------------------------------------------------------------------------------------------- operands
_BASE_ROWS = 4099     # (prime)


@functools.lru_cache(maxsize=None)
def _base(name, cols, seed, scale):
    return hashed(name, (_BASE_ROWS, cols), seed, scale).cuda()


def _mat(name, M, cols, seed, scale, offset=0.0):
    """(M, cols) hashed rows at `scale` plus `offset`, on the GPU.  Beyond 4099 rows (the walks: 131 k rows) the rows of one hashed block
    of 4099 are taken in a stride-31 order instead of hashing every value on the host: a tile still holds 256 different rows, and every
    row is compared with its own fp64 value."""
    if M <= _BASE_ROWS:
        return (hashed(f"{name}{M}", (M, cols), seed, scale) + offset).cuda()
    idx = (torch.arange(M, device="cuda") * 31) % _BASE_ROWS
    return _base(name, cols, seed, scale)[idx] + offset


def _weights(tag, N, K):
    W = hashed(f"ffW{tag}{N}x{K}", (N, K), 32, 1.0 / np.sqrt(K)).cuda()
    b = hashed(f"ffb{tag}{N}", (N,), 33, 0.5).cuda()
    return W, b


def _affine(tag, K):
    return (1 + 0.2 * hashed(f"ffg{tag}{K}", (K,), 35)).cuda(), (0.2 * hashed(f"ffbe{tag}{K}", (K,), 36)).cuda()


def _partials(X, st_np):
    """(M, st_np, 2): fp64 (sum, sum of squares) over K / st_np equal column blocks of every row, rounded to fp32."""
    M, K = X.shape
    assert K % st_np == 0
    blk = X.double().view(M, st_np, K // st_np)
    return torch.stack((blk.sum(2), (blk * blk).sum(2)), dim=2).float().contiguous()


def _folded_ref(X, W, b, g, be, gelu):
    K = X.shape[1]
    ref = F.layer_norm(X.double(), (K,), g.double(), be.double(), EPS) @ W.double().t() + b.double()
    return F.gelu(ref) if gelu else ref


def _decode_qkv(hi, lo, qcols):
    v = hi.float() + lo.float()
    v[:, qcols:] /= 8
    return v


def _qkv_errors(hi, lo, ref, qcols, K):
    """(worst error / bound over the q columns, max error over them, max error over the k / v columns, their bound)."""
    err = (_decode_qkv(hi, lo, qcols).double() - ref).abs()
    q_bound = _tol(K) + torch.clamp(ref[:, :qcols].abs() * 2.0 ** -22, min=2.0 ** -25)
    return (err[:, :qcols] / q_bound).max().item(), err[:, :qcols].max().item(), err[:, qcols:].max().item(), _tol(K) + 2e-6


# ---------------------------------------------------------------------------------------------------------------- qkv form
QKV_WIDTHS = [(384, 128, 128), (768, 256, 256), (1536, 512, 512), (3072, 1024, 1024)]
QKV_CASES = ([(rows, N, K, q, st) for (N, K, q) in QKV_WIDTHS for rows in ("small", "mid") for st in (1, K // 64)]
             + [("mid", 768, 256, 256, 16)]
             + [("walk256", N, K, q, st) for (N, K, q) in ((768, 256, 256), (512, 128, 128)) for st in (1, K // 64)]
             + [("walk256", 512, 96, 128, 1), ("walk256", 512, 96, 128, 3)])     # odd K / 32: 256 x 256 tiles, one workgroup each


@pytest.mark.parametrize("rows,N,K,qcols,st_np", QKV_CASES)
def test_qkv_form_matches_fp64(rows, N, K, qcols, st_np):
    """(FX_LNF, EPI_NONE, outsplit 1): folded norm1, hi / lo planes, the q third at scale 1.  The q columns and the k / v columns meet
    their bounds separately: a wrong qcols boundary (a block of columns decoded at the wrong scale: 8x off) cannot hide in an overall
    maximum, nor can a wrong - rstd mean csum term of one tile position (the row mean is 0.3: the term is O(0.1) per value)."""
    M = _m(rows, N)
    shape = _expect_shape(rows, M, N, K)
    X = _mat("ffXq", M, K, 31, 2.0, 0.3)
    (W, b), (g, be) = _weights("q", N, K), _affine("q", K)
    hi, lo = _E().op_linear_folded(X, W, b, g, be, _partials(X, st_np), EPS, "none", qcols)
    ratio, eq, ekv, tkv = _qkv_errors(hi, lo, _folded_ref(X, W, b, g, be, False), qcols, K)
    print(f"qkv form {rows} ({shape}) M={M} N={N} K={K} st_np={st_np}: q columns {eq:.3e} ({ratio:.2f} of the per-value bound), "
          f"k/v columns {ekv:.3e} (tol {tkv:.3e})")
    assert ratio < 1.0
    assert ekv < tkv


# ---------------------------------------------------------------------------------------------------------------- fc1 form
FC1_CASES = ([(rows, N, K, st) for (N, K) in ((512, 256), (1024, 512), (2048, 1024)) for rows in ("small", "mid") for st in (1, K // 64)]
             + [("walk256", 512, 128, st) for st in (1, 8, 16)]                  # 1, 8: statistics by LDS-DMA; 16: loaded in the kernel
             + [("walk256", 512, 96, 16)])                                        # odd K / 32: 256 x 256 tiles, one workgroup each


@pytest.mark.parametrize("rows,N,K,st_np", FC1_CASES)
def test_fc1_form_matches_fp64(rows, N, K, st_np):
    """(FX_LNF, EPI_GELU, outsplit 2): folded norm2, GELU, accumulator-order pair planes, read back to fp32 -- the plane bound.  The
    walk with 16 partials per row (256 rows x 16 x 8 bytes > the 16 KiB the walk stages) takes the in-kernel loads of a PERSIST
    instantiation: the path of every large-batch D = 1024 call."""
    M = _m(rows, N)
    shape = _expect_shape(rows, M, N, K)
    X = _mat("ffXf", M, K, 41, 2.0, 0.3)
    (W, b), (g, be) = _weights("f", N, K), _affine("f", K)
    h = _E().op_linear_folded(X, W, b, g, be, _partials(X, st_np), EPS, "gelu")
    e = (h.double() - _folded_ref(X, W, b, g, be, True)).abs().max().item()
    print(f"fc1 form {rows} ({shape}) M={M} N={N} K={K} st_np={st_np}: {e:.3e} (tol {_tol(K) + 2e-6:.3e})")
    assert e < _tol(K) + 2e-6


# ---------------------------------------------------------------------------------------------------------------- proj form
def _residual_operands(tag, M, N, K):
    A = _mat(f"ffA{tag}", M, K, 21, 2.0)
    R = _mat(f"ffR{tag}", M, N, 24, 1.5, 0.3)
    W, b = _weights(tag, N, K)
    return A, W, b, R, R.double() + A.double() @ W.double().t() + b.double()


PROJ_CASES = [(rows, D) for D in (128, 256, 512, 1024) for rows in ("small", "mid")] + [("walk256", 512)]


@pytest.mark.parametrize("rows,D", PROJ_CASES)
def test_proj_form_matches_fp64(rows, D):
    """(FX_RP | FX_SO, EPI_RESIDUAL, outsplit 2): plane residual in place, (sum, sum of squares) per row and 64 columns -- 2, 4, 8 and 16
    partials per row; "walk256" at N = 512 is proj's own 192-row walk.  Rows 100 .. 229 alone (another tile shape, other tile positions)
    give the same bits, planes and statistics."""
    N = K = D
    M = _m(rows, N)
    shape = _expect_shape(rows, M, N, K, proj=True)
    A, W, b, R, ref = _residual_operands("p", M, N, K)
    x, st = _E().op_linear_plane_residual(A, W, b, R)
    assert st.shape == (M, N // 64, 2)
    e = (x.double() - ref).abs().max().item()
    blocks = ref.view(M, N // 64, 64)
    es = (st[:, :, 0].double() - blocks.sum(2)).abs().max().item()
    esq = (st[:, :, 1].double() - (blocks * blocks).sum(2)).abs().max().item()
    print(f"proj form {rows} ({shape}) M={M} N=K={D}: planes {e:.3e} (tol {_tol(K) + 2e-6:.3e}); statistics {es:.3e} {esq:.3e} "
          f"(tol {ST_SUM:.0e} {ST_SQ:.0e})")
    assert e < _tol(K) + 2e-6
    assert es < ST_SUM and esq < ST_SQ
    part, pst = _E().op_linear_plane_residual(A[100:229].contiguous(), W, b, R[100:229].contiguous())
    assert torch.equal(part, x[100:229]) and torch.equal(pst, st[100:229])


# ---------------------------------------------------------------------------------------------------------------- fc2-to-fp32 form
@pytest.mark.parametrize("rows", ["small", "mid"])
@pytest.mark.parametrize("N,K", [(128, 256), (256, 512), (1024, 2048)])
def test_fc2_fp32_form_matches_fp64(N, K, rows):
    """(FX_RP, EPI_RESIDUAL, outsplit 0): plane residual, fp32 out -- the only fc2 of the D = 128 / 256 / 1024 models."""
    M = _m(rows, N)
    shape = _expect_shape(rows, M, N, K)
    A, W, b, R, ref = _residual_operands("c", M, N, K)
    y, st = _E().op_linear_plane_residual(A, W, b, R, with_stats=False)
    assert st is None
    e = (y.double() - ref).abs().max().item()
    print(f"fc2-to-fp32 form {rows} ({shape}) M={M} N={N} K={K}: {e:.3e} (tol {_tol(K):.3e})")
    assert e < _tol(K)


# ---------------------------------------------------------------------------------------------------------------- chain proj -> fc1
@pytest.mark.parametrize("D", [256, 1024])
def test_proj_statistics_feed_the_folded_fc1(D):
    """fc1 as the engine runs it: the planes and the D / 64 statistics partials of the proj form are the operands of the folded fc1.
    (The proj hook hands the planes over as fp32: (hi + lo) / 8 is exact in fp32, and splitting it again gives hi and lo back --
    fp16(hi + lo) = hi, since |lo| is at most half an ulp of hi and a tie went to the even hi already.)
    Three comparisons: (1) with fp64 of fc1 on the hook's own x: fc1's bound; (2) with fp64 of the composed operation: on top of (1),
    the proj error e_x = _tol(D) + 2e-6 per element of x passes through the LayerNorm (gain rstd gamma) and the D-term product with W1.
    Treated as independent errors of at most e_x, the sum over a row of W1 diag(gamma) has a standard deviation of at most e_x rstd
    |gamma W1[n]|_2; the bound takes six of them, times GELU's largest slope 1.13 -- all from the inputs, none from the kernel's
    output; (3) with the same call fed partials made in Python from x: bit-equal if those partials are the hook's bits, else within
    _tol(D) (partials that differ in their last bits move the mean and rstd of a row by parts in 1e7)."""
    E = _E()
    M, Dm = 300, 2 * D
    A, Wp, bp, R, xref = _residual_operands("ch", M, D, D)
    W1, b1 = _weights("ch1", Dm, D)
    g, be = _affine("ch", D)
    x, st = E.op_linear_plane_residual(A, Wp, bp, R)
    h = E.op_linear_folded(x, W1, b1, g, be, st, EPS, "gelu")
    own = (h.double() - _folded_ref(x, W1, b1, g, be, True)).abs().max().item()
    e_x = _tol(D) + 2e-6
    rstd = (xref.var(1, unbiased=False) + EPS).rsqrt().max().item()
    prop = 6 * 1.13 * e_x * rstd * (g.double() * W1.double()).norm(dim=1).max().item()
    composed = (h.double() - _folded_ref(xref, W1, b1, g, be, True)).abs().max().item()
    py = _partials(x, D // 64)
    h_py = E.op_linear_folded(x, W1, b1, g, be, py, EPS, "gelu")
    same = torch.equal(py, st)
    d = maxabs(h, h_py.cpu())
    print(f"chain D={D}: fc1 on the hook's x {own:.3e} (tol {_tol(D) + 2e-6:.3e}); composed {composed:.3e} (tol {_tol(D) + 2e-6 + prop:.3e}); "
          f"Python partials {'bit-equal' if same else 'differ'}, outputs differ by {d:.3e} (tol {_tol(D):.3e})")
    assert own < _tol(D) + 2e-6
    assert composed < _tol(D) + 2e-6 + prop
    if same:
        assert torch.equal(h, h_py)
    else:
        assert d < _tol(D)


# ---------------------------------------------------------------------------------------------------------------- shape independence
def _walk_rows(N, K, proj=False):
    """[(name, M)] of the three launch shapes of one (N, K), checked against the ladder."""
    out = []
    for rows in ("small", "mid", "walk256"):
        M = _m(rows, N)
        _expect_shape(rows, M, N, K, proj)
        out.append((rows, M))
    return out


@pytest.mark.parametrize("form", ["qkv", "fc1", "proj", "fc2"])
def test_values_do_not_depend_on_the_launch_shape(form):
    """"Values do not depend on the tile shape" (launch_x3q_auto): rows 0 .. 128 of one matrix, run as the head of a 129-row call (128 x
    128 tiles), of a mid-size call (256 x 128 tiles) and of a walk (256-row; proj: 192-row), are the same bits in every output."""
    E = _E()
    N, K = (512, 512) if form == "proj" else (512, 128)
    cases = _walk_rows(N, K, proj=form == "proj")
    Mmax = max(M for _, M in cases)
    if form in ("qkv", "fc1"):
        X = _mat("ffXs", Mmax, K, 51, 2.0, 0.3)
        (W, b), (g, be) = _weights("s", N, K), _affine("s", K)
        st = _partials(X, K // 64)
        run = lambda M: E.op_linear_folded(X[:M].contiguous(), W, b, g, be, st[:M].contiguous(), EPS, "none" if form == "qkv" else "gelu",
                                           128 if form == "qkv" else 0)
    else:
        A, W, b, R, _ = _residual_operands("s", Mmax, N, K)
        run = lambda M: E.op_linear_plane_residual(A[:M].contiguous(), W, b, R[:M].contiguous(), with_stats=form == "proj")
    heads = {}
    for rows, M in cases:
        out = run(M)
        heads[rows] = [t[:129].clone() for t in (out if isinstance(out, tuple) else (out,)) if t is not None]
    for rows in ("mid", "walk256"):
        for a, c in zip(heads["small"], heads[rows]):
            assert torch.equal(a, c), f"{form}: rows 0 .. 128 differ between the small launch and {rows}"


# ---------------------------------------------------------------------------------------------------------------- row kernel
LN_TOL = 3e-6        # tests/test_gpu_ops.py::test_layernorm, on the same operands


def _plane_quantum(v, scale=8.0):
    """What a value may lose in planes of scale * v: max(2^-22 |v|, 2^-25 / scale) (module docstring)."""
    return torch.clamp(v.abs() * 2.0 ** -22, min=2.0 ** -25 / scale)


def _ln_inputs(rows, D):
    x = hashed("lnx", (rows, D), 3, 3.0).cuda() + 0.7
    g = (1 + 0.1 * hashed("lng", (D,), 4)).cuda()
    b = (0.1 * hashed("lnb", (D,), 5)).cuda()
    pos = hashed("pnpos", (9, D), 27, 0.5).cuda()
    tv = hashed("pntvr", ((rows + 50) // 51, D), 29, 0.5).cuda()
    r = torch.arange(rows, device="cuda")
    add = pos.double()[(r // 17) % 9] + tv.double()[r // 51]
    return x, g, b, pos, tv, add


@pytest.mark.parametrize("rows", [3, 333])
@pytest.mark.parametrize("D", [32, 128, 256, 512, 1024])
def test_row_kernel_stream_entry_and_postnorm_forms(D, rows):
    """skip_ln1 (the entry of block 0: planes of the rows themselves + their statistics) and the post-norm form of the widths without
    the fc2 epilogue norm: y = LN(x) + pos + tvec as fp32, as planes and with statistics, in one launch.  Row classes as
    test_linear_postnorm_matches_fp64: pos_div 17, 9 positions, 51 rows per batch element."""
    E = _E()
    x, g, b, pos, tv, add = _ln_inputs(rows, D)
    o = E.op_layernorm_forms(x, skip_ln1=True, outputs=("y", "y_x3", "stats"))
    xd = x.double()
    assert torch.equal(o["y"], x)
    assert ((o["y_x3"] - x).abs() <= _plane_quantum(x)).all()
    es, esq = maxabs(o["stats"][:, 0], xd.sum(1).cpu()), maxabs(o["stats"][:, 1], (xd * xd).sum(1).cpu())
    o2 = E.op_layernorm_forms(x, skip_ln1=True, pos=pos, pos_div=17, tvec=tv, rows_per_batch=51, outputs=("y",))
    e_skip = (o2["y"].double() - (xd + add)).abs().max().item()
    ref = F.layer_norm(xd, (D,), g.double(), b.double(), EPS) + add
    p = E.op_layernorm_forms(x, g, b, EPS, pos=pos, pos_div=17, tvec=tv, rows_per_batch=51, outputs=("y", "y_x3", "stats"))
    e = (p["y"].double() - ref).abs().max().item()
    ps, psq = maxabs(p["stats"][:, 0], ref.sum(1).cpu()), maxabs(p["stats"][:, 1], (ref * ref).sum(1).cpu())
    plane = ((p["y_x3"] - p["y"]).abs() / _plane_quantum(p["y"])).max().item()
    print(f"row kernel D={D} rows={rows}: entry statistics {es:.3e} {esq:.3e}, entry + pos + tvec {e_skip:.3e}; post-norm y {e:.3e} "
          f"(tol {LN_TOL:.0e}), planes vs y {plane:.2f} of the quantum, statistics {ps:.3e} {psq:.3e} (tol {ST_SUM:.0e} {ST_SQ:.0e})")
    assert es < ST_SUM and esq < ST_SQ
    assert e_skip < 1e-6                      # two fp32 additions to values below 8: 2 x 2^-22
    assert e < LN_TOL
    assert plane <= 1.0
    assert ps < ST_SUM and psq < ST_SQ
    # the plain forms one at a time give the bits of the combined launch
    assert torch.equal(E.op_layernorm_forms(x, g, b, EPS, pos=pos, pos_div=17, tvec=tv, rows_per_batch=51, outputs=("y",))["y"], p["y"])
    assert torch.equal(E.op_layernorm_forms(x, g, b, EPS, outputs=("y",))["y"], E.op_layernorm(x, g, b, EPS))


@pytest.mark.parametrize("rows", [3, 333])
@pytest.mark.parametrize("D", [32, 128, 256, 512, 1024])
def test_row_kernel_second_layernorm_forms(D, rows):
    """h = LN2(y) behind y = LN1(x) + pos + tvec (the post-norm followed by the next block's norm1 of the plain flow), as fp32, as
    planes and as bf16 rows.  h against fp64 of LN2 on the kernel's own y: the LayerNorm bound; against fp64 of both norms: y's error
    (at most LN_TOL) passes LN2 with the gain rstd2 |gamma2| <= 1.2 rstd2, rstd2 from the fp64 y."""
    E = _E()
    x, g, b, pos, tv, add = _ln_inputs(rows, D)
    g2 = (1 + 0.2 * hashed("lng2", (D,), 6)).cuda()
    b2 = (0.2 * hashed("lnb2", (D,), 7)).cuda()
    kw = dict(pos=pos, pos_div=17, tvec=tv, rows_per_batch=51, gamma2=g2, beta2=b2, eps2=1e-5)
    yref = F.layer_norm(x.double(), (D,), g.double(), b.double(), EPS) + add
    ln2 = lambda y: F.layer_norm(y, (D,), g2.double(), b2.double(), 1e-5)
    href = ln2(yref)
    a = E.op_layernorm_forms(x, g, b, EPS, outputs=("y", "h"), **kw)
    own = (a["h"].double() - ln2(a["y"].double())).abs().max().item()
    both = (a["h"].double() - href).abs().max().item()
    tol_both = LN_TOL * (1 + 1.2 * (yref.var(1, unbiased=False) + 1e-5).rsqrt().max().item())
    c = E.op_layernorm_forms(x, g, b, EPS, outputs=("y_x3", "stats", "h_x3"), **kw)
    plane = ((c["h_x3"] - a["h"]).abs() / _plane_quantum(a["h"])).max().item()
    d = E.op_layernorm_forms(x, g, b, EPS, outputs=("y", "h_bf16"), **kw)
    hb = d["h_bf16"]
    assert hb.dtype == torch.bfloat16
    ulp = torch.exp2(torch.floor(torch.log2(href.abs().clamp(min=2.0 ** -126))) - 7)      # a bf16 keeps 8 bits
    ok = (hb == a["h"].bfloat16()) | ((hb.double() - href).abs() <= ulp)
    print(f"row kernel LN2 D={D} rows={rows}: h vs LN2 of its y {own:.3e} (tol {LN_TOL:.0e}), vs both norms in fp64 {both:.3e} "
          f"(tol {tol_both:.3e}); h planes {plane:.2f} of the quantum; bf16 rows off torch's rounding: {int((hb != a['h'].bfloat16()).sum())}")
    assert own < LN_TOL and both < tol_both
    assert plane <= 1.0
    assert ok.all()
    assert torch.equal(d["y"], a["y"]) and ((c["y_x3"] - a["y"]).abs() <= _plane_quantum(a["y"])).all()
    assert maxabs(c["stats"][:, 0], yref.sum(1).cpu()) < ST_SUM and maxabs(c["stats"][:, 1], (yref * yref).sum(1).cpu()) < ST_SQ
