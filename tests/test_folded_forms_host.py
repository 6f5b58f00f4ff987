"""Host-side contract of the single-op hooks behind tests/test_gpu_folded_forms.py (include/d3d.h: d3d_op_linear_folded,
d3d_op_linear_plane_residual, d3d_op_layernorm_forms): exported and declared, and every argument refusal -- the checks come before
any device work, so host memory stands in for the (never touched) device pointers.  No GPU needed."""
import ctypes as C
import os
import re

import pytest
import torch

from diff3dhpe_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUP = -1, -5   # D3D_EINVAL, D3D_EUNSUP (include/d3d.h)
HOOKS = ("d3d_op_linear_folded", "d3d_op_linear_plane_residual", "d3d_op_layernorm_forms")


@pytest.fixture(scope="module")
def host():
    buf = (C.c_float * 16)()
    return _lib.lib(), C.cast(buf, C.c_void_p), buf     # (buf keeps the memory alive)


def test_error_code_constants():
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    for name, value in (("D3D_EINVAL", EINVAL), ("D3D_EUNSUP", EUNSUP)):
        m = re.search(r"#define\s+%s\s+\((-?\d+)\)" % name, hdr)
        assert m and int(m.group(1)) == value


def test_hooks_are_exported_declared_and_wrapped():
    from diff3dhpe_amd import engine
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    for name in HOOKS:
        assert hasattr(_lib.lib(), name)
        assert name in _lib.ABI_SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, hdr)
        assert callable(getattr(engine, name[len("d3d_"):]))
    assert _lib.lib().d3d_version() >= 144


def test_folded_hook_refuses_bad_arguments(host):
    L, p, _ = host

    def call(M=64, N=256, K=128, st_np=2, epi=0, qcols=64, eps=1e-6, X=p, st=p, H=p, hi=p, lo=p):
        return L.d3d_op_linear_folded(X, p, p, p, p, eps, st, st_np, epi, qcols, H, hi, lo, M, N, K, None)
    for kw in (dict(M=0), dict(st_np=0), dict(st_np=-1), dict(epi=2), dict(epi=-1), dict(eps=0.0), dict(X=None), dict(st=None)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(N=100), dict(N=64), dict(N=0), dict(K=48), dict(K=0), dict(N=192)):
        assert call(**kw) == EUNSUP, kw
    for kw in (dict(qcols=-64), dict(qcols=320), dict(qcols=32), dict(hi=None), dict(lo=None), dict(epi=1, H=None)):
        assert call(**kw) == EINVAL, kw
    assert b"qcols" in L.d3d_last_error()


def test_plane_residual_hook_refuses_bad_arguments(host):
    L, p, _ = host

    def call(M=64, N=256, K=128, with_stats=1, A=p, R=p, Y=p, stats=p):
        return L.d3d_op_linear_plane_residual(A, p, p, R, Y, stats, with_stats, M, N, K, None)
    for kw in (dict(M=0), dict(A=None), dict(R=None), dict(Y=None), dict(stats=None)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(N=64), dict(N=320), dict(N=0), dict(K=40), dict(K=0), dict(with_stats=0, N=96)):
        assert call(**kw) == EUNSUP, kw


def test_row_kernel_hook_refuses_bad_arguments(host):
    L, p, _ = host

    def call(rows=8, D=64, skip=0, x=p, g1=p, b1=p, pos=None, pos_div=1, pos_mod=1, tvec=None, stride=0, rpb=1, g2=p, b2=p, y=p, yx3=None,
             stats=None, h=None, hx3=None, hbf16=None):
        return L.d3d_op_layernorm_forms(x, g1, b1, 1e-6, skip, pos, pos_div, pos_mod, tvec, stride, rpb, g2, b2, 1e-6, y, yx3, stats, h, hx3,
                                        hbf16, rows, D, None)
    for kw in (dict(rows=0), dict(D=0), dict(x=None), dict(g1=None), dict(b1=None), dict(y=None),            # (y=None: no output at all)
               dict(h=p, hx3=p), dict(h=p, hbf16=p), dict(hx3=p, hbf16=p),                                   # one second-LayerNorm output
               dict(y=None, h=p), dict(h=p, g2=None), dict(hbf16=p, b2=None),                                # h is formed from y, by gamma2 / beta2
               dict(pos=p, pos_div=0), dict(pos=p, pos_mod=0), dict(tvec=p, stride=64, rpb=0)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(D=6), dict(D=2048), dict(D=36, yx3=p), dict(D=36, hx3=p)):
        assert call(**kw) == EUNSUP, kw
    assert call(skip=1, g1=None, b1=None, y=None) == EINVAL          # skip_ln1 needs no gamma1 / beta1, but still an output


def test_wrappers_check_their_own_arguments():
    from diff3dhpe_amd import engine
    z = torch.zeros
    with pytest.raises(ValueError):
        engine.op_linear_folded(z(4, 32), z(128, 32), z(128), z(32), z(32), z(4, 2))            # statistics are (M, st_np, 2)
    with pytest.raises(ValueError):
        engine.op_linear_folded(z(4, 32), z(128, 32), z(128), z(32), z(32), z(5, 1, 2))
    with pytest.raises(KeyError):
        engine.op_linear_folded(z(4, 32), z(128, 32), z(128), z(32), z(32), z(4, 1, 2), epi="residual")
    with pytest.raises(ValueError):
        engine.op_layernorm_forms(z(4, 32), outputs=("y", "h_f16"))
    with pytest.raises(ValueError):
        engine.op_layernorm_forms(z(4, 32), outputs=())


def test_shared_helpers_moved_unchanged():
    """_ROWS / _rows (from test_gpu_ops.py) and _tol (from test_gpu_latency_mode_proj_fc1.py) live in tests/helpers.py."""
    import helpers
    assert set(helpers._ROWS) == {"walk256", "rows128", "rowswalk"}
    assert helpers._ROWS["walk256"](256) == 131172 and helpers._ROWS["rows128"](256) == 32845 and helpers._ROWS["rowswalk"](256) == 131149
    assert helpers._rows(17) == 17
    assert helpers._tol(32) == pytest.approx(5e-6) and helpers._tol(512) == pytest.approx(1.4e-5)
    for fn in ("test_gpu_ops.py", "test_gpu_latency_mode_proj_fc1.py", "test_gpu_folded_forms.py"):
        src = open(os.path.join(ROOT, "tests", fn)).read()
        assert re.search(r"^from helpers import .*\b(_tol|_rows)\b", src, re.M), fn
        assert not re.search(r"^def (_tol|_rows)\(", src, re.M), fn
