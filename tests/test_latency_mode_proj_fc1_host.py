"""Host-side contract of "latency_mode" for proj and fc1 (include/d3d.h, d3d_kernels.h): the two rules, the forced-S option keys, the
info keys, the op-level exports and their shape predicates.  No GPU needed: the rules are plain host functions of the library (reached
through their C++ symbols), engines are created on the host only, and the op hooks refuse a shape before they touch the device."""
import ctypes as C
from functools import partial
import os
import re

import pytest

from diff3dhpe_amd import _lib
from host_helpers import engine_info, host_engine_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EUNSUP = -5   # D3D_EUNSUP (include/d3d.h)


def _rule(name):
    """d3d::<name>(int M, int N, int K, int n_cu) of d3d_kernels.h (Itanium mangling: _ZN3d3d<len><name>Eiiii)."""
    f = getattr(_lib.lib(), f"_ZN3d3d{len(name)}{name}Eiiii")
    f.restype, f.argtypes = C.c_int, [C.c_int] * 4
    return f


RULES = [("proj_splitk_choose", 512, 512), ("fc1_splitk_choose", 1024, 512)]
MS = [1, 17, 130, 459, 918, 1377, 1836, 2754, 4131, 5508, 8262, 16524, 264384]
CUS = [1, 8, 64, 104, 256, 304]


host_engine = host_engine_fixture(num_frame=243, embed_dim=512, depth=8)
_info = partial(engine_info, sentinel=-99)     # -1 is a value these keys hold


def test_error_code_constant():
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    m = re.search(r"#define\s+D3D_EUNSUP\s+\((-?\d+)\)", hdr)
    assert m and int(m.group(1)) == EUNSUP


@pytest.mark.parametrize("name,N,K", RULES)
def test_rule_is_deterministic_and_returns_0_2_or_4(name, N, K):
    f = _rule(name)
    for cu in CUS:
        for M in MS:
            a = f(M, N, K, cu)
            assert a in (0, 2, 4), (name, M, cu, a)
            assert all(f(M, N, K, cu) == a for _ in range(3))
    assert f(0, N, K, 256) == 0 and f(-5, N, K, 256) == 0 and f(459, N, K, 0) == 0


@pytest.mark.parametrize("name,N,K", RULES)
def test_rule_keeps_the_present_kernels_at_the_headline_shape(name, N, K):
    f = _rule(name)
    for cu in CUS:
        assert f(64 * 243 * 17, N, K, cu) == 0


@pytest.mark.parametrize("name,N,K", RULES)
def test_rule_never_leaves_fewer_than_four_k_tiles(name, N, K):
    """K / 32 / S >= 4.  Depths that give fewer for every S (K <= 224) return 0 at every M; so do widths outside the D = 512 flow."""
    f = _rule(name)
    for k in (32, 64, 128, 192, 224):
        for M in MS:
            assert f(M, N, k, 256) == 0, (name, M, k)
    for k in (256, 384, 512, 1024):
        for M in MS:
            s = f(M, N, k, 256)
            assert s == 0 or (k // 32) // s >= 4, (name, M, k, s)
    assert f(459, 64, 64, 256) == 0


@pytest.mark.parametrize("name,N,K", RULES)
def test_rule_never_exceeds_two_workgroups_per_cu(name, N, K):
    f = _rule(name)
    for cu in CUS:
        for M in MS:
            s = f(M, N, K, cu)
            if s:
                assert ((M + 127) // 128) * (N // 128) * s <= 2 * cu, (name, M, cu, s)
    # a shape at which every split form is beyond 2 x CUs
    assert f(4131, N, K, 8) == 0 and f(459, N, K, 1) == 0


def test_fc1_rule_respects_the_scratch_bound():
    f = _rule("fc1_splitk_choose")
    for cu in (256, 304, 1024, 4096):
        for M in MS:
            s = f(M, 1024, 512, cu)
            assert M * s <= 8192, (M, cu, s)


def test_option_and_info_keys(host_engine):
    L, h = host_engine
    for key in ("proj_split_last", "fc1_split_last"):
        assert _info(L, h, key) == (0, 0)
    for key in ("proj_split", "fc1_split"):
        assert _info(L, h, key) == (0, -1)                               # the rule by default
        for v in (0, 2, 4, -1):
            assert L.d3d_engine_set_option(h, key.encode(), v) == 0
            assert _info(L, h, key) == (0, v)
        assert L.d3d_engine_set_option(h, key.encode(), 3) == EUNSUP
        assert L.d3d_engine_set_option(h, key.encode(), 8) == EUNSUP   # K = 512: 16 k-tiles / 8 = 2 < 4
        assert L.d3d_engine_set_option(h, key.encode(), 1) == EUNSUP
        assert _info(L, h, key) == (0, -1)                               # a refused value changes nothing
    assert L.d3d_engine_set_option(h, b"latency_mode", 1) == 0
    for key in ("proj_split_last", "fc1_split_last"):
        assert _info(L, h, key) == (0, 0)                                # nothing ran yet
    assert L.d3d_engine_set_option(h, b"latency_mode", 0) == 0


def test_workspace_bytes_do_not_depend_on_the_options(host_engine):
    L, h = host_engine
    before = [L.d3d_workspace_bytes(h, B) for B in (1, 2, 4, 64)]
    assert L.d3d_engine_set_option(h, b"latency_mode", 1) == 0
    assert L.d3d_engine_set_option(h, b"proj_split", 4) == 0
    assert L.d3d_engine_set_option(h, b"fc1_split", 4) == 0
    assert [L.d3d_workspace_bytes(h, B) for B in (1, 2, 4, 64)] == before
    assert L.d3d_engine_set_option(h, b"latency_mode", 0) == 0
    assert [L.d3d_workspace_bytes(h, B) for B in (1, 2, 4, 64)] == before


def test_op_entries_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    for name in ("d3d_op_linear_splitk_residual", "d3d_op_linear_splitk_gelu"):
        assert hasattr(_lib.lib(), name)
        assert name in _lib.ABI_SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, hdr)
    for key in ("proj_split_last", "fc1_split_last", '"proj_split"', '"fc1_split"'):
        assert key in hdr


def test_op_hooks_reject_shapes_outside_their_predicate():
    """The shape check comes before any device work: host memory stands in for the (never touched) device pointers."""
    L = _lib.lib()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    ms = C.c_float(0)

    def res(M, N, K, S):
        return L.d3d_op_linear_splitk_residual(p, p, p, p, p, None, M, N, K, S, p, 1, C.byref(ms), None)

    def gelu(M, N, K, S):
        return L.d3d_op_linear_splitk_gelu(p, p, p, p, p, 1e-6, p, M, N, K, S, p, 1, C.byref(ms), None)
    for M, N, K, S in ((64, 256, 512, 2), (64, 512, 512, 3), (64, 512, 512, 8), (64, 512, 128, 2), (64, 512, 500, 2), (64, 512, 512, 1)):
        assert res(M, N, K, S) == EUNSUP, (M, N, K, S)
    for M, N, K, S in ((64, 1000, 512, 2), (64, 1024, 512, 3), (64, 1024, 512, 8), (64, 1024, 128, 2), (64, 1024, 480, 2), (64, 256, 512, 2)):
        assert gelu(M, N, K, S) == EUNSUP, (M, N, K, S)


def test_new_translation_unit_is_built_like_the_other_row_kernels():
    """tests/test_abi_host.py scans every object file of diff3dhpe_amd.build.SOURCES for the packed-fp32 form: the new file must be in
    that list, built without the SLP vectoriser."""
    from diff3dhpe_amd.build import SOURCES, EXTRA_FLAGS
    assert "kernels_splitk_reduce.hip" in SOURCES
    assert EXTRA_FLAGS.get("kernels_splitk_reduce.hip") == EXTRA_FLAGS.get("kernels_fc2_splitk.hip")
    assert "-fno-slp-vectorize" in EXTRA_FLAGS["kernels_splitk_reduce.hip"]
