"""Host-side contract of "attn_f32_h128" (include/d3d.h): FP32 engines whose heads are 128 columns wide (embed_dim 1024 with 8 heads) run
their attention on kernels_attn_f32_h128.hip.  The option and info keys, the op-level exports, an unchanged workspace size, the build
list, the predicates.  No GPU needed: engines are created on the host only."""
import ctypes as C
import os
import re

import pytest

from diff3dhpe_amd import _lib
from diff3dhpe_amd.spec import DenoiserConfig
from host_helpers import engine_info, host_engine_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY, LAST = "attn_f32_h128", "attn_f32_h128_last"
VERSION = 143
UNIT = "kernels_attn_f32_h128.hip"
# (op symbol, Python wrapper)
OPS = [("d3d_op_attention_f32_h128", "op_attention_f32_h128"), ("d3d_op_attention_long_f32_h128", "op_attention_long_f32_h128")]
CFG = dict(num_frame=243, embed_dim=1024, depth=8, num_heads=8)
assert DenoiserConfig(**CFG).head_dim == 128

host_engine = host_engine_fixture(prec="fp32", **CFG)


def _documented_default():
    """The default include/d3d.h states for the key: the first number of its entry in the option table."""
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    m = re.search(r'^ \*   "%s"\s+([01]) \(default\) / ([01]):' % re.escape(KEY), hdr, re.M)
    assert m, f'no \'"{KEY}"  <v> (default) / <other>:\' entry in the option table of include/d3d.h'
    assert {m.group(1), m.group(2)} == {"0", "1"}
    return int(m.group(1))


def test_option_reads_the_documented_default_and_round_trips(host_engine):
    L, h = host_engine
    dflt = _documented_default()
    assert engine_info(L, h, KEY) == (0, dflt)
    for v in (1 - dflt, dflt):
        assert L.d3d_engine_set_option(h, KEY.encode(), v) == 0
        assert engine_info(L, h, KEY) == (0, v)


def test_last_reads_zero_before_any_forward(host_engine):
    L, h = host_engine
    for v in (1, 0):
        assert L.d3d_engine_set_option(h, KEY.encode(), v) == 0
        assert engine_info(L, h, LAST) == (0, 0)


def test_workspace_bytes_do_not_depend_on_the_option(host_engine):
    """The kernels read the qkv rows and write the attention rows the generic kernel does: nothing more to allocate."""
    L, h = host_engine
    size = {}
    for v in (1, 0):
        assert L.d3d_engine_set_option(h, KEY.encode(), v) == 0
        size[v] = [L.d3d_workspace_bytes(h, B) for B in (1, 3, 8)]
    assert all(b > 0 for b in size[1])
    assert size[1] == size[0]


@pytest.mark.parametrize("symbol,wrapper", OPS, ids=[o[0] for o in OPS])
def test_op_entry_is_exported_declared_and_callable(symbol, wrapper):
    assert hasattr(_lib.lib(), symbol)
    assert symbol in _lib.ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    assert re.search(r"\b%s\s*\(" % symbol, hdr)
    assert f'"{LAST}"' in hdr
    from diff3dhpe_amd import engine
    assert callable(getattr(engine, wrapper))
    assert _lib.lib().d3d_version() >= VERSION


def test_the_new_translation_unit_is_in_the_build_list():
    """tests/test_abi_host.py scans the object file of every entry of SOURCES for the packed fp32 form no attention file may hold."""
    from diff3dhpe_amd.build import SOURCES
    assert UNIT in SOURCES


def _cxx(name, nargs):
    """A host predicate of the library through its C++ symbol, as tests/test_group_lengths_host.py reaches them."""
    f = getattr(_lib.lib(), f"_ZN3d3d{len(name)}{name}E" + "i" * nargs)
    f.restype, f.argtypes = C.c_bool, [C.c_int] * nargs
    return f


def test_predicates():
    res, lng = _cxx("attn_f32_h128_ok", 3), _cxx("attn_f32_h128_long_ok", 3)
    for N, D, H in ((1, 1024, 8), (128, 1024, 8), (17, 128, 1)):
        assert res(N, D, H) and lng(N, D, H), (N, D, H)
    for N, D, H in ((0, 1024, 8), (0, 128, 1), (129, 1024, 8), (27, 512, 8), (27, 256, 8)):
        assert not res(N, D, H), (N, D, H)
    for T in (129, 243, 513):
        assert lng(T, 1024, 8) and not res(T, 1024, 8), T
    for T, D, H in ((0, 1024, 8), (243, 512, 8), (27, 512, 8), (300, 64, 1), (27, 256, 8)):
        assert not lng(T, D, H), (T, D, H)
