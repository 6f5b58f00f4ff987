"""Host-side contract of "long_temporal_h32" and "long_temporal_f32_h32" (include/d3d.h): engines whose heads are 32 columns wide
(embed_dim 256 with 8 heads) and whose window is longer than 256 frames run their temporal blocks on kernels_attn_x3_long.hip at width 32
(F16X3) / kernels_attn_f32_h32_long.hip (FP32).  The option and info keys, the op-level exports, an unchanged workspace size, the build list, the
predicates.  No GPU needed: engines are created on the host only."""
import ctypes as C
import os
import re

import pytest

from diff3dhpe_amd import _lib
from diff3dhpe_amd.spec import DenoiserConfig
from host_helpers import create_host_engine, engine_info

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (option key, engine precision, op symbol, Python wrapper, translation unit)
FEATURES = [("long_temporal_h32", "f16x3", "d3d_op_attention_long_h32", "op_attention_long_h32", "kernels_attn_x3_long.hip"),
            ("long_temporal_f32_h32", "fp32", "d3d_op_attention_long_f32_h32", "op_attention_long_f32_h32", "kernels_attn_f32_h32_long.hip")]
KEYS = [(f[0], f[1]) for f in FEATURES]
CFG = dict(num_frame=300, embed_dim=256, depth=8)
assert DenoiserConfig(**CFG).num_heads == 8 and DenoiserConfig(**CFG).head_dim == 32


def _documented_default(key):
    """The default include/d3d.h states for the key: the first number of its entry in the option table."""
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    m = re.search(r'^ \*   "%s"\s+([01]) \(default\) / ([01]):' % re.escape(key), hdr, re.M)
    assert m, f'no \'"{key}"  <v> (default) / <other>:\' entry in the option table of include/d3d.h'
    assert {m.group(1), m.group(2)} == {"0", "1"}
    return int(m.group(1))


@pytest.fixture(params=KEYS, ids=[k for k, _ in KEYS])
def keyed_engine(request):
    key, prec = request.param
    L = _lib.lib()
    h = create_host_engine(prec, **CFG)
    yield L, h, key
    L.d3d_engine_destroy(h)


def test_option_reads_the_documented_default_and_round_trips(keyed_engine):
    L, h, key = keyed_engine
    dflt = _documented_default(key)
    assert engine_info(L, h, key) == (0, dflt)
    for v in (1 - dflt, dflt):
        assert L.d3d_engine_set_option(h, key.encode(), v) == 0
        assert engine_info(L, h, key) == (0, v)


def test_last_reads_zero_before_any_forward(keyed_engine):
    L, h, key = keyed_engine
    for v in (1, 0):
        assert L.d3d_engine_set_option(h, key.encode(), v) == 0
        assert engine_info(L, h, key + "_last") == (0, 0)


def test_workspace_bytes_do_not_depend_on_the_option(keyed_engine):
    """The kernels read the qkv planes / rows and write the attention rows the launches they replace do: nothing more to allocate."""
    L, h, key = keyed_engine
    size = {}
    for v in (1, 0):
        assert L.d3d_engine_set_option(h, key.encode(), v) == 0
        size[v] = [L.d3d_workspace_bytes(h, B) for B in (1, 3, 8)]
    assert all(b > 0 for b in size[1])
    assert size[1] == size[0]


@pytest.mark.parametrize("key,prec,symbol,wrapper,unit", FEATURES, ids=[f[0] for f in FEATURES])
def test_op_entry_is_exported_declared_and_callable(key, prec, symbol, wrapper, unit):
    assert hasattr(_lib.lib(), symbol)
    assert symbol in _lib.ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    assert re.search(r"\b%s\s*\(" % symbol, hdr)
    assert f'"{key}_last"' in hdr
    from diff3dhpe_amd import engine
    assert callable(getattr(engine, wrapper))
    assert _lib.lib().d3d_version() >= 141


@pytest.mark.parametrize("unit", [f[4] for f in FEATURES])
def test_the_new_translation_units_are_in_the_build_list(unit):
    """tests/test_abi_host.py scans the object file of every entry of SOURCES for the packed fp32 form no attention file may hold."""
    from diff3dhpe_amd.build import SOURCES
    assert unit in SOURCES


def _cxx(name, nargs):
    """A host predicate of the library through its C++ symbol, as tests/test_group_lengths_host.py reaches them."""
    f = getattr(_lib.lib(), f"_ZN3d3d{len(name)}{name}E" + "i" * nargs)
    f.restype, f.argtypes = C.c_bool, [C.c_int] * nargs
    return f


def test_predicates():
    x3, f32 = _cxx("attn_x3_h32_long_ok", 3), _cxx("attn_temporal_f32_h32_long_ok", 3)
    for T, D, H in ((1, 256, 8), (256, 256, 8), (257, 256, 8), (100000, 64, 2)):
        assert x3(T, D, H) and f32(T, D, H), (T, D, H)
    for T, D, H in ((0, 256, 8), (300, 512, 8), (300, 256, 4)):
        assert not x3(T, D, H) and not f32(T, D, H), (T, D, H)
    # odd head counts: the F16X3 kernel works on head pairs, the fp32 one on single heads
    assert not x3(300, 96, 3) and f32(300, 96, 3)
    assert not x3(300, 32, 1) and f32(300, 32, 1)
