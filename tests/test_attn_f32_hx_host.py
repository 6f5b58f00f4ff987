"""Host-side contract of "attn_f32_hx" (include/d3d.h): FP32 engines whose heads are 48 or 96 columns wide (embed_dim 384 / 768 with 8
heads) run their attention on kernels_attn_f32_hx.hip.  The option and info keys, the op-level exports, an unchanged workspace size, the
build list, the predicates.  No GPU needed: engines are created on the host only."""
import ctypes as C
import os
import re

import pytest

from diff3dhpe_amd import _lib
from diff3dhpe_amd.spec import DenoiserConfig
from host_helpers import create_host_engine, engine_info

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY, LAST = "attn_f32_hx", "attn_f32_hx_last"
VERSION = 146
UNIT = "kernels_attn_f32_hx.hip"
# (op symbol, Python wrapper)
OPS = [("d3d_op_attention_f32_hx", "op_attention_f32_hx"), ("d3d_op_attention_long_f32_hx", "op_attention_long_f32_hx")]
CFGS = {"384": dict(num_frame=243, embed_dim=384, depth=8, num_heads=8), "768": dict(num_frame=243, embed_dim=768, depth=8, num_heads=8)}
assert DenoiserConfig(**CFGS["384"]).head_dim == 48 and DenoiserConfig(**CFGS["768"]).head_dim == 96


@pytest.fixture(params=sorted(CFGS))
def host_engine(request):
    """(L, h) of an FP32 host engine of each of the two widths, destroyed at teardown."""
    L = _lib.lib()
    h = create_host_engine("fp32", **CFGS[request.param])
    yield L, h
    L.d3d_engine_destroy(h)


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
    res, lng = _cxx("attn_f32_hx_ok", 3), _cxx("attn_f32_hx_long_ok", 3)
    for N, D, H in ((1, 384, 8), (256, 384, 8), (1, 768, 8), (192, 768, 8), (17, 48, 1), (17, 96, 1), (256, 144, 3), (192, 288, 3)):
        assert res(N, D, H) and lng(N, D, H), (N, D, H)
    for N, D, H in ((0, 384, 8), (0, 768, 8), (0, 48, 1), (257, 384, 8), (193, 768, 8), (256, 768, 8),
                    (27, 256, 8), (27, 512, 8), (27, 1024, 8), (27, 32, 1), (27, 64, 1), (27, 128, 1), (27, 0, 0)):
        assert not res(N, D, H), (N, D, H)
    for T in (1, 27, 192, 193, 243, 256, 257, 513, 100000):          # any T >= 1 at these widths
        for D, H in ((384, 8), (768, 8), (48, 1), (96, 1)):
            assert lng(T, D, H), (T, D, H)
    for T in (193, 243, 256, 257, 513):
        assert not res(T, 768, 8), T
    for T in (257, 300, 513):
        assert not res(T, 384, 8), T
    for T, D, H in ((0, 384, 8), (0, 768, 8), (243, 256, 8), (243, 512, 8), (27, 512, 8), (243, 1024, 8), (300, 64, 1), (27, 0, 0)):
        assert not lng(T, D, H), (T, D, H)
