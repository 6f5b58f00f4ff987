"""Host-side contract of head width 128 (include/d3d.h): embed_dim 1024 with the runner's 8 heads is admitted in FP32 and F16X3, an F16X3
engine of that width runs its attention on kernels_attn_x3_h128.hip / kernels_attn_x3_long.hip (width 128) behind the option "attn_h128".
Admission and refusals, the weight inventory, the option and info keys, the op-level exports, an unchanged workspace size, the build list,
the predicates.  No GPU needed: engines are created on the host only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from diff3dhpe_amd import _lib
from diff3dhpe_amd.spec import DenoiserConfig, denoiser_param_spec
from host_helpers import create_host_engine, engine_info, host_engine_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY, LAST = "attn_h128", "attn_h128_last"
VERSION = 142
# (op symbol, Python wrapper, translation unit)
OPS = [("d3d_op_attention_h128", "op_attention_h128", "kernels_attn_x3_h128.hip"),
       ("d3d_op_attention_long_h128", "op_attention_long_h128", "kernels_attn_x3_long.hip")]
CFG = dict(num_frame=243, embed_dim=1024, depth=8, num_heads=8)
assert DenoiserConfig(**CFG).head_dim == 128

host_engine = host_engine_fixture(prec="f16x3", **CFG)


def _create(prec, **kw):
    """(rc, handle) of d3d_engine_create for DenoiserConfig(**kw)."""
    cfg = DenoiserConfig(**kw)
    c = _lib.Config(cfg.num_frame, cfg.num_joints, cfg.in_chans, cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.mlp_hidden,
                    int(cfg.with_time_emb), int(cfg.seq2frame), _lib.PRECISIONS[prec])
    h = C.c_void_p()
    return _lib.lib().d3d_engine_create(C.byref(c), C.byref(h)), h


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("D,H", [(1024, 8), (128, 1)])
def test_head_width_128_is_admitted(prec, D, H):
    rc, h = _create(prec, num_frame=243, embed_dim=D, depth=8, num_heads=H)
    assert rc == 0, _lib.lib().d3d_last_error()
    _lib.lib().d3d_engine_destroy(h)


def test_bf16_stays_refused_at_this_width():
    rc, _ = _create("bf16", **CFG)
    assert rc == -5
    assert b"BF16" in _lib.lib().d3d_last_error()


def test_head_width_256_stays_refused():
    rc, _ = _create("f16x3", num_frame=243, embed_dim=1024, depth=8, num_heads=4)
    assert rc == -5
    assert b"128" in _lib.lib().d3d_last_error()      # the message names the widest admitted width
    rc, _ = _create("fp32", num_frame=243, embed_dim=1024, depth=8, num_heads=4)
    assert rc == -5


def test_weight_inventory_matches_the_spec(host_engine):
    L, h = host_engine
    cfg = DenoiserConfig(**CFG)
    names = []
    for i in range(L.d3d_engine_num_weights(h)):
        name, n = C.c_char_p(), C.c_int64()
        assert L.d3d_engine_weight_info(h, i, C.byref(name), C.byref(n)) == 0
        names.append((name.value.decode(), n.value))
    assert names == [(n, int(np.prod(s))) for n, s, _, _ in denoiser_param_spec(cfg)]


def _documented_default(key):
    """The default include/d3d.h states for the key: the first number of its entry in the option table."""
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    m = re.search(r'^ \*   "%s"\s+([01]) \(default\) / ([01]):' % re.escape(key), hdr, re.M)
    assert m, f'no \'"{key}"  <v> (default) / <other>:\' entry in the option table of include/d3d.h'
    assert {m.group(1), m.group(2)} == {"0", "1"}
    return int(m.group(1))


def test_option_reads_the_documented_default_and_round_trips(host_engine):
    L, h = host_engine
    dflt = _documented_default(KEY)
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
    """The kernels read the qkv planes and write the attention rows the launches they replace do: nothing more to allocate."""
    L, h = host_engine
    size = {}
    for v in (1, 0):
        assert L.d3d_engine_set_option(h, KEY.encode(), v) == 0
        size[v] = [L.d3d_workspace_bytes(h, B) for B in (1, 3, 8)]
    assert all(b > 0 for b in size[1])
    assert size[1] == size[0]


@pytest.mark.parametrize("symbol,wrapper,unit", OPS, ids=[o[0] for o in OPS])
def test_op_entry_is_exported_declared_and_callable(symbol, wrapper, unit):
    assert hasattr(_lib.lib(), symbol)
    assert symbol in _lib.ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    assert re.search(r"\b%s\s*\(" % symbol, hdr)
    assert f'"{LAST}"' in hdr
    from diff3dhpe_amd import engine
    assert callable(getattr(engine, wrapper))
    assert _lib.lib().d3d_version() >= VERSION


@pytest.mark.parametrize("unit", [o[2] for o in OPS])
def test_the_new_translation_units_are_in_the_build_list(unit):
    """tests/test_abi_host.py scans the object file of every entry of SOURCES."""
    from diff3dhpe_amd.build import SOURCES
    assert unit in SOURCES


def _cxx(name, nargs):
    """A host predicate of the library through its C++ symbol, as tests/test_group_lengths_host.py reaches them."""
    f = getattr(_lib.lib(), f"_ZN3d3d{len(name)}{name}E" + "i" * nargs)
    f.restype, f.argtypes = C.c_bool, [C.c_int] * nargs
    return f


def test_predicates():
    res, lng = _cxx("attn_x3_h128_ok", 3), _cxx("attn_x3_h128_long_ok", 3)
    for N, D, H in ((1, 1024, 8), (17, 1024, 8), (128, 1024, 8), (100, 128, 1), (33, 256, 2), (81, 384, 3)):
        assert res(N, D, H) and lng(N, D, H), (N, D, H)
    for N, D, H in ((129, 1024, 8), (243, 1024, 8), (100000, 128, 1)):
        assert not res(N, D, H) and lng(N, D, H), (N, D, H)
    for N, D, H in ((0, 1024, 8), (27, 512, 8), (27, 256, 8), (27, 1024, 4), (27, 1024, 16), (27, 96, 3), (27, 0, 0)):
        assert not res(N, D, H) and not lng(N, D, H), (N, D, H)
