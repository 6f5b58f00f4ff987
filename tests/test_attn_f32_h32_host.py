"""Host-side contract of "attn_f32_h32" (include/d3d.h): FP32 engines whose heads are 32 columns wide (embed_dim 256 with 8 heads) run
their attention on kernels_attn_f32_h32.hip.  The option and info keys, the op-level export, an unchanged workspace size, the build list,
the predicates.  No GPU needed: engines are created on the host only."""
import ctypes as C
import os
import re

from diff3dhpe_amd import _lib
from diff3dhpe_amd.spec import DenoiserConfig
from host_helpers import engine_info, host_engine_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY, LAST = b"attn_f32_h32", "attn_f32_h32_last"


def _documented_default():
    """The default include/d3d.h states for the key: the first number of its entry in the option table."""
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    m = re.search(r'^ \*   "attn_f32_h32"\s+([01]) \(default\) / ([01]):', hdr, re.M)
    assert m, 'no \'"attn_f32_h32"  <v> (default) / <other>:\' entry in the option table of include/d3d.h'
    assert {m.group(1), m.group(2)} == {"0", "1"}
    return int(m.group(1))


CFG = dict(num_frame=243, embed_dim=256, depth=8)
assert DenoiserConfig(**CFG).num_heads == 8 and DenoiserConfig(**CFG).head_dim == 32
host_engine = host_engine_fixture(**CFG, prec="fp32")


def test_option_reads_the_documented_default_and_round_trips(host_engine):
    L, h = host_engine
    dflt = _documented_default()
    assert engine_info(L, h, KEY.decode()) == (0, dflt)
    for v in (1 - dflt, dflt):
        assert L.d3d_engine_set_option(h, KEY, v) == 0
        assert engine_info(L, h, KEY.decode()) == (0, v)


def test_last_reads_zero_before_any_forward(host_engine):
    L, h = host_engine
    for v in (1, 0):
        assert L.d3d_engine_set_option(h, KEY, v) == 0
        assert engine_info(L, h, LAST) == (0, 0)


def test_workspace_bytes_do_not_depend_on_the_option(host_engine):
    """The kernels read the qkv rows and write the attention rows the generic kernel does: nothing more to allocate."""
    L, h = host_engine
    size = {}
    for v in (1, 0):
        assert L.d3d_engine_set_option(h, KEY, v) == 0
        size[v] = [L.d3d_workspace_bytes(h, B) for B in (1, 3, 8)]
    assert all(b > 0 for b in size[1])
    assert size[1] == size[0]


def test_op_entry_is_exported_declared_and_callable():
    assert hasattr(_lib.lib(), "d3d_op_attention_f32_h32")
    assert "d3d_op_attention_f32_h32" in _lib.ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    assert re.search(r"\bd3d_op_attention_f32_h32\s*\(", hdr)
    assert '"attn_f32_h32_last"' in hdr
    from diff3dhpe_amd import engine
    assert callable(engine.op_attention_f32_h32)
    assert _lib.lib().d3d_version() >= 140


def test_the_new_translation_unit_is_in_the_build_list():
    """tests/test_abi_host.py scans the object file of every entry of SOURCES for the packed fp32 form no attention file may hold."""
    from diff3dhpe_amd.build import SOURCES
    assert "kernels_attn_f32_h32.hip" in SOURCES


def _cxx(name, nargs):
    """A host predicate of the library through its C++ symbol, as tests/test_group_lengths_host.py reaches them."""
    f = getattr(_lib.lib(), f"_ZN3d3d{len(name)}{name}E" + "i" * nargs)
    f.restype, f.argtypes = C.c_bool, [C.c_int] * nargs
    return f


def test_predicates():
    tp, sp = _cxx("attn_temporal_f32_h32_ok", 3), _cxx("attn_spatial_f32_h32_ok", 3)
    for T, D, H in ((1, 256, 8), (256, 256, 8), (27, 96, 3)):
        assert tp(T, D, H), (T, D, H)
    for J in (15, 16, 17):
        assert sp(J, 256, 8), J
    for T, D, H in ((0, 256, 8), (257, 256, 8), (27, 512, 8)):
        assert not tp(T, D, H), (T, D, H)
    for J, D, H in ((14, 256, 8), (18, 256, 8), (17, 512, 8)):
        assert not sp(J, D, H), (J, D, H)
