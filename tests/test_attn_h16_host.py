"""Host-side contract of head width 16 (include/d3d.h): embed_dim 128 with the runner's 8 heads.  An F16X3 engine whose heads come in quads
runs its attention on kernels_attn_x3_h16.hip / kernels_attn_x3_long.hip (width 16) behind the option "attn_h16"; an FP32 engine runs the
DH = 16 walks of kernels_attn_f32_hx.hip behind "attn_f32_h16".  The op-level exports, the options and info keys, an unchanged workspace
size, the build list, the kernels in the device code, the predicates, unchanged admission.  No GPU needed: engines are created on the host
only."""
import ctypes as C
import os
import re

import pytest

from diff3dhpe_amd import _lib
from diff3dhpe_amd.spec import DenoiserConfig
from host_helpers import create_host_engine, engine_info
from test_abi_host import _device_isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERSION = 147
# precision of the engine an option acts on -> (option, info key)
KEYS = {"f16x3": ("attn_h16", "attn_h16_last"), "fp32": ("attn_f32_h16", "attn_f32_h16_last")}
# (op symbol, Python wrapper, translation unit)
OPS = [("d3d_op_attention_h16", "op_attention_h16", "kernels_attn_x3_h16.hip"),
       ("d3d_op_attention_long_h16", "op_attention_long_h16", "kernels_attn_x3_long.hip"),
       ("d3d_op_attention_f32_h16", "op_attention_f32_h16", "kernels_attn_f32_hx.hip"),
       ("d3d_op_attention_long_f32_h16", "op_attention_long_f32_h16", "kernels_attn_f32_hx.hip")]
CFG = dict(num_frame=243, embed_dim=128, depth=8, num_heads=8)
assert DenoiserConfig(**CFG).head_dim == 16


@pytest.fixture(params=sorted(KEYS))
def host_engine(request):
    """(L, h, option, info key) of a host engine of embed_dim 128 in each of the two precisions, destroyed at teardown."""
    L = _lib.lib()
    h = create_host_engine(request.param, **CFG)
    yield (L, h) + KEYS[request.param]
    L.d3d_engine_destroy(h)


def _create(prec, **kw):
    """(rc, handle) of d3d_engine_create for DenoiserConfig(**kw)."""
    cfg = DenoiserConfig(**kw)
    c = _lib.Config(cfg.num_frame, cfg.num_joints, cfg.in_chans, cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.mlp_hidden,
                    int(cfg.with_time_emb), int(cfg.seq2frame), _lib.PRECISIONS[prec])
    h = C.c_void_p()
    return _lib.lib().d3d_engine_create(C.byref(c), C.byref(h)), h


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("D,H", [(128, 8), (32, 2)])
def test_admission_is_unchanged_admitted(prec, D, H):
    rc, h = _create(prec, num_frame=243, embed_dim=D, depth=8, num_heads=H)
    assert rc == 0, _lib.lib().d3d_last_error()
    _lib.lib().d3d_engine_destroy(h)


def test_admission_is_unchanged_bf16_refused():
    rc, _ = _create("bf16", **CFG)
    assert rc == -5


def _documented_default(key):
    """The default include/d3d.h states for the key: the first number of its entry in the option table."""
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    m = re.search(r'^ \*   "%s"\s+([01]) \(default\) / ([01]):' % re.escape(key), hdr, re.M)
    assert m, f'no \'"{key}"  <v> (default) / <other>:\' entry in the option table of include/d3d.h'
    assert {m.group(1), m.group(2)} == {"0", "1"}
    return int(m.group(1))


def test_both_options_read_the_documented_default_and_round_trip(host_engine):
    """Either engine holds both options (the one of the other precision has no effect on it)."""
    L, h, _, _ = host_engine
    for key, _ in KEYS.values():
        dflt = _documented_default(key)
        assert engine_info(L, h, key) == (0, dflt)
        for v in (1 - dflt, dflt):
            assert L.d3d_engine_set_option(h, key.encode(), v) == 0
            assert engine_info(L, h, key) == (0, v)


def test_both_last_keys_read_zero_before_any_forward(host_engine):
    L, h, _, _ = host_engine
    for key, _ in KEYS.values():
        for v in (1, 0, _documented_default(key)):
            assert L.d3d_engine_set_option(h, key.encode(), v) == 0
            for _, last in KEYS.values():
                assert engine_info(L, h, last) == (0, 0)


def test_workspace_bytes_do_not_depend_on_the_options(host_engine):
    """The kernels read the qkv rows / planes and write the attention rows the launches they replace do: nothing more to allocate."""
    L, h, _, _ = host_engine
    size = {}
    for a in (1, 0):
        for b in (1, 0):
            assert L.d3d_engine_set_option(h, b"attn_h16", a) == 0 and L.d3d_engine_set_option(h, b"attn_f32_h16", b) == 0
            size[a, b] = [L.d3d_workspace_bytes(h, B) for B in (1, 3, 8)]
    for key, _ in KEYS.values():
        assert L.d3d_engine_set_option(h, key.encode(), _documented_default(key)) == 0
    assert all(b > 0 for b in size[1, 1])
    assert len({tuple(v) for v in size.values()}) == 1, size


@pytest.mark.parametrize("symbol,wrapper,unit", OPS, ids=[o[0] for o in OPS])
def test_op_entry_is_exported_declared_and_callable(symbol, wrapper, unit):
    assert hasattr(_lib.lib(), symbol)
    assert symbol in _lib.ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    assert re.search(r"\b%s\s*\(" % symbol, hdr)
    for _, last in KEYS.values():
        assert f'"{last}"' in hdr
    from diff3dhpe_amd import engine
    assert callable(getattr(engine, wrapper))
    assert _lib.lib().d3d_version() >= VERSION


@pytest.mark.parametrize("unit", sorted({o[2] for o in OPS}))
def test_the_translation_units_are_in_the_build_list(unit):
    """tests/test_abi_host.py scans the object file of every entry of SOURCES."""
    from diff3dhpe_amd.build import SOURCES
    assert unit in SOURCES


# object file -> (the MFMA the kernels must be built on, names in the mangled symbols of the new instantiations)
ISA = {"kernels_attn_x3_h16.o": ("v_mfma_f32_32x32x16_f16", ["k_attn_x3_h16ILi%dELi1E" % n for n in range(1, 9)] + ["k_attn_x3_h16ILi1ELi8E"]),
       "kernels_attn_x3_long.o": ("v_mfma_f32_32x32x16_f16", ["k_attn_x3_streamILi16ELi8E"]),
       "kernels_attn_f32_hx.o": ("v_mfma_f32_32x32x2_f32", ["k_attn_f32_hxILi16ELi%dE" % n for n in range(1, 9)] + ["k_attn_f32_hx_streamILi16E"])}


@pytest.mark.parametrize("obj", sorted(ISA))
def test_the_device_code_holds_the_kernels_on_their_mfma(obj):
    """Every new instantiation is in the gfx950 code object, and its body holds the MFMA it is written around."""
    mfma, names = ISA[obj]
    isa = _device_isa(obj)
    bodies = re.split(r"^[0-9a-f]+ <([^>]+)>:$", isa, flags=re.M)      # [junk, symbol, body, symbol, body, ...]
    by_symbol = dict(zip(bodies[1::2], bodies[2::2]))
    for name in names:
        hits = [s for s in by_symbol if name in s]
        assert hits, f"{name}: no such kernel in {obj}"
        for s in hits:
            assert mfma in by_symbol[s], f"{s}: no {mfma}"


def _cxx(name, nargs):
    """A host predicate of the library through its C++ symbol, as tests/test_attn_hx_host.py reaches them."""
    f = getattr(_lib.lib(), f"_ZN3d3d{len(name)}{name}E" + "i" * nargs)
    f.restype, f.argtypes = C.c_bool, [C.c_int] * nargs
    return f


def test_predicates_f16x3():
    res, lng = _cxx("attn_x3_h16_ok", 3), _cxx("attn_x3_h16_long_ok", 3)
    for H in (4, 8):
        for N in (1, 17, 27, 33, 243, 256):
            assert res(N, 16 * H, H) and lng(N, 16 * H, H), (N, H)
        for N in (257, 300, 100000):
            assert not res(N, 16 * H, H) and lng(N, 16 * H, H), (N, H)
        assert not res(0, 16 * H, H) and not lng(0, 16 * H, H)
        for N in (1, 27, 256, 300):
            for D in (32 * H, 48 * H, 64 * H):
                assert not res(N, D, H) and not lng(N, D, H), (N, D, H)
    for H in (1, 2, 3, 6):                                       # heads of 16 columns that do not come in quads
        for N in (1, 27, 256, 300):
            assert not res(N, 16 * H, H) and not lng(N, 16 * H, H), (N, H)
    assert not res(27, 0, 0) and not lng(27, 0, 0)


def test_predicates_fp32():
    res, lng = _cxx("attn_f32_h16_ok", 3), _cxx("attn_f32_h16_long_ok", 3)
    for H in (1, 2, 3, 8):
        for N in (1, 17, 27, 33, 243, 256):
            assert res(N, 16 * H, H) and lng(N, 16 * H, H), (N, H)
        for N in (257, 300, 100000):
            assert not res(N, 16 * H, H) and lng(N, 16 * H, H), (N, H)
        assert not res(0, 16 * H, H) and not lng(0, 16 * H, H)
        for N in (1, 27, 256, 300):
            for D in (32 * H, 48 * H, 64 * H):
                assert not res(N, D, H) and not lng(N, D, H), (N, D, H)
    assert not res(27, 0, 0) and not lng(27, 0, 0)
