"""Host-side contract of head widths 48 and 96 (include/d3d.h): embed_dim 384 and 768 with the runner's 8 heads are admitted in FP32 and
F16X3, an F16X3 engine of these widths runs its attention on kernels_attn_x3_hx.hip / kernels_attn_x3_long.hip (widths 48 and 96) behind
the option "attn_hx".  Admission and refusals, the weight inventory, the option and info keys, the op-level exports, an unchanged
workspace size, the build list, the predicates.  No GPU needed: engines are created on the host only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from diff3dhpe_amd import _lib
from diff3dhpe_amd.spec import DenoiserConfig, denoiser_param_spec
from host_helpers import create_host_engine, engine_info

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY, LAST = "attn_hx", "attn_hx_last"
VERSION = 145
# (op symbol, Python wrapper, translation unit)
OPS = [("d3d_op_attention_hx", "op_attention_hx", "kernels_attn_x3_hx.hip"),
       ("d3d_op_attention_long_hx", "op_attention_long_hx", "kernels_attn_x3_long.hip")]
CFG48 = dict(num_frame=243, embed_dim=384, depth=8, num_heads=8)
CFG96 = dict(num_frame=243, embed_dim=768, depth=8, num_heads=8)
assert DenoiserConfig(**CFG48).head_dim == 48 and DenoiserConfig(**CFG96).head_dim == 96

CFGS = {"384": CFG48, "768": CFG96}


@pytest.fixture(params=sorted(CFGS))
def host_engine(request):
    """(L, h, cfg) of an F16X3 host engine of each of the two widths, destroyed at teardown."""
    L = _lib.lib()
    h = create_host_engine("f16x3", **CFGS[request.param])
    yield L, h, DenoiserConfig(**CFGS[request.param])
    L.d3d_engine_destroy(h)


def _create(prec, **kw):
    """(rc, handle) of d3d_engine_create for DenoiserConfig(**kw)."""
    cfg = DenoiserConfig(**kw)
    c = _lib.Config(cfg.num_frame, cfg.num_joints, cfg.in_chans, cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.mlp_hidden,
                    int(cfg.with_time_emb), int(cfg.seq2frame), _lib.PRECISIONS[prec])
    h = C.c_void_p()
    return _lib.lib().d3d_engine_create(C.byref(c), C.byref(h)), h


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("D,H", [(384, 8), (768, 8), (48, 1), (96, 1)])
def test_head_widths_48_and_96_are_admitted(prec, D, H):
    """(48, 1): embed_dim 48 is a multiple of 16 alone.  Admitted with heads of 48 columns; such an engine runs the FP32 kernels in both
    precisions (include/d3d.h; tests/test_gpu_attn_hx_engine.py runs it)."""
    rc, h = _create(prec, num_frame=243, embed_dim=D, depth=8, num_heads=H)
    assert rc == 0, _lib.lib().d3d_last_error()
    _lib.lib().d3d_engine_destroy(h)


@pytest.mark.parametrize("cfg", [CFG48, CFG96], ids=["384", "768"])
def test_bf16_stays_refused_at_these_widths(cfg):
    rc, _ = _create("bf16", **cfg)
    assert rc == -5
    assert b"BF16" in _lib.lib().d3d_last_error() and b"head_dim 64" in _lib.lib().d3d_last_error()


@pytest.mark.parametrize("D,H", [(640, 8), (896, 8), (192, 8), (1024, 4)], ids=["80", "112", "24", "256"])
def test_other_widths_stay_refused(D, H):
    for prec in ("f16x3", "fp32"):
        rc, _ = _create(prec, num_frame=243, embed_dim=D, depth=8, num_heads=H)
        assert rc == -5, (prec, D, H)
        msg = _lib.lib().d3d_last_error()
        assert b"48" in msg and b"96" in msg and b"128" in msg      # the message lists the admitted widths


@pytest.mark.parametrize("D,H", [(16, 1), (48, 3), (80, 5), (112, 7), (144, 9), (48, 2)])
def test_other_widths_that_are_no_multiple_of_32_stay_refused(D, H):
    """embed_dim % 32 == 16 is admitted for heads of 48 columns alone: head widths 16 and 24 at such a D stay refused."""
    for prec in ("f16x3", "fp32", "bf16"):
        rc, _ = _create(prec, num_frame=243, embed_dim=D, depth=8, num_heads=H)
        assert rc == -5, (prec, D, H)
    rc, _ = _create("bf16", num_frame=243, embed_dim=48, depth=8, num_heads=1)
    assert rc == -5


def test_weight_inventory_matches_the_spec(host_engine):
    L, h, cfg = host_engine
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
    L, h, _ = host_engine
    dflt = _documented_default(KEY)
    assert engine_info(L, h, KEY) == (0, dflt)
    for v in (1 - dflt, dflt):
        assert L.d3d_engine_set_option(h, KEY.encode(), v) == 0
        assert engine_info(L, h, KEY) == (0, v)


def test_last_reads_zero_before_any_forward(host_engine):
    L, h, _ = host_engine
    dflt = _documented_default(KEY)
    for v in (1, 0, dflt):
        assert L.d3d_engine_set_option(h, KEY.encode(), v) == 0
        assert engine_info(L, h, LAST) == (0, 0)


def test_workspace_bytes_do_not_depend_on_the_option(host_engine):
    """The kernels read the qkv planes and write the attention rows the launches they replace do: nothing more to allocate."""
    L, h, _ = host_engine
    dflt = _documented_default(KEY)
    size = {}
    for v in (1, 0):
        assert L.d3d_engine_set_option(h, KEY.encode(), v) == 0
        size[v] = [L.d3d_workspace_bytes(h, B) for B in (1, 3, 8)]
    assert L.d3d_engine_set_option(h, KEY.encode(), dflt) == 0
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
def test_the_new_translation_unit_is_in_the_build_list(unit):
    """tests/test_abi_host.py scans the object file of every entry of SOURCES."""
    from diff3dhpe_amd.build import SOURCES
    assert unit in SOURCES


def _cxx(name, nargs):
    """A host predicate of the library through its C++ symbol, as tests/test_group_lengths_host.py reaches them."""
    f = getattr(_lib.lib(), f"_ZN3d3d{len(name)}{name}E" + "i" * nargs)
    f.restype, f.argtypes = C.c_bool, [C.c_int] * nargs
    return f


def test_predicates():
    res, lng = _cxx("attn_x3_hx_ok", 3), _cxx("attn_x3_hx_long_ok", 3)
    for H in (1, 2, 3, 8):
        for N in (1, 17, 27, 33, 81, 128):                       # resident at both widths
            for D in (48 * H, 96 * H):
                assert res(N, D, H) and lng(N, D, H), (N, D, H)
        for N in (129, 243, 256):                                # resident at width 48 alone
            assert res(N, 48 * H, H) and lng(N, 48 * H, H), (N, H)
            assert not res(N, 96 * H, H) and lng(N, 96 * H, H), (N, H)
        for N in (257, 300, 513, 100000):                        # streaming alone
            for D in (48 * H, 96 * H):
                assert not res(N, D, H) and lng(N, D, H), (N, D, H)
        for N in (0, 1, 27, 150, 300):                           # the other widths, and no tokens
            for D in (32 * H, 64 * H, 128 * H, 80 * H):
                if D in (48 * H, 96 * H):
                    continue
                assert not res(N, D, H) and not lng(N, D, H), (N, D, H)
        for D in (48 * H, 96 * H):
            assert not res(0, D, H) and not lng(0, D, H)
    assert not res(27, 0, 0) and not lng(27, 0, 0)
