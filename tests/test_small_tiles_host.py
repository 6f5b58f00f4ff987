"""Host-side contract of "small_tiles" (include/d3d.h): the option and info keys, the workspace, the op-level export and its shape
predicate, the launch predicate and the translation unit.  No GPU needed: engines are created on the host only, the predicates are plain
host functions of the library (reached through their C++ symbols), and the op hook refuses a shape before it touches the device."""
import ctypes as C
from functools import partial
import os
import re

import pytest

from diff3dhpe_amd import _lib
from host_helpers import create_host_engine, engine_info, host_engine_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUP = -1, -5   # D3D_EINVAL, D3D_EUNSUP (include/d3d.h)


host_engine = host_engine_fixture(num_frame=81, embed_dim=512, depth=2)
_info = partial(engine_info, sentinel=-99)     # a value no key of this module holds


def test_error_code_constants():
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    for name, val in (("D3D_EINVAL", EINVAL), ("D3D_EUNSUP", EUNSUP)):
        m = re.search(r"#define\s+%s\s+\((-?\d+)\)" % name, hdr)
        assert m and int(m.group(1)) == val


def test_option_defaults_to_0_and_round_trips(host_engine):
    L, h = host_engine
    assert _info(L, h, "small_tiles") == (0, 0)
    for v in (1, 0, 1):
        assert L.d3d_engine_set_option(h, b"small_tiles", v) == 0
        assert _info(L, h, "small_tiles") == (0, v)
    for bad in (2, -1):
        assert L.d3d_engine_set_option(h, b"small_tiles", bad) == EINVAL
        assert _info(L, h, "small_tiles") == (0, 1)                       # a refused value changes nothing
    assert L.d3d_engine_set_option(h, b"small_tiles", 0) == 0


@pytest.mark.parametrize("precision", ["f16x3", "fp32", "bf16"])
def test_last_key_reads_0_on_a_fresh_engine(precision):
    L = _lib.lib()
    h = create_host_engine(precision, num_frame=81, embed_dim=512, depth=2)
    try:
        assert _info(L, h, "small_tiles_last") == (0, 0)
        assert L.d3d_engine_set_option(h, b"latency_mode", 1) == 0
        assert L.d3d_engine_set_option(h, b"small_tiles", 1) == 0
        assert _info(L, h, "small_tiles_last") == (0, 0)                  # nothing ran yet
    finally:
        L.d3d_engine_destroy(h)


def test_key_is_accepted_without_latency_mode(host_engine):
    """Accepted and kept whatever "latency_mode" says (it is read only while that mode is on: the GPU tests show it is inert without);
    neither key moves the other."""
    L, h = host_engine
    assert _info(L, h, "latency_mode") == (0, 0)
    assert L.d3d_engine_set_option(h, b"small_tiles", 1) == 0
    assert _info(L, h, "small_tiles") == (0, 1) and _info(L, h, "latency_mode") == (0, 0)
    assert L.d3d_engine_set_option(h, b"latency_mode", 1) == 0
    assert L.d3d_engine_set_option(h, b"latency_mode", 0) == 0
    assert _info(L, h, "small_tiles") == (0, 1)
    assert _info(L, h, "small_tiles_last") == (0, 0)


def test_workspace_bytes_do_not_depend_on_the_option(host_engine):
    L, h = host_engine
    before = [L.d3d_workspace_bytes(h, B) for B in (1, 2, 4, 64)]
    assert L.d3d_engine_set_option(h, b"small_tiles", 1) == 0
    assert [L.d3d_workspace_bytes(h, B) for B in (1, 2, 4, 64)] == before
    assert L.d3d_engine_set_option(h, b"latency_mode", 1) == 0
    assert [L.d3d_workspace_bytes(h, B) for B in (1, 2, 4, 64)] == before
    assert L.d3d_engine_set_option(h, b"latency_mode", 0) == 0
    assert L.d3d_engine_set_option(h, b"small_tiles", 0) == 0
    assert [L.d3d_workspace_bytes(h, B) for B in (1, 2, 4, 64)] == before


def test_op_entry_is_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    name = "d3d_op_qkv_attn_x3_small"
    assert hasattr(_lib.lib(), name)
    assert name in _lib.ABI_SYMBOLS
    assert re.search(r"\b%s\s*\(" % name, hdr)
    for key in ('"small_tiles"', '"small_tiles_last"'):
        assert key in hdr
    from diff3dhpe_amd import engine as E
    assert callable(E.op_qkv_attn_x3_small)
    assert _lib.lib().d3d_version() >= 138


def test_launch_predicate():
    """d3d::qkv_attn_x3_small_ok(N, stride, J, D, H, K): D = 512, H = 8, K % 64 = 0, groups of at most 127 tokens; spatial groups are the
    15 .. 17 joints of a frame (stride 1), temporal groups the frames of a joint (stride J)."""
    ok = getattr(_lib.lib(), "_ZN3d3d20qkv_attn_x3_small_okEiiiiii")
    ok.restype, ok.argtypes = C.c_bool, [C.c_int] * 6
    for J in (15, 16, 17):
        assert ok(J, 1, J, 512, 8, 512)
        for T in (2, 9, 27, 81, 127):
            assert ok(T, J, J, 512, 8, 512), (T, J)
        for T in (128, 243, 256):
            assert not ok(T, J, J, 512, 8, 512), (T, J)
    for J in (14, 18, 21):
        assert not ok(J, 1, J, 512, 8, 512)                               # spatial: another joint count
    assert ok(81, 21, 21, 512, 8, 512)                                    # temporal groups of such a skeleton are fine
    assert not ok(81, 3, 17, 512, 8, 512)                                 # a stride that is neither 1 nor J
    assert not ok(0, 17, 17, 512, 8, 512)
    for D, H, K in ((256, 4, 256), (512, 4, 512), (512, 8, 96), (512, 8, 32), (1024, 16, 1024)):
        assert not ok(81, 17, 17, D, H, K), (D, H, K)


def test_op_hook_rejects_shapes_outside_its_predicate():
    """The shape check comes before any device work: host memory stands in for the (never touched) device pointers."""
    L = _lib.lib()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)

    def op(groups, N, stride, D, H, temporal, eps=1e-6):
        return L.d3d_op_qkv_attn_x3_small(p, p, p, p, p, eps, groups, N, stride, D, H, temporal, p, None)
    assert op(17, 128, 17, 512, 8, 1) == EUNSUP                           # a group longer than a tile
    assert op(17, 243, 17, 512, 8, 1) == EUNSUP
    assert op(27, 21, 1, 512, 8, 0) == EUNSUP                             # spatial groups of 21 joints
    assert op(34, 17, 2, 512, 8, 0) == EUNSUP                             # spatial groups are consecutive rows
    assert op(17, 81, 17, 256, 4, 1) == EUNSUP                            # another width
    assert op(17, 81, 17, 512, 4, 1) == EUNSUP
    assert op(18, 81, 17, 512, 8, 1) == EINVAL                            # groups not a multiple of the stride
    assert op(0, 81, 17, 512, 8, 1) == EINVAL
    assert op(17, 81, 17, 512, 8, 1, eps=0.0) == EINVAL
    assert L.d3d_op_qkv_attn_x3_small(None, p, p, p, p, 1e-6, 17, 81, 17, 512, 8, 1, p, None) == EINVAL


def test_new_translation_unit_is_in_the_build():
    """tests/test_abi_host.py scans every object file of diff3dhpe_amd.build.SOURCES: the new file must be in that list."""
    from diff3dhpe_amd.build import SOURCES
    assert "kernels_qkv_attn_x3_small.hip" in SOURCES
    assert os.path.exists(os.path.join(ROOT, "diff3dhpe_amd", "csrc", "kernels_qkv_attn_x3_small.hip"))


def test_model_class_forwards_the_attribute():
    import diff3dhpe_amd as d3d
    cls = d3d.HPE_model(d3d.S2S_NAME)
    assert cls.latency_small_tiles is False and cls.latency_mode is False
