"""Host-side contract of "fused_narrow" (include/d3d.h): the option and info keys, the workspace, the op-level export and its shape check,
the launch predicate, the model attribute, and the tile-order images of the weight commit at embed_dim 256 and 128.  No GPU needed:
engines are created on the host only, the predicate is a plain host function of the library (reached through its C++ symbol), the op
hook refuses a shape before it touches the device, and the packing runs as a stand-alone program under AddressSanitizer + UBSan."""
import ctypes as C
from functools import partial
import os
import re
import shutil
import subprocess

import pytest

from diff3dhpe_amd import _lib
from diff3dhpe_amd import build as B
from host_helpers import create_host_engine, engine_info, host_engine_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUP = -1, -5   # D3D_EINVAL, D3D_EUNSUP (include/d3d.h)
VERSION = 148
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer"]

host_engine = host_engine_fixture(num_frame=81, embed_dim=256, depth=2)
_info = partial(engine_info, sentinel=-99)     # a value no key of this module holds


def test_error_code_constants():
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    for name, val in (("D3D_EINVAL", EINVAL), ("D3D_EUNSUP", EUNSUP)):
        m = re.search(r"#define\s+%s\s+\((-?\d+)\)" % name, hdr)
        assert m and int(m.group(1)) == val


def test_option_defaults_to_0_and_round_trips(host_engine):
    L, h = host_engine
    assert _info(L, h, "fused_narrow") == (0, 0)
    for v in (1, 0, 1):
        assert L.d3d_engine_set_option(h, b"fused_narrow", v) == 0
        assert _info(L, h, "fused_narrow") == (0, v)
    for bad in (2, -1):
        assert L.d3d_engine_set_option(h, b"fused_narrow", bad) == EINVAL
        assert _info(L, h, "fused_narrow") == (0, 1)                      # a refused value changes nothing
    assert L.d3d_engine_set_option(h, b"fused_narrow", 0) == 0


def test_option_does_not_move_latency_mode_or_small_tiles(host_engine):
    L, h = host_engine
    assert L.d3d_engine_set_option(h, b"fused_narrow", 1) == 0
    assert _info(L, h, "latency_mode") == (0, 0) and _info(L, h, "small_tiles") == (0, 0)
    assert L.d3d_engine_set_option(h, b"latency_mode", 1) == 0
    assert L.d3d_engine_set_option(h, b"latency_mode", 0) == 0
    assert _info(L, h, "fused_narrow") == (0, 1)


@pytest.mark.parametrize("precision,D", [("f16x3", 256), ("f16x3", 128), ("f16x3", 512), ("fp32", 256), ("fp32", 128), ("bf16", 512)])
def test_last_key_reads_0_on_a_fresh_engine(precision, D):
    """(BF16 engines exist at embed_dim 512 only.)"""
    L = _lib.lib()
    h = create_host_engine(precision, num_frame=81, embed_dim=D, depth=2)
    try:
        assert _info(L, h, "fused_narrow_last") == (0, 0)
        assert L.d3d_engine_set_option(h, b"fused_narrow", 1) == 0
        assert _info(L, h, "fused_narrow_last") == (0, 0)                 # nothing ran yet
    finally:
        L.d3d_engine_destroy(h)


@pytest.mark.parametrize("D", [256, 128])
def test_workspace_bytes_do_not_depend_on_the_option(D):
    L = _lib.lib()
    h = create_host_engine("f16x3", num_frame=81, embed_dim=D, depth=2)
    try:
        before = [L.d3d_workspace_bytes(h, B_) for B_ in (1, 2, 4, 64)]
        assert all(b > 0 for b in before)
        assert L.d3d_engine_set_option(h, b"fused_narrow", 1) == 0
        assert [L.d3d_workspace_bytes(h, B_) for B_ in (1, 2, 4, 64)] == before
        assert L.d3d_engine_set_option(h, b"fused_narrow", 0) == 0
        assert [L.d3d_workspace_bytes(h, B_) for B_ in (1, 2, 4, 64)] == before
    finally:
        L.d3d_engine_destroy(h)


def test_op_entry_is_exported_declared_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    name = "d3d_op_qkv_attn_x3_narrow"
    assert hasattr(_lib.lib(), name)
    assert name in _lib.ABI_SYMBOLS
    assert re.search(r"\b%s\s*\(" % name, hdr)
    for key in ('"fused_narrow"', '"fused_narrow_last"'):
        assert key in hdr
    from diff3dhpe_amd import engine as E
    assert callable(E.op_qkv_attn_x3_narrow)
    assert "fused_narrow" in E.Engine.set_option.__doc__ and "fused_narrow_last" in E.Engine.info.__doc__
    assert _lib.lib().d3d_version() >= VERSION


def _predicate():
    ok = getattr(_lib.lib(), "_ZN3d3d21qkv_attn_x3_narrow_okEiiiiii")
    ok.restype, ok.argtypes = C.c_bool, [C.c_int] * 6
    return ok


def test_launch_predicate_admits():
    """d3d::qkv_attn_x3_narrow_ok(N, stride, J, D, H, K): heads of 32 columns in pairs or 16 in quads, K = D >= 128, groups of at most
    127 tokens; spatial groups are the J joints of a frame (stride 1, any J), temporal groups the frames of a joint (stride J)."""
    ok = _predicate()
    for args in ((17, 1, 17, 256, 8, 256), (21, 1, 21, 256, 8, 256), (81, 17, 17, 256, 8, 256), (127, 5, 5, 128, 8, 128)):
        assert ok(*args), args
    for D, H in ((256, 8), (128, 8), (128, 4), (256, 16), (512, 16), (192, 12)):
        for J in (1, 15, 16, 17, 21, 127):
            assert ok(J, 1, J, D, H, D), (J, D, H)
            for T in (1, 2, 27, 81, 127):
                assert ok(T, J, J, D, H, D), (T, J, D, H)


def test_launch_predicate_refuses():
    ok = _predicate()
    assert not ok(0, 17, 17, 256, 8, 256) and not ok(0, 1, 0, 256, 8, 256)
    assert not ok(128, 17, 17, 256, 8, 256) and not ok(128, 1, 128, 256, 8, 256)
    assert not ok(243, 17, 17, 256, 8, 256)
    for D, H in ((512, 8), (96, 3), (32, 2), (384, 8), (64, 2), (64, 4), (1024, 8), (768, 8), (160, 5), (80, 5), (112, 7), (48, 3)):
        assert not ok(17, 1, 17, D, H, D), (D, H)
        assert not ok(81, 17, 17, D, H, D), (D, H)
    assert not ok(81, 3, 17, 256, 8, 256)                                 # a stride that is neither 1 with N = J nor J
    assert not ok(81, 1, 17, 256, 8, 256)
    assert not ok(17, 2, 17, 128, 8, 128)
    assert not ok(17, 1, 17, 256, 8, 128) and not ok(17, 1, 17, 256, 8, 512)   # K is the model width
    assert not ok(17, 1, 17, 256, 6, 256) and not ok(17, 1, 17, 128, 2, 128)   # another head width


def test_op_hook_rejects_shapes_outside_its_predicate():
    """The shape check comes before any device work: host memory stands in for the (never touched) device pointers."""
    L = _lib.lib()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)

    def op(groups, N, stride, D, H, temporal, eps=1e-6):
        return L.d3d_op_qkv_attn_x3_narrow(p, p, p, p, p, eps, groups, N, stride, D, H, temporal, p, None)
    assert op(17, 128, 17, 256, 8, 1) == EUNSUP                           # a group longer than a tile
    assert op(17, 243, 17, 128, 8, 1) == EUNSUP
    assert op(34, 17, 2, 256, 8, 0) == EUNSUP                             # spatial groups are consecutive rows
    assert op(17, 81, 17, 512, 8, 1) == EUNSUP                            # other widths
    assert op(17, 81, 17, 384, 8, 1) == EUNSUP
    assert op(17, 81, 17, 96, 3, 1) == EUNSUP
    assert op(17, 81, 17, 64, 2, 1) == EUNSUP
    assert op(18, 81, 17, 256, 8, 1) == EINVAL                            # groups not a multiple of the stride
    assert op(0, 81, 17, 256, 8, 1) == EINVAL
    assert op(17, 81, 17, 256, 8, 1, eps=0.0) == EINVAL
    assert L.d3d_op_qkv_attn_x3_narrow(None, p, p, p, p, 1e-6, 17, 81, 17, 256, 8, 1, p, None) == EINVAL


def test_model_class_forwards_the_attribute():
    import diff3dhpe_amd as d3d
    cls = d3d.HPE_model(d3d.S2S_NAME)
    assert cls.fused_narrow is False


def test_tile_order_images_under_host_sanitizers(tmp_path):
    """tests/host/narrow_tile_order_check.cpp + weight_pack.hip as one program: row r of the D = 256 / 128 images is folded row
    tile_order_src_row(r, D, D / 64), csum and bias alike, the exponent the untiled image's."""
    hipcc = os.environ.get("HIPCC", "hipcc")
    assert shutil.which(hipcc), f"{hipcc} not found: the weight packing cannot be checked"     # (no skip: as test_weight_pack_host.py)
    objs = []
    for src in (os.path.join(B.CSRC, "weight_pack.hip"), os.path.join(ROOT, "tests", "host", "narrow_tile_order_check.cpp")):
        o = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run([hipcc] + B.FLAGS + B.EXTRA_FLAGS.get(os.path.basename(src), []) + SAN + ["-I", B.CSRC, "-c", src, "-o", o], check=True)
        objs.append(o)
    exe = str(tmp_path / "narrow_tile_order_check")
    subprocess.run([hipcc] + SAN + ["-o", exe] + objs, check=True)        # (host link only: the sanitizers never reach device code)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    report = [l for l in (r.stdout + r.stderr).splitlines() if "Sanitizer" in l or "runtime error" in l]
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert not report, "\n".join(report)
    assert not r.stderr.strip(), r.stderr[-4000:]
    assert r.stdout.strip().endswith("narrow_tile_order_check: ok"), r.stdout[-2000:]
