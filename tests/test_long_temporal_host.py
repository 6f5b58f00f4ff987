"""Host-side contract of "long_temporal" (include/d3d.h): F16X3 engines with windows of more than 256 frames keep the folded flow, their
temporal blocks on the key-streaming attention kernel (kernels_attn_x3_long.hip).  The option and info keys, the op-level export, an
unchanged workspace size, and BF16 engines still refusing such windows.  No GPU needed: engines are created on the host only."""
import ctypes as C
import os
import re

from diff3dhpe_amd import _lib
from host_helpers import engine_info, host_engine_fixture
from diff3dhpe_amd.spec import DenoiserConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _create(prec, T=300):
    cfg = DenoiserConfig(num_frame=T, embed_dim=512, depth=8)
    c = _lib.Config(cfg.num_frame, cfg.num_joints, cfg.in_chans, cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.mlp_hidden,
                    int(cfg.with_time_emb), int(cfg.seq2frame), _lib.PRECISIONS[prec])
    h = C.c_void_p()
    return _lib.lib().d3d_engine_create(C.byref(c), C.byref(h)), h


host_engine = host_engine_fixture(num_frame=300, embed_dim=512, depth=8)


def test_option_defaults_to_on_and_round_trips(host_engine):
    L, h = host_engine
    assert engine_info(L, h, "long_temporal") == (0, 1)
    assert L.d3d_engine_set_option(h, b"long_temporal", 0) == 0
    assert engine_info(L, h, "long_temporal") == (0, 0)
    assert L.d3d_engine_set_option(h, b"long_temporal", 1) == 0
    assert engine_info(L, h, "long_temporal") == (0, 1)


def test_last_reads_zero_before_any_forward(host_engine):
    L, h = host_engine
    assert engine_info(L, h, "long_temporal_last") == (0, 0)
    assert L.d3d_engine_set_option(h, b"long_temporal", 0) == 0
    assert engine_info(L, h, "long_temporal_last") == (0, 0)


def test_workspace_bytes_do_not_depend_on_the_option(host_engine):
    """The folded flow and the plain flow share one carve-up: the option never changes what a caller has to allocate."""
    L, h = host_engine
    on = [L.d3d_workspace_bytes(h, B) for B in (1, 3, 8)]
    assert all(b > 0 for b in on)
    assert L.d3d_engine_set_option(h, b"long_temporal", 0) == 0
    off = [L.d3d_workspace_bytes(h, B) for B in (1, 3, 8)]
    assert L.d3d_engine_set_option(h, b"long_temporal", 1) == 0
    assert on == off == [L.d3d_workspace_bytes(h, B) for B in (1, 3, 8)]


def test_op_entry_is_exported_and_declared():
    assert hasattr(_lib.lib(), "d3d_op_attention_long")
    assert "d3d_op_attention_long" in _lib.ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    assert re.search(r"\bd3d_op_attention_long\s*\(", hdr)
    from diff3dhpe_amd import engine
    assert callable(engine.op_attention_long)


def test_the_new_translation_unit_is_in_the_build_list():
    """tests/test_abi_host.py scans the object file of every entry of SOURCES for the packed fp32 form no attention file may hold."""
    from diff3dhpe_amd.build import SOURCES
    assert "kernels_attn_x3_long.hip" in SOURCES


def test_bf16_engines_still_refuse_windows_longer_than_256():
    rc, h = _create("bf16")
    assert rc != 0
    assert "num_frame <= 256" in _lib.lib().d3d_last_error().decode()
    rc, h = _create("bf16", T=243)
    assert rc == 0
    _lib.lib().d3d_engine_destroy(h)
