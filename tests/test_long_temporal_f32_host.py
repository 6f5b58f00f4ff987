"""Host-side contract of "long_temporal_f32" (include/d3d.h): FP32 engines with windows of more than 256 frames run their temporal blocks'
attention on the key-streaming fp32 MFMA kernel (kernels_attn_f32_long.hip).  The option and info keys, the op-level export and an
unchanged workspace size.  No GPU needed: engines are created on the host only."""
import os
import re

from diff3dhpe_amd import _lib
from host_helpers import engine_info, host_engine_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


host_engine = host_engine_fixture(num_frame=300, embed_dim=512, depth=8, prec="fp32")


def test_version_is_136_or_later():
    assert _lib.lib().d3d_version() >= 136


def test_option_defaults_to_on_and_round_trips(host_engine):
    L, h = host_engine
    assert engine_info(L, h, "long_temporal_f32") == (0, 1)
    assert L.d3d_engine_set_option(h, b"long_temporal_f32", 0) == 0
    assert engine_info(L, h, "long_temporal_f32") == (0, 0)
    assert L.d3d_engine_set_option(h, b"long_temporal_f32", 1) == 0
    assert engine_info(L, h, "long_temporal_f32") == (0, 1)


def test_last_reads_zero_before_any_forward(host_engine):
    L, h = host_engine
    assert engine_info(L, h, "long_temporal_f32_last") == (0, 0)
    assert L.d3d_engine_set_option(h, b"long_temporal_f32", 0) == 0
    assert engine_info(L, h, "long_temporal_f32_last") == (0, 0)
    assert engine_info(L, h, "long_temporal_last") == (0, 0)


def test_workspace_bytes_do_not_depend_on_the_option(host_engine):
    """The kernel reads the packed qkv rows and writes the attention rows the generic kernel does: nothing new to allocate."""
    L, h = host_engine
    on = [L.d3d_workspace_bytes(h, B) for B in (1, 3, 8)]
    assert all(b > 0 for b in on)
    assert L.d3d_engine_set_option(h, b"long_temporal_f32", 0) == 0
    off = [L.d3d_workspace_bytes(h, B) for B in (1, 3, 8)]
    assert L.d3d_engine_set_option(h, b"long_temporal_f32", 1) == 0
    assert on == off == [L.d3d_workspace_bytes(h, B) for B in (1, 3, 8)]


def test_op_entry_is_exported_and_declared():
    assert hasattr(_lib.lib(), "d3d_op_attention_long_f32")
    assert "d3d_op_attention_long_f32" in _lib.ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    assert re.search(r"\bd3d_op_attention_long_f32\s*\(", hdr)
    from diff3dhpe_amd import engine
    assert callable(engine.op_attention_long_f32)


def test_the_new_translation_unit_is_in_the_build_list():
    """tests/test_abi_host.py scans the object file of every entry of SOURCES for the packed fp32 form no attention file may hold."""
    from diff3dhpe_amd.build import SOURCES
    assert "kernels_attn_f32_long.hip" in SOURCES
