"""Host-side contract of the fused bf16 qkv GEMM + attention kernels (kernels_qkv_attn_bf16.hip): both kernels are in the device code
of the new object file, the file is in build.SOURCES (tests/test_abi_host.py walks that list for the packed-fp32 pin) and built without
the SLP vectoriser, the op export and the two info keys exist.  No GPU needed: engines are created on the host only."""
import os
import re

import pytest

from diff3dhpe_amd import _lib
from host_helpers import create_host_engine, engine_info

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("prec", ["bf16", "f16x3"])
def test_info_keys_read_zero_on_a_fresh_engine(prec):
    L = _lib.lib()
    h = create_host_engine(prec, num_frame=81, embed_dim=512, depth=8)
    try:
        assert engine_info(L, h, "bf16_fused_spatial_last") == (0, 0)
        assert engine_info(L, h, "bf16_fused_temporal_last") == (0, 0)
        for key in (b"fused_spatial", b"fused_temporal"):            # the option keys the fused bf16 flow answers to
            assert L.d3d_engine_set_option(h, key, 0) == 0 and L.d3d_engine_set_option(h, key, 1) == 0
        assert engine_info(L, h, "bf16_fused_spatial_last") == (0, 0)      # still no forward
    finally:
        L.d3d_engine_destroy(h)


def test_workspace_bytes_do_not_depend_on_the_options():
    """The attention output of a fused block takes the region the q / k / v tensor would have taken."""
    L = _lib.lib()
    h = create_host_engine("bf16", num_frame=81, embed_dim=512, depth=8)
    try:
        before = [L.d3d_workspace_bytes(h, B) for B in (1, 4, 128)]
        for key in (b"fused_spatial", b"fused_temporal"):
            assert L.d3d_engine_set_option(h, key, 0) == 0
        assert [L.d3d_workspace_bytes(h, B) for B in (1, 4, 128)] == before and all(b > 0 for b in before)
    finally:
        L.d3d_engine_destroy(h)


def test_op_entry_is_exported_and_declared():
    assert hasattr(_lib.lib(), "d3d_op_qkv_attn_bf16")
    assert "d3d_op_qkv_attn_bf16" in _lib.ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    assert re.search(r"\bd3d_op_qkv_attn_bf16\s*\(", hdr)
    assert "bf16_fused_spatial_last" in hdr and "bf16_fused_temporal_last" in hdr


def test_both_kernels_are_in_the_device_code_of_the_new_object_file():
    from diff3dhpe_amd.build import SOURCES, EXTRA_FLAGS
    from test_abi_host import _device_isa
    assert "kernels_qkv_attn_bf16.hip" in SOURCES
    assert "-fno-slp-vectorize" in EXTRA_FLAGS.get("kernels_qkv_attn_bf16.hip", [])
    isa = _device_isa("kernels_qkv_attn_bf16.o")
    assert "k_qkv_sattn_bf16" in isa and "k_qkv_tattn_bf16" in isa
    assert "v_mfma_f32_16x16x32_bf16" in isa and "v_mfma_f32_32x32x16_bf16" in isa and "global_load_lds_dwordx4" in isa
