"""Host-side contract of the fused spatial path at 15, 16 and 17 joints (kernels_qkv_sattn.hip, the fp32 spatial kernel of kernels_attn.hip):
the info key "fused_spatial_last" exists and reads 0 before any forward in every precision, the workspace size does not depend on the
options that select the path, the
version and the header name the feature, and every translation unit with a spatial kernel is in build.SOURCES.  No GPU needed: engines are
created on the host only."""
import os

import pytest

from diff3dhpe_amd import _lib
from host_helpers import create_host_engine, engine_info

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOINTS = (15, 16, 17)


@pytest.mark.parametrize("J", JOINTS)
@pytest.mark.parametrize("prec", ["f16x3", "bf16", "fp32"])
def test_fused_spatial_last_reads_zero_on_a_fresh_engine(prec, J):
    L = _lib.lib()
    h = create_host_engine(prec, num_frame=27, num_joints=J, embed_dim=512, depth=1)
    try:
        assert engine_info(L, h, "fused_spatial_last") == (0, 0)
        assert engine_info(L, h, "block0_direct_last") == (0, 0)
        for key in (b"fused_spatial", b"block0_direct"):
            assert L.d3d_engine_set_option(h, key, 0) == 0 and L.d3d_engine_set_option(h, key, 1) == 0
        assert engine_info(L, h, "fused_spatial_last") == (0, 0)           # still no forward
        assert engine_info(L, h, "bf16_fused_spatial_last") == (0, 0)      # the bf16 key is its own
    finally:
        L.d3d_engine_destroy(h)


@pytest.mark.parametrize("J", JOINTS)
@pytest.mark.parametrize("T", [9, 27, 243])
def test_workspace_bytes_do_not_depend_on_the_spatial_options(J, T):
    L = _lib.lib()
    h = create_host_engine("f16x3", num_frame=T, num_joints=J, embed_dim=512, depth=1)
    try:
        before = [L.d3d_workspace_bytes(h, B) for B in (1, 3, 8)]
        assert all(b > 0 for b in before)
        for fused, direct in ((0, 1), (1, 0), (0, 0)):
            assert L.d3d_engine_set_option(h, b"fused_spatial", fused) == 0 and L.d3d_engine_set_option(h, b"block0_direct", direct) == 0
            assert [L.d3d_workspace_bytes(h, B) for B in (1, 3, 8)] == before
    finally:
        L.d3d_engine_destroy(h)


def test_version_header_and_sources():
    assert _lib.lib().d3d_version() >= 137
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    assert "fused_spatial_last" in hdr and "15, 16 or 17 joints" in hdr
    from diff3dhpe_amd.build import SOURCES
    assert "kernels_qkv_sattn.hip" in SOURCES and "kernels_attn.hip" in SOURCES
    csrc = os.path.join(ROOT, "diff3dhpe_amd", "csrc")
    for f in os.listdir(csrc):      # no spatial kernel lives in a file the build (and the object-file scans that walk SOURCES) does not know
        if f.endswith(".hip"):
            assert f in SOURCES, f


def test_every_joint_count_has_its_kernels_in_the_device_code():
    from test_abi_host import _device_isa
    isa = _device_isa("kernels_qkv_sattn.o")
    for J in JOINTS:
        assert f"k_qkv_sattnILi{J}E" in isa, J
        for cin2 in (1, 2, 3):
            for planes in (0, 1):
                assert f"k_qkv_sattn_directILi{J}ELi{cin2}ELb{planes}E" in isa, (J, cin2, planes)
    isa = _device_isa("kernels_attn.o")
    for J in JOINTS:
        assert f"k_attn_spatial_f32ILi{J}E" in isa, J
