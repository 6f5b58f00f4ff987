"""Host-side contract of the opt-in "latency_mode" (include/d3d.h): the option and info keys, the op-level export, an unchanged
workspace size, and the packed-fp32 ISA pin on the new object file.  No GPU needed: engines are created on the host only."""
import os
import re

from diff3dhpe_amd import _lib
from host_helpers import engine_info, host_engine_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


host_engine = host_engine_fixture(num_frame=243, embed_dim=512, depth=8)


def test_option_and_info_keys(host_engine):
    L, h = host_engine
    assert engine_info(L, h, "latency_mode") == (0, 0)                      # off by default
    assert L.d3d_engine_set_option(h, b"latency_mode", 1) == 0        # D3D_OK
    assert engine_info(L, h, "latency_mode") == (0, 1)
    assert L.d3d_engine_set_option(h, b"latency_mode", 0) == 0
    assert engine_info(L, h, "latency_mode") == (0, 0)


def test_split_info_reads_zero_before_any_forward(host_engine):
    L, h = host_engine
    assert engine_info(L, h, "fc2_split_last") == (0, 0)
    assert L.d3d_engine_set_option(h, b"latency_mode", 1) == 0
    assert engine_info(L, h, "fc2_split_last") == (0, 0)


def test_op_entry_is_exported_and_declared():
    assert hasattr(_lib.lib(), "d3d_op_linear_splitk_postnorm")
    assert "d3d_op_linear_splitk_postnorm" in _lib.ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    assert re.search(r"\bd3d_op_linear_splitk_postnorm\s*\(", hdr)


def test_workspace_bytes_do_not_depend_on_the_option(host_engine):
    """The partials live in regions that are dead during fc2: the option never changes what a caller has to allocate."""
    L, h = host_engine
    before = [L.d3d_workspace_bytes(h, B) for B in (1, 4, 64)]
    assert all(b > 0 for b in before)
    assert L.d3d_engine_set_option(h, b"latency_mode", 1) == 0
    during = [L.d3d_workspace_bytes(h, B) for B in (1, 4, 64)]
    assert L.d3d_engine_set_option(h, b"latency_mode", 0) == 0
    after = [L.d3d_workspace_bytes(h, B) for B in (1, 4, 64)]
    assert before == during == after
    # ... and the partials fit where the engine puts them: S (M, D) fp32 tensors in w.HN (>= M D floats) + w.QKV (3 M D floats)
    for B in (1, 4):
        M = B * 243 * 17
        assert 4 * M * 512 * 4 <= before[(1, 4).index(B)]


def test_packed_fp32_isa_scan_covers_the_new_object_file():
    """tests/test_abi_host.py walks diff3dhpe_amd.build.SOURCES: the new translation unit must be in that list, built without the SLP
    vectoriser like the other row kernels, and its device code must hold both no `op_sel` src1 broadcast and the row kernel itself."""
    from diff3dhpe_amd.build import SOURCES, EXTRA_FLAGS
    from test_abi_host import _device_isa
    assert "kernels_fc2_splitk.hip" in SOURCES
    assert "-fno-slp-vectorize" in EXTRA_FLAGS.get("kernels_fc2_splitk.hip", [])
    isa = _device_isa("kernels_fc2_splitk.o")
    assert "k_splitk_postnorm" in isa
    bad = []
    for line in isa.splitlines():
        t = line.strip()
        if not (t.startswith("v_pk_") and "_f32" in t.split()[0]):
            continue
        sel = re.search(r"op_sel:\[([01,]+)\]", t)
        if sel and len(sel.group(1).split(",")) >= 2 and sel.group(1).split(",")[1] == "1":
            bad.append(t.split("//")[0].strip())
    assert not bad, bad[:10]
    # the split GEMM lives beside the template it instantiates
    assert "k_linear_x3q_splitk" in _device_isa("kernels_gemm_x3p.o")
