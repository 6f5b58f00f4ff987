"""Host-side contract of the fp16 operand mode (D3D_PREC_F16, include/d3d.h): admission and refusal of engines (the bf16 mode's exactly),
the workspace (the bf16 engine's at every batch size), the header, and the host rounding the weight commit uses (f16_rne, pack_bf16's
fp16 form) against torch's .to(float16).  No GPU: engines are created through the C ABI and never committed; the rounding runs in a
stand-alone host program (tests/host/f16_rne_check.cpp + the packing unit) under the host sanitizers."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import pytest
import torch

from diff3dhpe_amd import _lib, build as B
from diff3dhpe_amd.spec import DenoiserConfig
from host_helpers import create_host_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EUNSUP = -5   # D3D_EUNSUP


def _create(prec_value, **kw):
    """(rc, handle, message) of d3d_engine_create with a raw precision value."""
    cfg = DenoiserConfig(**kw)
    c = _lib.Config(cfg.num_frame, cfg.num_joints, cfg.in_chans, cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.mlp_hidden,
                    int(cfg.with_time_emb), int(cfg.seq2frame), prec_value)
    h = C.c_void_p()
    rc = _lib.lib().d3d_engine_create(C.byref(c), C.byref(h))
    msg = _lib.lib().d3d_last_error()
    return rc, h, (msg.decode() if msg else "")


def test_the_python_layer_names_the_precision():
    assert _lib.PREC_F16 == 3 and _lib.PRECISIONS["f16"] == 3
    assert {k: v for k, v in _lib.PRECISIONS.items() if k != "f16"} == {"fp32": 0, "f16x3": 1, "bf16": 2}
    assert "d3d_op_qkv_attn_f16" in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), "d3d_op_qkv_attn_f16")
    from diff3dhpe_amd import engine
    assert callable(engine.op_qkv_attn_f16)


@pytest.mark.parametrize("J", [15, 17, 32])
@pytest.mark.parametrize("T", [9, 27, 243, 256])
def test_admission_at_embed_dim_512(T, J):
    L = _lib.lib()
    h = create_host_engine("f16", num_frame=T, num_joints=J, embed_dim=512, depth=1)
    L.d3d_engine_destroy(h)


REFUSED = [("head_dim 4", dict(num_frame=9, embed_dim=32, num_heads=8)), ("head_dim 32", dict(num_frame=9, embed_dim=256, num_heads=8)),
           ("head_dim 128", dict(num_frame=9, embed_dim=1024, num_heads=8)), ("T 257", dict(num_frame=257, embed_dim=512)),
           ("J 33", dict(num_frame=9, num_joints=33, embed_dim=512)), ("mlp_hidden % 64", dict(num_frame=9, embed_dim=512, mlp_ratio=2.0625))]


@pytest.mark.parametrize("what,kw", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusal_names_the_mode(what, kw):
    cfg = DenoiserConfig(depth=1, **kw)
    if what.startswith("mlp"):
        assert cfg.mlp_hidden % 64 != 0 and cfg.mlp_hidden % 32 == 0, cfg.mlp_hidden   # (the case is what its name says)
    rc, h, msg = _create(_lib.PREC_F16, depth=1, **kw)
    assert rc == EUNSUP and "D3D_PREC_F16 needs" in msg, (rc, msg)
    rc, h, msg = _create(_lib.PREC_BF16, depth=1, **kw)                               # the bf16 text stays as it was
    assert rc == EUNSUP and "D3D_PREC_BF16 needs" in msg and "D3D_PREC_F16" not in msg, (rc, msg)


def test_unknown_precision_is_still_refused():
    for p in (4, 7, -1):
        rc, h, msg = _create(p, num_frame=9, embed_dim=512, depth=1)
        assert rc == EUNSUP and "precision must be" in msg, (p, rc, msg)


def test_version_moved():
    assert _lib.lib().d3d_version() >= 149


@pytest.mark.parametrize("kw", [dict(num_frame=27, embed_dim=512, depth=2), dict(num_frame=243, embed_dim=512, depth=1),
                                dict(num_frame=81, num_joints=15, embed_dim=256, num_heads=4, depth=1),
                                dict(num_frame=27, embed_dim=512, depth=1, seq2frame=True)])
def test_workspace_bytes_equal_the_bf16_engines(kw):
    L = _lib.lib()
    hs = {p: create_host_engine(p, **kw) for p in ("bf16", "f16")}
    try:
        for Bn in (1, 3, 8):
            a, b = L.d3d_workspace_bytes(hs["bf16"], Bn), L.d3d_workspace_bytes(hs["f16"], Bn)
            assert a == b and a > 0, (Bn, a, b)
    finally:
        for h in hs.values():
            L.d3d_engine_destroy(h)


def test_header_names_the_mode_and_its_hook():
    hdr = open(os.path.join(ROOT, "include", "d3d.h")).read()
    assert "#define D3D_PREC_F16 3" in hdr and "int d3d_op_qkv_attn_f16(" in hdr
    # the shared option / info keys are said to serve both 16-bit modes; no parallel f16_* keys
    assert "serve both" in hdr and '"f16_' not in hdr


def _f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _rounding_table():
    """fp32 bit patterns: ties of normal and subnormal results, the range's ends, the subnormal range and below it, non-finite values."""
    u = []
    two = lambda e: 2.0 ** e
    vals = [0.0, 1.0, -2.5, 1.0 + two(-11), 1.0 + 3 * two(-11), 1.0 + two(-11) + two(-23), 1.0 + two(-11) - two(-24),   # ties: to even, above, below
            2.0 - two(-11), 2.0 - two(-12),                                # a mantissa carry into the exponent (tie -> 2.0), just below it
            65504.0, 65504.0 + 8.0, 65519.0, 65520.0, -65520.0, 65536.0, 1e5, 3.0e38,    # the largest finite value, the tie to inf, beyond
            two(-14), two(-14) - two(-25), two(-14) - two(-26), two(-15), 3 * two(-24), 2.5 * two(-24), 3.5 * two(-24), 1.5 * two(-24),
            two(-24), 0.75 * two(-24), two(-25), two(-25) + two(-48), two(-25) - two(-49), two(-26), two(-30), 1e-40, -1e-40,    # (fp32 subnormals)
            6.1e-5, -6.0e-5, 5.96e-8, 1.0e-7, -2.98e-8, 0.1, -0.3333, 1234.5678, 3.14159e-6]
    u += [_f32_bits(v) for v in vals]
    u += [0x7f800000, 0xff800000, 0x7fc00000, 0x7f800001, 0xffc01234, 0x80000000, 0x477fefff, 0x477ff000, 0x477ff001, 0x33000000, 0x33000001,
          0x32ffffff, 0x387fffff, 0x38800000, 0x387fe000, 0x387ff000]
    g = torch.Generator().manual_seed(16)
    u += torch.randint(0, 2 ** 31 - 1, (4000,), generator=g).tolist()                                   # any exponent
    u += (torch.randint(0, 2 ** 23, (4000,), generator=g) + (torch.randint(100, 145, (4000,), generator=g) << 23)).tolist()   # around fp16's range
    return u


def test_f16_rne_and_the_fp16_pack_match_torch(tmp_path):
    hipcc = os.environ.get("HIPCC", "hipcc")
    assert shutil.which(hipcc), f"{hipcc} not found: the fp16 rounding of the weight commit cannot be checked"
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer"]
    objs = []
    for src in (os.path.join(B.CSRC, "weight_pack.hip"), os.path.join(ROOT, "tests", "host", "f16_rne_check.cpp")):
        o = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run([hipcc] + B.FLAGS + B.EXTRA_FLAGS.get(os.path.basename(src), []) + san + ["-I", B.CSRC, "-c", src, "-o", o], check=True)
        objs.append(o)
    exe = str(tmp_path / "f16_rne_check")
    subprocess.run([hipcc] + san + ["-o", exe] + objs, check=True)
    table = _rounding_table()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], input="\n".join(f"{u:08x}" for u in table) + "\n", capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "pack: ok" and len(lines) == len(table) + 1, lines[-3:]
    x = torch.tensor(table, dtype=torch.int64).to(torch.int32).view(torch.float32)
    want = x.to(torch.float16)
    wbits = (want.view(torch.int16).to(torch.int32) & 0xffff).tolist()
    wnan, wnonfinite = torch.isnan(want).tolist(), (~torch.isfinite(want)).tolist()
    n_sub = n_inf = 0
    for u, line, wb, isnan, nonfin in zip(table, lines, wbits, wnan, wnonfinite):
        hb, flag = line.split()
        hb = int(hb, 16)
        if isnan:
            assert (hb & 0x7c00) == 0x7c00 and (hb & 0x3ff) != 0, f"{u:08x}: {hb:04x} is not a NaN"
        else:
            assert hb == wb, f"{u:08x}: f16_rne {hb:04x}, torch {wb:04x}"
        assert int(flag) == int(nonfin), f"{u:08x}: flag {flag}, torch non-finite {nonfin}"
        n_sub += (hb & 0x7c00) == 0 and (hb & 0x3ff) != 0
        n_inf += (hb & 0x7fff) == 0x7c00
    assert n_sub >= 100 and n_inf >= 100          # the table does reach the subnormal range and the overflow
    # the cases the mode's contract names, by value
    by = {u: line.split() for u, line in zip(table, lines)}
    assert by[_f32_bits(65504.0)] == ["7bff", "0"] and by[_f32_bits(65520.0)] == ["7c00", "1"] and by[0x477fefff] == ["7bff", "0"]
    assert by[_f32_bits(2.0 ** -24)] == ["0001", "0"] and by[_f32_bits(2.0 ** -25)] == ["0000", "0"] and by[0x33000001] == ["0001", "0"]
