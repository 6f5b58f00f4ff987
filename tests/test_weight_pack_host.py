"""The host-side weight packing (diff3dhpe_amd/csrc/weight_pack.hip: split, LayerNorm fold, tile order, block-0 tables, bf16, the whole
engine's images) under AddressSanitizer + UBSan, on the CPU: tests/host/weight_pack_check.cpp is compiled together with the unit into a
stand-alone program and run as an ordinary executable.  No GPU, no library, no preloaded runtime."""
import os
import shutil
import subprocess

from diff3dhpe_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer"]


def test_weight_pack_unit_under_host_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC", "hipcc")
    # no skip: a missing compiler must fail here -- this test is the only place the packing arithmetic runs without a device
    assert shutil.which(hipcc), f"{hipcc} not found: the weight packing cannot be checked"
    assert "weight_pack.hip" in B.SOURCES and "weight_pack.h" in B.HEADERS
    objs = []
    for src in (os.path.join(B.CSRC, "weight_pack.hip"), os.path.join(ROOT, "tests", "host", "weight_pack_check.cpp")):
        o = str(tmp_path / (os.path.basename(src) + ".o"))
        # the unit with exactly the library's flags (the bits depend on them) + the host sanitizers
        subprocess.run([hipcc] + B.FLAGS + B.EXTRA_FLAGS.get(os.path.basename(src), []) + SAN + ["-I", B.CSRC, "-c", src, "-o", o], check=True)
        objs.append(o)
    exe = str(tmp_path / "weight_pack_check")
    subprocess.run([hipcc] + SAN + ["-o", exe] + objs, check=True)     # (host link only: the sanitizers never reach device code)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    report = [l for l in (r.stdout + r.stderr).splitlines() if "Sanitizer" in l or "runtime error" in l]
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert not report, "\n".join(report)
    assert not r.stderr.strip(), r.stderr[-4000:]
    assert r.stdout.strip().endswith("weight_pack_check: ok"), r.stdout[-2000:]
