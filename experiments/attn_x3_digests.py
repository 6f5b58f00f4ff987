"""Record a golden file of output digests: one SHA-256 of the output bytes per case of a digest test module (the cases, their inputs and
the file's path live there), with the ROCm version and the commit of the library that computed them.

    python experiments/attn_x3_digests.py [--cases MODULE] [--out FILE] [--commit REV]

--cases: test_gpu_attn_x3_digests (the default; tests/golden/attn_x3_digests.json), test_gpu_attn_x3_width_digests
(tests/golden/attn_x3_width_digests.json) or test_gpu_attn_f32_digests (tests/golden/attn_f32_digests.json).

Run it on the MI355X with the library of the commit whose bits are to be pinned -- the commit BEFORE a change to the shared attention
pieces, never the change itself.  --commit names that revision where the tree is not a git checkout."""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="test_gpu_attn_x3_digests",
                    choices=["test_gpu_attn_x3_digests", "test_gpu_attn_x3_width_digests", "test_gpu_attn_f32_digests"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    cases = importlib.import_module(args.cases)
    args.out = args.out or cases.DIGESTS
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    rec = {"commit": commit, "rocm": torch.version.hip, "device": torch.cuda.get_device_properties(0).name,
           "what": f"sha256 of the fp32 output bytes of every case of tests/{args.cases}.py", "sha256": {}}
    for name in cases.CASES:
        rec["sha256"][name] = cases.digest(name)
        print(name, rec["sha256"][name], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
