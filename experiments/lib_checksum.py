"""Checksums of 2-step samplings with the in-tree library, one SHA-256 prefix per configuration: run it under two builds of the library (or
in two trees) to see whether a change kept the results bit for bit (experiments/ab_libs.sh swaps the file).  The configurations cover
every resident weight image of the commit: F16X3 with and without the tile-order copies and the block-0 tables, BF16, FP32."""
import hashlib, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import cfg_full, inputs, build_product
CASES = (("f16x3 T=27 B=5", cfg_full(27), 5, "f16x3"),
         ("f16x3 T=243 B=3", cfg_full(243), 3, "f16x3"),
         ("f16x3 T=300 B=1 (long temporal)", cfg_full(300), 1, "f16x3"),
         ("f16x3 J=15 T=27 B=2", cfg_full(27, num_joints=15), 2, "f16x3"),
         ("f16x3 J=16 T=27 B=2", cfg_full(27, num_joints=16), 2, "f16x3"),
         ("f16x3 no time emb T=27 B=2", cfg_full(27, with_time_emb=False), 2, "f16x3"),
         ("f16x3 seq2frame T=27 B=2", cfg_full(27, seq2frame=True), 2, "f16x3"),
         ("bf16 T=27 B=5", cfg_full(27), 5, "bf16"),
         ("fp32 T=27 B=2", cfg_full(27), 2, "fp32"))
for name, cfg, B, prec in CASES:
    _, diff = build_product(cfg, 5, sampling=2, precision=prec)
    inp = inputs(B, cfg.num_frame, 78)
    x2d, nz = inp["x2d"], inp["noise"]
    if cfg.num_joints != 17:
        x2d, nz = x2d[:, :, :cfg.num_joints].contiguous(), nz[:, :, :cfg.num_joints].contiguous()
    if cfg.seq2frame:
        nz = nz[:, :1].contiguous()
    y = diff._engine(torch.device("cuda", 0)).ddim_sample(x2d.cuda(), nz.cuda())
    torch.cuda.synchronize()
    print(name, hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()[:16], flush=True)
    del diff
