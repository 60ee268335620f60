#!/usr/bin/env python3
"""Times the attention kernel at the network's shapes, one line per shape and work decomposition.

python tools/attn_tune.py            the library's own choice (under MSLAM_ATTN_SPLIT, one process per setting), then
                                     every instantiated (key split, query groups per block) pair through
                                     mslam_attention_bf16_cfg
python tools/attn_tune.py REPS       the same, REPS times over (the spread of a line is its run-to-run range)

Shapes (batch, heads) at 768 x 768 tokens: one frame through the encoder (1, 16), one pair through the decoder (2, 12),
backend batches of the decoder (4, 12), (8, 12) and of the encoder (8, 16), and the loop's encoder batch of 12 frames
(12, 16) and decoder group of 6 pairs (12, 12)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam-quality-dualtsdf_amd"), os.path.join(ROOT, "tools")]
from bench_kernels import attn
SHAPES = ((1, 16), (1, 12), (2, 12), (4, 12), (8, 12), (8, 16), (12, 12), (12, 16))
CONFIGS = ((2, 2), (2, 4), (4, 2))   # what csrc/attention.hip instantiates; add a pair there to time it here
if __name__ == "__main__":
    print("split", os.environ.get("MSLAM_ATTN_SPLIT", "auto"))
    for _ in range(int(sys.argv[1]) if len(sys.argv) > 1 else 1):
        for B, H in SHAPES:
            attn(B, H, 768)
            for cfg in CONFIGS:
                attn(B, H, 768, cfg)
