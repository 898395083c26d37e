"""Dev tool (GPU): where a 512-row projection's ~10 us go -- time against K (slope = the K loop, intercept = launch +
prologue + epilogue), against N, and with the tile choice forced (pio_gemm_kernel_override: 0 automatic, 64, 128)."""
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
import gemm_bench as G  # noqa: E402

for ov in (0, 64, 128):
    G.lib.pio_gemm_kernel_override(ov)
    print(f"override {ov}", flush=True)
    for M in (512, 1024, 2048):
        for K in (256, 512, 1024, 2048):
            G.run(M, 1024, K, False, False, 0, iters=200)
        G.run(M, 3072, 1024, False, False, 0, iters=200)
    G.run(2048, 1536, 512, False, False, 0, iters=200)
    G.run(2048, 512, 512, False, False, 0, iters=200)
G.lib.pio_gemm_kernel_override(0)
