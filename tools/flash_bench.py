"""Dev tool (GPU): device time of the fused SELF-attention kernel on the hot shape (B x 512 latents x 8 heads of 128,
V row-major out of the fused q|k|v GEMM).  PIO_FLASH_PIPE=0 selects the lock-step 8-wave kernel for comparison.
--pair: the language model's stack shape instead (B x 256 latents x 8 heads of (32, 160)) under "fp16x3fq" -- the pair-operand
flash_attn_kernel<32,160> -- and under "fp16x3f" (single-operand xattn_kernel<32,160>), B = 2 and 100.
--pair-wide: the classifier's stack shape (B x 512 x 512, 8 heads of (128, 128), V^T) through the raw entry
pio_flash_attention_pair: the pair-operand flash_attn_kernel<128,128> next to its single-operand sibling (Q_lo = K_lo =
NULL) on the same buffers, B = 32 and 4; device time per launch from the library's launch accounting."""
import ctypes as C
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT]
import torch  # noqa: E402
import perceiverio_pytorch_amd as P  # noqa: E402
from perceiverio_pytorch_amd import _lib as L  # noqa: E402
from perceiverio_pytorch_amd.transformer_primitives import SelfAttention  # noqa: E402


def pair_wide(lib, dev):
    H, T, d, n = 8, 512, 128, 20
    s = torch.cuda.current_stream(dev).cuda_stream
    for B in (32, 4):
        q, k = (torch.randn(B, T, H * d, device=dev) for _ in range(2))
        qh, kh = q.half(), k.half()
        ql, kl = (q - qh.float()).half(), (k - kh.float()).half()
        vt = torch.rand(B, H * d, T, device=dev).half()
        o, olo = (torch.empty(B, T, H * d, dtype=torch.float16, device=dev) for _ in range(2))
        strides = (H * d, H * d, T, H * d, T * H * d, T * H * d, H * d * T, T * H * d)
        res = {}
        for pair in (False, True):
            def launch():
                L.check(lib.pio_flash_attention_pair(L.PIO_DT_F16, d, d, d, qh.data_ptr(), ql.data_ptr() if pair else None,
                                                     kh.data_ptr(), kl.data_ptr() if pair else None, vt.data_ptr(),
                                                     o.data_ptr(), olo.data_ptr() if pair else None, B, H, T, T, *strides,
                                                     0, None, None, 1, None, 0, s), "pio_flash_attention_pair")
            for _ in range(3):
                launch()
            torch.cuda.synchronize()
            L.check(lib.pio_prof_begin(4096))
            for _ in range(n):
                launch()
            ms = (C.c_double * 9)(); fl = (C.c_double * 9)(); ln = (C.c_int64 * 9)()
            lib.pio_prof_end(ms, fl, None, ln)
            res[pair] = us = ms[5] / n * 1e3
            print(f"[{'pair' if pair else 'single'}] B={B} H={H} {T} x {T} (128, 128) V^T: {us:8.1f} us per launch "
                  f"({fl[5] / n / (us * 1e-6) / 1e12:7.1f} algorithmic TFLOP/s, {ln[5] // n} launch) "
                  f"checksum {float(o.double().abs().mean()):.6f}", flush=True)
        print(f"B={B}: pair / single = {res[True] / res[False]:.2f}", flush=True)


def main():
    lib = P.lib()
    dev = torch.device("cuda:0")
    if "--pair-wide" in sys.argv:
        return pair_wide(lib, dev)
    pair = "--pair" in sys.argv
    runs = ([(B, 256, 1280, pol) for B in (2, 100) for pol in ("fp16x3f", "fp16x3fq")] if pair
            else [(B, T, 1024, "fp16") for B, T in ((32, 512), (32, 1024), (4, 512))])
    for B, T, D, policy in runs:
        P.set_precision_policy(policy)
        m = (SelfAttention(D, widening_factor=1, num_heads=8, qk_channels=256) if pair
             else SelfAttention(D, widening_factor=1, num_heads=8)).to(dev).eval()
        x = torch.randn(B, T, D, device=dev)
        with torch.no_grad():
            for _ in range(3):
                y = m(x)
            torch.cuda.synchronize()
            n = 20
            L.check(lib.pio_prof_begin(4096))
            for _ in range(n):
                m(x)
            ms = (C.c_double * 9)(); fl = (C.c_double * 9)(); by = (C.c_double * 9)(); ln = (C.c_int64 * 9)()
            lib.pio_prof_end(ms, fl, by, ln)
        us = ms[5] / n * 1e3
        print("   per class us per forward:", {k: round(ms[k] / n * 1e3, 1) for k in range(9) if ms[k] > 0}, flush=True)
        print(f"[{policy}] B={B} T={T} D={D}: fused self-attention {us:8.1f} us ({fl[5] / n / (us * 1e-6) / 1e12:7.1f} algorithmic "
              f"TFLOP/s, {ln[5] // n} launches) PIO_FLASH_PIPE={os.environ.get('PIO_FLASH_PIPE', '1')} "
              f"checksum {float(y.double().abs().mean()):.6f}", flush=True)


if __name__ == "__main__":
    main()
