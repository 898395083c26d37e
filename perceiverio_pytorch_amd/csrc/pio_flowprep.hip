// Front end of the optical-flow model in one pass (pio_flow_patch_tokens): the zero-padded 3x3 neighbourhood of every
// pixel of a frame pair (processor_utils.py:98-116 patches_for_flow -> :59-95 extract_patches), the two frames side by
// side in the channel axis (processor_utils.py:21-38 space_to_depth, temporal block 2) and the 1x1 projection behind them
// (preprocessors.py: conv_after_patching, nn.Linear(18 C, out)) -- algebraically ONE 3x3 "same" convolution from the
// 2 C input planes to `out` channels-last outputs:
//
//   y[n, r W + x, o] = bias[o] + sum_{t, py, px, c} w[o, t 9C + (py 3 + px) C + c] * frame_t[n, c, r + py - 1, x + px - 1]
//
// with 0 outside the image.  The chain it replaces (stack, pad, unfold, two permute copies, a BLAS call) writes 27 values
// per pixel and frame three times over; this kernel reads the 2 C planes once and writes the [N, H W, out] fp32 features.
//
// One workgroup (four waves) owns a 4-row x 64-column tile of one sample; wave = row, lane = column.
//   * The (4 + 2) x (64 + 2) halo of the 2 C planes is staged in LDS with one guarded dword load per cell: a cell outside
//     [0, H) x [0, W) is written as 0 and its address is never formed into a load.  Frames may be arbitrary strided views
//     (x contiguous, 4-byte aligned), so there is no wider load to make.
//   * A lane gathers its pixel's K = 18 C taps from LDS (lane-consecutive dwords: conflict-free) into registers, in the
//     channel order of the formula above.
//   * Weights and bias are wave-uniform: indexed by loop counters only, they arrive through the scalar cache as operands of
//     the FMAs and cost neither LDS nor vector registers.  16 outputs (then 4 for a tail) are accumulated at a time, each
//     as ONE fp32 FMA chain bias -> k = 0 .. K-1: the result does not depend on the launch geometry and is bit-identical
//     from run to run.
//   * Each lane stores its pixel's outputs as 16-byte vectors (rows are 16-byte aligned: ldy % 4 == 0).
//   * w == NULL: the K taps themselves are the output (conv_after_patching = False); K is even, rows leave as 8-byte vectors.
#include "pio_internal.h"

namespace pio {

namespace {

constexpr int FP_TH = 4, FP_TW = 64;            // tile: rows (= waves) x columns (= lanes)
constexpr int FP_HH = FP_TH + 2, FP_HW = FP_TW + 2;

typedef float f32x2 __attribute__((ext_vector_type(2)));

// NO outputs o0 .. o0 + NO - 1 of one pixel: bias + the FMA chain over the K taps in x, stored as NO / 4 16-byte vectors
template <int K, int NO>
__device__ __forceinline__ void flow_project(const float (&x)[K], const float *__restrict__ w,
                                             const float *__restrict__ bias, int o0, float *__restrict__ yrow) {
    float acc[NO];
#pragma unroll
    for (int j = 0; j < NO; ++j) acc[j] = bias[o0 + j];
#pragma unroll
    for (int j = 0; j < NO; ++j) {
        const float *wr = w + (int64_t)(o0 + j) * K;
#pragma unroll
        for (int k = 0; k < K; ++k) acc[j] = __builtin_fmaf(wr[k], x[k], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < NO; j += 4) {
        f32x4 v = {acc[j], acc[j + 1], acc[j + 2], acc[j + 3]};
        *reinterpret_cast<f32x4 *>(yrow + o0 + j) = v;
    }
}

template <int C>
__global__ __launch_bounds__(256) void flow_patch_tokens_kernel(const float *__restrict__ f0, const float *__restrict__ f1,
                                                                int64_t sn0, int64_t sc0, int64_t sy0, int64_t sn1,
                                                                int64_t sc1, int64_t sy1, const float *__restrict__ w,
                                                                const float *__restrict__ bias, float *__restrict__ y,
                                                                int64_t ldy, int H, int W, int out) {
    constexpr int K = 18 * C;
    __shared__ float halo[2 * C * FP_HH * FP_HW];  // [plane = t C + c][row][column]
    const int n = blockIdx.z, r0 = blockIdx.y * FP_TH, c0 = blockIdx.x * FP_TW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    for (int idx = threadIdx.x; idx < 2 * C * FP_HH * FP_HW; idx += 256) {
        const int p = idx / (FP_HH * FP_HW), rem = idx - p * (FP_HH * FP_HW);
        const int hr = rem / FP_HW, hc = rem - hr * FP_HW;
        const int gy = r0 - 1 + hr, gx = c0 - 1 + hc;
        float v = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const int t = p / C, c = p - t * C;
            v = t == 0 ? f0[(int64_t)n * sn0 + (int64_t)c * sc0 + (int64_t)gy * sy0 + gx]
                       : f1[(int64_t)n * sn1 + (int64_t)c * sc1 + (int64_t)gy * sy1 + gx];
        }
        halo[idx] = v;
    }
    __syncthreads();

    const int gy = r0 + wave, gx = c0 + lane;
    if (gy >= H || gx >= W) return;

    float x[K];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int py = 0; py < 3; ++py)
#pragma unroll
            for (int px = 0; px < 3; ++px)
#pragma unroll
                for (int c = 0; c < C; ++c)
                    x[t * 9 * C + (py * 3 + px) * C + c] = halo[((t * C + c) * FP_HH + wave + py) * FP_HW + lane + px];

    float *yrow = y + ((int64_t)n * H * W + (int64_t)gy * W + gx) * ldy;
    if (w == nullptr) {  // raw patches: out == K
#pragma unroll
        for (int k = 0; k < K; k += 2) {
            f32x2 v = {x[k], x[k + 1]};
            *reinterpret_cast<f32x2 *>(yrow + k) = v;
        }
        return;
    }
    int o0 = 0;
    for (; o0 + 16 <= out; o0 += 16) flow_project<K, 16>(x, w, bias, o0, yrow);
    for (; o0 < out; o0 += 4) flow_project<K, 4>(x, w, bias, o0, yrow);
}

}  // namespace

int flow_patch_tokens_launch(const float *f0, const float *f1, int64_t sn0, int64_t sc0, int64_t sy0, int64_t sn1,
                             int64_t sc1, int64_t sy1, const float *w, const float *bias, float *y, int64_t ldy, int N,
                             int C, int H, int W, int out, hipStream_t s) {
    if (!f0 || !f1 || !y || (w && !bias)) return PIO_E_ARG;
    if (N <= 0 || H <= 0 || W <= 0 || C < 1 || C > 4 || out <= 0 || out > 128) return PIO_E_SHAPE;
    if (w ? (out % 4 != 0) : (out != 18 * C)) return PIO_E_SHAPE;
    if (ldy < out) return PIO_E_SHAPE;
    const int tx = (W + FP_TW - 1) / FP_TW, ty = (H + FP_TH - 1) / FP_TH;
    if (N > 65535 || ty > 65535) return PIO_E_SHAPE;
    if (ldy % 4 != 0 || ((uintptr_t)y & 15) || ((uintptr_t)f0 & 3) || ((uintptr_t)f1 & 3) || ((uintptr_t)w & 3) ||
        ((uintptr_t)bias & 3))
        return PIO_E_ALIGN;
    const double px = (double)N * H * W;
    ProfScope prof(PROF_LAYERNORM, w ? 2.0 * px * 18 * C * out : 0.0, 4.0 * px * (2 * C + out), s);
    const dim3 grid((unsigned)tx, (unsigned)ty, (unsigned)N);
#define PIO_FLOWPREP_LAUNCH(CC)                                                                                        \
    hipLaunchKernelGGL(flow_patch_tokens_kernel<CC>, grid, dim3(256), 0, s, f0, f1, sn0, sc0, sy0, sn1, sc1, sy1, w, bias, \
                       y, ldy, H, W, out)
    switch (C) {
        case 1: PIO_FLOWPREP_LAUNCH(1); break;
        case 2: PIO_FLOWPREP_LAUNCH(2); break;
        case 3: PIO_FLOWPREP_LAUNCH(3); break;
        default: PIO_FLOWPREP_LAUNCH(4); break;
    }
#undef PIO_FLOWPREP_LAUNCH
    return launch_status();
}

}  // namespace pio
