// Front end of the 1x1-conv image classifier in one pass (pio_conv1x1_tokens): nn.Conv2d(C, N, kernel_size=1, stride=s) of
// an image batch and the channels-last copy behind it (io_processors.py ImagePreprocessor "conv1x1": convnet_1x1 ->
// movedim -> reshape, preprocessors.py:57-258), written once as the token rows [B, OH*OW, N] the encoder reads.  With
// OH = H / s, OW = W / s, m = i OW + j:
//
//   y[b, m, n] = fma chain  acc = bias ? bias[n] : 0;  c = 0 .. C-1 ascending: acc = fmaf(w[n, c], x[b, c, i s, j s], acc)
//
// The chain it replaces writes [B, N, OH, OW] (MIOpen), then reads and writes all of it again for the channels-last copy;
// this kernel reads the C planes once and stores every output element once.  It is bound by its stores: C <= 4 FMAs per
// 4-byte output.
//
// One wave owns a strip of 64 consecutive tokens m of one sample (a workgroup is four independent waves: no LDS, no barrier).
//   * lane = token while loading: each lane reads its pixel's C values (dword loads through the source's own four strides --
//     along an image row of a contiguous source a wave instruction reads 256 contiguous bytes; any stride, 4-byte alignment).
//   * lane = four output channels while storing: outputs n = 4 lane + 256 k (k < NV = ceil(N / 256)); the 4 C weights and 4
//     biases of each k stay in registers for the whole strip.
//   * per token the pixel's C values are broadcast from the owning lane's registers (v_readlane -> scalar operands of the
//     FMAs), and the row leaves as one 16-byte store per lane and k: at N = 256 one wave instruction writes one whole 1 KiB row,
//     a strip 64 KiB of contiguous rows.
//   * ONE fp32 FMA chain per output in the order above: the bits of a value depend on its pixel, its weights and its bias
//     only -- not on the batch, the grid or the strip it fell into.
// All offsets are 64-bit; the B * OH * OW rows must stay below 2^31.
//
// Stores are non-temporal (measured faster than plain ones: the note at cv_store).
#include "pio_internal.h"

namespace pio {

namespace {

constexpr int CV_STRIP = 64;   // tokens per wave
constexpr int CV_NMAX = 1024;  // == PIO_CONV1X1_MAX_N (pio_hip.h: the registers a lane keeps per 256 outputs)

// Non-temporal stores ship: measured faster than plain stores on an MI355X in the kernel alone at every size above one
// sample (B = 8: 79 against 82 us, 5.2 against 5.0 TB/s; B = 32: 297 against 312 us, 5.5 against 5.3 TB/s; B = 1: 11 us either
// way; two sessions each, five alternating repeats), and not slower in the whole forward, where the encoder's LayerNorm reads
// the rows next (B = 1: 3.60 - 3.61 against 3.61 - 3.65 ms; B = 8: 9.48 - 9.61 against 9.50 - 9.60 ms; three alternating
// runs, two sessions; profiles/classify_front_ends.json).  -DPIO_CONV1X1_PLAIN builds the plain-store variant for A/B runs.
#ifdef PIO_CONV1X1_PLAIN
__device__ __forceinline__ void cv_store(f32x4 *p, f32x4 v) { *p = v; }
#else
__device__ __forceinline__ void cv_store(f32x4 *p, f32x4 v) { __builtin_nontemporal_store(v, p); }
#endif

struct Conv1x1Args {
    const float *x, *w, *bias;
    float *y;
    int64_t sb, sc, sy, sx, ldw, ldy, sYb;  // sy, sx: already multiplied by the stride s
    int32_t OW, M, N, strips;               // strips per sample
    int64_t total;                          // strips of the launch
};

template <int C, int NV>
__global__ __launch_bounds__(256) void conv1x1_tokens_kernel(const Conv1x1Args a) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t strip = (int64_t)blockIdx.x * 4 + wave;
    if (strip >= a.total) return;
    const int b = (int)(strip / a.strips);
    const int m0 = (int)(strip - (int64_t)b * a.strips) * CV_STRIP;
    const int n = min(CV_STRIP, a.M - m0);

    float wv[NV][4][C], bv[NV][4];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int n0 = 4 * lane + 256 * k;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            bv[k][e] = (a.bias && n0 < a.N) ? a.bias[n0 + e] : 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) wv[k][e][c] = n0 < a.N ? a.w[(int64_t)(n0 + e) * a.ldw + c] : 0.0f;
        }
    }

    float xv[C];
#pragma unroll
    for (int c = 0; c < C; ++c) xv[c] = 0.0f;
    if (lane < n) {
        const int m = m0 + lane, i = m / a.OW, j = m - i * a.OW;
        const float *px = a.x + (int64_t)b * a.sb + (int64_t)i * a.sy + (int64_t)j * a.sx;
#pragma unroll
        for (int c = 0; c < C; ++c) xv[c] = px[(int64_t)c * a.sc];
    }

    float *yrow = a.y + (int64_t)b * a.sYb + (int64_t)m0 * a.ldy;
    for (int p = 0; p < n; ++p, yrow += a.ldy) {
        float xs[C];
#pragma unroll
        for (int c = 0; c < C; ++c)
            xs[c] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xv[c]), p));
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int n0 = 4 * lane + 256 * k;
            if (n0 < a.N) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float acc = bv[k][e];
#pragma unroll
                    for (int c = 0; c < C; ++c) acc = __builtin_fmaf(wv[k][e][c], xs[c], acc);
                    v[e] = acc;
                }
                cv_store(reinterpret_cast<f32x4 *>(yrow + n0), v);
            }
        }
    }
}

}  // namespace

int conv1x1_tokens_launch(const float *x, int64_t sb, int64_t sc, int64_t sy, int64_t sx, const float *w, int64_t ldw,
                          const float *bias, float *y, int64_t ldy, int64_t sYb, int B, int C, int H, int W, int s, int N,
                          hipStream_t st) {
    if (!x || !w || !y) return PIO_E_ARG;
    if (B < 1 || H < 1 || W < 1 || C < 1 || C > 4 || s < 1 || s > 8 || N < 4 || N > CV_NMAX || N % 4 != 0) return PIO_E_SHAPE;
    if (H % s != 0 || W % s != 0 || ldw < C || ldy < N) return PIO_E_SHAPE;
    const int OH = H / s, OW = W / s;
    const int64_t M = (int64_t)OH * OW;
    if (M * B > 0x7fffffffLL) return PIO_E_SHAPE;
    if (B > 1 && (ldy > INT64_MAX / M || sYb < M * ldy)) return PIO_E_SHAPE;
    if (ldy % 4 != 0 || (B > 1 && sYb % 4 != 0) || ((uintptr_t)y & 15) ||
        (((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias) & 3))
        return PIO_E_ALIGN;
    Conv1x1Args a;
    a.x = x, a.w = w, a.bias = bias, a.y = y;
    a.sb = B > 1 ? sb : 0, a.sc = sc, a.sy = sy * s, a.sx = sx * s, a.ldw = ldw, a.ldy = ldy, a.sYb = B > 1 ? sYb : 0;
    a.OW = OW, a.M = (int32_t)M, a.N = N, a.strips = (int32_t)((M + CV_STRIP - 1) / CV_STRIP);
    a.total = (int64_t)a.strips * B;
    const double px = (double)M * B;
    ProfScope prof(PROF_LAYERNORM, 2.0 * px * C * N, 4.0 * px * (C + N), st);
    const dim3 grid((unsigned)((a.total + 3) / 4));
#define PIO_CONV1X1_LAUNCH(CC, NV) hipLaunchKernelGGL((conv1x1_tokens_kernel<CC, NV>), grid, dim3(256), 0, st, a)
#define PIO_CONV1X1_BY_N(CC)                                                                                           \
    switch ((N + 255) / 256) {                                                                                         \
        case 1: PIO_CONV1X1_LAUNCH(CC, 1); break;                                                                      \
        case 2: PIO_CONV1X1_LAUNCH(CC, 2); break;                                                                      \
        case 3: PIO_CONV1X1_LAUNCH(CC, 3); break;                                                                      \
        default: PIO_CONV1X1_LAUNCH(CC, 4); break;                                                                     \
    }
    switch (C) {
        case 1: PIO_CONV1X1_BY_N(1) break;
        case 2: PIO_CONV1X1_BY_N(2) break;
        case 3: PIO_CONV1X1_BY_N(3) break;
        default: PIO_CONV1X1_BY_N(4) break;
    }
#undef PIO_CONV1X1_BY_N
#undef PIO_CONV1X1_LAUNCH
    return launch_status();
}

}  // namespace pio
