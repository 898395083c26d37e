// Narrow output heads behind the decoder in one pass (pio_project_heads): up to four row segments of the decoder output
// x [B, Q, K] fp32, each with its own small linear head (1 .. 16 output columns), written straight into each head's final
// output array:
//
//   y_s[b, r, j] = bias_s[j] + sum_k w_s[j, k] x[b, row0_s + r, k]          r in [0, rows_s), j in [0, n_out_s)
//
// The chain this stands for (postprocessors.py ProjectionPostprocessor / AudioPostprocessor through runtime.hip_linear)
// copies the row slice, rounds it to 16 bits (twice under a split policy), multiplies and copies the result into place;
// here x is read once, as fp32, and multiplied as fp32.  A head this narrow is bound by the read of its input.
//
// One workgroup (four waves) owns a strip of HD_TS consecutive rows of one segment of one sample; the grid is the flat list
// of strips times B.  The block stages its segment's weights once in LDS ([NO, K] fp32, NO = n_out rounded up to 1, 2, 3, 4, 8
// or 16, the rows behind n_out zero).  A WAVE owns a row; four rows are in flight per wave, two for heads of more than 4 columns
// (16-byte loads of x, one LDS weight read serves all of them).
//
// SUMMATION ORDER (part of the definition: the bits of an output row depend on that row of x, w, bias, n_out and K only).
// Lane l of the wave owns the floats k = 4 (l + 64 i) + e, e = 0 .. 3, i = 0 .. ceil(K / 256) - 1, with k < K:
//   p_l = +0;  for i ascending, for e ascending:  p_l = fmaf(w[j, k], x[k], p_l)      (lanes with no k < K keep +0)
//   s   = xor-shuffle tree over the 64 lanes, offsets 32, 16, 8, 4, 2, 1:  p_l = fadd_rn(p_l, p_(l xor offset))
//   y   = bias ? fadd_rn(s, bias[j]) : s
// Every lane ends with the same s (fp32 addition commutes), lane j < n_out stores it.  No atomics, nothing depends on B, Q,
// row0, rows, the strides, the other segments or the block a row lands in: rows past the end of a strip recompute the
// strip's last row and store nothing.
//   * All offsets are 64-bit.  The segment table travels by value in the kernel arguments.  Only vector stores.
#include "pio_device.h"

namespace pio {

namespace {

constexpr int HD_TS = 64;                 // rows per strip: four waves, HD_R rows in flight per wave (4; 2 from 8 columns on)
constexpr size_t HD_MAX_LDS = 64 * 1024;  // [16, 1024] fp32: the widest head at the longest K

struct HeadSeg {
    const float *w, *bias;
    float *y;
    int64_t ldw, y_sb, y_rs;
    int32_t row0, rows, n_out, no, strip0;  // no: n_out rounded up to an instantiated width
};
struct HeadArgs {
    HeadSeg seg[PIO_MAX_HEAD_SEGMENTS];
    int32_t nseg, strips;  // strips: per sample
};

template <int NO, int HD_R>
__device__ __forceinline__ void head_rows(const HeadSeg &g, const float *__restrict__ xs, int64_t ldx, int K, int b, int m0,
                                          int n, const float *wl) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sweeps = (K + 255) >> 8;
    for (int r0 = wave * HD_R; r0 < n; r0 += 4 * HD_R) {
        const float *xr[HD_R];
#pragma unroll
        for (int q = 0; q < HD_R; ++q) xr[q] = xs + (int64_t)(g.row0 + m0 + min(r0 + q, n - 1)) * ldx;
        float acc[HD_R][NO];
#pragma unroll
        for (int q = 0; q < HD_R; ++q)
#pragma unroll
            for (int j = 0; j < NO; ++j) acc[q][j] = 0.0f;
        for (int i = 0; i < sweeps; ++i) {
            const int k = 4 * (lane + 64 * i);
            if (k < K) {
                f32x4 xv[HD_R];
#pragma unroll
                for (int q = 0; q < HD_R; ++q) xv[q] = *reinterpret_cast<const f32x4 *>(xr[q] + k);
#pragma unroll
                for (int j = 0; j < NO; ++j) {
                    const f32x4 wv = *reinterpret_cast<const f32x4 *>(wl + j * K + k);
#pragma unroll
                    for (int q = 0; q < HD_R; ++q) {
                        float p = acc[q][j];
                        p = __fmaf_rn(wv.x, xv[q].x, p);
                        p = __fmaf_rn(wv.y, xv[q].y, p);
                        p = __fmaf_rn(wv.z, xv[q].z, p);
                        p = __fmaf_rn(wv.w, xv[q].w, p);
                        acc[q][j] = p;
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < HD_R; ++q) {
            float mine = 0.0f;
#pragma unroll
            for (int j = 0; j < NO; ++j) {
                float p = acc[q][j];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) p = __fadd_rn(p, __shfl_xor(p, off, 64));
                if (lane == j) mine = p;
            }
            if (r0 + q < n && lane < g.n_out) {
                if (g.bias) mine = __fadd_rn(mine, g.bias[lane]);
                g.y[(int64_t)b * g.y_sb + (int64_t)(m0 + r0 + q) * g.y_rs + lane] = mine;
            }
        }
    }
}

__global__ __launch_bounds__(256) void project_heads_kernel(const HeadArgs a, const float *__restrict__ x, int64_t x_sb,
                                                            int64_t ldx, int K) {
    extern __shared__ __align__(16) float hd_lds[];
    const int b = blockIdx.x / a.strips, strip = blockIdx.x - b * a.strips;
    int si = 0;
#pragma unroll
    for (int i = 1; i < PIO_MAX_HEAD_SEGMENTS; ++i)
        if (i < a.nseg && strip >= a.seg[i].strip0) si = i;
    const HeadSeg &g = a.seg[si];
    const int m0 = (strip - g.strip0) * HD_TS;
    const int n = min(HD_TS, g.rows - m0);

    // the segment's weights, once per block: [no, K] with zero rows behind n_out (K % 4 == 0: whole 16-byte pieces)
    const int kv = K >> 2;
    for (int v = threadIdx.x; v < g.no * kv; v += 256) {
        const int j = v / kv, k = (v - j * kv) * 4;
        f32x4 wv = {0.0f, 0.0f, 0.0f, 0.0f};
        if (j < g.n_out) wv = *reinterpret_cast<const f32x4 *>(g.w + (int64_t)j * g.ldw + k);
        *reinterpret_cast<f32x4 *>(hd_lds + j * K + k) = wv;
    }
    __syncthreads();

    const float *xs = x + (int64_t)b * x_sb;
    switch (g.no) {
        case 1: head_rows<1, 4>(g, xs, ldx, K, b, m0, n, hd_lds); break;
        case 2: head_rows<2, 4>(g, xs, ldx, K, b, m0, n, hd_lds); break;
        case 3: head_rows<3, 4>(g, xs, ldx, K, b, m0, n, hd_lds); break;
        case 4: head_rows<4, 4>(g, xs, ldx, K, b, m0, n, hd_lds); break;
        case 8: head_rows<8, 2>(g, xs, ldx, K, b, m0, n, hd_lds); break;
        default: head_rows<16, 2>(g, xs, ldx, K, b, m0, n, hd_lds); break;
    }
}

}  // namespace

int project_heads_launch(const pio_head_segment_t *segs, int nseg, const float *x, int64_t x_sb, int64_t ldx, int B, int Q,
                         int K, hipStream_t s) {
    if (!segs || !x || nseg < 1 || nseg > PIO_MAX_HEAD_SEGMENTS) return PIO_E_ARG;
    for (int i = 0; i < nseg; ++i)
        if (!segs[i].w || !segs[i].y) return PIO_E_ARG;
    if (B < 1 || Q < 1 || K < 4 || K > 1024 || (K & 3) || ldx < K) return PIO_E_SHAPE;
    HeadArgs a;
    int64_t strips = 0;
    size_t lds = 0;
    double bytes = 0.0;
    for (int i = 0; i < nseg; ++i) {
        const pio_head_segment_t &g = segs[i];
        if (g.n_out < 1 || g.n_out > 16 || g.rows < 0 || g.ldw < K || g.y_rs < g.n_out) return PIO_E_SHAPE;
        if (g.row0 < 0 || (int64_t)g.row0 + g.rows > Q) return PIO_E_SHAPE;
        for (int k = 0; k < i; ++k)  // (an empty range overlaps nothing)
            if (g.rows > 0 && segs[k].rows > 0 && (int64_t)g.row0 < (int64_t)segs[k].row0 + segs[k].rows &&
                (int64_t)segs[k].row0 < (int64_t)g.row0 + g.rows)
                return PIO_E_SHAPE;
        const int no = g.n_out <= 4 ? g.n_out : g.n_out <= 8 ? 8 : 16;
        a.seg[i] = HeadSeg{g.w, g.bias, g.y, g.ldw, g.y_sb, g.y_rs, g.row0, g.rows, g.n_out, no, (int32_t)strips};
        strips += (g.rows + HD_TS - 1) / HD_TS;
        const size_t need = sizeof(float) * (size_t)no * K;
        lds = need > lds ? need : lds;
        bytes += (double)B * g.rows * 4.0 * (K + g.n_out);
    }
    if (lds > HD_MAX_LDS || strips * B > 0x7fffffffLL) return PIO_E_SHAPE;
    if (((uintptr_t)x & 15) || (ldx & 3) || (x_sb & 3)) return PIO_E_ALIGN;
    for (int i = 0; i < nseg; ++i) {
        const pio_head_segment_t &g = segs[i];
        if (((uintptr_t)g.w & 15) || (g.ldw & 3) || (((uintptr_t)g.y | (uintptr_t)g.bias) & 3)) return PIO_E_ALIGN;
    }
    if (strips == 0) return PIO_OK;  // (only empty segments: nothing to do)
    a.nseg = nseg;
    a.strips = (int32_t)strips;
    for (int i = nseg; i < PIO_MAX_HEAD_SEGMENTS; ++i) a.seg[i] = a.seg[0];
    ProfScope prof(PROF_LAYERNORM, 0.0, bytes, s);
    hipLaunchKernelGGL(project_heads_kernel, dim3((unsigned)(strips * B)), dim3(256), lds, s, a, x, x_sb, ldx, K);
    return launch_status();
}

}  // namespace pio
