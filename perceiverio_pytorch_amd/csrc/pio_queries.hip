// Decoder queries of the multimodal model in one pass (pio_build_queries): per output modality the Fourier features of
// its sub-sampled index points (output_queries.py BasicQuery._encode -> position_encoding.py generate_fourier_features)
// or a learned table, the learned padding embedding behind them, the modalities one after the other along the row axis
// (perceiver.py PerceiverIO.decoder_query).  Batch-invariant: ONE [Qtot, Cq] fp32 array.  Per segment and row m:
//
//   FOURIER: i = (points ? points[m] : start + m) mod prod(dims), coordinates = row-major unravel of i,
//            p_j = axis[j][coord_j],  phase(j, k) = fmul(fmul(p_j, bands[j, k]), (float)pi)   (two rounded products)
//     x[0 : d]                   = p_j                       (concat_pos only; the blocks behind it move down otherwise)
//     x[c0 + j K + k]            = sinf(phase(j, k))
//     x[c0 + d K + j K + k]      = cosf(phase(j, k))         (unless sine_only)
//     x[width : Cq]              = pad[c - width]
//   TABLE:   x[0 : C] = table[m, :],  x[C : Cq] = pad[c - C]
//   y[row0 + m, c] = x[c]
//
// The chain of torch ops this stands for writes every element several times and keeps temporaries of the result's size;
// here every output element is stored once.
//
// One workgroup (four waves) owns a strip of QR_TS consecutive rows of one segment; the grid is the flat list of strips.
//   * FOURIER, three steps with a barrier between them.  (1) one thread per row unravels the index and reads the d
//     coordinates; one thread per axis then marks, for every row, the first row of the run of equal coordinates it
//     belongs to (consecutive points share t and y of a video for a whole image row).  (2) wave = row, lane = (j, k):
//     the rows that START a run evaluate sincosf of the phase ONCE and leave sine and cosine in the strip's feature
//     rows in LDS, laid out as the channels are; the other rows of the run read the first one's.  The accurate sincosf
//     (no fast intrinsics: a phase reaches 48 255 rad) and __fmul_rn, so nothing contracts or reassociates the phase.
//     (3) wave = output row, lanes = that row's 16-byte vectors (Cq % 4 == 0, y 16-byte aligned, ldy % 4 == 0), 8-byte
//     vectors (Cq % 2 == 0, y 8-byte aligned, ldy % 2 == 0: the shipped 1026) or dwords; a lane composes its vector
//     element by element because the three ranges start at arbitrary channels.
//   * All offsets are 64-bit.  The segment table travels by value in the kernel arguments.
#include "pio_internal.h"

namespace pio {

namespace {

constexpr int QR_TS = 32;                 // rows per strip
constexpr size_t QR_MAX_LDS = 64 * 1024;  // the strip's feature rows have to fit

struct QrySeg {
    const float *axis[3], *bands, *table, *pad;
    const int64_t *points;
    int64_t start, ldb, ldt, total;
    int32_t kind, row0, M, d, K, dims[3], c0, width, F, sine_only, strip0;  // width: channels in front of the padding
};
struct QryArgs {
    QrySeg seg[PIO_MAX_QUERY_SEGMENTS];
    int32_t nseg;
};

typedef float f32x2 __attribute__((ext_vector_type(2)));

// V = 4 / 2 / 1: rows leave as 16-byte vectors, 8-byte vectors, dwords
template <int V>
__global__ __launch_bounds__(256) void build_queries_kernel(const QryArgs a, float *__restrict__ y, int64_t ldy, int Cq) {
    extern __shared__ __align__(16) float qr_lds[];
    // [QR_TS x 3 positions] [QR_TS x 3 coordinates] [QR_TS x 3 run starts] [d K axis of a (j, k) pair] [QR_TS x F features]
    float *pos = qr_lds;
    int *coord = reinterpret_cast<int *>(qr_lds + 3 * QR_TS);
    int *src = reinterpret_cast<int *>(qr_lds + 6 * QR_TS);
    int *axis_of = reinterpret_cast<int *>(qr_lds + 9 * QR_TS);

    const int strip = blockIdx.x;
    int si = 0;
#pragma unroll
    for (int i = 1; i < PIO_MAX_QUERY_SEGMENTS; ++i)
        if (i < a.nseg && strip >= a.seg[i].strip0) si = i;
    const QrySeg &g = a.seg[si];
    const int m0 = (strip - g.strip0) * QR_TS;
    const int n = min(QR_TS, g.M - m0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int dK = g.d * g.K, F = g.F, c0 = g.c0, width = g.width;
    float *feat = qr_lds + 9 * QR_TS + dK;
    const bool fourier = g.kind == PIO_QUERY_FOURIER;

    if (fourier) {
        if ((int)threadIdx.x < n) {
            const int64_t m = m0 + (int)threadIdx.x;
            int64_t i = (g.points ? g.points[m] : g.start + m) % g.total;
            if (i < 0) i += g.total;
#pragma unroll
            for (int j = 2; j >= 0; --j)
                if (j < g.d) {
                    const int cj = (int)(i % g.dims[j]);
                    i /= g.dims[j];
                    coord[threadIdx.x * 3 + j] = cj;
                    pos[threadIdx.x * 3 + j] = g.axis[j][cj];
                }
        }
        for (int q = threadIdx.x; q < dK; q += 256) axis_of[q] = q / g.K;
        __syncthreads();
        if ((int)threadIdx.x < g.d) {
            const int j = threadIdx.x;
            int first = 0;
            for (int r = 0; r < n; ++r) {
                if (r > 0 && coord[r * 3 + j] != coord[(r - 1) * 3 + j]) first = r;
                src[r * 3 + j] = first;
            }
        }
        __syncthreads();
        for (int r = wave; r < n; r += 4)
            for (int q = lane; q < dK; q += 64) {
                const int j = axis_of[q];
                if (src[r * 3 + j] != r) continue;
                const float band = g.bands[(int64_t)j * g.ldb + (q - j * g.K)];
                const float phase = __fmul_rn(__fmul_rn(pos[r * 3 + j], band), 3.14159274101257324f);  // (float)M_PI
                if (g.sine_only) {
                    feat[r * F + q] = sinf(phase);
                } else {
                    float sn, cs;
                    sincosf(phase, &sn, &cs);
                    feat[r * F + q] = sn;
                    feat[r * F + dK + q] = cs;
                }
            }
        __syncthreads();
    }

    for (int r = wave; r < n; r += 4) {
        const int64_t m = m0 + r;
        const float *trow = g.table + m * g.ldt;  // (TABLE only)
        const float *prow = g.pad - width;        // (indexed with c >= width only)
        float *yrow = y + (g.row0 + m) * ldy;
        for (int cv = lane; cv * V < Cq; cv += 64) {
            float v[V];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int c = cv * V + e;
                float x;
                if (c >= width) {
                    x = prow[c];
                } else if (!fourier) {
                    x = trow[c];
                } else if (c < c0) {
                    x = pos[r * 3 + c];
                } else {
                    const int q = c - c0;
                    x = feat[src[r * 3 + axis_of[q >= dK ? q - dK : q]] * F + q];
                }
                v[e] = x;
            }
            if constexpr (V == 4) {
                f32x4 o = {v[0], v[1], v[2], v[3]};
                reinterpret_cast<f32x4 *>(yrow)[cv] = o;
            } else if constexpr (V == 2) {
                f32x2 o = {v[0], v[1]};
                reinterpret_cast<f32x2 *>(yrow)[cv] = o;
            } else {
                yrow[cv] = v[0];
            }
        }
    }
}

}  // namespace

int build_queries_launch(const pio_query_segment_t *segs, int nseg, float *y, int64_t ldy, int Qtot, int Cq,
                         hipStream_t s) {
    if (!y || !segs || nseg < 1 || nseg > PIO_MAX_QUERY_SEGMENTS) return PIO_E_ARG;
    for (int i = 0; i < nseg; ++i) {
        const pio_query_segment_t &g = segs[i];
        if (g.kind == PIO_QUERY_FOURIER) {
            if (g.d < 1 || g.d > 3 || g.K < 1 || !g.bands) return PIO_E_ARG;
            for (int j = 0; j < g.d; ++j)
                if (!g.axis[j]) return PIO_E_ARG;
        } else if (g.kind == PIO_QUERY_TABLE) {
            if (g.C > 0 && !g.table) return PIO_E_ARG;
        } else {
            return PIO_E_ARG;
        }
    }
    if (Qtot <= 0 || Cq <= 0 || ldy < Cq) return PIO_E_SHAPE;
    QryArgs a;
    int64_t strips = 0;
    size_t lds = 0;
    double bytes = 0.0;
    for (int i = 0; i < nseg; ++i) {
        const pio_query_segment_t &g = segs[i];
        QrySeg &t = a.seg[i];
        t = QrySeg{{g.axis[0], g.axis[1], g.axis[2]}, g.bands, g.table, g.pad, g.points, g.start, g.ldb, g.ldt, 1,
                   g.kind, g.row0, g.M, 0, 1, {1, 1, 1}, 0, 0, 0, g.sine_only != 0, (int32_t)strips};
        if (g.M <= 0) return PIO_E_SHAPE;
        int64_t width;
        if (g.kind == PIO_QUERY_FOURIER) {
            const int64_t dK = (int64_t)g.d * g.K, F = dK * (g.sine_only ? 1 : 2);
            for (int j = 0; j < g.d; ++j) {
                if (g.dims[j] < 1 || t.total * g.dims[j] > 0x7fffffffLL) return PIO_E_SHAPE;
                t.total *= g.dims[j];
                t.dims[j] = g.dims[j];
            }
            if (g.ldb < g.K) return PIO_E_SHAPE;
            t.d = g.d, t.K = g.K, t.c0 = g.concat_pos ? g.d : 0;
            width = t.c0 + F;
            if (width > Cq) return PIO_E_SHAPE;
            const size_t need = sizeof(float) * (size_t)(9 * QR_TS + dK + QR_TS * F);
            if (need > QR_MAX_LDS) return PIO_E_SHAPE;
            t.F = (int32_t)F;
            lds = need > lds ? need : lds;
        } else {
            if (g.C < 0 || g.C > Cq || (g.C > 0 && g.ldt < g.C)) return PIO_E_SHAPE;
            width = g.C;
        }
        t.width = (int32_t)width;
        if (width < Cq && !g.pad) return PIO_E_ARG;
        if (g.row0 < 0 || (int64_t)g.row0 + g.M > Qtot) return PIO_E_SHAPE;
        for (int k = 0; k < i; ++k)
            if ((int64_t)g.row0 < (int64_t)segs[k].row0 + segs[k].M && (int64_t)segs[k].row0 < (int64_t)g.row0 + g.M)
                return PIO_E_SHAPE;
        strips += (g.M + QR_TS - 1) / QR_TS;
        bytes += 4.0 * g.M * Cq + (g.kind == PIO_QUERY_TABLE ? 4.0 * g.M * g.C : g.points ? 8.0 * g.M : 0.0);
    }
    if (strips > 0x7fffffffLL) return PIO_E_SHAPE;
    if ((uintptr_t)y & 3) return PIO_E_ALIGN;
    for (int i = 0; i < nseg; ++i) {
        const pio_query_segment_t &g = segs[i];
        if (((uintptr_t)g.axis[0] | (uintptr_t)g.axis[1] | (uintptr_t)g.axis[2] | (uintptr_t)g.bands | (uintptr_t)g.table |
             (uintptr_t)g.pad) & 3)
            return PIO_E_ALIGN;
        if ((uintptr_t)g.points & 7) return PIO_E_ALIGN;
    }
    a.nseg = nseg;
    for (int i = nseg; i < PIO_MAX_QUERY_SEGMENTS; ++i) a.seg[i] = a.seg[0];
    ProfScope prof(PROF_LAYERNORM, 0.0, bytes, s);
    const dim3 grid((unsigned)strips);
    if (Cq % 4 == 0 && ldy % 4 == 0 && !((uintptr_t)y & 15))
        hipLaunchKernelGGL(build_queries_kernel<4>, grid, dim3(256), lds, s, a, y, ldy, Cq);
    else if (Cq % 2 == 0 && ldy % 2 == 0 && !((uintptr_t)y & 7))
        hipLaunchKernelGGL(build_queries_kernel<2>, grid, dim3(256), lds, s, a, y, ldy, Cq);
    else
        hipLaunchKernelGGL(build_queries_kernel<1>, grid, dim3(256), lds, s, a, y, ldy, Cq);
    return launch_status();
}

}  // namespace pio
