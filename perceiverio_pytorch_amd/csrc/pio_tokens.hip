// Front end of the multimodal model in one pass (pio_assemble_tokens): every modality's features, its batch-invariant
// position table and its learned padding embedding side by side in the channel axis, a mask token in place of a masked
// modality, the modalities one after the other along the token axis (perceiver.py:451-499 MultimodalPreprocessor; the
// image features are processor_utils.py:21-38 space_to_depth with temporal block 1).  Per segment, row m, sample b:
//
//   x[c] = feature(b, m, c)            c in [0, C1)
//        = table[m, c - C1]            c in [C1, C1 + C2)
//        = pad[c - C1 - C2]            c in [C1 + C2, Cc)
//   y[b, row0 + m, c] = x[c]                          token == NULL
//                     = token[c] + 0.0f * x[c]        otherwise (two rounded fp32 operations: inf / NaN in x give NaN)
//
//   ROWS: feature(b, m, j) = f[b sb + m sm + j]
//   S2D:  m = (t H/s + y) W/s + x,  j = (dy s + dx) C + c:  feature(b, m, j) = f[b sb + t st + c sc + (y s + dy) sy + x s + dx]
//
// Everything is a move (the masked form is exact), so the result equals the chain of torch.cat calls it replaces bit
// for bit.  The chain writes each sample's array about 2.4 times over and keeps three temporaries of its size alive;
// this kernel stores every output element once.
//
// One workgroup (four waves) owns a strip of TK_TS consecutive tokens of one sample and segment; the grid is the flat
// list of strips, sample slowest, so later samples find the tables in cache.
//   * S2D: the strip's pixels -- C s image-row pieces per token -- go to LDS first, read along x (lanes walk the s
//     contiguous pixels of a token and on into the next token's: coalesced runs of a whole strip while it stays in one
//     token row); each token's frame offset is computed once per strip and the (dy, dx, c) -> LDS offset of the C1 output
//     channels once per workgroup, so the gather itself has no division.  Only pixels of tokens inside the strip are
//     addressed.
//   * wave = output row, lanes = that row's 16-byte vectors (Cc % 4 == 0: ldy % 4 == 0 and y 16-byte aligned) or its
//     dwords.  The three source ranges begin at arbitrary channels (48 | 195 | 461), so a lane composes its vector
//     element by element; a wave instruction stores 1 KiB of one output row.
//   * All offsets are 64-bit.  The segment table travels by value in the kernel arguments.
#include "pio_internal.h"

namespace pio {

namespace {

constexpr int TK_TS = 32;          // tokens per strip
constexpr int TK_MAXC1 = 8 * 8 * 4;  // S2D: s <= 8, C <= 4

struct TokSeg {
    const float *f, *table, *pad, *token;
    int64_t sb, sm, st, sc, sy, ldt;
    int32_t kind, row0, M, C1, C2, C, Hs, Ws, s, strip0;  // Hs = H / s, Ws = W / s; strip0: first strip of the segment
};
struct TokArgs {
    TokSeg seg[PIO_MAX_TOKEN_SEGMENTS];
    int32_t nseg, strips;  // strips per sample
};

#ifdef PIO_TOKENS_NT  // A/B builds only (profiles/multimodal_front_end.json): non-temporal stores of the output
template <typename T>
__device__ __forceinline__ void tok_store(T *p, T v) { __builtin_nontemporal_store(v, p); }
#else
template <typename T>
__device__ __forceinline__ void tok_store(T *p, T v) { *p = v; }
#endif

// V = 4: rows leave as 16-byte vectors; V = 1: as dwords
template <int V>
__global__ __launch_bounds__(256) void assemble_tokens_kernel(const TokArgs a, float *__restrict__ y, int64_t ldy,
                                                              int64_t sYb, int Cc) {
    extern __shared__ __align__(16) float tk_lds[];
    // [TK_TS token offsets (int64)] [TK_MAXC1 channel offsets (int)] [pixels: C s rows of pitch TK_TS s + 1]
    int64_t *tokoff = reinterpret_cast<int64_t *>(tk_lds);
    int *chanoff = reinterpret_cast<int *>(tk_lds + 2 * TK_TS);
    float *pix = tk_lds + 2 * TK_TS + TK_MAXC1;

    const int b = blockIdx.x / a.strips, strip = blockIdx.x - b * a.strips;
    int si = 0;
#pragma unroll
    for (int i = 1; i < PIO_MAX_TOKEN_SEGMENTS; ++i)
        if (i < a.nseg && strip >= a.seg[i].strip0) si = i;
    const TokSeg &g = a.seg[si];
    const int m0 = (strip - g.strip0) * TK_TS;
    const int n = min(TK_TS, g.M - m0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C1 = g.C1, C12 = g.C1 + g.C2;
    const int pitch = TK_TS * g.s + 1;

    if (g.kind == PIO_TOKENS_S2D) {
        const int s = g.s, C = g.C;
        if ((int)threadIdx.x < n) {
            const int m = m0 + threadIdx.x, x = m % g.Ws, q = m / g.Ws, yy = q % g.Hs, t = q / g.Hs;
            tokoff[threadIdx.x] = (int64_t)t * g.st + (int64_t)yy * s * g.sy + (int64_t)x * s;
        }
        for (int j = threadIdx.x; j < C1; j += 256) {
            const int c = j % C, q = j / C, dx = q % s, dy = q / s;
            chanoff[j] = (c * s + dy) * pitch + dx;
        }
        __syncthreads();
        const float *fb = g.f + (int64_t)b * g.sb;
        for (int ch = wave; ch < C * s; ch += 4) {
            const int c = ch / s, dy = ch - c * s;
            const float *fr = fb + (int64_t)c * g.sc + (int64_t)dy * g.sy;
            for (int e = lane; e < n * s; e += 64) {
                const int tok = e / s, dx = e - tok * s;
                pix[ch * pitch + e] = fr[tokoff[tok] + dx];
            }
        }
        __syncthreads();
    }

    for (int r = wave; r < n; r += 4) {
        const int64_t m = m0 + r;
        const float *frow = g.f + (int64_t)b * g.sb + m * g.sm;  // (ROWS only)
        const float *trow = g.table + m * g.ldt - C1;            // (indexed with c >= C1 only)
        const float *prow = g.pad - C12;
        const float *xrow = pix + r * g.s;
        float *yrow = y + (int64_t)b * sYb + (g.row0 + m) * ldy;
        for (int cv = lane; cv * V < Cc; cv += 64) {
            float v[V];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int c = cv * V + e;
                float x;
                if (c < C1)
                    x = g.kind == PIO_TOKENS_S2D ? xrow[chanoff[c]] : frow[c];
                else if (c < C12)
                    x = trow[c];
                else
                    x = prow[c];
                if (g.token) x = __fadd_rn(g.token[c], __fmul_rn(0.0f, x));
                v[e] = x;
            }
            if constexpr (V == 4) {
                f32x4 o = {v[0], v[1], v[2], v[3]};
                tok_store(reinterpret_cast<f32x4 *>(yrow) + cv, o);
            } else {
                tok_store(yrow + cv, v[0]);
            }
        }
    }
}

}  // namespace

int assemble_tokens_launch(const pio_token_segment_t *segs, int nseg, float *y, int64_t ldy, int64_t sYb, int B, int Mtot,
                           int Cc, hipStream_t s) {
    if (!y || !segs || nseg < 1 || nseg > PIO_MAX_TOKEN_SEGMENTS) return PIO_E_ARG;
    for (int i = 0; i < nseg; ++i) {
        const pio_token_segment_t &g = segs[i];
        if (g.kind != PIO_TOKENS_ROWS && g.kind != PIO_TOKENS_S2D) return PIO_E_ARG;
        if ((g.C1 > 0 && !g.feature) || (g.C2 > 0 && !g.table)) return PIO_E_ARG;
        if (g.C1 >= 0 && g.C2 >= 0 && (int64_t)g.C1 + g.C2 < Cc && !g.pad) return PIO_E_ARG;
    }
    if (B <= 0 || Mtot <= 0 || Cc <= 0 || ldy < Cc) return PIO_E_SHAPE;
    if (B > 1 && sYb < (int64_t)(Mtot - 1) * ldy + Cc) return PIO_E_SHAPE;
    TokArgs a;
    int64_t strips = 0;
    size_t lds = 0;
    double bytes = 0.0;
    for (int i = 0; i < nseg; ++i) {
        const pio_token_segment_t &g = segs[i];
        if (g.M <= 0 || g.C1 < 0 || g.C2 < 0 || (int64_t)g.C1 + g.C2 > Cc) return PIO_E_SHAPE;
        if (g.row0 < 0 || (int64_t)g.row0 + g.M > Mtot) return PIO_E_SHAPE;
        for (int k = 0; k < i; ++k)
            if ((int64_t)g.row0 < (int64_t)segs[k].row0 + segs[k].M && (int64_t)segs[k].row0 < (int64_t)g.row0 + g.M)
                return PIO_E_SHAPE;
        TokSeg &t = a.seg[i];
        t = TokSeg{g.feature, g.table, g.pad, g.token, g.sb, g.sm, g.st, g.sc, g.sy, g.ldt, g.kind, g.row0, g.M, g.C1, g.C2,
                   1, 1, 1, 1, (int32_t)strips};
        if (g.kind == PIO_TOKENS_S2D) {
            if (g.s < 1 || g.s > 8 || g.C < 1 || g.C > 4 || g.T < 1 || g.H < 1 || g.W < 1 || g.H % g.s || g.W % g.s)
                return PIO_E_SHAPE;
            if (g.C1 != g.s * g.s * g.C || (int64_t)g.T * (g.H / g.s) * (g.W / g.s) != g.M) return PIO_E_SHAPE;
            t.C = g.C, t.Hs = g.H / g.s, t.Ws = g.W / g.s, t.s = g.s;
            const size_t need = sizeof(float) * (2 * TK_TS + TK_MAXC1 + (size_t)g.C * g.s * (TK_TS * g.s + 1));
            lds = need > lds ? need : lds;
        }
        strips += (g.M + TK_TS - 1) / TK_TS;
        bytes += 4.0 * B * g.M * ((double)Cc + g.C1) + 4.0 * g.M * g.C2;
    }
    if (strips * B > 0x7fffffffLL) return PIO_E_SHAPE;
    const bool vec = Cc % 4 == 0;
    if ((uintptr_t)y & 3) return PIO_E_ALIGN;
    for (int i = 0; i < nseg; ++i)
        if (((uintptr_t)segs[i].feature | (uintptr_t)segs[i].table | (uintptr_t)segs[i].pad | (uintptr_t)segs[i].token) & 3)
            return PIO_E_ALIGN;
    if (vec && (((uintptr_t)y & 15) || ldy % 4 != 0 || (B > 1 && sYb % 4 != 0))) return PIO_E_ALIGN;
    a.nseg = nseg;
    a.strips = (int32_t)strips;
    for (int i = nseg; i < PIO_MAX_TOKEN_SEGMENTS; ++i) a.seg[i] = a.seg[0];
    ProfScope prof(PROF_LAYERNORM, 0.0, bytes, s);
    const dim3 grid((unsigned)(strips * B));
    if (vec)
        hipLaunchKernelGGL(assemble_tokens_kernel<4>, grid, dim3(256), lds, s, a, y, ldy, sYb, Cc);
    else
        hipLaunchKernelGGL(assemble_tokens_kernel<1>, grid, dim3(256), lds, s, a, y, ldy, sYb, Cc);
    return launch_status();
}

}  // namespace pio
