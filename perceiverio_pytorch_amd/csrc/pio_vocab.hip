// Vocabulary head + top-k behind the decoder in one pass (pio_vocab_topk): rows of the decoder output x [B, Q, K] fp32 against
// the (tied) embedding w [V, K] fp32, V <= 1024, then per row the log-sum-exp of its V logits and the k <= 8 best tokens:
//
//   logit[r, j] = bias[j] + sum_k w[j, k] x[r, k]                      r = b Q + q in [0, B Q), j in [0, V)
//   lse[r]      = m + log(sum_j exp(logit[r, j] - m)),  m = max_j logit[r, j]
//   ids[r, t]   = the t-th token of row r in the order (logit descending, id ascending among equal logits; -0.0 == +0.0)
//   logprob[r, t] = logit[r, ids[r, t]] - lse[r]
//
// The chain this stands for (EmbeddingPostprocessor through runtime.hip_linear, then log_softmax and topk in torch) rounds x
// to 16 bits (twice under a split policy) for a GEMM and writes all V logits of every row; here x is multiplied as fp32 and
// only ids, logprob and lse leave the chip (the logits too when asked for).
// A second mode (x == w == NULL) takes the logits as given and runs the selection alone: for row counts where the GEMM is
// the better multiplier.
//
// One workgroup (eight waves) owns a strip of VT_TS = 8 consecutive rows.  Every lane keeps its share of the strip's x rows in
// registers; a WAVE owns the vocabulary rows j = wave, wave + 8, ...: it streams w[j] (L2-resident: 805 KB at 262 x 768) with
// 16-byte loads, one row ahead, and multiplies it against the eight x rows.  The strip's logits stay in LDS ([8, V] fp32);
// wave q then reduces row q from there.
//
// SUMMATION ORDER (part of the definition: the bits of a row's results depend on that row of x, w, bias, V, K and k only).
// Lane l of the wave owns the floats k = 4 (l + 64 i) + e, e = 0 .. 3, i = 0 .. ceil(K / 256) - 1, with k < K:
//   p_l   = +0;  for i ascending, for e ascending:  p_l = fmaf(w[j, k], x[k], p_l)      (lanes with no k < K keep +0)
//   s     = xor-shuffle tree over the 64 lanes, offsets 32, 16, 8, 4, 2, 1:  p_l = fadd_rn(p_l, p_(l xor offset))
//   logit = bias ? fadd_rn(s, bias[j]) : s
// (the order of pio_heads.hip).  Selection, per row, lane l owning the ids j = l + 64 t, t ascending:
//   m     = max over the lane's ids (fmaxf, from -inf), then the xor-shuffle tree with fmaxf
//   e_l   = +0;  for t ascending:  e_l = fadd_rn(e_l, expf(fsub_rn(logit_j, m)));  S = the xor-shuffle tree with fadd_rn
//   lse   = fadd_rn(m, logf(S));   logprob = fadd_rn(logit, -lse)
//   top-k = k rounds of a wave argmax under the order above; round t + 1 considers the ids strictly behind round t's winner.
// Comparisons with a NaN are false: a NaN logit is never chosen; a row that runs out of candidates repeats id 0 with a NaN
// logprob.  Every id written is in [0, V).
//   * All offsets are 64-bit.  Arguments travel by value.  Only vector stores.  No atomics.  Rows past the end of the last strip
//     recompute the last row and store nothing.
#include "pio_device.h"

#include <math.h>

namespace pio {

namespace {

constexpr int VT_TS = 8;         // rows per strip = waves per workgroup
constexpr int VT_THREADS = 512;
constexpr int VT_SWEEPS = 4;     // K <= 1024: at most four 16-byte pieces of a row per lane

struct VocabArgs {
    const float *x, *w, *bias, *lg_in;
    int32_t *ids;
    float *logprob, *lse, *lg_out;
    int64_t x_sb, ldx, ldw, ld_in, ld_out, R;
    int32_t Q, V, K, k;
};

__device__ __forceinline__ bool vt_before(float v, int j, float pv, int pj) {
    // (v, j) strictly in front of (pv, pj): greater logit, or an equal one (-0.0 == +0.0) with the lower id; pj < 0: nothing
    return j >= 0 && (pj < 0 || v > pv || (v == pv && j < pj));
}

__device__ __forceinline__ void vt_load_w(f32x4 (&wv)[VT_SWEEPS], const float *__restrict__ wr, int K, int lane) {
#pragma unroll
    for (int i = 0; i < VT_SWEEPS; ++i) {
        const int kk = 4 * (lane + 64 * i);
        if (kk < K) wv[i] = *reinterpret_cast<const f32x4 *>(wr + kk);
    }
}

__global__ __launch_bounds__(VT_THREADS) void vocab_topk_kernel(const VocabArgs a) {
    extern __shared__ __align__(16) float vt_lg[];  // [VT_TS, V]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int V = a.V, K = a.K;
    const int64_t r0 = (int64_t)blockIdx.x * VT_TS;
    const int n = (int)min((int64_t)VT_TS, a.R - r0);

    if (a.x) {
        // this lane's share of the strip's rows, in registers (rows past the end: the last row again)
        f32x4 xv[VT_TS][VT_SWEEPS];
#pragma unroll
        for (int q = 0; q < VT_TS; ++q) {
            const int64_t r = r0 + min(q, n - 1);
            const int64_t b = r / a.Q;
            const float *xr = a.x + b * a.x_sb + (r - b * a.Q) * a.ldx;
#pragma unroll
            for (int i = 0; i < VT_SWEEPS; ++i) {
                const int kk = 4 * (lane + 64 * i);
                xv[q][i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (kk < K) xv[q][i] = *reinterpret_cast<const f32x4 *>(xr + kk);
            }
        }
        f32x4 wc[VT_SWEEPS], wn[VT_SWEEPS];
#pragma unroll
        for (int i = 0; i < VT_SWEEPS; ++i) wc[i] = wn[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (wave < V) vt_load_w(wc, a.w + (int64_t)wave * a.ldw, K, lane);
        for (int j = wave; j < V; j += VT_TS) {
            if (j + VT_TS < V) vt_load_w(wn, a.w + (int64_t)(j + VT_TS) * a.ldw, K, lane);
            float mine = 0.0f;
#pragma unroll
            for (int q = 0; q < VT_TS; ++q) {
                float p = 0.0f;
#pragma unroll
                for (int i = 0; i < VT_SWEEPS; ++i) {
                    if (4 * (lane + 64 * i) < K) {
                        p = __fmaf_rn(wc[i].x, xv[q][i].x, p);
                        p = __fmaf_rn(wc[i].y, xv[q][i].y, p);
                        p = __fmaf_rn(wc[i].z, xv[q][i].z, p);
                        p = __fmaf_rn(wc[i].w, xv[q][i].w, p);
                    }
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) p = __fadd_rn(p, __shfl_xor(p, off, 64));
                if (lane == q) mine = p;
            }
            if (lane < VT_TS) {
                if (a.bias) mine = __fadd_rn(mine, a.bias[j]);
                vt_lg[lane * V + j] = mine;
            }
#pragma unroll
            for (int i = 0; i < VT_SWEEPS; ++i) wc[i] = wn[i];
        }
    } else {
        // selection alone: the strip's logits as given
        for (int v = threadIdx.x; v < n * V; v += VT_THREADS) {
            const int q = v / V, j = v - q * V;
            vt_lg[v] = a.lg_in[(r0 + q) * a.ld_in + j];
        }
    }
    __syncthreads();

    if (a.lg_out)
        for (int v = threadIdx.x; v < n * V; v += VT_THREADS) {
            const int q = v / V, j = v - q * V;
            a.lg_out[(r0 + q) * a.ld_out + j] = vt_lg[v];
        }

    if (wave >= n) return;  // (wave q reduces row q; no barrier follows)
    const float *lg = vt_lg + wave * V;
    const int64_t r = r0 + wave;

    float m = -INFINITY;
    for (int j = lane; j < V; j += 64) m = fmaxf(m, lg[j]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    float e = 0.0f;
    for (int j = lane; j < V; j += 64) e = __fadd_rn(e, expf(__fsub_rn(lg[j], m)));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) e = __fadd_rn(e, __shfl_xor(e, off, 64));
    const float lse = __fadd_rn(m, logf(e));
    if (a.lse && lane == 0) a.lse[r] = lse;

    if (!a.ids && !a.logprob) return;
    float pv = 0.0f, myv = 0.0f;
    int pj = -1, myj = 0;  // the previous round's winner (pj < 0: none yet); lane t keeps round t's
    for (int t = 0; t < a.k; ++t) {
        float bv = 0.0f;
        int bj = -1;
        for (int j = lane; j < V; j += 64) {
            const float v = lg[j];
            // behind the previous winner, in front of this lane's best so far (ids ascend: an equal logit does not replace)
            if ((pj < 0 ? v == v : vt_before(pv, pj, v, j)) && (bj < 0 || v > bv)) {
                bv = v;
                bj = j;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oj = __shfl_xor(bj, off, 64);
            if (vt_before(ov, oj, bv, bj)) {
                bv = ov;
                bj = oj;
            }
        }
        float outv = __fadd_rn(bv, -lse);
        int outj = bj;
        if (bj < 0) {  // no candidate left (NaN logits): id 0, a NaN logprob; the next rounds find nothing either
            outv = __builtin_nanf("");
            outj = 0;
        } else {
            pv = bv;
            pj = bj;
        }
        if (lane == t) {
            myv = outv;
            myj = outj;
        }
    }
    if (lane < a.k) {
        if (a.ids) a.ids[r * a.k + lane] = myj;
        if (a.logprob) a.logprob[r * a.k + lane] = myv;
    }
}

}  // namespace

int vocab_topk_launch(const float *x, int64_t x_sb, int64_t ldx, const float *w, int64_t ldw, const float *bias, int B, int Q,
                      int V, int K, int k, int32_t *ids, float *logprob, float *lse, float *logits, int64_t ldl,
                      hipStream_t s) {
    const bool compute = x != nullptr;
    if ((x == nullptr) != (w == nullptr)) return PIO_E_ARG;
    if (!compute && (!logits || bias)) return PIO_E_ARG;                // (selection alone: the logits are the input)
    if (!ids && !logprob && !lse && !(compute && logits)) return PIO_E_ARG;  // (nothing to write)
    if (B < 1 || Q < 1 || V < 1 || V > 1024 || k < 1 || k > 8 || k > V) return PIO_E_SHAPE;
    if ((int64_t)B * Q > 0x7fffffffLL || (logits && ldl < V)) return PIO_E_SHAPE;
    if (compute && (K < 4 || K > 1024 || (K & 3) || ldx < K || ldw < K)) return PIO_E_SHAPE;
    if (compute && ((((uintptr_t)x | (uintptr_t)w) & 15) || (ldx & 3) || (ldw & 3) || (B > 1 && (x_sb & 3)))) return PIO_E_ALIGN;
    if (((uintptr_t)bias | (uintptr_t)ids | (uintptr_t)logprob | (uintptr_t)lse | (uintptr_t)logits) & 3) return PIO_E_ALIGN;
    VocabArgs a;
    a.x = x, a.w = w, a.bias = bias, a.lg_in = compute ? nullptr : logits;
    a.ids = ids, a.logprob = logprob, a.lse = lse, a.lg_out = compute ? logits : nullptr;
    a.x_sb = B > 1 ? x_sb : 0, a.ldx = ldx, a.ldw = ldw, a.ld_in = ldl, a.ld_out = ldl, a.R = (int64_t)B * Q;
    a.Q = Q, a.V = V, a.K = compute ? K : 0, a.k = k;
    const int64_t strips = (a.R + VT_TS - 1) / VT_TS;
    const double bytes = compute ? (double)strips * V * K * 4.0 + (double)a.R * K * 4.0 : (double)a.R * V * 4.0;
    ProfScope prof(PROF_SOFTMAX, compute ? 2.0 * a.R * V * K : 0.0, bytes, s);
    hipLaunchKernelGGL(vocab_topk_kernel, dim3((unsigned)strips), dim3(VT_THREADS), sizeof(float) * VT_TS * V, s, a);
    return launch_status();
}

}  // namespace pio
