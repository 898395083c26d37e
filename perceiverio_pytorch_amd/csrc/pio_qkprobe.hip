// Logit probe: max |scale * q_i . k_j| of one attention call, read from the 16-bit Q / K the fused cores read.
// A calibration tool (pio_qk_logit_absmax / pio_logit_probe_begin, pio_capi.hip): never on the product path, no
// throughput target.
//
// qk_absmax_kernel: one wave owns a 32-row query tile and walks its workgroup's share of the key axis in 32-key tiles;
// per tile 2 x 2 MFMA 16x16x32 blocks accumulate over dk in 32-channel chunks, the operands going from global memory
// straight into the MFMA layout (lane l: row l & 15, channels 8 (l >> 4) .. + 7 of the chunk = one 16-byte piece).  Every
// piece is predicated on row < T and channel < dkp and zero-filled in registers otherwise: nothing behind Tq / Tk / dkp
// is ever read.  S is never written: each lane keeps the maximum of its accumulators over the attendable positions, the
// workgroup reduces it (shuffles, then LDS) and one lane merges it into the caller's word with one atomicMax on the bit
// pattern (non-negative floats order like unsigned integers; +inf is the largest of them).
#include "pio_internal.h"

namespace pio {

namespace {

constexpr int P_WAVES = 4;            // waves per workgroup
constexpr int P_QROWS = 32;           // query rows per wave
constexpr int P_KTILE = 32;           // keys per step
constexpr int64_t P_TARGET_WG = 2048; // workgroups a launch aims for (8 per CU): the key axis is cut to get there

template <int DT>
__global__ __launch_bounds__(64 * P_WAVES) void qk_absmax_kernel(
    const typename Op<DT>::T *__restrict__ Q, const typename Op<DT>::T *__restrict__ K, int dkp, float scale, int H, int Tq,
    int Tk, int64_t ldq, int64_t ldk, int64_t sQb, int64_t sKb, int keys_per_wg, const uint8_t *__restrict__ kv_mask,
    const uint8_t *__restrict__ q_mask, const uint8_t *__restrict__ full_mask, unsigned int *__restrict__ out) {
    typedef typename Op<DT>::T T;
    typedef typename Op<DT>::V8 V8;
    __shared__ float wave_max[P_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z / H, h = blockIdx.z % H;
    const int q0 = ((int)blockIdx.x * P_WAVES + wave) * P_QROWS;
    const int key_lo = (int)blockIdx.y * keys_per_wg;
    const int key_hi = key_lo + keys_per_wg < Tk ? key_lo + keys_per_wg : Tk;
    const int r16 = lane & 15, cgrp = lane >> 4;
    const T *Qb = Q + (int64_t)b * sQb + (int64_t)h * dkp;
    const T *Kb = K + (int64_t)b * sKb + (int64_t)h * dkp;
    const uint8_t *qm = q_mask ? q_mask + (int64_t)b * Tq : nullptr;
    const uint8_t *km = kv_mask ? kv_mask + (int64_t)b * Tk : nullptr;
    const uint8_t *fm = full_mask ? full_mask + (int64_t)b * Tq * Tk : nullptr;
    const V8 zero = {};
    float m = 0.f;
    if (q0 < Tq) {
        for (int k0 = key_lo; k0 < key_hi; k0 += P_KTILE) {
            f32x4 acc[2][2] = {};
            for (int c0 = 0; c0 < dkp; c0 += 32) {
                const int ch = c0 + 8 * cgrp;
                const bool ch_ok = ch < dkp;
                V8 qa[2], kb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int qr = q0 + 16 * i + r16, kr = k0 + 16 * i + r16;
                    qa[i] = (ch_ok && qr < Tq) ? *(const V8 *)(Qb + (int64_t)qr * ldq + ch) : zero;
                    kb[i] = (ch_ok && kr < Tk) ? *(const V8 *)(Kb + (int64_t)kr * ldk + ch) : zero;
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = Op<DT>::mfma16(qa[i], kb[j], acc[i][j]);
            }
            // accumulator layout: key (column) = lane & 15, query row = 4 (lane >> 4) + register
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int key = k0 + 16 * j + r16;
                if (key >= key_hi || (km && !km[key])) continue;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = q0 + 16 * i + 4 * cgrp + r;
                        if (row >= Tq || (qm && !qm[row]) || (fm && !fm[(int64_t)row * Tk + key])) continue;
                        float v = fabsf(acc[i][j][r] * scale);
                        if (!(v <= 3.4028234664e38f)) v = __builtin_inff();  // NaN or inf: reported, not dropped
                        m = v > m ? v : m;
                    }
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float o = __shfl_xor(m, off, 64);
        m = o > m ? o : m;
    }
    if (lane == 0) wave_max[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < P_WAVES; ++w) m = wave_max[w] > m ? wave_max[w] : m;
        if (m > 0.f) atomicMax(out, __float_as_uint(m));
    }
}

struct ProbeState {
    bool on = false;
    float *records = nullptr;
    int max_records = 0, n = 0;
} g_probe;

}  // namespace

int qk_absmax_launch(int dtype, int dkp, int dk, const void *Q, const void *K, int B, int H, int Tq, int Tk, int64_t ldq,
                     int64_t ldk, int64_t sQb, int64_t sKb, const uint8_t *kv_mask, const uint8_t *q_mask,
                     const uint8_t *full_mask, float *absmax, hipStream_t s) {
    if (dtype != PIO_DT_F16 && dtype != PIO_DT_BF16) return PIO_E_ARG;
    if (!Q || !K || !absmax) return PIO_E_ARG;
    if (dkp <= 0 || (dkp % 8) || dk <= 0 || dk > dkp || B <= 0 || H <= 0 || Tq < 0 || Tk < 0) return PIO_E_SHAPE;
    if ((ldq % 8) || (ldk % 8) || (sQb % 8) || (sKb % 8) || (((uintptr_t)Q | (uintptr_t)K) & 15) || ((uintptr_t)absmax & 3))
        return PIO_E_ALIGN;
    if (ldq < (int64_t)H * dkp || ldk < (int64_t)H * dkp) return PIO_E_SHAPE;
    if (Tq == 0 || Tk == 0) return PIO_OK;  // nothing attendable: the word keeps its value
    const int64_t nqt = ((int64_t)Tq + P_WAVES * P_QROWS - 1) / (P_WAVES * P_QROWS), bh = (int64_t)B * H;
    const int64_t nkt = ((int64_t)Tk + P_KTILE - 1) / P_KTILE;
    int64_t nkc = (P_TARGET_WG + nqt * bh - 1) / (nqt * bh);
    nkc = nkc < 1 ? 1 : nkc > nkt ? nkt : nkc;
    const int64_t tiles_per_wg = (nkt + nkc - 1) / nkc;
    nkc = (nkt + tiles_per_wg - 1) / tiles_per_wg;
    if (bh > 65535 || nkc > 65535 || nqt > 0x7fffffff) return PIO_E_SHAPE;
    const dim3 grid((unsigned)nqt, (unsigned)nkc, (unsigned)bh), block(64 * P_WAVES);
    const float scale = 1.0f / sqrtf((float)dk);
    const int keys_per_wg = (int)(tiles_per_wg * P_KTILE);
    if (dtype == PIO_DT_F16)
        qk_absmax_kernel<PIO_DT_F16><<<grid, block, 0, s>>>((const _Float16 *)Q, (const _Float16 *)K, dkp, scale, H, Tq, Tk, ldq,
                                                            ldk, sQb, sKb, keys_per_wg, kv_mask, q_mask, full_mask,
                                                            (unsigned int *)absmax);
    else
        qk_absmax_kernel<PIO_DT_BF16><<<grid, block, 0, s>>>((const __bf16 *)Q, (const __bf16 *)K, dkp, scale, H, Tq, Tk, ldq,
                                                             ldk, sQb, sKb, keys_per_wg, kv_mask, q_mask, full_mask,
                                                             (unsigned int *)absmax);
    return launch_status();
}

bool logit_probe_active() { return g_probe.on; }

int logit_probe_record(int dtype, int dkp, int dk, const AttnOperands &t, int B, int H, int Tq, int Tk,
                       const uint8_t *kv_mask, const uint8_t *q_mask, const uint8_t *full_mask, hipStream_t s) {
    const int idx = g_probe.n++;
    if (idx >= g_probe.max_records) return PIO_OK;  // counted, not recorded
    return qk_absmax_launch(dtype, dkp, dk, t.Q, t.K, B, H, Tq, Tk, t.ldq, t.ldk, t.sQb, t.sKb, kv_mask, q_mask, full_mask,
                            g_probe.records + idx, s);
}

int logit_probe_begin(float *records, int max_records) {
    if (!records || max_records <= 0 || ((uintptr_t)records & 3)) return PIO_E_ARG;
    g_probe.records = records;
    g_probe.max_records = max_records;
    g_probe.n = 0;
    g_probe.on = true;
    return PIO_OK;
}

int logit_probe_end() {
    const int n = g_probe.on ? g_probe.n : 0;
    g_probe = ProbeState();
    return n;
}

}  // namespace pio
