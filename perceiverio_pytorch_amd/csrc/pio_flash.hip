// Fused multi-head attention core for gfx950: O = softmax(Q K^T / sqrt(dk)) V without materialising the
// score matrix.  Replaces transformer_primitives.py:138-166 (scores, scale, softmax, P.v, head merge) for the
// un-masked case with per-head widths 32/64/128 (qk) and 32..160 (v) -- the latent self-attention stack.
//
// Structure (one workgroup = 4 waves = 128 query rows of one (batch, head); one wave = 32 query rows):
//   * "swapped" products so that the softmax axis never crosses lanes:
//       S^T[k][q] = K[k][:] . Q[q][:]      mfma_32x32x16(A = K fragment, B = Q fragment)  -> column q on the lane
//       O^T[d][q] = V^T[d][:] . P^T[:][q]  mfma_32x32x16(A = V^T fragment, B = P^T)       -> P^T is the S^T
//     accumulator itself, converted to 16 bit in place (registers 8s..8s+7 are the B fragment of k-step s):
//     no LDS round trip, no shuffles for P.  Lanes l and l+32 hold the two halves of a column; only the
//     running max crosses them (one ds_bpermute per 64-key tile), the row sums are combined once at the end.
//   * Q fragments stay in registers for the whole kernel; K [64 keys][dk] and V^T [dv][64 keys] tiles are
//     staged HBM -> LDS by LDS-DMA (global_load_lds_dwordx4), double buffered, one barrier per tile, with the
//     XOR swizzle applied on the source address and on the ds_read side (conflict-free K reads, 2-way V^T reads).
//   * V is consumed K-contiguous (V^T [dv][keys]), which is exactly what the V projection GEMM writes.
//   * online softmax in base 2 (scale folded into the exponent constant), fp32 statistics and accumulators.
//   * QK_PAIR (DK = 32 and DK = DV = 128, fp16): Q and K arrive as (hi, lo) pairs and S^T = K_lo Q_hi^T + K_hi Q_lo^T + K_hi Q_hi^T,
//     accumulated in fp32 IN THAT ORDER (the two small products first, the large one last); lo x lo is dropped.  Q_lo is
//     a second set of register fragments, K_lo a second K tile in every ring stage (same pieces, same swizzle, same
//     conflict-free reads, same single barrier per tile).  Everything behind S^T is unchanged; the output may leave as a
//     pair (O_lo: the rounding residual), which the split-operand out projection behind the core consumes.
//     The same for the 128-wide stack heads (DK = DV = 128, fp16, no key split): there the K fragments are streamed per
//     k-step for the two small products and K_hi is read from LDS a second time for the large one.  Everything else --
//     64-wide heads, bf16, a key-split pair variant -- has no pair instantiation: PIO_E_SHAPE from the launcher.
// Shared with the other fused cores: the block-id remap (pio_device.h), the half-wave maximum, the Q-fragment loader
// and the 4-wide pair cast (pio_attn_device.h); the launch plan (pio_attn_route.h).  The row-sum combine and the staged
// whole-row epilogue keep their own spelling: through a helper they reorder instructions of this kernel.
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>

#include "pio_attn_device.h"

namespace pio {

#ifndef PIO_FLASH_DEFAULT_VARIANT
#define PIO_FLASH_DEFAULT_VARIANT 0
#endif

struct FlashParams {
    const void *Q, *K, *VT;
    void *O;
    int Tq, Tk, H, nqt;
    int64_t ldq, ldk, ldvt, ldo;
    int64_t sQb, sKb, sVb, sOb;  // batch strides (elements); 0 for a batch-invariant Q
    float scale_log2;            // log2(e) / sqrt(dk)
    int o_rows16;                // O rows are 16-byte aligned: the epilogue may store whole 16-byte chunks
    const void *Q_lo, *K_lo;     // QK_PAIR instantiations only: the rounding residuals of Q / K (same strides)
    void *O_lo;                  // QK_PAIR instantiations only (optional): o - float(O); the launcher clears o_rows16 with it
};


// VROW = true: V is consumed ROW-major ([keys][H*dv], the layout a plain projection GEMM writes, so Q | K | V come out
// of ONE fused GEMM) through transposed LDS reads; VROW = false: V^T [dv][keys] as before.
// Row-major tile in LDS: key row r at byte r * DV * 2, its 16-byte chunk c at position c ^ vrow_swz<DV>(r).  One
// ds_read_b64_tr_b16 touches, per half wave, 4 consecutive keys x 4 consecutive chunks (4d .. 4d+3): conflict-free when
// those 16 units fall into 16 different 16-byte bank slots, slot = (r * DV / 8 + position) mod 16 --
//   DV = 128 (16 chunks per row): slot = position: f(r) = ((r & 3) << 2) | ((r >> 2) & 3) (also conflict-free row reads)
//   DV = 64  ( 8 chunks per row): slot = 8 (r & 1) + position: f(r) = ((r >> 1) & 1) << 2
//   DV = 32, 160 (4, 20 chunks):  slot = 4 (r & 3) + position mod 16: no swizzle needed
// NW = waves per workgroup: 4 (128 query rows, two workgroups per CU) or 8 (256 query rows, one workgroup per CU:
// every staged K / V tile then serves twice the queries, i.e. half the L2 -> LDS traffic per flop).
template <int DV>
__device__ __forceinline__ int vrow_swz(int r) {
    if constexpr (DV == 128) return ((r & 3) << 2) | ((r >> 2) & 3);
    else if constexpr (DV == 64) return ((r >> 1) & 1) << 2;
    else return 0;
}

// KS = 2 (NW = 8; launcher: Tk % 128 == 0 and at most one 128-row workgroup per CU): the KEY axis is split over two wave
// groups of the workgroup -- wave w owns query block w % 4 and key half w / 4 -- which run their halves side by side
// (two waves per SIMD: one wave's dependent MFMA -> exp2 -> MFMA chain covers the other's) and merge (m, l, O) through
// LDS at the end.  For the shapes that offer only one 4-wave workgroup per CU: the flow stack (16 heads x 2048 latents:
// 256 workgroups of ~1 900 cycles per 64-key tile against 256 cycles of MFMAs), small ImageNet batches.
// QK_PAIR on the 128-wide head (DK = DV = 128, KS = 1): a ring stage is K + K_lo + V = 48 KB, two stages 96 KB -- one
// workgroup per CU whatever NW is -- and Q_hi, Q_lo, O and S already take 224 registers of a wave, so the K fragments
// are not all held at once as for DK = 32: see the S^T block.
template <int DT, int DK, int DV, bool VROW, int NW, int KS = 1, bool QK_PAIR = false>
__global__ __launch_bounds__(NW * 64, (NW >= 8 || (QK_PAIR && DK == 128)) ? 1 : 2) void flash_attn_kernel(const FlashParams p) {
    static_assert(!QK_PAIR || (DT == PIO_DT_F16 && (DK == 32 || (DK == 128 && DV == 128 && KS == 1))),
                  "pair-operand Q K^T: the DK = 32 and the (128, 128) un-split fp16 instantiations");
    typedef typename Op<DT>::T T;
    typedef typename Op<DT>::V8 V8;
    typedef typename Op<DT>::V4 V4;
    typedef short tr4 __attribute__((__vector_size__(4 * sizeof(short))));
    static_assert(!VROW || DV == 128 || DV == 64 || DV == 32 || DV == 160, "row-major V: swizzles exist for these widths");
    constexpr int KT = 64;                       // keys per tile
    constexpr int K_TILE = KT * DK * 2;          // bytes
    constexpr int K_STG = QK_PAIR ? 2 * K_TILE : K_TILE;   // K part of a ring stage: the K tile (+ the K_lo tile behind it)
    constexpr int V_TILE = DV * KT * 2;          // bytes
    constexpr int KCPR = DK / 8;                 // 16-byte chunks per K row (4, 8, 16)
    constexpr int KRPB = 16 / KCPR;              // K rows per 256-byte bank row
    constexpr int K_PIECES = K_TILE / 1024;      // 1-KiB LDS-DMA pieces per tile
    constexpr int V_PIECES = V_TILE / 1024;
    constexpr int NDT = DV / 32;                 // 32-row O^T tiles
    constexpr int NQS = DK / 16;                 // k-steps of the Q.K product
    constexpr int OROW = DV * 2 + 16;            // epilogue staging: bytes per output row (+16: rows spread over banks)
    static_assert(KS == 1 || ((KS == 2 || KS == 4) && NW == 4 * KS), "key split: KS groups of four waves");
    constexpr int NWQ = NW / KS;                 // waves along the query axis
    constexpr int MRG = KS > 1 ? (KS - 1) * NWQ * 64 * (NDT * 16 + 2) * 4 : 0;   // merge area: (O^T, m, l) of the other key parts
    constexpr int RING = 2 * KS * (K_STG + V_TILE), OSTG = NW * 32 * OROW;
    constexpr int SM0 = RING > OSTG ? RING : OSTG;
    static_assert((SM0 > MRG ? SM0 : MRG) <= 160 * 1024, "LDS budget of one CU");
    __shared__ __attribute__((aligned(16))) char smem[SM0 > MRG ? SM0 : MRG];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r32 = lane & 31, hh = lane >> 5;
    // 1-D grid, remapped so that the q-tiles of one (batch, head) -- which stream the same K / V^T -- are
    // consecutive on ONE XCD (ids are dealt round-robin over the 8 XCDs): their K/V re-reads hit that L2.
    const int bid = xcd_contiguous(blockIdx.x, gridDim.x);
    const int qt = bid % p.nqt, bh = bid / p.nqt;
    const int b = bh / p.H, h = bh % p.H;
    const int qb = KS == 1 ? wave : wave % NWQ, kh = KS == 1 ? 0 : wave / NWQ;   // query block, key half of this wave
    const int q0 = qt * (NWQ * 32) + qb * 32;

    const T *Qg = (const T *)p.Q + b * p.sQb + (int64_t)h * DK;
    const T *Kg = (const T *)p.K + b * p.sKb + (int64_t)h * DK;
    const T *Vg = (const T *)p.VT + b * p.sVb + (VROW ? (int64_t)h * DV : (int64_t)h * DV * p.ldvt);
    const T *zsrc = (const T *)g_zero16;
    const T *Klg = nullptr;
    if constexpr (QK_PAIR) Klg = (const T *)p.K_lo + b * p.sKb + (int64_t)h * DK;

    V8 qf[NQS];  // Q fragments (B operand), loaded behind the first tile's request: the two latencies overlap
    V8 ql[QK_PAIR ? NQS : 1];  // QK_PAIR: the Q_lo fragments, same layout

    const int ntiles_all = (p.Tk + KT - 1) / KT;
    const int ntiles = ntiles_all / KS;          // (KS == 2: an even tile count -- launcher) tiles of this key half
    const int tile0 = kh * ntiles;               // its first tile

    auto stage = [&](int kt, int buf) {          // tile kt of THIS key half, staged by the half's NWQ waves
        char *kb = smem + (buf * KS + kh) * (K_STG + V_TILE);
        char *vb = kb + K_STG;
        const int k0 = (tile0 + kt) * KT;
        // K tile: piece = 64 chunks = 64/KCPR rows
        for (int pc = qb; pc < K_PIECES; pc += NWQ) {
            const int row = pc * (64 / KCPR) + lane / KCPR;
            const int slot = lane % KCPR;
            const int c = slot ^ ((row / KRPB) & (KCPR - 1));
            int key = k0 + row;
            key = key < p.Tk ? key : p.Tk - 1;
            const T *src = Kg + (int64_t)key * p.ldk + c * 8;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                             (__attribute__((address_space(3))) void *)(kb + pc * 1024), 16, 0, 0);
            if constexpr (QK_PAIR)   // the K_lo tile: same rows, same chunk order, K_TILE bytes further
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void *)(Klg + (int64_t)key * p.ldk + c * 8),
                    (__attribute__((address_space(3))) void *)(kb + K_TILE + pc * 1024), 16, 0, 0);
        }
        if constexpr (VROW) {
            // row-major V tile [64 keys][DV]: DV / 8 chunks per row, a 1-KiB piece = 64 consecutive chunks
            constexpr int VCPR = DV / 8;
            for (int pc = qb; pc < V_PIECES; pc += NWQ) {
                const int idx = pc * 64 + lane;
                const int row = idx / VCPR;
                const int slot = idx - row * VCPR;
                const int c = slot ^ vrow_swz<DV>(row);
                int key = k0 + row;
                key = key < p.Tk ? key : p.Tk - 1;
                const T *src = Vg + (int64_t)key * p.ldvt + c * 8;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                                 (__attribute__((address_space(3))) void *)(vb + pc * 1024), 16, 0,
                                                 0);
            }
        } else
        // V^T tile: rows = dv (128-byte rows, 8 chunks), piece = 8 rows
        for (int pc = qb; pc < V_PIECES; pc += NWQ) {
            const int row = pc * 8 + (lane >> 3);
            const int slot = lane & 7;
            const int c = slot ^ ((row >> 1) & 7);
            const int kcol = k0 + c * 8;
            const T *src = (kcol < p.ldvt) ? Vg + (int64_t)row * p.ldvt + kcol : zsrc;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                             (__attribute__((address_space(3))) void *)(vb + pc * 1024), 16, 0, 0);
        }
    };

    f32x16 oacc[NDT];
#pragma unroll
    for (int i = 0; i < NDT; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) oacc[i][j] = 0.f;
    float m_run = -INFINITY;  // running max (already in base-2 scaled units), identical in lanes l and l+32
    float l_run = 0.f;        // this lane's partial row sum

    // per-lane read offsets
    int k_off[2];  // K fragment row byte offsets for the two 32-key halves (chunk part added per step)
#pragma unroll
    for (int t = 0; t < 2; ++t) k_off[t] = (32 * t + r32) * (DK * 2);
    const int k_swz = (r32 / KRPB) & (KCPR - 1);  // 32t is a multiple of 16*KRPB?  (32t + r32)/KRPB & mask:
    // (32/KRPB) is a multiple of KCPR for every supported DK (KCPR*KRPB = 16 divides 32), so t drops out.
    const int v_swz = (r32 >> 1) & 7;             // 32*dvt is even and a multiple of 16 rows -> drops out as well

    stage(0, 0);
    load_q_frags<DT>(qf, Qg, q0 + r32, p.Tq, p.ldq, hh);  // lane holds Q[q0 + r32][16*s + 8*hh + 0..7]
    if constexpr (QK_PAIR) load_q_frags<DT>(ql, (const T *)p.Q_lo + b * p.sQb + (int64_t)h * DK, q0 + r32, p.Tq, p.ldq, hh);
    for (int kt = 0; kt < ntiles; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 1 < ntiles) stage(kt + 1, (kt + 1) & 1);
        const char *kb = smem + ((kt & 1) * KS + kh) * (K_STG + V_TILE);
        const char *vb = kb + K_STG;

        // ---- S^T = K Q^T for the two 32-key halves
        f32x16 sacc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int j = 0; j < 16; ++j) sacc[t][j] = 0.f;
            if constexpr (QK_PAIR && DK == 128) {
                // The same sum in the same order -- the two small products first, the large one last -- with the K
                // fragments streamed: K_lo and K_hi of one k-step feed the two small products and are dropped, then K_hi
                // is read from LDS a second time for the large product (16 fragments held at once would be 64 registers).
#pragma unroll
                for (int s = 0; s < NQS; ++s) {
                    const int chunk = (2 * s + hh) ^ k_swz;
                    const V8 kl = *(const V8 *)(kb + K_TILE + k_off[t] + chunk * 16);
                    const V8 kf = *(const V8 *)(kb + k_off[t] + chunk * 16);
                    sacc[t] = Op<DT>::mfma32(kl, qf[s], sacc[t]);
                    sacc[t] = Op<DT>::mfma32(kf, ql[s], sacc[t]);
                }
                asm volatile("" ::: "memory");   // (keeps the second read a read: no K_hi fragment lives across this line)
#pragma unroll
                for (int s = 0; s < NQS; ++s) {
                    const int chunk = (2 * s + hh) ^ k_swz;
                    const V8 kf = *(const V8 *)(kb + k_off[t] + chunk * 16);
                    sacc[t] = Op<DT>::mfma32(kf, qf[s], sacc[t]);
                }
            } else if constexpr (QK_PAIR) {
                // the small products first (K_lo Q_hi^T, then K_hi Q_lo^T), the large one last; every K fragment is read
                // from LDS once
                V8 kh_f[NQS], kl_f[NQS];
#pragma unroll
                for (int s = 0; s < NQS; ++s) {
                    const int chunk = (2 * s + hh) ^ k_swz;
                    kh_f[s] = *(const V8 *)(kb + k_off[t] + chunk * 16);
                    kl_f[s] = *(const V8 *)(kb + K_TILE + k_off[t] + chunk * 16);
                }
#pragma unroll
                for (int s = 0; s < NQS; ++s) sacc[t] = Op<DT>::mfma32(kl_f[s], qf[s], sacc[t]);
#pragma unroll
                for (int s = 0; s < NQS; ++s) sacc[t] = Op<DT>::mfma32(kh_f[s], ql[s], sacc[t]);
#pragma unroll
                for (int s = 0; s < NQS; ++s) sacc[t] = Op<DT>::mfma32(kh_f[s], qf[s], sacc[t]);
            } else
#pragma unroll
            for (int s = 0; s < NQS; ++s) {
                const int chunk = (2 * s + hh) ^ k_swz;
                const V8 kf = *(const V8 *)(kb + k_off[t] + chunk * 16);
                sacc[t] = Op<DT>::mfma32(kf, qf[s], sacc[t]);
            }
        }
        // ---- scale to base 2, mask keys past Tk (last tile only), tile max
        const bool tail = KS == 1 && (kt == ntiles - 1) && (p.Tk % KT != 0);
        // The max is taken on the RAW scores (scale > 0 commutes with max); the scale and the max subtraction are
        // then one FMA per element:  p = exp2(s * c - m * c).
        float mx = -INFINITY;
        if (tail) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = (tile0 + kt) * KT + 32 * t + (i & 3) + 8 * (i >> 2) + 4 * hh;
                    if (key >= p.Tk) sacc[t][i] = -INFINITY;
                }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sacc[t][i]);
        mx = max_halves(mx) * p.scale_log2;
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // first tile: exp2(-inf) = 0
        m_run = m_new;
        float psum = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float e = __builtin_amdgcn_exp2f(fmaf(sacc[t][i], p.scale_log2, -m_new));
                sacc[t][i] = e;
                psum += e;
            }
        l_run = l_run * alpha + psum;
        // rescale the output accumulators only when some row's running max actually moved (alpha == 1
        // exactly otherwise): after the first few tiles this is rare and saves NDT*16 multiplies per tile
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
#pragma unroll
            for (int d = 0; d < NDT; ++d)
#pragma unroll
                for (int j = 0; j < 16; ++j) oacc[d][j] *= alpha;
        }

        // ---- P^T fragments: registers 8s..8s+7 of the S^T accumulator are the B operand of k-step s
        V8 pf[2][2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[t][s][j] = Op<DT>::from_f32(sacc[t][8 * s + j]);

        // ---- O^T += V^T P^T.  A fragment element j <-> key 32t + 16s + 8(j>>2) + 4hh + (j&3)
#pragma unroll
        for (int d = 0; d < NDT; ++d) {
            const char *vrow = vb + (32 * d + r32) * 128;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    V4 lo, hi;
                    if constexpr (VROW) {
                        // V tile is ROW-major [64 keys][DV]; the fragment is read TRANSPOSED by
                        // ds_read_b64_tr_b16: per 16-lane group a 4-key x 16-column block, lane 4q+p supplies the
                        // address of key q / columns 4p..4p+3 and receives its own column of the 4 keys.
                        // chunk swizzle vrow_swz<DV>(row): conflict-free transposed reads (see the top of the kernel)
                        const int q4 = (lane & 15) >> 2, p4 = lane & 3, g1 = (lane >> 4) & 1;
                        const int chunk = d * 4 + 2 * g1 + (p4 >> 1);
#pragma unroll
                        for (int jj = 0; jj < 2; ++jj) {
                            const int key = 32 * t + 16 * s + 8 * jj + 4 * hh + q4;
                            const int f = vrow_swz<DV>(key);
                            const char *a = vb + key * (DV * 2) + ((chunk ^ f) << 4) + 8 * (p4 & 1);
                            const tr4 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                                (__attribute__((address_space(3))) tr4 *)a);
                            if (jj == 0) lo = __builtin_bit_cast(V4, r);
                            else hi = __builtin_bit_cast(V4, r);
                        }
                    } else {
                        const int g = 8 * t + 4 * s + hh;  // 8-byte granule of keys [4g, 4g+4); second one is g+2
                        lo = *(const V4 *)(vrow + ((((g >> 1)) ^ v_swz) << 4) + (g & 1) * 8);
                        hi = *(const V4 *)(vrow + ((((g + 2) >> 1) ^ v_swz) << 4) + (g & 1) * 8);
                    }
                    V8 vf;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        vf[j] = lo[j];
                        vf[4 + j] = hi[j];
                    }
                    oacc[d] = Op<DT>::mfma32(vf, pf[t][s], oacc[d]);
                }
        }
    }

    if constexpr (KS > 1) {
        // ---- merge the key parts: parts 1 .. KS-1 park (O^T, m, l) in LDS (the ring is free behind the barrier), part 0
        // folds them in one after the other: m = max(m0, m1), O = O0 2^(m0 - m) + O1 2^(m1 - m), l likewise (per-lane
        // partials)
        __syncthreads();
        constexpr int MW = NDT * 16 + 2;
        if (kh > 0) {
            float *mg = (float *)smem + (size_t)(((kh - 1) * NWQ + qb) * 64 + lane) * MW;
#pragma unroll
            for (int d = 0; d < NDT; ++d)
#pragma unroll
                for (int j = 0; j < 16; ++j) mg[d * 16 + j] = oacc[d][j];
            mg[NDT * 16] = m_run;
            mg[NDT * 16 + 1] = l_run;
        }
        __syncthreads();
        if (kh == 0) {
#pragma unroll
            for (int part = 1; part < KS; ++part) {
                const float *mg = (const float *)smem + (size_t)(((part - 1) * NWQ + qb) * 64 + lane) * MW;
                const float m1 = mg[NDT * 16], l1 = mg[NDT * 16 + 1];
                const float m = fmaxf(m_run, m1);
                const float a0 = __builtin_amdgcn_exp2f(m_run - m), a1 = __builtin_amdgcn_exp2f(m1 - m);
#pragma unroll
                for (int d = 0; d < NDT; ++d)
#pragma unroll
                    for (int j = 0; j < 16; ++j) oacc[d][j] = oacc[d][j] * a0 + mg[d * 16 + j] * a1;
                l_run = l_run * a0 + l1 * a1;
                m_run = m;
            }
        }
    }
    // ---- epilogue: combine the two half-column sums, normalise, store O[q][h*DV + d]
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    if (p.o_rows16) {
        // Through LDS (the ring is free after the barrier), so that this wave's 32 rows leave as whole lines -- a lane
        // stores 16 contiguous bytes, DV / 8 lanes one row -- instead of 8-byte pieces of 32 different rows per
        // instruction (stamps of the pipelined kernel below: that form spent 8.7 k cycles per workgroup issuing stores).
        __syncthreads();
        if (kh != 0) return;                     // (KS > 1: the first key part's waves hold the merged result)
        char *const ost = smem + qb * (32 * OROW);
        char *const orow = ost + r32 * OROW;
#pragma unroll
        for (int d = 0; d < NDT; ++d)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                V4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = Op<DT>::from_f32(oacc[d][4 * g4 + j] * inv);
                *(V4 *)(orow + (32 * d + 8 * g4 + 4 * hh) * 2) = o;
            }
        constexpr int CPR = DV / 8;  // 16-byte chunks per row
        T *const og = (T *)p.O + b * p.sOb + (int64_t)h * DV;
#pragma unroll
        for (int idx0 = 0; idx0 < 32 * CPR; idx0 += 64) {
            const int idx = idx0 + lane;
            const int row = idx / CPR, ch = idx % CPR;
            if (idx < 32 * CPR && q0 + row < p.Tq)
                *(V8 *)(og + (int64_t)(q0 + row) * p.ldo + ch * 8) = *(const V8 *)(ost + row * OROW + ch * 16);
        }
        return;
    }
    const int q = q0 + r32;
    if (q < p.Tq && kh == 0) {
        T *orow = (T *)p.O + b * p.sOb + (int64_t)q * p.ldo + (int64_t)h * DV;
#pragma unroll
        for (int d = 0; d < NDT; ++d)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                V4 o, l;
                scaled_pair4<DT>(oacc[d], 4 * g4, inv, o, l);
                *(V4 *)(orow + 32 * d + 8 * g4 + 4 * hh) = o;
                if constexpr (QK_PAIR)  // the output as a pair: lo = o - float(hi)
                    if (p.O_lo) *(V4 *)((T *)p.O_lo + (orow - (T *)p.O) + 32 * d + 8 * g4 + 4 * hh) = l;
            }
    }
}

#ifdef PIO_EXPERIMENTS
#include "../../tools/experiments/pio_flash_variants.inc"
#endif

#ifdef PIO_EXPERIMENTS
// (experiments build only) variant of the row-major-V kernel: 0 = lock-step waves (flash_attn_kernel, the shipped one),
// 1 = one wave per SIMD with the softmax in the MFMAs' shadow (flash_attn_pipe_kernel), 2 = two staggered wave groups
// (flash_attn_stag_kernel).  which == -2 only reads; returns the previous setting.  Initial value: env PIO_FLASH_VARIANT.
int flash_variant_override(int which) {
    static int cur = [] {
        const char *e = getenv("PIO_FLASH_VARIANT");
        const int v = e ? atoi(e) : PIO_FLASH_DEFAULT_VARIANT;
        return (v >= 0 && v <= 2) ? v : PIO_FLASH_DEFAULT_VARIANT;
    }();
    const int prev = cur;
    if (which >= 0 && which <= 2) cur = which;
    return prev;
}
extern "C" int pio_debug_flash_variant(int which) { return flash_variant_override(which); }
#endif

// The instantiation flash_route names: (V^T, 4, 1), (row, 4, 1), (row, 8, 1), (row, 8, 2) for every head shape, and
// (row, 16, 4) for the narrow heads.  The pair-operand 128-wide head (flash_pair_route) has the first three: two key parts
// would need 192 KB of ring.
template <int DT, int DK, int DV, bool PAIR>
static void flash_launch(const FlashRoute &r, dim3 grid, hipStream_t s, const FlashParams &p) {
    void (*k)(FlashParams) = flash_attn_kernel<DT, DK, DV, false, 4, 1, PAIR>;
    if (r.v_rowmajor) k = flash_attn_kernel<DT, DK, DV, true, 4, 1, PAIR>;
    if constexpr (PAIR && DK == 128) {
        if (r.NW == 8) k = flash_attn_kernel<DT, DK, DV, true, 8, 1, PAIR>;
    } else {
        if (r.NW == 8) k = r.KS == 2 ? flash_attn_kernel<DT, DK, DV, true, 8, 2, PAIR> : flash_attn_kernel<DT, DK, DV, true, 8, 1, PAIR>;
        if constexpr (DK <= 64 && DV <= 64)
            if (r.NW == 16) k = flash_attn_kernel<DT, DK, DV, true, 16, 4, PAIR>;
    }
    hipLaunchKernelGGL(k, grid, dim3(r.threads), 0, s, p);
}
// ... over the operand dtype and, on the DK = 32 and the (128, 128) fp16 heads, the pair-operand (QK_PAIR) instantiations
template <int DK, int DV>
static void flash_launch_dt(int dtype, bool pair, const FlashRoute &r, dim3 grid, hipStream_t s, const FlashParams &p) {
    if constexpr (DK == 32 || (DK == 128 && DV == 128))
        if (pair) return flash_launch<PIO_DT_F16, DK, DV, true>(r, grid, s, p);
    if (dtype == PIO_DT_F16) flash_launch<PIO_DT_F16, DK, DV, false>(r, grid, s, p);
    else flash_launch<PIO_DT_BF16, DK, DV, false>(r, grid, s, p);
}

int flash_attention_launch(int dtype, int dkp, int dvp, int dk_logical, const AttnOperands &t, int B, int H, int Tq, int Tk,
                           bool v_rowmajor, hipStream_t s) {
    static const bool ksplit_on = [] {
        const char *e = getenv("PIO_FLASH_KSPLIT");
        return !e || atoi(e) != 0;
    }();
    const FlashPlan plan = flash_launch_plan(dtype, dkp, dvp, t, B, H, Tq, Tk, v_rowmajor, ksplit_on, cu_budget());
    if (plan.err) return plan.err;
    const FlashRoute &r = plan.route;
    FlashParams p{t.Q, t.K, t.VT, t.O, Tq, Tk, H, r.nqt, t.ldq, t.ldk, t.ldvt, t.ldo, t.sQb, t.sKb, t.sVb, t.sOb,
                  attn_scale_log2(dk_logical), plan.o_rows16, t.Q_lo, t.K_lo, t.O_lo};
    dim3 grid((unsigned)plan.grid, 1, 1);
    const AttnWork work = attn_work(dkp, dvp, B, H, Tq, Tk);
    ProfScope prof(PROF_FLASH, work.flops, work.bytes, s);
    int variant = 0;
#ifdef PIO_EXPERIMENTS
    variant = flash_variant_override(-2);   // (experiments build: pio_debug_flash_variant / env PIO_FLASH_VARIANT)
#endif
    static const bool debug = [] {
        const char *e = getenv("PIO_FLASH_DEBUG");
        return e && atoi(e) != 0;
    }();
    if (debug)
        fprintf(stderr, "[pio] fused attention B=%d H=%d Tq=%d Tk=%d dkp=%d dvp=%d v_rowmajor=%d NW=%d KS=%d variant=%d\n", B,
                H, Tq, Tk, dkp, dvp, (int)v_rowmajor, r.NW, r.KS, variant);
#ifdef PIO_EXPERIMENTS
    if (!plan.pair && v_rowmajor && Tq >= 256 && Tk % 128 == 0 && variant == 1 && plan.o_rows16) {
        FlashParams pp = p;
        pp.nqt = (Tq + 255) / 256;
        dim3 pgrid((unsigned)(pp.nqt * B * H), 1, 1);
        if (dtype == PIO_DT_F16) hipLaunchKernelGGL((flash_attn_pipe_kernel<PIO_DT_F16>), pgrid, dim3(256), 0, s, pp);
        else hipLaunchKernelGGL((flash_attn_pipe_kernel<PIO_DT_BF16>), pgrid, dim3(256), 0, s, pp);
        return launch_status();
    }
    if (!plan.pair && r.NW == 8 && r.KS == 1 && variant == 2) {
        if (dtype == PIO_DT_F16) hipLaunchKernelGGL((flash_attn_stag_kernel<PIO_DT_F16>), grid, dim3(512), 0, s, p);
        else hipLaunchKernelGGL((flash_attn_stag_kernel<PIO_DT_BF16>), grid, dim3(512), 0, s, p);
        return launch_status();
    }
#endif
    if (dkp == 128) flash_launch_dt<128, 128>(dtype, plan.pair, r, grid, s, p);
    else if (dkp == 64) flash_launch_dt<64, 64>(dtype, plan.pair, r, grid, s, p);
    else if (dvp == 32) flash_launch_dt<32, 32>(dtype, plan.pair, r, grid, s, p);
    else flash_launch_dt<32, 160>(dtype, plan.pair, r, grid, s, p);
    return launch_status();
}

}  // namespace pio
