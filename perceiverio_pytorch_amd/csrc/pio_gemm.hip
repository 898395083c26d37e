// NT GEMM on gfx950 matrix cores:  C = epilogue(alpha * A B^T)
//   A [M,K], B [N,K]: 16-bit operands (fp16 / bf16), K contiguous -- exactly the layout of an
//   nn.Linear weight ([out,in], transformer_primitives.py:73-75) and of a row-major activation, so
//   neither operand is ever transposed in memory.
//   Replaces F.linear / matmul at transformer_primitives.py:93-95, 110, 138, 163, 213-215.
//
// v1 structure (128x128x64 tile, 4 waves as 2x2, one 64x64 sub-tile per wave, MFMA 16x16x32):
//   * both operand tiles go HBM -> LDS by LDS-DMA (global_load_lds_dwordx4): the LDS image is lane-linear,
//     the XOR swizzle is applied to the per-lane SOURCE address and again on the ds_read_b128 side;
//   * rows past M / N are clamped (their results are never stored), 8-element K chunks past K read a
//     16-byte zero block, so no operand needs padding beyond a multiple of 8;
//   * double-buffered, ONE barrier per K step: the DMA of tile t+1 is in flight while tile t is multiplied;
//   * the MFMA is issued as (B-fragment, A-fragment) so that each lane ends up with 4 CONSECUTIVE output
//     columns of one row: bias / residual / stores are 8- or 16-byte vectors;
//   * optional second K sweep with one operand replaced by its *_lo image (W = W_hi + W_lo, the "x2w"
//     precision policy) accumulating into the same registers.
#include "pio_gemm_common.h"

namespace pio {


#ifdef PIO_G128_STAMPS
// Dev-only (tools/g128_stamps.py builds a private copy of the library with this flag): thread 0 of one workgroup records
// s_memtime at four points of each of the first 30 K steps (in LDS: stores would count in vmcnt), and at the kernel's edges.
__device__ unsigned long long g128_stamps[128];
__device__ int g128_block;
#define G128_STAMP(i)                                                                  \
    do {                                                                               \
        if (stamp_on && (i) < 128) stamp_lds[i] = __builtin_readcyclecounter();        \
    } while (0)
#else
#define G128_STAMP(i)
#endif

constexpr int BK = 64;   // (the default tile BM x BN: pio_gemm_route.h; the kernel is templated on TM x TN)

// KIND only tags the instantiation (0: one flat [rows,K]x[N,K] linear, 1: batched attention product) so that
// profilers report the two uses under different kernel names.
// TM x TN: 128 x 128 (four waves of 64 x 64) or 64 x 64 (four waves of 32 x 32: problems whose 128 x 128 tiling would
// leave most of the 256 CUs idle -- a 2048-row latent stack at batch 1 has 64 such tiles per GEMM).
// NS: operand stages in LDS.  2 = double buffer, the DMA of step t+1 against the MFMAs of step t (two workgroups per CU
// hide each other's waits: the 128 x 128 tile on problems with many tiles).  4 (the 64 x 64 tile: problems of at most a
// tile per CU, where nobody else covers a wait) = a RING: the pieces of step t+3 are issued at the top of step t, a
// counted s_waitcnt vmcnt leaves two steps in flight across a raw s_barrier, every wave issues the same number of pieces
// per step (steps past the end re-read valid memory into the slot the ring would use next: never read) -- with the
// double buffer a 64 x 64 x 1024 tile spent ~1.9 k cycles per 64-deep step (the latency of one LDS-DMA round trip under
// load) on 128 cycles of MFMAs.  (A six-stage ring -- four steps in flight, 96 KiB, one workgroup per CU -- measured no
// better than four stages with two workgroups per CU: DESIGN_LOG R3.3.)
// KG: K groups.  2 = EIGHT waves, two teams of four that each run the whole loop below on every other 64-deep K step
// (own ring, own accumulators; the row pass sums the two epilogue images).  An LDS-DMA piece of 16 bytes a lane holds its
// wave for ~150 cycles (tools/g128_stamps.py: the 3-4 pieces of a step are ~440 of its ~700 cycles, four waves together
// reach 27 B/clk where tools/dma_bench.hip needs eight for the path's 54): a tile that owns its CU alone gets the second
// team instead of a second workgroup.
template <int DT, int KIND, int TM, int TN, int NS, int KG = 1>
__global__ __launch_bounds__(256 * KG) void gemm_nt_128(const GemmParams p) {
    typedef typename Op<DT>::T T;
    typedef typename Op<DT>::V8 V8;
    constexpr int A_BYTES = TM * BK * 2, B_BYTES = TN * BK * 2;     // operand tiles: rows x 128 bytes
    constexpr int A_PPW = TM / 32, B_PPW = TN / 32;                  // 1-KiB pieces (8 rows) per wave
    constexpr int MI = TM / 32, NI = TN / 32;                        // 16 x 16 units per wave (waves as 2 x 2)
    constexpr int EPI_BYTES = TM * TN * 4;
    // (+ TM x (rstd, -mean rstd) behind the epilogue image: the LayerNorm fold's consumer)
    constexpr int TEAM_BYTES = NS * (A_BYTES + B_BYTES);           // one team's ring
    constexpr int SMEM = KG * (TEAM_BYTES > EPI_BYTES ? TEAM_BYTES : EPI_BYTES) + TM * 8;
    static_assert(NS == 2 || (NS - 2) * (A_PPW + B_PPW) <= 63, "the counted wait must fit vmcnt");
    __shared__ __attribute__((aligned(16))) char smem[SMEM];        // A stages, B stages (then the epilogue image)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);   // inside the team
    const int kg = KG == 1 ? 0 : __builtin_amdgcn_readfirstlane(tid >> 8);
    char *const ring = smem + kg * TEAM_BYTES;
    const int wm = wave >> 1, wn = wave & 1;
#ifdef PIO_G128_STAMPS
    __shared__ unsigned long long stamp_lds[128];
    const bool stamp_on = (int)blockIdx.x == g128_block && blockIdx.y == 0 && tid == 0;
    G128_STAMP(120);
#endif

    const int tile_n = blockIdx.x % p.tiles_n;
    const int tile_m = blockIdx.x / p.tiles_n;
    const int z = blockIdx.y;
    const int zb = z / p.nh, zh = z % p.nh;

    const T *A = (const T *)p.A + zb * p.sAb + zh * p.sAh;
    const T *B = (const T *)p.B + zb * p.sBb + zh * p.sBh;

    // ---- staging addresses: wave w, piece i covers tile rows (w*4+i)*8 .. +8, lane -> (row, 16-B slot)
    const int srow = lane >> 3;
    const int sslot = lane & 7;
    const T *a_src[A_PPW];
    const T *b_src[B_PPW];
    int a_koff[A_PPW], b_koff[B_PPW];
#pragma unroll
    for (int i = 0; i < A_PPW; ++i) {
        const int r = (wave * A_PPW + i) * 8 + srow;       // row inside the tile
        const int c = sslot ^ ((r >> 1) & 7);              // source chunk that lands in this slot
        a_koff[i] = c * 8;
        int gm = tile_m * TM + r;
        gm = gm < p.M ? gm : p.M - 1;
        a_src[i] = A + (int64_t)gm * p.lda + c * 8;
    }
#pragma unroll
    for (int i = 0; i < B_PPW; ++i) {
        const int r = (wave * B_PPW + i) * 8 + srow;
        const int c = sslot ^ ((r >> 1) & 7);
        b_koff[i] = c * 8;
        int gn = tile_n * TN + r;
        gn = gn < p.N ? gn : p.N - 1;
        b_src[i] = B + (int64_t)gn * p.ldb + c * 8;
    }
    const T *zsrc = (const T *)g_zero16;

    const int nk1 = (p.K + BK * KG - 1) / (BK * KG);   // steps per pass (of one team)
    const int nk = p.npass * nk1;

    auto stage = [&](int kt, int buf) {
        const int pass = (kt >= nk1) + (kt >= 2 * nk1);   // wave-uniform
        const int k0 = ((kt - pass * nk1) * KG + kg) * BK;   // (a team's step past K reads the zero chunk)
        const int64_t dA = pass == 0 ? 0 : (pass == 1 ? p.dA1 : p.dA2);
        const int64_t dB = pass == 0 ? 0 : (pass == 1 ? p.dB1 : p.dB2);
        char *abase = ring + buf * A_BYTES;
        char *bbase = ring + NS * A_BYTES + buf * B_BYTES;
#pragma unroll
        for (int i = 0; i < A_PPW; ++i) {
            const T *sa = (k0 + a_koff[i]) < p.K ? (a_src[i] + k0 + dA) : zsrc;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)sa,
                                             (__attribute__((address_space(3))) void *)(abase + (wave * A_PPW + i) * 1024),
                                             16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < B_PPW; ++i) {
            const T *sb = (k0 + b_koff[i]) < p.K ? (b_src[i] + k0 + dB) : zsrc;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)sb,
                                             (__attribute__((address_space(3))) void *)(bbase + (wave * B_PPW + i) * 1024),
                                             16, 0, 0);
        }
    };

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // ---- fragment read addresses (bytes inside a tile): row = base16 + (lane&15), chunk = ks*4 + (lane>>4)
    const int frow = lane & 15;
    const int fswz = (frow >> 1) & 7;
    const int fchunk = lane >> 4;
    int a_off[MI], b_off[NI];
#pragma unroll
    for (int i = 0; i < MI; ++i) a_off[i] = (wm * (TM / 2) + i * 16 + frow) * 128;
#pragma unroll
    for (int i = 0; i < NI; ++i) b_off[i] = (wn * (TN / 2) + i * 16 + frow) * 128;

    // Epilogue operands fetched HERE, ahead of the ring (older than every DMA piece: the counted waits still hold): the
    // bias / LayerNorm-fold column constants of this thread's four columns and, for the fold's consumer, the row's partial
    // sums -- on the small tiles their round trips (two dependent ones: statistics -> barrier -> constants) were ~1.5 us of
    // a ~9 us launch, exposed behind the last K step.
    constexpr int CPR_ = TN / 4;
    const int pre_n0 = tile_n * TN + (tid & (CPR_ - 1)) * 4;
    f32x4 bias_pre = {0.f, 0.f, 0.f, 0.f}, lnc_pre = {0.f, 0.f, 0.f, 0.f};
    constexpr int MAXS = 24;                     // statistics slots held in registers (K <= 1536 in 64-column slots)
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    f32x2 part_pre[MAXS];
    // (branch-free: whole 16-byte loads of interior columns, slot indices clamped -- a conditional load costs a branch and
    //  a drained vmcnt each; edge tiles and unaligned operands fetch in the epilogue as before)
    // (only the 32 x 64 tile: same-box A/B of the ImageNet forward, graph replay, B = 1 2.940 -> 2.899 ms; with it on the
    //  64 x 64 tile B = 4 4.66 -> 4.73, B = 8 7.20 -> 7.23 -- two workgroups per CU cover each other's epilogue, the 48
    //  registers only cost)
    constexpr bool PRE = TM == 32;
    const bool pre_cols = PRE && tid < 256 && pre_n0 + 3 < p.N && (p.bias_mode != 1 || p.bias_vec) &&
                          (!p.ln_part || ((uintptr_t)p.ln_c & 15) == 0);
    const bool pre_stat = PRE && p.ln_part && p.ln_slots <= MAXS && ((uintptr_t)p.ln_part & 7) == 0;
    if (pre_cols) {
        if (p.bias_mode == 1) bias_pre = *(const f32x4 *)(p.bias + pre_n0);
        if (p.ln_part) lnc_pre = *(const f32x4 *)(p.ln_c + pre_n0);
    }
    if (pre_stat && tid < TM) {
        int m = tile_m * TM + tid;
        m = m < p.M ? m : p.M - 1;
        const f32x2 *pr = (const f32x2 *)(p.ln_part + (int64_t)m * p.ln_slots * 2);
        const int last = p.ln_slots - 1;
#pragma unroll
        for (int i = 0; i < MAXS; ++i) part_pre[i] = pr[i < last ? i : last];
    }
    // (nothing of the above may sink below a DMA piece: a younger plain load would shift the window of the counted waits)
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (NS == 2) stage(0, 0);
    else {
        // ring prologue: steps 0 .. NS-2 in flight (a step past the end repeats step 0's valid sources: the counts stay
        // exact, the slot is never read)
#pragma unroll
        for (int j = 0; j < NS - 1; ++j) stage(j < nk ? j : 0, j);
    }
    int slot = 0;  // (NS > 2) ring slot of step kt
    G128_STAMP(121);
    for (int kt = 0; kt < nk; ++kt) {
        G128_STAMP(kt < 30 ? kt * 4 : 127);
        const int cur = NS == 2 ? (kt & 1) : slot;
        const char *abase = ring + cur * A_BYTES;
        const char *bbase = ring + NS * A_BYTES + cur * B_BYTES;
        V8 af[2][MI], bf[2][NI];
        // the step's fragment reads go out BEFORE the next stage's DMA pieces (whose issue holds the wave for ~130 cycles a
        // piece with all four waves at the TA together: tools/g128_stamps.py), so the LDS latency passes under the issue
        auto frags = [&]() {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int coff = ((ks * 4 + fchunk) ^ fswz) << 4;
#pragma unroll
                for (int i = 0; i < MI; ++i) af[ks][i] = *(const V8 *)(abase + a_off[i] + coff);
#pragma unroll
                for (int i = 0; i < NI; ++i) bf[ks][i] = *(const V8 *)(bbase + b_off[i] + coff);
            }
        };
        if constexpr (NS == 2) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            G128_STAMP(kt < 30 ? kt * 4 + 1 : 127);
            frags();
            if (kt + 1 < nk) stage(kt + 1, (kt + 1) & 1);
        } else {
            // all but the youngest NS-2 steps' pieces have landed: step kt is complete in this wave's share, after the
            // barrier in every wave's; and every wave has left step kt-1 (its fragment reads were consumed by its
            // MFMAs), whose slot takes step kt+NS-1.  A raw s_barrier: __syncthreads() would drain vmcnt to zero.
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * (A_PPW + B_PPW)) : "memory");
            __builtin_amdgcn_s_barrier();
            G128_STAMP(kt < 30 ? kt * 4 + 1 : 127);
            const int nslot = slot == 0 ? NS - 1 : slot - 1;
            frags();
            G128_STAMP(kt < 30 ? kt * 4 + 3 : 127);   // (the stamp's own lgkmcnt(0) waits for the fragment reads)
            stage(kt + NS - 1 < nk ? kt + NS - 1 : 0, nslot);
        }
        G128_STAMP(kt < 30 ? kt * 4 + 2 : 127);
        if constexpr (NS != 2) slot = slot + 1 == NS ? 0 : slot + 1;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = Op<DT>::mfma16(bf[ks][ni], af[ks][mi], acc[mi][ni]);
    }

    // ---- epilogue through LDS: the accumulators (lane = one row, 4 consecutive columns) are parked in a
    // [TM][TN] fp32 image (16-byte chunks XOR-swizzled by row, conflict-free both ways) so that the
    // bias / GELU / residual / store pass walks whole rows: a wave touches 2 rows x 512 contiguous bytes
    // (fp32) or 2 rows x 256 bytes (16-bit) per instruction instead of 16 rows x 64 bytes.
    G128_STAMP(122);
    if constexpr (NS != 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the ring's surplus pieces: land before the image)
    __syncthreads();  // every wave is done reading the last operand tile
    G128_STAMP(123);
    float *cs = (float *)smem + kg * (TM * TN);   // (team kg's image; both are summed in the row pass)
    constexpr int CPR = TN / 4;  // 16-byte chunks per image row (32 or 16)
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int ml = wm * (TM / 2) + mi * 16 + (lane & 15);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            const int c = wn * (CPR / 2) + ni * 4 + (lane >> 4);
            *(f32x4 *)(cs + ml * TN + ((c ^ (ml & (CPR - 1))) << 2)) = acc[mi][ni];
        }
    }
    // LayerNorm fold on the small tiles (stacks too short for the 256 x 256 kernel: the flow / multimodal latents, small
    // batches).  Consumer: row m's (mean, rstd) from the ln_slots partial (sum, sum of squares) pairs its producer left,
    // once per tile row, parked behind the image.  Producer (below): residual pair in, result pair out, 64-column sums.
    float *const stat = (float *)(smem + SMEM - TM * 8);
    if (p.ln_part && tid < TM) {
        int m = tile_m * TM + tid;
        m = m < p.M ? m : p.M - 1;
        const float *pr = p.ln_part + (int64_t)m * p.ln_slots * 2;
        float sm = 0.f, sq = 0.f;
        if (pre_stat) {
#pragma unroll
            for (int i = 0; i < MAXS; ++i) {     // (same order of additions as the loop below)
                sm += i < p.ln_slots ? part_pre[i][0] : 0.f;
                sq += i < p.ln_slots ? part_pre[i][1] : 0.f;
            }
        } else {
            for (int i = 0; i < p.ln_slots; ++i) {
                sm += pr[2 * i];
                sq += pr[2 * i + 1];
            }
        }
        const float mean = sm * p.ln_inv_k;
        float var = sq * p.ln_inv_k - mean * mean;
        var = var > 0.f ? var : 0.f;
        const float rstd = 1.0f / sqrtf(var + p.ln_eps);
        stat[2 * tid] = rstd;
        stat[2 * tid + 1] = -mean * rstd;
    }
    __syncthreads();
    if (KG > 1 && tid >= 256) return;   // the row pass belongs to the first team (no barrier below)
    cs = (float *)smem;
    const int64_t coffz = zb * p.sCb + zh * p.sCh;
    const int c = tid & (CPR - 1);
    constexpr int RPI = 256 / CPR;  // rows per pass of the 256 threads (8 or 16)
    const int n0 = tile_n * TN + c * 4;
    if (n0 < p.n_store) {
        const bool nfull = n0 + 3 < p.N;
        f32x4 bias_n = bias_pre, lnc = lnc_pre;   // (fetched ahead of the K loop ...
        if (!pre_cols) {                          //  ... except on edge tiles / unaligned operands)
            if (p.bias_mode == 1) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n0 + r < p.N) bias_n[r] = p.bias[n0 + r];
            }
            if (p.ln_part) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n0 + r < p.N) lnc[r] = p.ln_c[n0 + r];
            }
        }
#pragma unroll 4
        for (int it = 0; it < TM / RPI; ++it) {
            const int ml = it * RPI + tid / CPR;
            const int m = tile_m * TM + ml;
            if (m >= p.M) break;  // rows are visited in increasing order
            f32x4 v = *(const f32x4 *)(cs + ml * TN + ((c ^ (ml & (CPR - 1))) << 2));
            if constexpr (KG > 1) {
                const f32x4 v2 = *(const f32x4 *)(cs + TM * TN + ml * TN + ((c ^ (ml & (CPR - 1))) << 2));
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += v2[r];
            }
            if (p.row_part) {
                // ---- fold producer (launcher: N % 64 == 0, n_store == N, 16-bit rows 8-byte aligned): x = acc + bias +
                // residual pair, leaves as the pair (X16, X16_lo) [+ fp32 C] with the row's (sum, sum of squares) over
                // this thread group's 64 columns; the 16 lanes of a group sit in one wave and share the row
                typedef typename Op<DT>::V4 V4;
                const V4 hh = *(const V4 *)((const T *)p.R16_hi + (int64_t)m * p.ld16 + n0);
                const V4 ll = *(const V4 *)((const T *)p.R16_lo + (int64_t)m * p.ld16 + n0);
                V4 h, l;
                float rsum = 0.f, rsq = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float x = v[r] * p.alpha + bias_n[r] + (Op<DT>::to_f32(hh[r]) + Op<DT>::to_f32(ll[r]));
                    v[r] = x;
                    h[r] = Op<DT>::from_f32(x);
                    l[r] = Op<DT>::from_f32(x - Op<DT>::to_f32(h[r]));
                    rsum += x;
                    rsq += x * x;
                }
                *(V4 *)((T *)p.X16 + (int64_t)m * p.ld16 + n0) = h;
                *(V4 *)((T *)p.X16_lo + (int64_t)m * p.ld16 + n0) = l;
                if (p.C) *(f32x4 *)((float *)p.C + (int64_t)m * p.ldc + n0) = v;
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) {
                    rsum += __shfl_xor(rsum, o, 64);
                    rsq += __shfl_xor(rsq, o, 64);
                }
                if ((tid & 15) == 0) {
                    float *dst = p.row_part + ((int64_t)m * (p.N >> 6) + (n0 >> 6)) * 2;
                    dst[0] = rsum;
                    dst[1] = rsq;
                    if (p.range_flag && !(rsq <= 3.0e38f)) *p.range_flag = 1;
                }
                continue;
            }
            if (p.ln_part) {
                // ---- fold consumer: LayerNorm(x) W^T + b = rstd (x W'^T) - rstd mean c + b'   (alpha == 1: launcher)
                const float rs = stat[2 * ml], nm = stat[2 * ml + 1];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = v[r] * rs + nm * lnc[r];
            }
            const float bias_m = (p.bias_mode == 2) ? p.bias[m] : 0.f;
            const float *rrow = nullptr;
            if (p.R) {
                rrow = (p.r_rows > 0)
                           ? p.R + (int64_t)(m / p.r_rows) * p.r_stride_b + (int64_t)(m % p.r_rows) * p.ldr
                           : p.R + (int64_t)m * p.ldr;
            }
            f32x4 rv = {0.f, 0.f, 0.f, 0.f};
            if (rrow) {
                if (nfull && p.r_vec) {
                    rv = *(const f32x4 *)(rrow + n0);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (n0 + r < p.N) rv[r] = rrow[n0 + r];
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float x = v[r] * p.alpha + bias_n[r] + bias_m;
                if (p.act == 1) x = gelu_erf(x);
                x += rv[r];
                v[r] = (n0 + r < p.N) ? x : 0.f;  // columns [N, n_store) are written as zeros
            }
            const bool sfull = n0 + 3 < p.n_store;
            if (p.out_f32) {
                float *crow = (float *)p.C + coffz + (int64_t)m * p.ldc;
                if (p.vec_ok && sfull) {
                    *(f32x4 *)(crow + n0) = v;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (n0 + r < p.n_store) crow[n0 + r] = v[r];
                }
            } else {
                T *crow = (T *)p.C + coffz + (int64_t)m * p.ldc;
                T *lrow = p.C_lo ? (T *)p.C_lo + coffz + (int64_t)m * p.ldc : nullptr;
                typename Op<DT>::V4 h, l;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    h[r] = Op<DT>::from_f32(v[r]);
                    l[r] = Op<DT>::from_f32(v[r] - Op<DT>::to_f32(h[r]));
                }
                if (p.vec_ok && sfull) {
                    *(typename Op<DT>::V4 *)(crow + n0) = h;
                    if (lrow) *(typename Op<DT>::V4 *)(lrow + n0) = l;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (n0 + r < p.n_store) {
                            crow[n0 + r] = h[r];
                            if (lrow) lrow[n0 + r] = l[r];
                        }
                }
            }
        }
    }
#ifdef PIO_G128_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    G128_STAMP(124);
    if (stamp_on)
        for (int i = 0; i < 128; ++i) g128_stamps[i] = stamp_lds[i];
#endif
}

#ifdef PIO_G128_STAMPS
extern "C" int pio_debug_g128_stamps(unsigned long long *out128, int block) {
    if (out128 && hipMemcpyFromSymbol(out128, HIP_SYMBOL(g128_stamps), sizeof(g128_stamps)) != hipSuccess) return 1;
    if (block >= 0 && hipMemcpyToSymbol(HIP_SYMBOL(g128_block), &block, sizeof(int)) != hipSuccess) return 2;
    return 0;
}
#endif

// C[M, n_store <= NMAX] = A B^T for a handful of output columns (the flow decoder's final Linear: 182 528 x 328 -> 2; on
// a 128 x 128 tile 98 % of the MFMAs multiply padding: 234 us for a read of 240 MB).  No matrix pipe: a wave takes one row
// at a time, lane j the 16-byte chunk j of that row (of every K sweep's A image), multiplies it with the same chunk of the
// NMAX weight rows (LDS) in fp32, and the 64 lanes are summed by xor-shuffles.  Bound by the read of A.
template <int DT, int NMAX>
__global__ __launch_bounds__(256) void gemm_nt_skinny(const GemmParams p) {
    typedef typename Op<DT>::T T;
    typedef typename Op<DT>::V8 V8;
    extern __shared__ __attribute__((aligned(16))) char sk_smem[];   // [npass][NMAX][K] weight rows (zeros past N)
    T *const bs = (T *)sk_smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int K = p.K, cpr = K >> 3;   // 16-byte chunks per row (K % 8 == 0: launcher)
    for (int i = tid; i < p.npass * NMAX * cpr; i += 256) {
        const int pass = i / (NMAX * cpr), r = i - pass * NMAX * cpr;
        const int n = r / cpr, c = r - n * cpr;
        const int64_t dB = pass == 0 ? 0 : (pass == 1 ? p.dB1 : p.dB2);
        V8 w;
#pragma unroll
        for (int e = 0; e < 8; ++e) w[e] = Op<DT>::from_f32(0.f);
        if (n < p.N) w = *(const V8 *)((const T *)p.B + dB + (int64_t)n * p.ldb + c * 8);
        *(V8 *)(bs + ((int64_t)pass * NMAX + n) * K + c * 8) = w;
    }
    __syncthreads();
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (tid >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t m = wave0; m < p.M; m += nwaves) {
        float acc[NMAX];
#pragma unroll
        for (int n = 0; n < NMAX; ++n) acc[n] = 0.f;
        for (int c = lane; c < cpr; c += 64) {
            for (int pass = 0; pass < p.npass; ++pass) {
                const int64_t dA = pass == 0 ? 0 : (pass == 1 ? p.dA1 : p.dA2);
                const V8 a = *(const V8 *)((const T *)p.A + dA + m * p.lda + c * 8);
                if constexpr (DT == PIO_DT_F16) {
                    // v_dot2_f32_f16: two products and the sum in fp32 per instruction
                    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
#pragma unroll
                    for (int n = 0; n < NMAX; ++n) {
                        const V8 w = *(const V8 *)(bs + ((int64_t)pass * NMAX + n) * K + c * 8);
#pragma unroll
                        for (int e = 0; e < 8; e += 2)
                            acc[n] = __builtin_amdgcn_fdot2(h2{a[e], a[e + 1]}, h2{w[e], w[e + 1]}, acc[n], false);
                    }
                } else {
                    float af[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) af[e] = Op<DT>::to_f32(a[e]);
#pragma unroll
                    for (int n = 0; n < NMAX; ++n) {
                        const V8 w = *(const V8 *)(bs + ((int64_t)pass * NMAX + n) * K + c * 8);
#pragma unroll
                        for (int e = 0; e < 8; ++e) acc[n] = fmaf(af[e], Op<DT>::to_f32(w[e]), acc[n]);
                    }
                }
            }
        }
#pragma unroll
        for (int n = 0; n < NMAX; ++n)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc[n] += __shfl_xor(acc[n], o, 64);
        if (lane < p.n_store) {
            float x = 0.f;
#pragma unroll
            for (int n = 0; n < NMAX; ++n)
                if (n == lane) x = acc[n];
            x = x * p.alpha + ((p.bias_mode == 1 && lane < p.N) ? p.bias[lane] : 0.f);
            if (lane >= p.N) x = 0.f;   // columns [N, n_store) are written as zeros
            if (p.out_f32) ((float *)p.C)[m * p.ldc + lane] = x;
            else ((T *)p.C)[m * p.ldc + lane] = Op<DT>::from_f32(x);
        }
    }
}

// kernel selection override (pio_gemm_kernel_override; initial value from env PIO_GEMM_TILE)
static int &gemm_kernel_choice() {
    static int choice = [] {
        const char *e = getenv("PIO_GEMM_TILE");
        return e ? atoi(e) : 0;
    }();
    return choice;
}
int gemm_kernel_override(int which) {
    int &c = gemm_kernel_choice();
    const int prev = c;
    c = which;
    return prev;
}

// Dev aid: PIO_GEMM_LOG=1 prints one line per launch (shape, sweeps, epilogue form, kernel chosen) to stderr.
static bool gemm_log_on() {
    static const bool on = [] {
        const char *e = getenv("PIO_GEMM_LOG");
        return e && atoi(e) != 0;
    }();
    return on;
}
static void gemm_log(const char *kernel, const pio_gemm_t &g, const GemmParams &p) {
    if (!gemm_log_on()) return;
    fprintf(stderr, "pio_gemm %-10s M=%d N=%d K=%d batch=%d npass=%d act=%d out_f32=%d res=%d fold=%s n_store=%d\n", kernel, g.M,
            g.N, g.K, g.batch, p.npass, g.act, g.out_f32, (g.R || g.R16_hi) ? 1 : 0,
            g.ln_part ? "consumer" : (g.row_part ? "producer" : "-"), p.n_store);
}

// algorithmic bytes (profiler): operands once (every precision sweep reads its own image), the result in every form it
// leaves in (fp32 C if written, 16-bit C [+ C_lo], the LayerNorm fold's 16-bit pair X16 [+ X16_lo] and row sums), the
// residual in the form it arrives in (fp32 R or the 16-bit pair R16_hi + R16_lo), the consumer's row sums
static double gemm_algo_bytes(const pio_gemm_t &g) {
    const double elems = (double)g.batch * ((double)g.M * g.K + (double)g.N * g.K);
    const double mn = (double)g.batch * g.M * g.N;
    double algo_bytes = 2.0 * elems + (g.B_lo ? 2.0 * g.batch * (double)g.N * g.K : 0.0) +
                        (g.A_lo ? 2.0 * g.batch * (double)g.M * g.K : 0.0);
    if (g.out_f32) algo_bytes += g.C ? 4.0 * mn : 0.0;
    else algo_bytes += (g.C_lo ? 4.0 : 2.0) * mn;
    if (g.X16) algo_bytes += (g.X16_lo ? 4.0 : 2.0) * mn;
    if (g.row_part) algo_bytes += 8.0 * g.M * (double)(g.N / 128);
    if (g.R16_hi) algo_bytes += 4.0 * mn;
    else if (g.R) algo_bytes += 4.0 * mn;
    if (g.ln_part) algo_bytes += 64.0 * g.M;
    return algo_bytes;
}

template <int DT, int KIND>
static void gemm_tile_launch(GemmKernel k, dim3 grid, const GemmParams &p, hipStream_t s) {
    const dim3 block(256, 1, 1), block2(512, 1, 1);   // (two K teams: eight waves)
    switch (k) {
    case GemmKernel::T128_KG2: hipLaunchKernelGGL((gemm_nt_128<DT, KIND, 128, 128, 2, 2>), grid, block2, 0, s, p); break;
    case GemmKernel::T32_KG2: hipLaunchKernelGGL((gemm_nt_128<DT, KIND, 32, 64, 4, 2>), grid, block2, 0, s, p); break;
    case GemmKernel::T64_KG2: hipLaunchKernelGGL((gemm_nt_128<DT, KIND, 64, 64, 4, 2>), grid, block2, 0, s, p); break;
    case GemmKernel::T32: hipLaunchKernelGGL((gemm_nt_128<DT, KIND, 32, 64, 4>), grid, block, 0, s, p); break;
    case GemmKernel::T64: hipLaunchKernelGGL((gemm_nt_128<DT, KIND, 64, 64, 4>), grid, block, 0, s, p); break;
    default: hipLaunchKernelGGL((gemm_nt_128<DT, KIND, 128, 128, 2>), grid, block, 0, s, p); break;
    }
}

template <int DT>
static void gemm_skinny_launch(GemmKernel k, dim3 grid, const GemmParams &p, hipStream_t s) {
    const int nmax = k == GemmKernel::SKINNY2 ? 2 : 4;
    const size_t lds = (size_t)p.npass * nmax * p.K * 2;   // <= 48 KiB
    if (nmax == 2) hipLaunchKernelGGL((gemm_nt_skinny<DT, 2>), grid, dim3(256), lds, s, p);
    else hipLaunchKernelGGL((gemm_nt_skinny<DT, 4>), grid, dim3(256), lds, s, p);
}

int gemm_nt_launch(const pio_gemm_t &g, hipStream_t s) {
    GemmParams p;
    const int err = gemm_params(g, &p);
    if (err) return err;
    const int forced = gemm_kernel_choice();
    const GemmRoute r = gemm_route(g, p, forced, cu_budget());
    if (r.err) return r.err;
    p.tiles_n = r.tiles_n;
    gemm_log(r.label, g, p);

    const bool attn = g.batch > 1, f16 = g.dtype == PIO_DT_F16;
    int cls = attn ? PROF_GEMM_ATTN : PROF_GEMM_SMALL;   // kernel gemm_nt_128 / gemm_nt_skinny
    if (r.kernel == GemmKernel::WIDE) cls = PROF_GEMM_WIDE;
    if (r.kernel == GemmKernel::STREAM) cls = PROF_GEMM_STREAM;
    if (r.kernel == GemmKernel::T256) cls = PROF_GEMM_LINEAR;
#ifdef PIO_EXPERIMENTS
    if (r.kernel == GemmKernel::DUO) cls = PROF_GEMM_WIDE;
#endif
    ProfScope prof(cls, 2.0 * g.M * g.N * (double)g.K * g.batch, gemm_algo_bytes(g), s);
    const dim3 grid(r.grid_x, r.grid_y, 1);
    switch (r.kernel) {
    case GemmKernel::SKINNY2:
    case GemmKernel::SKINNY4:
        if (f16) gemm_skinny_launch<PIO_DT_F16>(r.kernel, grid, p, s);
        else gemm_skinny_launch<PIO_DT_BF16>(r.kernel, grid, p, s);
        break;
    case GemmKernel::WIDE: gemm_wide_launch(p, g.dtype, (int)r.grid_x, s); break;
    case GemmKernel::STREAM: gemm_stream_launch(p, g.dtype, g.batch, (int)r.grid_x, s); break;
    case GemmKernel::T256: gemm256_launch(p, g.dtype, attn, grid, s); break;
#ifdef PIO_EXPERIMENTS
    case GemmKernel::DUO: gemm_duo_launch(p, g.dtype, s); break;
#endif
    default:
        if (f16 && attn) gemm_tile_launch<PIO_DT_F16, 1>(r.kernel, grid, p, s);
        else if (f16) gemm_tile_launch<PIO_DT_F16, 0>(r.kernel, grid, p, s);
        else if (attn) gemm_tile_launch<PIO_DT_BF16, 1>(r.kernel, grid, p, s);
        else gemm_tile_launch<PIO_DT_BF16, 0>(r.kernel, grid, p, s);
        break;
    }
    return launch_status();
}

}  // namespace pio
