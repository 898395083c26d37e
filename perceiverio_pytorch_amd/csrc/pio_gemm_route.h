// GEMM routing (host only, plain C++17: no HIP, no environment, no state): pio_gemm_t -> GemmParams (gemm_params), the
// legality of the persistent kernels (gemm_wide_ok / gemm_stream_ok), and which kernel / tile a launch goes to
// (gemm_route).  pio_gemm.hip launches what gemm_route returns; tests/test_gemm_route.py checks it on the CPU.
#pragma once
#include <stdint.h>

#include "../../include/pio_hip.h"

namespace pio {

constexpr int BM = 128, BN = 128;                        // gemm_nt_128: the default tile (pio_gemm.hip)
constexpr int W_BM = 256, W_BN = 256, W_BK = 32;         // gemm_nt_wide (pio_gemm_wide.hip)
constexpr int S_BM = 256, S_BN = 128, S_BK = 64;         // gemm_nt_stream (pio_gemm_stream.hip)
constexpr int S_TAB_N = 256;  // gemm_nt_stream: tile-table entries (32 B each), this workgroup's tile list, decoded once

struct GemmParams {
    const void *A, *B;
    int64_t dA1, dB1, dA2, dB2;  // element offsets of the pass-1 / pass-2 operands relative to A / B
    int npass;                   // 1..3 K sweeps accumulating into the same registers
    int staged_epi;              // (gemm_nt_wide, LayerNorm-fold producer) 1: LDS-staged, row-coalesced epilogue
    int reserved0;               // nothing reads it: keeps the kernel-argument offsets; goes with the next real change here
    int lo_n0;                   // (gemm_nt_wide only) B_lo exists for columns >= lo_n0 (multiple of 256); 0 = all
    int k_rev;                   // (gemm_nt_wide only) odd tiles of a workgroup sweep K backwards (see its walk)
    void *C, *C_lo;
    int M, N, K;
    int64_t lda, ldb, ldc;
    int nh;
    int64_t sAb, sAh, sBb, sBh, sCb, sCh;
    const float *bias;
    int bias_mode, act;
    float alpha;
    const float *R;
    int64_t ldr, r_stride_b;
    int r_rows;
    int out_f32, n_store;
    int tiles_n;
    int vec_ok;    // C rows are 16-byte (fp32) / 8-byte (16-bit) aligned for 4-column vectors
    int r_vec;     // residual rows are 16-byte aligned
    int bias_vec;  // bias is 16-byte aligned
    // LayerNorm fold (gemm_nt_wide only): producer outputs / consumer inputs, see pio_gemm_t
    void *X16;
    int64_t ld16;
    float *row_part;
    const float *ln_part, *ln_c;
    float ln_eps;
    void *X16_lo;
    const void *R16_hi, *R16_lo;
    int *range_flag;  // producer: set to 1 when a row statistic is not finite (the folded stack's fp16 range guard)
    // consumer: ln_part holds ln_slots (sum, sum of squares) pairs per row (K / 128 from the wide kernel's producer, K / 64
    // from the small-tile kernels'), ln_inv_k = 1 / K; producer: slot_w = columns per slot (128 wide kernel, 64 small tiles)
    int ln_slots;
    float ln_inv_k;
    int slot_w;
};

// Validates the descriptor and fills p (PIO_OK or the first PIO_E_* code that applies).
inline int gemm_params(const pio_gemm_t &g, GemmParams *pp) {
    if (!g.A || !g.B) return PIO_E_ARG;
    if (!g.C && !(g.X16 && g.X16_lo && g.out_f32)) return PIO_E_ARG;  // (fp32 C is optional beside a 16-bit pair)
    if (g.M <= 0 || g.N <= 0 || g.K <= 0 || g.batch <= 0 || g.nh <= 0) return PIO_E_SHAPE;
    if (g.K % 8) return PIO_E_SHAPE;
    if (g.batch % g.nh) return PIO_E_SHAPE;
    if ((g.lda % 8) || (g.ldb % 8) || (g.sAb % 8) || (g.sAh % 8) || (g.sBb % 8) || (g.sBh % 8)) return PIO_E_ALIGN;
    if (((uintptr_t)g.A & 15) || ((uintptr_t)g.B & 15) || ((uintptr_t)g.A_lo & 15) || ((uintptr_t)g.B_lo & 15) ||
        ((uintptr_t)g.C_lo & 7))
        return PIO_E_ALIGN;
    if (g.batch > 65535) return PIO_E_SHAPE;
    if (g.bias_mode && !g.bias) return PIO_E_ARG;
    if (g.dtype != PIO_DT_F16 && g.dtype != PIO_DT_BF16) return PIO_E_ARG;

    GemmParams &p = *pp;
    p = GemmParams{};
    p.A = g.A; p.B = g.B; p.C = g.C;
    p.C_lo = g.out_f32 ? nullptr : g.C_lo;
    // K sweeps: (A,B) [+ (A,B_lo)] [+ (A_lo,B)]  -- the dropped A_lo*B_lo term is ~2^-22 relative
    p.npass = 1;
    auto delta = [](const void *lo, const void *hi) { return (int64_t)(((intptr_t)lo - (intptr_t)hi) / 2); };
    if (g.B_lo) { p.dB1 = delta(g.B_lo, g.B); p.npass = 2; }
    if (g.A_lo) {
        if (p.npass == 1) { p.dA1 = delta(g.A_lo, g.A); p.npass = 2; }
        else              { p.dA2 = delta(g.A_lo, g.A); p.npass = 3; }
    }
    p.M = g.M; p.N = g.N; p.K = g.K;
    p.lda = g.lda; p.ldb = g.ldb; p.ldc = g.ldc;
    p.nh = g.nh;
    p.sAb = g.sAb; p.sAh = g.sAh; p.sBb = g.sBb; p.sBh = g.sBh; p.sCb = g.sCb; p.sCh = g.sCh;
    p.bias = g.bias; p.bias_mode = g.bias_mode; p.act = g.act; p.alpha = g.alpha;
    p.R = g.R; p.ldr = g.ldr; p.r_stride_b = g.r_stride_b; p.r_rows = g.r_rows_per_batch;
    // a residual whose batches are contiguous ([B, T, C] with stride_b == T * ld) is one flat [B*T, C] matrix
    if (p.R && p.r_rows > 0 && p.r_stride_b == (int64_t)p.r_rows * p.ldr) p.r_rows = 0;
    p.out_f32 = g.out_f32;
    p.X16 = g.X16; p.ld16 = g.ld16; p.row_part = g.row_part;
    p.ln_part = g.ln_part; p.ln_c = g.ln_c; p.ln_eps = g.ln_eps;
    p.X16_lo = g.X16_lo; p.R16_hi = g.R16_hi; p.R16_lo = g.R16_lo;
    p.range_flag = g.row_part ? g.range_flag : nullptr;
    p.lo_n0 = g.B_lo ? g.b_lo_n0 : 0;
    p.k_rev = 0;        // (gemm_nt_wide: K walked forwards on every tile)
    p.staged_epi = 1;   // (gemm_nt_wide: the fold producer's staged epilogue)
    p.ln_slots = g.ln_part ? (g.ln_slots > 0 ? g.ln_slots : g.K / 128) : 0;
    p.ln_inv_k = 1.0f / (float)g.K;
    p.slot_w = g.row_part ? (g.row_slot_w > 0 ? g.row_slot_w : 128) : 0;
    if (g.b_lo_n0 && (!g.B_lo || g.A_lo)) return PIO_E_ARG;
    p.n_store = g.n_store > g.N ? g.n_store : g.N;
    if (g.C && p.n_store > g.ldc) return PIO_E_SHAPE;
    p.tiles_n = (p.n_store + BN - 1) / BN;
    const size_t esz = g.out_f32 ? 4 : 2;
    const size_t valign = g.out_f32 ? 16 : 8;
    const bool vec = (((uintptr_t)g.C) % valign == 0) && ((g.ldc * esz) % valign == 0) && ((g.sCb * esz) % valign == 0) &&
                     ((g.sCh * esz) % valign == 0);
    p.vec_ok = vec ? 1 : 0;
    p.r_vec = (g.R && ((uintptr_t)g.R % 16 == 0) && (g.ldr % 4 == 0) && (g.r_stride_b % 4 == 0)) ? 1 : 0;
    p.bias_vec = (g.bias && ((uintptr_t)g.bias % 16 == 0)) ? 1 : 0;
    return PIO_OK;
}

// Epilogue forms the routing and the launchers both ask about.
// An fp32 residual with the hi + lo pair of a 16-bit result (the dense decoders' fc2).
inline bool gemm_pair_res(const GemmParams &p) { return p.R && !p.out_f32 && p.C_lo; }
// Either half of the LayerNorm fold.
inline bool gemm_fold(const GemmParams &p) {
    return p.X16 || p.row_part || p.ln_part || p.ln_c || p.X16_lo || p.R16_hi || p.R16_lo;
}
// Workgroups of a persistent kernel: one per CU, a multiple of 8 (the XCD count) when possible.
inline int persistent_grid(int64_t tiles, int n_cu) {
    int G = (int)(tiles < n_cu ? tiles : n_cu);
    if (G >= 8) G &= ~7;
    return G;
}

// gemm_nt_wide (persistent 256x256 four-wave kernel) takes p.
inline bool gemm_wide_ok(const GemmParams &p, int batch) {
    if (batch != 1 || p.npass > 3) return false;
    // a second sweep against B_lo only (weights as hi + lo, single activations) may start at a 256-aligned column; the
    // sweeps with an A_lo image (split activations: dA1 or dA2) cover every column
    const bool b_lo_only = p.npass == 2 && p.dA1 == 0;
    // (the fold forms run the two-way sweep code: B_lo only)
    if (!b_lo_only && p.npass > 1 && (p.ln_part || p.ln_c || p.R16_hi || p.R16_lo || (p.row_part && !p.R))) return false;
    if (b_lo_only && (p.dB1 == 0 || p.lo_n0 < 0 || (p.lo_n0 % W_BN))) return false;
    if (!b_lo_only && p.lo_n0 != 0) return false;
    if (p.K < 4 * W_BK || (p.K % (2 * W_BK))) return false;
    if (p.act != 0 && p.act != 1) return false;
    // the hi + lo pair of the result: the plain 16-bit epilogue only (not the fold forms, not fp32 out)
    if (p.C_lo && (p.out_f32 || p.ln_part || p.row_part || p.X16 || ((uintptr_t)p.C_lo & 15))) return false;
    if (p.out_f32 && (p.act != 0 || (p.C && (p.ldc & 3)))) return false;
    // an fp32 residual: with an fp32 result, or -- the dense decoders' fc2 -- with the hi + lo pair of the result (the
    // fold producer's epilogue without its statistics: gemm_wide_launch maps C / C_lo onto X16 / X16_lo)
    const bool pair_res = gemm_pair_res(p) && p.C && p.act == 0 && !p.X16 && !p.row_part && !p.ln_part;
    if (p.R && ((!p.out_f32 && !pair_res) || !p.r_vec || p.r_rows != 0 || (p.ldr & 3))) return false;
    if (pair_res && (((uintptr_t)p.C & 15) || ((uintptr_t)p.C_lo & 15) || (p.ldc & 7))) return false;
    if (p.X16 || p.row_part || p.X16_lo || p.R16_hi || p.R16_lo) {  // LayerNorm-fold producer
        const bool pair_r = p.R16_hi || p.R16_lo;
        if (!p.X16 || !p.row_part || !p.out_f32 || (p.N & 127) || p.slot_w != 128 || (p.ld16 & 7) || ((uintptr_t)p.X16 & 15) ||
            ((uintptr_t)p.row_part & 7) || p.ln_part || p.ln_c)
            return false;
        if (pair_r ? (!p.R16_hi || !p.R16_lo || p.R || ((uintptr_t)p.R16_hi & 15) || ((uintptr_t)p.R16_lo & 15)) : !p.R)
            return false;
        if (((uintptr_t)p.X16_lo & 15) || (!p.C && !p.X16_lo)) return false;
    }
    if (p.ln_part || p.ln_c) {  // LayerNorm-fold consumer
        if (!p.ln_part || !p.ln_c || p.out_f32 || (p.K & 127) || p.K > 1536 || p.ln_slots != p.K / 128 ||
            (p.ln_slots & 1) || p.alpha != 1.0f || ((uintptr_t)p.ln_c & 15) || ((uintptr_t)p.ln_part & 15))
            return false;
    }
    if (p.bias_mode > 1 || (p.bias_mode == 1 && !p.bias_vec)) return false;
    if ((p.N & 7) || (p.n_store & 7) || (p.C && ((p.ldc & 7) || ((uintptr_t)p.C & 15)))) return false;
    if ((p.lda & 7) || (p.ldb & 7) || ((uintptr_t)p.A & 15) || ((uintptr_t)p.B & 15)) return false;
    if (((int64_t)p.M * p.lda + p.K) * 2 >= (1ll << 32) || ((int64_t)p.N * p.ldb + p.K) * 2 >= (1ll << 32)) return false;
    return true;
}

// gemm_nt_stream (persistent 256x128 streaming kernel) takes p on n_cu CUs.
inline bool gemm_stream_ok(const GemmParams &p, int batch, int n_cu) {
    const int nk = p.npass * ((p.K + S_BK - 1) / S_BK);
    if (nk < 16 || (p.K % S_BK)) return false;
    if (p.bias_mode > 1 || (p.bias_mode == 1 && !p.bias_vec)) return false;
    if ((p.N & 3) || (p.n_store & 3) || !p.vec_ok) return false;
    if (p.act != 0 && p.act != 1) return false;
    if (p.alpha == 0.0f) return false;
    // (a residual with a 16-bit result -- the decoder's fc2 leaving y as the operand of the final Linear -- rides the same
    //  way: the residual is loaded into the vacated accumulators, the output form is the epilogue's business)
    if (p.R && (!p.r_vec || p.alpha != 1.0f || p.act != 0 || p.r_rows != 0)) return false;
    // (... as ONE 16-bit array: the hi + lo pair form of that variant spills 11 registers, which the counted waits of this
    //  kernel cannot carry -- those launches go to gemm_nt_256)
    if (gemm_pair_res(p)) return false;
    if (p.out_f32 && p.act != 0) return false;
    if (p.out_f32 && p.C_lo) return false;
    // per-lane DMA offsets are 32-bit byte offsets inside one (batch, head) slice
    if (((int64_t)p.M * p.lda + p.K) * 2 >= (1ll << 32) || ((int64_t)p.N * p.ldb + p.K) * 2 >= (1ll << 32)) return false;
    // the per-workgroup tile list is decoded into an LDS table of S_TAB_N entries
    const int64_t tiles = (int64_t)((p.M + S_BM - 1) / S_BM) * ((p.n_store + S_BN - 1) / S_BN) * batch;
    const int G = persistent_grid(tiles, n_cu);
    if ((tiles + G - 1) / G + 8 > S_TAB_N) return false;
    return true;
}

// The fold on the small tiles (a stack too short for 256 x 256 tiles): chosen by the caller through the slot form -- a
// producer asked for 64-column slots, a consumer given anything but K / 128 slots (or a shape the wide kernel does not
// take).
inline bool gemm_fold_small(const GemmParams &p, int batch) {
    return gemm_fold(p) &&
           (p.row_part ? p.slot_w == 64 : (p.ln_slots != p.K / 128 || p.M < 2048 || !gemm_wide_ok(p, batch)));
}

#ifdef PIO_EXPERIMENTS
// the LayerNorm fold's producer with two 128x256-tile workgroups per CU (tools/experiments/pio_gemm_duo.hip)
bool gemm_duo_ok(const GemmParams &p, int batch);
#endif

enum class GemmKernel {
    NONE,      // (an error)
    SKINNY2,   // gemm_nt_skinny<., 2>: up to two output columns
    SKINNY4,   // gemm_nt_skinny<., 4>
    WIDE,      // gemm_nt_wide: persistent 256x256, four waves
    STREAM,    // gemm_nt_stream: persistent 256x128, epilogue behind the next tile's MFMAs
    T256,      // gemm_nt_256: 256x256 tiles
    T128,      // gemm_nt_128 on 128x128 tiles, double buffer
    T128_KG2,  // ... two K teams
    T64,       // gemm_nt_128 on 64x64 tiles, four-stage ring
    T64_KG2,
    T32,       // gemm_nt_128 on 32x64 tiles, four-stage ring
    T32_KG2,
#ifdef PIO_EXPERIMENTS
    DUO,       // (experiments build) gemm_nt_duo, override 3
#endif
};

struct GemmRoute {
    int err;                  // PIO_OK, or the PIO_E_* code of a descriptor no kernel takes
    GemmKernel kernel;
    unsigned grid_x, grid_y;  // workgroups (the persistent kernels: grid_x only)
    int tiles_n;              // GemmParams.tiles_n of the launch (tile columns of the tile kernels)
    const char *label;        // the kernel's name in the PIO_GEMM_LOG lines
};

// Which kernel takes (g, p): `forced` is the pio_gemm_kernel_override value (0 = automatic), n_cu the CUs a persistent
// kernel sizes its grid for.
inline GemmRoute gemm_route(const pio_gemm_t &g, const GemmParams &p, int forced, int n_cu) {
    auto route = [&](GemmKernel k, const char *label, int64_t gx, int64_t gy = 1, int tiles_n = -1) {
        return GemmRoute{PIO_OK, k, (unsigned)gx, (unsigned)gy, tiles_n >= 0 ? tiles_n : p.tiles_n, label};
    };
    const GemmRoute refuse = {PIO_E_SHAPE, GemmKernel::NONE, 0, 0, 0, nullptr};

    // A handful of output columns over many rows: no tile kernel (see gemm_nt_skinny).
    // (up to four columns: 182 528 x 328 -> 2 with split activations 42 us against 70 on the 128 x 128 tile; at eight
    //  columns x K = 1032 the fp32 FMAs of this kernel cost more than the tile's padding: 190 against 125 us)
    const bool plain = !gemm_fold(p) && !p.R && !p.C_lo && g.act == 0 && g.bias_mode <= 1 && !g.b_lo_n0 && g.C;
    if (forced == 0 && plain && g.batch == 1 && p.n_store <= 4 && g.M >= 2048 && g.K <= 2048 && p.n_store <= g.ldc)
        return route(p.n_store <= 2 ? GemmKernel::SKINNY2 : GemmKernel::SKINNY4, "skinny",
                     g.M / 4 < 256 * 8 ? (g.M + 3) / 4 : 256 * 8);

    const int tn256 = (p.n_store + 255) / 256, tm256 = (g.M + 255) / 256;
    const int64_t t256 = (int64_t)tm256 * tn256;
    const bool fold = gemm_fold(p), fold_small = gemm_fold_small(p, g.batch);

    // Persistent 256x256 four-wave kernel (pio_gemm_wide.hip): 16-bit-out projections (bias, optional GELU) with at least
    // one tile per CU.  Its epilogue is exposed, but it is bound by the stores, which the caches absorb at ~7 TB/s, and
    // the GELU arithmetic hides behind them: 16384x1024x1024 takes 36 us (GELU: 42) against 42 (48) on the streaming
    // kernel.  Override 2 forces it wherever it is legal.
    // (With a residual the kernel is legal but not chosen: the 64 MB residual read of a 16384x1024 launch is exposed in
    //  its epilogue -- 49 us against 39 without -- where the streaming kernel hides most of it.)
    // (from 128 tiles on: below one tile per CU the four-wave kernel still beats gemm_nt_256 tile for tile -- the
    //  language model's 8192 x 1280 projections have 160 -- and with fewer than two 256x128 tiles per CU the streaming
    //  kernel has nothing to hide a residual epilogue behind, so those come here too)
    // (a residual with the hi + lo pair of the result -- the dense decoders' fc2 -- has no streaming variant: here rather
    //  than on gemm_nt_256; multimodal forward 23.23 -> 22.00 ms, in-process A/B)
    // (N = 384 = 1.5 tile columns: a third of the MFMAs multiply padding and the kernel still beats the 128 x 128 tile's
    //  exact three columns -- 182 528 x 384 x 384, split activations, GELU, pair out: 204 against 291 us)
    const bool fill_ok = (double)tn256 * 256.0 <= 1.25 * p.n_store ||
                         (p.n_store >= 384 && (double)tn256 * 256.0 <= 1.34 * p.n_store);
    bool wide = g.batch == 1 && g.M >= 2048 && fill_ok && t256 >= 128 && (!p.R || 2 * t256 < 448 || gemm_pair_res(p));
    if (forced == 2) wide = true;
    if (forced == 1 || forced == 128 || forced == 256) wide = false;
    if (fold_small) {
        if (g.batch != 1 || p.npass != 1 || p.lo_n0 || g.bias_mode > 1) return refuse;
        if (p.row_part) {  // producer
            if (!p.X16 || !p.X16_lo || !p.R16_hi || !p.R16_lo || !g.out_f32 || p.R || (g.N & 63) || p.n_store != g.N ||
                (p.ld16 & 3) || ((uintptr_t)p.X16 & 7) || ((uintptr_t)p.X16_lo & 7) || ((uintptr_t)p.R16_hi & 7) ||
                ((uintptr_t)p.R16_lo & 7) || p.ln_part || g.act != 0 || (g.C && ((g.ldc & 3) || ((uintptr_t)g.C & 15))))
                return refuse;
        } else {           // consumer
            if (!p.ln_part || !p.ln_c || g.out_f32 || g.alpha != 1.0f || p.ln_slots <= 0) return refuse;
        }
        wide = false;
    } else if (fold) {
#ifdef PIO_EXPERIMENTS
        if (forced == 3 && gemm_duo_ok(p, g.batch)) return route(GemmKernel::DUO, "duo", 0);
#endif
        if (!gemm_wide_ok(p, g.batch)) return refuse;
        wide = true;
    }
    if (wide && gemm_wide_ok(p, g.batch))
        return route(GemmKernel::WIDE, "wide", persistent_grid((int64_t)((g.M + W_BM - 1) / W_BM) * tn256, n_cu));
    if (p.lo_n0) return refuse;  // (a partial B_lo is a gemm_nt_wide feature)

    // Persistent 256x128 streaming kernel (epilogue of tile j hidden behind the MFMAs of tile j+1): deep-K flat problems
    // with about two or more tiles per CU (with fewer there is nothing to hide an epilogue behind and the 256x256 tile's
    // lower operand traffic wins).  Override 1 forces it wherever it is legal.
    const int tn128 = (p.n_store + 127) / 128;
    bool stream = !fold_small && g.batch == 1 && g.M >= 1024 && p.n_store >= 128 &&
                  (double)tn128 * 128.0 <= 1.25 * p.n_store && (int64_t)tm256 * tn128 >= 448;
    if (forced == 1 && !fold_small) stream = true;   // (never a fold: the streaming kernel has no fold epilogue)
    if (forced == 128 || forced == 256) stream = false;
    if (stream && gemm_stream_ok(p, g.batch, n_cu))
        return route(GemmKernel::STREAM, "stream",
                     persistent_grid((int64_t)((g.M + S_BM - 1) / S_BM) * tn128 * g.batch, n_cu));

    // Large problems go to the 256x256-tile / 4-slot-ring kernel: enough rows, and an N that fills whole 256-column tiles
    // reasonably (<= 25 % padding).  Overrides 128 / 256 force the 128 / 256 tile.
    bool big = g.batch == 1 && g.M >= 1024 && p.n_store >= 256 && (double)tn256 * 256.0 <= 1.25 * p.n_store && t256 >= 128;
    if (forced == 128) big = false;
    if (forced == 256) big = true;
    if (big && !fold_small) return route(GemmKernel::T256, "t256", t256, g.batch, tn256);

    // gemm_nt_128.  64 x 64 tiles when the 128 x 128 tiling would leave most CUs without a tile (small batches: the
    // 2048-row latent stack of the flow model at B = 1 has 64 tiles of 128 x 128 per GEMM, 256 of 64 x 64); override 64
    // forces them ...
    const int64_t tiles128 = (int64_t)((g.M + BM - 1) / BM) * p.tiles_n * g.batch;
    // ... and up to ONE 128 x 128 tile per CU (the double buffer then has no second workgroup to hide its waits behind)
    // when the 64 x 64 tiling fills whole rounds of the chip's 512 resident workgroups or K is short: same box, ms per
    // forward (tools/latency_probe.py / ab_env.py): ImageNet B = 8 (4096 x 1024 x 1024 projections: 256 -> 1024 tiles)
    // 7.63 -> 7.27, flow (q|k|v 2048 x 1536 x 512: 192 -> 768 tiles) 5.31 -> 5.24; NOT the B = 2 q|k|v (1024 x 3072 x
    // 1024: 192 -> 768 tiles = 1.5 rounds of 16 K steps): 4.11 -> 4.18.
    const int64_t tiles64 = (int64_t)((g.M + 63) / 64) * ((p.n_store + 63) / 64) * g.batch;
    const bool one_round = tiles128 <= n_cu && (g.K <= 512 || tiles64 % (2 * (int64_t)n_cu) == 0);
    const bool small = forced == 64 || (forced == 0 && (tiles128 < 192 || one_round));
    // ... and 32 x 64 tiles when even the 64 x 64 tiling leaves a third of the CUs without one (ImageNet B = 1: the
    // 512 x 1024 projections have 128 tiles of 64 x 64, 256 of 32 x 64)
    const bool tiny = small && forced == 0 && 3 * tiles64 < 2 * (int64_t)n_cu;
    const int tiles_n = small ? (p.n_store + 63) / 64 : p.tiles_n;
    const int64_t grid_x = small ? (int64_t)((g.M + (tiny ? 31 : 63)) / (tiny ? 32 : 64)) * tiles_n
                                 : (int64_t)((g.M + BM - 1) / BM) * tiles_n;
    // Two K teams (eight waves) for tiles that own their CU alone (see the kernel), from K = 1024 on: the flow stack's
    // 2048 x 512 x 512 projections -- four steps a team -- lose 2 % of a forward to it, ImageNet B = 1 gains 5.6 %
    // (tools/ab_env.py); on the 128 x 128 tile ImageNet B = 2 (the 1024 x 3072 x 1024 q|k|v GEMM has 192 tiles): forward
    // 4.62 -> 4.46 ms.
    const bool kg2 = forced == 0 && p.npass * g.K >= 1024 && grid_x * g.batch <= (int64_t)n_cu;
    const char *label = tiny ? "t32" : small ? "t64" : "t128";
    GemmKernel k = tiny    ? (kg2 ? GemmKernel::T32_KG2 : GemmKernel::T32)
                   : small ? (kg2 ? GemmKernel::T64_KG2 : GemmKernel::T64)
                           : (kg2 ? GemmKernel::T128_KG2 : GemmKernel::T128);
    return route(k, label, grid_x, g.batch, tiles_n);
}

}  // namespace pio
