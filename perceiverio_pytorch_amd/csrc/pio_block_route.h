// Block composition (host only, plain C++17: no HIP, no environment, no state): the workspace layout of every block
// entry point (the *Plan structs), whether and on which kernel family a SelfAttention block runs with its LayerNorms
// folded into the GEMMs around them (self_fold_route), whether a decoder's fc2 writes the final Linear's 16-bit operand
// itself (decoder_y16_direct), and the GEMM descriptor of one nn.Linear in each form a block asks for (linear_gemm).
// pio_blocks.hip reads the switches and launches what these return; the plans only add offsets to the caller's base
// pointer, nothing here reads through one.  tests/test_block_route.py checks them on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/pio_hip.h"
#include "pio_attn_route.h"

namespace pio {

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
inline int pad8(int c) { return (c + 7) & ~7; }
// Pitch (elements) of a CHANNEL axis in the 16-bit operand arrays = the K of the GEMM that reads them: a multiple of 8
// (one 16-byte DMA piece); from 256 channels on a multiple of 64, which the staged kernels (gemm_nt_wide / _stream:
// whole 64-deep K slices) require -- the multimodal decoder's 1026-channel queries run on 1088 (+5 % K) and its
// GEMMs 15-25 % faster for it (tools/mm_dec_gemm_bench.py); the flow decoder's 322 channels on 384 (round 4: its
// 182 528-row projections then run on gemm_nt_wide, 20-30 % faster: DESIGN_LOG R4.15).  Head dims and key counts keep pad8.
inline int padc(int c) { return c >= 256 ? (c + 63) & ~63 : (c + 7) & ~7; }
// Row pitch (floats) of an INTERNAL fp32 activation buffer: whole float4 groups, so that a channel count like 1026 or
// 322 does not force the GEMM epilogues and LayerNorm reads onto 4-byte accesses.  The columns [C, pitch4(C)) hold
// zeros or stale values and are never read as data.
inline int pitch4(int c) { return (c + 3) & ~3; }
// Row pitch (floats) of x1, the cross-attend's fp32 result: the residual of fc2, which as the decoders' 16-bit y computes
// all pad8(C) columns of its packed image and reads that many residual columns.  The out projection writes the columns
// [C, pitch8(C)) as zeros in every call (n_store), so nothing there depends on what the workspace held.
inline int pitch8(int c) { return (c + 7) & ~7; }

// carve helper for caller-provided workspaces (256-byte aligned pieces)
struct Carver {
    char *base;
    size_t off;
    explicit Carver(void *p) : base((char *)p), off(0) {}
    void *take(size_t bytes) {
        void *r = base ? base + off : nullptr;
        off += (size_t)round_up((int64_t)bytes, 256);
        return r;
    }
};

struct Pair {  // a 16-bit operand and its optional rounding residual
    void *hi = nullptr, *lo = nullptr;
};

inline Pair take_pair(Carver &c, size_t elems, bool split) {
    Pair p;
    p.hi = c.take(elems * 2);
    p.lo = split ? c.take(elems * 2) : nullptr;
    return p;
}

// Upper bound of the materialised score matrix held at once (fp32 scores + 16-bit probabilities are carved for this many
// (batch, row) slabs): attention over more than this is run sample by sample and, inside a sample, in chunks of query
// rows.  Only the 3-sweep policies ("x3": split activations) still materialise scores for the wide cross-attends; the
// optical-flow ones (2048 x 182 528 scores: 1.5 GB fp32 + as much again for the probability pair) then run in two
// passes of <= 1 GiB.  (A 256 MiB cap was measured too: 8 passes, each P V product with only 6 output tiles of a
// 182 528-deep K loop -- 96 ms instead of 29 per forward.)
constexpr int64_t kScoreCapBytes = 1ll << 30;

struct ScoreChunks {
    int b_chunk;  // samples per pass (>= 1)
    int q_chunk;  // query rows per pass (== Tq unless b_chunk == 1 and one sample exceeds the cap)
};
inline ScoreChunks score_chunks(int B, int H, int Tq, int Tk) {
    const int64_t per_sample = (int64_t)H * Tq * (int64_t)Tk * 4;
    ScoreChunks c{B, Tq};
    if ((int64_t)B * per_sample <= kScoreCapBytes) return c;
    int64_t bc = kScoreCapBytes / (per_sample > 0 ? per_sample : 1);
    if (bc >= 1) {
        c.b_chunk = (int)bc;
        return c;
    }
    c.b_chunk = 1;
    int64_t qc = kScoreCapBytes / ((int64_t)H * Tk * 4);
    qc = qc / 128 * 128;
    c.q_chunk = (int)(qc < 128 ? 128 : qc);
    if (c.q_chunk > Tq) c.q_chunk = Tq;
    return c;
}

// ======================================================================================================
// plans (workspace layouts)
// ======================================================================================================
struct AttnScratch {
    Pair q16, k16, vt16, p16, o16;
    float *scores;
    void *xpart;  // key bits / fp32 split partials of the fused cross-attention cores
    // lean: the caller never passes a full mask / bias / probability output: no score buffers where attn_plan has a fused core
    // masked: ... but may pass key / query mask vectors (a cross-attend)
    void carve(Carver &c, const pio_attention_t &a, int Bq, int B, int Tq, int Tk, bool lean = false, bool masked = false) {
        const int64_t ldq = (int64_t)a.heads * a.dkp, ldo = (int64_t)a.heads * a.dvp, tkp = pad8(Tk);
        const int64_t tkv = round_up(Tk, 32);  // V^T row pitch: whole 32-key tiles, zero padded (pio_xattn.hip)
        const bool sp = a.act_split != 0;
        const AttnRoute plan = attn_plan(a, B, Bq, Tq, Tk, lean, masked);
        q16 = take_pair(c, (size_t)Bq * Tq * ldq, sp);
        // (the fused cross-attention kernel reads whole 32-key tiles: up to 31 rows behind key Tk - 1 of the last
        //  sample.  They only have to be readable -- their scores are masked by assignment -- and they are: vt16 and
        //  o16 follow in the same workspace.  No padding here: the fused q|k|v form needs q16 | k16 | vt16 adjacent.)
        k16 = take_pair(c, (size_t)B * Tk * ldq, sp);
        vt16 = take_pair(c, (size_t)B * ldo * tkv, sp);
        scores = nullptr;
        p16 = Pair();
        if (plan.need_scores) {
            const ScoreChunks ch = score_chunks(B, a.heads, Tq, Tk);
            scores = (float *)c.take((size_t)ch.b_chunk * a.heads * ch.q_chunk * (int64_t)Tk * 4);
            p16 = take_pair(c, (size_t)ch.b_chunk * a.heads * ch.q_chunk * tkp, sp);
        }
        o16 = take_pair(c, (size_t)B * Tq * ldo, sp);
        xpart = plan.xpart_bytes ? c.take(plan.xpart_bytes) : nullptr;
    }
};

struct AttentionPlan {
    Pair xq16, xk16, xv16;
    AttnScratch core;
    size_t carve(void *base, const pio_attention_t &a, int B, int Tq, int Tk, bool qb, bool same) {
        Carver c(base);
        const bool sp = a.act_split != 0;
        const int Bq = qb ? 1 : B;
        xq16 = take_pair(c, (size_t)Bq * Tq * padc(a.q_in), sp);
        xk16 = take_pair(c, (size_t)B * Tk * padc(a.k_in), sp);
        xv16 = same ? xk16 : take_pair(c, (size_t)B * Tk * padc(a.v_in), sp);
        core.carve(c, a, Bq, B, Tq, Tk);
        return c.off;
    }
};

struct MlpPlan {
    Pair x16, h16;
    size_t carve(void *base, const pio_mlp_t &m, int64_t rows) {
        Carver c(base);
        x16 = take_pair(c, (size_t)rows * padc(m.in), m.act_split != 0);
        h16 = take_pair(c, (size_t)rows * padc(m.hidden), m.act_split != 0);
        return c.off;
    }
};

struct SelfPlan {
    Pair x16, h16;
    float *x1;
    AttnScratch core;
    // LayerNorm fold (pio_ln_fold_t): 16-bit copy of x1 and the per-row partial sums of x (A) and x1 (B); the 16-bit
    // copy of x lives in x16
    void *x16b = nullptr, *lo_a = nullptr, *lo_b = nullptr;  // lo_*: x - x16 / x1 - x16b (the stream as a 16-bit pair)
    float *part_a = nullptr, *part_b = nullptr;
    // lean: the caller never passes a full mask / bias / probability output (the encoder stack): no score buffers
    // when a fused kernel covers the block
    size_t carve(void *base, const pio_self_attention_t &sa, int B, int N, bool lean = false) {
        Carver c(base);
        const int64_t rows = (int64_t)B * N;
        const int cmax = padc(sa.attn.q_in) > padc(sa.mlp.in) ? padc(sa.attn.q_in) : padc(sa.mlp.in);
        x16 = take_pair(c, (size_t)rows * cmax, sa.attn.act_split || sa.mlp.act_split);
        h16 = take_pair(c, (size_t)rows * padc(sa.mlp.hidden), sa.mlp.act_split != 0);
        x1 = (float *)c.take((size_t)rows * sa.attn.out * 4);
        core.carve(c, sa.attn, B, B, N, N, lean);
        if (sa.fold.qkv.w_hi && sa.fold.fc1.w_hi) {
            // The residual GEMMs (out, fc2) read the residual pair and write the result pair element for element from
            // the same lane (load, add, store), and their A operand is another array (attention output / hidden
            // activations): the stream is updated IN PLACE -- one 16-bit pair (x16b = x16.hi, lo_b = lo_a), and the
            // hidden activations take the attention output's buffer (dead once the out projection has run).  Per layer
            // at B = 32 the arrays in flight are 192 MB (two ping-pong pairs: 288 MB, beyond the 256 MB Infinity Cache).
            x16b = x16.hi;
            lo_a = lo_b = c.take((size_t)rows * cmax * 2);
            part_a = (float *)c.take((size_t)rows * (cmax / 64 + 1) * 2 * 4);  // (up to one slot per 64 columns)
            part_b = (float *)c.take((size_t)rows * (cmax / 64 + 1) * 2 * 4);
            if (!sa.mlp.act_split && !sa.attn.act_split &&
                (size_t)rows * padc(sa.mlp.hidden) <= (size_t)rows * sa.attn.heads * sa.attn.dvp)
                h16.hi = core.o16.hi;
        }
        return c.off;
    }
};

struct CrossPlan {
    Pair q16, kv16, h16;
    float *x1;
    AttnScratch core;
    bool q_bcast;
    size_t carve(void *base, const pio_cross_attention_t &ca, int B, int Tq, int Tk, bool qb, bool lean = false) {
        Carver c(base);
        q_bcast = qb;
        const int Bq = qb ? 1 : B;
        const int64_t rows = (int64_t)B * Tq;
        const bool sp = ca.attn.act_split || ca.mlp.act_split;
        // q16 is reused for LN2(x1): size it for all B*Tq rows
        q16 = take_pair(c, (size_t)rows * padc(ca.attn.q_in), sp);
        kv16 = take_pair(c, (size_t)B * Tk * padc(ca.attn.k_in), ca.attn.act_split != 0);
        h16 = take_pair(c, (size_t)rows * padc(ca.mlp.hidden), ca.mlp.act_split != 0);
        x1 = (float *)c.take((size_t)rows * pitch8(ca.attn.out) * 4);
        core.carve(c, ca.attn, Bq, B, Tq, Tk, lean, true);
        return c.off;
    }
};

struct DecoderPlan {
    CrossPlan cp;
    float *y;
    Pair y16;
    size_t carve(void *base, const pio_cross_attention_t &cross, const pio_linear_t *fin, int B, int Q, int N,
                 bool qb) {
        Carver c(base);
        const int64_t rows = (int64_t)B * Q;
        y = nullptr;
        y16 = Pair();
        if (fin) {
            y = (float *)c.take((size_t)rows * pitch4(cross.attn.q_in) * 4);
            y16 = take_pair(c, (size_t)rows * padc(cross.attn.q_in), cross.mlp.act_split != 0);
        }
        const size_t inner = cp.carve(base ? (char *)base + c.off : nullptr, cross, B, Q, N, qb, true);
        return c.off + inner;
    }
};

// ======================================================================================================
// LayerNorm fold of a SelfAttention block
// ======================================================================================================
struct FoldKnobs {  // every switch the fold consults, read by the caller (pio_blocks.hip: env, pio_ln_fold_enable, call opts)
    int choice;  // 0 off, 1 where it pays, 2 wherever offered
    int64_t wide_min_rows, small_min_rows, small_max_rows;  // row bounds of the two kernel families
};

struct SelfCall {  // what self_attention_run knows about one call, as plain facts
    int B, N, C;
    int64_t stride_t, stride_b;  // of the fp32 input (elements)
    bool x_aligned16;            // ... whose data pointer is 16-byte aligned
    bool has_fold_buffers;       // the plan carved the fold's buffers (SelfPlan.x16b)
    bool kv_mask, q_mask, full_mask, bias, probs;  // which optional operands the call passes
};

struct SelfFold {
    enum { NONE, SMALL, WIDE } family;
    int slot_w, nslots;  // statistics slots: columns per slot, slots per row (0 when un-folded)
};

// LayerNorm fold: contiguous rows of 512 / 768 / 1024 / 1280 / 1536 channels, single-sweep activations, the fused
// q|k|v form (head widths the fused attention kernel covers), nothing that needs the score matrix.  Two kernel
// families: the 256 x 256-tile kernel with 128-column statistics slots for stacks with enough rows to fill the chip
// (weights may then be (hi, lo) pairs -- policies "x2s" / "x2w": second K sweep against the lo image; of the stacked
// q|k|v image only the V rows may have one), the tile kernels with 64-column slots below that (single weights).
inline SelfFold self_fold_route(const pio_self_attention_t &sa, const SelfCall &c, const FoldKnobs &k) {
    const int64_t rows = (int64_t)c.B * c.N;
    const bool fold_ok = k.choice != 0 && c.has_fold_buffers && c.C >= 512 && c.C <= 1536 && (c.C % 256) == 0 &&
                         c.stride_t == c.C && (c.B == 1 || c.stride_b == (int64_t)c.N * c.C) && !sa.attn.act_split &&
                         !sa.mlp.act_split && sa.attn.qkv.w_hi &&
                         (!sa.fold.qkv.w_lo || sa.fold.qkv.lo_row0 == 2 * sa.attn.heads * sa.attn.dkp) &&
                         (!sa.fold.fc1.w_lo || sa.fold.fc1.lo_row0 == 0) && flash_supported(sa.attn.dkp, sa.attn.dvp) &&
                         sa.fold.qkv.n == sa.attn.qkv.n && sa.fold.qkv.k == c.C && sa.fold.fc1.k == c.C &&
                         sa.fold.fc1.n == sa.mlp.fc1.n && sa.mlp.hidden == c.C && sa.mlp.dtype == sa.attn.dtype &&
                         !c.kv_mask && !c.q_mask && !c.full_mask && !c.bias && !c.probs && c.x_aligned16;
    const bool fold_wide = fold_ok && rows >= k.wide_min_rows;
    // (tile-kernel family: up to 4095 rows in the automatic mode -- ImageNet B = 8, 4096 rows, measures 8.33 ms folded on
    //  the tile kernels against 7.86 un-folded, whose q|k|v GEMM runs on the 256 x 256-tile kernel; B = 1 / 2 / 4:
    //  3.78 / 4.28 / 5.05 against 3.97 / 4.39 / 5.27 ms -- tools/r4_probe4.sh)
    const bool fold_small = fold_ok && !fold_wide && rows >= k.small_min_rows &&
                            (k.choice == 2 || rows < k.small_max_rows) && !sa.fold.qkv.w_lo &&
                            !sa.fold.fc1.w_lo && !sa.attn.o.w_lo && !sa.mlp.fc2.w_lo;
    if (!fold_wide && !fold_small) return SelfFold{SelfFold::NONE, 0, 0};
    const int slot_w = fold_wide ? 128 : 64;
    return SelfFold{fold_wide ? SelfFold::WIDE : SelfFold::SMALL, slot_w, c.C / slot_w};
}

// A decoder with a final Linear: the cross-attend's result is only ever that Linear's operand, so fc2 writes it as 16-bit
// rows directly when the packed image's K is the channel pitch of those rows.
inline bool decoder_y16_direct(const pio_linear_t *final_layer, int q_c) {
    return final_layer && final_layer->k == padc(q_c);
}

// ======================================================================================================
// the GEMM descriptor of one nn.Linear
// ======================================================================================================
inline pio_gemm_t gemm_defaults(int dtype) {
    pio_gemm_t g = {};
    g.batch = 1;
    g.nh = 1;
    g.alpha = 1.f;
    g.dtype = dtype;
    return g;
}

struct Residual {
    const float *ptr = nullptr;
    int64_t ld = 0, stride_b = 0;
    int rows_per_batch = 0;
};

inline Residual residual_of(const pio_tensor3_t &t) { return Residual{t.data, t.stride_t, t.stride_b, t.T}; }

// LayerNorm fold plumbing of one GEMM (pio_ln_fold_t; all null = plain GEMM).  Consumer side: the 16-bit input is the
// UN-normalised activation and `in_part` its per-row partial sums -- the GEMM then uses the folded weights `w` / row
// sums `c`.  Producer side: where the (fp32 + residual) GEMM leaves the 16-bit copy and the partial sums of its result.
struct LnFold {
    const float *in_part = nullptr;
    const pio_linear_t *w = nullptr;
    const float *c = nullptr;
    float eps = 0.f;
    void *out16 = nullptr;
    int64_t ld16 = 0;
    float *out_part = nullptr;
    // ... and the residual stream as a 16-bit pair: lo half of the result, residual given as (hi, lo); with both the
    // fp32 output pointer of the GEMM may be null
    void *out16_lo = nullptr;
    const void *res16_hi = nullptr, *res16_lo = nullptr;
    int32_t *range_flag = nullptr;  // producer: the caller's range-guard word (pio_ln_fold_t.range_flag)
    // slot form of the row statistics (pio_gemm_t.ln_slots / row_slot_w): 128-column slots = the 256 x 256-tile kernel,
    // 64-column slots = the tile kernels (stacks of fewer rows)
    int in_slots = 0, slot_w = 0;
};

constexpr int kActNone = 0, kActGelu = 1;  // pio_gemm_t.act

// Where and how the result of one linear leaves.  Three forms, each with a name (below); the optional parts of a form
// are added behind it: pair16_at(h, ld).gelu().folded(&f), f32_at(out, n, ld).plus(&res).folded(&f).zeros_to(n8).
struct LinearOut {
    void *y = nullptr, *y_lo = nullptr;
    bool f32 = false;
    int n_logical = 0;              // fp32 form: logical width (a 16-bit form computes all lin.n packed columns)
    int64_t ldc = 0;                // row pitch of y (elements)
    int act = kActNone;
    const Residual *res = nullptr;  // fp32 residual (null, or ptr null: none)
    const LnFold *fold = nullptr;   // consumer (in_part) or producer (out16) of a LayerNorm fold
    int n_store16 = 0;              // columns written per row when wider than those computed: the rest as zeros

    LinearOut gelu() const { LinearOut o = *this; o.act = kActGelu; return o; }
    LinearOut plus(const Residual *r) const { LinearOut o = *this; o.res = r; return o; }
    LinearOut folded(const LnFold *f) const { LinearOut o = *this; o.fold = f; return o; }
    LinearOut zeros_to(int n) const { LinearOut o = *this; o.n_store16 = n; return o; }
};
// a 16-bit pair (lo may be null) at row pitch ld
inline LinearOut pair16_at(Pair y, int64_t ld) {
    LinearOut o;
    o.y = y.hi; o.y_lo = y.lo; o.ldc = ld;
    return o;
}
// fp32 rows of n_logical columns at row pitch ld
inline LinearOut f32_at(float *y, int n_logical, int64_t ld) {
    LinearOut o;
    o.y = y; o.f32 = true; o.n_logical = n_logical; o.ldc = ld;
    return o;
}
// the decoders' y in front of their final Linear: fc2 leaves (+ residual) as the 16-bit operand rows of that GEMM, pitch
// ld = padc(channels), zero-filled behind the computed columns
inline LinearOut out16_at(Pair y, int64_t ld, const Residual *res) {
    return pair16_at(y, ld).plus(res).zeros_to((int)ld);
}

// y[rows, n] = x16[rows, lin.k] * W^T (+bias) (act) (+R); a 16-bit output has ldc = lin.n (padded).
inline pio_gemm_t linear_gemm(const pio_linear_t &lin_plain, int dtype, Pair x, int64_t rows, const LinearOut &o) {
    const LnFold *fold = o.fold;
    const pio_linear_t &lin = (fold && fold->in_part) ? *fold->w : lin_plain;
    pio_gemm_t g = gemm_defaults(dtype);
    if (fold && fold->in_part) {
        g.ln_part = fold->in_part;
        g.ln_c = fold->c;
        g.ln_eps = fold->eps;
        g.ln_slots = fold->in_slots;
    }
    if (fold && fold->out16) {
        g.X16 = fold->out16;
        g.ld16 = fold->ld16;
        g.row_part = fold->out_part;
        g.X16_lo = fold->out16_lo;
        g.R16_hi = fold->res16_hi;
        g.R16_lo = fold->res16_lo;
        g.range_flag = fold->range_flag;
        g.row_slot_w = fold->slot_w;
    }
    g.A = x.hi;
    g.A_lo = x.lo;
    g.B = lin.w_hi;
    g.B_lo = lin.w_lo;
    g.b_lo_n0 = lin.w_lo ? lin.lo_row0 : 0;
    g.C = o.y;
    g.C_lo = o.y_lo;
    g.M = (int)rows;
    g.N = o.f32 ? o.n_logical : lin.n;
    // fp32 rows with a rounded-up pitch (pitch4: internal buffers): compute whole float4 groups -- the packed image has
    // zero rows / zero bias behind the logical ones -- so that every store and residual load is a 16-byte one
    // (n_store16 on an fp32 result -- x1 of a cross-attend, pitch8: the columns up to it are written as zeros, so a residual
    //  there adds nothing a caller's wider rows might hold behind the logical columns)
    if (o.f32 && (o.n_logical & 3) && o.ldc >= pitch4(o.n_logical) && lin.n >= pitch4(o.n_logical) &&
        !(o.res && o.res->ptr && (o.res->ld < pitch4(o.n_logical) || o.n_store16 > o.n_logical)))
        g.N = pitch4(o.n_logical);
    g.K = lin.k;
    g.lda = lin.k;
    g.ldb = lin.k;
    g.ldc = o.ldc;
    g.bias = lin.bias;
    g.bias_mode = lin.bias ? 1 : 0;
    g.act = o.act;
    g.out_f32 = o.f32 ? 1 : 0;
    g.n_store = o.n_store16 > g.N ? o.n_store16 : g.N;   // (rows zero-filled up to the channel pitch / the pitch of x1)
    if (o.res && o.res->ptr && !(fold && fold->res16_hi)) {
        g.R = o.res->ptr;
        g.ldr = o.res->ld;
        g.r_stride_b = o.res->stride_b;
        g.r_rows_per_batch = o.res->rows_per_batch;
    }
    return g;
}

}  // namespace pio
