// Host-side composition of the PerceiverIO hot-path blocks out of the gfx950 kernels.
// One C call per reference nn.Module.forward; every launch goes to the caller's stream, all scratch
// comes from the caller's workspace (graph-capture safe: no allocation, no synchronisation).
//
//   attention_core   <- Attention.forward / attend        transformer_primitives.py:90-180
//   mlp_core         <- MLP.forward                        transformer_primitives.py:212-216
//   self_attention   <- SelfAttention.forward              transformer_primitives.py:275-297
//   cross_attention  <- CrossAttention.forward             transformer_primitives.py:371-406
//   encoder / decoder<- PerceiverEncoder/Decoder.forward   perceiver.py:98-107, 166-180
//
// 16-bit operands travel as (hi, lo) pairs: lo == nullptr unless the descriptor says act_split
// (precision policy "*x3": every product is hi*hi + hi*lo + lo*hi, i.e. ~fp32-exact).
#include "pio_internal.h"

namespace pio {

#define PIO_TRY(expr)                  \
    do {                               \
        int _e = (expr);               \
        if (_e != PIO_OK) return _e;   \
    } while (0)

// Range probe (pio_range_probe_begin; tooling, off by default): one pio_absmax16 over the hi half of a 16-bit activation
// buffer, right behind its producer.  kind: PIO_RK_*; the extent is (batch x) rows x cols with row pitch ld.
#define PIO_RANGE(kind, dtype, ptr, rows, cols, ld, batch, stride_b, stream) \
    do {                                                                      \
        if (range_probe_active())                                             \
            PIO_TRY(range_probe_record(kind, dtype, ptr, rows, cols, ld, batch, stride_b, stream)); \
    } while (0)

// One nn.Linear: the descriptor is linear_gemm's (pio_block_route.h); `o` names the form the result leaves in.
static int linear_fwd(const pio_linear_t &lin, int dtype, Pair x, int64_t rows, const LinearOut &o, hipStream_t s) {
    return gemm_nt_launch(linear_gemm(lin, dtype, x, rows, o), s);
}

// (LayerNorm +) cast of fp32 rows to the 16-bit operand pair; range_kind: the PIO_RK_* label of its range-probe record
static int cast_pair(const pio_tensor3_t &x, const pio_layernorm_t *ln, Pair y, int c_pad, int dtype, int range_kind,
                     hipStream_t s) {
    PIO_TRY(layernorm_cast_launch(x, ln, y.hi, y.lo, c_pad, dtype, s));
    PIO_RANGE(range_kind, dtype, y.hi, (int64_t)x.B * x.T, x.C, c_pad, 1, 0, s);
    return PIO_OK;
}

// ------------------------------------------------------------------------------------------------------
// attention core on already normalised / cast 16-bit inputs
// ------------------------------------------------------------------------------------------------------
static int check_attention(const pio_attention_t &a) {
    if (a.heads <= 0 || a.dk <= 0 || a.dv <= 0) return PIO_E_SHAPE;
    if (a.dkp != pad8(a.dk) || a.dvp != pad8(a.dv)) return PIO_E_SHAPE;
    if (a.q.n != a.heads * a.dkp || a.k.n != a.heads * a.dkp || a.v.n != a.heads * a.dvp) return PIO_E_SHAPE;
    if (a.o.k != a.heads * a.dvp || a.q.k != padc(a.q_in) || a.k.k != padc(a.k_in) || a.v.k != padc(a.v_in))
        return PIO_E_SHAPE;
    if (!a.q.w_hi || !a.k.w_hi || !a.v.w_hi || !a.o.w_hi) return PIO_E_ARG;
    // (split ACTIVATIONS do not require split weights: the "x2a" policies run A_hi B^T + A_lo B^T against single weights)
    return PIO_OK;
}

// K / V projection fold of the single-head cross-attends (attention_core step 0b); PIO_KV_FOLD=0 turns it off (read at
// every call: an A/B switch for tools/, not an API).
static bool kv_fold_enabled() {
    const char *e = getenv("PIO_KV_FOLD");
    return !e || atoi(e) != 0;
}

// Projected queries kept by the CALLER across calls (pio_decoder_call_t.q16_hi): a decoder whose query array depends on
// parameters and constants only (the multimodal model's chunk queries) normalises and projects it once, not per call.
struct QCache {
    Pair pair;    // [Bq * Tq][H * dkp] 16-bit (+ lo half when the attention carries split activations)
    bool valid;   // false: compute into `pair`; true: `pair` holds the projection -- skip LayerNorm_q and proj_q
};

// Materialised attention (steps 4-6) on the projected q / k (t) and w.vt16, in passes of (b_chunk samples) x (q_chunk
// query rows) so that the score matrix held at once stays below kScoreCapBytes.  Row chunks inside a sample only happen
// with b_chunk == 1 (mask pointers then move with the sample and the row).
static int materialised_core(const pio_attention_t &a, const AttnOperands &t, bool q_bcast, int B, int Tq, int Tk,
                             const AttnOptional &opt, AttnScratch &w, hipStream_t s) {
    const int H = a.heads;
    const int64_t ldq = t.ldq, ldo = (int64_t)H * a.dvp, tkp = pad8(Tk), tkv = round_up(Tk, 32);
    const ScoreChunks ch = score_chunks(B, H, Tq, Tk);
    // full masks / biases / probability outputs are [B,H,Tq,Tk]-sized themselves: callers that pass them have the memory;
    // they run in one pass per sample
    if ((opt.full_mask || opt.bias || opt.probs) && ch.q_chunk != Tq) return PIO_E_WORKSPACE;
    for (int b0 = 0; b0 < B; b0 += ch.b_chunk) {
        const int nb = b0 + ch.b_chunk <= B ? ch.b_chunk : B - b0;
        for (int r0 = 0; r0 < Tq; r0 += ch.q_chunk) {
            const int nr = r0 + ch.q_chunk <= Tq ? ch.q_chunk : Tq - r0;
            const int64_t qoff = (q_bcast ? 0 : (int64_t)b0 * Tq * ldq) + (int64_t)r0 * ldq;
            const int64_t koff = (int64_t)b0 * Tk * ldq;
            // 4: S[b,h] = Q[b,h] K[b,h]^T (transformer_primitives.py:138), fp32 scores
            {
                pio_gemm_t g = gemm_defaults(a.dtype);
                g.A = (const char *)t.Q + qoff * 2;
                g.A_lo = t.Q_lo ? (const char *)t.Q_lo + qoff * 2 : nullptr;
                g.B = (const char *)t.K + koff * 2;
                g.B_lo = t.K_lo ? (const char *)t.K_lo + koff * 2 : nullptr;
                g.C = w.scores;
                g.M = nr;
                g.N = Tk;
                g.K = a.dkp;
                g.lda = ldq;
                g.ldb = ldq;
                g.ldc = Tk;
                g.batch = nb * H;
                g.nh = H;
                g.sAb = t.sQb;
                g.sAh = a.dkp;
                g.sBb = t.sKb;
                g.sBh = a.dkp;
                g.sCb = (int64_t)H * nr * Tk;
                g.sCh = (int64_t)nr * Tk;
                g.out_f32 = 1;
                g.n_store = Tk;
                PIO_TRY(gemm_nt_launch(g, s));
            }
            // 5: bias, scale, mask, softmax, wipe (transformer_primitives.py:143-158, 168-175)
            {
                const int64_t moff = (int64_t)b0 * H * Tq * Tk;  // (full-size operands: only with nr == Tq)
                PIO_TRY(softmax_rows_launch(w.scores, Tk, w.p16.hi, w.p16.lo, tkp, nb, H, nr, Tk,
                                            1.0f / sqrtf((float)a.dk), opt.kv_mask ? opt.kv_mask + (int64_t)b0 * Tk : nullptr,
                                            opt.q_mask ? opt.q_mask + (int64_t)b0 * Tq + r0 : nullptr,
                                            opt.full_mask ? opt.full_mask + (int64_t)b0 * Tq * Tk : nullptr,
                                            opt.bias ? opt.bias + moff : nullptr, a.dtype,
                                            opt.probs ? opt.probs + moff : nullptr, s));
            }
            // 6: O[b,:,h] = P[b,h] V[b,h] (transformer_primitives.py:163-166), heads merged by the store layout
            {
                const int64_t ooff = ((int64_t)b0 * Tq + r0) * ldo, voff = (int64_t)b0 * ldo * tkv;
                pio_gemm_t g = gemm_defaults(a.dtype);
                g.A = w.p16.hi;
                g.A_lo = w.p16.lo;
                g.B = (const char *)w.vt16.hi + voff * 2;
                g.B_lo = w.vt16.lo ? (const char *)w.vt16.lo + voff * 2 : nullptr;
                g.C = (char *)w.o16.hi + ooff * 2;
                g.C_lo = w.o16.lo ? (char *)w.o16.lo + ooff * 2 : nullptr;
                g.M = nr;
                g.N = a.dvp;
                g.K = (int)tkp;
                g.lda = tkp;
                g.ldb = tkv;
                g.ldc = ldo;
                g.batch = nb * H;
                g.nh = H;
                g.sAb = (int64_t)H * nr * tkp;
                g.sAh = (int64_t)nr * tkp;
                g.sBb = ldo * tkv;
                g.sBh = (int64_t)a.dvp * tkv;
                g.sCb = (int64_t)Tq * ldo;
                g.sCh = a.dvp;
                g.n_store = a.dvp;
                PIO_TRY(gemm_nt_launch(g, s));
            }
        }
    }
    return PIO_OK;
}

// One route (attn_route, pio_attn_route.h), then: the projections it names, one core launch, the out projection.
struct AttnExtras {  // what a caller may add to one attention_core call (the default value: none of it)
    const Residual *res = nullptr;                         // fp32 residual of the out projection
    const LnFold *fold_in = nullptr, *fold_out = nullptr;  // LayerNorm fold in front of q|k|v / behind the out projection
    int64_t out_ld = 0;        // row pitch of `out` (0: a.out; an internal buffer may round it up: pitch8)
    const QCache *qc = nullptr;
};
static int attention_core(const pio_attention_t &a, Pair xq, bool q_bcast, Pair xk, Pair xv, int B, int Tq, int Tk,
                          const AttnOptional &opt, float *out, AttnScratch &w, const AttnExtras &x, hipStream_t s) {
    const LnFold *fold_out = x.fold_out;
    const QCache *qc = x.qc;
    const int64_t out_ld = x.out_ld ? x.out_ld : a.out;
    PIO_TRY(check_attention(a));
    if (qc) {
        if (!qc->pair.hi || (a.act_split && !qc->pair.lo)) return PIO_E_ARG;
        w.q16 = qc->pair;  // (the plan's own q16 carve stays unused)
    }
    const int H = a.heads;
    const int64_t hdk = (int64_t)H * a.dkp, ldo = (int64_t)H * a.dvp, ld3 = 2 * hdk + ldo, tkv = round_up(Tk, 32);
    const int Bq = q_bcast ? 1 : B;
    AttnCall call = {};
    call.B = B; call.Bq = Bq; call.Tq = Tq; call.Tk = Tk; call.q_bcast = q_bcast; call.same_qk = xq.hi == xk.hi;
    call.same_kv = xk.hi == xv.hi; call.kv_fold_on = kv_fold_enabled();
    note_optional(call, opt);
    call.qcache = qc; call.fold_in = x.fold_in; call.fold_out = fold_out;
    call.fold_qkv = (x.fold_in && x.fold_in->in_part) ? x.fold_in->w : nullptr;
    // (q16, k16, vt16 are consecutive carves: together they hold the [rows, ld3] matrix of the q|k|v form, q16 | k16 the
    //  [rows, 2 hdk] one of the q|k form)
    call.qkv_adjacent = (char *)w.q16.hi < (char *)w.k16.hi && (char *)w.k16.hi < (char *)w.vt16.hi &&
                        (size_t)((char *)w.vt16.hi - (char *)w.q16.hi) + (size_t)B * ldo * tkv * 2 >= (size_t)B * Tq * ld3 * 2;
    call.qk_adjacent = (char *)w.q16.hi + (size_t)B * Tq * hdk * 2 <= (char *)w.k16.hi;
    const AttnRoute r = attn_route(a, call);
    if (r.err != PIO_OK) return r.err;
    if (r.qk_pair && (!w.q16.lo || !w.k16.lo)) return PIO_E_ARG;
    if (r.need_scores && !w.scores) return PIO_E_WORKSPACE;  // (the plan promised a fused kernel)
    const bool kv_fold = r.core == AttnCore::KVFOLD_XATTN || r.core == AttnCore::KVFOLD_XTALL;
    const int64_t sQ = q_bcast ? 0 : 1;  // batch-invariant queries: batch stride 0
    const Pair q16_hi = {w.q16.hi, nullptr};  // where the stacked q|k and q|k|v GEMMs write (single-sweep activations)

    // Projections (transformer_primitives.py:93-95), head-padded columns; t: the operands they leave for the core
    AttnOperands t = {};
    t.O = w.o16.hi;
    t.O_lo = r.out_pair ? w.o16.lo : nullptr;
    if (r.core == AttnCore::QKV_FLASH) {
        // ONE GEMM over the stacked [q | k | v] weight image; the core reads V row-major (transposed LDS reads)
        PIO_TRY(linear_fwd(a.qkv, a.dtype, xq, (int64_t)B * Tq, pair16_at(q16_hi, ld3).folded(x.fold_in), s));
        PIO_RANGE(PIO_RK_Q, a.dtype, w.q16.hi, (int64_t)B * Tq, ld3, ld3, 1, 0, s);
        const char *base = (const char *)w.q16.hi;
        t.Q = base; t.K = base + hdk * 2; t.VT = base + 2 * hdk * 2;
        t.ldq = t.ldk = t.ldvt = ld3; t.ldo = ldo;
        t.sQb = t.sKb = t.sVb = (int64_t)Tq * ld3; t.sOb = (int64_t)Tq * ldo;
    } else if (kv_fold) {
        // K / V projection fold (pio_attention_t.kq / vo): the fused kernel reads the LayerNorm'd input
        // array itself as K and its transpose as V^T.  Per call: Q = LN_q(xq) Wq^T + bq (as always), Q' = Q Wk into the
        // (otherwise unused) k16 scratch, one 16-bit transpose of the inputs and the out projection (Wo Wv) over K = C.
        const int64_t kvp = a.dkp, ldx = padc(a.k_in);  // ldx: row pitch of the LayerNorm'd inputs
        PIO_TRY(linear_fwd(a.q, a.dtype, xq, (int64_t)Bq * Tq, pair16_at(w.q16, hdk), s));
        PIO_RANGE(PIO_RK_Q, a.dtype, w.q16.hi, (int64_t)Bq * Tq, hdk, hdk, 1, 0, s);
        PIO_TRY(linear_fwd(a.kq, a.dtype, w.q16, (int64_t)Bq * Tq, pair16_at(w.k16, kvp), s));
        PIO_RANGE(PIO_RK_Q, a.dtype, w.k16.hi, (int64_t)Bq * Tq, kvp, kvp, 1, 0, s);  // (Q Wk: the core's query operand)
        PIO_TRY(transpose16_launch(xk.hi, ldx, B, Tk, (int)kvp, w.vt16.hi, tkv, s));
        t.Q = w.k16.hi; t.K = xk.hi; t.VT = w.vt16.hi;
        t.ldq = kvp; t.ldk = ldx; t.ldvt = tkv; t.ldo = kvp;
        t.sQb = sQ * Tq * kvp; t.sKb = (int64_t)Tk * ldx; t.sVb = kvp * tkv; t.sOb = (int64_t)Tq * kvp;
    } else {
        // Q and K: one GEMM over the stacked [q rows | k rows] image (the adjacent q16 / k16 regions as one
        // [rows, 2*H*dkp] matrix) when the route says so, else one each (a valid query cache holds Q already)
        const int64_t ldq = r.fuse_qk ? 2 * hdk : hdk;
        if (r.fuse_qk) {
            PIO_TRY(linear_fwd(a.qk, a.dtype, xq, (int64_t)B * Tq, pair16_at(q16_hi, ldq), s));
            PIO_RANGE(PIO_RK_Q, a.dtype, w.q16.hi, (int64_t)B * Tq, ldq, ldq, 1, 0, s);
        } else {
            if (!(qc && qc->valid)) {
                PIO_TRY(linear_fwd(a.q, a.dtype, xq, (int64_t)Bq * Tq, pair16_at(w.q16, ldq), s));
                PIO_RANGE(PIO_RK_Q, a.dtype, w.q16.hi, (int64_t)Bq * Tq, ldq, ldq, 1, 0, s);
            }
            PIO_TRY(linear_fwd(a.k, a.dtype, xk, (int64_t)B * Tk, pair16_at(w.k16, ldq), s));
            PIO_RANGE(PIO_RK_K, a.dtype, w.k16.hi, (int64_t)B * Tk, ldq, ldq, 1, 0, s);
        }
        // V^T[b] = Wv * X_v[b]^T + bv produced directly in the K-contiguous layout the P*V product wants; the weight is
        // the A operand (batch stride 0), bias is per output ROW.
        pio_gemm_t g = gemm_defaults(a.dtype);
        g.A = a.v.w_hi;
        g.A_lo = a.v.w_lo;
        g.B = xv.hi;
        g.B_lo = xv.lo;
        g.C = w.vt16.hi;
        g.C_lo = w.vt16.lo;
        g.M = a.v.n;
        g.N = Tk;
        g.K = a.v.k;
        g.lda = a.v.k;
        g.ldb = a.v.k;
        g.ldc = tkv;
        g.batch = B;
        g.sBb = (int64_t)Tk * a.v.k;
        g.sCb = ldo * tkv;
        g.bias = a.v.bias;
        g.bias_mode = a.v.bias ? 2 : 0;
        g.n_store = (int)tkv;  // columns [Tk, tkv) are written as zeros
        PIO_TRY(gemm_nt_launch(g, s));
        PIO_RANGE(PIO_RK_V, a.dtype, w.vt16.hi, ldo, Tk, tkv, B, ldo * tkv, s);
        t.Q = w.q16.hi; t.K = r.fuse_qk ? (const char *)w.q16.hi + hdk * 2 : w.k16.hi; t.VT = w.vt16.hi;
        if (r.qk_pair) { t.Q_lo = w.q16.lo; t.K_lo = w.k16.lo; }
        t.ldq = t.ldk = ldq; t.ldvt = tkv; t.ldo = ldo;
        t.sQb = sQ * Tq * ldq; t.sKb = (int64_t)Tk * ldq; t.sVb = ldo * tkv; t.sOb = (int64_t)Tq * ldo;
    }

    // logit probe (pio_logit_probe_begin; tooling, off by default): the operands the core is about to exponentiate --
    // hi halves, without the bias -- under the call's masks
    if (logit_probe_active())
        PIO_TRY(logit_probe_record(a.dtype, a.dkp, a.dk, t, B, H, Tq, Tk, opt.kv_mask, opt.q_mask, opt.full_mask, s));
    switch (r.core) {
    case AttnCore::QKV_FLASH: case AttnCore::PAIR_FLASH: case AttnCore::FLASH:
        PIO_TRY(flash_attention_launch(a.dtype, a.dkp, a.dvp, a.dk, t, B, H, Tq, Tk, r.core == AttnCore::QKV_FLASH, s));
        break;
    case AttnCore::KVFOLD_XATTN: case AttnCore::PAIR_XATTN: case AttnCore::XATTN:
        PIO_TRY(xattn_launch(a.dtype, a.dkp, a.dvp, a.dk, t, B, H, Tq, Tk, opt.kv_mask, opt.q_mask, w.xpart, s));
        break;
    case AttnCore::KVFOLD_XTALL: case AttnCore::XTALL:
        PIO_TRY(xtall_launch(a.dtype, a.dkp, a.dvp, a.dk, t, B, H, Tq, Tk, opt.kv_mask, opt.q_mask, w.xpart, s));
        break;
    case AttnCore::MATERIALISED:
        PIO_TRY(materialised_core(a, t, q_bcast, B, Tq, Tk, opt, w, s));
        break;
    }
    PIO_RANGE(PIO_RK_ATTN, a.dtype, w.o16.hi, (int64_t)B * Tq, t.ldo, t.ldo, 1, 0, s);
    // final projection (+ residual) (transformer_primitives.py:110; SelfAttention :290, CrossAttention :396-399); behind
    // the K / V fold it is Wo Wv.  (An internal pitch: zeros behind the logical columns.)
    PIO_TRY(linear_fwd(kv_fold ? a.vo : a.o, a.dtype, w.o16, (int64_t)B * Tq,
                       f32_at(out, a.out, out_ld).plus(x.res).folded(fold_out).zeros_to(out_ld > a.out ? (int)out_ld : 0), s));
    if (fold_out && fold_out->out16)
        PIO_RANGE(PIO_RK_STREAM, a.dtype, fold_out->out16, (int64_t)B * Tq, a.out, fold_out->ld16, 1, 0, s);
    return PIO_OK;
}

// ------------------------------------------------------------------------------------------------------
// MLP core on a 16-bit input
// ------------------------------------------------------------------------------------------------------
// out16 (optional; then `out` is not written): the result leaves as the 16-bit operand (pair under split activations) of
// the GEMM that follows -- rows of padc(m.out) elements, zero-filled behind the logical columns -- instead of as fp32 rows
// that a cast pass would re-read (the decoders' y in front of their final Linear).
struct MlpExtras {  // what a caller may add to one mlp_core call (the default value: none of it)
    const Residual *res = nullptr;                         // fp32 residual of fc2
    const LnFold *fold_in = nullptr, *fold_out = nullptr;  // LayerNorm fold in front of fc1 / behind fc2
    int64_t out_ld = 0;                                    // row pitch of `out` (0: m.out)
    const Pair *out16 = nullptr;
};
static int mlp_core(const pio_mlp_t &m, Pair x, int64_t rows, Pair h, float *out, const MlpExtras &e, hipStream_t s) {
    const int64_t out_ld = e.out_ld ? e.out_ld : m.out;
    if (m.fc1.k != padc(m.in) || m.fc1.n != padc(m.hidden) || m.fc2.k != m.fc1.n) return PIO_E_SHAPE;
    PIO_TRY(linear_fwd(m.fc1, m.dtype, x, rows, pair16_at(h, m.fc1.n).gelu().folded(e.fold_in), s));
    PIO_RANGE(PIO_RK_HIDDEN, m.dtype, h.hi, rows, m.hidden, m.fc1.n, 1, 0, s);
    if (e.out16) {
        // (this GEMM computes all fc2.n = pad8(m.out) columns, so its epilogue reads that many residual columns: the
        //  caller's residual rows have a pitch of at least pad8(m.out) and zeros behind the logical columns -- x1 of
        //  cross_attention_run, pitch8)
        if (e.res && e.res->ptr && e.res->ld < m.fc2.n) return PIO_E_SHAPE;
        PIO_TRY(linear_fwd(m.fc2, m.dtype, h, rows, out16_at(*e.out16, padc(m.out), e.res), s));
        PIO_RANGE(PIO_RK_STREAM, m.dtype, e.out16->hi, rows, m.out, padc(m.out), 1, 0, s);
        return PIO_OK;
    }
    PIO_TRY(linear_fwd(m.fc2, m.dtype, h, rows, f32_at(out, m.out, out_ld).plus(e.res).folded(e.fold_out), s));
    if (e.fold_out && e.fold_out->out16)
        PIO_RANGE(PIO_RK_STREAM, m.dtype, e.fold_out->out16, rows, m.out, e.fold_out->ld16, 1, 0, s);
    return PIO_OK;
}

static bool same_tensor(const pio_tensor3_t &a, const pio_tensor3_t &b) {
    return a.data == b.data && a.stride_b == b.stride_b && a.stride_t == b.stride_t && a.B == b.B && a.T == b.T &&
           a.C == b.C;
}

static pio_tensor3_t first_batch(const pio_tensor3_t &t) {
    pio_tensor3_t r = t;
    r.B = 1;
    return r;
}

static Pair pair_if(Pair p, bool split) {
    if (!split) p.lo = nullptr;
    return p;
}

// LayerNorm fold switch (pio_ln_fold_enable; initial value from env PIO_LN_FOLD, default 1).
// 0: never, 1: where it pays, 2: wherever a block offers it.  "Where it pays": the fold's GEMMs are the 256 x 256-tile
// kernel, which needs >= 96 tiles of a 1024-wide output to beat the 128 / 64-tile kernels of the un-folded block --
// measured on the ImageNet classifier (tools/latency_probe.py, ms per forward, fold on / off): B=4 7.75 / 5.22,
// B=8 8.12 / 7.64, B=12 10.14 / 10.09, B=16 10.69 / 11.57, B=32 16.62 / 18.24 -- hence 6144 rows (env
// PIO_LN_FOLD_MIN_ROWS).
static int &ln_fold_global() {
    static int choice = [] {
        const char *e = getenv("PIO_LN_FOLD");
        const int v = e ? atoi(e) : 1;
        return v < 0 ? 0 : v > 2 ? 2 : v;
    }();
    return choice;
}
// The per-call CU budget (pio_call_opts_t.cu_budget): thread-local for the duration of one C-ABI call -- the GEMM and
// flash launchers read cu_budget() -- so that two threads driving two encoders never see each other's share.
struct CuBudgetScope {
    int prev;
    explicit CuBudgetScope(const pio_call_opts_t &o) : prev(cu_budget_call(-1)) {
        cu_budget_call(o.cu_budget > 0 ? o.cu_budget : 0);
    }
    ~CuBudgetScope() { cu_budget_call(prev); }
};
static int64_t ln_fold_min_rows(int choice) {
    static const int64_t auto_rows = [] {
        const char *e = getenv("PIO_LN_FOLD_MIN_ROWS");
        const long long v = e ? atoll(e) : 6144;
        return (int64_t)(v < 2048 ? 2048 : v);
    }();
    return choice == 2 ? 2048 : auto_rows;
}
// Below that row count the fold runs on the tile kernels (64-column statistics slots) -- from this many rows on
// (env PIO_LN_FOLD_SMALL_MIN_ROWS; mode 2: from 128 rows).
static int64_t ln_fold_small_min_rows(int choice) {
    static const int64_t auto_rows = [] {
        const char *e = getenv("PIO_LN_FOLD_SMALL_MIN_ROWS");
        const long long v = e ? atoll(e) : 512;
        return (int64_t)(v < 128 ? 128 : v);
    }();
    return choice == 2 ? 128 : auto_rows;
}
static int64_t ln_fold_small_max_rows() {
    static const int64_t max_rows = [] {
        const char *e = getenv("PIO_LN_FOLD_SMALL_MAX_ROWS");
        return (int64_t)(e ? atoll(e) : 4096);
    }();
    return max_rows;
}
// Every switch of the fold as the plain values pio_block_route.h takes; filled once per C-ABI call.  The mode is the
// call's own (pio_call_opts_t.ln_fold: 1 = off, 2 = where it pays, 3 = wherever offered) or, with 0, the process-wide one.
static FoldKnobs fold_knobs(const pio_call_opts_t &o) {
    const int choice = (o.ln_fold >= 1 && o.ln_fold <= 3) ? o.ln_fold - 1 : ln_fold_global();
    return FoldKnobs{choice, ln_fold_min_rows(choice), ln_fold_small_min_rows(choice), ln_fold_small_max_rows()};
}

// Carried from one SelfAttention block to the next inside a stack: the 16-bit copy and the partial sums of the block's
// INPUT, left in the plan's (x16, part_a) buffers by the previous block's fc2 GEMM.
struct FoldCarry {
    const void *x = nullptr;  // the fp32 tensor they describe (its CONTENT is stale unless f32_valid)
    const void *x16 = nullptr;
    const float *part = nullptr;
    bool f32_valid = true;
};

struct SelfExtras {  // what the encoder stack adds to one self_attention_run call (the default value: a block on its own)
    FoldCarry *carry = nullptr;
    bool need_f32_out = true;  // false: a folded block inside a stack leaves `out` unwritten (the pair carries the stream)
};
static int self_attention_run(const pio_self_attention_t &sa, const pio_tensor3_t &x, const AttnOptional &opt, float *out,
                              SelfPlan &p, const FoldKnobs &knobs, const SelfExtras &e, hipStream_t s) {
    FoldCarry *const carry = e.carry;
    const int B = x.B, N = x.T;
    const int64_t rows = (int64_t)B * N;
    if (x.C != sa.attn.q_in || sa.attn.k_in != x.C || sa.attn.v_in != x.C || sa.attn.out != x.C ||
        sa.mlp.in != x.C || sa.mlp.out != x.C)
        return PIO_E_SHAPE;  // residual adds need matching widths (the reference raises a RuntimeError)
    SelfCall call = {};
    call.B = B; call.N = N; call.C = x.C; call.stride_t = x.stride_t; call.stride_b = x.stride_b;
    call.x_aligned16 = (((uintptr_t)x.data) & 15) == 0; call.has_fold_buffers = p.x16b != nullptr;
    note_optional(call, opt);
    const SelfFold fold = self_fold_route(sa, call, knobs);
    if (fold.family != SelfFold::NONE) {
        // x16 / part_a: the block input (from the previous block's fc2, or computed here for the first block)
        // Inside the fold the residual stream is the 16-bit pair (x16, lo): 22 mantissa bits, and 64 MB less traffic
        // per residual GEMM than fp32 + copy.  The fp32 form is read here once (first block) and written when the
        // caller needs it (last block).
        if (!(carry && carry->x == x.data && carry->x16 == p.x16.hi && carry->part == p.part_a)) {
            if (carry && !carry->f32_valid) return PIO_E_ARG;  // (the stack decides the fold for all its blocks)
            PIO_TRY(rowstats_cast_launch(x.data, rows, x.C, fold.slot_w, p.x16.hi, p.lo_a, p.part_a, sa.attn.dtype, s));
            PIO_RANGE(PIO_RK_STREAM, sa.attn.dtype, p.x16.hi, rows, x.C, x.C, 1, 0, s);
        }
        const Pair xa = {p.x16.hi, nullptr};
        LnFold f_qkv, f_out, f_fc1, f_fc2;
        f_qkv.in_part = p.part_a; f_qkv.w = &sa.fold.qkv; f_qkv.c = sa.fold.qkv_c; f_qkv.eps = sa.ln1.eps;
        f_out.out16 = p.x16b; f_out.ld16 = x.C; f_out.out_part = p.part_b;
        f_out.out16_lo = p.lo_b; f_out.res16_hi = p.x16.hi; f_out.res16_lo = p.lo_a;
        f_out.range_flag = f_fc2.range_flag = sa.fold.range_flag;
        f_qkv.in_slots = f_fc1.in_slots = fold.nslots;
        f_out.slot_w = f_fc2.slot_w = fold.slot_w;
        f_fc1.in_part = p.part_b; f_fc1.w = &sa.fold.fc1; f_fc1.c = sa.fold.fc1_c; f_fc1.eps = sa.ln2.eps;
        f_fc2.out16 = p.x16.hi; f_fc2.ld16 = x.C; f_fc2.out_part = p.part_a;
        f_fc2.out16_lo = p.lo_a; f_fc2.res16_hi = p.x16b; f_fc2.res16_lo = p.lo_b;
        const Residual rx = residual_of(x);
        AttnExtras ax;
        ax.res = &rx; ax.fold_in = &f_qkv; ax.fold_out = &f_out;
        // (the fold is taken without optional operands only; x1 exists as the pair (x16b, lo_b) only: no fp32 `out`)
        PIO_TRY(attention_core(sa.attn, xa, false, xa, xa, B, N, N, AttnOptional(), nullptr, p.core, ax, s));
        pio_tensor3_t t1 = {p.x1, (int64_t)N * x.C, x.C, B, N, x.C};
        const Pair xm = {p.x16b, nullptr};
        const Residual r1 = residual_of(t1);
        MlpExtras mx;
        mx.res = &r1; mx.fold_in = &f_fc1; mx.fold_out = &f_fc2;
        PIO_TRY(mlp_core(sa.mlp, xm, rows, p.h16, e.need_f32_out ? out : nullptr, mx, s));
        if (carry) {
            carry->x = out;
            carry->x16 = p.x16.hi;
            carry->part = p.part_a;
            carry->f32_valid = e.need_f32_out;
        }
        return PIO_OK;
    }
    if (carry) {
        if (!carry->f32_valid) return PIO_E_ARG;  // (the stack decides the fold for all its blocks)
        *carry = FoldCarry();
    }
    // LN1 -> attention -> + x     (transformer_primitives.py:281-290)
    const Pair xa = pair_if(p.x16, sa.attn.act_split);
    PIO_TRY(cast_pair(x, &sa.ln1, xa, padc(x.C), sa.attn.dtype, PIO_RK_CAST, s));
    const Residual rx = residual_of(x);
    AttnExtras ax;
    ax.res = &rx;
    PIO_TRY(attention_core(sa.attn, xa, false, xa, xa, B, N, N, opt, p.x1, p.core, ax, s));
    // LN2 -> MLP -> + x1          (transformer_primitives.py:292)
    pio_tensor3_t t1 = {p.x1, (int64_t)N * x.C, x.C, B, N, x.C};
    const Pair xm = pair_if(p.x16, sa.mlp.act_split);
    PIO_TRY(cast_pair(t1, &sa.ln2, xm, padc(x.C), sa.mlp.dtype, PIO_RK_CAST, s));
    const Residual r1 = residual_of(t1);
    MlpExtras mx;
    mx.res = &r1;
    return mlp_core(sa.mlp, xm, rows, p.h16, out, mx, s);
}

// ikv_tail (optional): the key / value input arrives as TWO arrays whose channels are concatenated, [ikv | ikv_tail]
// (ikv_tail->B == 1: one batch-invariant table, e.g. Fourier position features); layer_norm_kv runs over the virtual
// concatenation and nothing is ever concatenated in HBM.  iq_tail (optional, blocks without a query residual): the same
// for the query rows, [iq | iq_tail] under layer_norm_q (the dense decoders whose queries ARE the network's input).
struct CrossExtras {  // what the encoder / decoder add to one cross_attention_run call (the default value: none of it)
    const pio_tensor3_t *ikv_tail = nullptr, *iq_tail = nullptr;
    int64_t out_ld = 0;           // row pitch of `out` (0: the query channels)
    const QCache *qc = nullptr;
    const Pair *out16 = nullptr;  // the result leaves as 16-bit operand rows instead (mlp_core)
};
static int cross_attention_run(const pio_cross_attention_t &ca, const pio_tensor3_t &iq, const pio_tensor3_t &ikv,
                               const AttnOptional &opt, float *out, CrossPlan &p, const CrossExtras &e, hipStream_t s) {
    const pio_tensor3_t *ikv_tail = e.ikv_tail, *iq_tail = e.iq_tail;
    const int B = iq.B, Tq = iq.T, Tk = ikv.T;
    const int64_t rows = (int64_t)B * Tq;
    const int kv_c = ikv.C + (ikv_tail ? ikv_tail->C : 0);
    const int q_c = iq.C + (iq_tail ? iq_tail->C : 0);
    if (q_c != ca.attn.q_in || kv_c != ca.attn.k_in || kv_c != ca.attn.v_in || ikv.B != B) return PIO_E_SHAPE;
    if (ca.attn.out != q_c || ca.mlp.in != q_c || ca.mlp.out != q_c) return PIO_E_SHAPE;
    if (iq_tail && (ca.use_query_residual || e.qc || p.q_bcast)) return PIO_E_ARG;  // (the rows themselves are needed then)
    // layer_norm_kv, layer_norm_q  (transformer_primitives.py:379-380)
    if (ikv_tail) {
        PIO_TRY(layernorm_cast_cat_launch(ikv, *ikv_tail, ca.ln_kv, p.kv16.hi, p.kv16.lo, padc(kv_c), ca.attn.dtype, s));
        PIO_RANGE(PIO_RK_CAST, ca.attn.dtype, p.kv16.hi, (int64_t)B * Tk, kv_c, padc(kv_c), 1, 0, s);
    } else
        PIO_TRY(cast_pair(ikv, &ca.ln_kv, p.kv16, padc(ikv.C), ca.attn.dtype, PIO_RK_CAST, s));
    const pio_tensor3_t q1 = p.q_bcast ? first_batch(iq) : iq;
    const Pair qa = pair_if(p.q16, ca.attn.act_split);
    if (e.qc && ca.use_query_residual) return PIO_E_ARG;  // (the query rows themselves are needed then)
    if (iq_tail) {
        PIO_TRY(layernorm_cast_cat_launch(iq, *iq_tail, ca.ln_q, qa.hi, qa.lo, padc(q_c), ca.attn.dtype, s));
        PIO_RANGE(PIO_RK_CAST, ca.attn.dtype, qa.hi, rows, q_c, padc(q_c), 1, 0, s);
    } else if (!(e.qc && e.qc->valid)) PIO_TRY(cast_pair(q1, &ca.ln_q, qa, padc(q_c), ca.attn.dtype, PIO_RK_CAST, s));
    const Residual rq = residual_of(iq);
    AttnExtras ax;
    ax.res = ca.use_query_residual ? &rq : nullptr; ax.out_ld = pitch8(q_c); ax.qc = e.qc;
    PIO_TRY(attention_core(ca.attn, qa, p.q_bcast, p.kv16, p.kv16, B, Tq, Tk, opt, p.x1, p.core, ax, s));
    // x + MLP(LN2(x))  (transformer_primitives.py:401)
    pio_tensor3_t t1 = {p.x1, (int64_t)Tq * pitch8(q_c), pitch8(q_c), B, Tq, q_c};
    const Pair qm = pair_if(p.q16, ca.mlp.act_split);
    PIO_TRY(cast_pair(t1, &ca.ln2, qm, padc(q_c), ca.mlp.dtype, PIO_RK_CAST, s));
    const Residual r1 = residual_of(t1);
    MlpExtras mx;
    mx.res = &r1; mx.out_ld = e.out_ld; mx.out16 = e.out16;
    return mlp_core(ca.mlp, qm, rows, p.h16, out, mx, s);
}

// Range probe: the part label (pio_range_probe_mark) an entry point changes on its way, restored when it returns.
struct RangePart {
    bool changed = false;
    int prev = 0;
    void set(int part) {
        if (!range_probe_active()) return;
        const int was = range_probe_mark(part);
        if (!changed) prev = was;
        changed = true;
    }
    ~RangePart() {
        if (changed) range_probe_mark(prev);
    }
};

}  // namespace pio

using namespace pio;

extern "C" {

size_t pio_attention_workspace_bytes(const pio_attention_t *a, int32_t B, int32_t Tq, int32_t Tk) {
    if (!a) return 0;
    AttentionPlan p;
    const bool q_bcast = false, same_kv = false;  // (the larger plan: per-sample queries, k and v cast apart)
    return p.carve(nullptr, *a, B, Tq, Tk, q_bcast, same_kv);
}

int pio_attention_fwd(const pio_attention_t *a, const pio_tensor3_t *iq, const pio_tensor3_t *ik,
                      const pio_tensor3_t *iv, const uint8_t *kv_mask, const uint8_t *q_mask,
                      const uint8_t *full_mask, const float *attention_bias, float *out, float *probs_out,
                      void *workspace, size_t workspace_bytes, void *stream) {
    if (!a || !iq || !ik || !iv || !out || !workspace) return PIO_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (iq->C != a->q_in || ik->C != a->k_in || iv->C != a->v_in) return PIO_E_SHAPE;
    if (ik->B != iq->B || iv->B != iq->B || ik->T != iv->T) return PIO_E_SHAPE;
    const int B = iq->B, Tq = iq->T, Tk = ik->T;
    const bool qb = (iq->stride_b == 0 && B > 1);
    const bool same = same_tensor(*ik, *iv);
    AttentionPlan p;
    if (p.carve(workspace, *a, B, Tq, Tk, qb, same) > workspace_bytes) return PIO_E_WORKSPACE;
    const pio_tensor3_t q1 = qb ? first_batch(*iq) : *iq;
    PIO_TRY(cast_pair(q1, nullptr, p.xq16, padc(a->q_in), a->dtype, PIO_RK_CAST, s));
    PIO_TRY(cast_pair(*ik, nullptr, p.xk16, padc(a->k_in), a->dtype, PIO_RK_CAST, s));
    if (!same) PIO_TRY(cast_pair(*iv, nullptr, p.xv16, padc(a->v_in), a->dtype, PIO_RK_CAST, s));
    const AttnOptional opt = {kv_mask, q_mask, full_mask, attention_bias, probs_out};
    return attention_core(*a, p.xq16, qb, p.xk16, p.xv16, B, Tq, Tk, opt, out, p.core, AttnExtras(), s);
}

// ======================================================================================================
// MLP.forward
// ======================================================================================================
size_t pio_mlp_workspace_bytes(const pio_mlp_t *m, int64_t rows) {
    if (!m) return 0;
    MlpPlan p;
    return p.carve(nullptr, *m, rows);
}

int pio_mlp_fwd(const pio_mlp_t *m, const pio_tensor3_t *x, float *out, void *workspace, size_t workspace_bytes,
                void *stream) {
    if (!m || !x || !out || !workspace) return PIO_E_ARG;
    if (x->C != m->in) return PIO_E_SHAPE;
    const int64_t rows = (int64_t)x->B * x->T;
    MlpPlan p;
    if (p.carve(workspace, *m, rows) > workspace_bytes) return PIO_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    PIO_TRY(cast_pair(*x, nullptr, p.x16, padc(m->in), m->dtype, PIO_RK_CAST, s));
    return mlp_core(*m, p.x16, rows, p.h16, out, MlpExtras(), s);
}

// ======================================================================================================
// SelfAttention.forward / CrossAttention.forward
// ======================================================================================================
int pio_ln_fold_enable(int on) {
    int &c = ln_fold_global();
    const int prev = c;
    c = on < 0 ? 0 : on > 2 ? 2 : on;
    return prev;
}

size_t pio_self_attention_workspace_bytes(const pio_self_attention_t *sa, int32_t B, int32_t N) {
    if (!sa) return 0;
    SelfPlan p;
    return p.carve(nullptr, *sa, B, N);
}

int pio_self_attention_fwd(const pio_self_attention_t *sa, const pio_tensor3_t *x, const uint8_t *kv_mask,
                           const uint8_t *q_mask, const uint8_t *full_mask, const float *attention_bias, float *out,
                           float *probs_out, const pio_call_opts_t *opts, void *workspace, size_t workspace_bytes,
                           void *stream) {
    if (!sa || !x || !out || !workspace) return PIO_E_ARG;
    const pio_call_opts_t o = opts ? *opts : pio_call_opts_t{};
    CuBudgetScope scope(o);
    SelfPlan p;
    if (p.carve(workspace, *sa, x->B, x->T) > workspace_bytes) return PIO_E_WORKSPACE;
    const AttnOptional opt = {kv_mask, q_mask, full_mask, attention_bias, probs_out};
    return self_attention_run(*sa, *x, opt, out, p, fold_knobs(o), SelfExtras(), (hipStream_t)stream);
}

size_t pio_cross_attention_workspace_bytes(const pio_cross_attention_t *ca, int32_t B, int32_t Tq, int32_t Tk) {
    if (!ca) return 0;
    CrossPlan p;
    const bool q_bcast = false;  // (the larger plan: per-sample queries)
    return p.carve(nullptr, *ca, B, Tq, Tk, q_bcast);
}

int pio_cross_attention_fwd(const pio_cross_attention_t *ca, const pio_tensor3_t *iq, const pio_tensor3_t *ikv,
                            const uint8_t *kv_mask, const uint8_t *q_mask, const uint8_t *full_mask,
                            const float *attention_bias, float *out, float *probs_out, void *workspace,
                            size_t workspace_bytes, void *stream) {
    if (!ca || !iq || !ikv || !out || !workspace) return PIO_E_ARG;
    CrossPlan p;
    const bool qb = (iq->stride_b == 0 && iq->B > 1);
    if (p.carve(workspace, *ca, iq->B, iq->T, ikv->T, qb) > workspace_bytes) return PIO_E_WORKSPACE;
    const AttnOptional opt = {kv_mask, q_mask, full_mask, attention_bias, probs_out};
    return cross_attention_run(*ca, *iq, *ikv, opt, out, p, CrossExtras(), (hipStream_t)stream);
}

// ======================================================================================================
// PerceiverEncoder.forward
// ======================================================================================================
size_t pio_encoder_workspace_bytes(const pio_cross_attention_t *cross, const pio_self_attention_t *layers, int32_t L,
                                   int32_t B, int32_t M, int32_t N) {
    if (!cross) return 0;
    CrossPlan cp;
    size_t need = cp.carve(nullptr, *cross, B, N, M, false, true);
    for (int l = 0; l < L; ++l) {
        SelfPlan sp;
        const size_t n = sp.carve(nullptr, layers[l], B, N, true);
        if (n > need) need = n;
    }
    return need;
}

int pio_encoder_fwd(const pio_encoder_call_t *c, void *workspace, size_t workspace_bytes, void *stream) {
    if (!c || !c->cross || !c->inputs || !c->latents || !c->out || !workspace || (c->L > 0 && !c->layers)) return PIO_E_ARG;
    const pio_tensor3_t *inputs = c->inputs, *latents = c->latents;
    const int L = c->L, num_blocks = c->num_blocks;
    float *const out = c->out;
    CuBudgetScope scope(c->opts);
    if (L < 0 || num_blocks < 0) return PIO_E_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    const int B = inputs->B, M = inputs->T, N = latents->T, D = latents->C;
    if (latents->B != B) return PIO_E_SHAPE;
    if (pio_encoder_workspace_bytes(c->cross, c->layers, L, B, M, N) > workspace_bytes) return PIO_E_WORKSPACE;
    RangePart range_part;  // range probe: the cross-attend keeps the caller's part, the stack is marked here
    {
        CrossPlan cp;
        const bool qb = (latents->stride_b == 0 && B > 1);
        cp.carve(workspace, *c->cross, B, N, M, qb, true);
        // perceiver.py:99-103: only the cross-attend is masked, with mask[b,i,j] = input_mask[b,j]
        AttnOptional opt;
        opt.kv_mask = c->input_mask;
        CrossExtras cx;
        cx.ikv_tail = c->inputs_tail;
        PIO_TRY(cross_attention_run(*c->cross, *latents, *inputs, opt, out, cp, cx, s));
    }
    const pio_tensor3_t z = {out, (int64_t)N * D, D, B, N, D};
    range_part.set(PIO_RP_STACK);
    const FoldKnobs knobs = fold_knobs(c->opts);
    FoldCarry carry;  // LayerNorm fold: the row statistics of z travel from one block's fc2 to the next block's q|k|v
    for (int blk = 0; blk < num_blocks; ++blk) {  // perceiver.py:104-106: weights shared across blocks
        for (int l = 0; l < L; ++l) {
            // (per_block: block blk has its own IMAGES of the shared parameters -- same shapes -- at layers[blk * L + l])
            const pio_self_attention_t &lay = c->layers[(c->per_block ? (size_t)blk * L : 0) + l];
            SelfPlan sp;
            sp.carve(workspace, lay, B, N, true);
            SelfExtras sx;
            sx.carry = &carry;
            sx.need_f32_out = blk == num_blocks - 1 && l == L - 1;  // (the last block of the stack)
            PIO_TRY(self_attention_run(lay, z, AttnOptional(), out, sp, knobs, sx, s));
        }
    }
    return PIO_OK;
}

// ======================================================================================================
// PerceiverDecoder.forward
// ======================================================================================================
size_t pio_decoder_workspace_bytes(const pio_cross_attention_t *cross, const pio_linear_t *final_layer, int32_t B,
                                   int32_t Q, int32_t N) {
    if (!cross) return 0;
    DecoderPlan p;
    return p.carve(nullptr, *cross, final_layer, B, Q, N, false);
}

size_t pio_decoder_qcache_bytes(const pio_cross_attention_t *cross, int32_t Bq, int32_t Q) {
    if (!cross || Bq <= 0 || Q <= 0) return 0;
    return (size_t)round_up((int64_t)Bq * Q * cross->attn.heads * cross->attn.dkp * 2, 256);
}

int pio_decoder_fwd(const pio_decoder_call_t *c, void *workspace, size_t workspace_bytes, void *stream) {
    if (!c || !c->cross || !c->query || !c->latents || !c->out || !workspace) return PIO_E_ARG;
    const pio_cross_attention_t *cross = c->cross;
    const pio_linear_t *final_layer = c->final_layer;
    const pio_tensor3_t *query = c->query, *query_tail = c->query_tail, *latents = c->latents;
    float *const out = c->out;
    const int q_c = query->C + (query_tail ? query_tail->C : 0);
    QCache qcache{{c->q16_hi, c->q16_lo}, c->q16_valid != 0};
    const QCache *qc = c->q16_hi ? &qcache : nullptr;
    if (qc && (((uintptr_t)c->q16_hi & 15) || ((uintptr_t)c->q16_lo & 15))) return PIO_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int B = query->B, Q = query->T, N = latents->T;
    if (latents->B != B) return PIO_E_SHAPE;
    DecoderPlan p;
    const bool qb = (query->stride_b == 0 && B > 1);
    if (p.carve(workspace, *cross, final_layer, B, Q, N, qb) > workspace_bytes) return PIO_E_WORKSPACE;
    // perceiver.py:172-177: mask[b,i,j] = query_mask[b,i]
    float *y = final_layer ? p.y : out;
    const int64_t y_ld = final_layer ? pitch4(q_c) : q_c;  // (y is internal when a final layer follows)
    // (with a final Linear the cross-attend's result is only ever its operand: fc2 writes it as 16-bit rows directly)
    const bool direct = decoder_y16_direct(final_layer, q_c);
    AttnOptional opt;
    opt.q_mask = c->query_mask;
    CrossExtras cx;
    cx.iq_tail = query_tail; cx.out_ld = y_ld; cx.qc = qc; cx.out16 = direct ? &p.y16 : nullptr;
    PIO_TRY(cross_attention_run(*cross, *query, *latents, opt, y, p.cp, cx, s));
    if (!final_layer) return PIO_OK;
    // perceiver.py:178-179: final nn.Linear on every query row
    if (final_layer->k != padc(q_c)) return PIO_E_SHAPE;
    const pio_tensor3_t ty = {y, (int64_t)Q * y_ld, y_ld, B, Q, q_c};
    if (!direct) PIO_TRY(cast_pair(ty, nullptr, p.y16, padc(q_c), cross->attn.dtype, PIO_RK_STREAM, s));
    return linear_fwd(*final_layer, cross->attn.dtype, p.y16, (int64_t)B * Q, f32_at(out, c->final_out, c->final_out), s);
}

}  // extern "C"
