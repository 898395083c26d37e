"""CPU: the workspace layout of every block entry point, the LayerNorm-fold decision of a SelfAttention block and the
decoder's "fc2 writes the 16-bit operand" choice (perceiverio_pytorch_amd/csrc/pio_block_route.h, compiled with g++ into a
small driver; descriptors and the workspace base are fake, aligned pointers that are never dereferenced).  Every plan
line is `total bytes, member=offset from the base ...` (-1: not carved; equal offsets: an alias).  The expected values
were produced by the structs and the fold expression this header replaced (pasted into a driver of the same cases) and
the byte totals also by the pio_*_workspace_bytes entry points of the library before the move; a sweep of old against
new over 1.5e9 fold calls and 8.9e6 plans showed no disagreement.  The tables are a readable extract of it.

The same for the GEMM descriptor of one nn.Linear (linear_gemm, LINEARS below): expected values from the body of
pio_blocks.hip's linear_fwd before it moved here, run on the same cases; a sweep of old against new over randomised
arguments (widths 1..2048, pitches, residual, fold, n_store16) showed no disagreement."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''
#include <stdio.h>
#include <string.h>
#include "pio_block_route.h"
using namespace pio;

static const void *W = (const void *)(uintptr_t)0x10000000;   // a fake, aligned pointer: never dereferenced
static char *const BASE = (char *)(uintptr_t)0x40000000;      // the fake workspace

// ---- descriptors as the Python front end packs them (runtime.py PackedLinear / PackedStack, _POLICIES) ---------------
// (one constant per policy the cases use, written by _policies_cpp() from the answers of runtime.py itself)
struct Policy { bool q, k, v, o, fc1, fc2, final_layer, split; int act_split; bool kv_fold, ln_fold, qkv_stack; };
@POLICIES@
static pio_linear_t lin(int n, int k, bool two, int lo_row0 = 0) {
    pio_linear_t l = {};
    l.w_hi = W; l.w_lo = two ? W : nullptr; l.n = n; l.k = k; l.lo_row0 = two ? lo_row0 : 0;
    return l;
}
// transformer_primitives.py Attention._build_desc
static pio_attention_t attn(const Policy &p, int H, int q_in, int kv_in, int qk, int v, int out) {
    pio_attention_t a = {};
    const int dk = qk / H, dv = v / H, dkp = pad8(dk), dvp = pad8(dv);
    a.heads = H; a.dk = dk; a.dv = dv; a.dkp = dkp; a.dvp = dvp; a.q_in = q_in; a.k_in = a.v_in = kv_in; a.out = out;
    a.dtype = PIO_DT_F16; a.act_split = p.act_split;
    a.q = lin(H * dkp, padc(q_in), p.q); a.k = lin(H * dkp, padc(kv_in), p.k); a.v = lin(H * dvp, padc(kv_in), p.v);
    a.o = lin(pad8(out), H * dvp, p.o);
    if (H == 1 && dk == kv_in && dv == kv_in && p.kv_fold) {   // K / V projection fold offered
        a.kq = lin(pad8(kv_in), pad8(qk), true); a.vo = lin(pad8(out), pad8(kv_in), true);
    }
    if (q_in == kv_in && !p.split) {
        a.qk = lin(2 * H * dkp, padc(q_in), p.q && p.k);
        const bool fused_head = (dkp == 128 && dvp == 128) || (dkp == 64 && dvp == 64) || (dkp == 32 && dvp == 32) ||
                                (dkp == 32 && dvp == 160);       // FUSED_SELF_HEADS
        if (p.qkv_stack && fused_head && (!p.v || (2 * H * dkp) % 256 == 0))
            a.qkv = lin(2 * H * dkp + H * dvp, padc(q_in), p.v, 2 * H * dkp);
    }
    return a;
}
// MLP._build_desc
static pio_mlp_t mlp(const Policy &p, int in, int widening, int out) {
    pio_mlp_t m = {};
    m.in = in; m.hidden = widening * in; m.out = out; m.dtype = PIO_DT_F16; m.act_split = p.split;
    m.fc1 = lin(padc(m.hidden), padc(in), p.fc1); m.fc2 = lin(pad8(out), padc(m.hidden), p.fc2);
    return m;
}
// SelfAttention._build_desc + _build_ln_fold
static pio_self_attention_t self_block(const Policy &p, int C, int H, int qk = 0, int v = 0, int widening = 1) {
    pio_self_attention_t sa = {};
    qk = qk ? qk : C; v = v ? v : qk;
    sa.attn = attn(p, H, C, C, qk, v, v);
    sa.mlp = mlp(p, v, widening, v);
    if (!(!p.ln_fold || C % 256 || C < 512 || C > 1536 || !sa.attn.qkv.w_hi || widening != 1 || v != C)) {
        sa.fold.qkv = lin(sa.attn.qkv.n, padc(C), p.v, 2 * H * sa.attn.dkp);
        sa.fold.fc1 = lin(padc(C), padc(C), p.fc1);
        sa.fold.qkv_c = sa.fold.fc1_c = (const float *)W;
    }
    return sa;
}
// CrossAttention.__init__ / _desc (shape_for_attn "kv": qk channels default to the key / value input's)
static pio_cross_attention_t cross_block(const Policy &p, int q_in, int kv_in, int H, int qk = 0, int v = 0,
                                         bool residual = true) {
    pio_cross_attention_t ca = {};
    qk = qk ? qk : kv_in; v = v ? v : qk;
    ca.attn = attn(p, H, q_in, kv_in, qk, v, q_in);
    ca.mlp = mlp(p, q_in, 1, q_in);
    ca.use_query_residual = residual;
    return ca;
}
// PerceiverDecoder._final_desc: nn.Linear(query channels, outputs)
static pio_linear_t final_layer(const Policy &p, int q_c, int out) { return lin(pad8(out), padc(q_c), p.final_layer); }

// ---- printing ------------------------------------------------------------------------------------------------------
static long long off(const void *p) { return p ? (long long)((const char *)p - BASE) : -1; }
static void pair(const char *n, const Pair &p) { printf(" %s.hi=%lld %s.lo=%lld", n, off(p.hi), n, off(p.lo)); }
// (qbytes / kbytes: the un-rounded sizes of q16.hi and k16.hi, for the adjacency invariant)
static void core(const AttnScratch &w, const pio_attention_t &a, int Bq, int B, int Tq, int Tk) {
    pair("core.q16", w.q16); pair("core.k16", w.k16); pair("core.vt16", w.vt16);
    printf(" core.scores=%lld", off(w.scores));
    pair("core.p16", w.p16); pair("core.o16", w.o16);
    printf(" core.xpart=%lld split=%d qbytes=%lld kbytes=%lld", off(w.xpart), a.act_split != 0,
           (long long)Bq * Tq * a.heads * a.dkp * 2, (long long)B * Tk * a.heads * a.dkp * 2);
}
static void show_attention(const char *id, const pio_attention_t &a, int B, int Tq, int Tk, bool qb, bool same) {
    AttentionPlan p, n;
    const size_t total = p.carve(BASE, a, B, Tq, Tk, qb, same);
    printf("plan %s total=%zu null_base_total=%zu", id, total, n.carve(nullptr, a, B, Tq, Tk, qb, same));
    pair("xq16", p.xq16); pair("xk16", p.xk16); pair("xv16", p.xv16);
    core(p.core, a, qb ? 1 : B, B, Tq, Tk);
    printf("\n");
}
static void show_mlp(const char *id, const pio_mlp_t &m, int64_t rows) {
    MlpPlan p, n;
    const size_t total = p.carve(BASE, m, rows);
    printf("plan %s total=%zu null_base_total=%zu", id, total, n.carve(nullptr, m, rows));
    pair("x16", p.x16); pair("h16", p.h16);
    printf("\n");
}
static void show_self(const char *id, const pio_self_attention_t &sa, int B, int N, bool lean) {
    SelfPlan p, n;
    const size_t total = p.carve(BASE, sa, B, N, lean);
    printf("plan %s total=%zu null_base_total=%zu", id, total, n.carve(nullptr, sa, B, N, lean));
    pair("x16", p.x16); pair("h16", p.h16);
    printf(" x1=%lld", off(p.x1));
    core(p.core, sa.attn, B, B, N, N);
    printf(" x16b=%lld lo_a=%lld lo_b=%lld part_a=%lld part_b=%lld\n", off(p.x16b), off(p.lo_a), off(p.lo_b),
           off(p.part_a), off(p.part_b));
}
static void cross_members(const CrossPlan &p, const pio_cross_attention_t &ca, int B, int Tq, int Tk, bool qb) {
    pair("q16", p.q16); pair("kv16", p.kv16); pair("h16", p.h16);
    printf(" x1=%lld", off(p.x1));
    core(p.core, ca.attn, qb ? 1 : B, B, Tq, Tk);
}
static void show_cross(const char *id, const pio_cross_attention_t &ca, int B, int Tq, int Tk, bool qb, bool lean) {
    CrossPlan p, n;
    const size_t total = p.carve(BASE, ca, B, Tq, Tk, qb, lean);
    printf("plan %s total=%zu null_base_total=%zu", id, total, n.carve(nullptr, ca, B, Tq, Tk, qb, lean));
    cross_members(p, ca, B, Tq, Tk, qb);
    printf("\n");
}
// (pitch4 / pad8 / padc of the query channels: the pitches of y, of a 16-bit row at the 8-element pitch, and of y16)
static void show_decoder(const char *id, const pio_cross_attention_t &ca, const pio_linear_t *fin, int B, int Q, int N,
                         bool qb) {
    DecoderPlan p, n;
    const size_t total = p.carve(BASE, ca, fin, B, Q, N, qb);
    printf("plan %s total=%zu null_base_total=%zu y=%lld", id, total, n.carve(nullptr, ca, fin, B, Q, N, qb), off(p.y));
    pair("y16", p.y16);
    cross_members(p.cp, ca, B, Q, N, qb);
    printf(" pitch4=%d pad8=%d padc=%d y16_direct=%d\n", pitch4(ca.attn.q_in), pad8(ca.attn.q_in), padc(ca.attn.q_in),
           decoder_y16_direct(fin, ca.attn.q_in));
}
// pio_encoder_workspace_bytes' rule against what pio_encoder_fwd carves (latents broadcast over the batch or not)
static void show_encoder(const char *id, const pio_cross_attention_t &ca, const pio_self_attention_t &sa, int B, int M,
                         int N) {
    CrossPlan cp; SelfPlan sp;
    size_t rule = cp.carve(nullptr, ca, B, N, M, false, true);
    const size_t n = sp.carve(nullptr, sa, B, N, true);
    if (n > rule) rule = n;
    const size_t run_self = sp.carve(BASE, sa, B, N, true);
    const size_t c0 = cp.carve(BASE, ca, B, N, M, false, true), c1 = cp.carve(BASE, ca, B, N, M, true, true);
    printf("encoder %s %zu %zu %zu\n", id, rule, c0 > run_self ? c0 : run_self, c1 > run_self ? c1 : run_self);
}

static void plan_cases() {
    // The four shipped models at the (B, M, N, Q) and policies of bench.py CONFIGS (= models.py DEFAULT_POLICY); channel
    // and head counts: models.py ClassificationPerceiver / LanguagePerceiver / FlowPerceiver / MultiModalPerceiver
    // imagenet "fp16x2w/fp16sd/fp16x2af": 3136 x 322 inputs, 512 x 1024 latents, 8 heads, 1000 batch-invariant queries
    const pio_cross_attention_t im_x = cross_block(X2W, 1024, 322, 1), im_d = cross_block(X2AF, 1024, 1024, 1);
    const pio_self_attention_t im_s = self_block(FP16, 1024, 8);
    const pio_linear_t im_f = final_layer(X2AF, 1024, 1000);
    show_cross("imagenet_cross", im_x, 32, 512, 3136, true, true);
    show_self("imagenet_stack", im_s, 32, 512, true);
    show_decoder("imagenet_decoder", im_d, &im_f, 32, 1000, 512, true);
    show_encoder("imagenet", im_x, im_s, 32, 3136, 512);
    // language "fp16x2w/fp16x2o/fp16x3f": 2048 x 768 tokens, 256 x 1280 latents, 8 heads of (32, 160); decoder heads (32, 96)
    const pio_cross_attention_t la_x = cross_block(X2W, 1280, 768, 8, 256, 1280), la_d = cross_block(X3F, 768, 1280, 8, 256, 768, false);
    const pio_self_attention_t la_s = self_block(X2O, 1280, 8, 256, 1280);
    show_cross("language_cross", la_x, 100, 256, 2048, true, true);
    show_self("language_stack", la_s, 100, 256, true);
    show_decoder("language_decoder", la_d, nullptr, 100, 2048, 256, false);
    show_encoder("language", la_x, la_s, 100, 2048, 256);
    // flow "fp16/fp16x2af": 182 528 x 322 pixels, 2048 x 512 latents, 16 heads of 32; the queries are the inputs
    const pio_cross_attention_t fl_x = cross_block(FP16, 512, 322, 1), fl_d = cross_block(X2AF, 322, 512, 1, 0, 0, false);
    const pio_self_attention_t fl_s = self_block(FP16, 512, 16);
    const pio_linear_t fl_f = final_layer(X2AF, 322, 2);
    show_cross("flow_cross", fl_x, 1, 2048, 182528, true, true);
    show_self("flow_stack", fl_s, 1, 2048, true);
    show_decoder("flow_decoder_322", fl_d, &fl_f, 1, 182528, 2048, false);
    show_decoder("flow_decoder_322_no_final", fl_d, nullptr, 1, 182528, 2048, false);
    show_encoder("flow", fl_x, fl_s, 1, 182528, 2048);
    // multimodal "fp16x2w/fp16x2afo": 52 097 x 704 inputs, 784 x 512 latents, 8 heads of 64, chunks of 6288 x 1026 queries
    const pio_cross_attention_t mm_x = cross_block(X2W, 512, 704, 1), mm_d = cross_block(X2AFO, 1026, 512, 1, 0, 0, false);
    const pio_self_attention_t mm_s = self_block(X2W, 512, 8);
    const pio_linear_t mm_f = final_layer(X2AFO, 1026, 512);
    show_cross("multimodal_cross", mm_x, 1, 784, 52097, true, true);
    show_self("multimodal_stack", mm_s, 1, 784, true);
    show_decoder("multimodal_decoder_1026", mm_d, &mm_f, 1, 6288, 784, false);
    show_decoder("multimodal_decoder_1026_no_final", mm_d, nullptr, 1, 6288, 784, false);
    show_encoder("multimodal", mm_x, mm_s, 1, 52097, 784);

    // act_split 0 / 1 / 2 / 3 on one small block of each kind
    const Policy *pol[4] = {&FP16, &X3, &X3F, &X3FQ};
    for (int s = 0; s < 4; ++s) {
        char id[64];
        snprintf(id, sizeof id, "self_512_act_split_%d", s);
        show_self(id, self_block(*pol[s], 512, 16), 2, 256, false);
        snprintf(id, sizeof id, "cross_act_split_%d", s);
        show_cross(id, cross_block(*pol[s], 256, 96, 8, 256, 256), 2, 128, 200, false, false);
        snprintf(id, sizeof id, "attention_act_split_%d", s);
        show_attention(id, attn(*pol[s], 8, 256, 96, 256, 256, 256), 2, 128, 200, false, true);
        snprintf(id, sizeof id, "mlp_act_split_%d", s);
        show_mlp(id, mlp(*pol[s], 322, 4, 322), 300);
    }
    show_attention("attention_v_apart_q_bcast", attn(FP16, 8, 256, 96, 256, 256, 256), 2, 128, 200, true, false);
    // lean on / off, q_bcast on / off
    show_self("imagenet_stack_b1_not_lean", im_s, 1, 512, false);
    show_self("imagenet_stack_b1_lean", im_s, 1, 512, true);
    show_cross("flow_cross_b2_small_not_lean", fl_x, 2, 256, 1000, false, false);
    show_cross("flow_cross_b2_small_lean", fl_x, 2, 256, 1000, false, true);
    show_cross("flow_cross_b2_small_lean_q_bcast", fl_x, 2, 256, 1000, true, true);
    show_decoder("imagenet_decoder_b2", im_d, &im_f, 2, 1000, 512, false);
    show_decoder("imagenet_decoder_b2_q_bcast", im_d, &im_f, 2, 1000, 512, true);
    // the in-place stream (policy with split weights: the fold's buffers are carved all the same)
    show_self("imagenet_stack_b4_inplace", im_s, 4, 512, true);
    show_self("stack_x2w_1024_inplace", self_block(X2W, 1024, 8), 4, 512, true);
    // h16.hi == core.o16.hi at its edge: padc(hidden) == heads * dvp (1280 = 8 x 160) / greater (widening 4: no fold offered;
    // and a fold descriptor handed to a block whose hidden width is larger than its attention output)
    show_self("alias_edge_hidden_equal", self_block(FP16, 1280, 8, 256, 1280), 2, 256, true);
    pio_self_attention_t wide_hidden = self_block(FP16, 1280, 8, 256, 1280);
    wide_hidden.mlp = mlp(FP16, 1280, 2, 1280);
    show_self("alias_edge_hidden_greater", wide_hidden, 2, 256, true);
    show_self("no_fold_offered_widening_4", self_block(FP16, 1024, 8, 0, 0, 4), 2, 256, true);
}

static void chunk_cases() {   // score_chunks: all at once / whole samples per pass / row chunks of one sample
    const struct { const char *id; int B, H, Tq, Tk; } c[] = {
        {"fits", 32, 8, 512, 512}, {"exactly_the_cap", 4, 1, 256, 262144}, {"samples_per_pass", 64, 8, 1024, 1024},
        {"one_sample_per_pass", 2, 1, 1024, 262144}, {"flow_2048_x_182528", 1, 1, 2048, 182528},
        {"row_chunk_floor_128", 1, 8, 2048, 1 << 20}, {"row_chunk_capped_by_tq", 1, 64, 100, 1 << 20}};
    for (const auto &k : c) {
        const ScoreChunks s = score_chunks(k.B, k.H, k.Tq, k.Tk);
        printf("chunks %s %d %d\n", k.id, s.b_chunk, s.q_chunk);
    }
    // ... and the plan that holds the flow encoder's scores under a 3-sweep policy
    show_cross("flow_cross_x3_scores", cross_block(X3, 512, 322, 1), 1, 2048, 182528, true, true);
}

// ---- the fold ------------------------------------------------------------------------------------------------------
static const FoldKnobs MODE0 = {0, 6144, 512, 4096}, MODE1 = {1, 6144, 512, 4096},
                       MODE2 = {2, 2048, 128, 4096};    // (mode 2: the caller lowers the bounds to 2048 / 128)
static SelfCall call_of(int B, int N, int C) {
    SelfCall c = {};
    c.B = B; c.N = N; c.C = C; c.stride_t = C; c.stride_b = (int64_t)N * C; c.x_aligned16 = c.has_fold_buffers = true;
    return c;
}
static void show_fold(const char *id, const pio_self_attention_t &sa, const SelfCall &c, const FoldKnobs &k) {
    const SelfFold f = self_fold_route(sa, c, k);
    printf("fold %s %s %d %d\n", id, f.family == SelfFold::NONE ? "NONE" : f.family == SelfFold::SMALL ? "SMALL" : "WIDE",
           f.slot_w, f.nslots);
}
static SelfCall with(SelfCall c, bool SelfCall::*flag, bool v = true) { c.*flag = v; return c; }

static void fold_cases() {
    char id[64];
    // channel counts (8 heads of C / 8 are outside the fused heads for 256 / 768 / 1536 / 1792: 16 heads of 32 there)
    const int chans[] = {256, 512, 768, 1536, 1792, 520};
    for (int C : chans) {
        pio_self_attention_t sa = self_block(FP16, C, C == 512 ? 8 : C / 32);
        if (!sa.fold.qkv.w_hi) {   // a caller that offers the images outside 512..1536 / multiples of 256 all the same
            sa.fold.qkv = lin(sa.attn.qkv.n, padc(C), false); sa.fold.fc1 = lin(padc(C), padc(C), false);
        }
        snprintf(id, sizeof id, "channels_%d", C);
        show_fold(id, sa, call_of(8, 1024, C), MODE1);
    }
    const pio_self_attention_t sa = self_block(FP16, 1024, 8);
    const SelfCall ok = call_of(8, 1024, 1024);
    show_fold("imagenet_b32", sa, call_of(32, 512, 1024), MODE1);
    SelfCall c = ok; c.stride_t = 1032; c.stride_b = 1024 * 1032;
    show_fold("row_stride_not_c", sa, c, MODE1);
    c = ok; c.stride_b = 1024 * 1024 + 1024;
    show_fold("batch_stride_not_n_c", sa, c, MODE1);
    c = call_of(1, 8192, 1024); c.stride_b = 0;
    show_fold("batch_stride_ignored_at_b1", sa, c, MODE1);
    show_fold("misaligned_pointer", sa, with(ok, &SelfCall::x_aligned16, false), MODE1);
    show_fold("no_fold_buffers", sa, with(ok, &SelfCall::has_fold_buffers, false), MODE1);
    show_fold("kv_mask", sa, with(ok, &SelfCall::kv_mask), MODE1);
    show_fold("q_mask", sa, with(ok, &SelfCall::q_mask), MODE1);
    show_fold("full_mask", sa, with(ok, &SelfCall::full_mask), MODE1);
    show_fold("bias", sa, with(ok, &SelfCall::bias), MODE1);
    show_fold("probs", sa, with(ok, &SelfCall::probs), MODE1);
    pio_self_attention_t t = sa; t.attn.act_split = 2;
    show_fold("attn_act_split", t, ok, MODE1);
    t = sa; t.mlp.act_split = 1;
    show_fold("mlp_act_split", t, ok, MODE1);
    t = sa; t.attn.qkv.w_hi = nullptr;
    show_fold("no_qkv_image", t, ok, MODE1);
    const pio_self_attention_t s2 = self_block(X2S, 1024, 8), w2 = self_block(X2W, 1024, 8);
    show_fold("qkv_lo_row0_right", s2, ok, MODE1);
    t = s2; t.fold.qkv.lo_row0 = 0;
    show_fold("qkv_lo_row0_wrong", t, ok, MODE1);
    show_fold("fc1_lo_row0_right", w2, ok, MODE1);
    t = w2; t.fold.fc1.lo_row0 = 256;
    show_fold("fc1_lo_row0_wrong", t, ok, MODE1);
    t = sa; t.mlp.hidden = 2048;
    show_fold("mlp_hidden_not_c", t, ok, MODE1);
    t = sa; t.mlp.dtype = PIO_DT_BF16;
    show_fold("dtype_mismatch", t, ok, MODE1);
    t = sa; t.attn.dkp = t.attn.dvp = 256;
    show_fold("head_shape_not_fused", t, ok, MODE1);
    t = sa; t.fold.qkv.n += 8;
    show_fold("fold_qkv_rows_differ", t, ok, MODE1);
    t = sa; t.fold.qkv.k = 1088;
    show_fold("fold_qkv_k_differs", t, ok, MODE1);
    t = sa; t.fold.fc1.k = 1088;
    show_fold("fold_fc1_k_differs", t, ok, MODE1);
    t = sa; t.fold.fc1.n = 2048;
    show_fold("fold_fc1_rows_differ", t, ok, MODE1);
    // row bounds
    const int rows1[] = {511, 512, 4095, 4096, 6143, 6144}, rows2[] = {127, 128, 2047, 2048, 4096};
    for (int r : rows1) {
        snprintf(id, sizeof id, "mode1_rows_%d", r);
        show_fold(id, sa, call_of(1, r, 1024), MODE1);
    }
    for (int r : rows2) {
        snprintf(id, sizeof id, "mode2_rows_%d", r);
        show_fold(id, sa, call_of(1, r, 1024), MODE2);
    }
    show_fold("mode0_rows_8192", sa, ok, MODE0);
    // split weights forbid the tile-kernel family: fold image lo halves, the out projection's, fc2's
    show_fold("x2s_rows_2048_mode1", s2, call_of(1, 2048, 1024), MODE1);
    show_fold("x2s_rows_6144_mode1", s2, call_of(1, 6144, 1024), MODE1);
    show_fold("x2w_rows_2047_mode2", w2, call_of(1, 2047, 1024), MODE2);
    show_fold("x2w_rows_2048_mode2", w2, call_of(1, 2048, 1024), MODE2);
    show_fold("x2o_rows_2048_mode1", self_block(X2O, 1024, 8), call_of(1, 2048, 1024), MODE1);
    t = sa; t.mlp.fc2.w_lo = W;
    show_fold("fc2_lo_rows_2048_mode1", t, call_of(1, 2048, 1024), MODE1);
    show_fold("fc2_lo_rows_6144_mode1", t, call_of(1, 6144, 1024), MODE1);
}

static void y16_cases() {
    const pio_linear_t k384 = lin(8, 384, false), k328 = lin(8, 328, false);
    printf("y16 no_final_layer %d\n", decoder_y16_direct(nullptr, 322));
    printf("y16 k_is_padc %d\n", decoder_y16_direct(&k384, 322));
    printf("y16 k_is_pad8_only %d\n", decoder_y16_direct(&k328, 322));
}

// ---- the GEMM descriptor of one nn.Linear, in every form pio_blocks.hip asks for ------------------------------------------
// every non-pointer field of the pio_gemm_t, then the pointer fields that are set
static void show_linear(const char *id, const pio_gemm_t &g) {
    printf("linear %s M=%d N=%d K=%d lda=%lld ldb=%lld ldc=%lld batch=%d nh=%d sAb=%lld sAh=%lld sBb=%lld sBh=%lld sCb=%lld "
           "sCh=%lld bias_mode=%d act=%d alpha=%g ldr=%lld r_stride_b=%lld r_rows_per_batch=%d out_f32=%d n_store=%d dtype=%d "
           "ld16=%lld ln_eps=%g b_lo_n0=%d ln_slots=%d row_slot_w=%d ptrs=",
           id, g.M, g.N, g.K, (long long)g.lda, (long long)g.ldb, (long long)g.ldc, g.batch, g.nh, (long long)g.sAb,
           (long long)g.sAh, (long long)g.sBb, (long long)g.sBh, (long long)g.sCb, (long long)g.sCh, g.bias_mode, g.act,
           g.alpha, (long long)g.ldr, (long long)g.r_stride_b, g.r_rows_per_batch, g.out_f32, g.n_store, g.dtype,
           (long long)g.ld16, g.ln_eps, g.b_lo_n0, g.ln_slots, g.row_slot_w);
    const struct { const char *n; const void *p; } ps[] = {
        {"A", g.A}, {"A_lo", g.A_lo}, {"B", g.B}, {"B_lo", g.B_lo}, {"C", g.C}, {"C_lo", g.C_lo}, {"bias", g.bias}, {"R", g.R},
        {"X16", g.X16}, {"X16_lo", g.X16_lo}, {"row_part", g.row_part}, {"ln_part", g.ln_part}, {"ln_c", g.ln_c},
        {"R16_hi", g.R16_hi}, {"R16_lo", g.R16_lo}, {"range_flag", g.range_flag}};
    const char *sep = "";
    for (const auto &q : ps)
        if (q.p) { printf("%s%s", sep, q.n); sep = ","; }
    printf("\n");
}
static pio_linear_t biased(pio_linear_t l) { l.bias = (const float *)W; return l; }   // (as every packed nn.Linear but kq)

static void linear_cases() {
    void *const P = BASE;                  // any 16-bit buffer
    float *const F = (float *)BASE;        // any fp32 buffer
    const Pair hi = {P, nullptr}, both = {P, P};
    const int F16 = PIO_DT_F16;
    // the classifier's stack (1024 channels, 8 heads of 128; 32 x 512 rows) and its decoder (1024-channel queries, 1000
    // classes), the flow model (322-channel inputs AND queries: pitch8 328, pitch4 324, padc 384) and the multimodal
    // decoder (1026-channel queries: pitch8 1032, pitch4 1028, padc 1088)
    const pio_self_attention_t st = self_block(FP16, 1024, 8);
    const pio_cross_attention_t im_d = cross_block(X2AF, 1024, 1024, 1), fl_x = cross_block(FP16, 512, 322, 1),
                                fl_d = cross_block(X2AF, 322, 512, 1, 0, 0, false),
                                mm_d = cross_block(X2AFO, 1026, 512, 1, 0, 0, false);
    const pio_linear_t im_f = biased(final_layer(X2AF, 1024, 1000)), fl_f = biased(final_layer(X2AF, 322, 2)),
                       mm_f = biased(final_layer(X2AFO, 1026, 512));
    const int64_t rows = 32 * 512, hdk = 1024, ld3 = 3072;
    const pio_tensor3_t x = {F, 512 * 1024, 1024, 32, 512, 1024};
    const Residual rx = residual_of(x);

    // q, k, q|k, q|k|v: 16-bit pairs at the pitch of the (stacked) heads
    show_linear("q_plain", linear_gemm(biased(im_d.attn.q), F16, both, 1000, pair16_at(both, hdk)));
    show_linear("q_322", linear_gemm(biased(fl_d.attn.q), F16, both, 182528, pair16_at(both, 512)));
    show_linear("q_1026", linear_gemm(biased(mm_d.attn.q), F16, both, 6288, pair16_at(both, 512)));
    show_linear("k_plain", linear_gemm(biased(im_d.attn.k), F16, both, rows, pair16_at(both, hdk)));
    show_linear("k_322", linear_gemm(biased(fl_x.attn.k), F16, hi, 182528, pair16_at(hi, 328)));
    show_linear("qk_plain", linear_gemm(biased(st.attn.qk), F16, hi, rows, pair16_at(hi, 2 * hdk)));
    show_linear("qkv_plain", linear_gemm(biased(st.attn.qkv), F16, hi, rows, pair16_at(hi, ld3)));
    pio_self_attention_t folded = st;
    folded.fold.qkv = biased(folded.fold.qkv); folded.fold.fc1 = biased(folded.fold.fc1);
    LnFold f_qkv, f_out, f_fc1, f_fc2;       // as self_attention_run wires them (WIDE family: 128-column slots)
    f_qkv.in_part = F; f_qkv.w = &folded.fold.qkv; f_qkv.c = F; f_qkv.eps = 1e-5f; f_qkv.in_slots = 8;
    f_fc1 = f_qkv; f_fc1.w = &folded.fold.fc1;
    f_out.out16 = P; f_out.ld16 = 1024; f_out.out_part = F; f_out.out16_lo = P; f_out.res16_hi = P; f_out.res16_lo = P;
    f_out.range_flag = (int32_t *)BASE; f_out.slot_w = 128;
    f_fc2 = f_out;
    show_linear("qkv_folded", linear_gemm(biased(st.attn.qkv), F16, hi, rows, pair16_at(hi, ld3).folded(&f_qkv)));
    LnFold f_small = f_qkv; f_small.in_slots = 16;
    show_linear("qkv_folded_small", linear_gemm(biased(st.attn.qkv), F16, hi, 600, pair16_at(hi, ld3).folded(&f_small)));
    const pio_self_attention_t s2 = self_block(X2S, 1024, 8);     // (the fold's q|k|v image with a lo half for its V rows)
    LnFold f_s2 = f_qkv; f_s2.w = &s2.fold.qkv;
    show_linear("qkv_folded_v_lo", linear_gemm(s2.attn.qkv, F16, hi, rows, pair16_at(hi, ld3).folded(&f_s2)));
    // kq (K / V projection fold: Q Wk, no bias), at 322 channels on pad8
    show_linear("kq_322", linear_gemm(fl_x.attn.kq, F16, hi, 2048, pair16_at(hi, 328)));

    // out projection: fp32 rows
    show_linear("out_plain", linear_gemm(biased(st.attn.o), F16, hi, rows, f32_at(F, 1024, 1024)));
    show_linear("out_322_plain", linear_gemm(biased(fl_d.attn.o), F16, both, 182528, f32_at(F, 322, 322)));
    show_linear("out_residual", linear_gemm(biased(st.attn.o), F16, hi, rows, f32_at(F, 1024, 1024).plus(&rx)));
    show_linear("out_fold_producer",
                linear_gemm(biased(st.attn.o), F16, hi, rows, f32_at(nullptr, 1024, 1024).plus(&rx).folded(&f_out)));
    // ... into x1 of a cross-attend at its internal pitch (pitch8), zeros behind the logical columns
    const pio_tensor3_t z = {F, 0, 512, 1, 2048, 512};
    const Residual rz = residual_of(z), none;
    show_linear("out_pitch8_1024", linear_gemm(biased(im_d.attn.o), F16, both, 32000, f32_at(F, 1024, 1024).plus(&none)));
    show_linear("out_pitch8_322", linear_gemm(biased(fl_d.attn.o), F16, both, 182528, f32_at(F, 322, 328).zeros_to(328)));
    show_linear("out_pitch8_1026", linear_gemm(biased(mm_d.attn.o), F16, both, 6288, f32_at(F, 1026, 1032).zeros_to(1032)));
    show_linear("out_pitch8_vo_residual", linear_gemm(biased(fl_x.attn.vo), F16, hi, 2048, f32_at(F, 512, 512).plus(&rz)));
    pio_cross_attention_t odd = cross_block(FP16, 322, 512, 1);   // a 322-channel block WITH the query residual
    const pio_tensor3_t q322 = {F, 100 * 322, 322, 2, 100, 322};
    const Residual rq = residual_of(q322);
    show_linear("out_pitch8_322_residual",
                linear_gemm(biased(odd.attn.o), F16, hi, 200, f32_at(F, 322, 328).plus(&rq).zeros_to(328)));

    // fc1: 16-bit pair, GELU
    show_linear("fc1_plain", linear_gemm(biased(st.mlp.fc1), F16, hi, rows, pair16_at(hi, st.mlp.fc1.n).gelu()));
    show_linear("fc1_1026", linear_gemm(biased(mm_d.mlp.fc1), F16, both, 6288, pair16_at(both, mm_d.mlp.fc1.n).gelu()));
    show_linear("fc1_322", linear_gemm(biased(fl_d.mlp.fc1), F16, both, 182528, pair16_at(both, fl_d.mlp.fc1.n).gelu()));
    show_linear("fc1_folded", linear_gemm(biased(st.mlp.fc1), F16, hi, rows, pair16_at(hi, st.mlp.fc1.n).gelu().folded(&f_fc1)));
    // fc2: fp32 (+ residual x1), the fold's producer, the decoders' 16-bit y
    const pio_tensor3_t t1 = {F, 512 * 1024, 1024, 32, 512, 1024};
    const Residual r1 = residual_of(t1);
    show_linear("fc2_f32", linear_gemm(biased(st.mlp.fc2), F16, hi, rows, f32_at(F, 1024, 1024).plus(&r1)));
    show_linear("fc2_no_residual", linear_gemm(biased(st.mlp.fc2), F16, hi, rows, f32_at(F, 1024, 1024)));
    show_linear("fc2_fold_producer",
                linear_gemm(biased(st.mlp.fc2), F16, hi, rows, f32_at(F, 1024, 1024).plus(&r1).folded(&f_fc2)));
    show_linear("fc2_fold_producer_no_f32",
                linear_gemm(biased(st.mlp.fc2), F16, hi, rows, f32_at(nullptr, 1024, 1024).plus(&r1).folded(&f_fc2)));
    // (a cross-attend's x1 has pitch8 rows; `out` the caller's pitch, or pitch4 for a decoder's internal y)
    const pio_tensor3_t t322 = {F, 182528ll * 328, 328, 1, 182528, 322}, t1026 = {F, 6288 * 1032, 1032, 1, 6288, 1026};
    const Residual r322 = residual_of(t322), r1026 = residual_of(t1026);
    show_linear("fc2_f32_322_caller_pitch", linear_gemm(biased(fl_d.mlp.fc2), F16, both, 182528, f32_at(F, 322, 322).plus(&r322)));
    show_linear("fc2_f32_322_pitch4", linear_gemm(biased(fl_d.mlp.fc2), F16, both, 182528, f32_at(F, 322, 324).plus(&r322)));
    show_linear("fc2_f32_1026_caller_pitch", linear_gemm(biased(mm_d.mlp.fc2), F16, both, 6288, f32_at(F, 1026, 1026).plus(&r1026)));
    show_linear("fc2_f32_1026_pitch4", linear_gemm(biased(mm_d.mlp.fc2), F16, both, 6288, f32_at(F, 1026, 1028).plus(&r1026)));
    const Residual r322_narrow = residual_of(q322);   // (a residual at the logical pitch keeps the logical width)
    show_linear("fc2_f32_322_pitch4_narrow_residual",
                linear_gemm(biased(fl_d.mlp.fc2), F16, both, 200, f32_at(F, 322, 324).plus(&r322_narrow)));
    const pio_tensor3_t t1024 = {F, 1000 * 1024, 1024, 32, 1000, 1024};
    const Residual r1024 = residual_of(t1024);
    show_linear("fc2_out16_1024", linear_gemm(biased(im_d.mlp.fc2), F16, both, 32000, out16_at(both, padc(1024), &r1024)));
    show_linear("fc2_out16_322", linear_gemm(biased(fl_d.mlp.fc2), F16, both, 182528, out16_at(both, padc(322), &r322)));
    show_linear("fc2_out16_1026", linear_gemm(biased(mm_d.mlp.fc2), F16, both, 6288, out16_at(both, padc(1026), &r1026)));
    // the decoders' final Linear
    show_linear("final_1000", linear_gemm(im_f, F16, both, 32000, f32_at(F, 1000, 1000)));
    show_linear("final_2_from_322", linear_gemm(fl_f, F16, both, 182528, f32_at(F, 2, 2)));
    show_linear("final_512_from_1026", linear_gemm(mm_f, PIO_DT_BF16, both, 6288, f32_at(F, 512, 512)));
}

int main() {
    plan_cases();
    chunk_cases();
    fold_cases();
    y16_cases();
    linear_cases();
    return 0;
}
'''

# id -> total bytes (with a workspace / with a null base, as the *_workspace_bytes entry points carve), then every
# member's offset; split, qbytes, kbytes: what the adjacency check below needs
PLANS = {
    "imagenet_cross":
        "total=397300480 null_base_total=397300480 q16.hi=0 q16.lo=-1 kv16.hi=33554432 kv16.lo=-1 "
        "h16.hi=110624768 h16.lo=-1 x1=144179200 core.q16.hi=211288064 core.q16.lo=-1 core.k16.hi=211623936 "
        "core.k16.lo=-1 core.vt16.hi=277454848 core.vt16.lo=-1 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 "
        "core.o16.hi=343285760 core.o16.lo=-1 core.xpart=354033664 split=0 qbytes=335872 kbytes=65830912",
    "imagenet_stack":
        "total=306448384 null_base_total=306448384 x16.hi=0 x16.lo=-1 h16.hi=234881024 h16.lo=-1 x1=67108864 "
        "core.q16.hi=134217728 core.q16.lo=-1 core.k16.hi=167772160 core.k16.lo=-1 core.vt16.hi=201326592 "
        "core.vt16.lo=-1 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 core.o16.hi=234881024 core.o16.lo=-1 "
        "core.xpart=268435456 split=0 qbytes=33554432 kbytes=33554432 x16b=0 lo_a=268437504 lo_b=268437504 "
        "part_a=301991936 part_b=304220160",
    "imagenet_decoder":
        "total=991856640 null_base_total=991856640 y=0 y16.hi=131072000 y16.lo=196608000 q16.hi=262144000 "
        "q16.lo=327680000 kv16.hi=393216000 kv16.lo=426770432 h16.hi=460324864 h16.lo=525860864 x1=591396864 "
        "core.q16.hi=722468864 core.q16.lo=724516864 core.k16.hi=726564864 core.k16.lo=760119296 "
        "core.vt16.hi=793673728 core.vt16.lo=827228160 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 "
        "core.o16.hi=860782592 core.o16.lo=926318592 core.xpart=991854592 split=1 qbytes=2048000 "
        "kbytes=33554432 pitch4=1024 pad8=1024 padc=1024 y16_direct=1",
    "language_cross":
        "total=1271555072 null_base_total=1271555072 q16.hi=0 q16.lo=-1 kv16.hi=65536000 kv16.lo=-1 "
        "h16.hi=380108800 h16.lo=-1 x1=445644800 core.q16.hi=576716800 core.q16.lo=-1 core.k16.hi=576847872 "
        "core.k16.lo=-1 core.vt16.hi=681705472 core.vt16.lo=-1 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 "
        "core.o16.hi=1205993472 core.o16.lo=-1 core.xpart=1271529472 split=0 qbytes=131072 kbytes=104857600",
    "language_stack":
        "total=493571328 null_base_total=493571328 x16.hi=0 x16.lo=-1 h16.hi=353894400 h16.lo=-1 x1=131072000 "
        "core.q16.hi=262144000 core.q16.lo=-1 core.k16.hi=275251200 core.k16.lo=-1 core.vt16.hi=288358400 "
        "core.vt16.lo=-1 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 core.o16.hi=353894400 core.o16.lo=-1 "
        "core.xpart=419430400 split=0 qbytes=13107200 kbytes=13107200 x16b=0 lo_a=419433728 lo_b=419433728 "
        "part_a=484969728 part_b=489270528",
    "language_decoder":
        "total=2962230528 null_base_total=2962230528 y=-1 y16.hi=-1 y16.lo=-1 q16.hi=0 q16.lo=314572800 "
        "kv16.hi=629145600 kv16.lo=694681600 h16.hi=760217600 h16.lo=1074790400 x1=1389363200 "
        "core.q16.hi=2018508800 core.q16.lo=2123366400 core.k16.hi=2228224000 core.k16.lo=2241331200 "
        "core.vt16.hi=2254438400 core.vt16.lo=2293760000 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 "
        "core.o16.hi=2333081600 core.o16.lo=2647654400 core.xpart=2962227200 split=1 qbytes=104857600 "
        "kbytes=13107200 pitch4=768 pad8=768 padc=768 y16_direct=0",
    "flow_cross":
        "total=434011136 null_base_total=434011136 q16.hi=0 q16.lo=-1 kv16.hi=2097152 kv16.lo=-1 "
        "h16.hi=142278656 h16.lo=-1 x1=144375808 core.q16.hi=148570112 core.q16.lo=-1 core.k16.hi=149913600 "
        "core.k16.lo=-1 core.vt16.hi=269651968 core.vt16.lo=-1 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 "
        "core.o16.hi=389390336 core.o16.lo=-1 core.xpart=390733824 split=0 qbytes=1343488 kbytes=119738368",
    "flow_stack":
        "total=28082944 null_base_total=28082944 x16.hi=0 x16.lo=-1 h16.hi=14680064 h16.lo=-1 x1=4194304 "
        "core.q16.hi=8388608 core.q16.lo=-1 core.k16.hi=10485760 core.k16.lo=-1 core.vt16.hi=12582912 "
        "core.vt16.lo=-1 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 core.o16.hi=14680064 core.o16.lo=-1 "
        "core.xpart=16777216 split=0 qbytes=2097152 kbytes=2097152 x16b=0 lo_a=25690880 lo_b=25690880 "
        "part_a=27788032 part_b=27935488",
    "flow_decoder_322":
        "total=2077339904 null_base_total=2077339904 y=0 y16.hi=236556288 y16.lo=376737792 q16.hi=516919296 "
        "q16.lo=657100800 kv16.hi=797282304 kv16.lo=799379456 h16.hi=801476608 h16.lo=941658112 x1=1081839616 "
        "core.q16.hi=1321316352 core.q16.lo=1508225024 core.k16.hi=1695133696 core.k16.lo=1697230848 "
        "core.vt16.hi=1699328000 core.vt16.lo=1701425152 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 "
        "core.o16.hi=1703522304 core.o16.lo=1890430976 core.xpart=2077339648 split=1 qbytes=186908672 "
        "kbytes=2097152 pitch4=324 pad8=328 padc=384 y16_direct=1",
    "flow_decoder_322_no_final":
        "total=1560420608 null_base_total=1560420608 y=-1 y16.hi=-1 y16.lo=-1 q16.hi=0 q16.lo=140181504 "
        "kv16.hi=280363008 kv16.lo=282460160 h16.hi=284557312 h16.lo=424738816 x1=564920320 "
        "core.q16.hi=804397056 core.q16.lo=991305728 core.k16.hi=1178214400 core.k16.lo=1180311552 "
        "core.vt16.hi=1182408704 core.vt16.lo=1184505856 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 "
        "core.o16.hi=1186603008 core.o16.lo=1373511680 core.xpart=1560420352 split=1 qbytes=186908672 "
        "kbytes=2097152 pitch4=324 pad8=328 padc=384 y16_direct=0",
    "multimodal_cross":
        "total=254310144 null_base_total=254310144 q16.hi=0 q16.lo=-1 kv16.hi=802816 kv16.lo=-1 "
        "h16.hi=74155520 h16.lo=-1 x1=74958336 core.q16.hi=76563968 core.q16.lo=-1 core.k16.hi=77667840 "
        "core.k16.lo=-1 core.vt16.hi=151020544 core.vt16.lo=-1 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 "
        "core.o16.hi=224416768 core.o16.lo=-1 core.xpart=225520640 split=0 qbytes=1103872 kbytes=73352576",
    "multimodal_stack":
        "total=12323072 null_base_total=12323072 x16.hi=0 x16.lo=-1 h16.hi=5636096 h16.lo=-1 x1=1605632 "
        "core.q16.hi=3211264 core.q16.lo=-1 core.k16.hi=4014080 core.k16.lo=-1 core.vt16.hi=4816896 "
        "core.vt16.lo=-1 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 core.o16.hi=5636096 core.o16.lo=-1 "
        "core.xpart=6438912 split=0 qbytes=802816 kbytes=802816 x16b=0 lo_a=11407104 lo_b=11407104 "
        "part_a=12209920 part_b=12266496",
    "multimodal_decoder_1026":
        "total=203299840 null_base_total=203299840 y=0 y16.hi=25856256 y16.lo=39538944 q16.hi=53221632 "
        "q16.lo=66904320 kv16.hi=80587008 kv16.lo=81389824 h16.hi=82192640 h16.lo=95875328 x1=109558016 "
        "core.q16.hi=135514880 core.q16.lo=141953792 core.k16.hi=148392704 core.k16.lo=149195520 "
        "core.vt16.hi=149998336 core.vt16.lo=150817536 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 "
        "core.o16.hi=151636736 core.o16.lo=158075648 core.xpart=164514560 split=1 qbytes=6438912 "
        "kbytes=802816 pitch4=1028 pad8=1032 padc=1088 y16_direct=1",
    "multimodal_decoder_1026_no_final":
        "total=150078208 null_base_total=150078208 y=-1 y16.hi=-1 y16.lo=-1 q16.hi=0 q16.lo=13682688 "
        "kv16.hi=27365376 kv16.lo=28168192 h16.hi=28971008 h16.lo=42653696 x1=56336384 core.q16.hi=82293248 "
        "core.q16.lo=88732160 core.k16.hi=95171072 core.k16.lo=95973888 core.vt16.hi=96776704 "
        "core.vt16.lo=97595904 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 core.o16.hi=98415104 "
        "core.o16.lo=104854016 core.xpart=111292928 split=1 qbytes=6438912 kbytes=802816 pitch4=1028 "
        "pad8=1032 padc=1088 y16_direct=0",
    "self_512_act_split_0":
        "total=17375488 null_base_total=17375488 x16.hi=0 x16.lo=-1 h16.hi=16252928 h16.lo=-1 x1=1048576 "
        "core.q16.hi=2097152 core.q16.lo=-1 core.k16.hi=2621440 core.k16.lo=-1 core.vt16.hi=3145728 "
        "core.vt16.lo=-1 core.scores=3670016 core.p16.hi=12058624 core.p16.lo=-1 core.o16.hi=16252928 "
        "core.o16.lo=-1 core.xpart=16777216 split=0 qbytes=524288 kbytes=524288 x16b=0 lo_a=16777472 "
        "lo_b=16777472 part_a=17301760 part_b=17338624",
    "cross_act_split_0":
        "total=3755264 null_base_total=3755264 q16.hi=0 q16.lo=-1 kv16.hi=131072 kv16.lo=-1 h16.hi=207872 "
        "h16.lo=-1 x1=338944 core.q16.hi=601088 core.q16.lo=-1 core.k16.hi=732160 core.k16.lo=-1 "
        "core.vt16.hi=936960 core.vt16.lo=-1 core.scores=1166336 core.p16.hi=2804736 core.p16.lo=-1 "
        "core.o16.hi=3623936 core.o16.lo=-1 core.xpart=3755008 split=0 qbytes=131072 kbytes=204800",
    "attention_act_split_0":
        "total=3362048 null_base_total=3362048 xq16.hi=0 xq16.lo=-1 xk16.hi=131072 xk16.lo=-1 xv16.hi=131072 "
        "xv16.lo=-1 core.q16.hi=207872 core.q16.lo=-1 core.k16.hi=338944 core.k16.lo=-1 core.vt16.hi=543744 "
        "core.vt16.lo=-1 core.scores=773120 core.p16.hi=2411520 core.p16.lo=-1 core.o16.hi=3230720 "
        "core.o16.lo=-1 core.xpart=3361792 split=0 qbytes=131072 kbytes=204800",
    "mlp_act_split_0":
        "total=1036800 null_base_total=1036800 x16.hi=0 x16.lo=-1 h16.hi=230400 h16.lo=-1",
    "self_512_act_split_1":
        "total=24117248 null_base_total=24117248 x16.hi=0 x16.lo=524288 h16.hi=1048576 h16.lo=1572864 "
        "x1=2097152 core.q16.hi=3145728 core.q16.lo=3670016 core.k16.hi=4194304 core.k16.lo=4718592 "
        "core.vt16.hi=5242880 core.vt16.lo=5767168 core.scores=6291456 core.p16.hi=14680064 "
        "core.p16.lo=18874368 core.o16.hi=23068672 core.o16.lo=23592960 core.xpart=-1 split=1 qbytes=524288 "
        "kbytes=524288 x16b=-1 lo_a=-1 lo_b=-1 part_a=-1 part_b=-1",
    "cross_act_split_1":
        "total=5609472 null_base_total=5609472 q16.hi=0 q16.lo=131072 kv16.hi=262144 kv16.lo=338944 "
        "h16.hi=415744 h16.lo=546816 x1=677888 core.q16.hi=940032 core.q16.lo=1071104 core.k16.hi=1202176 "
        "core.k16.lo=1406976 core.vt16.hi=1611776 core.vt16.lo=1841152 core.scores=2070528 "
        "core.p16.hi=3708928 core.p16.lo=4528128 core.o16.hi=5347328 core.o16.lo=5478400 core.xpart=-1 "
        "split=1 qbytes=131072 kbytes=204800",
    "attention_act_split_1":
        "total=5085184 null_base_total=5085184 xq16.hi=0 xq16.lo=131072 xk16.hi=262144 xk16.lo=338944 "
        "xv16.hi=262144 xv16.lo=338944 core.q16.hi=415744 core.q16.lo=546816 core.k16.hi=677888 "
        "core.k16.lo=882688 core.vt16.hi=1087488 core.vt16.lo=1316864 core.scores=1546240 core.p16.hi=3184640 "
        "core.p16.lo=4003840 core.o16.hi=4823040 core.o16.lo=4954112 core.xpart=-1 split=1 qbytes=131072 "
        "kbytes=204800",
    "mlp_act_split_1":
        "total=2073600 null_base_total=2073600 x16.hi=0 x16.lo=230400 h16.hi=460800 h16.lo=1267200",
    "self_512_act_split_2":
        "total=24117504 null_base_total=24117504 x16.hi=0 x16.lo=524288 h16.hi=1048576 h16.lo=1572864 "
        "x1=2097152 core.q16.hi=3145728 core.q16.lo=3670016 core.k16.hi=4194304 core.k16.lo=4718592 "
        "core.vt16.hi=5242880 core.vt16.lo=5767168 core.scores=6291456 core.p16.hi=14680064 "
        "core.p16.lo=18874368 core.o16.hi=23068672 core.o16.lo=23592960 core.xpart=24117248 split=1 "
        "qbytes=524288 kbytes=524288 x16b=-1 lo_a=-1 lo_b=-1 part_a=-1 part_b=-1",
    "cross_act_split_2":
        "total=5609728 null_base_total=5609728 q16.hi=0 q16.lo=131072 kv16.hi=262144 kv16.lo=338944 "
        "h16.hi=415744 h16.lo=546816 x1=677888 core.q16.hi=940032 core.q16.lo=1071104 core.k16.hi=1202176 "
        "core.k16.lo=1406976 core.vt16.hi=1611776 core.vt16.lo=1841152 core.scores=2070528 "
        "core.p16.hi=3708928 core.p16.lo=4528128 core.o16.hi=5347328 core.o16.lo=5478400 core.xpart=5609472 "
        "split=1 qbytes=131072 kbytes=204800",
    "attention_act_split_2":
        "total=5085440 null_base_total=5085440 xq16.hi=0 xq16.lo=131072 xk16.hi=262144 xk16.lo=338944 "
        "xv16.hi=262144 xv16.lo=338944 core.q16.hi=415744 core.q16.lo=546816 core.k16.hi=677888 "
        "core.k16.lo=882688 core.vt16.hi=1087488 core.vt16.lo=1316864 core.scores=1546240 core.p16.hi=3184640 "
        "core.p16.lo=4003840 core.o16.hi=4823040 core.o16.lo=4954112 core.xpart=5085184 split=1 qbytes=131072 "
        "kbytes=204800",
    "mlp_act_split_2":
        "total=2073600 null_base_total=2073600 x16.hi=0 x16.lo=230400 h16.hi=460800 h16.lo=1267200",
    "self_512_act_split_3":
        "total=24117504 null_base_total=24117504 x16.hi=0 x16.lo=524288 h16.hi=1048576 h16.lo=1572864 "
        "x1=2097152 core.q16.hi=3145728 core.q16.lo=3670016 core.k16.hi=4194304 core.k16.lo=4718592 "
        "core.vt16.hi=5242880 core.vt16.lo=5767168 core.scores=6291456 core.p16.hi=14680064 "
        "core.p16.lo=18874368 core.o16.hi=23068672 core.o16.lo=23592960 core.xpart=24117248 split=1 "
        "qbytes=524288 kbytes=524288 x16b=-1 lo_a=-1 lo_b=-1 part_a=-1 part_b=-1",
    "cross_act_split_3":
        "total=5609728 null_base_total=5609728 q16.hi=0 q16.lo=131072 kv16.hi=262144 kv16.lo=338944 "
        "h16.hi=415744 h16.lo=546816 x1=677888 core.q16.hi=940032 core.q16.lo=1071104 core.k16.hi=1202176 "
        "core.k16.lo=1406976 core.vt16.hi=1611776 core.vt16.lo=1841152 core.scores=2070528 "
        "core.p16.hi=3708928 core.p16.lo=4528128 core.o16.hi=5347328 core.o16.lo=5478400 core.xpart=5609472 "
        "split=1 qbytes=131072 kbytes=204800",
    "attention_act_split_3":
        "total=5085440 null_base_total=5085440 xq16.hi=0 xq16.lo=131072 xk16.hi=262144 xk16.lo=338944 "
        "xv16.hi=262144 xv16.lo=338944 core.q16.hi=415744 core.q16.lo=546816 core.k16.hi=677888 "
        "core.k16.lo=882688 core.vt16.hi=1087488 core.vt16.lo=1316864 core.scores=1546240 core.p16.hi=3184640 "
        "core.p16.lo=4003840 core.o16.hi=4823040 core.o16.lo=4954112 core.xpart=5085184 split=1 qbytes=131072 "
        "kbytes=204800",
    "mlp_act_split_3":
        "total=2073600 null_base_total=2073600 x16.hi=0 x16.lo=230400 h16.hi=460800 h16.lo=1267200",
    "attention_v_apart_q_bcast":
        "total=3307776 null_base_total=3307776 xq16.hi=0 xq16.lo=-1 xk16.hi=65536 xk16.lo=-1 xv16.hi=142336 "
        "xv16.lo=-1 core.q16.hi=219136 core.q16.lo=-1 core.k16.hi=284672 core.k16.lo=-1 core.vt16.hi=489472 "
        "core.vt16.lo=-1 core.scores=718848 core.p16.hi=2357248 core.p16.lo=-1 core.o16.hi=3176448 "
        "core.o16.lo=-1 core.xpart=3307520 split=0 qbytes=65536 kbytes=204800",
    "imagenet_stack_b1_not_lean":
        "total=26419968 null_base_total=26419968 x16.hi=0 x16.lo=-1 h16.hi=19922944 h16.lo=-1 x1=2097152 "
        "core.q16.hi=4194304 core.q16.lo=-1 core.k16.hi=5242880 core.k16.lo=-1 core.vt16.hi=6291456 "
        "core.vt16.lo=-1 core.scores=7340032 core.p16.hi=15728640 core.p16.lo=-1 core.o16.hi=19922944 "
        "core.o16.lo=-1 core.xpart=20971520 split=0 qbytes=1048576 kbytes=1048576 x16b=0 lo_a=25232128 "
        "lo_b=25232128 part_a=26280704 part_b=26350336",
    "imagenet_stack_b1_lean":
        "total=13837056 null_base_total=13837056 x16.hi=0 x16.lo=-1 h16.hi=7340032 h16.lo=-1 x1=2097152 "
        "core.q16.hi=4194304 core.q16.lo=-1 core.k16.hi=5242880 core.k16.lo=-1 core.vt16.hi=6291456 "
        "core.vt16.lo=-1 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 core.o16.hi=7340032 core.o16.lo=-1 "
        "core.xpart=8388608 split=0 qbytes=1048576 kbytes=1048576 x16b=0 lo_a=12649216 lo_b=12649216 "
        "part_a=13697792 part_b=13767424",
    "flow_cross_b2_small_not_lean":
        "total=12736512 null_base_total=12736512 q16.hi=0 q16.lo=-1 kv16.hi=524288 kv16.lo=-1 h16.hi=2060288 "
        "h16.lo=-1 x1=2584576 core.q16.hi=3633152 core.q16.lo=-1 core.k16.hi=3969024 core.k16.lo=-1 "
        "core.vt16.hi=5281024 core.vt16.lo=-1 core.scores=6624512 core.p16.hi=8672512 core.p16.lo=-1 "
        "core.o16.hi=9696512 core.o16.lo=-1 core.xpart=10032384 split=0 qbytes=335872 kbytes=1312000",
    "flow_cross_b2_small_lean":
        "total=9664512 null_base_total=9664512 q16.hi=0 q16.lo=-1 kv16.hi=524288 kv16.lo=-1 h16.hi=2060288 "
        "h16.lo=-1 x1=2584576 core.q16.hi=3633152 core.q16.lo=-1 core.k16.hi=3969024 core.k16.lo=-1 "
        "core.vt16.hi=5281024 core.vt16.lo=-1 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 "
        "core.o16.hi=6624512 core.o16.lo=-1 core.xpart=6960384 split=0 qbytes=335872 kbytes=1312000",
    "flow_cross_b2_small_lean_q_bcast":
        "total=9496576 null_base_total=9496576 q16.hi=0 q16.lo=-1 kv16.hi=524288 kv16.lo=-1 h16.hi=2060288 "
        "h16.lo=-1 x1=2584576 core.q16.hi=3633152 core.q16.lo=-1 core.k16.hi=3801088 core.k16.lo=-1 "
        "core.vt16.hi=5113088 core.vt16.lo=-1 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 "
        "core.o16.hi=6456576 core.o16.lo=-1 core.xpart=6792448 split=0 qbytes=167936 kbytes=1312000",
    "imagenet_decoder_b2":
        "total=69927168 null_base_total=69927168 y=0 y16.hi=8192000 y16.lo=12288000 q16.hi=16384000 "
        "q16.lo=20480000 kv16.hi=24576000 kv16.lo=26673152 h16.hi=28770304 h16.lo=32866304 x1=36962304 "
        "core.q16.hi=45154304 core.q16.lo=49250304 core.k16.hi=53346304 core.k16.lo=55443456 "
        "core.vt16.hi=57540608 core.vt16.lo=59637760 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 "
        "core.o16.hi=61734912 core.o16.lo=65830912 core.xpart=69926912 split=1 qbytes=4096000 kbytes=2097152 "
        "pitch4=1024 pad8=1024 padc=1024 y16_direct=1",
    "imagenet_decoder_b2_q_bcast":
        "total=65831168 null_base_total=65831168 y=0 y16.hi=8192000 y16.lo=12288000 q16.hi=16384000 "
        "q16.lo=20480000 kv16.hi=24576000 kv16.lo=26673152 h16.hi=28770304 h16.lo=32866304 x1=36962304 "
        "core.q16.hi=45154304 core.q16.lo=47202304 core.k16.hi=49250304 core.k16.lo=51347456 "
        "core.vt16.hi=53444608 core.vt16.lo=55541760 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 "
        "core.o16.hi=57638912 core.o16.lo=61734912 core.xpart=65830912 split=1 qbytes=2048000 kbytes=2097152 "
        "pitch4=1024 pad8=1024 padc=1024 y16_direct=1",
    "imagenet_stack_b4_inplace":
        "total=55345920 null_base_total=55345920 x16.hi=0 x16.lo=-1 h16.hi=29360128 h16.lo=-1 x1=8388608 "
        "core.q16.hi=16777216 core.q16.lo=-1 core.k16.hi=20971520 core.k16.lo=-1 core.vt16.hi=25165824 "
        "core.vt16.lo=-1 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 core.o16.hi=29360128 core.o16.lo=-1 "
        "core.xpart=33554432 split=0 qbytes=4194304 kbytes=4194304 x16b=0 lo_a=50594560 lo_b=50594560 "
        "part_a=54788864 part_b=55067392",
    "stack_x2w_1024_inplace":
        "total=55345920 null_base_total=55345920 x16.hi=0 x16.lo=-1 h16.hi=29360128 h16.lo=-1 x1=8388608 "
        "core.q16.hi=16777216 core.q16.lo=-1 core.k16.hi=20971520 core.k16.lo=-1 core.vt16.hi=25165824 "
        "core.vt16.lo=-1 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 core.o16.hi=29360128 core.o16.lo=-1 "
        "core.xpart=33554432 split=0 qbytes=4194304 kbytes=4194304 x16b=0 lo_a=50594560 lo_b=50594560 "
        "part_a=54788864 part_b=55067392",
    "alias_edge_hidden_equal":
        "total=9871616 null_base_total=9871616 x16.hi=0 x16.lo=-1 h16.hi=7077888 h16.lo=-1 x1=2621440 "
        "core.q16.hi=5242880 core.q16.lo=-1 core.k16.hi=5505024 core.k16.lo=-1 core.vt16.hi=5767168 "
        "core.vt16.lo=-1 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 core.o16.hi=7077888 core.o16.lo=-1 "
        "core.xpart=8388608 split=0 qbytes=262144 kbytes=262144 x16b=0 lo_a=8388864 lo_b=8388864 "
        "part_a=9699584 part_b=9785600",
    "alias_edge_hidden_greater":
        "total=11182336 null_base_total=11182336 x16.hi=0 x16.lo=-1 h16.hi=1310720 h16.lo=-1 x1=3932160 "
        "core.q16.hi=6553600 core.q16.lo=-1 core.k16.hi=6815744 core.k16.lo=-1 core.vt16.hi=7077888 "
        "core.vt16.lo=-1 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 core.o16.hi=8388608 core.o16.lo=-1 "
        "core.xpart=9699328 split=0 qbytes=262144 kbytes=262144 x16b=0 lo_a=9699584 lo_b=9699584 "
        "part_a=11010304 part_b=11096320",
    "no_fold_offered_widening_4":
        "total=11534592 null_base_total=11534592 x16.hi=0 x16.lo=-1 h16.hi=1048576 h16.lo=-1 x1=5242880 "
        "core.q16.hi=7340032 core.q16.lo=-1 core.k16.hi=8388608 core.k16.lo=-1 core.vt16.hi=9437184 "
        "core.vt16.lo=-1 core.scores=-1 core.p16.hi=-1 core.p16.lo=-1 core.o16.hi=10485760 core.o16.lo=-1 "
        "core.xpart=11534336 split=0 qbytes=1048576 kbytes=1048576 x16b=-1 lo_a=-1 lo_b=-1 part_a=-1 "
        "part_b=-1",
    "flow_cross_x3_scores":
        "total=2833268736 null_base_total=2833268736 q16.hi=0 q16.lo=2097152 kv16.hi=4194304 "
        "kv16.lo=144375808 h16.hi=284557312 h16.lo=286654464 x1=288751616 core.q16.hi=292945920 "
        "core.q16.lo=294289408 core.k16.hi=295632896 core.k16.lo=415371264 core.vt16.hi=535109632 "
        "core.vt16.lo=654848000 core.scores=774586368 core.p16.hi=1802584064 core.p16.lo=2316582912 "
        "core.o16.hi=2830581760 core.o16.lo=2831925248 core.xpart=-1 split=1 qbytes=1343488 kbytes=119738368",
}

# id -> family, columns per statistics slot, slots per row
FOLDS = {
    "channels_256": ("NONE", 0, 0),
    "channels_512": ("WIDE", 128, 4),
    "channels_768": ("WIDE", 128, 6),
    "channels_1536": ("WIDE", 128, 12),
    "channels_1792": ("NONE", 0, 0),
    "channels_520": ("NONE", 0, 0),
    "imagenet_b32": ("WIDE", 128, 8),
    "row_stride_not_c": ("NONE", 0, 0),
    "batch_stride_not_n_c": ("NONE", 0, 0),
    "batch_stride_ignored_at_b1": ("WIDE", 128, 8),
    "misaligned_pointer": ("NONE", 0, 0),
    "no_fold_buffers": ("NONE", 0, 0),
    "kv_mask": ("NONE", 0, 0),
    "q_mask": ("NONE", 0, 0),
    "full_mask": ("NONE", 0, 0),
    "bias": ("NONE", 0, 0),
    "probs": ("NONE", 0, 0),
    "attn_act_split": ("NONE", 0, 0),
    "mlp_act_split": ("NONE", 0, 0),
    "no_qkv_image": ("NONE", 0, 0),
    "qkv_lo_row0_right": ("WIDE", 128, 8),
    "qkv_lo_row0_wrong": ("NONE", 0, 0),
    "fc1_lo_row0_right": ("WIDE", 128, 8),
    "fc1_lo_row0_wrong": ("NONE", 0, 0),
    "mlp_hidden_not_c": ("NONE", 0, 0),
    "dtype_mismatch": ("NONE", 0, 0),
    "head_shape_not_fused": ("NONE", 0, 0),
    "fold_qkv_rows_differ": ("NONE", 0, 0),
    "fold_qkv_k_differs": ("NONE", 0, 0),
    "fold_fc1_k_differs": ("NONE", 0, 0),
    "fold_fc1_rows_differ": ("NONE", 0, 0),
    "mode1_rows_511": ("NONE", 0, 0),
    "mode1_rows_512": ("SMALL", 64, 16),
    "mode1_rows_4095": ("SMALL", 64, 16),
    "mode1_rows_4096": ("NONE", 0, 0),
    "mode1_rows_6143": ("NONE", 0, 0),
    "mode1_rows_6144": ("WIDE", 128, 8),
    "mode2_rows_127": ("NONE", 0, 0),
    "mode2_rows_128": ("SMALL", 64, 16),
    "mode2_rows_2047": ("SMALL", 64, 16),
    "mode2_rows_2048": ("WIDE", 128, 8),
    "mode2_rows_4096": ("WIDE", 128, 8),
    "mode0_rows_8192": ("NONE", 0, 0),
    "x2s_rows_2048_mode1": ("NONE", 0, 0),
    "x2s_rows_6144_mode1": ("WIDE", 128, 8),
    "x2w_rows_2047_mode2": ("NONE", 0, 0),
    "x2w_rows_2048_mode2": ("WIDE", 128, 8),
    "x2o_rows_2048_mode1": ("NONE", 0, 0),
    "fc2_lo_rows_2048_mode1": ("NONE", 0, 0),
    "fc2_lo_rows_6144_mode1": ("WIDE", 128, 8),
}

# score_chunks: samples per pass, query rows per pass
CHUNKS = {
    "fits": (32, 512),
    "exactly_the_cap": (4, 256),
    "samples_per_pass": (32, 1024),
    "one_sample_per_pass": (1, 1024),
    "flow_2048_x_182528": (1, 1408),
    "row_chunk_floor_128": (1, 128),
    "row_chunk_capped_by_tq": (1, 100),
}

# pio_encoder_workspace_bytes' rule; the largest carve of a run with per-sample latents / with batch-invariant latents
ENCODER = {
    "imagenet": (407712512, 407712512, 397300480),
    "language": (1284531200, 1284531200, 1271555072),
    "flow": (434011136, 434011136, 434011136),
    "multimodal": (254310144, 254310144, 254310144),
}

Y16 = {"no_final_layer": 0, "k_is_padc": 1, "k_is_pad8_only": 0}

# linear_gemm: id -> every non-pointer field of the pio_gemm_t, then the pointer fields that are set.  One line per form in
# which pio_blocks.hip asks for an nn.Linear (pair16_at / f32_at / out16_at and their optional parts) at the shapes of the
# shipped models, the ragged widths 322 and 1026 included: there the pitch4 widening of N and the n_store rule turn.
LINEARS = {
    "q_plain":
        "M=1000 N=1024 K=1024 lda=1024 ldb=1024 ldc=1024 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=0 n_store=1024 dtype=0 "
        "ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,C_lo,bias",
    "q_322":
        "M=182528 N=512 K=384 lda=384 ldb=384 ldc=512 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=0 n_store=512 dtype=0 ld16=0 "
        "ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,C_lo,bias",
    "q_1026":
        "M=6288 N=512 K=1088 lda=1088 ldb=1088 ldc=512 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=0 n_store=512 dtype=0 ld16=0 "
        "ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,C_lo,bias",
    "k_plain":
        "M=16384 N=1024 K=1024 lda=1024 ldb=1024 ldc=1024 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=0 n_store=1024 dtype=0 "
        "ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,C_lo,bias",
    "k_322":
        "M=182528 N=328 K=384 lda=384 ldb=384 ldc=328 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=0 n_store=328 dtype=0 ld16=0 "
        "ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,B,C,bias",
    "qk_plain":
        "M=16384 N=2048 K=1024 lda=1024 ldb=1024 ldc=2048 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=0 n_store=2048 dtype=0 "
        "ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,B,C,bias",
    "qkv_plain":
        "M=16384 N=3072 K=1024 lda=1024 ldb=1024 ldc=3072 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=0 n_store=3072 dtype=0 "
        "ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,B,C,bias",
    "qkv_folded":
        "M=16384 N=3072 K=1024 lda=1024 ldb=1024 ldc=3072 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=0 n_store=3072 dtype=0 "
        "ld16=0 ln_eps=1e-05 b_lo_n0=0 ln_slots=8 row_slot_w=0 ptrs=A,B,C,bias,ln_part,ln_c",
    "qkv_folded_small":
        "M=600 N=3072 K=1024 lda=1024 ldb=1024 ldc=3072 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=0 n_store=3072 dtype=0 "
        "ld16=0 ln_eps=1e-05 b_lo_n0=0 ln_slots=16 row_slot_w=0 ptrs=A,B,C,bias,ln_part,ln_c",
    "qkv_folded_v_lo":
        "M=16384 N=3072 K=1024 lda=1024 ldb=1024 ldc=3072 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=0 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=0 n_store=3072 dtype=0 "
        "ld16=0 ln_eps=1e-05 b_lo_n0=2048 ln_slots=8 row_slot_w=0 ptrs=A,B,B_lo,C,ln_part,ln_c",
    "kq_322":
        "M=2048 N=328 K=328 lda=328 ldb=328 ldc=328 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=0 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=0 n_store=328 dtype=0 ld16=0 "
        "ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,B,B_lo,C",
    "out_plain":
        "M=16384 N=1024 K=1024 lda=1024 ldb=1024 ldc=1024 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=1 n_store=1024 dtype=0 "
        "ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,B,C,bias",
    "out_322_plain":
        "M=182528 N=322 K=512 lda=512 ldb=512 ldc=322 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=1 n_store=322 dtype=0 ld16=0 "
        "ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,bias",
    "out_residual":
        "M=16384 N=1024 K=1024 lda=1024 ldb=1024 ldc=1024 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=1024 r_stride_b=524288 r_rows_per_batch=512 out_f32=1 n_store=1024 "
        "dtype=0 ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,B,C,bias,R",
    "out_fold_producer":
        "M=16384 N=1024 K=1024 lda=1024 ldb=1024 ldc=1024 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=1 n_store=1024 dtype=0 "
        "ld16=1024 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=128 "
        "ptrs=A,B,bias,X16,X16_lo,row_part,R16_hi,R16_lo,range_flag",
    "out_pitch8_1024":
        "M=32000 N=1024 K=1024 lda=1024 ldb=1024 ldc=1024 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=1 n_store=1024 dtype=0 "
        "ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,bias",
    "out_pitch8_322":
        "M=182528 N=324 K=512 lda=512 ldb=512 ldc=328 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=1 n_store=328 dtype=0 ld16=0 "
        "ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,bias",
    "out_pitch8_1026":
        "M=6288 N=1028 K=512 lda=512 ldb=512 ldc=1032 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=1 n_store=1032 dtype=0 "
        "ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,B_lo,C,bias",
    "out_pitch8_vo_residual":
        "M=2048 N=512 K=328 lda=328 ldb=328 ldc=512 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=512 r_stride_b=0 r_rows_per_batch=2048 out_f32=1 n_store=512 dtype=0 "
        "ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,B,B_lo,C,bias,R",
    "out_pitch8_322_residual":
        "M=200 N=322 K=512 lda=512 ldb=512 ldc=328 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=322 r_stride_b=32200 r_rows_per_batch=100 out_f32=1 n_store=328 "
        "dtype=0 ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,B,C,bias,R",
    "fc1_plain":
        "M=16384 N=1024 K=1024 lda=1024 ldb=1024 ldc=1024 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=1 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=0 n_store=1024 dtype=0 "
        "ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,B,C,bias",
    "fc1_1026":
        "M=6288 N=1088 K=1088 lda=1088 ldb=1088 ldc=1088 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=1 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=0 n_store=1088 dtype=0 "
        "ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,C_lo,bias",
    "fc1_322":
        "M=182528 N=384 K=384 lda=384 ldb=384 ldc=384 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=1 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=0 n_store=384 dtype=0 ld16=0 "
        "ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,C_lo,bias",
    "fc1_folded":
        "M=16384 N=1024 K=1024 lda=1024 ldb=1024 ldc=1024 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=1 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=0 n_store=1024 dtype=0 "
        "ld16=0 ln_eps=1e-05 b_lo_n0=0 ln_slots=8 row_slot_w=0 ptrs=A,B,C,bias,ln_part,ln_c",
    "fc2_f32":
        "M=16384 N=1024 K=1024 lda=1024 ldb=1024 ldc=1024 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=1024 r_stride_b=524288 r_rows_per_batch=512 out_f32=1 n_store=1024 "
        "dtype=0 ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,B,C,bias,R",
    "fc2_no_residual":
        "M=16384 N=1024 K=1024 lda=1024 ldb=1024 ldc=1024 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=1 n_store=1024 dtype=0 "
        "ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,B,C,bias",
    "fc2_fold_producer":
        "M=16384 N=1024 K=1024 lda=1024 ldb=1024 ldc=1024 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=1 n_store=1024 dtype=0 "
        "ld16=1024 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=128 "
        "ptrs=A,B,C,bias,X16,X16_lo,row_part,R16_hi,R16_lo,range_flag",
    "fc2_fold_producer_no_f32":
        "M=16384 N=1024 K=1024 lda=1024 ldb=1024 ldc=1024 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=1 n_store=1024 dtype=0 "
        "ld16=1024 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=128 "
        "ptrs=A,B,bias,X16,X16_lo,row_part,R16_hi,R16_lo,range_flag",
    "fc2_f32_322_caller_pitch":
        "M=182528 N=322 K=384 lda=384 ldb=384 ldc=322 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=328 r_stride_b=59869184 r_rows_per_batch=182528 out_f32=1 n_store=322 "
        "dtype=0 ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,bias,R",
    "fc2_f32_322_pitch4":
        "M=182528 N=324 K=384 lda=384 ldb=384 ldc=324 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=328 r_stride_b=59869184 r_rows_per_batch=182528 out_f32=1 n_store=324 "
        "dtype=0 ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,bias,R",
    "fc2_f32_1026_caller_pitch":
        "M=6288 N=1026 K=1088 lda=1088 ldb=1088 ldc=1026 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=1032 r_stride_b=6489216 r_rows_per_batch=6288 out_f32=1 n_store=1026 "
        "dtype=0 ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,bias,R",
    "fc2_f32_1026_pitch4":
        "M=6288 N=1028 K=1088 lda=1088 ldb=1088 ldc=1028 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=1032 r_stride_b=6489216 r_rows_per_batch=6288 out_f32=1 n_store=1028 "
        "dtype=0 ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,bias,R",
    "fc2_f32_322_pitch4_narrow_residual":
        "M=200 N=322 K=384 lda=384 ldb=384 ldc=324 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=322 r_stride_b=32200 r_rows_per_batch=100 out_f32=1 n_store=322 "
        "dtype=0 ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,bias,R",
    "fc2_out16_1024":
        "M=32000 N=1024 K=1024 lda=1024 ldb=1024 ldc=1024 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=1024 r_stride_b=1024000 r_rows_per_batch=1000 out_f32=0 n_store=1024 "
        "dtype=0 ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,C_lo,bias,R",
    "fc2_out16_322":
        "M=182528 N=328 K=384 lda=384 ldb=384 ldc=384 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=328 r_stride_b=59869184 r_rows_per_batch=182528 out_f32=0 n_store=384 "
        "dtype=0 ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,C_lo,bias,R",
    "fc2_out16_1026":
        "M=6288 N=1032 K=1088 lda=1088 ldb=1088 ldc=1088 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=1032 r_stride_b=6489216 r_rows_per_batch=6288 out_f32=0 n_store=1088 "
        "dtype=0 ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,C_lo,bias,R",
    "final_1000":
        "M=32000 N=1000 K=1024 lda=1024 ldb=1024 ldc=1000 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=1 n_store=1000 dtype=0 "
        "ld16=0 ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,bias",
    "final_2_from_322":
        "M=182528 N=2 K=384 lda=384 ldb=384 ldc=2 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=1 n_store=2 dtype=0 ld16=0 "
        "ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,C,bias",
    "final_512_from_1026":
        "M=6288 N=512 K=1088 lda=1088 ldb=1088 ldc=512 batch=1 nh=1 sAb=0 sAh=0 sBb=0 sBh=0 sCb=0 sCh=0 "
        "bias_mode=1 act=0 alpha=1 ldr=0 r_stride_b=0 r_rows_per_batch=0 out_f32=1 n_store=512 dtype=1 ld16=0 "
        "ln_eps=0 b_lo_n0=0 ln_slots=0 row_slot_w=0 ptrs=A,A_lo,B,B_lo,C,bias",
}


POLICY_CONSTANTS = {"FP16": "fp16", "X2O": "fp16x2o", "X2S": "fp16x2s", "X2W": "fp16x2w", "X2AF": "fp16x2af",
                    "X2AFO": "fp16x2afo", "X3": "fp16x3", "X3F": "fp16x3f", "X3FQ": "fp16x3fq"}


def _policies_cpp():
    """The driver's `Policy` constants, in the order of the struct's members."""
    from perceiverio_pytorch_amd import runtime as R

    def row(n):
        vals = [R.splits(lin, n) for lin in ("proj_q", "proj_k", "proj_v", "final", "fc1", "fc2", "final_layer")]
        vals += [R.policy(n).act_split, R.attention_act_split(n), R.kv_fold_offered(n), R.ln_fold_offered(n),
                 R.qkv_stack_allowed(n)]
        return "{" + ", ".join(str(int(v)) for v in vals) + "}"
    return "static const Policy " + ", ".join(f"{c} = {row(n)}" for c, n in POLICY_CONSTANTS.items()) + ";"


def _run_driver():
    inc = os.path.join(ROOT, "include")
    csrc = os.path.join(ROOT, "perceiverio_pytorch_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "route.cpp")
        open(src, "w").write(DRIVER.replace("@POLICIES@", _policies_cpp()))
        exe = os.path.join(d, "route")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", inc, "-I", csrc, src, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    got = {"plan": {}, "fold": {}, "chunks": {}, "encoder": {}, "y16": {}, "linear": {}}
    for line in filter(None, out):
        kind, name, rest = line.split(" ", 2)
        vals = tuple(int(x) if x.lstrip("-").isdigit() else x for x in rest.split())
        got[kind][name] = rest if kind in ("plan", "linear") else vals[0] if len(vals) == 1 else vals
    return got


GOT = None


def _got():
    global GOT
    if GOT is None:
        GOT = _run_driver()
    return GOT


def _members(line):
    return {k: int(v) for k, v in (f.split("=") for f in line.split())}


def _ru256(n):
    return (n + 255) // 256 * 256


def test_plan_table():
    got = _got()["plan"]
    assert sorted(got) == sorted(PLANS)
    for name, line in PLANS.items():
        assert _members(got[name]) == _members(line), name


def test_fold_table():
    assert _got()["fold"] == FOLDS


def test_linear_table():
    got = _got()["linear"]
    assert sorted(got) == sorted(LINEARS)
    for name, line in LINEARS.items():
        assert dict(f.split("=") for f in got[name].split()) == dict(f.split("=") for f in line.split()), name


def test_score_chunks_and_y16_direct():
    assert _got()["chunks"] == CHUNKS
    assert _got()["y16"] == Y16


def test_workspace_bytes_rule_equals_what_the_run_carves():
    """Every *_workspace_bytes entry point carves the same plan with a null base: same total.  pio_encoder_workspace_bytes
    takes the maximum over the cross plan (per-sample latents) and the layer plans; the run carves exactly those plans,
    the cross plan possibly with batch-invariant latents, which never needs more."""
    for name, line in _got()["plan"].items():
        m = _members(line)
        assert m["total"] == m["null_base_total"], name
    assert _got()["encoder"] == ENCODER
    for name, (rule, run, run_q_bcast) in _got()["encoder"].items():
        assert rule == run and run_q_bcast <= rule, name


def test_offsets_are_256_byte_multiples():
    for name, line in _got()["plan"].items():
        m = _members(line)
        for k, v in m.items():
            if k == "total" or k.endswith((".hi", ".lo")) or k in ("x1", "y", "x16b", "lo_a", "lo_b", "part_a", "part_b",
                                                                   "core.scores", "core.xpart"):
                assert v == -1 or v % 256 == 0, (name, k, v)


def test_q16_k16_vt16_are_adjacent():
    """attention_core's fused q|k|v (and q|k) projection writes one matrix across the q16 | k16 | vt16 carves
    (qkv_adjacent): without split activations nothing lies between them."""
    seen = 0
    for name, line in _got()["plan"].items():
        m = _members(line)
        if "core.q16.hi" not in m or m["split"]:
            continue
        assert m["core.k16.hi"] == m["core.q16.hi"] + _ru256(m["qbytes"]), name
        assert m["core.vt16.hi"] == m["core.k16.hi"] + _ru256(m["kbytes"]), name
        seen += 1
    assert seen >= 20


def test_in_place_aliases():
    """The in-place residual stream: x16b is x16.hi, lo_b is lo_a, and the hidden activations take the attention output's
    buffer when they fit (padc(hidden) <= heads * dvp)."""
    p = {k: _members(v) for k, v in _got()["plan"].items()}
    for name in ("imagenet_stack_b4_inplace", "stack_x2w_1024_inplace", "alias_edge_hidden_equal"):
        m = p[name]
        assert m["x16b"] == m["x16.hi"] and m["lo_b"] == m["lo_a"] and m["h16.hi"] == m["core.o16.hi"], name
    m = p["alias_edge_hidden_greater"]
    assert m["x16b"] == m["x16.hi"] and m["lo_b"] == m["lo_a"] and m["h16.hi"] != m["core.o16.hi"]
    assert p["no_fold_offered_widening_4"]["x16b"] == -1


def test_header_is_host_only():
    """No HIP include, no environment read, no state: the header compiles with a plain C++ compiler (above) and names none."""
    src = open(os.path.join(ROOT, "perceiverio_pytorch_amd", "csrc", "pio_block_route.h")).read()
    assert "hip_runtime" not in src and "getenv" not in src and "static " not in src
