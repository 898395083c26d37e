"""CPU: which core every attention call runs on, what its plan carves and which variant of the self-attention kernel a
launch gets (perceiverio_pytorch_amd/csrc/pio_attn_route.h, compiled with g++ into a small driver; the descriptors carry
fake, aligned pointers that are never dereferenced).  The cases are the attention shapes of the four shipped models under
their default policies and under "fp16x3fq", plus the edge of every rule; then the launch plans of the three fused cores
(accepted plans and every refusal, with calls that break two rules at once to pin the order of the checks).  The expected values were produced by the
predicates and the attention_core ladder the header replaced (a sweep of 5.1e9 calls showed no disagreement); the table
is a readable extract of it.  The launch-plan rows (FPLAN, XPLAN, TPLAN) were read off the three launchers as they stood
before the plans existed: the order of their refusals and their grid arithmetic."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''
#include <stdio.h>
#include "pio_attn_route.h"
using namespace pio;

static const char *name(AttnCore k) {
    switch (k) {
    case AttnCore::QKV_FLASH: return "QKV_FLASH";
    case AttnCore::KVFOLD_XATTN: return "KVFOLD_XATTN";
    case AttnCore::KVFOLD_XTALL: return "KVFOLD_XTALL";
    case AttnCore::PAIR_FLASH: return "PAIR_FLASH";
    case AttnCore::PAIR_XATTN: return "PAIR_XATTN";
    case AttnCore::FLASH: return "FLASH";
    case AttnCore::XATTN: return "XATTN";
    case AttnCore::XTALL: return "XTALL";
    default: return "MATERIALISED";
    }
}
// id core fuse_qk qk_pair out_pair need_scores xpart_bytes | plan (lean): fused xpart_bytes | the un-masked call: fused
static void show(const char *id, const pio_attention_t &a, const AttnCall &c) {
    const AttnRoute r = attn_route(a, c);
    if (r.err) {
        printf("route %s %s\n", id, r.err == PIO_E_SHAPE ? "PIO_E_SHAPE" : r.err == PIO_E_ARG ? "PIO_E_ARG" : "error");
        return;
    }
    AttnCall plain = c;
    plain.kv_mask = plain.q_mask = plain.full_mask = plain.bias = plain.probs = false;
    const AttnRoute p = attn_plan(a, c.B, c.Bq, c.Tq, c.Tk, true), u = attn_route(a, plain);
    printf("route %s %s %d %d %d %d %zu %d %zu %d\n", id, name(r.core), r.fuse_qk, r.qk_pair, r.out_pair, r.need_scores,
           r.xpart_bytes, !p.need_scores, p.xpart_bytes, u.core != AttnCore::MATERIALISED);
}
static void splits(const char *id, int dkp, int dvp, int B, int H, int Tq, int Tk) {
    printf("splits %s %d %zu\n", id, xattn_splits(dkp, dvp, B, H, Tq, Tk), xattn_partial_bytes(dkp, dvp, B, H, Tq, Tk));
}
static void flash(const char *id, int dkp, int dvp, int B, int H, int Tq, int Tk, bool v_rowmajor, bool ksplit_on) {
    const FlashRoute r = flash_route(dkp, dvp, B, H, Tq, Tk, v_rowmajor, ksplit_on, 256);
    printf("flash %s %s %d %d %d %d\n", id, r.v_rowmajor ? "row" : "V^T", r.NW, r.KS, r.nqt, r.threads);
}
static const void *W = (const void *)(uintptr_t)0x10000000;   // a fake, aligned pointer: never dereferenced

// Attention descriptor as the Python front end packs it: heads of (dk, dv) channels, every stacked image offered
static pio_attention_t attn(int heads, int dk, int dv, int act_split = 0, int dtype = PIO_DT_F16, int kv_in = 0) {
    pio_attention_t a = {};
    const int dkp = (dk + 7) & ~7, dvp = (dv + 7) & ~7;
    a.heads = heads; a.dk = dk; a.dv = dv; a.dkp = dkp; a.dvp = dvp; a.dtype = dtype; a.act_split = act_split;
    a.q_in = a.out = heads * dv; a.k_in = a.v_in = kv_in ? kv_in : heads * dv;
    a.q.w_hi = a.k.w_hi = a.v.w_hi = a.o.w_hi = W;
    a.qk.w_hi = W; a.qk.n = 2 * heads * dkp;
    a.qkv.w_hi = W; a.qkv.n = 2 * heads * dkp + heads * dvp;
    return a;
}
// ... with the K / V projection fold packed (single head, dk == dv == kv channels)
static pio_attention_t kvfold(int c, int act_split = 0) {
    pio_attention_t a = attn(1, c, c, act_split, PIO_DT_F16, c);
    a.kq.w_hi = a.vo.w_hi = W; a.kq.k = a.dkp; a.kq.n = a.vo.k = (c + 7) & ~7;
    return a;
}
// self-attention call: one input for q, k and v, adjacent scratch
static AttnCall self_call(int B, int T) {
    AttnCall c = {};
    c.B = c.Bq = B; c.Tq = c.Tk = T; c.same_qk = c.same_kv = true; c.kv_fold_on = true; c.qkv_adjacent = c.qk_adjacent = true;
    return c;
}
// cross-attention call: k and v read the same input
static AttnCall cross_call(int B, int Tq, int Tk, bool q_bcast = false) {
    AttnCall c = {};
    c.B = B; c.Bq = q_bcast ? 1 : B; c.Tq = Tq; c.Tk = Tk; c.q_bcast = q_bcast; c.same_kv = true; c.kv_fold_on = true;
    c.qk_adjacent = true;
    return c;
}
static AttnCall with(AttnCall c, bool AttnCall::*flag) { c.*flag = true; return c; }

static void cases() {
    // fused q|k|v: the four head shapes of the self-attention kernel
    show("qkv_128_128_imagenet_stack", attn(8, 128, 128), self_call(32, 512));
    show("qkv_64_64", attn(8, 64, 64), self_call(2, 256));
    show("qkv_32_32_flow_stack", attn(16, 32, 32), self_call(1, 2048));
    show("qkv_32_160_language_stack", attn(8, 32, 160), self_call(2, 256));
    pio_attention_t a = attn(8, 128, 128);
    a.qkv.w_lo = W; a.qkv.lo_row0 = 2 * 8 * 128;
    show("qkv_lo_image_outside_the_fold", a, self_call(32, 512));            // -> q|k, not q|k|v
    AttnCall c = self_call(32, 512);
    c.fold_in = c.fold_out = true; c.fold_qkv = &a.qkv;
    show("qkv_lo_image_inside_the_fold", a, c);
    show("qkv_scratch_not_adjacent", attn(8, 128, 128), [] { AttnCall c = self_call(32, 512); c.qkv_adjacent = false; return c; }());
    // the same block with masks
    show("stack_kv_mask", attn(8, 128, 128), with(self_call(32, 512), &AttnCall::kv_mask));
    show("stack_q_mask", attn(8, 128, 128), with(self_call(32, 512), &AttnCall::q_mask));
    show("stack_full_mask", attn(8, 128, 128), with(self_call(32, 512), &AttnCall::full_mask));
    show("stack_bias", attn(8, 128, 128), with(self_call(32, 512), &AttnCall::bias));
    show("stack_probs", attn(8, 128, 128), with(self_call(32, 512), &AttnCall::probs));
    // act_split on the language heads (32, 160), 8 heads
    for (int s = 1; s <= 3; ++s) {
        char id[64];
        snprintf(id, sizeof id, "language_act_split_%d", s);
        show(id, attn(8, 32, 160, s), self_call(2, 256));
        snprintf(id, sizeof id, "language_act_split_%d_kv_mask", s);
        show(id, attn(8, 32, 160, s), with(cross_call(2, 256, 2048, true), &AttnCall::kv_mask));
    }
    show("language_decoder_32_96_pair_q_mask", attn(8, 32, 96, 3), with(cross_call(2, 2048, 256), &AttnCall::q_mask));
    show("pair_request_wide_head", attn(1, 512, 512, 3), cross_call(2, 384, 1024));
    show("pair_request_bf16", attn(8, 32, 160, 3, PIO_DT_BF16), self_call(2, 256));
    // single wide heads
    show("flow_encoder_328", attn(1, 322, 322, 0, PIO_DT_F16, 64), cross_call(1, 2048, 182528, true));
    show("decoder_512", attn(1, 512, 512, 0, PIO_DT_F16, 64), cross_call(1, 2048, 2048));
    show("multimodal_encoder_704", attn(1, 704, 704, 0, PIO_DT_F16, 64), with(cross_call(1, 784, 52128, true), &AttnCall::kv_mask));
    show("imagenet_decoder_1024_over_512", attn(1, 1024, 1024), cross_call(8, 1000, 512, true));
    show("wide_1024_over_520", attn(1, 1024, 1024), cross_call(8, 1000, 520, true));
    show("wide_1024_over_512_x3f", attn(1, 1024, 1024, 2), cross_call(8, 1000, 512, true));
    // the K / V fold: taken, then refused by each condition in turn
    show("kvfold_xattn", kvfold(322), cross_call(1, 2048, 182528, true));
    show("kvfold_xattn_x3f", kvfold(322, 2), cross_call(1, 2048, 182528, true));
    show("kvfold_xtall", kvfold(1024), cross_call(8, 100, 512));
    show("kvfold_kv_mask", kvfold(322), with(cross_call(1, 2048, 182528, true), &AttnCall::kv_mask));
    show("kvfold_too_few_keys", kvfold(322), cross_call(2, 1024, 4095));     // 4 Bq Tq > B Tk
    show("kvfold_enough_keys", kvfold(322), cross_call(2, 1024, 4096));
    show("kvfold_query_cache", kvfold(322), with(cross_call(1, 2048, 182528, true), &AttnCall::qcache));
    show("kvfold_act_split_1", kvfold(322, 1), cross_call(1, 2048, 182528, true));
    show("kvfold_act_split_3", kvfold(322, 3), cross_call(1, 2048, 182528, true));
    show("kvfold_switch_off", kvfold(322), [] { AttnCall c = cross_call(1, 2048, 182528, true); c.kv_fold_on = false; return c; }());
    // the query cache and batch-invariant queries keep Q and K apart
    show("self_with_query_cache", attn(8, 128, 128), with(self_call(32, 512), &AttnCall::qcache));
    show("self_with_q_bcast", attn(8, 128, 128), [] { AttnCall c = self_call(32, 512); c.q_bcast = true; c.Bq = 1; return c; }());
    show("multimodal_decoder_query_cache", attn(1, 512, 512, 2, PIO_DT_F16, 64), with(cross_call(1, 8192, 784, true), &AttnCall::qcache));
    // a fold wired to a call that cannot take the q|k|v form
    c = with(self_call(32, 512), &AttnCall::kv_mask);
    c.fold_in = c.fold_out = true;
    show("fold_with_kv_mask", attn(8, 128, 128), c);
    c = self_call(32, 512);
    c.fold_out = true;
    show("fold_on_split_activations", attn(8, 128, 128, 2), c);
}

static void split_cases() {
    splits("flow_encoder", 328, 328, 1, 1, 2048, 182528);
    splits("flow_decoder", 512, 512, 1, 1, 182528, 2048);
    splits("language_encoder", 32, 160, 2, 8, 256, 2048);
    splits("tiny", 32, 32, 2, 2, 128, 128);
}

static void flash_cases() {
    flash("imagenet_b32", 128, 128, 32, 8, 512, 512, true, true);
    flash("imagenet_b1", 128, 128, 1, 8, 512, 512, true, true);
    flash("narrow_small_batch", 32, 32, 1, 16, 2048, 2048, true, true);
    flash("narrow_64_small_batch", 64, 64, 1, 8, 1024, 1024, true, true);
    flash("wide_head_many_keys", 128, 128, 1, 8, 1024, 1024, true, true);   // dk > 64: two key parts, not four
    flash("tk_not_multiple_of_128", 128, 128, 1, 8, 512, 500, true, true);
    flash("ksplit_off", 128, 128, 1, 8, 512, 512, true, false);
    flash("v_transposed", 32, 160, 2, 8, 256, 256, false, true);
    flash("v_transposed_b32", 128, 128, 32, 8, 512, 512, false, true);
}

// ---- launch plans: what the three launchers decide before they fill their kernel's parameters ----------------------
static const char *code(int err) {
    return err == PIO_E_ARG ? "PIO_E_ARG" : err == PIO_E_SHAPE ? "PIO_E_SHAPE" : err == PIO_E_ALIGN ? "PIO_E_ALIGN"
           : err == PIO_E_WORKSPACE ? "PIO_E_WORKSPACE" : "error";
}
// operands of a well-formed call: dense [T][H*d] rows, V^T rows padded to 64 keys, aligned fake pointers
static AttnOperands ops(int H, int dkp, int dvp, int Tq, int Tk, bool v_rowmajor = false) {
    AttnOperands t = {};
    t.Q = t.K = t.VT = W; t.O = (void *)W;
    t.ldq = t.ldk = (int64_t)H * dkp; t.ldo = (int64_t)H * dvp;
    t.ldvt = v_rowmajor ? (int64_t)H * dvp : (Tk + 63) / 64 * 64;
    t.sQb = Tq * t.ldq; t.sKb = Tk * t.ldk; t.sOb = Tq * t.ldo;
    t.sVb = v_rowmajor ? Tk * t.ldvt : (int64_t)H * dvp * t.ldvt;
    return t;
}
static void *const LO = (void *)(uintptr_t)0x20000000;
static void as_pair(AttnOperands &t) { t.Q_lo = t.K_lo = LO; }
static void none(AttnOperands &) {}
typedef void (*Edit)(AttnOperands &);

// fplan id: V layout, NW, KS, nqt, pair, o_rows16, grid
static void fplan(const char *id, int dtype, int dkp, int dvp, int B, int H, int Tq, int Tk, bool vrow, Edit edit = none) {
    AttnOperands t = ops(H, dkp, dvp, Tq, Tk, vrow);
    edit(t);
    const FlashPlan p = flash_launch_plan(dtype, dkp, dvp, t, B, H, Tq, Tk, vrow, true, 256);
    if (p.err) printf("fplan %s %s\n", id, code(p.err));
    else printf("fplan %s %s %d %d %d %d %d %lld\n", id, p.route.v_rowmajor ? "row" : "V^T", p.route.NW, p.route.KS,
                p.route.nqt, p.pair, p.o_rows16, (long long)p.grid);
}
// xplan id: dkl, dvs, pair, nqt, nslice, nsplit, ntiles, tiles_per_split, grid, part_o_off, part_ml_off
static void xplan(const char *id, int dtype, int dkp, int dvp, int B, int H, int Tq, int Tk, bool mask, bool scratch,
                  Edit edit = none) {
    AttnOperands t = ops(H, dkp, dvp, Tq, Tk);
    edit(t);
    const XattnPlan p = xattn_launch_plan(dtype, dkp, dvp, t, B, H, Tq, Tk, mask, scratch);
    if (p.err) printf("xplan %s %s\n", id, code(p.err));
    else printf("xplan %s %d %d %d %d %d %d %d %d %lld %zu %zu\n", id, p.cfg.dkl, p.cfg.dvs, p.pair, p.nqt, p.nslice,
                p.nsplit, p.ntiles, p.tiles_per_split, (long long)p.grid, p.part_o_off, p.part_ml_off);
}
// tplan id: nqt, nka, npass, grid
static void tplan(const char *id, int dkp, int dvp, int B, int H, int Tq, int Tk, bool mask, bool scratch, Edit edit = none) {
    AttnOperands t = ops(H, dkp, dvp, Tq, Tk);
    edit(t);
    const XtallPlan p = xtall_launch_plan(dkp, dvp, t, B, H, Tq, Tk, mask, scratch);
    if (p.err) printf("tplan %s %s\n", id, code(p.err));
    else printf("tplan %s %d %d %d %lld\n", id, p.nqt, p.nka, p.npass, (long long)p.grid);
}
// one edit per alignment rule of attn_operands_aligned
static const struct { const char *name; Edit edit; } MISALIGNED[] = {
    {"ldq", [](AttnOperands &t) { t.ldq += 4; }},   {"ldk", [](AttnOperands &t) { t.ldk += 4; }},
    {"ldvt", [](AttnOperands &t) { t.ldvt += 4; }}, {"ldo", [](AttnOperands &t) { t.ldo += 2; }},
    {"sQb", [](AttnOperands &t) { t.sQb += 4; }},   {"sKb", [](AttnOperands &t) { t.sKb += 4; }},
    {"sVb", [](AttnOperands &t) { t.sVb += 4; }},   {"sOb", [](AttnOperands &t) { t.sOb += 2; }},
    {"Q_ptr", [](AttnOperands &t) { t.Q = (const char *)t.Q + 8; }},
    {"O_ptr", [](AttnOperands &t) { t.O = (char *)t.O + 4; }},
};

static void plan_cases() {
    const int F16 = PIO_DT_F16, BF16 = PIO_DT_BF16;
    char id[64];
    // ---- self-attention kernel: one plan per instantiation group of flash_launch
    fplan("vt_4_1", F16, 32, 160, 2, 8, 256, 256, false);
    fplan("row_4_1", F16, 128, 128, 1, 8, 512, 500, true);
    fplan("row_8_1", BF16, 128, 128, 32, 8, 512, 512, true);
    fplan("row_8_2", F16, 128, 128, 1, 8, 512, 512, true);
    fplan("row_16_4", F16, 32, 32, 1, 16, 2048, 2048, true);
    fplan("pair_128_no_key_split", F16, 128, 128, 1, 8, 512, 512, true, as_pair);
    fplan("pair_32_key_split", F16, 32, 32, 1, 16, 2048, 2048, true, as_pair);
    fplan("rows16_off_ldo", F16, 128, 128, 1, 8, 512, 512, true, [](AttnOperands &t) { t.ldo += 4; });
    fplan("rows16_off_O_ptr", F16, 128, 128, 1, 8, 512, 512, true, [](AttnOperands &t) { t.O = (char *)t.O + 8; });
    fplan("rows16_off_O_lo", F16, 128, 128, 1, 8, 512, 512, true, [](AttnOperands &t) { as_pair(t); t.O_lo = LO; });
    fplan("no_shape", F16, 64, 128, 1, 8, 512, 512, true);
    fplan("no_Q", F16, 128, 128, 1, 8, 512, 512, true, [](AttnOperands &t) { t.Q = nullptr; });
    fplan("no_VT", F16, 128, 128, 1, 8, 512, 512, true, [](AttnOperands &t) { t.VT = nullptr; });
    fplan("Q_lo_alone", F16, 128, 128, 1, 8, 512, 512, true, [](AttnOperands &t) { t.Q_lo = LO; });
    fplan("O_lo_without_pair", F16, 128, 128, 1, 8, 512, 512, true, [](AttnOperands &t) { t.O_lo = LO; });
    fplan("pair_64", F16, 64, 64, 1, 8, 512, 512, true, as_pair);
    fplan("pair_bf16", BF16, 32, 32, 1, 8, 512, 512, true, as_pair);
    fplan("no_batch", F16, 128, 128, 0, 8, 512, 512, true);
    fplan("no_keys", F16, 128, 128, 1, 8, 512, 0, true);
    fplan("grid_overflow", F16, 32, 32, 1 << 20, 1 << 10, 512, 512, true);
    for (const auto &m : MISALIGNED) {
        snprintf(id, sizeof id, "misaligned_%s", m.name);
        fplan(id, F16, 128, 128, 1, 8, 512, 512, true, m.edit);
    }
    fplan("no_shape_before_no_Q", F16, 64, 128, 1, 8, 512, 512, true, [](AttnOperands &t) { t.Q = nullptr; });
    fplan("O_lo_without_pair_before_misaligned", F16, 128, 128, 1, 8, 512, 512, true, [](AttnOperands &t) { t.O_lo = LO; t.ldq += 4; });
    fplan("no_batch_before_misaligned", F16, 128, 128, 0, 8, 512, 512, true, [](AttnOperands &t) { t.ldq += 4; });
    // ---- cross-attention kernel: one plan per XCfg, a key split, a mask
    xplan("cfg_32_96", F16, 32, 96, 2, 8, 256, 256, false, false);
    xplan("cfg_32_160_pair", F16, 32, 160, 2, 8, 256, 256, false, false, as_pair);
    xplan("cfg_128_128", BF16, 128, 128, 2, 8, 256, 256, false, false);
    xplan("cfg_352_352", F16, 328, 328, 2, 1, 256, 256, false, false);
    xplan("cfg_512_512", F16, 512, 512, 2, 1, 256, 256, false, false);
    xplan("cfg_704_256_sliced", F16, 704, 704, 2, 1, 256, 256, false, false);
    xplan("key_split_flow_encoder", F16, 328, 328, 1, 1, 2048, 182528, false, true);
    xplan("masked_language_encoder", F16, 32, 160, 2, 8, 256, 2048, true, true);
    xplan("no_cfg", F16, 1024, 1024, 2, 1, 256, 256, false, false);
    xplan("no_K", F16, 32, 96, 2, 8, 256, 256, false, false, [](AttnOperands &t) { t.K = nullptr; });
    xplan("no_VT", F16, 32, 96, 2, 8, 256, 256, false, false, [](AttnOperands &t) { t.VT = nullptr; });
    xplan("K_lo_alone", F16, 32, 96, 2, 8, 256, 256, false, false, [](AttnOperands &t) { t.K_lo = LO; });
    xplan("pair_128", F16, 128, 128, 2, 8, 256, 256, false, false, as_pair);
    xplan("pair_bf16", BF16, 32, 96, 2, 8, 256, 256, false, false, as_pair);
    xplan("no_keys", F16, 32, 96, 2, 8, 256, 0, false, false);
    xplan("dkp_not_padded", F16, 36, 96, 2, 8, 256, 256, false, false);
    for (const auto &m : MISALIGNED) {
        snprintf(id, sizeof id, "misaligned_%s", m.name);
        xplan(id, F16, 32, 96, 2, 8, 256, 256, false, false, m.edit);
    }
    xplan("ldvt_below_8", F16, 32, 96, 2, 8, 256, 256, false, false, [](AttnOperands &t) { t.ldvt = 0; });
    xplan("ldk_offset_limit", F16, 32, 96, 2, 8, 256, 256, false, false, [](AttnOperands &t) { t.ldk = 1ll << 26; });
    xplan("ldvt_offset_limit", F16, 512, 512, 2, 1, 256, 256, false, false, [](AttnOperands &t) { t.ldvt = 1ll << 22; });
    xplan("mask_without_scratch", F16, 32, 160, 2, 8, 256, 256, true, false);
    xplan("split_without_scratch", F16, 328, 328, 1, 1, 2048, 182528, false, false);
    xplan("ldvt_not_whole_tiles", F16, 32, 96, 2, 8, 256, 256, false, false, [](AttnOperands &t) { t.ldvt = 264; });
    xplan("grid_overflow", F16, 32, 96, 1 << 20, 1 << 10, 256, 256, false, false);
    xplan("no_scratch_before_ldvt_tiles", F16, 32, 160, 2, 8, 256, 256, true, false, [](AttnOperands &t) { t.ldvt = 264; });
    xplan("pair_128_before_misaligned", F16, 128, 128, 2, 8, 256, 256, false, false, [](AttnOperands &t) { as_pair(t); t.ldq += 4; });
    xplan("ldk_limit_before_no_scratch", F16, 32, 160, 2, 8, 256, 256, true, false, [](AttnOperands &t) { t.ldk = 1ll << 26; });
    // ---- tall-head kernel
    tplan("one_pass", 64, 256, 2, 2, 200, 100, false, false);
    tplan("imagenet_decoder_four_passes", 1024, 1024, 8, 1, 1000, 512, true, true);
    tplan("too_many_keys", 1024, 1024, 8, 1, 1000, 520, false, false);
    tplan("pair", 1024, 1024, 8, 1, 1000, 512, false, false, as_pair);
    tplan("no_O", 1024, 1024, 8, 1, 1000, 512, false, false, [](AttnOperands &t) { t.O = nullptr; });
    tplan("no_VT", 1024, 1024, 8, 1, 1000, 512, false, false, [](AttnOperands &t) { t.VT = nullptr; });
    tplan("no_queries", 1024, 1024, 8, 1, 0, 512, false, false);
    for (const auto &m : MISALIGNED) {
        snprintf(id, sizeof id, "misaligned_%s", m.name);
        tplan(id, 1024, 1024, 8, 1, 1000, 512, false, false, m.edit);
    }
    tplan("ldvt_below_64", 1024, 1024, 8, 1, 1000, 512, false, false, [](AttnOperands &t) { t.ldvt = 32; });
    tplan("ldk_offset_limit", 1024, 1024, 8, 1, 1000, 512, false, false, [](AttnOperands &t) { t.ldk = 1ll << 22; });
    tplan("ldq_offset_limit", 1024, 1024, 8, 1, 1024, 512, false, false, [](AttnOperands &t) { t.ldq = 1ll << 21; });
    tplan("ldvt_offset_limit", 1024, 1024, 8, 1, 1000, 512, false, false, [](AttnOperands &t) { t.ldvt = 1ll << 23; });
    tplan("mask_without_scratch", 1024, 1024, 8, 1, 1000, 512, true, false);
    tplan("grid_overflow", 64, 256, 1 << 20, 1 << 11, 128, 512, false, false);
    tplan("Q_lo_alone_is_a_shape", 1024, 1024, 8, 1, 1000, 512, false, false, [](AttnOperands &t) { t.Q_lo = LO; });
    tplan("ldvt_below_64_before_no_scratch", 1024, 1024, 8, 1, 1000, 512, true, false, [](AttnOperands &t) { t.ldvt = 32; });
    tplan("no_O_before_no_queries", 1024, 1024, 8, 1, 0, 512, false, false, [](AttnOperands &t) { t.O = nullptr; });
}
int main() {
    cases();
    split_cases();
    flash_cases();
    plan_cases();
    return 0;
}
'''

# id -> (core, fuse_qk, Q / K as pairs, output pair, score buffers, xpart bytes,
#        plan (lean): fused core promised, xpart bytes; the same call without masks / bias / probabilities: fused core)
# or the error code
ROUTES = {
    "qkv_128_128_imagenet_stack": ("QKV_FLASH", 0, 0, 0, 0, 2048, 1, 2048, 1),
    "qkv_64_64": ("QKV_FLASH", 0, 0, 0, 0, 256, 1, 256, 1),
    "qkv_32_32_flow_stack": ("QKV_FLASH", 0, 0, 0, 0, 8913664, 1, 8913664, 1),
    "qkv_32_160_language_stack": ("QKV_FLASH", 0, 0, 0, 0, 256, 1, 256, 1),
    "qkv_lo_image_outside_the_fold": ("FLASH", 1, 0, 0, 0, 2048, 1, 2048, 1),
    "qkv_lo_image_inside_the_fold": ("QKV_FLASH", 0, 0, 0, 0, 2048, 1, 2048, 1),
    "qkv_scratch_not_adjacent": ("FLASH", 1, 0, 0, 0, 2048, 1, 2048, 1),
    "stack_kv_mask": ("XATTN", 1, 0, 0, 0, 2048, 1, 2048, 1),
    "stack_q_mask": ("XATTN", 1, 0, 0, 0, 2048, 1, 2048, 1),
    "stack_full_mask": ("MATERIALISED", 1, 0, 0, 1, 2048, 1, 2048, 1),
    "stack_bias": ("MATERIALISED", 1, 0, 0, 1, 2048, 1, 2048, 1),
    "stack_probs": ("MATERIALISED", 1, 0, 0, 1, 2048, 1, 2048, 1),
    "language_act_split_1": ("MATERIALISED", 0, 1, 1, 1, 0, 0, 0, 0),
    "language_act_split_1_kv_mask": ("MATERIALISED", 0, 1, 1, 1, 0, 0, 0, 0),
    "language_act_split_2": ("XATTN", 0, 0, 1, 0, 256, 1, 256, 1),
    "language_act_split_2_kv_mask": ("XATTN", 0, 0, 1, 0, 21234688, 1, 21234688, 1),
    "language_act_split_3": ("PAIR_FLASH", 0, 1, 1, 0, 256, 1, 256, 1),
    "language_act_split_3_kv_mask": ("PAIR_XATTN", 0, 1, 1, 0, 21234688, 1, 21234688, 1),
    "language_decoder_32_96_pair_q_mask": ("PAIR_XATTN", 0, 1, 1, 0, 256, 1, 256, 1),
    "pair_request_wide_head": ("MATERIALISED", 0, 1, 1, 1, 0, 0, 0, 0),
    "pair_request_bf16": ("MATERIALISED", 0, 1, 1, 1, 0, 0, 0, 0),
    "flow_encoder_328": ("XATTN", 0, 0, 0, 0, 43277312, 1, 43277312, 1),
    "decoder_512": ("XATTN", 0, 0, 0, 0, 33686272, 1, 33686272, 1),
    "multimodal_encoder_704": ("XATTN", 0, 0, 0, 0, 28789376, 1, 28789376, 1),
    "imagenet_decoder_1024_over_512": ("XTALL", 0, 0, 0, 0, 512, 1, 512, 1),
    "wide_1024_over_520": ("MATERIALISED", 0, 0, 0, 1, 0, 0, 0, 0),
    "wide_1024_over_512_x3f": ("XTALL", 0, 0, 1, 0, 512, 1, 512, 1),
    "kvfold_xattn": ("KVFOLD_XATTN", 0, 0, 0, 0, 43277312, 1, 43277312, 1),
    "kvfold_xattn_x3f": ("KVFOLD_XATTN", 0, 0, 1, 0, 43277312, 1, 43277312, 1),
    "kvfold_xtall": ("KVFOLD_XTALL", 0, 0, 0, 0, 512, 1, 512, 1),
    "kvfold_kv_mask": ("XATTN", 0, 0, 0, 0, 43277312, 1, 43277312, 1),
    "kvfold_too_few_keys": ("XATTN", 0, 0, 0, 0, 43255296, 1, 43255296, 1),
    "kvfold_enough_keys": ("KVFOLD_XATTN", 0, 0, 0, 0, 43255296, 1, 43255296, 1),
    "kvfold_query_cache": ("XATTN", 0, 0, 0, 0, 43277312, 1, 43277312, 1),
    "kvfold_act_split_1": ("MATERIALISED", 0, 1, 1, 1, 0, 0, 0, 0),
    "kvfold_act_split_3": ("MATERIALISED", 0, 1, 1, 1, 0, 0, 0, 0),
    "kvfold_switch_off": ("XATTN", 0, 0, 0, 0, 43277312, 1, 43277312, 1),
    "self_with_query_cache": ("FLASH", 0, 0, 0, 0, 2048, 1, 2048, 1),
    "self_with_q_bcast": ("FLASH", 0, 0, 0, 0, 2048, 1, 2048, 1),
    "multimodal_decoder_query_cache": ("XATTN", 0, 0, 1, 0, 50529024, 1, 50529024, 1),
    "fold_with_kv_mask": "PIO_E_SHAPE",
    "fold_on_split_activations": "PIO_E_SHAPE",
}

# xattn_splits, xattn_partial_bytes
SPLITS = {
    "flow_encoder": (16, 43277312),
    "flow_decoder": (1, 256),
    "language_encoder": (8, 21234688),
    "tiny": (1, 256),
}

# flash_route at 256 CUs: V layout, waves per workgroup, key parts, query tiles, block threads
FLASH = {
    "imagenet_b32": ("row", 8, 1, 2, 512),
    "imagenet_b1": ("row", 8, 2, 4, 512),
    "narrow_small_batch": ("row", 16, 4, 16, 1024),
    "narrow_64_small_batch": ("row", 16, 4, 8, 1024),
    "wide_head_many_keys": ("row", 8, 2, 8, 512),
    "tk_not_multiple_of_128": ("row", 4, 1, 4, 256),
    "ksplit_off": ("row", 4, 1, 4, 256),
    "v_transposed": ("V^T", 4, 1, 2, 256),
    "v_transposed_b32": ("V^T", 4, 1, 4, 256),
}

# flash_launch_plan at 256 CUs, key split on: V layout, NW, KS, query tiles, pair, o_rows16, grid -- or the refusal.
# Expected values read off flash_attention_launch as it stood before the plan existed: flash_supported, operands
# present, O_lo without a pair, pair support, extents and grid, alignment -- in that order.
FPLAN = {
    "vt_4_1": ("V^T", 4, 1, 2, 0, 1, 32),
    "row_4_1": ("row", 4, 1, 4, 0, 1, 32),
    "row_8_1": ("row", 8, 1, 2, 0, 1, 512),
    "row_8_2": ("row", 8, 2, 4, 0, 1, 32),
    "row_16_4": ("row", 16, 4, 16, 0, 1, 256),
    "pair_128_no_key_split": ("row", 4, 1, 4, 1, 1, 32),
    "pair_32_key_split": ("row", 16, 4, 16, 1, 1, 256),
    "rows16_off_ldo": ("row", 8, 2, 4, 0, 0, 32),
    "rows16_off_O_ptr": ("row", 8, 2, 4, 0, 0, 32),
    "rows16_off_O_lo": ("row", 4, 1, 4, 1, 0, 32),
    "no_shape": "PIO_E_SHAPE",
    "no_Q": "PIO_E_ARG",
    "no_VT": "PIO_E_ARG",
    "Q_lo_alone": "PIO_E_ARG",
    "O_lo_without_pair": "PIO_E_ARG",
    "pair_64": "PIO_E_SHAPE",
    "pair_bf16": "PIO_E_SHAPE",
    "no_batch": "PIO_E_SHAPE",
    "no_keys": "PIO_E_SHAPE",
    "grid_overflow": "PIO_E_SHAPE",
    "misaligned_ldq": "PIO_E_ALIGN",
    "misaligned_ldk": "PIO_E_ALIGN",
    "misaligned_ldvt": "PIO_E_ALIGN",
    "misaligned_ldo": "PIO_E_ALIGN",
    "misaligned_sQb": "PIO_E_ALIGN",
    "misaligned_sKb": "PIO_E_ALIGN",
    "misaligned_sVb": "PIO_E_ALIGN",
    "misaligned_sOb": "PIO_E_ALIGN",
    "misaligned_Q_ptr": "PIO_E_ALIGN",
    "misaligned_O_ptr": "PIO_E_ALIGN",
    "no_shape_before_no_Q": "PIO_E_SHAPE",
    "O_lo_without_pair_before_misaligned": "PIO_E_ARG",
    "no_batch_before_misaligned": "PIO_E_SHAPE",
}

# xattn_launch_plan: XCfg (dkl, dvs), pair, nqt, nslice, nsplit, ntiles, tiles_per_split, grid, byte offsets of part_o /
# part_ml in the scratch -- or the refusal.  Order in xattn_launch: cfg, operands present, pair support, extents and
# padded widths, alignment, the 32-bit offset limits, scratch, ldvt % 32, grid.
XPLAN = {
    "cfg_32_96": (32, 96, 0, 2, 1, 1, 8, 8, 32, 256, 1573120),
    "cfg_32_160_pair": (32, 160, 1, 2, 1, 1, 8, 8, 32, 256, 2621696),
    "cfg_128_128": (128, 128, 0, 2, 1, 1, 8, 8, 32, 256, 2097408),
    "cfg_352_352": (352, 352, 0, 2, 1, 1, 8, 8, 4, 256, 672000),
    "cfg_512_512": (512, 512, 0, 2, 1, 1, 8, 8, 4, 256, 1048832),
    "cfg_704_256_sliced": (704, 256, 0, 2, 3, 1, 8, 8, 12, 256, 1442048),
    "key_split_flow_encoder": (352, 352, 0, 16, 1, 16, 5704, 357, 256, 23040, 43014656),
    "masked_language_encoder": (32, 160, 0, 2, 1, 8, 64, 8, 256, 512, 20972032),
    "no_cfg": "PIO_E_SHAPE",
    "no_K": "PIO_E_ARG",
    "no_VT": "PIO_E_ARG",
    "K_lo_alone": "PIO_E_ARG",
    "pair_128": "PIO_E_SHAPE",
    "pair_bf16": "PIO_E_SHAPE",
    "no_keys": "PIO_E_SHAPE",
    "dkp_not_padded": "PIO_E_SHAPE",
    "misaligned_ldq": "PIO_E_ALIGN",
    "misaligned_ldk": "PIO_E_ALIGN",
    "misaligned_ldvt": "PIO_E_ALIGN",
    "misaligned_ldo": "PIO_E_ALIGN",
    "misaligned_sQb": "PIO_E_ALIGN",
    "misaligned_sKb": "PIO_E_ALIGN",
    "misaligned_sVb": "PIO_E_ALIGN",
    "misaligned_sOb": "PIO_E_ALIGN",
    "misaligned_Q_ptr": "PIO_E_ALIGN",
    "misaligned_O_ptr": "PIO_E_ALIGN",
    "ldvt_below_8": "PIO_E_SHAPE",
    "ldk_offset_limit": "PIO_E_SHAPE",
    "ldvt_offset_limit": "PIO_E_SHAPE",
    "mask_without_scratch": "PIO_E_WORKSPACE",
    "split_without_scratch": "PIO_E_WORKSPACE",
    "ldvt_not_whole_tiles": "PIO_E_ALIGN",
    "grid_overflow": "PIO_E_SHAPE",
    "no_scratch_before_ldvt_tiles": "PIO_E_WORKSPACE",
    "pair_128_before_misaligned": "PIO_E_SHAPE",
    "ldk_limit_before_no_scratch": "PIO_E_SHAPE",
}

# xtall_launch_plan: nqt, nka, npass, grid -- or the refusal.  Order in xtall_launch: shape / pair operands, operands
# present, extents, alignment, ldvt and the 32-bit offset limits, scratch, grid.
TPLAN = {
    "one_pass": (2, 2, 1, 8),
    "imagenet_decoder_four_passes": (8, 32, 4, 64),
    "too_many_keys": "PIO_E_SHAPE",
    "pair": "PIO_E_SHAPE",
    "no_O": "PIO_E_ARG",
    "no_VT": "PIO_E_ARG",
    "no_queries": "PIO_E_SHAPE",
    "misaligned_ldq": "PIO_E_ALIGN",
    "misaligned_ldk": "PIO_E_ALIGN",
    "misaligned_ldvt": "PIO_E_ALIGN",
    "misaligned_ldo": "PIO_E_ALIGN",
    "misaligned_sQb": "PIO_E_ALIGN",
    "misaligned_sKb": "PIO_E_ALIGN",
    "misaligned_sVb": "PIO_E_ALIGN",
    "misaligned_sOb": "PIO_E_ALIGN",
    "misaligned_Q_ptr": "PIO_E_ALIGN",
    "misaligned_O_ptr": "PIO_E_ALIGN",
    "ldvt_below_64": "PIO_E_SHAPE",
    "ldk_offset_limit": "PIO_E_SHAPE",
    "ldq_offset_limit": "PIO_E_SHAPE",
    "ldvt_offset_limit": "PIO_E_SHAPE",
    "mask_without_scratch": "PIO_E_WORKSPACE",
    "grid_overflow": "PIO_E_SHAPE",
    "Q_lo_alone_is_a_shape": "PIO_E_SHAPE",
    "ldvt_below_64_before_no_scratch": "PIO_E_SHAPE",
    "no_O_before_no_queries": "PIO_E_ARG",
}


def _run_driver():
    inc = os.path.join(ROOT, "include")
    csrc = os.path.join(ROOT, "perceiverio_pytorch_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "route.cpp")
        open(src, "w").write(DRIVER)
        exe = os.path.join(d, "route")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", inc, "-I", csrc, src, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    got = {"route": {}, "splits": {}, "flash": {}, "fplan": {}, "xplan": {}, "tplan": {}}
    for line in filter(None, out):
        f = line.split()
        vals = tuple(int(x) if x.isdigit() else x for x in f[2:])
        got[f[0]][f[1]] = vals[0] if len(vals) == 1 else vals
    return got


GOT = None


def _got():
    global GOT
    if GOT is None:
        GOT = _run_driver()
    return GOT


def test_attention_routing_table():
    assert _got()["route"] == ROUTES


def test_plan_and_run_agree():
    """The plan promises a fused core -- no score buffers under `lean` -- exactly when attn_route returns one for the call
    without masks / bias / probabilities, and carves the xpart bytes the run reports."""
    for name, r in _got()["route"].items():
        if isinstance(r, str):
            continue
        xpart, plan_fused, plan_xpart, plain_fused = r[5:9]
        assert plan_fused == plain_fused, name
        assert plan_xpart == xpart, name


def test_key_splits_and_partials():
    assert _got()["splits"] == SPLITS


def test_flash_route_table():
    assert _got()["flash"] == FLASH


def test_flash_launch_plans():
    assert _got()["fplan"] == FPLAN


def test_xattn_launch_plans():
    assert _got()["xplan"] == XPLAN


def test_xtall_launch_plans():
    assert _got()["tplan"] == TPLAN


def test_header_is_host_only():
    """No HIP include, no environment read, no state: the header compiles with a plain C++ compiler (above) and names none."""
    src = open(os.path.join(ROOT, "perceiverio_pytorch_amd", "csrc", "pio_attn_route.h")).read()
    assert "hip_runtime" not in src and "getenv" not in src and "static " not in src
