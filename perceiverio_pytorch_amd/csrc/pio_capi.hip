// extern "C" surface for the library/device queries and the primitive kernels (include/pio_hip.h).
#include "pio_internal.h"

#include <string.h>

#include <vector>

using namespace pio;

// ---------------------------------------------------------------------------------------------------------
// per-launch timing (bench only).  One global recorder: NOT thread-safe, never enabled on the product path.
// ---------------------------------------------------------------------------------------------------------
namespace {
struct ProfRec {
    int cls;
    double flops, bytes;
};
struct Prof {
    bool on = false;
    std::vector<hipEvent_t> ev;  // 2 per record
    std::vector<ProfRec> rec;
    size_t cap = 0;
} g_prof;
}  // namespace

namespace pio {
ProfScope::ProfScope(int cls, double flops, double bytes, hipStream_t stream) : idx(-1), s(stream) {
    if (!g_prof.on || g_prof.rec.size() >= g_prof.cap) return;
    idx = (int)g_prof.rec.size();
    g_prof.rec.push_back({cls, flops, bytes});
    (void)hipEventRecord(g_prof.ev[2 * idx], s);
}
ProfScope::~ProfScope() {
    if (idx >= 0) (void)hipEventRecord(g_prof.ev[2 * idx + 1], s);
}

// CU budget of the persistent kernels' grids (pio_set_cu_budget): 0 = every CU of the device
static int g_cu_budget = 0;
// ... and the per-call value (pio_call_opts_t.cu_budget), thread-local for the duration of a *_opts call: it wins over
// the process-wide one.  cu_budget_call(v >= 0) sets it, any call returns the previous value.
static thread_local int tl_cu_budget = 0;
int cu_budget_call(int v) {
    const int prev = tl_cu_budget;
    if (v >= 0) tl_cu_budget = v;
    return prev;
}
int cu_budget() {
    static const int n_cu = [] {
        int dev = 0, n = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        return n > 0 ? n : 256;
    }();
    const int want = tl_cu_budget > 0 ? tl_cu_budget : g_cu_budget;
    return (want > 0 && want < n_cu) ? want : n_cu;
}
}  // namespace pio

extern "C" {

int pio_set_cu_budget(int32_t n_cu) {
    const int prev = g_cu_budget;
    g_cu_budget = n_cu > 0 ? n_cu : 0;
    return prev;
}

int pio_prof_begin(int32_t max_records) {
    if (max_records <= 0) return PIO_E_ARG;
    while (g_prof.ev.size() < (size_t)2 * max_records) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return PIO_E_LAUNCH;
        g_prof.ev.push_back(e);
    }
    g_prof.cap = (size_t)max_records;
    g_prof.rec.clear();
    g_prof.on = true;
    return PIO_OK;
}

int pio_prof_end(double *ms, double *flops, double *bytes, int64_t *launches) {
    g_prof.on = false;
    for (int c = 0; c < PROF_CLASSES; ++c) {
        if (ms) ms[c] = 0;
        if (flops) flops[c] = 0;
        if (bytes) bytes[c] = 0;
        if (launches) launches[c] = 0;
    }
    for (size_t i = 0; i < g_prof.rec.size(); ++i) {
        if (hipEventSynchronize(g_prof.ev[2 * i + 1]) != hipSuccess) return PIO_E_LAUNCH;
        float t = 0.f;
        if (hipEventElapsedTime(&t, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]) != hipSuccess) return PIO_E_LAUNCH;
        const ProfRec &r = g_prof.rec[i];
        if (ms) ms[r.cls] += t;
        if (flops) flops[r.cls] += r.flops;
        if (bytes) bytes[r.cls] += r.bytes;
        if (launches) launches[r.cls] += 1;
    }
    const int n = (int)g_prof.rec.size();
    g_prof.rec.clear();
    return n;
}

int pio_logit_probe_begin(float *records, int32_t max_records) { return logit_probe_begin(records, max_records); }

int pio_logit_probe_end(void) { return logit_probe_end(); }

int pio_qk_logit_absmax(int32_t dtype, int32_t dkp, int32_t dk, const void *Q, const void *K, int32_t B, int32_t H,
                        int32_t Tq, int32_t Tk, int64_t ldq, int64_t ldk, int64_t sQb, int64_t sKb, const uint8_t *kv_mask,
                        const uint8_t *q_mask, const uint8_t *full_mask, float *absmax, void *stream) {
    return qk_absmax_launch(dtype, dkp, dk, Q, K, B, H, Tq, Tk, ldq, ldk, sQb, sKb, kv_mask, q_mask, full_mask, absmax,
                            (hipStream_t)stream);
}

int pio_absmax16(int32_t dtype, const void *x, int64_t rows, int32_t cols, int64_t ld, int32_t batch, int64_t stride_b,
                 float *absmax, void *stream) {
    return absmax16_launch(dtype, x, rows, cols, ld, batch, stride_b, absmax, (hipStream_t)stream);
}

int pio_range_probe_begin(float *records, int32_t max_records) { return range_probe_begin(records, max_records); }

int pio_range_probe_mark(int32_t part) {
    if (part < PIO_RP_ATTENTION || part > PIO_RP_DECODER) return PIO_E_ARG;
    range_probe_mark(part);
    return PIO_OK;
}

int pio_range_probe_end(int32_t *parts, int32_t *kinds, int32_t cap) { return range_probe_end(parts, kinds, cap); }

int pio_version(void) { return PIO_VERSION; }

int pio_arch_ok(void) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return PIO_E_LAUNCH;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return PIO_E_LAUNCH;
    return strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
}

const char *pio_error_string(int code) {
    switch (code) {
        case PIO_OK: return "ok";
        case PIO_E_SHAPE: return "unsupported or inconsistent shape";
        case PIO_E_ALIGN: return "pointer/stride alignment";
        case PIO_E_ARCH: return "device is not gfx950";
        case PIO_E_WORKSPACE: return "workspace too small";
        case PIO_E_LAUNCH: return "HIP launch failed";
        case PIO_E_ARG: return "invalid argument";
        case PIO_E_RANGE: return "values outside the range of the 16-bit operand dtype";
        default: return "unknown error";
    }
}

int32_t pio_pad8(int32_t c) { return pad8(c); }
int32_t pio_padc(int32_t c) { return padc(c); }

int pio_gemm_kernel_override(int which) { return gemm_kernel_override(which); }

size_t pio_packed_weight_bytes(int32_t out, int32_t in, int32_t row_heads, int32_t col_heads) {
    if (out <= 0 || in <= 0 || row_heads <= 0 || col_heads <= 0 || out % row_heads || in % col_heads) return 0;
    return (size_t)row_heads * pad8(out / row_heads) * (size_t)col_heads * pad8(in / col_heads) * 2;
}

int pio_pack_linear(const float *w, const float *bias, int32_t out, int32_t in, int64_t ldw, int32_t row_heads,
                    int32_t col_heads, void *dst_hi, void *dst_lo, float *dst_bias, int32_t dst_row0, int32_t k_pad,
                    int32_t dtype, void *stream) {
    return pack_linear_launch(w, bias, out, in, ldw, row_heads, col_heads, dst_hi, dst_lo, dst_bias, dst_row0, k_pad,
                              dtype, (hipStream_t)stream);
}

int pio_layernorm_cast(const pio_tensor3_t *x, const pio_layernorm_t *ln, void *y, void *y_lo, int32_t c_pad,
                       int32_t dtype, void *stream) {
    if (!x) return PIO_E_ARG;
    return layernorm_cast_launch(*x, ln, y, y_lo, c_pad, dtype, (hipStream_t)stream);
}

int pio_layernorm_cast_cat(const pio_tensor3_t *x1, const pio_tensor3_t *x2, const pio_layernorm_t *ln, void *y,
                           void *y_lo, int32_t c_pad, int32_t dtype, void *stream) {
    if (!x1 || !x2 || !ln) return PIO_E_ARG;
    return layernorm_cast_cat_launch(*x1, *x2, *ln, y, y_lo, c_pad, dtype, (hipStream_t)stream);
}

int pio_rowstats_cast(const float *x, int64_t rows, int32_t C, int32_t slot_w, void *y16, void *y16_lo, float *part,
                      int32_t dtype, void *stream) {
    return rowstats_cast_launch(x, rows, C, slot_w, y16, y16_lo, part, dtype, (hipStream_t)stream);
}

int pio_transpose16(const void *x, int64_t ldx, int32_t B, int32_t T, int32_t C, void *vt, int64_t tkv, void *stream) {
    return transpose16_launch(x, ldx, B, T, C, vt, tkv, (hipStream_t)stream);
}

int pio_bn_relu_maxpool_tokens(const float *x, const float *scale, const float *shift, float *y, int32_t B, int32_t C,
                               int32_t H, int32_t W, int32_t pad_top, int32_t pad_left, void *stream) {
    return bn_relu_pool_nhwc_launch(x, scale, shift, y, B, C, H, W, pad_top, pad_left, (hipStream_t)stream);
}

int pio_flow_patch_tokens(const float *frame0, const float *frame1, int64_t sn0, int64_t sc0, int64_t sy0, int64_t sn1,
                          int64_t sc1, int64_t sy1, const float *w, const float *bias, float *y, int64_t ldy, int32_t N,
                          int32_t C, int32_t H, int32_t W, int32_t out, void *stream) {
    return flow_patch_tokens_launch(frame0, frame1, sn0, sc0, sy0, sn1, sc1, sy1, w, bias, y, ldy, N, C, H, W, out,
                                    (hipStream_t)stream);
}

int pio_conv1x1_tokens(const float *x, int64_t sb, int64_t sc, int64_t sy, int64_t sx, const float *w, int64_t ldw,
                       const float *bias, float *y, int64_t ldy, int64_t sYb, int32_t B, int32_t C, int32_t H, int32_t W,
                       int32_t s, int32_t N, void *stream) {
    return conv1x1_tokens_launch(x, sb, sc, sy, sx, w, ldw, bias, y, ldy, sYb, B, C, H, W, s, N, (hipStream_t)stream);
}

int pio_assemble_tokens(const pio_token_segment_t *segs, int32_t nseg, float *y, int64_t ldy, int64_t sYb, int32_t B,
                        int32_t Mtot, int32_t Cc, void *stream) {
    return assemble_tokens_launch(segs, nseg, y, ldy, sYb, B, Mtot, Cc, (hipStream_t)stream);
}

int pio_build_queries(const pio_query_segment_t *segs, int32_t nseg, float *y, int64_t ldy, int32_t Qtot, int32_t Cq,
                      void *stream) {
    return build_queries_launch(segs, nseg, y, ldy, Qtot, Cq, (hipStream_t)stream);
}

int pio_project_heads(const pio_head_segment_t *segs, int32_t nseg, const float *x, int64_t x_sb, int64_t ldx,
                      int32_t B, int32_t Q, int32_t K, void *stream) {
    return project_heads_launch(segs, nseg, x, x_sb, ldx, B, Q, K, (hipStream_t)stream);
}

int pio_vocab_topk(const float *x, int64_t x_sb, int64_t ldx, const float *w, int64_t ldw, const float *bias, int32_t B,
                   int32_t Q, int32_t V, int32_t K, int32_t k, int32_t *ids, float *logprob, float *lse, float *logits,
                   int64_t ldl, void *stream) {
    return vocab_topk_launch(x, x_sb, ldx, w, ldw, bias, B, Q, V, K, k, ids, logprob, lse, logits, ldl, (hipStream_t)stream);
}

int pio_embed_tokens(const void *ids, int32_t id_bytes, int64_t ids_sb, const float *table, int64_t ldt, int32_t V,
                     const float *pos, int64_t ldp, float *y, int64_t y_sb, int64_t ldy, float *tokens, int64_t tok_sb,
                     int64_t ldtok, int32_t *bad_ids, int32_t B, int32_t T, int32_t C, void *stream) {
    return embed_tokens_launch(ids, id_bytes, ids_sb, table, ldt, V, pos, ldp, y, y_sb, ldy, tokens, tok_sb, ldtok, bad_ids,
                               B, T, C, (hipStream_t)stream);
}

int pio_flow_blend_tiles(const pio_flow_blend_t *p, float *out, int64_t on, int64_t oc, int64_t oy, void *stream) {
    return flow_blend_tiles_launch(p, out, on, oc, oy, (hipStream_t)stream);
}

int pio_flow_to_image(const float *flow, int64_t sn, int64_t sy, int64_t sx, int64_t sc, int32_t b, int32_t h, int32_t w,
                      float clip_flow, int32_t has_clip, int32_t bgr, uint8_t *out, uint32_t *rad_max, void *stream) {
    return flow_to_image_launch(flow, sn, sy, sx, sc, b, h, w, clip_flow, has_clip, bgr, out, rad_max, (hipStream_t)stream);
}

int pio_finish_media(const float *x, int64_t sn, int64_t sy, int64_t sx, int64_t sc, int32_t n, int32_t h, int32_t w,
                     int32_t C, int32_t kind, int32_t reverse, void *y, void *stream) {
    return finish_media_launch(x, sn, sy, sx, sc, n, h, w, C, kind, reverse, y, (hipStream_t)stream);
}

int pio_prepare_images(const pio_image_src_t *srcs, int32_t nsrc, int32_t C, int32_t oh, int32_t ow, int32_t antialias,
                       int32_t reverse_channels, const float *mean, const float *std, float *out, int64_t out_sb,
                       void *stream) {
    return prepare_images_launch(srcs, nsrc, C, oh, ow, antialias, reverse_channels, mean, std, out, out_sb,
                                 (hipStream_t)stream);
}

int pio_gemm_nt(const pio_gemm_t *g, void *stream) {
    if (!g) return PIO_E_ARG;
    return gemm_nt_launch(*g, (hipStream_t)stream);
}

int pio_softmax_rows(const float *S, int64_t lds, void *P, void *P_lo, int64_t ldp, int32_t B, int32_t H, int32_t Tq,
                     int32_t Tk, float scale, const uint8_t *kv_mask, const uint8_t *q_mask, const uint8_t *full_mask,
                     const float *bias, int32_t dtype, void *stream) {
    return softmax_rows_launch(S, lds, P, P_lo, ldp, B, H, Tq, Tk, scale, kv_mask, q_mask, full_mask, bias, dtype, nullptr,
                               (hipStream_t)stream);
}

int pio_flash_attention(int32_t dtype, int32_t dkp, int32_t dvp, int32_t dk, const void *Q, const void *K, const void *V,
                        void *O, int32_t B, int32_t H, int32_t Tq, int32_t Tk, int64_t ldq, int64_t ldk, int64_t ldv,
                        int64_t ldo, int64_t sQb, int64_t sKb, int64_t sVb, int64_t sOb, int32_t v_rowmajor, void *stream) {
    if (dtype != PIO_DT_F16 && dtype != PIO_DT_BF16) return PIO_E_ARG;
    const AttnOperands t = {Q, nullptr, K, nullptr, V, O, nullptr, ldq, ldk, ldv, ldo, sQb, sKb, sVb, sOb};
    return flash_attention_launch(dtype, dkp, dvp, dk, t, B, H, Tq, Tk, v_rowmajor != 0, (hipStream_t)stream);
}

size_t pio_flash_attention_pair_workspace_bytes(int32_t dkp, int32_t dvp, int32_t B, int32_t H, int32_t Tq, int32_t Tk) {
    // enough for whichever core the caller names: a shape both cross-attention kernels cover gets the larger figure
    const size_t tiled = xattn_supported(dkp, dvp) ? xattn_partial_bytes(dkp, dvp, B, H, Tq, Tk) : 0;
    const size_t tall = xtall_supported(dkp, dvp, Tk) ? xtall_scratch_bytes(B) : 0;
    return tiled > tall ? tiled : tall;
}

int pio_flash_attention_pair(int32_t dtype, int32_t dkp, int32_t dvp, int32_t dk, const void *Q, const void *Q_lo,
                             const void *K, const void *K_lo, const void *V, void *O, void *O_lo, int32_t B, int32_t H,
                             int32_t Tq, int32_t Tk, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t sQb,
                             int64_t sKb, int64_t sVb, int64_t sOb, int32_t v_rowmajor, const uint8_t *kv_mask,
                             const uint8_t *q_mask, int32_t core, void *workspace, size_t workspace_bytes, void *stream) {
    if (dtype != PIO_DT_F16 && dtype != PIO_DT_BF16) return PIO_E_ARG;
    const AttnOperands t = {Q, Q_lo, K, K_lo, V, O, O_lo, ldq, ldk, ldv, ldo, sQb, sKb, sVb, sOb};
    if (core < 0 || core > 3 || !attn_lo_halves_paired(t)) return PIO_E_ARG;
    const bool masked = kv_mask || q_mask;
    // core 0: what attention_core's route takes for the shape (fused_core, pio_attn_route.h), short of the tall-head kernel
    if (core == 1 || (core == 0 && fused_core(dkp, dvp, Tk, masked, true) == AttnCore::FLASH)) {
        if (masked) return PIO_E_ARG;  // (the self-attention kernel takes no mask)
        if (!flash_o_lo_allowed(t)) return PIO_E_ARG;
        return flash_attention_launch(dtype, dkp, dvp, dk, t, B, H, Tq, Tk, v_rowmajor != 0, (hipStream_t)stream);
    }
    if (v_rowmajor) return PIO_E_ARG;  // (the cross-attention kernels read V^T)
    if (core == 3) {                   // the tall-head kernel: no pair operands, key-bit words as its only scratch
        if (!xtall_takes(dkp, dvp, Tk, t)) return PIO_E_SHAPE;
        if (xtall_scratch_bytes(B) > workspace_bytes) return PIO_E_WORKSPACE;
        return xtall_launch(dtype, dkp, dvp, dk, t, B, H, Tq, Tk, kv_mask, q_mask, workspace, (hipStream_t)stream);
    }
    if (!xattn_supported(dkp, dvp)) return PIO_E_SHAPE;
    if (xattn_partial_bytes(dkp, dvp, B, H, Tq, Tk) > workspace_bytes) return PIO_E_WORKSPACE;
    return xattn_launch(dtype, dkp, dvp, dk, t, B, H, Tq, Tk, kv_mask, q_mask, workspace, (hipStream_t)stream);
}

}  // extern "C"
