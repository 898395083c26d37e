// Internal declarations shared by the HIP translation units of libpio_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/pio_hip.h"
#include "pio_attn_route.h"
#include "pio_block_route.h"

namespace pio {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Operand-dtype traits: the 16-bit type fed to MFMA.
template <int DT> struct Op;
template <> struct Op<PIO_DT_F16> {
    typedef _Float16 T;
    typedef f16x8 V8;
    typedef f16x4 V4;
    static __device__ __forceinline__ T from_f32(float x) { return (T)x; }
    static __device__ __forceinline__ float to_f32(T x) { return (float)x; }
    static __device__ __forceinline__ f32x4 mfma16(V8 a, V8 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x16 mfma32(V8 a, V8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
};
template <> struct Op<PIO_DT_BF16> {
    typedef __bf16 T;
    typedef bf16x8 V8;
    typedef bf16x4 V4;
    static __device__ __forceinline__ T from_f32(float x) { return (T)x; }  // v_cvt_pk_bf16_f32 (RNE, NaN kept)
    static __device__ __forceinline__ float to_f32(T x) { return (float)x; }
    static __device__ __forceinline__ f32x4 mfma16(V8 a, V8 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x16 mfma32(V8 a, V8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
};

static inline int launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? PIO_OK : PIO_E_LAUNCH;
}

// ---- optional per-launch timing for bench.py (pio_prof_begin / pio_prof_end); off by default ----------
enum {
    PROF_GEMM_LINEAR = 0,  // kernel gemm_nt_256 (large flat GEMMs that do not qualify for the streaming kernel)
    PROF_GEMM_ATTN = 1,    // kernel gemm_nt_128<.,1> (batched products)
    PROF_LAYERNORM = 2,
    PROF_SOFTMAX = 3,
    PROF_PACK = 4,
    PROF_FLASH = 5,
    PROF_GEMM_SMALL = 6,   // kernel gemm_nt_128<.,0> (flat problems too small / ragged for the 256 tile)
    PROF_GEMM_STREAM = 7,  // kernel gemm_nt_stream (persistent 256x128 tiles: the weight GEMMs of the latent stack)
    PROF_GEMM_WIDE = 8,    // kernel gemm_nt_wide (persistent 256x256 tiles, four waves: the fused q|k|v projection)
    PROF_CLASSES = 9
};
struct ProfScope {
    int idx;
    hipStream_t s;
    ProfScope(int cls, double flops, double bytes, hipStream_t stream);
    ~ProfScope();
};

// CUs a persistent kernel may size its grid for: the device's CU count, or the budget set with pio_set_cu_budget
// (launches on a CU-masked stream that owns only part of the chip)
int cu_budget();
int cu_budget_call(int v);  // per-call (thread-local) budget: v >= 0 sets it (0 = none); returns the previous value

// ---- internal launchers (defined in the .hip files) ---------------------------------------------
int gemm_nt_launch(const pio_gemm_t &g, hipStream_t s);
int gemm_kernel_override(int which);  // 0 auto, 64 / 128 / 256 tile, 1 = streaming, 2 = wide (experiments build: 3 = duo); returns the previous choice
int layernorm_cast_launch(const pio_tensor3_t &x, const pio_layernorm_t *ln, void *y, void *y_lo, int c_pad,
                          int dtype, hipStream_t s);
// LayerNorm over the concatenation [x1 | x2] of two sources (x2 may be one batch-invariant table, B == 1)
int layernorm_cast_cat_launch(const pio_tensor3_t &x1, const pio_tensor3_t &x2, const pio_layernorm_t &ln, void *y,
                              void *y_lo, int c_pad, int dtype, hipStream_t s);
// LayerNorm fold: 16-bit cast of contiguous C-channel rows (C % 256 == 0) + their (sum, sum of squares) per slot of slot_w
// (64 / 128) columns, the form the fold's consumer GEMM reads (first layer of a stack: later layers get both from the
// producing GEMM)
int rowstats_cast_launch(const float *x, int64_t rows, int C, int slot_w, void *y16, void *y16_lo, float *part, int dtype,
                         hipStream_t s);
// VT[b][c][t] = X[b][t][c] (16-bit; columns t in [T, tkv) zero): the values of a K / V-folded cross-attend
int transpose16_launch(const void *x, int64_t ldx, int B, int T, int C, void *vt, int64_t tkv, hipStream_t s);
int softmax_rows_launch(const float *S, int64_t lds, void *P, void *P_lo, int64_t ldp, int B, int H, int Tq, int Tk,
                        float scale, const uint8_t *kv_mask, const uint8_t *q_mask, const uint8_t *full_mask,
                        const float *bias, int dtype, float *probs_out, hipStream_t s);
// The fused attention cores on one operand bundle (AttnOperands; shape tables and routing: pio_attn_route.h).
// v_rowmajor: t.VT points at V [B][Tk][.. h*dvp ..] (row stride ldvt) instead of V^T [B][H*dvp][Tk].
int flash_attention_launch(int dtype, int dkp, int dvp, int dk_logical, const AttnOperands &t, int B, int H, int Tq, int Tk,
                           bool v_rowmajor, hipStream_t s);
// scratch: xattn_partial_bytes / xtall_scratch_bytes of the launch (key bits of a masked launch, split partials)
int xattn_launch(int dtype, int dkp, int dvp, int dk_logical, const AttnOperands &t, int B, int H, int Tq, int Tk,
                 const uint8_t *kv_mask, const uint8_t *q_mask, void *scratch, hipStream_t s);
int xtall_launch(int dtype, int dkp, int dvp, int dk_logical, const AttnOperands &t, int B, int H, int Tq, int Tk,
                 const uint8_t *kv_mask, const uint8_t *q_mask, void *scratch, hipStream_t s);
// Logit probe (pio_qkprobe.hip; tooling, off by default): max |q_i . k_j| / sqrt(dk) over the attendable positions of
// one attention call, max-merged into *absmax.  logit_probe_record: what attention_core calls while the probe is active
// (record n++ of pio_logit_probe_begin's buffer).
int qk_absmax_launch(int dtype, int dkp, int dk, const void *Q, const void *K, int B, int H, int Tq, int Tk, int64_t ldq,
                     int64_t ldk, int64_t sQb, int64_t sKb, const uint8_t *kv_mask, const uint8_t *q_mask,
                     const uint8_t *full_mask, float *absmax, hipStream_t s);
bool logit_probe_active();
int logit_probe_record(int dtype, int dkp, int dk, const AttnOperands &t, int B, int H, int Tq, int Tk,
                       const uint8_t *kv_mask, const uint8_t *q_mask, const uint8_t *full_mask, hipStream_t s);
int logit_probe_begin(float *records, int max_records);
int logit_probe_end();
// Range probe (pio_rangeprobe.hip; tooling, off by default): max |x| of one 16-bit buffer, max-merged into *absmax.
// range_probe_record: what the block entry points call behind every producer of a 16-bit activation buffer while the probe
// is active (record n++ of pio_range_probe_begin's buffer, labelled with the current part and `kind`, a PIO_RK_*).
// range_probe_mark sets the part (PIO_RP_*) of the records that follow and returns the previous one.
int absmax16_launch(int dtype, const void *x, int64_t rows, int64_t cols, int64_t ld, int64_t batch, int64_t stride_b,
                    float *absmax, hipStream_t s);
bool range_probe_active();
int range_probe_record(int kind, int dtype, const void *x, int64_t rows, int64_t cols, int64_t ld, int64_t batch,
                       int64_t stride_b, hipStream_t s);
int range_probe_begin(float *records, int max_records);
int range_probe_mark(int part);
int range_probe_end(int32_t *parts, int32_t *kinds, int cap);
// eval BatchNorm -> ReLU -> 3x3/2 SAME max-pool -> channels-last tokens (tail of Conv2DDownsample)
int bn_relu_pool_nhwc_launch(const float *x, const float *scale, const float *shift, float *y, int B, int C, int H, int W,
                             int pad_top, int pad_left, hipStream_t s);
// flow front end: 3x3 zero-padded patches of a frame pair + the 1x1 projection behind them (w == NULL: the raw patches)
int flow_patch_tokens_launch(const float *f0, const float *f1, int64_t sn0, int64_t sc0, int64_t sy0, int64_t sn1,
                             int64_t sc1, int64_t sy1, const float *w, const float *bias, float *y, int64_t ldy, int N,
                             int C, int H, int W, int out, hipStream_t s);
// 1x1-conv classifier front end: a stride-s 1x1 convolution of an image batch written as channels-last token rows
int conv1x1_tokens_launch(const float *x, int64_t sb, int64_t sc, int64_t sy, int64_t sx, const float *w, int64_t ldw,
                          const float *bias, float *y, int64_t ldy, int64_t sYb, int B, int C, int H, int W, int s, int N,
                          hipStream_t st);
// multimodal front end: features | position table | padding embedding (| mask token) of up to 8 row segments in one launch
int assemble_tokens_launch(const pio_token_segment_t *segs, int nseg, float *y, int64_t ldy, int64_t sYb, int B, int Mtot,
                           int Cc, hipStream_t s);
// language front end: table[ids[b, t]] + pos[t] (and optionally table[ids[b, t]] alone); NaN rows + a flag for bad ids
int embed_tokens_launch(const void *ids, int id_bytes, int64_t ids_sb, const float *table, int64_t ldt, int V,
                        const float *pos, int64_t ldp, float *y, int64_t y_sb, int64_t ldy, float *tokens, int64_t tok_sb,
                        int64_t ldtok, int32_t *bad_ids, int B, int T, int C, hipStream_t s);
// tiled flow inference: ramp-weighted sum of all tile flows over the summed ramps, in tile order
int flow_blend_tiles_launch(const pio_flow_blend_t *p, float *out, int64_t on, int64_t oc, int64_t oy, hipStream_t s);
// flow visualisation: the Middlebury colour wheel of a batch of flow fields, one maximum radius per image (two launches)
int flow_to_image_launch(const float *flow, int64_t sn, int64_t sy, int64_t sx, int64_t sc, int b, int h, int w,
                         float clip_flow, int has_clip, int bgr, uint8_t *out, uint32_t *rad_max, hipStream_t s);
// media samples: fp32 [n, h, w, C] read through strides -> clipped uint8 (optionally channel-reversed) or saturated int16
int finish_media_launch(const float *x, int64_t sn, int64_t sy, int64_t sx, int64_t sc, int n, int h, int w, int C, int kind,
                        int reverse, void *y, hipStream_t s);
// input images: crop, bilinear resize (antialiased or not), channel reversal and (v - mean) / std of up to 32 sources
int prepare_images_launch(const pio_image_src_t *srcs, int nsrc, int C, int oh, int ow, int antialias, int reverse,
                          const float *mean, const float *std, float *out, int64_t out_sb, hipStream_t s);
// decoder queries: Fourier features of index points | learned table, each with its padding embedding, up to 4 row segments
int build_queries_launch(const pio_query_segment_t *segs, int nseg, float *y, int64_t ldy, int Qtot, int Cq, hipStream_t s);
// output heads: up to 4 row segments of the decoder output, each through its own narrow fp32 linear head, written in place
int project_heads_launch(const pio_head_segment_t *segs, int nseg, const float *x, int64_t x_sb, int64_t ldx, int B, int Q,
                         int K, hipStream_t s);
// vocabulary head: fp32 logits of decoder rows against a [V <= 1024, K] embedding, their log-sum-exp and top-k (or the
// selection alone on given logits: x == w == NULL)
int vocab_topk_launch(const float *x, int64_t x_sb, int64_t ldx, const float *w, int64_t ldw, const float *bias, int B, int Q,
                      int V, int K, int k, int32_t *ids, float *logprob, float *lse, float *logits, int64_t ldl,
                      hipStream_t s);
int pack_linear_launch(const float *w, const float *bias, int out, int in, int64_t ldw, int row_heads,
                       int col_heads, void *dst_hi, void *dst_lo, float *dst_bias, int dst_row0, int k_pad,
                       int dtype, hipStream_t s);

}  // namespace pio
