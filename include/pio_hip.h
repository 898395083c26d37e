/*
 * pio_hip.h -- C-ABI of libpio_hip.so: the MI355X (gfx950) PerceiverIO forward hot path.
 *
 * This is the drop-in boundary for the reference's perceiver_io/transformer_primitives.py and the
 * encoder/decoder drivers of perceiver_io/perceiver.py.  The reference is pure Python and has no
 * FFI of its own; each entry point below names the reference callable
 * (file:line under /root/reference) whose arithmetic it replaces.  INTEGRATION.md shows the ctypes
 * stub a maintainer of the reference would add to bind them.
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures: `stream` is a hipStream_t passed as void*.
 *   - every pointer is a DEVICE pointer owned by the caller; compute calls allocate and free nothing and
 *     keep no state between calls => they are thread-safe per (stream, workspace).  The only process-wide
 *     mutable state is opt-in tooling, none of it thread-safe: the per-launch profiler (pio_prof_*), the logit
 *     probe (pio_logit_probe_*), the range probe (pio_range_probe_*) and the A/B switches pio_ln_fold_enable / pio_gemm_kernel_override / pio_set_cu_budget (set them before
 *     concurrent use).
 *   - scratch memory is caller-provided: query pio_*_workspace_bytes() first.  Its CONTENT on entry is undefined --
 *     stale 16-bit activations, fp32 scores, key-bit words and key-split partials of an earlier, larger call, NaN
 *     patterns included -- and no result depends on it: every pad region a kernel reads is written by its producer
 *     inside the call, or masked by assignment.  The same holds for the caller-owned query cache of
 *     pio_decoder_fwd (pio_decoder_call_t.q16_hi) while q16_valid == 0 (tests/test_workspace_stale_gpu.py runs every block entry point and
 *     route of tests/workspace_stale_cases.py on a zeroed, a 0xFF- and a 0x7B-filled workspace, bit for bit).
 *   - tensors at the boundary are float32, last dimension contiguous; batch / row strides are given
 *     in ELEMENTS (a batch stride of 0 is a broadcast view, e.g. the latent table of
 *     position_encoding.py:117-121).
 *   - masks are uint8, the storage of torch.bool: a mask byte is true iff non-zero (0 = masked out; 1, 2, 0x80, 0xFF
 *     all attend).
 *   - return value: PIO_OK (0) or a negative PIO_E_* code; no exceptions cross the ABI.
 *   - matrix operands inside the library are fp16 (default) or bf16 with fp32 accumulation;
 *     LayerNorm, softmax, bias, GELU and the residual stream are fp32.
 */
#ifndef PIO_HIP_H
#define PIO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PIO_VERSION 101 /* 0.1.1 */

enum {
    PIO_OK = 0,
    PIO_E_SHAPE = -1,     /* unsupported / inconsistent shape                       */
    PIO_E_ALIGN = -2,     /* pointer or stride alignment requirement violated       */
    PIO_E_ARCH = -3,      /* device is not gfx950                                   */
    PIO_E_WORKSPACE = -4, /* workspace too small                                    */
    PIO_E_LAUNCH = -5,    /* HIP launch error (hipGetLastError)                     */
    PIO_E_ARG = -6,       /* NULL / invalid argument                                */
    PIO_E_RANGE = -7      /* values left the range of the 16-bit operand dtype (raised by the host-side guard of the
                             LayerNorm-folded stack, whose residual stream is an fp16 pair: see pio_ln_fold_t)     */
};

/* operand dtype of the MFMA matrices (accumulation is always fp32) */
enum { PIO_DT_F16 = 0, PIO_DT_BF16 = 1 };

/* --- descriptors (host structs holding device pointers) --------------------------------------- */

/* One nn.Linear packed for the kernels: `y = x W^T + b`, W is [out,in] in the reference
 * (transformer_primitives.py:73-75,86 / 201-206).  Packed image: [n_pad][k_pad] operand dtype, K
 * contiguous, zero padded; optional second image w_lo = W - float(w_hi) (two-pass weights). */
typedef struct pio_linear_t {
    const void *w_hi;
    const void *w_lo;  /* NULL => single pass */
    const float *bias; /* [n_pad] zero padded, or NULL */
    int32_t n;         /* padded output features: heads x pio_pad8(head dim); pio_padc(hidden) for MLP.fc1         */
    int32_t k;         /* padded input features: pio_padc(channels); heads x pio_pad8(dv) for Attention.final      */
    int32_t lo_row0;   /* w_lo holds rows [lo_row0, n) only (a stacked q|k|v image whose v part alone is split);
                          0 = every row.  Must be a multiple of 256; honoured by the wide GEMM kernel only.          */
} pio_linear_t;

/* nn.LayerNorm(c) (transformer_primitives.py:270-271, 365-367) */
typedef struct pio_layernorm_t {
    const float *gamma;
    const float *beta;
    int32_t c;
    float eps;
} pio_layernorm_t;

/* Attention (transformer_primitives.py:34-88): proj_q/k/v + final.  Per-head widths are padded to
 * multiples of 8 inside the packed images (dkp, dvp); logical widths are dk, dv. */
typedef struct pio_attention_t {
    pio_linear_t q, k, v, o;
    int32_t heads;
    int32_t dk, dv;   /* logical channels per head for q/k and v  */
    int32_t dkp, dvp; /* padded (multiple of 8)                    */
    int32_t q_in, k_in, v_in, out; /* logical channel counts (k_in == v_in inside Self/CrossAttention) */
    int32_t dtype;     /* PIO_DT_*                                  */
    int32_t act_split; /* 1: activations are carried as hi+lo pairs too (3 MFMA sweeps, ~fp32 products);
                          2: the same for the four projections, but the attention core (Q K^T, softmax, P V) runs
                          single-sweep on the hi halves through the fused kernel wherever one covers the shape (no
                          score matrix) and returns its output as a pair;
                          3: as 2, and Q and K enter the fused core as (hi, lo) pairs: S = Q_hi K_hi + Q_lo K_hi + Q_hi K_lo,
                          fp32 accumulation, inside the kernel (policy "fp16x3fq").  Pair cores exist for fp16 heads with
                          dkp <= 32 and dvp <= 160 (cross-attention kernel; key / query mask vectors, key splits) and
                          (dkp, dvp) in {(32,32), (32,160), (128,128)} (self-attention kernel, un-masked).  Every other
                          shape -- 64-wide heads, 128-wide heads with mask vectors, wide single heads, the tall-head
                          kernel, the K / V-folded path, bf16 -- has no pair core and runs the
                          materialised split-operand path of act_split = 1: the request is never served by a single-
                          operand Q K^T                                                                       */
    pio_linear_t qk;   /* optional (w_hi may be NULL): proj_q and proj_k stacked along the output rows
                          [q rows | k rows], used as ONE GEMM when inputs_q and inputs_k are the same tensor */
    pio_linear_t qkv;  /* optional (w_hi may be NULL): [q rows | k rows | v rows] for self-attention with head widths
                          the fused kernel covers: one GEMM, V consumed row-major by the fused attention kernel */
    /* Optional K / V projection fold of a SINGLE-HEAD cross-attend over many keys (both w_hi non-NULL; SURVEY.md section 7,
     * transformer_primitives.py:93-95,138,163): q (x Wk^T + bk)^T = (q Wk) x^T + const, and P (x Wv^T + bv) Wo^T + bo =
     * (P x) (Wo Wv)^T + (Wo bv + bo) because softmax rows sum to one.  kq = Wk^T packed as a linear [k_in <- qk] without
     * bias (Q' = Q Wk), vo = Wo Wv packed [out <- v_in] with bias Wo bv + bo.  The fused kernel then reads the
     * LayerNorm'd inputs themselves as K and (transposed) as V: the two [keys, C] x [C, C] projection GEMMs vanish.
     * Taken when heads == 1, dk == dv == k_in == v_in, inputs_k is inputs_v, no mask / bias / probabilities, and
     * keys outnumber query rows at least 4 : 1. */
    pio_linear_t kq, vo;
} pio_attention_t;

/* MLP (transformer_primitives.py:183-216) */
typedef struct pio_mlp_t {
    pio_linear_t fc1, fc2;
    int32_t in, hidden, out;
    int32_t dtype;
    int32_t act_split;
} pio_mlp_t;

/* Optional LayerNorm fold of a SelfAttention block (all pointers NULL = not available): the two GEMMs that
 * consume a LayerNorm output take the un-normalised 16-bit activations instead and apply mean / rstd in their
 * epilogue; the GEMMs that produce the LayerNorm input leave the row statistics (pio_gemm_t.X16 / row_part).
 * qkv: [q | k | v] rows packed from W * gamma1 with bias W beta1 + b; fc1: from W1 * gamma2, bias W1 beta2 + b1;
 * *_c[n] = sum_k of the packed 16-bit weights of row n.  Used for 1024-channel blocks under the single-sweep
 * policies when the block has at least 2048 rows and no mask / bias / probabilities are requested. */
typedef struct pio_ln_fold_t {
    pio_linear_t qkv;
    const float *qkv_c;
    pio_linear_t fc1;
    const float *fc1_c;
    /* Range guard of the folded stack (optional device word, zeroed by the caller): inside the fold the residual stream
     * is a 16-bit pair, so an activation beyond the operand range (fp16: 65504) turns into inf / NaN there.  Every GEMM
     * that produces the stream ORs 1 into *range_flag when a row statistic of its result is not finite -- no extra
     * kernel, no host synchronisation; the caller reads the word when it next synchronises anyway and re-runs the call
     * un-folded (PIO_E_RANGE if that does not help).  NULL: not reported. */
    int32_t *range_flag;
} pio_ln_fold_t;

/* SelfAttention (transformer_primitives.py:219-297) */
typedef struct pio_self_attention_t {
    pio_layernorm_t ln1, ln2;
    pio_attention_t attn;
    pio_mlp_t mlp;
    pio_ln_fold_t fold;
} pio_self_attention_t;

/* CrossAttention (transformer_primitives.py:300-406) */
typedef struct pio_cross_attention_t {
    pio_layernorm_t ln_q, ln_kv, ln2;
    pio_attention_t attn;
    pio_mlp_t mlp;
    int32_t use_query_residual;
} pio_cross_attention_t;

/* A float32 activation tensor [B, T, C] at the boundary: element strides, C contiguous. */
typedef struct pio_tensor3_t {
    const float *data;
    int64_t stride_b; /* 0 = broadcast over the batch */
    int64_t stride_t;
    int32_t B, T, C;
} pio_tensor3_t;

/* --- library / device ---------------------------------------------------------------------------- */
int pio_version(void);
/* 1 when the current HIP device is gfx950, 0 otherwise, <0 on error. */
int pio_arch_ok(void);
const char *pio_error_string(int code);

/* --- per-launch timing for benchmarks (NOT thread-safe, off by default) ------------------------ */
/* classes: 0 gemm_nt_256 (flat 256x256 tiles), 1 batched gemm_nt_128 (materialised attention products),
 *          2 layernorm / cast / row statistics, 3 softmax_rows, 4 pack, 5 fused attention (flash_attn),
 *          6 flat gemm_nt_128 (small / ragged problems), 7 gemm_nt_stream (persistent 256x128 tiles: fp32 + residual
 *          projections outside a folded stack), 8 gemm_nt_wide (persistent 256x256 four-wave kernel:
 *          every weight GEMM of the latent self-attend stack -- q|k|v, out, fc1, fc2 -- and the decoder projections) */
#define PIO_PROF_CLASSES 9
/* Start recording a HIP-event pair around every kernel launch (up to max_records launches). */
int pio_prof_begin(int32_t max_records);
/* Stop, wait for the recorded launches and sum per class: device milliseconds, ALGORITHMIC flops
 * (2*M*N*K per product, extra precision sweeps not counted), algorithmic bytes, launch count.
 * Arrays have PIO_PROF_CLASSES entries (any may be NULL).  Returns the number of records or <0. */
int pio_prof_end(double *ms, double *flops, double *bytes, int64_t *launches);

/* --- logit probe: how large are the attention logits? (calibration tooling, NOT thread-safe, off by default) ------ */
/* The fused attention cores round q and k once to the 16-bit operand dtype in front of Q K^T: delta s ~ |s| 2^-11 in the
 * exponent (fp16).  Whether a checkpoint needs the pair-operand policy "fp16x3fq" depends on how large |s| gets; these
 * calls measure it.
 *
 * pio_qk_logit_absmax: *absmax = max(*absmax, max |q_i . k_j| / sqrt(dk)) over all batches, heads, query rows i < Tq and
 * keys j < Tk of one attention call, leaving out rows with q_mask[b][i] == 0, keys with kv_mask[b][j] == 0 and positions
 * with full_mask[b][i][j] == 0 (each mask optional).  Q / K: 16-bit operands in the layout the fused cores read,
 * [B][T][.. h*dkp ..], row pitches ldq / ldk and batch strides sQb / sKb in elements (sQb = 0: batch-invariant queries);
 * both may be columns of one stacked q|k|v buffer.  fp32 accumulation; nothing behind row T - 1 or channel dkp - 1 is read.
 * A non-finite product reports +inf.  `absmax` is ONE device float the caller zeroed (results of several calls max-merge).
 * No score matrix, no workspace.  PIO_E_SHAPE: dkp % 8 != 0, dk outside [1, dkp], a row pitch below H * dkp;
 * PIO_E_ALIGN: pointers not 16-byte / pitches and strides not 8-element aligned; PIO_E_ARG: NULL operand, unknown dtype. */
int pio_qk_logit_absmax(int32_t dtype, int32_t dkp, int32_t dk, const void *Q, const void *K, int32_t B, int32_t H,
                        int32_t Tq, int32_t Tk, int64_t ldq, int64_t ldk, int64_t sQb, int64_t sKb, const uint8_t *kv_mask,
                        const uint8_t *q_mask, const uint8_t *full_mask, float *absmax, void *stream);
/* Process-wide switch (modelled on pio_prof_begin / pio_prof_end): while active, EVERY attention call of the block entry
 * points (pio_attention_fwd ... pio_encoder_fwd / pio_decoder_fwd) runs pio_qk_logit_absmax once, on the call's stream,
 * over the operands its core is about to exponentiate and with the call's masks -- whichever route the call takes (stacked
 * q|k|v buffer; K / V fold: Q Wk against the LayerNorm'd inputs, without the per-row constant q . bk that softmax cancels;
 * pair cores: hi halves; tall-head; materialised) -- and writes records[n++].  The attention bias is not part of the
 * figure.  `records`: caller-zeroed device buffer of max_records floats, alive until pio_logit_probe_end.  Routing, the
 * workspace sizes and every result are unchanged; with the probe inactive nothing extra is launched. */
int pio_logit_probe_begin(float *records, int32_t max_records);
/* Stop; returns the number of attention calls seen since begin (calls past max_records are counted, not recorded; 0 when
 * the probe was not active).  Does not synchronise: the records are complete once the streams used have drained. */
int pio_logit_probe_end(void);

/* --- range probe: do the 16-bit operands fit their dtype? (calibration tooling, NOT thread-safe, off by default) ---- */
/* Every matrix operand inside the library is 16-bit; with fp16 anything beyond 65 504 becomes inf.  Only the LayerNorm-
 * folded stack has a device-side guard (pio_ln_fold_t.range_flag); these calls measure every other 16-bit buffer, so that
 * a caller can tell which part of a model needs a bf16 policy.
 *
 * pio_absmax16: *absmax = max(*absmax, max |float(x[b][r][c])|) over b < batch, r < rows, c < cols.  x: 16-bit operands
 * (PIO_DT_F16 / PIO_DT_BF16), row pitch ld and batch stride stride_b in ELEMENTS; stride_b = 0 means one batch is read.
 * A non-finite element (NaN, +-inf) reports +inf.  `absmax` is ONE device float the caller zeroed (results of several
 * calls max-merge).  Nothing behind column cols - 1 of a row, behind the last row or in front of x is read, whatever the
 * alignment of x (2 bytes suffice) and the pitch.  No workspace.  PIO_E_ARG: NULL pointer, unknown dtype; PIO_E_SHAPE: a
 * negative extent, cols > ld with rows > 1; PIO_E_ALIGN: x not 2-byte / absmax not 4-byte aligned.  Empty extents are
 * PIO_OK and leave *absmax unchanged. */
int pio_absmax16(int32_t dtype, const void *x, int64_t rows, int32_t cols, int64_t ld, int32_t batch, int64_t stride_b,
                 float *absmax, void *stream);
/* What a record of the range probe measured ... */
enum {
    PIO_RK_CAST = 0,   /* LayerNorm+cast or plain-cast output (the two-source form included)                        */
    PIO_RK_Q = 1,      /* projected queries; a stacked q|k or q|k|v GEMM is ONE record over the whole stacked width    */
    PIO_RK_K = 2,      /* projected keys                                                                               */
    PIO_RK_V = 3,      /* projected values (as V^T)                                                                    */
    PIO_RK_ATTN = 4,   /* output of the attention core (the materialised route's P V product as well)                  */
    PIO_RK_HIDDEN = 5, /* fc1 + GELU                                                                                   */
    PIO_RK_STREAM = 6  /* the LayerNorm fold's 16-bit residual stream X16, and a decoder's y16 in front of its final Linear */
};
/* ... and the part of the model it belongs to (pio_range_probe_mark) */
enum { PIO_RP_ATTENTION = 0, PIO_RP_CROSS = 1, PIO_RP_STACK = 2, PIO_RP_DECODER = 3 };
/* Process-wide switch (modelled on pio_logit_probe_begin / _end; the two probes may be active together): while active,
 * EVERY 16-bit activation buffer produced inside the block entry points (pio_attention_fwd, pio_mlp_fwd ...
 * pio_encoder_fwd / pio_decoder_fwd) gets one pio_absmax16 on the call's stream, right behind its producer, into
 * records[n++]; the library keeps (part, kind) of every record on the host.  Hi halves only (a lo residual is below one
 * ulp of its hi half); the probabilities P (at most 1), a projected-query cache that is read but not written, and the
 * transposed copy of the LayerNorm'd inputs a K / V-folded cross-attend makes produce no record.  `records`: caller-zeroed
 * device buffer of max_records floats, alive until pio_range_probe_end.  Routing, the workspace sizes and every result are
 * unchanged; with the probe inactive nothing extra is launched.  Not capturable (host-side state). */
int pio_range_probe_begin(float *records, int32_t max_records);
/* Host-side label of the records that follow: a PIO_RP_* (PIO_E_ARG otherwise); PIO_RP_ATTENTION after begin.  The
 * encoder entry points run the cross-attend and the stack in one call: they mark PIO_RP_STACK behind the cross-attend
 * themselves and restore the caller's part when they return.  Without an active probe the call does nothing. */
int pio_range_probe_mark(int32_t part);
/* Stop; returns the number of records seen since begin (records past max_records are counted, not recorded; 0 when the
 * probe was not active) and fills parts[i] / kinds[i] (HOST arrays of `cap` entries, either may be NULL) for the recorded
 * ones.  Does not synchronise: the figures are complete once the streams used have drained. */
int pio_range_probe_end(int32_t *parts, int32_t *kinds, int32_t cap);

/* --- LayerNorm fold of the SelfAttention blocks (pio_ln_fold_t), for tests and A/B benchmarks ------ */
/* 0: never; 1: where it pays (default; env PIO_LN_FOLD gives the initial value) -- blocks of >= 6144 rows (env
 * PIO_LN_FOLD_MIN_ROWS), below which the un-folded block's smaller GEMM tiles fill the chip better; 2: wherever a
 * block offers it (>= 2048 rows).  Returns the previous setting. */
int pio_ln_fold_enable(int on);

/* --- kernel selection of pio_gemm_nt, for tests and A/B benchmarks ------------------------------- */
/* 0: automatic (default; env PIO_GEMM_TILE gives the initial value), 64: 64x64 tiles of the 128-tile kernel (automatic
 * for problems with fewer than 192 tiles of 128x128: small batches), 128: 128x128 tile, 256: 256x256 tile,
 * 1: persistent 256x128 streaming kernel wherever it is legal, 2: persistent 256x256 four-wave kernel wherever
 * it is legal.  Returns the previous setting.  (Experiment kernels that measured level with these -- a two-workgroups-
 * per-CU fold producer, two more fused self-attention kernels -- are not in this library: tools/experiments, built by `make -C perceiverio_pytorch_amd/csrc experiments`.) */
int pio_gemm_kernel_override(int which);

/* --- running on a part of the chip ----------------------------------------------------------------- */
/* Process-wide (not thread-safe): the number of CUs the persistent GEMM kernels size their grids for; 0 (default) =
 * every CU of the device.  Set it to the population of a stream's CU mask (hipExtStreamCreateWithCUMask, the
 * caller's own) around the calls that launch on that stream.  Returns the previous value. */
int pio_set_cu_budget(int32_t n_cu);

/* --- weight packing (one-off, after load_state_dict) ------------------------------------------ */
/* Round a head dim / key count up to the packing granule (8). */
int32_t pio_pad8(int32_t c);
/* Pitch of a CHANNEL axis in the 16-bit operand arrays (= pio_linear_t.k of the layers that read it, and
 * pio_linear_t.n of MLP.fc1): a multiple of 8; from 512 channels on a multiple of 64 (322 -> 328, 1026 -> 1088). */
int32_t pio_padc(int32_t c);
/* Bytes of ONE packed image (hi or lo) for out x in with per-head padding of rows / columns:
 * rows = row_heads groups of (out/row_heads) padded to 8 each; columns likewise. */
size_t pio_packed_weight_bytes(int32_t out, int32_t in, int32_t row_heads, int32_t col_heads);
/* Pack W [out,in] fp32 (row stride ldw) into dst_hi (and dst_lo when non-NULL) starting at packed
 * row `dst_row0` of an image with `k_pad` columns.  Rows are split in `row_heads` equal groups, each
 * padded to a multiple of 8 rows; columns likewise with `col_heads`.  Padding is written as zeros.
 * bias (may be NULL) is packed the same way into dst_bias[dst_row0...]. */
int pio_pack_linear(const float *w, const float *bias, int32_t out, int32_t in, int64_t ldw,
                    int32_t row_heads, int32_t col_heads, void *dst_hi, void *dst_lo, float *dst_bias,
                    int32_t dst_row0, int32_t k_pad, int32_t dtype, void *stream);

/* --- primitive kernels (exposed for tests and for callers that compose their own blocks) ------- */
/* y[r, 0:c_pad] = operand_dtype( LN(x[r, 0:c]) ) with zero fill of [c, c_pad); ln == NULL => plain
 * cast.  Rows are (b, t) of x.  y_lo (optional) receives the rounding residual v - float(y).
 * Replaces nn.LayerNorm + the implicit cast in front of every GEMM. */
int pio_layernorm_cast(const pio_tensor3_t *x, const pio_layernorm_t *ln, void *y, void *y_lo, int32_t c_pad,
                       int32_t dtype, void *stream);

/* The same LayerNorm over the channel-wise CONCATENATION [x1 | x2] of two arrays, never materialised: x1 [B,T,C1],
 * x2 [B,T,C2] or ONE batch-invariant table [1,T,C2] (x2->B == 1); ln->c == C1 + C2; C1, C2 even, rows 8-byte aligned.
 * Replaces torch.cat([features, position_features], -1) of preprocessors.py:176-200 followed by layer_norm_kv
 * (transformer_primitives.py:379); bit-identical to pio_layernorm_cast of the concatenated array wherever that call runs
 * its 8-byte-lane kernel, whose arithmetic this one restates (a width that is no multiple of 4, or rows that are only
 * 8-byte aligned); a 16-byte-lane kernel sums in another order and may differ in the last bit of the fp32 statistics. */
int pio_layernorm_cast_cat(const pio_tensor3_t *x1, const pio_tensor3_t *x2, const pio_layernorm_t *ln, void *y,
                           void *y_lo, int32_t c_pad, int32_t dtype, void *stream);

/* First pass of a LayerNorm-folded self-attend stack (pio_ln_fold_t), exposed for tests and tools: the fp32 residual stream
 * x [rows, C] (contiguous rows) is cast -- NOT normalised -- to a 16-bit pair and its row statistics are left in the slot
 * form the first consumer GEMM reads (pio_gemm_t.ln_part):
 *   y16[r, c]       = rn(x[r, c]),   y16_lo[r, c] = rn(x[r, c] - float(y16[r, c]))        (y16_lo optional: NULL = not written)
 *   part[r][s][0]   = sum of x[r, c],  part[r][s][1] = sum of x[r, c]^2  over the slot_w columns c in [s slot_w, (s+1) slot_w)
 * with s < C / slot_w: part is [rows][C / slot_w][2] fp32, dense.  slot_w = 128 is the form gemm_nt_wide consumes, 64 the
 * tile kernels'.  The sums are fp32, four columns of a lane first, then a tree over the lanes of the slot; the squares may
 * be fused into the sum.  With integer-valued x every sum is exact (as pio_gemm_t's producer); a non-finite or overflowing
 * element makes the sum of squares of ITS slot non-finite and nothing else (the range guard of the fold reads that).
 *   read:    x rows < rows, columns < C -- nothing behind the last row;
 *   written: rows < rows x columns < C of y16 (and y16_lo), every slot of part of rows < rows; nothing behind them, and
 *            y16_lo == NULL is never touched.  One wave per row, four rows a workgroup: rows need not be a multiple of 4.
 * No workspace, no device allocation, no synchronisation.
 * PIO_E_ARG: NULL x / y16 / part, rows <= 0, unknown dtype; PIO_E_SHAPE: C <= 0 or C % 256 != 0, slot_w neither 64 nor 128;
 * PIO_E_ALIGN: x not 16-byte, y16 / y16_lo / part not 8-byte aligned.  Tested in that order.  A refused call launches
 * nothing. */
int pio_rowstats_cast(const float *x, int64_t rows, int32_t C, int32_t slot_w, void *y16, void *y16_lo, float *part,
                      int32_t dtype, void *stream);

/* The V^T operand of a K / V-folded cross-attend (pio_attention_t.kq / vo), exposed for tests and tools: a batched transpose
 * of a 16-bit array, pure data movement on the bit patterns (NaN payloads and -0 included; no dtype):
 *   vt[b][c][t] = x[b][t][c]   for b < B, c < C, t < T;      vt[b][c][t] = +0   for T <= t < tkv
 * x: [B][T][ldx] (row pitch ldx >= C elements, sample stride T * ldx), vt: [B][C][tkv] dense.  The zero columns are what
 * the cross-attention cores require behind key T - 1 of V^T (pio_flash_attention_pair); tkv may exceed T by whole tiles.
 *   read:    x rows < T of every sample, columns < C -- never the pitch columns [C, ldx), never a row behind T - 1 of the
 *            last sample;
 *   written: all B * C * tkv elements of vt and nothing else.
 * 64 x 64 tiles through LDS, 16-byte accesses on both sides.  No workspace, no device allocation, no synchronisation.
 * PIO_E_ARG: NULL x / vt, B, T or C <= 0; PIO_E_SHAPE: C, ldx or tkv not a multiple of 8, tkv < T, B > 65535;
 * PIO_E_ALIGN: x or vt not 16-byte aligned.  Tested in that order.  A refused call launches nothing. */
int pio_transpose16(const void *x, int64_t ldx, int32_t B, int32_t T, int32_t C, void *vt, int64_t tkv, void *stream);

/* Tail of Conv2DDownsample (processor_utils.py:163-180) in one pass over the conv's output x [B,C,H,W] fp32:
 * y[b, oh*OW + ow, c] = max over the 3x3 stride-2 TF-"SAME" window of relu(x * scale[c] + shift[c]) -- eval-mode
 * BatchNorm folded into (scale, shift) = (gamma / sqrt(var + eps), beta - mean * scale), or (1, 0) without one.
 * OH = ceil(H/2), OW = ceil(W/2); pad_top / pad_left = the leading SAME padding (0 or 1).  y is the channels-last token
 * array [B, OH*OW, C] the encoder consumes. */
int pio_bn_relu_maxpool_tokens(const float *x, const float *scale, const float *shift, float *y, int32_t B, int32_t C,
                               int32_t H, int32_t W, int32_t pad_top, int32_t pad_left, void *stream);

/* Front end of the optical-flow model in one pass over a frame pair: the zero-padded 3x3 neighbourhood of every pixel
 * (processor_utils.py:98-116 patches_for_flow, :59-95 extract_patches: colour fastest inside a patch position), the two
 * frames side by side in the channel axis (processor_utils.py:21-38 space_to_depth with temporal_block_size = 2: frame
 * slowest) and the projection behind them (preprocessors.py:57-258 ImagePreprocessor, conv_after_patching: nn.Linear) --
 * one 3x3 "same" convolution from 2 C planes to `out` channels-last outputs:
 *   y[n, r*W + x, o] = bias[o] + sum_{t<2} sum_{py,px<3} sum_{c<C} w[o, t*9*C + (py*3+px)*C + c]
 *                                                                  * frame_t[n, c, r+py-1, x+px-1]     (0 outside the image)
 * frame0 / frame1: fp32 [N, C, H, W] views with x contiguous and their own element strides (sample, plane, row); positions
 * outside [0,H) x [0,W) are never read.  w [out, 18*C] row-major, bias [out]; y [N, H*W, out] fp32 with row pitch ldy.
 * w == NULL (conv_after_patching = False): y receives the 18*C raw patch channels in the order above, out must equal 18*C
 * and bias is ignored.  fp32 FMA accumulation, one chain bias -> k = 0 .. 18*C-1 per output: the result does not depend on
 * the launch geometry and is bit-identical from run to run.  No workspace, no device allocation, no synchronisation.
 * PIO_E_ARG: NULL frame0 / frame1 / y, or w without bias; PIO_E_SHAPE: N, H, W <= 0, C outside [1, 4], out outside
 * [1, 128], out % 4 != 0 with w (out != 18*C without), ldy < out, N or ceil(H/4) above 65535; PIO_E_ALIGN: ldy % 4 != 0,
 * y not 16-byte aligned, a frame / w / bias pointer not 4-byte aligned.  A refused call launches nothing. */
int pio_flow_patch_tokens(const float *frame0, const float *frame1, int64_t sn0, int64_t sc0, int64_t sy0, int64_t sn1,
                          int64_t sc1, int64_t sy1, const float *w, const float *bias, float *y, int64_t ldy, int32_t N,
                          int32_t C, int32_t H, int32_t W, int32_t out, void *stream);

/* Front end of the 1x1-conv image classifier in one pass: nn.Conv2d(C, N, kernel_size=1, stride=s) of an image batch and the
 * channels-last copy behind it (preprocessors.py:57-258 ImagePreprocessor "conv1x1") as the token rows the encoder reads.
 * With OH = H / s, OW = W / s, m = i*OW + j:
 *   acc = bias ? bias[n] : 0.0f
 *   for c = 0 .. C-1 (ascending): acc = fmaf(w[n*ldw + c], x[b*sb + c*sc + (i*s)*sy + (j*s)*sx], acc)
 *   y[b*sYb + m*ldy + n] = acc
 * x: fp32 [B, C, H, W] through its own four element strides -- any of them: a channels-last view, a batch slice, a stride-0
 * batch, a pointer that is only 4-byte aligned; it is read in place (only pixels (i*s, j*s)), never copied.  w [N, C] fp32 with
 * row pitch ldw, bias [N] fp32 or NULL; y [B, OH*OW, N] fp32 with row pitch ldy and sample stride sYb.  sb and sYb are not read
 * when B == 1.  Only the N channels of each of the B*OH*OW rows are written: [N, ldy) and everything else stays untouched.
 * ONE fp32 FMA chain per output in the order above: the bits of a value depend on its own pixel, weights and bias only -- not
 * on the batch, the grid or the tile it fell into -- and are the same from run to run.  N <= PIO_CONV1X1_MAX_N: a lane keeps
 * the 4*C weights and 4 biases of its four outputs per 256 channels in registers for a whole strip of rows -- 80 of them at
 * C = 4, N = 1024, which with accumulators and addresses stays under the 128 registers per lane of four waves per SIMD.
 * No workspace, no device allocation, no synchronisation.
 * PIO_E_ARG: NULL x / w / y; PIO_E_SHAPE: B, H or W < 1, C outside [1, 4], s outside [1, 8], H % s or W % s != 0, N outside
 * [4, PIO_CONV1X1_MAX_N] or not a multiple of 4, ldw < C, ldy < N, B*OH*OW > 2^31 - 1, for B > 1 sYb < OH*OW*ldy;
 * PIO_E_ALIGN: ldy % 4 != 0, for B > 1 sYb % 4 != 0, y not 16-byte aligned, x / w / bias not 4-byte aligned.  A refused call
 * launches nothing. */
#define PIO_CONV1X1_MAX_N 1024
int pio_conv1x1_tokens(const float *x, int64_t sb, int64_t sc, int64_t sy, int64_t sx, const float *w, int64_t ldw,
                       const float *bias, float *y, int64_t ldy, int64_t sYb, int32_t B, int32_t C, int32_t H, int32_t W,
                       int32_t s, int32_t N, void *stream);

/* One segment of the multimodal front end: rows [row0, row0 + M) of every sample of the token array.  With
 * Cp = Cc - C1 - C2 >= 0 and x the row
 *   x[0       : C1     ] = feature(b, m, :)
 *   x[C1      : C1 + C2] = table[m*ldt : m*ldt + C2]        (one batch-invariant table, row pitch ldt)
 *   x[C1 + C2 : Cc     ] = pad[0 : Cp]
 * the segment writes  y[b, row0 + m, c] = x[c]  (token == NULL: an unmasked modality) or  token[c] + 0.0f * x[c]  (a
 * masked one -- perceiver.py:451-499, mask probability 1: two rounded fp32 operations, a non-finite x[c] gives NaN).
 * kind PIO_TOKENS_ROWS: feature(b, m, j) = feature[b*sb + m*sm + j]  (st, sc, sy, T, C, H, W, s ignored).
 * kind PIO_TOKENS_S2D:  space-to-depth (processor_utils.py:21-38) with spatial block s and temporal block 1 of frames
 *   [B, T, C, H, W] given by their strides (sb, st, sc, sy; x contiguous):  m = (t*(H/s) + y)*(W/s) + x,
 *   j = (dy*s + dx)*C + c,  feature(b, m, j) = feature[b*sb + t*st + c*sc + (y*s + dy)*sy + x*s + dx];
 *   1 <= s <= 8, 1 <= C <= 4, H % s == W % s == 0, C1 == s*s*C, M == T*(H/s)*(W/s)  (sm ignored; a 4-D image: T = 1).
 * A pointer may be NULL where its width (C1, C2, Cp) is 0. */
enum { PIO_TOKENS_ROWS = 0, PIO_TOKENS_S2D = 1 };
#define PIO_MAX_TOKEN_SEGMENTS 8
typedef struct pio_token_segment_t {
    const float *feature;
    const float *table;
    const float *pad;
    const float *token;
    int64_t sb, sm, st, sc, sy, ldt; /* element strides */
    int32_t kind;                    /* PIO_TOKENS_ROWS / PIO_TOKENS_S2D */
    int32_t row0, M;
    int32_t C1, C2;
    int32_t T, C, H, W, s;
} pio_token_segment_t;

/* The multimodal front end (MultimodalPreprocessor, perceiver.py:451-499: per modality features | position encoding |
 * padding embedding, optional mask token, concatenation over the modalities) as ONE launch: nseg (1 .. 8) segments fill
 * their rows of y [B, Mtot, Cc] fp32 (row pitch ldy, sample stride sYb; sYb is not read when B == 1).  Rows no segment
 * covers and the columns [Cc, ldy) are not written.  Only moves and the exact masked expression above: bit-identical to the
 * chain of torch.cat calls it replaces, and from run to run.  Cc % 4 == 0: rows leave as 16-byte vectors (y 16-byte aligned,
 * ldy % 4 == 0, sYb % 4 == 0); otherwise as dwords.  No workspace, no device allocation, no synchronisation.
 * PIO_E_ARG: NULL segs / y, nseg outside [1, 8], an unknown kind, a NULL feature / table / pad pointer whose width is > 0;
 * PIO_E_SHAPE: B, Mtot, Cc, M <= 0, C1 or C2 < 0, C1 + C2 > Cc, ldy < Cc, sYb below one sample's extent, the S2D
 * conditions above, a segment outside [0, Mtot), two segments that overlap; PIO_E_ALIGN: a pointer not 4-byte aligned, on
 * the vector path y not 16-byte aligned or ldy / sYb no multiple of 4.  A refused call launches nothing. */
int pio_assemble_tokens(const pio_token_segment_t *segs, int32_t nseg, float *y, int64_t ldy, int64_t sYb, int32_t B,
                        int32_t Mtot, int32_t Cc, void *stream);

/* One segment of the decoder query array: rows [row0, row0 + M) of y [Qtot, Cq].
 * kind PIO_QUERY_FOURIER: Fourier features of M index points of a d-dimensional grid (1 <= d <= 3) of sizes dims[0 : d]
 *   (output_queries.py BasicQuery._encode, position_encoding.py generate_fourier_features).  Row m:
 *     i = (points ? points[m] : start + m) mod prod(dims)   (the non-negative remainder, as unravel_index takes it),
 *     (coord_0, .., coord_{d-1}) the row-major unravel of i,  p_j = axis[j][coord_j]   (axis[j]: dims[j] floats),
 *     phase(j, k) = fmul_rn(fmul_rn(p_j, bands[j*ldb + k]), (float)M_PI)   (two separately rounded fp32 products),
 *   with c0 = concat_pos ? d : 0 and width = c0 + d*K*(sine_only ? 1 : 2):
 *     x[0 : d]               = p_j                 (concat_pos only)
 *     x[c0 + j*K + k]        = sinf(phase(j, k))
 *     x[c0 + d*K + j*K + k]  = cosf(phase(j, k))   (unless sine_only)
 *     x[width : Cq]          = pad[0 : Cq - width]
 *   bands: [d, K] with row pitch ldb >= K (K for a dense table).  The caller builds axis and bands with the host arithmetic
 *   of the chain it replaces (-1 + 2 * index / size; linspace(1, res / 2, K)).
 * kind PIO_QUERY_TABLE: x[0 : C] = table[m*ldt : m*ldt + C],  x[C : Cq] = pad[0 : Cq - C]   (width = C).
 * pad may be NULL where width == Cq, table where C == 0; axis[j] for j >= d, points, and the other kind's fields are not read. */
enum { PIO_QUERY_FOURIER = 0, PIO_QUERY_TABLE = 1 };
#define PIO_MAX_QUERY_SEGMENTS 4
typedef struct pio_query_segment_t {
    const float *axis[3];
    const float *bands;
    const int64_t *points;
    const float *table;
    const float *pad;
    int64_t start, ldb, ldt; /* first index when points == NULL; row pitches of bands and table in elements */
    int32_t kind;            /* PIO_QUERY_FOURIER / PIO_QUERY_TABLE */
    int32_t row0, M;
    int32_t d, dims[3], K, concat_pos, sine_only;
    int32_t C;
} pio_query_segment_t;

/* The decoder queries of a multi-modality model (PerceiverIO.decoder_query: per modality position encoding | padding
 * embedding, concatenated over the modalities) as ONE launch: nseg (1 .. 4) segments fill their rows of the batch-invariant
 * y [Qtot, Cq] fp32 (row pitch ldy).  Every element is stored once; rows no segment covers and the columns [Cq, ldy) are not
 * written.  Position, table and padding channels are moves; sine and cosine are the device library's accurate sincosf / sinf
 * of the phase above.  Rows leave as 16-byte vectors when Cq % 4 == 0, ldy % 4 == 0 and y is 16-byte aligned, as 8-byte
 * vectors when that holds with 2 and 8 (Cq = 1026), as dwords otherwise.  No workspace, no device allocation, no
 * synchronisation.
 * PIO_E_ARG: NULL segs / y, nseg outside [1, 4], an unknown kind, d outside [1, 3], K < 1, a NULL bands / axis[j < d] /
 * table (C > 0) pointer, a NULL pad where width < Cq; PIO_E_SHAPE: Qtot, Cq, M <= 0, ldy < Cq, dims[j] < 1 or prod(dims) >=
 * 2^31, ldb < K, C < 0, ldt < C, width > Cq, 32 feature rows (d*K*(sine_only ? 1 : 2) floats each) beyond 64 KiB of LDS
 * (d*K <= 247 with cosines, 487 without), a segment outside [0, Qtot), two segments that overlap; PIO_E_ALIGN: a float pointer not 4-byte
 * aligned, points not 8-byte aligned.  A refused call launches nothing. */
int pio_build_queries(const pio_query_segment_t *segs, int32_t nseg, float *y, int64_t ldy, int32_t Qtot, int32_t Cq,
                      void *stream);

/* One row segment of pio_project_heads: rows [row0, row0 + rows) of every sample of x go through the head (w, bias) into y.
 *   y[b*y_sb + r*y_rs + j] = bias[j] + sum_k w[j*ldw + k] * x[b*x_sb + (row0 + r)*ldx + k],  r in [0, rows), j in [0, n_out)
 * bias may be NULL (nothing is added); rows may be 0 (the segment does nothing, its pointers are still checked). */
#define PIO_MAX_HEAD_SEGMENTS 4
typedef struct pio_head_segment_t {
    int32_t row0, rows; /* rows [row0, row0 + rows) of every sample of x */
    const float *w;     /* [n_out, K] fp32, row pitch ldw >= K */
    int64_t ldw;
    const float *bias;  /* [n_out] fp32 or NULL */
    int32_t n_out;      /* 1 .. 16 */
    float *y;           /* y[b*y_sb + r*y_rs + j], r in [0, rows), j < n_out */
    int64_t y_sb, y_rs;
} pio_head_segment_t;

/* The narrow linear heads behind the decoder of a multi-modality model (postprocessors.py ProjectionPostprocessor /
 * AudioPostprocessor: an nn.Linear on a row range of the decoder output) as ONE launch: nseg (1 .. 4) segments of
 * x [B, Q, K] fp32 (row pitch ldx, sample stride x_sb; x_sb is not read when B == 1), each multiplied by its own
 * [n_out, K] fp32 weights and written straight into its own output array.  x is read once, as fp32, and the products are
 * fp32 FMAs: nothing is rounded to 16 bits, no temporary is made.  Rows of x that no segment covers are not read; of y only
 * the n_out columns of the rows [0, rows) of every sample are written: [n_out, y_rs) and everything else stay untouched.
 * Summation order (part of the definition): with lane l = (k / 4) % 64 and sweep i = k / 256,
 *   p_l = +0;  for i ascending, for k = 4*(l + 64*i) .. + 3 ascending (k < K):  p_l = fmaf(w[j, k], x[k], p_l)
 *   s   = pairwise tree over the 64 p_l: offsets 32, 16, 8, 4, 2, 1,  p_l = fadd_rn(p_l, p_(l xor offset))
 *   y   = bias ? fadd_rn(s, bias[j]) : s
 * so the bits of an output row depend only on that row of x, the segment's w, bias, n_out and K -- not on B, Q, row0, rows,
 * the strides, the other segments or the position of the row in the launch; there are no atomics.  A NaN in a row of x makes
 * the n_out outputs of that row NaN and no others.  No workspace, no device allocation, no synchronisation.
 * PIO_E_ARG: NULL segs / x / w / y, nseg outside [1, 4]; PIO_E_SHAPE: B or Q < 1, K outside [4, 1024] or not a multiple of
 * 4, ldx < K, n_out outside [1, 16], rows < 0, a segment outside [0, Q), ldw < K, y_rs < n_out, two non-empty segments whose
 * row ranges overlap, B * sum ceil(rows / 64) workgroups beyond 2^31 - 1; PIO_E_ALIGN: x or w not 16-byte aligned, ldx, ldw
 * or x_sb not a multiple of 4, y or bias not 4-byte aligned.  A refused call launches nothing. */
int pio_project_heads(const pio_head_segment_t *segs, int32_t nseg, const float *x, int64_t x_sb, int64_t ldx,
                      int32_t B, int32_t Q, int32_t K, void *stream);

/* The vocabulary head of the language model with its selection as ONE launch: rows r = b*Q + q of x [B, Q, K] fp32 (row pitch
 * ldx, sample stride x_sb; x_sb is not read when B == 1) against w [V, K] fp32 (row pitch ldw; the tied embedding), V <= 1024:
 *   logit[r, j]   = bias[j] + sum_k w[j*ldw + k] * x[b*x_sb + q*ldx + k]                    (bias may be NULL)
 *   lse[r]        = m + log(sum_j exp(logit[r, j] - m)),  m = max_j logit[r, j]
 *   ids[r*k + t]  = the t-th id of row r in the order: logit descending, the lower id first among equal logits (-0.0 and +0.0
 *                   are equal);  logprob[r*k + t] = fadd_rn(logit[r, ids[r*k + t]], -lse[r])
 * Outputs, each optional (NULL): ids int32 [B*Q, k], logprob fp32 [B*Q, k], lse fp32 [B*Q], logits fp32 [B*Q, V] with row
 * pitch ldl.  x is multiplied as fp32 (nothing is rounded to 16 bits) and only what is asked for is written.
 * Selection alone: x == w == NULL (bias NULL, K not read) -- logits is then the INPUT, [B*Q, V] with row pitch ldl, and ids,
 * logprob and lse are what the computing mode returns for those logits, bit for bit.
 * Summation order (part of the definition): with lane l = (k / 4) % 64 and sweep i = k / 256,
 *   p_l   = +0;  for i ascending, for k = 4*(l + 64*i) .. + 3 ascending (k < K):  p_l = fmaf(w[j, k], x[k], p_l)
 *   s     = pairwise tree over the 64 p_l: offsets 32, 16, 8, 4, 2, 1,  p_l = fadd_rn(p_l, p_(l xor offset))
 *   logit = bias ? fadd_rn(s, bias[j]) : s
 *   m     = fmaxf over j;  e_l = +0, for j = l, l + 64, .. ascending: e_l = fadd_rn(e_l, expf(fsub_rn(logit_j, m)));  S = the
 *           same tree over the 64 e_l;  lse = fadd_rn(m, logf(S))
 * so the bits of a row's results depend only on that row of x, w, bias, V, K and k -- not on B, Q, the strides or the
 * position of the row in the launch; there are no atomics.  A row holding a NaN logit has unspecified ids, all in [0, V),
 * and unspecified values; other rows are not affected.  No workspace, no device allocation, no synchronisation.
 * PIO_E_ARG: exactly one of x / w NULL, selection alone without logits or with a bias, no output pointer at all;
 * PIO_E_SHAPE: B or Q < 1, B*Q > 2^31 - 1, V outside [1, 1024], k outside [1, min(8, V)], logits given with ldl < V, and
 * when computing K outside [4, 1024] or not a multiple of 4, ldx < K, ldw < K; PIO_E_ALIGN: x or w not 16-byte aligned, ldx,
 * ldw or (B > 1) x_sb not a multiple of 4, any other pointer not 4-byte aligned.  A refused call launches nothing. */
int pio_vocab_topk(const float *x, int64_t x_sb, int64_t ldx, const float *w, int64_t ldw, const float *bias, int32_t B,
                   int32_t Q, int32_t V, int32_t K, int32_t k, int32_t *ids, float *logprob, float *lse, float *logits,
                   int64_t ldl, void *stream);

/* The language front end (io_processors.py EmbeddingPreprocessor: embed(ids) + learned position embedding) as ONE launch.
 * ids [B, T] int32 (id_bytes 4) or int64 (id_bytes 8), t contiguous, sample stride ids_sb elements; table [V, C] fp32 (row
 * pitch ldt); pos [T, C] fp32 (row pitch ldp); y [B, T, C] fp32 (row pitch ldy, sample stride y_sb); tokens: optional
 * (NULL) second output of the same shape with its own ldtok / tok_sb.  Sample strides are not read when B == 1.  Per
 * (b, t, c), with id = ids[b*ids_sb + t]:
 *   0 <= id < V:  y = fadd_rn(table[id*ldt + c], pos[t*ldp + c])  (one rounded fp32 add: the bits of `embed(ids) + pos`),
 *                 tokens = table[id*ldt + c];
 *   otherwise:    y and tokens are quiet NaN in all C channels of that row, no table row is read, and bad_ids[0] = 1 where
 *                 bad_ids (optional, a device int32) is given.  The range test is made on the full-width id.  The call never
 *                 clears the word and never reads it: the caller zeroes it on the stream before the call and reads it later.
 * Only the C channels of each of the B*T rows are written: [C, ld) and everything else stays untouched.  Rows leave as
 * 16-byte vectors when C, every pitch and (B > 1) every sample stride of a float array are multiples of 4 and table, pos, y
 * and tokens are 16-byte aligned; as dwords otherwise.  No workspace, no device allocation, no synchronisation.
 * PIO_E_ARG: NULL ids / table / pos / y, id_bytes not 4 or 8, ids not aligned to id_bytes, table / pos / y / tokens /
 * bad_ids not 4-byte aligned; PIO_E_SHAPE: B, T, C or V < 1, a pitch below C, for B > 1 ids_sb < T or y_sb < T*ldy or
 * tok_sb < T*ldtok, tokens == y, B * ceil(T / 32) workgroups beyond 2^31 - 1.  A refused call launches nothing. */
int pio_embed_tokens(const void *ids, int32_t id_bytes, int64_t ids_sb, const float *table, int64_t ldt, int32_t V,
                     const float *pos, int64_t ldp, float *y, int64_t y_sb, int64_t ldy, float *tokens, int64_t tok_sb,
                     int64_t ldtok, int32_t *bad_ids, int32_t B, int32_t T, int32_t C, void *stream);

/* The tail of tiled optical-flow inference (FlowPerceiver.forward with test_mode, flow_perceiver.py:165-190: every tile's
 * flow times a linear ramp that peaks at the tile centre, zero-padded to the image and summed, divided by the summed ramps)
 * as ONE launch.  The ny*nx tiles of size H x W have their top-left corners at the product ys x xs, ys outer, in list order:
 * tile k = iy*nx + ix lies in group[k / tiles_per_group] at local index j = k % tiles_per_group (the last group holds the
 * remaining tiles), and sample n of it is batch row j*N + n of that group, a fp32 [tiles*N, 2, H, W] view with the element
 * strides sn, sc, sy, sx (the same for every group).  out is [N, 2, h, w] fp32 with x contiguous and strides on, oc, oy.
 * Per output element (n, c, Y, X):
 *   acc = +0, wsum = +0
 *   for iy in 0 .. ny-1, for ix in 0 .. nx-1 (this order), ly = Y - ys[iy], lx = X - xs[ix], only where 0 <= ly < H and
 *   0 <= lx < W:
 *     r    = fdiv_rn((float)min(lx + 1, W - lx, ly + 1, H - ly), (float)min((W + 1) / 2, (H + 1) / 2))
 *     acc  = fadd_rn(acc, fmul_rn(flow_k[n, c, ly, lx], r))      (two rounded operations, never an FMA)
 *     wsum = fadd_rn(wsum, r)
 *   out = fdiv_rn(acc, wsum)                                      (both divisions correctly rounded)
 * which are the bits of the chain, signs of zeros included: where a tile does not cover a pixel the chain adds +0 to a sum
 * that began as +0.  The order of the tiles is part of the definition.  A tile begins inside the image and may hang over its
 * lower or right edge (compute_grid_indices makes such tiles when an inner corner lies behind h - H): what hangs over is
 * neither read nor written, as with the chain's negative padding.  Only the N*2*h*w elements of out are written: the
 * columns [w, oy) and everything else stay untouched; of a group only tile elements are read.  The struct is copied into the
 * kernel arguments: no table lives in device memory.  Both channels of a tile pixel are one 8-byte load when sc == 1,
 * sx == 2, sn and sy are even and every group pointer is 8-byte aligned (the permuted view of [B, H, W, 2] that
 * FlowPostprocessor returns); any other strides work, as two dword loads.  No workspace, no device allocation, no
 * synchronisation.
 * PIO_E_ARG: NULL p / out, NULL group[i] for i < ngroups; PIO_E_SHAPE: N, H or W < 1, h < H, w < W, ny or nx outside
 * [1, 64], ngroups outside [1, 64], tiles_per_group < 1, ngroups != ceil(ny*nx / tiles_per_group), a corner outside
 * [0, h - 1] / [0, w - 1], a row or column of the image that no tile covers (the chain gives 0 / 0 there), oy < w,
 * N * h * ceil(w / 256) workgroups beyond 2^31 - 1; PIO_E_ALIGN: out or a group pointer not 4-byte aligned.  A refused call
 * launches nothing. */
#define PIO_MAX_BLEND_AXIS 64
#define PIO_MAX_BLEND_GROUPS 64
typedef struct pio_flow_blend_t {
    const float *group[PIO_MAX_BLEND_GROUPS]; /* flows of tile group i */
    int64_t sn, sc, sy, sx; /* element strides of a group's [tiles*N, 2, H, W] view, the same for every group */
    int32_t ngroups, tiles_per_group;
    int32_t ny, nx; /* tile corners are the product ys x xs, ys outer, in list order */
    int32_t ys[PIO_MAX_BLEND_AXIS], xs[PIO_MAX_BLEND_AXIS];
    int32_t N, H, W, h, w; /* samples, tile size, image size */
} pio_flow_blend_t;
int pio_flow_blend_tiles(const pio_flow_blend_t *p, float *out, int64_t on, int64_t oc, int64_t oy, void *stream);

/* Optical-flow visualisation (utils/flow_utils.py flow_to_image, flow_utils.py:91-153 of the reference: the Middlebury
 * colour wheel, every image scaled by its own largest radius) for a batch, as a memset of the b maxima words and TWO
 * launches on the stream.  flow: fp32, element (n, y, x, component) at flow[n*sn + y*sy + x*sx + component*sc], read in
 * place ([b, 2, h, w] and a permuted [h, w, 2] view alike; the stride of a dimension of size 1 is not read); out: contiguous
 * uint8 [b, h, w, 3]; rad_max: b device words of scratch, overwritten (afterwards: each image's largest radius as an fp32
 * bit pattern).  Per image n and pixel, (u, v) the two components:
 *   has_clip:  u = u < 0 ? +0 : u, then u = u > clip_flow ? clip_flow : u, v likewise (np.clip; the lower bound IS 0; -0 stays)
 *   rad  = sqrt_rn(fadd_rn(fmul_rn(u, u), fmul_rn(v, v)));   rad_max[n] = max over the pixels of image n, never of the batch
 *   s    = fadd_rn(rad_max[n], 1e-5f);   un = fdiv_rn(u, s), vn = fdiv_rn(v, s);   radn = the rad of (un, vn)
 *   fk   = (atan2f(-vn, -un) / pi + 1) / 2 * 54;   k0 = floor(fk) clamped to [0, 54];   k1 = k0 + 1, 55 -> 0;   f = fk - k0
 *   col  = (1 - f) wheel[k0][ch] / 255 + f wheel[k1][ch] / 255;   col = radn <= 1 ? 1 - radn (1 - col) : 0.75 col
 *   out[n, y, x, bgr ? 2 - ch : ch] = floor(255 col)
 * Up to radn and the test radn <= 1 these are numpy's fp32 bits (every operation rounded on its own, no FMA; the maximum of
 * non-negative floats is taken with an integer atomic max on the bit pattern, so it is exact and the same in every run).
 * The wheel position and the colour run in fp32 where numpy goes through float64: a byte can differ from numpy's by one
 * where 255 col lies within about 1e-3 of an integer.  The sign of a zero component is honoured (atan2(-0, -u) against
 * atan2(+0, -u): wheel entry 0 against entry 54).  A non-finite flow value is undefined in the reference; here it yields
 * unspecified bytes for its image and nothing else: k0 and the byte are clamped before they index or convert anything.
 * The wheel (segments 15, 6, 4, 11, 13, 6) is a compile-time constant of the library.  A lane writes four consecutive
 * pixels of the flat [b*h*w] list as three dwords when out is 4-byte aligned (the last, partial group byte by byte), bytes
 * otherwise.  Only the 3*b*h*w bytes of out and the b words of rad_max are written.  No device allocation, no
 * synchronisation; the call can be captured into a graph.
 * PIO_E_ARG: NULL flow / out / rad_max; PIO_E_SHAPE: b, h or w < 1, h*w beyond 2^31 - 1, ceil(b*h*w / 1024) workgroups
 * beyond 2^31 - 1; PIO_E_ALIGN: flow or rad_max not 4-byte aligned.  A refused call launches nothing. */
int pio_flow_to_image(const float *flow, int64_t sn, int64_t sy, int64_t sx, int64_t sc, int32_t b, int32_t h, int32_t w,
                      float clip_flow, int32_t has_clip, int32_t bgr, uint8_t *out, uint32_t *rad_max, void *stream);

/* Media samples from an fp32 model output (what example_multimodal.py of the reference does on the host behind forward:
 * (np.clip(image, 0, 1) * 255).astype(np.uint8) frame by frame, (audio * 2**15).astype(np.int16)) as ONE launch.
 * x: fp32, element (i, r, p, c) of [n, h, w, C] at x[i*sn + r*sy + p*sx + c*sc], read in place (the stride of a dimension
 * of size 1 is not read); y: contiguous [n, h, w, C] of uint8 (PIO_MEDIA_U8) or int16 (PIO_MEDIA_S16); C in [1, 4].
 *   PIO_MEDIA_U8:   v = x < 0 ? 0 : x > 1 ? 1 : x, and v = 0 for a NaN;   y[.., reverse ? C - 1 - c : c] = (uint8) trunc(fmul_rn(v, 255))
 *                   -- numpy's fp32 bits of the expression above: -0.0 gives 0, 1 - ulp gives 254, 1 gives 255; reverse is
 *                   the channel order OpenCV's writer wants;
 *   PIO_MEDIA_S16:  t = fmul_rn(x, 32768) (exact);   y = trunc(t) saturated to [-32768, 32767], 0 for a NaN;  reverse must
 *                   be 0 -- inside [-1, 1) numpy's (a * 2**15).astype(np.int16); outside it numpy's conversion is undefined
 *                   (it wraps on common builds), here the sample SATURATES: 1.0 gives 32767, +-inf give 32767 / -32768.
 * Every output depends on its own input element only.  A lane writes four consecutive pixels of the flat [n*h*w] list, as
 * the widest vectors y's alignment allows where y is 4-byte aligned (the last, partial group element by element), as bytes
 * / shorts throughout otherwise.  sc == 1, sx == C, rows and images adjacent and x 16-byte aligned reads 16-byte vectors;
 * any other strides work, element by element.  Only the bytes of y are written.  No atomics, no workspace, no device
 * allocation, no synchronisation; the call can be captured into a graph.
 * PIO_E_ARG: NULL x / y, kind neither PIO_MEDIA_U8 nor PIO_MEDIA_S16, reverse with PIO_MEDIA_S16; PIO_E_SHAPE: n, h or w
 * < 1, C outside [1, 4], h*w beyond 2^31 - 1, ceil(n*h*w / 1024) workgroups beyond 2^31 - 1; PIO_E_ALIGN: x not 4-byte
 * aligned, an int16 y not 2-byte aligned.  A refused call launches nothing. */
#define PIO_MEDIA_U8 0
#define PIO_MEDIA_S16 1
int pio_finish_media(const float *x, int64_t sn, int64_t sy, int64_t sx, int64_t sc, int32_t n, int32_t h, int32_t w,
                     int32_t C, int32_t kind, int32_t reverse, void *y, void *stream);

/* Input images: crop, bilinear resize (with or without antialiasing), channel reversal and (v - mean) / std of a list of
 * images as ONE launch.  nsrc (1 .. PIO_MAX_IMAGE_SOURCES) descriptors, each n images of C channels and H x W pixels of uint8
 * or fp32 read in place: element (i, c, y, x) at data[i*sb + c*sc + y*sy + x*sx] (element strides, all >= 0; the stride of
 * an axis of length 1 is not read), of which the crop box rows [y0, y0 + ch), columns [x0, x0 + cw) is resampled to oh x ow.
 * out: fp32, image g (descriptors in order, images of a descriptor in order) at out + g*out_sb, [C, oh, ow] contiguous.
 * Per axis, `in` the crop length, `out` the output length, output index i has weights over crop indices j, every index
 * and numerator an integer and every weight ONE fp32 division (never scale * (i + 0.5) in floating point):
 *   antialias == 0:  q = max(0, (2i+1) in - out),  j0 = min(q / (2 out), in - 1),  l = (q - 2 out j0) / (2 out)
 *                    w[j0] = 1 - l,  w[j0 + 1] = l  (j0 == in - 1, where both taps fall on one pixel:  w[j0] = (1 - l) + l)
 *   antialias != 0:  d = 2 max(in, out),  lo = max(0, ((2i+1) in - d + out) / (2 out)),  hi = min(in, ((2i+1) in + d + out) / (2 out))
 *                    r[j] = max(0, 1 - |(2j+1) out - (2i+1) in| / d),  w[j] = r[j] / (r[lo] + .. + r[hi-1], ascending)
 * (integer divisions truncate), which are max(0, 1 - |j + 1/2 - centre| / support) of centre = (in/out)(i + 1/2), support =
 * max(in/out, 1) over trunc(centre -+ support + 1/2).  Then, with fmaf chains that start at +0 and run ascending:
 *   h[c, y, ox]  = sum_x wx[ox, x] * src[c, y0 + y, x0 + x]           (the horizontal pass, fp32 in LDS)
 *   v[c, oy, ox] = sum_y wy[oy, y] * h[c, y, ox]
 *   out[c, oy, ox] = fdiv_rn(fsub_rn(v[cs, oy, ox], mean[c]), std[c]),  cs = reverse_channels ? C - 1 - c : c
 * mean / std: HOST pointers to C floats, copied into the kernel arguments; NULL means 0 / 1.  The bits of an output value
 * depend on its own image, box and sizes only: not on n, the descriptor, its position or the other descriptors.  Non-finite
 * fp32 source values propagate as the arithmetic above has it (a zero weight times inf is NaN).  Exactly C*oh*ow values per
 * image are written and nothing else.  The table is copied into the kernel arguments; no workspace, no device allocation,
 * no synchronisation; the call can be captured into a graph.
 * PIO_E_ARG: NULL srcs / out / data, nsrc outside [1, PIO_MAX_IMAGE_SOURCES], dtype not PIO_IMAGE_U8 / PIO_IMAGE_F32;
 * PIO_E_SHAPE: C outside [1, 4] or a descriptor's C different, n < 1, H or W outside [1, 16384], oh or ow outside [1, 1024],
 * an empty box or one not inside the image, a negative stride, ch > PIO_IMAGE_MAX_REDUCTION * oh or cw > .. * ow, out_sb <
 * C*oh*ow with more than one image, more than 2^31 - 1 workgroups; PIO_E_ALIGN: fp32 data or out not 4-byte aligned.  A
 * refused call launches nothing. */
#define PIO_MAX_IMAGE_SOURCES 32
#define PIO_IMAGE_MAX_REDUCTION 40
#define PIO_IMAGE_U8 0
#define PIO_IMAGE_F32 1
typedef struct pio_image_src_t {
    const void *data;
    int64_t sb, sc, sy, sx; /* element strides: image, channel, row, column */
    int32_t dtype;          /* PIO_IMAGE_U8 / PIO_IMAGE_F32 */
    int32_t n, C, H, W;
    int32_t y0, x0, ch, cw; /* the crop box */
} pio_image_src_t;
int pio_prepare_images(const pio_image_src_t *srcs, int32_t nsrc, int32_t C, int32_t oh, int32_t ow, int32_t antialias,
                       int32_t reverse_channels, const float *mean, const float *std, float *out, int64_t out_sb,
                       void *stream);

/* C = epilogue(alpha * A B^T): A [M,K], B [N,K] operand dtype, K contiguous (multiple of 8).
 * Batched over z = zb*nh + zh with element strides; bias_mode 0 none / 1 per column / 2 per row;
 * act 0 none / 1 exact-erf GELU (F.gelu, transformer_primitives.py:214); optional fp32 residual R
 * added after the activation (row m of the flattened problem reads
 * R + (m / r_rows_per_batch)*r_stride_b + (m % r_rows_per_batch)*ldr when r_rows_per_batch > 0);
 * output fp32 (out_f32=1) or operand dtype with zero fill of columns [N, n_store).
 * The activation, y = gelu(x) of the fp32 pre-activation x = alpha acc + bias (tests/test_gemm_act_gpu.py holds every
 * kernel that applies it to this, over the whole domain):
 *   |x| <= 6:   within 1.1e-6 of x Phi(x) before the rounding of the output type (the fp32 model itself: 2.6e-7);
 *   |x| >  6:   Phi(-|x|) is frozen at Phi(-6) = 9.87e-10: y = x - x Phi(-6) for x > 0 and y = x Phi(-6) for x < 0 --
 *               not -> 0 --, an absolute error that grows as about 1e-9 |x|;
 *   the sign of y is the sign of x, gelu(+-0) = 0 and |y| <= |x| everywhere;
 *   NaN gives NaN; -inf gives -inf and +inf gives NaN (never a finite value: the range guard of the folded stacks
 *   relies on a non-finite activation staying visible).  gemm_nt_skinny applies no activation: act = 1 routes past it.
 * What a call touches (tests/test_gemm_addr_gpu.py holds every kernel to it, bit for bit, on NaN-surrounded buffers):
 *   read:    A / A_lo rows < M and B / B_lo rows < N of every (zb, zh) slice, columns < K -- never the pitch bytes
 *            [K, lda) / [K, ldb), never the gap between two slices, never rows of B_lo below b_lo_n0; bias entries < N
 *            (per column) or < M (per row); residual columns < N of the rows the formula above names -- one residual for
 *            every slice: it has no batch index of its own;
 *   written: rows < M, columns < n_store of every slice of C (and C_lo): columns [N, n_store) as +0, nothing in the
 *            pitch columns [n_store, ldc), nothing behind row M - 1, nothing between two slices.  Slices may interleave
 *            inside a row (sCh < ldc: heads side by side, n_store == N).
 * The LayerNorm-fold fields (tests/test_gemm_fold_gpu.py holds gemm_nt_wide and the six tile kernels to it the same way):
 *   producer  read:    R16_hi / R16_lo (or R) rows < M, columns < N -- never the pitch columns [N, ld16), never a row
 *                      behind M - 1; bias entries < N;
 *             written: rows < M, columns < N of X16, X16_lo and (when given) C, nothing in their pitch columns;
 *                      row_part[m < M][s < N / w][2]; *range_flag = 1 when some row's sum of squares is not finite, and
 *                      not touched otherwise (it is never cleared; the words beside it are never written).  In place
 *                      (R16_* == X16*) every element is read before it is written.  With integer-valued x every sum is
 *                      exact; else it is an fp32 sum in an order the kernel chooses.
 *   consumer  read:    ln_part rows < M, slots < ln_slots (any ln_slots > 0 on the tile kernels: it need not be K / 64),
 *                      ln_c and bias entries < N;
 *             written: rows < M, columns < n_store of C (and, tile kernels, C_lo), [N, n_store) as +0.
 *             mean = S / K, var = max(Q / K - mean^2, 0), rstd = 1 / sqrt(var + ln_eps) with S, Q the sums of the row's
 *             slots; 1 / sqrt is exact where var + ln_eps is a power of four.
 *   One K sweep on the tile kernels; on gemm_nt_wide the consumer and the 16-bit-pair producer also take B_lo, the
 *   fp32-residual producer B_lo and A_lo; alpha is applied by every producer; a consumer needs alpha == 1.
 * A descriptor no kernel takes returns its PIO_E_* code and writes nothing.  pio_gemm_kernel_override(1) never sends a
 * fold descriptor to the streaming kernel, which has no fold epilogue. */
typedef struct pio_gemm_t {
    const void *A, *B;
    const void *A_lo, *B_lo; /* optional extra K sweeps: C += A*B_lo^T, C += A_lo*B^T (split operands) */
    void *C;
    void *C_lo;              /* optional (16-bit output only): residual C - float(C16), same layout as C */
    int32_t M, N, K;
    int64_t lda, ldb, ldc;
    int32_t batch, nh;
    int64_t sAb, sAh, sBb, sBh, sCb, sCh;
    const float *bias;
    int32_t bias_mode;
    int32_t act;
    float alpha;
    const float *R;
    int64_t ldr, r_stride_b;
    int32_t r_rows_per_batch;
    int32_t out_f32;
    int32_t n_store;
    int32_t dtype;
    /* LayerNorm folded into the GEMMs around it (optional; a shape neither fold kernel takes: PIO_E_SHAPE).
     * Producer (fp32 out): X16 receives a 16-bit copy of the result (row stride ld16) and row_part, [M][N/w][2]
     * fp32, the (sum, sum of squares) of every result row over each w-column slot (w = row_slot_w below).
     * Consumer (16-bit out): ln_part is the row_part a producer wrote for this GEMM's A operand and
     * ln_c[n] = sum_k B[n,k]; the result is rstd_m * (A B^T)[m,n] - rstd_m * mean_m * ln_c[n] + bias[n] [GELU], i.e.
     * LayerNorm(x) W^T + b for B = W * gamma, bias = W beta + b (transformer_primitives.py:281-292). */
    void *X16;
    int64_t ld16;
    float *row_part;
    const float *ln_part;
    const float *ln_c;
    float ln_eps;
    /* The residual stream as a 16-bit pair (producer only): X16_lo receives result - float(X16) (same layout as X16),
     * and the residual may be given as R16_hi + R16_lo (row stride ld16, instead of the fp32 R).  With X16 and X16_lo
     * both set, C may be NULL: the fp32 result is then not written at all. */
    void *X16_lo;
    const void *R16_hi, *R16_lo;
    /* B_lo holds rows (= output columns) [b_lo_n0, N) only: the extra sweep C += A B_lo^T runs for those columns
     * alone.  0 = all rows.  Multiple of 256; kernel gemm_nt_wide only (else PIO_E_SHAPE). */
    int32_t b_lo_n0;
    /* LayerNorm-fold producer only (optional): *range_flag |= 1 when a row's (sum, sum of squares) is not finite */
    int32_t *range_flag;
    /* Slot form of the row statistics.  Producer: row_slot_w = columns per (sum, sum of squares) slot of row_part,
     * [M][N / row_slot_w][2]: 0 or 128 = the 256x256-tile kernel (gemm_nt_wide: N % 128 == 0), 64 = the 128 / 64-tile
     * kernel (stacks of fewer rows than the wide kernel takes; N % 64 == 0, residual and result as 16-bit pairs).
     * Consumer: ln_slots = slots per row of ln_part (0 = K / 128).  K / 128 slots, K % 128 == 0, K <= 1536 and
     * M >= 2048 run on gemm_nt_wide, anything else on the tile kernel. */
    int32_t ln_slots;
    int32_t row_slot_w;
} pio_gemm_t;
int pio_gemm_nt(const pio_gemm_t *g, void *stream);

/* P = softmax_j((S + bias) * scale) with masking, rows of length Tk (transformer_primitives.py:143-158,
 * 168-175): S fp32 [B,H,Tq,Tk] (row stride lds), P operand dtype [B,H,Tq,ldp] zero filled to ldp.
 * kv_mask [B,Tk], q_mask [B,Tq], full_mask [B,Tq,Tk] are optional uint8.  A row with no attendable key
 * is written as zeros (the reference's "wipe").  bias optional fp32 [B,H,Tq,Tk]; P_lo optional residual. */
int pio_softmax_rows(const float *S, int64_t lds, void *P, void *P_lo, int64_t ldp, int32_t B, int32_t H,
                     int32_t Tq, int32_t Tk, float scale, const uint8_t *kv_mask, const uint8_t *q_mask,
                     const uint8_t *full_mask, const float *bias, int32_t dtype, void *stream);

/* O = softmax(Q K^T / sqrt(dk)) V without the score matrix in HBM, un-masked (transformer_primitives.py:138-166 for the
 * latent self-attention): 16-bit Q [B][Tq][.. h*dkp ..] (row stride ldq, batch stride sQb elements), K likewise, V either
 * K-contiguous V^T [B][H*dvp][keys] (row stride ldv) or -- v_rowmajor != 0 -- row-major [B][Tk][.. h*dvp ..] (the layout ONE
 * fused q|k|v GEMM writes), O [B][Tq][.. h*dvp ..].  (dkp, dvp) in {(128,128), (64,64), (32,32), (32,160)}; dk = the logical
 * per-head width the scale uses.  The kernel the SelfAttention blocks run; exposed for tests and tools/r4_ceiling.py. */
int pio_flash_attention(int32_t dtype, int32_t dkp, int32_t dvp, int32_t dk, const void *Q, const void *K, const void *V,
                        void *O, int32_t B, int32_t H, int32_t Tq, int32_t Tk, int64_t ldq, int64_t ldk, int64_t ldv,
                        int64_t ldo, int64_t sQb, int64_t sKb, int64_t sVb, int64_t sOb, int32_t v_rowmajor, void *stream);

/* The fused attention cores with Q and K as 16-bit (hi, lo) PAIRS inside Q K^T (transformer_primitives.py:138-166; with the
 * mask vectors :168-175 too): S = Q_hi K_hi^T + Q_lo K_hi^T + Q_hi K_lo^T accumulated in fp32 (lo x lo dropped), everything
 * behind S as in the single-operand kernels (P rounded once).  Arguments as pio_flash_attention plus: Q_lo / K_lo (same
 * strides as their hi halves; both NULL = the single-operand sibling of the same kernel, for comparisons), O_lo (optional:
 * the rounding residual of O), kv_mask [B,Tk] / q_mask [B,Tq] (optional uint8 vectors; rows without an attendable key and
 * rows with q_mask == 0 are written as zeros) and
 *   core: 0 = by shape -- the self-attention kernel when no mask is given and it covers (dkp, dvp), else the cross-attention
 *         kernel; 1 = the self-attention kernel (flash_attn_kernel); 2 = the cross-attention kernel (xattn_kernel);
 *         3 = the tall-head kernel (xattn_tall_kernel: Tk <= 512, dkp >= 64 a multiple of 32, dvp a multiple of 256) with the
 *         operands of core 2 -- V^T (ldv >= 64, finite columns behind Tk), mask vectors, `workspace`, O_lo allowed, no
 *         Q_lo / K_lo -- PIO_E_SHAPE for any other shape, PIO_E_WORKSPACE below its key-bit words.  Core 0 never picks it.
 * The cross-attention kernel reads V^T only (v_rowmajor == 0, ldv a multiple of 32 with zero-filled columns behind Tk), reads
 * whole 32-key tiles of K / K_lo (the 31 rows behind key Tk - 1 of the last sample must be readable) and needs
 * `workspace` (pio_flash_attention_pair_workspace_bytes: key-bit words of a masked launch, fp32 partials of a key split;
 * for a shape only the tall-head kernel covers its key-bit words, for a shape both kernels cover the larger of the two, so
 * that the figure serves whichever core is named).
 * Pair operands: fp16 -- (32,32) / (32,160) / (128,128) on the self-attention kernel (the 128-wide head never with a key
 * split: 4 waves, or 8 under the 256-row rule), dkp <= 32 and dvp <= 160 on the cross-attention kernel; anything else with
 * Q_lo / K_lo is PIO_E_SHAPE: (64,64), (128,128) on core 2, bf16. */
size_t pio_flash_attention_pair_workspace_bytes(int32_t dkp, int32_t dvp, int32_t B, int32_t H, int32_t Tq, int32_t Tk);
int pio_flash_attention_pair(int32_t dtype, int32_t dkp, int32_t dvp, int32_t dk, const void *Q, const void *Q_lo,
                             const void *K, const void *K_lo, const void *V, void *O, void *O_lo, int32_t B, int32_t H,
                             int32_t Tq, int32_t Tk, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t sQb,
                             int64_t sKb, int64_t sVb, int64_t sOb, int32_t v_rowmajor, const uint8_t *kv_mask,
                             const uint8_t *q_mask, int32_t core, void *workspace, size_t workspace_bytes, void *stream);

/* --- blocks: the reference's nn.Module.forward calls ------------------------------------------ */
/* Attention.forward (transformer_primitives.py:90-115 + attend 117-180).  inputs_k and inputs_v must
 * have equal shapes.  out [B,Tq,out] fp32 contiguous.  probs_out (optional, fp32 [B,H,Tq,Tk]) receives
 * the attention matrix (return_matrix=True). */
size_t pio_attention_workspace_bytes(const pio_attention_t *a, int32_t B, int32_t Tq, int32_t Tk);
int pio_attention_fwd(const pio_attention_t *a, const pio_tensor3_t *inputs_q, const pio_tensor3_t *inputs_k,
                      const pio_tensor3_t *inputs_v, const uint8_t *kv_mask, const uint8_t *q_mask,
                      const uint8_t *full_mask, const float *attention_bias, float *out, float *probs_out,
                      void *workspace, size_t workspace_bytes, void *stream);

/* MLP.forward (transformer_primitives.py:212-216). out [B,T,out] fp32 contiguous. */
size_t pio_mlp_workspace_bytes(const pio_mlp_t *m, int64_t rows);
int pio_mlp_fwd(const pio_mlp_t *m, const pio_tensor3_t *x, float *out, void *workspace,
                size_t workspace_bytes, void *stream);

/* Per-call options of pio_encoder_fwd (pio_encoder_call_t.opts, by value) and pio_self_attention_fwd (a pointer; NULL or
 * all zero = the library defaults).  They replace, call by call and thread by thread, the process-wide switches
 * pio_ln_fold_enable / pio_set_cu_budget (which stay as test / A-B overrides): two threads driving two encoders on two
 * devices never see each other's choice.
 *   ln_fold:   0 = process-wide setting, 1 = LayerNorm fold off (the range guard's un-folded repeat), 2 = where it pays,
 *              3 = wherever a block offers it
 *   cu_budget: CUs the persistent GEMM kernels size their grids for (a CU-masked stream's share); 0 = process-wide */
typedef struct pio_call_opts_t {
    int32_t ln_fold;
    int32_t cu_budget;
} pio_call_opts_t;

/* SelfAttention.forward (transformer_primitives.py:275-297), no mask (perceiver.py:106 never passes one;
 * masks, attention_bias [B,H,N,N] and probs_out [B,H,N,N] (return_matrix) are accepted for interface
 * parity, all optional).  out [B,N,D] fp32 contiguous; out may alias x.data when x is contiguous.  opts: NULL = defaults. */
size_t pio_self_attention_workspace_bytes(const pio_self_attention_t *s, int32_t B, int32_t N);
int pio_self_attention_fwd(const pio_self_attention_t *s, const pio_tensor3_t *x, const uint8_t *kv_mask,
                           const uint8_t *q_mask, const uint8_t *full_mask, const float *attention_bias,
                           float *out, float *probs_out, const pio_call_opts_t *opts, void *workspace,
                           size_t workspace_bytes, void *stream);

/* CrossAttention.forward (transformer_primitives.py:371-406). out [B,Tq,q_in] fp32 contiguous. */
size_t pio_cross_attention_workspace_bytes(const pio_cross_attention_t *c, int32_t B, int32_t Tq, int32_t Tk);
int pio_cross_attention_fwd(const pio_cross_attention_t *c, const pio_tensor3_t *inputs_q,
                            const pio_tensor3_t *inputs_kv, const uint8_t *kv_mask, const uint8_t *q_mask,
                            const uint8_t *full_mask, const float *attention_bias, float *out, float *probs_out,
                            void *workspace, size_t workspace_bytes, void *stream);

/* PerceiverEncoder.forward (perceiver.py:98-107): cross-attend(latents <- inputs, key mask = input_mask)
 * then num_blocks x [layers[0..L)] weight-shared self-attends, as ONE call on one record (a zeroed record with cross,
 * layers, L, num_blocks, inputs, latents and out set is the plain call). */
typedef struct pio_encoder_call_t {
    const pio_cross_attention_t *cross;
    const pio_self_attention_t *layers; /* L descriptors (num_blocks * L with per_block); may be NULL when L == 0 */
    int32_t L, num_blocks;
    /* != 0: ONE SET OF PACKED IMAGES PER BLOCK, block b runs layers[b*L .. b*L + L).  The reference shares the parameters
     * of the L layers over the num_blocks blocks (perceiver.py:104-106); with one 16-bit image per weight its rounding
     * error then acts num_blocks times in the same direction.  Under the "fp16sd" policy the binder packs block b from
     * fp16(W + E_{b-1}), E_b = (W + E_{b-1}) - image_b (error feedback over the block index: every image is a rounding of
     * W within one ulp, their accumulated error stays below half an ulp) -- same shapes, same kernels, same time. */
    int32_t per_block;
    const pio_tensor3_t *inputs; /* [B,M,C] */
    /* optional: the encoder input given as two channel-wise concatenated arrays [inputs | inputs_tail] (inputs_tail->B
     * == 1: one batch-invariant table): the ImageNet preprocessor's 64 conv features [B,3136,64] and its [3136,258]
     * Fourier table instead of the replicated [B,3136,322] array (preprocessors.py:176-200); layer_norm_kv runs over the
     * virtual concatenation, nothing is concatenated in HBM. */
    const pio_tensor3_t *inputs_tail;
    /* the query tensor the caller built (PerceiverEncoder.latents, perceiver.py:94-96: normally a stride-0 broadcast of
     * the [N,D] table) */
    const pio_tensor3_t *latents;
    const uint8_t *input_mask; /* optional [B,M] */
    float *out;                /* [B,N,D] fp32 contiguous */
    pio_call_opts_t opts;      /* all zero = the library defaults */
} pio_encoder_call_t;
size_t pio_encoder_workspace_bytes(const pio_cross_attention_t *cross, const pio_self_attention_t *layers,
                                   int32_t L, int32_t B, int32_t M, int32_t N);
/* PIO_E_ARG: NULL record, cross, inputs, latents, out or workspace, NULL layers with L > 0. */
int pio_encoder_fwd(const pio_encoder_call_t *c, void *workspace, size_t workspace_bytes, void *stream);

/* PerceiverDecoder.forward (perceiver.py:166-180): cross-attend(query <- latents, query mask) and the optional final
 * nn.Linear, as ONE call on one record (a zeroed record with cross, query, latents and out set is the plain call). */
typedef struct pio_decoder_call_t {
    const pio_cross_attention_t *cross;
    const pio_linear_t *final_layer; /* NULL => final_project=False */
    int32_t final_out;               /* output channels of final_layer */
    const pio_tensor3_t *query;      /* [B,Q,C] */
    /* optional: the query rows handed over as TWO arrays whose channels are concatenated, [query | query_tail]
     * (query_tail->B == 1: one batch-invariant table) -- the dense decoders whose queries ARE the network's preprocessed
     * input (flow_perceiver.py: FlowQuery = [conv features | Fourier position table]): layer_norm_q runs over the virtual
     * concatenation, nothing is concatenated in HBM.  Needs cross->use_query_residual == 0, a per-sample query tensor and
     * q16_hi == NULL: PIO_E_ARG otherwise, before anything is launched. */
    const pio_tensor3_t *query_tail;
    const pio_tensor3_t *latents;
    const uint8_t *query_mask; /* optional [B,Q] */
    float *out;                /* [B,Q,out_channels] fp32 */
    /* optional: the PROJECTED QUERIES kept by the caller across calls.  A decoder whose query array depends on parameters
     * and constants only (the multimodal model's per-chunk Fourier queries, multimodal_perceiver.py:146-161) normalises
     * and projects it once: q16_hi (and q16_lo when the attention descriptor carries split activations) are caller-owned
     * device buffers of pio_decoder_qcache_bytes(cross, Bq, Q) bytes each, Bq = 1 for a stride-0 (batch-invariant) query
     * tensor, else B.  q16_valid == 0: LayerNorm_q + proj_q run and leave their result there; != 0: both are skipped and
     * the buffers are read.  Only for cross->use_query_residual == 0 (PIO_E_ARG otherwise: the query rows themselves are
     * needed then); the caller invalidates when the query array, layer_norm_q, proj_q or the precision policy change. */
    void *q16_hi, *q16_lo;
    int32_t q16_valid;
} pio_decoder_call_t;
size_t pio_decoder_workspace_bytes(const pio_cross_attention_t *cross, const pio_linear_t *final_layer,
                                   int32_t B, int32_t Q, int32_t N);
size_t pio_decoder_qcache_bytes(const pio_cross_attention_t *cross, int32_t Bq, int32_t Q);
/* PIO_E_ARG: NULL record, cross, query, latents, out or workspace; PIO_E_ALIGN: q16_hi / q16_lo not 16-byte aligned. */
int pio_decoder_fwd(const pio_decoder_call_t *c, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIO_HIP_H */
