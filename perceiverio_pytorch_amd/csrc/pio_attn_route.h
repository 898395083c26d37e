// Attention routing (host only, plain C++17: no HIP, no environment, no state): the shape tables of the fused attention
// kernels, which core one attention call runs on and what its plan has to carve (attn_route / attn_plan), the variant of
// the self-attention kernel a launch gets (flash_route), the operand bundle the three launchers share, and the launch plan
// of each of them (flash / xattn / xtall_launch_plan: the refusals in the order that decides a bad call's PIO_E_* code,
// then the grid arithmetic).  pio_blocks.hip and the three launchers launch what these return; tests/test_attn_route.py
// checks them on the CPU.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/pio_hip.h"

namespace pio {

// ---- self-attention kernel (pio_flash.hip) ------------------------------------------------------------------------
inline bool flash_supported(int dkp, int dvp) {
    return (dkp == 128 && dvp == 128) || (dkp == 64 && dvp == 64) || (dkp == 32 && dvp == 32) ||
           (dkp == 32 && dvp == 160);
}
// Q / K as (hi, lo) pairs inside the fused cores' Q K^T (S = Q_hi K_hi + Q_lo K_hi + Q_hi K_lo): the dk <= 32 fp16
// instantiations of both kernel families and the (128, 128) fp16 head of the self-attention kernel (the latent stack
// of the classifier).  A launch with Q_lo / K_lo on any other shape or dtype -- (64, 64), bf16 -- is PIO_E_SHAPE.
inline bool flash_pair_supported(int dtype, int dkp, int dvp) {
    return dtype == PIO_DT_F16 && ((dkp == 32 && (dvp == 32 || dvp == 160)) || (dkp == 128 && dvp == 128));
}

struct FlashRoute {
    bool v_rowmajor;  // V [keys][H*dv] through transposed LDS reads (the q|k|v form) / V^T [dv][keys]
    int NW, KS;       // waves per workgroup (4, 8, 16), key parts (1, 2, 4): the kernel's template arguments
    int nqt;          // query tiles of 128 rows (NW = 8, KS = 1: 256 rows) per (batch, head)
    int threads;      // 64 NW
};
// The kernel variant of one launch.  ksplit_on: the PIO_FLASH_KSPLIT switch, cu_budget: CUs the launch may count on.
inline FlashRoute flash_route(int dkp, int dvp, int B, int H, int Tq, int Tk, bool v_rowmajor, bool ksplit_on,
                              int cu_budget) {
    // 256-row workgroups when that still gives every CU a workgroup (row-major-V flagship path only)
    const bool wide = v_rowmajor && Tq >= 256 && (int64_t)B * H * ((Tq + 255) / 256) >= 256;
    // (64-row workgroups for small batches -- B = 1: 64 workgroups instead of 32 -- were measured in round 3: 4.00 ms
    //  against 3.82 ms per B = 1 forward; two waves issuing a whole tile's DMA cost more than the idle CUs: not kept)
    const int nqt = wide ? (Tq + 255) / 256 : (Tq + 127) / 128;
    // key split over two wave groups (KS = 2): when the launch offers at most one 128-row workgroup per CU
    const bool ksplit = ksplit_on && v_rowmajor && !wide && Tk >= 256 && (Tk % 128) == 0 && (int64_t)B * H * nqt <= cu_budget;
    // (four key parts = 16 waves per workgroup, four per SIMD: the narrow heads, whose waves need < 128 registers)
    const bool ksplit4 = ksplit && dkp <= 64 && dvp <= 64 && Tk >= 1024 && (Tk % 256) == 0;
    const int NW = ksplit4 ? 16 : (ksplit || wide) ? 8 : 4;
    return FlashRoute{v_rowmajor, NW, ksplit4 ? 4 : ksplit ? 2 : 1, nqt, 64 * NW};
}
// ... of a pair-operand launch (Q_lo / K_lo set).  dkp = 32: the same variants.  dkp = 128: a ring stage holds K, K_lo
// and V (48 KB), two key parts would need 192 KB of LDS -- no key split; 8 waves under the same rule, else 4.
inline FlashRoute flash_pair_route(int dkp, int dvp, int B, int H, int Tq, int Tk, bool v_rowmajor, bool ksplit_on,
                                   int cu_budget) {
    FlashRoute r = flash_route(dkp, dvp, B, H, Tq, Tk, v_rowmajor, ksplit_on, cu_budget);
    if (dkp == 128 && r.KS != 1) {  // (a key split never changes nqt: 128-row tiles either way)
        r.NW = 4;
        r.KS = 1;
        r.threads = 64 * r.NW;
    }
    return r;
}

// ---- cross-attention kernel (pio_xattn.hip): wide single heads, dv != dk, key / query mask vectors, key splits ------
struct XCfg { int dkl, dvs; };
// the kernel instantiations, narrowest first
// (the sliced <352,192> / <512,256> instantiations of round 2 became unreachable when the single-pass <352,352> /
// <512,512> ones were put in front of them in round 3 -- first match wins -- and are gone)
constexpr XCfg kCfgs[] = {{32, 96}, {32, 160}, {128, 128}, {352, 352}, {512, 512}, {704, 256}};

inline const XCfg *xattn_cfg(int dkp, int dvp) {
    for (const XCfg &c : kCfgs) {
        if (dkp > c.dkl) continue;
        // a head wider than one slice is cut into dv slices (each recomputes S): only where Q + O do not fit otherwise
        const bool sliced = c.dkl >= 352;
        if (dvp <= c.dvs || (sliced && dvp <= c.dkl)) return &c;
    }
    return nullptr;
}
inline bool xattn_supported(int dkp, int dvp) { return xattn_cfg(dkp, dvp) != nullptr; }
// pair-operand Q K^T: the narrow-head instantiations <32, 96> and <32, 160>, fp16
inline bool xattn_pair_supported(int dtype, int dkp, int dvp) {
    const XCfg *c = xattn_cfg(dkp, dvp);
    return dtype == PIO_DT_F16 && c && c->dkl == 32;
}

// key splits for a launch: about one workgroup per CU and resident slot (wide heads hold one workgroup per CU, narrow
// ones two) when batch x heads x query tiles x slices alone give clearly fewer, each split keeping >= 8 key tiles.
// The partials cost HBM traffic (4 dv bytes per query row and split, written and read back): no more splits than that.
inline int xattn_splits(int dkp, int dvp, int B, int H, int Tq, int Tk) {
    const XCfg *c = xattn_cfg(dkp, dvp);
    if (!c) return 1;
    const int nslice = (dvp + c->dvs - 1) / c->dvs;
    const int64_t base = (int64_t)B * H * ((Tq + 127) / 128) * nslice;
    const int ntiles = (Tk + 31) / 32;
    const int64_t target = (c->dkl <= 128 && c->dvs <= 160) ? 512 : 256;
    if (base * 5 >= target * 4 || ntiles < 16) return 1;
    int64_t s = (target + base - 1) / base;
    if (s > ntiles / 8) s = ntiles / 8;
    return s < 1 ? 1 : (int)s;
}

// scratch of one launch: the key-bit words of a masked launch [B][ntiles], then the fp32 partials of the key splits
inline size_t keybits_bytes(int B, int Tk) { return ((size_t)B * ((Tk + 31) / 32) * 4 + 255) & ~(size_t)255; }
inline size_t xattn_partial_bytes(int dkp, int dvp, int B, int H, int Tq, int Tk) {
    const int s = xattn_splits(dkp, dvp, B, H, Tq, Tk);
    return keybits_bytes(B, Tk) + (s <= 1 ? 0 : (size_t)B * H * s * Tq * ((size_t)dvp * 4 + 8) + 512);
}

// ---- cross-attention for a head wider than the key axis is long (pio_xtall.hip): Tk <= 512, S computed once per query
// row and kept in registers (the ImageNet decoder's 1024-wide head over 512 latents) ---------------------------------
constexpr int T_NKB = 16;  // key blocks of 32: the kernel always covers 512 keys
inline bool xtall_supported(int dkp, int dvp, int Tk) {
    return Tk >= 1 && Tk <= 32 * T_NKB && dkp >= 64 && (dkp % 32) == 0 && dvp >= 256 && (dvp % 256) == 0;
}
inline size_t xtall_scratch_bytes(int B) { return ((size_t)B * T_NKB * 4 + 255) & ~(size_t)255; }  // key-bit words

// ---- operands of one fused-core launch ----------------------------------------------------------------------------
struct AttnOperands {
    const void *Q, *Q_lo, *K, *K_lo, *VT;  // *_lo: rounding residuals (both or neither; pair instantiations only)
    void *O, *O_lo;                        // O_lo (optional): the output as a pair
    int64_t ldq, ldk, ldvt, ldo;           // row pitches (elements); VT is V^T [B][H*dvp][keys] unless v_rowmajor
    int64_t sQb, sKb, sVb, sOb;            // batch strides (elements); sQb = 0 for batch-invariant queries
};
inline bool attn_lo_halves_paired(const AttnOperands &t) { return (!t.Q_lo) == (!t.K_lo); }
inline int attn_operands_present(const AttnOperands &t) {
    return (!t.Q || !t.K || !t.VT || !t.O || !attn_lo_halves_paired(t)) ? PIO_E_ARG : PIO_OK;
}
// 16-byte operand rows / pointers (one LDS-DMA piece), 8-byte output rows
inline int attn_operands_aligned(const AttnOperands &t) {
    if ((t.ldq % 8) || (t.ldk % 8) || (t.ldvt % 8) || (t.ldo % 4) || (t.sQb % 8) || (t.sKb % 8) || (t.sVb % 8) || (t.sOb % 4))
        return PIO_E_ALIGN;
    const uintptr_t in = (uintptr_t)t.Q | (uintptr_t)t.K | (uintptr_t)t.VT | (uintptr_t)t.Q_lo | (uintptr_t)t.K_lo;
    return ((in & 15) || (((uintptr_t)t.O | (uintptr_t)t.O_lo) & 7)) ? PIO_E_ALIGN : PIO_OK;
}

// ---- launch plans of the three fused cores ---------------------------------------------------------------------------
// Everything a launcher decides before it fills its kernel's parameter struct.  `err` first: the refusals come in the
// launcher's own order, which is part of the C ABI's contract (a call that breaks two rules gets the first one's code).
inline float attn_scale_log2(int dk_logical) { return 1.4426950408889634f / sqrtf((float)dk_logical); }  // log2(e) / sqrt(dk)
// what the profiler books for one fused-core launch (S recomputed per dv slice counts once: the reference's flops)
struct AttnWork { double flops, bytes; };
inline AttnWork attn_work(int dkp, int dvp, int B, int H, int Tq, int Tk) {
    return AttnWork{2.0 * B * H * (double)Tq * Tk * (dkp + dvp),
                    2.0 * B * H * ((double)Tq * (dkp + dvp) + (double)Tk * (dkp + dvp))};
}
// The checks all three share, behind each launcher's shape table: operands present, the launcher's pair rule (its code,
// PIO_OK when it has no objection), positive extents, alignment.
inline int attn_launch_checks(const AttnOperands &t, int pair_err, bool extents_ok) {
    if (attn_operands_present(t) != PIO_OK) return PIO_E_ARG;
    if (pair_err != PIO_OK) return pair_err;
    if (!extents_ok) return PIO_E_SHAPE;
    return attn_operands_aligned(t);
}
constexpr int64_t kGridMax = 0x7fffffffLL, kOffsetLimit = 1ll << 31;  // workgroups of a 1-D grid; 32-bit element offsets

// O_lo only with Q_lo / K_lo: the single-operand instantiations of the self-attention kernel write one half
inline bool flash_o_lo_allowed(const AttnOperands &t) { return !t.O_lo || t.Q_lo; }
struct FlashPlan {
    int err;
    FlashRoute route;
    bool pair;      // Q and K as (hi, lo) pairs
    int o_rows16;   // O rows are 16-byte aligned and leave as one half: the staged whole-row epilogue
    int64_t grid;
};
inline FlashPlan flash_launch_plan(int dtype, int dkp, int dvp, const AttnOperands &t, int B, int H, int Tq, int Tk,
                                   bool v_rowmajor, bool ksplit_on, int cu_budget) {
    FlashPlan p = {};
    p.pair = t.Q_lo != nullptr;
    const int pair_err = !flash_o_lo_allowed(t) ? PIO_E_ARG
                         : (p.pair && !flash_pair_supported(dtype, dkp, dvp)) ? PIO_E_SHAPE : PIO_OK;  // (never a silent single-operand run)
    p.err = !flash_supported(dkp, dvp)
                ? PIO_E_SHAPE
                : attn_launch_checks(t, pair_err, B > 0 && H > 0 && Tq > 0 && Tk > 0 && (int64_t)B * H * ((Tq + 127) / 128) <= kGridMax);
    if (p.err) return p;
    p.route = p.pair ? flash_pair_route(dkp, dvp, B, H, Tq, Tk, v_rowmajor, ksplit_on, cu_budget)
                     : flash_route(dkp, dvp, B, H, Tq, Tk, v_rowmajor, ksplit_on, cu_budget);
    // (an output PAIR leaves through the per-lane 8-byte stores: the staged whole-row epilogue carries one half only)
    p.o_rows16 = (!t.O_lo && t.ldo % 8 == 0 && t.sOb % 8 == 0 && ((uintptr_t)t.O & 15) == 0) ? 1 : 0;
    p.grid = (int64_t)p.route.nqt * B * H;
    return p;
}

struct XattnPlan {
    int err;
    XCfg cfg;
    bool pair;
    int nqt, nslice, nsplit, ntiles, tiles_per_split;
    int64_t grid;
    size_t part_o_off, part_ml_off;  // bytes into the scratch, behind the key-bit words (part_ml: key splits only)
};
inline XattnPlan xattn_launch_plan(int dtype, int dkp, int dvp, const AttnOperands &t, int B, int H, int Tq, int Tk,
                                   bool has_kv_mask, bool has_scratch) {
    XattnPlan p = {};
    const XCfg *c = xattn_cfg(dkp, dvp);
    p.pair = t.Q_lo != nullptr;
    const int pair_err = (p.pair && !xattn_pair_supported(dtype, dkp, dvp)) ? PIO_E_SHAPE : PIO_OK;  // (never a silent single-operand run)
    p.err = !c ? PIO_E_SHAPE
               : attn_launch_checks(t, pair_err, B > 0 && H > 0 && Tq > 0 && Tk > 0 && !(dkp & 7) && !(dvp & 7));
    if (p.err) return p;
    p.cfg = *c;
    auto refuse = [&p](int err) { p.err = err; return p; };
    // (the kernel's per-lane source offsets are 32-bit element offsets)
    if (t.ldvt < 8 || 32 * t.ldk >= kOffsetLimit || (int64_t)dvp * t.ldvt >= kOffsetLimit) return refuse(PIO_E_SHAPE);
    p.nslice = (dvp + c->dvs - 1) / c->dvs;
    p.nqt = (Tq + 127) / 128;
    p.nsplit = xattn_splits(dkp, dvp, B, H, Tq, Tk);
    p.ntiles = (Tk + 31) / 32;
    p.tiles_per_split = (p.ntiles + p.nsplit - 1) / p.nsplit;
    if ((p.nsplit > 1 || has_kv_mask) && !has_scratch) return refuse(PIO_E_WORKSPACE);
    if (t.ldvt % 32) return refuse(PIO_E_ALIGN);  // V^T rows are read in whole 32-key tiles (zero padded by the caller)
    p.grid = (int64_t)B * H * p.nqt * p.nslice * p.nsplit;
    if (p.grid > kGridMax) return refuse(PIO_E_SHAPE);
    p.part_o_off = keybits_bytes(B, Tk);
    p.part_ml_off = p.part_o_off + (size_t)B * H * p.nsplit * Tq * dvp * sizeof(float);
    return p;
}

// the tall-head kernel has no pair-operand instantiation
inline bool xtall_takes(int dkp, int dvp, int Tk, const AttnOperands &t) { return xtall_supported(dkp, dvp, Tk) && !t.Q_lo; }
struct XtallPlan {
    int err;
    int nqt, nka, npass;  // query tiles of 128 rows, dk chunks of 32, dv passes of 256
    int64_t grid;
};
inline XtallPlan xtall_launch_plan(int dkp, int dvp, const AttnOperands &t, int B, int H, int Tq, int Tk, bool has_kv_mask,
                                   bool has_scratch) {
    XtallPlan p = {};
    p.err = !xtall_takes(dkp, dvp, Tk, t) ? PIO_E_SHAPE : attn_launch_checks(t, PIO_OK, B > 0 && H > 0 && Tq > 0);
    if (p.err) return p;
    auto refuse = [&p](int err) { p.err = err; return p; };
    if (t.ldvt < 64 || (int64_t)Tk * t.ldk >= kOffsetLimit || (int64_t)Tq * t.ldq >= kOffsetLimit || 256 * t.ldvt >= kOffsetLimit)
        return refuse(PIO_E_SHAPE);
    if (has_kv_mask && !has_scratch) return refuse(PIO_E_WORKSPACE);
    p.nqt = (Tq + 127) / 128;
    p.nka = dkp / 32;
    p.npass = dvp / 256;
    p.grid = (int64_t)B * H * p.nqt;
    if (p.grid > kGridMax) return refuse(PIO_E_SHAPE);
    return p;
}

// ---- which core one attention call runs on ------------------------------------------------------------------------
enum class AttnCore {
    QKV_FLASH,     // one GEMM over the stacked [q | k | v] image, self-attention kernel reading V row-major
    KVFOLD_XATTN,  // K / V projection fold (pio_attention_t.kq / vo): the cross-attention kernel on the inputs themselves
    KVFOLD_XTALL,  // ... the tall-head kernel
    PAIR_FLASH,    // act_split 3: Q and K as (hi, lo) pairs, self-attention kernel
    PAIR_XATTN,    // ... cross-attention kernel (mask vectors)
    FLASH,         // self-attention kernel on V^T
    XATTN,         // cross-attention kernel
    XTALL,         // tall-head kernel
    MATERIALISED,  // score GEMM, softmax_rows, P V GEMM
};

// The fused core of a call that needs no score matrix: the self-attention kernel (where flash_ok) for un-masked
// attention with its head widths, the cross-attention kernels for key / query mask VECTORS, wide single heads, dv != dk
// and few query tiles (key splits).  MATERIALISED: none covers the shape.
inline AttnCore fused_core(int dkp, int dvp, int Tk, bool mask_vectors, bool flash_ok) {
    if (flash_ok && !mask_vectors && flash_supported(dkp, dvp)) return AttnCore::FLASH;
    if (xattn_supported(dkp, dvp)) return AttnCore::XATTN;
    // a head wider than the tiled kernel covers over <= 512 keys (the ImageNet decoder): the score row stays in registers
    return xtall_supported(dkp, dvp, Tk) ? AttnCore::XTALL : AttnCore::MATERIALISED;
}

// The optional operands of one attention call, as they travel from an entry point down to the core (all null = none):
// key mask [B,Tk], query mask [B,Tq], full mask [B,Tq,Tk], bias [B,H,Tq,Tk], probability output [B,H,Tq,Tk].
struct AttnOptional {
    const uint8_t *kv_mask = nullptr, *q_mask = nullptr, *full_mask = nullptr;
    const float *bias = nullptr;
    float *probs = nullptr;
};
// ... as the facts of an AttnCall / SelfCall (pio_block_route.h)
template <class Call>
inline void note_optional(Call &c, const AttnOptional &o) {
    c.kv_mask = o.kv_mask; c.q_mask = o.q_mask; c.full_mask = o.full_mask; c.bias = o.bias; c.probs = o.probs;
}

struct AttnCall {  // what attention_core knows about one call, as plain facts
    int B, Bq, Tq, Tk;  // Bq = 1 for batch-invariant queries (q_bcast), else B
    bool q_bcast;
    bool same_qk, same_kv;                         // q and k / k and v read the same 16-bit input
    bool kv_mask, q_mask, full_mask, bias, probs;  // which optional operands the call passes
    bool qcache;                                   // projected queries kept by the caller
    bool fold_in, fold_out;                        // LayerNorm fold wired in front of / behind the block
    const pio_linear_t *fold_qkv;                  // the fold's q|k|v image when it is the one in use, else null
    bool kv_fold_on;                               // the K / V-fold switch (PIO_KV_FOLD, read by the caller)
    bool qkv_adjacent, qk_adjacent;  // the caller's q16 | k16 (| vt16) carves hold one [rows, q|k(|v)] matrix
};

struct AttnRoute {
    int err;  // PIO_OK, or the PIO_E_* code of a call no form takes
    AttnCore core;
    bool fuse_qk;       // Q and K projections as one GEMM over the stacked [q | k] image
    bool qk_pair;       // Q and K enter the core as (hi, lo) pairs
    bool out_pair;      // the core returns its output as a pair
    bool need_scores;   // score and probability buffers
    size_t xpart_bytes; // scratch of the cross-attention cores (key bits, split partials) a plan of this shape holds
};

inline AttnRoute attn_route(const pio_attention_t &a, const AttnCall &c) {
    const int H = a.heads;
    const int64_t hdk = (int64_t)H * a.dkp, ldo = (int64_t)H * a.dvp;
    const bool mask_vectors = c.kv_mask || c.q_mask;
    const bool plain = !mask_vectors && !c.full_mask && !c.bias && !c.probs;  // nothing but Q, K, V
    // act_split == 2 ("x3f"): the projections around the core run with split operands, the core itself single-sweep
    // on the hi halves of q / k / v^T through the fused cross-attention kernel, which returns its output as a pair.
    // act_split == 3 ("x3fq"): as 2, with Q and K entering the core as the (hi, lo) pairs the projection GEMMs wrote (a
    // projected-query cache holds both halves too).  Pair cores exist for the dk <= 32 fp16 heads (both kernel families)
    // and for the (128, 128) fp16 head on the self-attention kernel alone, so the question is asked per core: a call with
    // mask vectors has one only in the cross-attention family.  Every other shape -- 64-wide heads, masked 128-wide heads,
    // wide single heads, xattn_tall_kernel, the K / V-folded path, bf16 -- takes the MATERIALISED split-operand path,
    // exactly what act_split == 1 runs: a pair request never silently becomes a single-operand Q K^T.
    const bool pair_core = a.act_split == 3 && (xattn_pair_supported(a.dtype, a.dkp, a.dvp) ||
                                                (!mask_vectors && flash_pair_supported(a.dtype, a.dkp, a.dvp)));
    const bool single_core = a.act_split == 2 || pair_core;
    const bool fused_policy = !a.act_split || single_core;
    AttnRoute r = {PIO_OK, AttnCore::MATERIALISED, false, false, false, false, 0};
    auto take = [&r](AttnCore core) { r.core = core; return r; };
    if (fused_policy)
        r.xpart_bytes = xattn_supported(a.dkp, a.dvp)     ? xattn_partial_bytes(a.dkp, a.dvp, c.B, H, c.Tq, c.Tk)
                        : xtall_supported(a.dkp, a.dvp, c.Tk) ? xtall_scratch_bytes(c.B) : 0;

    // 0: the fully fused self-attention form.  Needs: same input for q, k and v, single-sweep operands everywhere, head
    //    widths the fused kernel covers, nothing that wants the score matrix, and the q16 | k16 | vt16 scratch regions
    //    holding one [rows, H*(2 dk + dv)] matrix.  (A q|k|v image whose V rows alone carry a lo half -- policies "x2s" /
    //    "x2w" -- is taken only inside the LayerNorm fold, where the wide GEMM kernel, which honours lo_row0, is guaranteed.)
    const pio_linear_t &qkv_used = c.fold_qkv ? *c.fold_qkv : a.qkv;
    const bool qkv_lo_ok = !qkv_used.w_lo || (c.fold_qkv && qkv_used.lo_row0 == 2 * hdk);
    if (!c.qcache && a.qkv.w_hi && qkv_lo_ok && !a.act_split && !c.q_bcast && c.same_qk && c.same_kv && c.Tq == c.Tk &&
        flash_supported(a.dkp, a.dvp) && a.qkv.n == 2 * hdk + ldo && plain && c.qkv_adjacent)
        return take(AttnCore::QKV_FLASH);
    if (c.fold_in || c.fold_out) { r.err = PIO_E_SHAPE; return r; }  // the fold is wired into the fused q|k|v form only
    // 0b: K / V projection fold of a single-head cross-attend over many keys (no pair core on the folded path).
    // (no mask vectors: a row without an attendable key must come out as `final.bias` alone --
    //  transformer_primitives.py:168-175 -- but the folded bias Wo bv + bo assumes sum(P) = 1)
    const int kvp = (a.k_in + 7) & ~7;
    const AttnCore kv_core = fused_core(kvp, kvp, c.Tk, false, false);
    if (!c.qcache && c.kv_fold_on && a.kq.w_hi && a.vo.w_hi && H == 1 && a.k_in == a.v_in && c.same_kv && a.dk == a.k_in &&
        a.dv == a.v_in && a.dkp == kvp && a.dvp == kvp && a.act_split != 1 && a.act_split != 3 && plain &&
        kv_core != AttnCore::MATERIALISED && a.kq.k == hdk && a.kq.n == kvp && a.vo.k == kvp &&
        (int64_t)c.B * c.Tk >= 4 * (int64_t)c.Bq * c.Tq) {
        r.out_pair = a.act_split == 2;
        return take(kv_core == AttnCore::XATTN ? AttnCore::KVFOLD_XATTN : AttnCore::KVFOLD_XTALL);
    }
    // 1/2: Q and K reading the same 16-bit input (self-attention) are ONE GEMM over the stacked [q rows | k rows] image
    r.fuse_qk = !c.qcache && a.qk.w_hi && !a.act_split && !c.q_bcast && c.same_qk && c.Tq == c.Tk && c.qk_adjacent &&
                a.qk.n == 2 * hdk;
    // 4-6 fused when nothing needs the score matrix (no full mask / bias / return_matrix) and the policy allows it
    if (fused_policy && !c.full_mask && !c.bias && !c.probs) {
        if (pair_core) {
            r.qk_pair = r.out_pair = true;
            return take(!mask_vectors && flash_pair_supported(a.dtype, a.dkp, a.dvp) ? AttnCore::PAIR_FLASH : AttnCore::PAIR_XATTN);
        }
        r.core = fused_core(a.dkp, a.dvp, c.Tk, mask_vectors, !single_core);
        r.out_pair = single_core;
    }
    if (r.core == AttnCore::MATERIALISED) {  // split activations travel as pairs through all three of its kernels
        r.need_scores = true;
        r.qk_pair = r.out_pair = a.act_split != 0;
    }
    return r;
}

// The same at plan time, when masks and pointers are unknown: the route of the plain call (no mask, nothing shared, no
// fold, no cache).  lean: the caller never passes a full mask / bias / probability output (the encoder / decoder
// stacks), so the plan carves score buffers only when that route needs them; xpart_bytes holds for every call of the shape.
// mask_vectors: the caller may still pass key / query mask vectors (the cross-attends): where such a call has no fused core
// of its own -- a pair request on the 128-wide head -- the plan keeps the score buffers for it.
inline AttnRoute attn_plan(const pio_attention_t &a, int B, int Bq, int Tq, int Tk, bool lean, bool mask_vectors = false) {
    AttnCall c = {};
    c.B = B; c.Bq = Bq; c.Tq = Tq; c.Tk = Tk;
    AttnRoute r = attn_route(a, c);
    if (mask_vectors) {
        c.kv_mask = true;
        const AttnRoute m = attn_route(a, c);
        r.need_scores = r.need_scores || m.need_scores;
        if (m.xpart_bytes > r.xpart_bytes) r.xpart_bytes = m.xpart_bytes;
    }
    if (!lean) r.need_scores = true;
    return r;
}

}  // namespace pio
