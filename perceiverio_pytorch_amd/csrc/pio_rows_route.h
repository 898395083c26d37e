// Routing of the row primitives (host only, plain C++17: no HIP, no environment, no state): which kernel a
// layernorm_cast / softmax_rows launch goes to and on how many workgroups, and the shape / alignment refusals of
// layernorm_cast_cat.  pio_elementwise.hip checks its pointers for NULL, fills the call struct, and launches what the
// route names; tests/test_rows_route.py checks it on the CPU against the case tables of tests/primitive_cases.py.
// Addresses arrive as their low four bits (rows_addr_bits; a NULL optional pointer counts as aligned).
#pragma once
#include <stdint.h>

#include "../../include/pio_hip.h"

namespace pio {

inline unsigned rows_addr_bits(const void *p) { return (unsigned)((uintptr_t)p & 15); }
inline bool rows_dtype_ok(int dtype) { return dtype == PIO_DT_F16 || dtype == PIO_DT_BF16; }
// one wave per row, four rows a workgroup
inline unsigned rows_blocks4(int64_t rows) { return (unsigned)((rows + 3) / 4); }

// ---- layernorm_cast -------------------------------------------------------------------------------------------------
enum class LnKind {
    NONE,        // (an error)
    REG4,        // layernorm_cast_reg_kernel<., ., nv>: the row in registers, float4 lanes, nv = 4 (c_pad <= 1024) or 8
    REG2,        // layernorm_cast_reg2_kernel: the row in registers, float2 lanes (nv = 16)
    GEN_VEC,     // layernorm_cast_kernel<., true, .>: three passes, float4 lanes (rows wider than 2048)
    GEN_SCALAR,  // layernorm_cast_kernel<., false, .>: three passes, any width and alignment
};

struct LnCall {
    int B, T, C, c_pad;
    int64_t stride_b, stride_t;
    bool has_ln;
    int dtype;
    unsigned x, y, y_lo, gamma, beta;  // low four address bits
};

struct LnRoute {
    int err;         // PIO_OK or the PIO_E_* code of the refusal
    LnKind kind;
    int nv;          // vectors per lane of the register kernels (0: three-pass kernel)
    bool even_rows;  // REG4 only: rows evenly spaced (stride_b == T * stride_t), the kernel gets T = 0 and skips its division
    unsigned blocks;
};

inline LnRoute ln_route(const LnCall &c) {
    if (c.B <= 0 || c.T <= 0 || c.C <= 0 || c.c_pad < c.C || (c.c_pad % 8)) return {PIO_E_SHAPE, LnKind::NONE, 0, false, 0};
    if (!rows_dtype_ok(c.dtype)) return {PIO_E_ARG, LnKind::NONE, 0, false, 0};
    const unsigned blocks = rows_blocks4((int64_t)c.B * c.T);
    // float4 loads / 8-byte stores, float2 loads / 4-byte stores
    const bool vec = (c.C % 4 == 0) && !(c.x & 15) && (c.stride_b % 4 == 0) && (c.stride_t % 4 == 0) && !(c.y & 7) &&
                     !(c.y_lo & 7) && (!c.has_ln || (!(c.gamma & 15) && !(c.beta & 15)));
    const bool vec2 = (c.C % 2 == 0) && !(c.x & 7) && (c.stride_b % 2 == 0) && (c.stride_t % 2 == 0) && !(c.y & 3) &&
                      !(c.y_lo & 3) && (!c.has_ln || (!(c.gamma & 7) && !(c.beta & 7)));
    if (vec && c.c_pad <= 2048)
        return {PIO_OK, LnKind::REG4, c.c_pad <= 1024 ? 4 : 8, c.B == 1 || c.stride_b == (int64_t)c.T * c.stride_t, blocks};
    if (vec2 && c.c_pad <= 2048) return {PIO_OK, LnKind::REG2, 16, false, blocks};
    return {PIO_OK, vec ? LnKind::GEN_VEC : LnKind::GEN_SCALAR, 0, false, blocks};
}

// ---- layernorm_cast_cat: one kernel (float2 lanes over [x1 row | x2 row]); PIO_OK or the refusal ---------------------
struct LnCatCall {
    int B1, T1, C1, B2, T2, C2, ln_c, c_pad;
    int64_t sb1, st1, sb2, st2;
    int dtype;
    unsigned x1, x2, y, y_lo, gamma, beta;  // low four address bits
};

inline int ln_cat_check(const LnCatCall &c) {
    const int C = c.C1 + c.C2;
    if (c.B1 <= 0 || c.T1 <= 0 || c.C1 <= 0 || c.C2 <= 0 || c.T2 != c.T1 || (c.B2 != c.B1 && c.B2 != 1) || c.ln_c != C ||
        c.c_pad < C || (c.c_pad % 8) || c.c_pad > 2048 || (c.C1 & 1) || (c.C2 & 1))
        return PIO_E_SHAPE;
    if ((c.x1 & 7) || (c.x2 & 7) || (c.sb1 & 1) || (c.st1 & 1) || (c.sb2 & 1) || (c.st2 & 1) || (c.y & 3) || (c.y_lo & 3) ||
        (c.gamma & 7) || (c.beta & 7))
        return PIO_E_ALIGN;
    return rows_dtype_ok(c.dtype) ? PIO_OK : PIO_E_ARG;
}

// ---- softmax_rows ---------------------------------------------------------------------------------------------------
enum class SoftmaxKind {
    NONE,    // (an error)
    REG,     // softmax_rows_reg_kernel<., nv4, plain>: one wave per row, the row in registers (ldp <= 256 nv4)
    GEN_W1,  // softmax_rows_kernel<., 1>: one wave per row, three passes (Tk <= 2048)
    GEN_W4,  // softmax_rows_kernel<., 4>: one 256-thread workgroup per row
};

struct SoftmaxCall {
    int B, H, Tq, Tk;
    int64_t lds, ldp;
    int dtype;
    bool has_P_lo, has_bias, has_probs, has_kv_mask, has_q_mask, has_full_mask;
    unsigned S, P, P_lo, bias, probs, kv_mask, full_mask;  // low four address bits
};

struct SoftmaxRoute {
    int err;
    SoftmaxKind kind;
    int nv4;     // float4 per lane of the register kernel: 2 / 8 / 16 (0: three-pass kernel)
    bool plain;  // no mask, bias, lo or probability output
    unsigned blocks;
};

inline SoftmaxRoute softmax_route(const SoftmaxCall &c) {
    if (c.B <= 0 || c.H <= 0 || c.Tq <= 0 || c.Tk <= 0 || c.ldp < c.Tk || c.lds < c.Tk)
        return {PIO_E_SHAPE, SoftmaxKind::NONE, 0, false, 0};
    if (!rows_dtype_ok(c.dtype)) return {PIO_E_ARG, SoftmaxKind::NONE, 0, false, 0};
    const int64_t rows = (int64_t)c.B * c.H * c.Tq;
    const bool plain = !c.has_kv_mask && !c.has_q_mask && !c.has_full_mask && !c.has_bias && !c.has_P_lo && !c.has_probs;
    const bool vec4 = (c.Tk % 4 == 0) && (c.ldp % 4 == 0) && (c.lds % 4 == 0) && !(c.S & 15) && !(c.P & 7) && !(c.P_lo & 7) &&
                      !(c.bias & 15) && !(c.probs & 15) && !(c.kv_mask & 3) && !(c.full_mask & 3);
    if (vec4 && c.ldp <= 16 * 256)
        return {PIO_OK, SoftmaxKind::REG, c.ldp <= 2 * 256 ? 2 : c.ldp <= 8 * 256 ? 8 : 16, plain, rows_blocks4(rows)};
    if (c.Tk <= 2048) return {PIO_OK, SoftmaxKind::GEN_W1, 0, plain, rows_blocks4(rows)};
    return {PIO_OK, SoftmaxKind::GEN_W4, 0, plain, (unsigned)rows};
}

}  // namespace pio
