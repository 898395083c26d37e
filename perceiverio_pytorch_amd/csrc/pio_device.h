// Device-side primitives shared by the kernel translation units: one spelling of each helper the hand-counted waits and
// the hazard scan (tools/check_asm_hazards.py) depend on.  Device-only (pio_internal.h stays host-includable); an edit
// here is proved a no-op with tools/isa_diff.py.  The steps only the fused attention cores share: pio_attn_device.h.
#pragma once
#include <type_traits>

#include "pio_internal.h"

namespace pio {

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {  // compile-time loop: the index arrives as an integral_constant
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// The hi + lo pair of fp32 values in the operand type: h = round(x), l = round(x - h).  x: a float, or an ext_vector of
// 2 / 4 floats with h, l the operand vectors of the same width.
template <int DT, class FV, class OV>
__device__ __forceinline__ void cast_pair(const FV x, OV &h, OV &l) {
    if constexpr (std::is_same_v<FV, float>) {
        h = Op<DT>::from_f32(x);
        l = Op<DT>::from_f32(x - Op<DT>::to_f32(h));
    } else {
#pragma unroll
        for (int e = 0; e < (int)(sizeof(FV) / sizeof(float)); ++e) {
            h[e] = Op<DT>::from_f32(x[e]);
            l[e] = Op<DT>::from_f32(x[e] - Op<DT>::to_f32(h[e]));
        }
    }
}

// One LDS-DMA piece: every lane moves 16 bytes from its own global address to the wave's 1-KiB slice at `lds`.
__device__ __forceinline__ void lds_dma16(const void *src, void *lds) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                     (__attribute__((address_space(3))) void *)lds, 16, 0, 0);
}

// Per translation unit (a unit that uses neither emits neither).  g_zero16: the source of a 16-byte piece that lies
// outside its operand.  g_sink: stores of lanes outside the matrix go here, 16 bytes per lane, instead of being predicated
// off -- the store instruction is then ALWAYS issued, so the counted waits can count it.
__attribute__((unused)) static __device__ __attribute__((aligned(16))) uint32_t g_zero16[4] = {0, 0, 0, 0};
__attribute__((unused)) static __device__ __attribute__((aligned(16))) uint32_t g_sink[64 * 4];

// Every wait on an LDS-DMA stream is a COUNTED s_waitcnt vmcnt(n): n = the vector-memory operations this wave issued
// after the ones it needs (loads return in order; stores are counted too).  n: wave-uniform.
__device__ __forceinline__ void wait_vm_n(int n) {
#define PIO_W(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
    switch (n) {
        PIO_W(0) PIO_W(1) PIO_W(2) PIO_W(3) PIO_W(4) PIO_W(5) PIO_W(6) PIO_W(7) PIO_W(8) PIO_W(9) PIO_W(10)
        PIO_W(11) PIO_W(12) PIO_W(13) PIO_W(14) PIO_W(15) PIO_W(16) PIO_W(17) PIO_W(18) PIO_W(19)
        default: asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); break;
    }
#undef PIO_W
}

// The 32x32x16 MFMA as inline assembly with its register files pinned: left to the register allocator the accumulators
// wander between the two register files and some of them spill.  ACC_AGPR: the accumulator lives in AGPRs ("+a") and
// accumulates in place; else it lives in VGPRs, the B operand in AGPRs (B_AGPR: operands that are only ever MFMA
// operands) or VGPRs, and ZERO starts the sum (c = a b, SrcC = 0).  The compiler's hazard recogniser does not look inside
// an asm statement: where a VALU instruction reads what this MFMA wrote, or this MFMA reads an accumulator the VALU
// wrote, the kernel carries explicit s_nop padding (and the build scans for it).  (pio_gemm_wide.hip's MFMAs are plain
// asm of another instruction shape and stay there.)
template <int DT, bool ACC_AGPR, bool B_AGPR = false, bool ZERO = false>
__device__ __forceinline__ void mfma32_asm(f32x16 &c, typename Op<DT>::V8 a, typename Op<DT>::V8 b) {
    static_assert(!ACC_AGPR || (!B_AGPR && !ZERO), "an AGPR accumulator accumulates in place over VGPR operands");
    // (a macro: the constraint letters are part of the asm statement's string literals)
#define PIO_M(SRCC, CC, BC)                                                                                   \
    do {                                                                                                      \
        if constexpr (DT == PIO_DT_F16) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, " SRCC : CC(c) : "v"(a), BC(b)); \
        else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, " SRCC : CC(c) : "v"(a), BC(b));            \
    } while (0)
    if constexpr (ACC_AGPR) PIO_M("%0", "+a", "v");
    else if constexpr (ZERO && B_AGPR) PIO_M("0", "=&v", "a");
    else if constexpr (ZERO) PIO_M("0", "=&v", "v");
    else if constexpr (B_AGPR) PIO_M("%0", "+v", "a");
    else PIO_M("%0", "+v", "v");
#undef PIO_M
}

// Reads one accumulator element where it lives (an AGPR): without this the register allocator moves all 256 to VGPRs
// at the end of the K loop and a handful of address registers spill.
// acc_read: plain asm, the compiler may schedule it -- for accumulators of plain-asm MFMAs, read behind waits and a barrier.
__device__ __forceinline__ float acc_read(float a) {
    float v;
    asm("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(a));
    return v;
}
// acc_read_ordered: asm volatile, stays in program order among the volatile MFMAs (mfma32_asm) and their s_nop padding.
__device__ __forceinline__ float acc_read_ordered(float a) {
    float v;
    asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(a));
    return v;
}
// acc_write_ordered: the way back, `acc[i] = acc_write_ordered(v)` -- the value is written where the element lives.
__device__ __forceinline__ float acc_write_ordered(float v) {
    float a;
    asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(a) : "v"(v));
    return a;
}

// 1-D grid, remapped so that consecutive ids land on ONE XCD (ids are dealt round-robin over the 8 XCDs): neighbours that
// stream the same operand hit that XCD's L2.  Bijective; grids that are no multiple of 8 keep their order.
__device__ __forceinline__ int xcd_contiguous(int bid, int n) {
    if ((n & 7) == 0) bid = (bid & 7) * (n >> 3) + (bid >> 3);
    return bid;
}

}  // namespace pio
