// Device-side primitives shared by the kernel translation units: one spelling of each helper the hand-counted waits and
// the hazard scan (tools/check_asm_hazards.py) depend on.  Device-only (pio_internal.h stays host-includable); an edit
// here is proved a no-op with tools/isa_diff.py.
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

// The 32x32x16 MFMA as inline assembly with its accumulator pinned to AGPRs ("+a"), accumulating in place: left to the
// register allocator the accumulators wander between the two register files and some of them spill.  The compiler's
// hazard recogniser does not look inside an asm statement: where a VALU instruction reads what this MFMA wrote, or this
// MFMA reads an accumulator the VALU wrote, the kernel carries explicit s_nop padding (and the build scans for it).
template <int DT>
__device__ __forceinline__ void mfma32_agpr(f32x16 &c, typename Op<DT>::V8 a, typename Op<DT>::V8 b) {
    if constexpr (DT == PIO_DT_F16) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
    else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}

// Reads one accumulator element where it lives (an AGPR): without this the register allocator moves all 256 to VGPRs
// at the end of the K loop and a handful of address registers spill.
// acc_read: plain asm, the compiler may schedule it -- for accumulators of plain-asm MFMAs, read behind waits and a barrier.
__device__ __forceinline__ float acc_read(float a) {
    float v;
    asm("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(a));
    return v;
}
// acc_read_ordered: asm volatile, stays in program order among the volatile MFMAs (mfma32_agpr) and their s_nop padding.
__device__ __forceinline__ float acc_read_ordered(float a) {
    float v;
    asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(a));
    return v;
}

}  // namespace pio
