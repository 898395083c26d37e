// The steps the fused attention cores share (pio_flash.hip, pio_xattn.hip, pio_xtall.hip and the variants under
// tools/experiments): one spelling of each.  Device-only; an edit here is proved a no-op with tools/isa_diff.py.
// Conventions of all of them: a wave owns 32 query rows, lanes l and l + 32 (hh = l >> 5) hold the two halves of a
// query's column of the swapped products S^T = K Q^T and O^T = V^T P^T.
// (A helper is used only where it leaves the kernel's instruction stream as it was; the sites that keep their own
//  spelling for that reason say so.)
#pragma once
#include "pio_device.h"

namespace pio {

// max / sum of the two half-wave partials of a column, in both lanes
__device__ __forceinline__ float max_halves(float x) { return fmaxf(x, __shfl_xor(x, 32, 64)); }
__device__ __forceinline__ float sum_halves(float x) { return x + __shfl_xor(x, 32, 64); }

// Q fragments (B operand of S^T) of query row q, clamped to Tq - 1: the lane holds Qg[q][16 s + 8 hh + 0..7] for every
// k-step s.  Qg: the (batch, head) base.  Channels from `limit` on (a head narrower than the kernel's width) are zero.
template <int DT, int NQS>
__device__ __forceinline__ void load_q_frags(typename Op<DT>::V8 (&qf)[NQS], const typename Op<DT>::T *Qg, int q, int Tq,
                                             int64_t ldq, int hh, int limit = 16 * NQS) {
    typedef typename Op<DT>::V8 V8;
    q = q < Tq ? q : Tq - 1;
    const typename Op<DT>::T *qrow = Qg + (int64_t)q * ldq + 8 * hh;
    const V8 zero8 = {};
#pragma unroll
    for (int s = 0; s < NQS; ++s) qf[s] = (16 * s + 8 * hh < limit) ? *(const V8 *)(qrow + 16 * s) : zero8;
}

// Key bits: one 32-bit word per (sample, 32-key tile), bit j = key 32 tile + j is attendable.  Of a tile's word shifted
// for the lane half (word >> (8 hh)): accumulator element i of an S^T block is key 16 (i >> 3) + 8 hh + (i & 7) of the
// tile (K rows permuted: bits 2 and 3 swapped).
__device__ __forceinline__ bool key_bit(uint32_t bits, int i) { return (bits >> (16 * (i >> 3) + (i & 7))) & 1u; }

// Four consecutive accumulator elements acc[e0 .. e0 + 3], scaled, as 16-bit operands: o = round(v), l = round(v - o).
template <int DT, class A>
__device__ __forceinline__ void scaled_pair4(const A acc, int e0, float scale, typename Op<DT>::V4 &o,
                                             typename Op<DT>::V4 &l) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        typename Op<DT>::T h, r;
        cast_pair<DT>(acc[e0 + j] * scale, h, r);
        o[j] = h;
        l[j] = r;
    }
}

}  // namespace pio
