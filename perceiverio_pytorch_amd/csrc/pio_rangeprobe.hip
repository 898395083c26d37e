// Range probe: max |x| of one 16-bit operand buffer -- does a checkpoint's activations fit fp16 (65 504), or does a part
// of the model need the bf16 policies?  A calibration tool (pio_absmax16 / pio_range_probe_begin, pio_capi.hip): never on
// the product path, no throughput target beyond "one streaming read".
//
// absmax16_kernel: every row is cut into SLOTS of 8 elements on 16-byte ADDRESS boundaries (slot 0 starts at the
// boundary at or in front of the row's first element).  A slot that lies wholly inside [0, cols) is one 16-byte load; the
// (at most two) slots of a row that straddle its first or last element are read element by element, only the elements
// inside the row: nothing in front of the row, behind column cols - 1 or behind the last row is ever read, whatever the
// base alignment and pitch.  Slots are numbered row-major over (batch, row, slot) and walked with a grid-stride loop by
// a grid bounded by the CU count; each lane keeps the maximum of |x| (NaN and inf both count as +inf), the workgroup
// reduces it (shuffles, then LDS) and one lane merges it into the caller's word with one atomicMax on the bit pattern
// (non-negative floats order like unsigned integers; +inf, 0x7f800000, is the largest of them).
#include "pio_internal.h"

#include <vector>

namespace pio {

namespace {

constexpr int R_WAVES = 4;         // waves per workgroup
constexpr int R_WG_PER_CU = 8;     // grid bound: workgroups per CU

template <int DT>
__device__ __forceinline__ float abs_or_inf(typename Op<DT>::T x) {
    float v = fabsf(Op<DT>::to_f32(x));
    if (!(v <= 3.4028234664e38f)) v = __builtin_inff();  // NaN or inf: reported, not dropped
    return v;
}

// slots_per_row: upper bound of the slots one row can touch, (cols + 7 + 7) / 8 -- a slot index at or behind the row's own
// count is an empty slot.  single_row: rows * batch == 1 (the host collapses contiguous buffers into one row): no division.
// stride_b == 0: one batch.
template <int DT>
__global__ __launch_bounds__(64 * R_WAVES) void absmax16_kernel(const typename Op<DT>::T *__restrict__ x, int64_t rows,
                                                               int64_t cols, int64_t ld, int64_t stride_b,
                                                               int64_t slots_per_row, int64_t total_slots, int single_row,
                                                               unsigned int *__restrict__ out) {
    typedef typename Op<DT>::T T;
    typedef typename Op<DT>::V8 V8;
    __shared__ float wave_max[R_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float m = 0.f;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total_slots; t += step) {
        int64_t b = 0, r = 0, slot = t;
        if (!single_row) {
            r = t / slots_per_row;
            slot = t - r * slots_per_row;
            if (stride_b) {  // (0: one batch -- the host passes it so whenever a single batch is read)
                b = r / rows;
                r -= b * rows;
            }
        }
        const T *p = x + b * stride_b + r * ld;            // the row's first element
        const int64_t mis = (int64_t)(((uintptr_t)p & 15) >> 1);  // elements between the 16-byte boundary and p
        const int64_t e0 = slot * 8 - mis;                 // first element of the slot, relative to p (may be < 0)
        if (e0 >= cols) continue;                          // an empty slot behind the row's last one
        if (e0 >= 0 && e0 + 8 <= cols) {
            const V8 v = *(const V8 *)(p + e0);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float a = abs_or_inf<DT>(v[i]);
                m = a > m ? a : m;
            }
        } else {
            const int64_t lo = e0 < 0 ? 0 : e0, hi = e0 + 8 < cols ? e0 + 8 : cols;
            for (int64_t e = lo; e < hi; ++e) {
                const float a = abs_or_inf<DT>(p[e]);
                m = a > m ? a : m;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float o = __shfl_xor(m, off, 64);
        m = o > m ? o : m;
    }
    if (lane == 0) wave_max[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < R_WAVES; ++w) m = wave_max[w] > m ? wave_max[w] : m;
        if (m > 0.f) atomicMax(out, __float_as_uint(m));
    }
}

struct RangeRec {
    int32_t part, kind;
};
struct RangeState {
    bool on = false;
    float *records = nullptr;
    int max_records = 0, n = 0, part = 0;
    std::vector<RangeRec> labels;  // (part, kind) of the recorded calls, in call order
} g_range;

}  // namespace

int absmax16_launch(int dtype, const void *x, int64_t rows, int64_t cols, int64_t ld, int64_t batch, int64_t stride_b,
                    float *absmax, hipStream_t s) {
    if (dtype != PIO_DT_F16 && dtype != PIO_DT_BF16) return PIO_E_ARG;
    if (!x || !absmax) return PIO_E_ARG;
    if (((uintptr_t)x & 1) || ((uintptr_t)absmax & 3)) return PIO_E_ALIGN;
    if (rows < 0 || cols < 0 || batch < 0 || ld < 0 || stride_b < 0) return PIO_E_SHAPE;
    if (rows > 1 && cols > ld) return PIO_E_SHAPE;
    if (rows == 0 || cols == 0 || batch == 0) return PIO_OK;  // nothing to read: the word keeps its value
    if (stride_b == 0) batch = 1;                             // one batch is read
    // contiguous pieces become one long row: batches that follow each other, rows without slack columns
    if (batch > 1 && stride_b == rows * ld) {
        rows *= batch;
        batch = 1;
    }
    if (batch == 1) stride_b = 0;
    if (rows > 1 && cols == ld && batch == 1) {
        cols *= rows;
        rows = 1;
    }
    const int64_t slots_per_row = (cols + 14) / 8, nrows = rows * batch;
    if (slots_per_row > (int64_t)1 << 40 || nrows > (int64_t)1 << 40 ||
        (double)slots_per_row * (double)nrows > 9.0e18)
        return PIO_E_SHAPE;
    const int64_t total = slots_per_row * nrows;
    const int threads = 64 * R_WAVES;
    int64_t nwg = (total + threads - 1) / threads;
    const int64_t cap = (int64_t)cu_budget() * R_WG_PER_CU;
    if (nwg > cap) nwg = cap;
    const dim3 grid((unsigned)nwg), block(threads);
    const int single = nrows == 1 ? 1 : 0;
    if (dtype == PIO_DT_F16)
        absmax16_kernel<PIO_DT_F16><<<grid, block, 0, s>>>((const _Float16 *)x, rows, cols, ld, stride_b, slots_per_row, total,
                                                           single, (unsigned int *)absmax);
    else
        absmax16_kernel<PIO_DT_BF16><<<grid, block, 0, s>>>((const __bf16 *)x, rows, cols, ld, stride_b, slots_per_row, total,
                                                            single, (unsigned int *)absmax);
    return launch_status();
}

bool range_probe_active() { return g_range.on; }

int range_probe_record(int kind, int dtype, const void *x, int64_t rows, int64_t cols, int64_t ld, int64_t batch,
                       int64_t stride_b, hipStream_t s) {
    const int idx = g_range.n++;
    if (idx >= g_range.max_records) return PIO_OK;  // counted, not recorded
    g_range.labels.push_back({g_range.part, kind});
    return absmax16_launch(dtype, x, rows, cols, ld, batch, stride_b, g_range.records + idx, s);
}

int range_probe_begin(float *records, int max_records) {
    if (!records || max_records <= 0 || ((uintptr_t)records & 3)) return PIO_E_ARG;
    g_range = RangeState();
    g_range.labels.reserve((size_t)max_records);
    g_range.records = records;
    g_range.max_records = max_records;
    g_range.on = true;
    return PIO_OK;
}

int range_probe_mark(int part) {
    const int prev = g_range.part;
    if (g_range.on) g_range.part = part;
    return prev;
}

int range_probe_end(int32_t *parts, int32_t *kinds, int cap) {
    const int n = g_range.on ? g_range.n : 0;
    const int have = (int)g_range.labels.size();
    for (int i = 0; i < have && i < cap; ++i) {
        if (parts) parts[i] = g_range.labels[i].part;
        if (kinds) kinds[i] = g_range.labels[i].kind;
    }
    g_range = RangeState();
    return n;
}

}  // namespace pio
