// Optical-flow visualisation on the device (pio_flow_to_image): the Middlebury colour wheel of utils/flow_utils.py
// flow_to_image (flow_utils.py:91-153 of the reference) for a batch of fp32 flow fields read in place through four element
// strides, written as contiguous uint8 [b, h, w, 3].  Per image n and pixel (y, x), with (u, v) = flow[n, y, x, 0 / 1]:
//
//   1. clip (optional)   u = u < 0 ? +0 : u, then u = u > clip ? clip : u; v likewise (np.clip: -0 and NaN pass unchanged)
//   2. radius            rad = sqrt_rn(fadd_rn(fmul_rn(u, u), fmul_rn(v, v)));  rad_max[n] = max of rad over image n
//   3. normalise         s = fadd_rn(rad_max[n], 1e-5f);  un = fdiv_rn(u, s), vn = fdiv_rn(v, s);  radn = rad(un, vn)
//   4. wheel position    fk = (atan2f(-vn, -un) / pi + 1) / 2 * 54;  k0 = clamp(floor(fk), 0, 54);  f = fk - k0
//   5. colour, per ch    col = (1 - f) wheel[k0][ch] / 255 + f wheel[k0 + 1][ch] / 255   (entry 55 is entry 0)
//                        col = radn <= 1 ? 1 - radn (1 - col) : 0.75 col;  byte = floor(255 col), stored to ch or 2 - ch
//
// Steps 1 - 3 and the test radn <= 1 are the bits numpy computes: every operation is rounded on its own.  They are written
// with the plain operators under this file's `fp contract(off)` pragma, where `/` and sqrtf are the correctly rounded fp32
// forms, and NOT with the __f*_rn functions: those are inline functions of a header compiled with contraction allowed, so
// __fadd_rn(__fmul_rn(u, u), __fmul_rn(v, v)) comes out as a multiply and an FMA (seen in the assembly, and in one bit of
// rad_n on the device), and __fsqrt_rn is the 1-ulp native square root in this toolchain.  Steps 4 - 5 run in fp32 with the
// device library's accurate atan2f, which keeps the sign of zero: atan2(-0, -u) and atan2(+0, -u) select wheel entry 0 and
// entry 54.  A non-finite flow value is undefined in the reference; here k0 and the byte are clamped before they index or
// convert anything, nothing more.
//
// Two launches on the stream behind a memset of the b maxima words:
//   flow_radmax_kernel   rad of every pixel, reduced over wave and workgroup, ONE atomic max per workgroup and image on the
//                        bit pattern (non-negative floats order as unsigned integers, and a maximum does not depend on the
//                        order it is taken in: rad_max is exact and the same in every run)
//   flow_colour_kernel   steps 1 - 5, reading rad_max[n] from the word
// Both walk the b*h*w pixels as ONE flat list: a workgroup owns FV_SPAN consecutive pixels, a lane FV_PX consecutive ones,
// whatever rows or images they fall in (the position is advanced with carries), so a lane's 12 output bytes are three
// aligned dwords wherever `out` is 4-byte aligned; only the last, partial group of the list is stored byte by byte (as is
// everything when `out` is not aligned).  The wheel is built at compile time from the segment table and staged in LDS.
// All offsets are 64-bit.
#include "pio_device.h"

#pragma clang fp contract(off)

namespace pio {

namespace {

constexpr int FV_THREADS = 256;
constexpr int FV_PX = 4;                       // consecutive pixels per lane: 12 output bytes = three dwords
constexpr int FV_SPAN = FV_THREADS * FV_PX;    // pixels per workgroup
constexpr int FV_WHEEL = 55;

typedef float f32x2 __attribute__((ext_vector_type(2)));

// The colour wheel, r | g << 8 | b << 16 per entry; entry 55 repeats entry 0 so that k0 + 1 needs no wrap.
// Segments RY YG GC CB BM MR of 15, 6, 4, 11, 13, 6 entries: one channel at 255, one ramping floor(255 i / n) (rising in
// the even segments, falling from 255 in the odd ones), one at 0.
struct Wheel {
    uint32_t rgb[FV_WHEEL + 1];
};
constexpr Wheel make_wheel() {
    Wheel t{};
    const int seg[6] = {15, 6, 4, 11, 13, 6};
    int k = 0;
    for (int s = 0; s < 6; ++s) {
        const int full = ((s + 1) / 2) % 3, ramping = (1 + 2 * s) % 3;
        for (int i = 0; i < seg[s]; ++i, ++k) {
            const int ramp = 255 * i / seg[s];
            t.rgb[k] = (255u << (8 * full)) | ((uint32_t)(s % 2 ? 255 - ramp : ramp) << (8 * ramping));
        }
    }
    t.rgb[FV_WHEEL] = t.rgb[0];
    return t;
}
__constant__ const Wheel fv_wheel = make_wheel();

struct FlowVizArgs {
    const float *flow;
    uint8_t *out;
    uint32_t *radmax;                  // b words, bit patterns of non-negative floats
    int64_t sn, sy, sx, sc;            // element strides of flow[n, y, x, component]
    int64_t total;                     // b * h * w
    uint32_t hw, h, w;
    float clip;
    int32_t has_clip, bgr, out_dwords;  // out_dwords: out is 4-byte aligned
};

// position of a pixel of the flat list
struct Pos {
    int64_t n;
    uint32_t y, x;
};

// first pixel of this lane: q = blockIdx.x * FV_SPAN + FV_PX * threadIdx.x of the flat list (q may lie behind its end)
__device__ __forceinline__ Pos fv_first(const FlowVizArgs &a, int64_t &q) {
    const int64_t q0 = (int64_t)blockIdx.x * FV_SPAN;  // uniform
    const int64_t n0 = q0 / a.hw;
    const uint32_t t = (uint32_t)(q0 - n0 * a.hw) + FV_PX * threadIdx.x;  // < hw + FV_SPAN <= 2^31 - 1 + 1024
    const uint32_t dn = t / a.hw, p = t - dn * a.hw;
    q = q0 + FV_PX * threadIdx.x;
    Pos r;
    r.n = n0 + dn, r.y = p / a.w, r.x = p - r.y * a.w;
    return r;
}

__device__ __forceinline__ void fv_next(const FlowVizArgs &a, Pos &r) {
    if (++r.x == a.w) {
        r.x = 0;
        if (++r.y == a.h) r.y = 0, ++r.n;
    }
}

// np.clip(x, 0, c) as numpy's loops take it: a bound replaces x only where x lies strictly beyond it, so -0 stays -0 (and
// selects wheel entry 54, not 0, where it is v) and a NaN stays
__device__ __forceinline__ float fv_clip(float x, float c) {
    x = x < 0.0f ? 0.0f : x;
    return x > c ? c : x;
}

// steps 1 of a pixel: (u, v) as read (PAIR: one 8-byte load) and clipped
template <bool PAIR>
__device__ __forceinline__ void fv_load(const FlowVizArgs &a, const Pos &r, float &u, float &v) {
    const float *src = a.flow + r.n * a.sn + (int64_t)r.y * a.sy + (int64_t)r.x * a.sx;
    if constexpr (PAIR) {
        const f32x2 f = *reinterpret_cast<const f32x2 *>(src);
        u = f[0], v = f[1];
    } else {
        u = src[0], v = src[a.sc];
    }
    if (a.has_clip) u = fv_clip(u, a.clip), v = fv_clip(v, a.clip);
}

__device__ __forceinline__ float fv_rad(float u, float v) {
    return sqrtf(u * u + v * v);  // two products, one sum, one correctly rounded root (see the head of the file)
}

__device__ __forceinline__ uint32_t fv_wave_max(uint32_t m) {
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
    return m;
}

// PAIR: sc == 1, every other stride even, flow 8-byte aligned
template <bool PAIR>
__global__ __launch_bounds__(FV_THREADS) void flow_radmax_kernel(const FlowVizArgs a) {
    __shared__ uint32_t part[FV_THREADS / 64];
    int64_t q;
    Pos r = fv_first(a, q);
    // images of the first and the last pixel of this workgroup (uniform): equal in all but the workgroups that straddle
    const int64_t qa = (int64_t)blockIdx.x * FV_SPAN;
    const int64_t qb = min(qa + FV_SPAN, a.total) - 1;
    const int64_t na = qa / a.hw, nb = qb / a.hw;
    if (na == nb) {
        uint32_t m = 0;
        for (int j = 0; j < FV_PX; ++j) {
            if (q + j < a.total) {
                float u, v;
                fv_load<PAIR>(a, r, u, v);
                m = max(m, __float_as_uint(fv_rad(u, v)));
            }
            fv_next(a, r);
        }
        m = fv_wave_max(m);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int i = 1; i < FV_THREADS / 64; ++i) m = max(m, part[i]);
            atomicMax(a.radmax + na, m);
        }
    } else {
        // a workgroup that holds the end of one image and the start of the next (or several tiny images): every lane
        // merges its own pixels into their own image's word
        for (int j = 0; j < FV_PX; ++j) {
            if (q + j < a.total) {
                float u, v;
                fv_load<PAIR>(a, r, u, v);
                atomicMax(a.radmax + r.n, __float_as_uint(fv_rad(u, v)));
            }
            fv_next(a, r);
        }
    }
}

// steps 3 - 5 of a pixel: its three bytes in output order, byte 0 lowest
__device__ __forceinline__ uint32_t fv_colour(const uint32_t *wheel, float u, float v, float s, int bgr) {
    const float un = u / s, vn = v / s;
    const float radn = fv_rad(un, vn);
    const float a = atan2f(-vn, -un) / 3.14159274f;
    const float fk = (a + 1.0f) / 2.0f * (float)(FV_WHEEL - 1);
    const float fl = floorf(fk);
    const int k0 = (int)fminf(fmaxf(fl, 0.0f), (float)(FV_WHEEL - 1));  // clamped as a float: fmaxf drops a NaN
    const float f = fk - fl;
    const uint32_t w0 = wheel[k0], w1 = wheel[k0 + 1];
    uint32_t px = 0;
    for (int ch = 0; ch < 3; ++ch) {
        const float c0 = (float)((w0 >> (8 * ch)) & 255u), c1 = (float)((w1 >> (8 * ch)) & 255u);
        // (1 - f) c0 / 255 + f c1 / 255 as one interpolation: c1 - c0 is exact, and equal entries give c0 / 255 exactly
        float col = (c0 + f * (c1 - c0)) / 255.0f;
        col = radn <= 1.0f ? 1.0f - radn * (1.0f - col) : col * 0.75f;
        const float byte = fminf(fmaxf(floorf(255.0f * col), 0.0f), 255.0f);  // (fmaxf drops a NaN)
        px |= (uint32_t)byte << (8 * (bgr ? 2 - ch : ch));
    }
    return px;
}

template <bool PAIR>
__global__ __launch_bounds__(FV_THREADS) void flow_colour_kernel(const FlowVizArgs a) {
    __shared__ uint32_t wheel[64];
    if (threadIdx.x <= FV_WHEEL) wheel[threadIdx.x] = fv_wheel.rgb[threadIdx.x];
    __syncthreads();
    int64_t q;
    Pos r = fv_first(a, q);
    if (q >= a.total) return;
    uint32_t px[FV_PX];
    for (int j = 0; j < FV_PX; ++j) {
        px[j] = 0;
        if (q + j < a.total) {
            float u, v;
            fv_load<PAIR>(a, r, u, v);
            const float s = __uint_as_float(a.radmax[r.n]) + 1e-5f;
            px[j] = fv_colour(wheel, u, v, s, a.bgr);
        }
        fv_next(a, r);
    }
    uint8_t *o = a.out + 3 * q;
    if (a.out_dwords && q + FV_PX <= a.total) {
        uint32_t *o4 = reinterpret_cast<uint32_t *>(o);  // 3 q = 12 (q / 4): a multiple of 4
        o4[0] = px[0] | (px[1] << 24);
        o4[1] = (px[1] >> 8) | (px[2] << 16);
        o4[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
        for (int j = 0; j < FV_PX; ++j)
            if (q + j < a.total) {
                o[3 * j] = (uint8_t)px[j];
                o[3 * j + 1] = (uint8_t)(px[j] >> 8);
                o[3 * j + 2] = (uint8_t)(px[j] >> 16);
            }
    }
}

}  // namespace

int flow_to_image_launch(const float *flow, int64_t sn, int64_t sy, int64_t sx, int64_t sc, int b, int h, int w,
                         float clip_flow, int has_clip, int bgr, uint8_t *out, uint32_t *rad_max, hipStream_t s) {
    if (!flow || !out || !rad_max) return PIO_E_ARG;
    if (b < 1 || h < 1 || w < 1) return PIO_E_SHAPE;
    const int64_t hw = (int64_t)h * w;
    if (hw > 0x7fffffffLL) return PIO_E_SHAPE;  // (the position inside an image is 32-bit)
    const int64_t total = hw * b;               // < 2^62
    const int64_t groups = (total + FV_SPAN - 1) / FV_SPAN;
    if (groups > 0x7fffffffLL) return PIO_E_SHAPE;
    if (((uintptr_t)flow | (uintptr_t)rad_max) & 3) return PIO_E_ALIGN;
    FlowVizArgs a;
    a.flow = flow, a.out = out, a.radmax = rad_max;
    a.sn = b > 1 ? sn : 0, a.sy = h > 1 ? sy : 0, a.sx = w > 1 ? sx : 0, a.sc = sc;
    a.total = total, a.hw = (uint32_t)hw, a.h = (uint32_t)h, a.w = (uint32_t)w;
    a.clip = clip_flow, a.has_clip = has_clip != 0, a.bgr = bgr != 0, a.out_dwords = !((uintptr_t)out & 3);
    const bool pair = sc == 1 && !((a.sn | a.sy | a.sx) & 1) && !((uintptr_t)flow & 7);
    if (hipMemsetAsync(rad_max, 0, sizeof(uint32_t) * (size_t)b, s) != hipSuccess) return PIO_E_LAUNCH;
    const dim3 grid((unsigned)groups);
    {
        ProfScope prof(PROF_LAYERNORM, 0.0, 8.0 * (double)total, s);
        if (pair)
            hipLaunchKernelGGL(flow_radmax_kernel<true>, grid, dim3(FV_THREADS), 0, s, a);
        else
            hipLaunchKernelGGL(flow_radmax_kernel<false>, grid, dim3(FV_THREADS), 0, s, a);
    }
    ProfScope prof(PROF_LAYERNORM, 0.0, 11.0 * (double)total, s);
    if (pair)
        hipLaunchKernelGGL(flow_colour_kernel<true>, grid, dim3(FV_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL(flow_colour_kernel<false>, grid, dim3(FV_THREADS), 0, s, a);
    return launch_status();
}

}  // namespace pio
