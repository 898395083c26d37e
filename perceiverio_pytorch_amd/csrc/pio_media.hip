// Media samples from fp32 model outputs on the device (pio_finish_media): what example_multimodal.py of the reference does
// on the host behind forward -- (np.clip(image, 0, 1) * 255).astype(np.uint8) frame by frame, (audio * 2**15).astype(np.int16)
// -- for an fp32 array read in place through four element strides, written as contiguous [n, h, w, C] uint8 / int16:
//
//   PIO_MEDIA_U8    v = x > 0 ? (x > 1 ? 1 : x) : 0       (-0 and NaN give 0: both comparisons are false for a NaN)
//                   y[.., reverse ? C - 1 - c : c] = (uint8) trunc(fmul_rn(v, 255))
//   PIO_MEDIA_S16   t = fmul_rn(x, 32768)  (a power of two: exact);  y = trunc(t) saturated to [-32768, 32767], NaN gives 0
//
// The product is written with the plain operator under this file's `fp contract(off)` pragma (see pio_flowviz.hip on the
// __f*_rn functions); nothing follows it that it could be contracted with, the pragma keeps that true.
//
// One launch.  The n*h*w pixels are ONE flat list: a workgroup owns FM_SPAN consecutive pixels, a lane FM_PX consecutive ones
// whatever rows or images they fall in, so a lane's 4 C bytes (8 C for int16) are whole dwords wherever y is 4-byte aligned,
// stored as the widest vectors y's alignment allows; only the last, partial group of the list is stored element by element,
// as is everything when y is not 4-byte aligned.  FLAT (sc == 1, sx == C, rows and images adjacent, x 16-byte aligned: what
// the models hand out) reads a lane's 4 C floats as C 16-byte loads; any other strides are walked pixel by pixel with carries.
// All offsets are 64-bit.  No atomics, no LDS, no workspace.
#include "pio_device.h"

#pragma clang fp contract(off)

namespace pio {

namespace {

constexpr int FM_THREADS = 256;
constexpr int FM_PX = 4;                       // consecutive pixels per lane
constexpr int FM_SPAN = FM_THREADS * FM_PX;    // pixels per workgroup

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct MediaArgs {
    const float *x;
    void *y;
    int64_t sn, sy, sx, sc;            // element strides of x[n, row, column, channel]
    int64_t total;                     // n * h * w
    uint32_t hw, h, w;
    int32_t reverse;
    int32_t y_align;                   // 1, 2, 4, 8 or 16: the largest of these that divides y's address
};

// the sample of one value, in the low 8 / 16 bits
template <int KIND>
__device__ __forceinline__ uint32_t fm_sample(float x) {
    if constexpr (KIND == PIO_MEDIA_U8) {
        const float v = x > 0.0f ? (x > 1.0f ? 1.0f : x) : 0.0f;
        return (uint32_t)(v * 255.0f);                      // in [0, 255]: the conversion truncates
    } else {
        const float t = x * 32768.0f;
        const float c = fminf(fmaxf(t, -32768.0f), 32767.0f);   // (a NaN comes out as -32768 here: replaced below)
        const int32_t v = t == t ? (int32_t)c : 0;
        return (uint32_t)v & 0xffffu;
    }
}

// W dwords to a 4-byte aligned address as the widest vectors `align` allows
template <int W>
__device__ __forceinline__ void fm_store(uint32_t *p, const uint32_t (&d)[W], int align) {
    if (W % 4 == 0 && align >= 16) {
#pragma unroll
        for (int i = 0; i + 3 < W; i += 4) {
            u32x4 v = {d[i], d[i + 1], d[i + 2], d[i + 3]};
            *reinterpret_cast<u32x4 *>(p + i) = v;
        }
    } else if (W % 2 == 0 && align >= 8) {
#pragma unroll
        for (int i = 0; i + 1 < W; i += 2) {
            u32x2 v = {d[i], d[i + 1]};
            *reinterpret_cast<u32x2 *>(p + i) = v;
        }
    } else {
#pragma unroll
        for (int i = 0; i < W; ++i) p[i] = d[i];
    }
}

template <int C, int KIND, bool FLAT>
__global__ __launch_bounds__(FM_THREADS) void finish_media_kernel(const MediaArgs a) {
    constexpr int E = FM_PX * C;                            // elements of a lane
    constexpr int BYTES = KIND == PIO_MEDIA_U8 ? 1 : 2;     // per sample
    constexpr int W = E * BYTES / 4;                        // dwords of a lane's full group
    const int64_t q = (int64_t)blockIdx.x * FM_SPAN + FM_PX * threadIdx.x;  // first pixel of this lane in the flat list
    if (q >= a.total) return;
    const bool full = q + FM_PX <= a.total;
    float v[E];
    if constexpr (FLAT) {
        const float *src = a.x + q * C;                     // 16 C q bytes behind a 16-byte aligned x
        if (full) {
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const f32x4 f = reinterpret_cast<const f32x4 *>(src)[i];
                v[4 * i] = f[0], v[4 * i + 1] = f[1], v[4 * i + 2] = f[2], v[4 * i + 3] = f[3];
            }
        } else {
#pragma unroll
            for (int j = 0; j < FM_PX; ++j)
#pragma unroll
                for (int c = 0; c < C; ++c) v[j * C + c] = q + j < a.total ? src[j * C + c] : 0.0f;
        }
    } else {
        // position of pixel q: image, row, column (the workgroup's first pixel by a 64-bit division, uniform; the lane's
        // from there in 32 bits: t < hw + FM_SPAN <= 2^31 - 1 + 1024)
        const int64_t q0 = (int64_t)blockIdx.x * FM_SPAN;
        const int64_t n0 = q0 / a.hw;
        const uint32_t t = (uint32_t)(q0 - n0 * a.hw) + FM_PX * threadIdx.x;
        const uint32_t dn = t / a.hw, p = t - dn * a.hw;
        int64_t n = n0 + dn;
        uint32_t r = p / a.w, col = p - r * a.w;
#pragma unroll
        for (int j = 0; j < FM_PX; ++j) {
            const bool in = q + j < a.total;
            const float *src = a.x + n * a.sn + (int64_t)r * a.sy + (int64_t)col * a.sx;
#pragma unroll
            for (int c = 0; c < C; ++c) v[j * C + c] = in ? src[c * a.sc] : 0.0f;
            if (++col == a.w) {
                col = 0;
                if (++r == a.h) r = 0, ++n;
            }
        }
    }
    uint32_t e[E];                                          // samples in output order
#pragma unroll
    for (int j = 0; j < FM_PX; ++j)
#pragma unroll
        for (int c = 0; c < C; ++c)
            e[j * C + c] = fm_sample<KIND>(KIND == PIO_MEDIA_U8 && a.reverse ? v[j * C + C - 1 - c] : v[j * C + c]);
    if (full && a.y_align >= 4) {
        uint32_t d[W];
#pragma unroll
        for (int i = 0; i < W; ++i) {
            if constexpr (KIND == PIO_MEDIA_U8)
                d[i] = e[4 * i] | (e[4 * i + 1] << 8) | (e[4 * i + 2] << 16) | (e[4 * i + 3] << 24);
            else
                d[i] = e[2 * i] | (e[2 * i + 1] << 16);
        }
        // E BYTES q = 4 W (q / 4) bytes behind y: a multiple of 4 W, so y's alignment (up to 4 W) carries over
        fm_store<W>(reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(a.y) + (int64_t)BYTES * C * q), d, a.y_align);
    } else {
#pragma unroll
        for (int j = 0; j < FM_PX; ++j)
            if (q + j < a.total) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    if constexpr (KIND == PIO_MEDIA_U8)
                        static_cast<uint8_t *>(a.y)[(q + j) * C + c] = (uint8_t)e[j * C + c];
                    else
                        static_cast<uint16_t *>(a.y)[(q + j) * C + c] = (uint16_t)e[j * C + c];
                }
            }
    }
}

template <int C, int KIND>
void fm_launch(const MediaArgs &a, bool flat, dim3 grid, hipStream_t s) {
    if (flat)
        hipLaunchKernelGGL((finish_media_kernel<C, KIND, true>), grid, dim3(FM_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL((finish_media_kernel<C, KIND, false>), grid, dim3(FM_THREADS), 0, s, a);
}

template <int KIND>
void fm_launch_c(const MediaArgs &a, int C, bool flat, dim3 grid, hipStream_t s) {
    switch (C) {
        case 1: fm_launch<1, KIND>(a, flat, grid, s); break;
        case 2: fm_launch<2, KIND>(a, flat, grid, s); break;
        case 3: fm_launch<3, KIND>(a, flat, grid, s); break;
        default: fm_launch<4, KIND>(a, flat, grid, s); break;
    }
}

}  // namespace

int finish_media_launch(const float *x, int64_t sn, int64_t sy, int64_t sx, int64_t sc, int n, int h, int w, int C, int kind,
                        int reverse, void *y, hipStream_t s) {
    if (!x || !y) return PIO_E_ARG;
    if (kind != PIO_MEDIA_U8 && kind != PIO_MEDIA_S16) return PIO_E_ARG;
    if (kind == PIO_MEDIA_S16 && reverse) return PIO_E_ARG;
    if (n < 1 || h < 1 || w < 1 || C < 1 || C > 4) return PIO_E_SHAPE;
    const int64_t hw = (int64_t)h * w;
    if (hw > 0x7fffffffLL) return PIO_E_SHAPE;  // (the position inside an image is 32-bit)
    const int64_t total = hw * n;               // < 2^62
    const int64_t groups = (total + FM_SPAN - 1) / FM_SPAN;
    if (groups > 0x7fffffffLL) return PIO_E_SHAPE;
    if ((uintptr_t)x & 3) return PIO_E_ALIGN;
    if (kind == PIO_MEDIA_S16 && ((uintptr_t)y & 1)) return PIO_E_ALIGN;
    MediaArgs a;
    a.x = x, a.y = y;
    a.sn = n > 1 ? sn : 0, a.sy = h > 1 ? sy : 0, a.sx = w > 1 ? sx : 0, a.sc = C > 1 ? sc : 0;
    a.total = total, a.hw = (uint32_t)hw, a.h = (uint32_t)h, a.w = (uint32_t)w;
    a.reverse = reverse != 0;
    const uintptr_t ya = (uintptr_t)y;
    a.y_align = ya & 1 ? 1 : ya & 2 ? 2 : ya & 4 ? 4 : ya & 8 ? 8 : 16;
    const bool flat = (C == 1 || sc == 1) && (w == 1 || sx == C) && (h == 1 || sy == (int64_t)w * C) &&
                      (n == 1 || sn == hw * C) && !((uintptr_t)x & 15);
    const dim3 grid((unsigned)groups);
    const double bytes = (double)total * C * (kind == PIO_MEDIA_U8 ? 5.0 : 6.0);
    ProfScope prof(PROF_LAYERNORM, 0.0, bytes, s);
    if (kind == PIO_MEDIA_U8)
        fm_launch_c<PIO_MEDIA_U8>(a, C, flat, grid, s);
    else
        fm_launch_c<PIO_MEDIA_S16>(a, C, flat, grid, s);
    return launch_status();
}

}  // namespace pio
