// The step in front of the models in one pass (pio_prepare_images): crop, bilinear resize with or without antialiasing,
// channel reversal and (v - mean) / std of a list of uint8 / fp32 images of any sizes and layouts, read in place, into one
// fp32 [N, C, oh, ow] batch.  The definition (weights as ratios of small integers, one fp32 division each; fmaf chains in
// ascending order) is in include/pio_hip.h; ip_taps below is its only statement in code, shared by host and device.
//
// One workgroup (four waves) owns IP_BH output rows x IP_BW output columns x all C channels of one image:
//   * wave 0 makes the tile's IP_BW column weight lists, lanes 0 .. IP_BH - 1 of wave 1 the band's row weight lists, once,
//     into LDS (wx tap-major: lanes read consecutive words) -- no weight is recomputed per source row, tap or channel;
//   * the source rows the band needs go through the horizontal pass IP_SR at a time into LDS (fp32 [row][channel][column]):
//     wave = source row, lane = output column, all C channels of a pixel together (one 4- or 16-byte load when the four
//     channels of a pixel are contiguous and aligned, single elements otherwise); a row no output row of the band has a
//     tap on is skipped, and a row enters LDS once per tile;
//   * the vertical pass runs from LDS into at most IP_BH * 4 / 4 accumulators per lane (wave w owns the (row, channel)
//     pairs w, w + 4, ..), rows ascending across the chunks: one fixed chain per output value;
//   * stores are coalesced along ox, one wave instruction per (row, channel).
// LDS: wx TX x 64, wy 8 x TY, the lists' bounds, and 24 x C x 64 staged values -- at most 21 + 2.6 + 0.6 + 24.6 KB at the
// reduction cap (PIO_IMAGE_MAX_REDUCTION = 40: 82 taps), 19 KB for 3 channels at the usual 5 taps, so three to eight
// workgroups share a CU's 160 KB.  All offsets are 64-bit; the source table travels by value in the kernel arguments.
#include "pio_internal.h"

#pragma clang fp contract(off)

namespace pio {

namespace {

constexpr int IP_BH = 8;    // output rows per workgroup
constexpr int IP_BW = 64;   // output columns per workgroup: one per lane
constexpr int IP_SR = 24;   // source rows per staged chunk
constexpr int IP_ACC = IP_BH * 4 / 4;                       // (row, channel) pairs per wave: C <= 4, four waves
constexpr int IP_MAX_TAPS = 2 * PIO_IMAGE_MAX_REDUCTION + 2;

// the taps of output index i: crop indices [lo, lo + n), n >= 1, lo + n <= in
__host__ __device__ inline void ip_taps(int i, int in, int out, bool aa, int &lo, int &n) {
    const int c2 = (2 * i + 1) * in;
    if (aa) {
        const int d = 2 * (in > out ? in : out);
        const int a = c2 - d + out, b = c2 + d + out;
        lo = a > 0 ? a / (2 * out) : 0;
        int hi = b / (2 * out);
        hi = hi < in ? hi : in;
        n = hi - lo;
    } else {
        const int q = c2 > out ? c2 - out : 0;
        lo = q / (2 * out);
        lo = lo < in - 1 ? lo : in - 1;
        n = lo + 1 < in ? 2 : 1;
    }
}

// the n weights of output index i into w[0], w[stride], ..
__device__ inline void ip_weights(int i, int in, int out, bool aa, int lo, int n, float *w, int stride) {
    const int c2 = (2 * i + 1) * in;
    if (aa) {
        const float d = (float)(2 * (in > out ? in : out));
        float sum = 0.0f;
        for (int t = 0; t < n; ++t) {
            const int num = (2 * (lo + t) + 1) * out - c2;
            const float r = fmaxf(0.0f, 1.0f - (float)(num < 0 ? -num : num) / d);
            w[t * stride] = r;
            sum = sum + r;
        }
        for (int t = 0; t < n; ++t) w[t * stride] = w[t * stride] / sum;
    } else {
        const int q = c2 > out ? c2 - out : 0;
        const float l = (float)(q - 2 * out * lo) / (float)(2 * out);
        if (n == 2) {
            w[0] = 1.0f - l;
            w[stride] = l;
        } else {
            w[0] = (1.0f - l) + l;
        }
    }
}

struct IpSrc {
    const void *base;  // the crop box's first element of the descriptor's first image
    int64_t sb, sc, sy, sx;
    int32_t dtype, img0, ch, cw, vec4;  // img0: first output image; vec4: a pixel's four channels are one aligned load
};
struct IpArgs {
    IpSrc src[PIO_MAX_IMAGE_SOURCES];
    float mean[4], std[4];
    int32_t nsrc, C, oh, ow, aa, reverse, TX, TY, bands, tiles;
};

__global__ __launch_bounds__(256) void prepare_images_kernel(const IpArgs a, float *__restrict__ out, int64_t out_sb) {
    extern __shared__ __align__(16) float ip_lds[];
    // [wx: TX x IP_BW] [wy: IP_BH x TY] [xlo, xn: IP_BW each] [ylo, yn: IP_BH each] [h: IP_SR x C x IP_BW]
    float *wx = ip_lds;
    float *wy = wx + a.TX * IP_BW;
    int *xlo = reinterpret_cast<int *>(wy + IP_BH * a.TY);
    int *xn = xlo + IP_BW;
    int *ylo = xn + IP_BW;
    int *yn = ylo + IP_BH;
    float *h = reinterpret_cast<float *>(yn + IP_BH);

    const int per = a.bands * a.tiles;
    const int g = blockIdx.x / per, rest = blockIdx.x - g * per;
    const int band = rest / a.tiles, tile = rest - band * a.tiles;
    int si = 0;
    for (int i = 1; i < a.nsrc; ++i)
        if (g >= a.src[i].img0) si = i;
    const IpSrc &s = a.src[si];
    const int C = a.C, oh = a.oh, ow = a.ow, ch = s.ch, cw = s.cw;
    const bool aa = a.aa != 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int oy0 = band * IP_BH, nb = min(IP_BH, oh - oy0);
    const int ox = tile * IP_BW + lane;

    if (wave == 0) {
        int lo = 0, n = 0;
        if (ox < ow) {
            ip_taps(ox, cw, ow, aa, lo, n);
            ip_weights(ox, cw, ow, aa, lo, n, wx + lane, IP_BW);
        }
        xlo[lane] = lo, xn[lane] = n;
    } else if (wave == 1 && lane < IP_BH) {
        int lo = 0, n = 0;
        if (lane < nb) {
            ip_taps(oy0 + lane, ch, oh, aa, lo, n);
            ip_weights(oy0 + lane, ch, oh, aa, lo, n, wy + lane * a.TY, 1);
        }
        ylo[lane] = lo, yn[lane] = n;
    }
    __syncthreads();

    // this wave's (row, channel) pairs p = wave + 4 r < nb C: output row p / C of the band, output channel p % C
    float acc[IP_ACC];
    int row[IP_ACC], chan[IP_ACC];
#pragma unroll
    for (int r = 0; r < IP_ACC; ++r) {
        const int p = wave + 4 * r;
        acc[r] = 0.0f;
        row[r] = p < nb * C ? p / C : -1;
        chan[r] = p < nb * C ? p - row[r] * C : 0;
    }
    const int ymin = ylo[0], ymax = ylo[nb - 1] + yn[nb - 1];  // (lo and lo + n never decrease with the output index)
    const int mylo = xlo[lane], myn = xn[lane];
    const char *img = static_cast<const char *>(s.base);
    const int esz = s.dtype == PIO_IMAGE_U8 ? 1 : 4;
    img += (int64_t)(g - s.img0) * s.sb * esz;

    for (int yc = ymin; yc < ymax; yc += IP_SR) {
        // horizontal pass: wave = staged row, lane = output column
        for (int r = wave; r < IP_SR; r += 4) {
            const int y = yc + r;
            if (y >= ymax) break;
            bool used = false;
            for (int j = 0; j < nb; ++j) used = used || (y >= ylo[j] && y < ylo[j] + yn[j]);
            if (!used || myn == 0) continue;
            float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f, v3 = 0.0f;
            const char *prow = img + ((int64_t)y * s.sy + (int64_t)mylo * s.sx) * esz;
            const int64_t step = s.sx * esz;
            if (s.vec4) {
                for (int t = 0; t < myn; ++t, prow += step) {
                    const float w = wx[t * IP_BW + lane];
                    float x0, x1, x2, x3;
                    if (s.dtype == PIO_IMAGE_U8) {
                        const uint32_t px = *reinterpret_cast<const uint32_t *>(prow);
                        x0 = (float)(px & 255u), x1 = (float)((px >> 8) & 255u), x2 = (float)((px >> 16) & 255u),
                        x3 = (float)(px >> 24);
                    } else {
                        const f32x4 px = *reinterpret_cast<const f32x4 *>(prow);
                        x0 = px[0], x1 = px[1], x2 = px[2], x3 = px[3];
                    }
                    v0 = fmaf(w, x0, v0), v1 = fmaf(w, x1, v1), v2 = fmaf(w, x2, v2), v3 = fmaf(w, x3, v3);
                }
            } else {
                const int64_t sc = s.sc * esz;
                for (int t = 0; t < myn; ++t, prow += step) {
                    const float w = wx[t * IP_BW + lane];
                    float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (c < C)
                            x[c] = s.dtype == PIO_IMAGE_U8 ? (float)*reinterpret_cast<const uint8_t *>(prow + c * sc)
                                                           : *reinterpret_cast<const float *>(prow + c * sc);
                    v0 = fmaf(w, x[0], v0), v1 = fmaf(w, x[1], v1), v2 = fmaf(w, x[2], v2), v3 = fmaf(w, x[3], v3);
                }
            }
            float *hr = h + r * C * IP_BW + lane;
            hr[0] = v0;
            if (C > 1) hr[IP_BW] = v1;
            if (C > 2) hr[2 * IP_BW] = v2;
            if (C > 3) hr[3 * IP_BW] = v3;
        }
        __syncthreads();
        // vertical pass: rows of the chunk ascending, per accumulator
        if (myn != 0) {
#pragma unroll
            for (int r = 0; r < IP_ACC; ++r) {
                if (row[r] < 0) continue;
                const int lo = ylo[row[r]], n = yn[row[r]];
                const int cs = a.reverse ? C - 1 - chan[r] : chan[r];
                const int ya = max(lo, yc), yb = min(lo + n, min(yc + IP_SR, ymax));
                const float *wr = wy + row[r] * a.TY;
                const float *hc = h + cs * IP_BW + lane;
                for (int y = ya; y < yb; ++y) acc[r] = fmaf(wr[y - lo], hc[(y - yc) * C * IP_BW], acc[r]);
            }
        }
        __syncthreads();
    }

    if (myn != 0) {
        float *o = out + (int64_t)g * out_sb;
#pragma unroll
        for (int r = 0; r < IP_ACC; ++r) {
            if (row[r] < 0) continue;
            const int c = chan[r];
            o[((int64_t)c * oh + oy0 + row[r]) * ow + ox] = (acc[r] - a.mean[c]) / a.std[c];
        }
    }
}

}  // namespace

int prepare_images_launch(const pio_image_src_t *srcs, int nsrc, int C, int oh, int ow, int antialias, int reverse,
                          const float *mean, const float *std, float *out, int64_t out_sb, hipStream_t s) {
    if (!srcs || !out || nsrc < 1 || nsrc > PIO_MAX_IMAGE_SOURCES) return PIO_E_ARG;
    for (int i = 0; i < nsrc; ++i) {
        if (!srcs[i].data) return PIO_E_ARG;
        if (srcs[i].dtype != PIO_IMAGE_U8 && srcs[i].dtype != PIO_IMAGE_F32) return PIO_E_ARG;
    }
    if (C < 1 || C > 4 || oh < 1 || oh > 1024 || ow < 1 || ow > 1024) return PIO_E_SHAPE;
    IpArgs a;
    const bool aa = antialias != 0;
    int64_t images = 0;
    int tx = 1, ty = 1;
    double bytes = 0.0;
    for (int i = 0; i < nsrc; ++i) {
        const pio_image_src_t &g = srcs[i];
        if (g.C != C || g.n < 1 || g.H < 1 || g.H > 16384 || g.W < 1 || g.W > 16384) return PIO_E_SHAPE;
        if (g.y0 < 0 || g.x0 < 0 || g.ch < 1 || g.cw < 1 || (int64_t)g.y0 + g.ch > g.H || (int64_t)g.x0 + g.cw > g.W)
            return PIO_E_SHAPE;
        if ((g.n > 1 && g.sb < 0) || (C > 1 && g.sc < 0) || (g.H > 1 && g.sy < 0) || (g.W > 1 && g.sx < 0)) return PIO_E_SHAPE;
        if (g.ch > (int64_t)PIO_IMAGE_MAX_REDUCTION * oh || g.cw > (int64_t)PIO_IMAGE_MAX_REDUCTION * ow) return PIO_E_SHAPE;
        const int esz = g.dtype == PIO_IMAGE_U8 ? 1 : 4;
        if (esz == 4 && ((uintptr_t)g.data & 3)) return PIO_E_ALIGN;
        // (the stride of an axis of length 1 is not read: the kernel multiplies it by index 0 only, so zero it)
        const int64_t sb = g.n > 1 ? g.sb : 0, sc = C > 1 ? g.sc : 0, sy = g.H > 1 ? g.sy : 0, sx = g.W > 1 ? g.sx : 0;
        const char *base = static_cast<const char *>(g.data) + ((int64_t)g.y0 * sy + (int64_t)g.x0 * sx) * esz;
        const int64_t px = 4 * (int64_t)esz;  // bytes of a four-channel pixel
        const bool vec4 = C == 4 && sc == 1 && (uintptr_t)base % px == 0 && sb % 4 == 0 && sy % 4 == 0 && sx % 4 == 0;
        a.src[i] = IpSrc{base, sb, sc, sy, sx, g.dtype, (int32_t)images, g.ch, g.cw, vec4 ? 1 : 0};
        images += g.n;
        if (images > 0x7fffffffLL) return PIO_E_SHAPE;
        for (int k = 0; k < ow; ++k) {
            int lo, n;
            ip_taps(k, g.cw, ow, aa, lo, n);
            tx = n > tx ? n : tx;
        }
        for (int k = 0; k < oh; ++k) {
            int lo, n;
            ip_taps(k, g.ch, oh, aa, lo, n);
            ty = n > ty ? n : ty;
        }
        bytes += (double)g.n * C * ((double)g.ch * g.cw * esz + 4.0 * oh * ow);
    }
    if (tx > IP_MAX_TAPS || ty > IP_MAX_TAPS) return PIO_E_SHAPE;  // (cannot happen under the reduction cap)
    if (images > 1 && out_sb < (int64_t)C * oh * ow) return PIO_E_SHAPE;
    if ((uintptr_t)out & 3) return PIO_E_ALIGN;
    const int bands = (oh + IP_BH - 1) / IP_BH, tiles = (ow + IP_BW - 1) / IP_BW;
    if (images * bands * tiles > 0x7fffffffLL) return PIO_E_SHAPE;
    for (int i = nsrc; i < PIO_MAX_IMAGE_SOURCES; ++i) a.src[i] = a.src[0];
    for (int c = 0; c < 4; ++c) {
        a.mean[c] = mean && c < C ? mean[c] : 0.0f;
        a.std[c] = std && c < C ? std[c] : 1.0f;
    }
    a.nsrc = nsrc, a.C = C, a.oh = oh, a.ow = ow, a.aa = aa ? 1 : 0, a.reverse = reverse ? 1 : 0;
    a.TX = tx, a.TY = ty, a.bands = bands, a.tiles = tiles;
    const size_t lds = sizeof(float) * ((size_t)tx * IP_BW + (size_t)IP_BH * ty + 2 * IP_BW + 2 * IP_BH
                                        + (size_t)IP_SR * C * IP_BW);
    ProfScope prof(PROF_LAYERNORM, 0.0, bytes, s);
    hipLaunchKernelGGL(prepare_images_kernel, dim3((unsigned)(images * bands * tiles)), dim3(256), lds, s, a, out, out_sb);
    return launch_status();
}

}  // namespace pio
