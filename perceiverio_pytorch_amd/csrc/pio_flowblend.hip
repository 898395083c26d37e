// Tail of tiled optical-flow inference in one pass (pio_flow_blend_tiles): the flows of all training-size tiles of a frame,
// each weighted by a linear ramp that peaks at the tile centre, summed in tile order and divided by the summed ramps
// (models.py FlowPerceiver.forward, test_mode; flow_perceiver.py:165-190).  Per output element (n, c, Y, X):
//
//   acc = +0, wsum = +0
//   for iy < ny, for ix < nx (this order), ly = Y - ys[iy], lx = X - xs[ix], only where 0 <= ly < H and 0 <= lx < W:
//     r    = fdiv_rn((float)min(lx + 1, W - lx, ly + 1, H - ly), (float)min((W + 1) / 2, (H + 1) / 2))
//     acc  = fadd_rn(acc, fmul_rn(flow_k[n, c, ly, lx], r))          k = iy nx + ix; never an FMA
//     wsum = fadd_rn(wsum, r)
//   out[n, c, Y, X] = fdiv_rn(acc, wsum)
//
// The chain multiplies every tile by the ramp, zero-pads product and ramp to the image and adds both to full-image sums:
// about 5 launches and 2 full-image temporaries per tile.  Where a tile does not cover a pixel the chain adds +0 to a sum
// that began as +0, which never changes a bit, so leaving those tiles out gives the chain's result bit for bit, signs of
// zeros included.  This file is compiled without floating-point contraction (the pragma below): the product and the add
// stay two rounded operations, and `/` is the correctly rounded fp32 division.
//
// One workgroup owns FB_SPAN consecutive pixels of one image row of one sample; a lane owns a pixel and both of its
// channels.  The loops over iy and ix, the row test and the test of the span against a tile's columns are uniform across
// the workgroup, so corners and group pointers are read from the kernel arguments with uniform indices; only the test of a
// lane's own pixel against the tile is per lane.  In the shipped layout (the permuted view of [B, H, W, 2]: sc = 1, sx = 2)
// a lane reads both channels of a tile pixel as one 8-byte load (PAIR); any other strides read two dwords.  Stores are
// coalesced along x, one per channel.  All offsets are 64-bit; the argument struct travels by value.
#include "pio_internal.h"

#pragma clang fp contract(off)

namespace pio {

namespace {

constexpr int FB_SPAN = 256;  // pixels of a row per workgroup

typedef float f32x2 __attribute__((ext_vector_type(2)));

// PAIR: sc == 1, sx == 2, sn and sy even, every group pointer 8-byte aligned
template <bool PAIR>
__global__ __launch_bounds__(FB_SPAN) void flow_blend_kernel(const pio_flow_blend_t p, float *__restrict__ out, int64_t on,
                                                             int64_t oc, int64_t oy, int spans, float rmax) {
    const unsigned rowid = blockIdx.x / (unsigned)spans;
    const int x0 = (int)(blockIdx.x - rowid * (unsigned)spans) * FB_SPAN;
    const int n = (int)(rowid / (unsigned)p.h), Y = (int)(rowid - (unsigned)n * (unsigned)p.h);
    const int X = x0 + (int)threadIdx.x;
    float acc0 = 0.0f, acc1 = 0.0f, wsum = 0.0f;
    for (int iy = 0; iy < p.ny; ++iy) {
        const int ly = Y - p.ys[iy];
        if (ly < 0 || ly >= p.H) continue;
        const int ry = min(ly + 1, p.H - ly);
        for (int ix = 0; ix < p.nx; ++ix) {
            const int xs = p.xs[ix];
            if ((int64_t)xs + p.W <= x0 || xs >= x0 + FB_SPAN) continue;
            const int k = iy * p.nx + ix, g = k / p.tiles_per_group, j = k - g * p.tiles_per_group;
            const int lx = X - xs;
            if (lx >= 0 && lx < p.W && X < p.w) {
                const float *src = p.group[g] + ((int64_t)j * p.N + n) * p.sn + (int64_t)ly * p.sy + (int64_t)lx * p.sx;
                float f0, f1;
                if constexpr (PAIR) {
                    const f32x2 f = *reinterpret_cast<const f32x2 *>(src);
                    f0 = f[0], f1 = f[1];
                } else {
                    f0 = src[0], f1 = src[p.sc];
                }
                const float r = (float)min(min(lx + 1, p.W - lx), ry) / rmax;
                acc0 = acc0 + f0 * r;
                acc1 = acc1 + f1 * r;
                wsum = wsum + r;
            }
        }
    }
    if (X < p.w) {
        float *o = out + (int64_t)n * on + (int64_t)Y * oy + X;
        o[0] = acc0 / wsum;
        o[oc] = acc1 / wsum;
    }
}

// true when the intervals [c, c + len) of the n corners cover [0, size)
bool fb_covers(const int32_t *c, int n, int64_t len, int64_t size) {
    int64_t pos = 0;
    while (pos < size) {
        int64_t reach = pos;
        for (int i = 0; i < n; ++i)
            if (c[i] <= pos && c[i] + len > reach) reach = c[i] + len;
        if (reach == pos) return false;
        pos = reach;
    }
    return true;
}

}  // namespace

int flow_blend_tiles_launch(const pio_flow_blend_t *pp, float *out, int64_t on, int64_t oc, int64_t oy, hipStream_t s) {
    if (!pp || !out) return PIO_E_ARG;
    const pio_flow_blend_t &p = *pp;
    if (p.ngroups < 1 || p.ngroups > PIO_MAX_BLEND_GROUPS) return PIO_E_SHAPE;
    for (int i = 0; i < p.ngroups; ++i)
        if (!p.group[i]) return PIO_E_ARG;
    if (p.N < 1 || p.H < 1 || p.W < 1 || p.h < p.H || p.w < p.W) return PIO_E_SHAPE;
    if (p.ny < 1 || p.ny > PIO_MAX_BLEND_AXIS || p.nx < 1 || p.nx > PIO_MAX_BLEND_AXIS) return PIO_E_SHAPE;
    if (p.tiles_per_group < 1) return PIO_E_SHAPE;
    const int tiles = p.ny * p.nx;
    if (p.ngroups != (tiles + p.tiles_per_group - 1) / p.tiles_per_group) return PIO_E_SHAPE;
    // a tile begins inside the image; what hangs over its lower or right edge is cut off, as the chain's negative padding does
    for (int i = 0; i < p.ny; ++i)
        if (p.ys[i] < 0 || p.ys[i] >= p.h) return PIO_E_SHAPE;
    for (int i = 0; i < p.nx; ++i)
        if (p.xs[i] < 0 || p.xs[i] >= p.w) return PIO_E_SHAPE;
    if (!fb_covers(p.ys, p.ny, p.H, p.h) || !fb_covers(p.xs, p.nx, p.W, p.w)) return PIO_E_SHAPE;
    if (oy < p.w) return PIO_E_SHAPE;
    const int64_t spans = ((int64_t)p.w + FB_SPAN - 1) / FB_SPAN;
    if (spans * p.h > 0x7fffffffLL / p.N) return PIO_E_SHAPE;
    uintptr_t bits = (uintptr_t)out;
    for (int i = 0; i < p.ngroups; ++i) bits |= (uintptr_t)p.group[i];
    if (bits & 3) return PIO_E_ALIGN;
    bool pair = p.sc == 1 && p.sx == 2 && p.sn % 2 == 0 && p.sy % 2 == 0;
    for (int i = 0; i < p.ngroups; ++i) pair = pair && !((uintptr_t)p.group[i] & 7);
    pio_flow_blend_t a = p;
    for (int i = p.ngroups; i < PIO_MAX_BLEND_GROUPS; ++i) a.group[i] = p.group[0];
    for (int i = p.ny; i < PIO_MAX_BLEND_AXIS; ++i) a.ys[i] = 0;
    for (int i = p.nx; i < PIO_MAX_BLEND_AXIS; ++i) a.xs[i] = 0;
    const float rmax = (float)((p.W + 1) / 2 < (p.H + 1) / 2 ? (p.W + 1) / 2 : (p.H + 1) / 2);
    const double px = (double)p.N * p.h * p.w;
    ProfScope prof(PROF_LAYERNORM, 0.0, 8.0 * px + 8.0 * (double)p.N * tiles * p.H * p.W, s);
    const dim3 grid((unsigned)(spans * p.h * p.N));
    if (pair)
        hipLaunchKernelGGL(flow_blend_kernel<true>, grid, dim3(FB_SPAN), 0, s, a, out, on, oc, oy, (int)spans, rmax);
    else
        hipLaunchKernelGGL(flow_blend_kernel<false>, grid, dim3(FB_SPAN), 0, s, a, out, on, oc, oy, (int)spans, rmax);
    return launch_status();
}

}  // namespace pio
