// Forward-backward consistency of a batch of flows whose second half holds the reversed pairs of the first: value and gradient.
//
// The partner of sample n is m = (n + N/2) mod N.  With the sampler's transposed convention (channel 0 + the ROW index is x, the
// column; channel 1 + the COLUMN index is y, the row; resample_kernel of elem.hip), for pixel (i, j) of sample n, f = flow[n,i,j]:
//   x = f0 + i,  y = f1 + j               valid iff 0 <= x <= W-1 and 0 <= y <= H-1 (NaN and inf are not): every tap with a non-zero
//                                         weight lies inside the image, so a sample is never faded towards 0
//   s  = bilinear sample of flow[m] at (row y, column x), the sampler's taps ff cc fc cf and its weight expressions; a tap at
//        index W or H occurs only with weight 0, reads 0 and receives nothing
//   r0 = f0 + s1,  r1 = f1 + s0           the channel swap belongs to the transposed convention
//   d  = sqrt((r0 r0 + r1 r1) + eps^2),   phi = d - eps,   psi = (r0 / d, r1 / d)
//   C  = sum over the valid pixels of phi / (N H W),   valid_fraction = valid pixels / (N H W)
//   with k = weight / (N H W):
//   gathered[n,i,j] = ((psi0 + gx) k, (psi1 + gy) k)                         gx, gy the sampler's warp gradient for
//                                                                            dgen = (psi1, psi0), channels added in order from 0
//   scattered[m, tap q] += (w_q psi1, w_q psi0), the sum then times k
//   grad = gathered + scattered, stored, or added onto what is there with ONE fp32 addition per element
//
// Built with -ffp-contract=off: every step is fp32 in the order of the numpy twin (metrics.py flow_consistency_host at float32).
// sqrt and the division are the correctly rounded ones, so r == 0 gives d == eps, phi == 0 and psi == 0 exactly.  The sum of phi
// is kept in double and the count of valid pixels is integer-valued (a double below 2^53: exact), both reduced in a fixed order.
//
// The scatter is accumulated in 64-bit fixed point, like the data gradient of resampler.hip: integer addition is associative, so
// the order in which the atomics arrive cannot change a sum.  An element of flow[m] receives at most one tap of each of the H W
// pixels of sample n, and |w_q psi| < 1, so with
//   K = 62 - ceil(log2(H W))              (48 at 128 x 128; at least 32, because H, W <= 32768)
// the sum of the llrint(w_q psi 2^K) stays within H W 2^K <= 2^62: no element can overflow, and K needs no look at the data.
// Every entry is rounded once, by at most 2^-(K+1): an element that received e entries is off by at most e 2^-(K+1) |k| before
// the one fp32 rounding of the conversion.
//
// Three launches, no float atomics, no device state outside the caller's workspace:
//   tile     one workgroup of 256 threads per 16 x 64 pixel tile of one image, four pixels per thread.  Value: the tile's two
//            sums.  Gradient: the gathered part (direct term + warp term) goes into a float2 plane of the workspace, one writer
//            per element, and the thread clears the two int64 words of its own pixel.
//   scatter  (gradient only) the same tiles walked transposed (lanes along the rows, so a wave's taps are neighbours in the partner);
//            the per-pixel quantities are recomputed from the same expressions, and every tap with a non-zero entry gets one
//            64-bit integer atomicAdd per channel
//   final    gathered + (acc * 2^-K as fp32) * k, stored into grad or added onto it: one writer per element and, when it
//            accumulates, exactly one fp32 addition onto the contents (so accumulate == contents + the stored gradient, bit for
//            bit); its workgroup 0 then adds the tiles' sums in a fixed order and adds (or stores) weight * C into loss_accum
// A call without grad runs tile and a one-workgroup final; one without loss_accum skips the sums.
#include "image_common.h"
#include <algorithm>
#include <cfloat>

namespace mv3d {
namespace {

constexpr int FC_TW = 64;                          // tile width in pixels: one wave per row
constexpr int FC_TH = 16;                          // tile height
constexpr int FC_THREADS = IMG_THREADS;
constexpr int FC_ROWS = FC_TH / (FC_THREADS / FC_TW);      // pixel rows per thread (4)
constexpr int FC_MAX_GRID = 4096;                  // the final launch strides beyond this

static_assert(FC_THREADS % FC_TW == 0 && FC_TH % (FC_THREADS / FC_TW) == 0, "the walk covers the tile without a remainder");

struct FcArgs {
    const float* flow;
    double* part; unsigned long long* acc; float* gath; float* loss; float* stats; float* grad;
    int N, H, W, flow_ld, grad_ld, tx, ty, accumulate, overwrite, flow_vec, grad_vec;
    float eps, eps2, k, weight, xmax, ymax;
    double npix, scale, inv_scale;
};

struct FcPixel {
    float phi, psi0, psi1, gx, gy;
    float w[4];                                    // ff, cc, fc, cf
    int64_t tap[4];                                // pixel index inside the partner image, from clamped coordinates
    bool ok[4];
};

__device__ __forceinline__ float2 fc_load(const float* q, int vec) {
    if (vec) return *reinterpret_cast<const float2*>(q);
    return make_float2(q[0], q[1]);
}

// Everything one pixel contributes; false for a pixel that is not valid (o is then not filled).  `partner` is flow[m].
__device__ __forceinline__ bool fc_pixel(const FcArgs& p, const float* partner, int i, int j, float2 f, FcPixel& o) {
    const float x = f.x + (float)i;
    const float y = f.y + (float)j;
    if (!(x >= 0.0f && y >= 0.0f && x <= p.xmax && y <= p.ymax)) return false;      // a NaN fails every comparison
    const float fxf = floorf(x), fyf = floorf(y);
    const int fx = (int)fxf, fy = (int)fyf, cx = fx + 1, cy = fy + 1;               // 0 <= fx <= W-1, 0 <= fy <= H-1
    const float dx = (fxf + 1.0f) - x, dy = (fyf + 1.0f) - y;
    const int xs[4] = {fx, cx, fx, cx}, ys[4] = {fy, cy, cy, fy};
    float2 t[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        o.ok[q] = xs[q] < p.W && ys[q] < p.H;                                       // index W or H: weight 0, reads 0
        const int xc = min(xs[q], p.W - 1), yc = min(ys[q], p.H - 1);               // an address is never formed from an unclamped one
        o.tap[q] = (int64_t)yc * p.W + xc;
        const float2 v = fc_load(partner + o.tap[q] * p.flow_ld, p.flow_vec);
        t[q] = o.ok[q] ? v : make_float2(0.f, 0.f);
    }
    o.w[0] = dx * dy;
    o.w[1] = (1.0f - dx) * (1.0f - dy);
    o.w[2] = dx * (1.0f - dy);
    o.w[3] = (1.0f - dx) * dy;
    const float s0 = ((o.w[0] * t[0].x + o.w[1] * t[1].x) + o.w[2] * t[2].x) + o.w[3] * t[3].x;
    const float s1 = ((o.w[0] * t[0].y + o.w[1] * t[1].y) + o.w[2] * t[2].y) + o.w[3] * t[3].y;
    const float r0 = f.x + s1, r1 = f.y + s0;
    const float d = sqrtf((r0 * r0 + r1 * r1) + p.eps2);       // plain sqrtf and / are the correctly rounded ones, as in flow_smooth.hip
    o.phi = d - p.eps;
    o.psi0 = r0 / d;
    o.psi1 = r1 / d;
    // the sampler's warp gradient with dgen = (psi1, psi0): channel 0 first, then channel 1
    float gx = 0.f, gy = 0.f;
    gx = gx + o.psi1 * (dy * (t[3].x - t[0].x) + (1.0f - dy) * (t[1].x - t[2].x));
    gy = gy + o.psi1 * (dx * (t[2].x - t[0].x) + (1.0f - dx) * (t[1].x - t[3].x));
    gx = gx + o.psi0 * (dy * (t[3].y - t[0].y) + (1.0f - dy) * (t[1].y - t[2].y));
    gy = gy + o.psi0 * (dx * (t[2].y - t[0].y) + (1.0f - dx) * (t[1].y - t[3].y));
    o.gx = gx;
    o.gy = gy;
    return true;
}

__global__ __launch_bounds__(FC_THREADS) void flow_consist_tile_kernel(const FcArgs p) {
    __shared__ double s_red[2 * (FC_THREADS / 64)];
    const int tiles = p.tx * p.ty;
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int y0 = (t / p.tx) * FC_TH, x0 = (t % p.tx) * FC_TW;
    const int tid = threadIdx.x;
    const int m = n >= p.N / 2 ? n - p.N / 2 : n + p.N / 2;
    const int64_t plane = (int64_t)p.H * p.W;
    const float* own = p.flow + (int64_t)n * plane * p.flow_ld;
    const float* partner = p.flow + (int64_t)m * plane * p.flow_ld;
    const bool want_value = p.loss != nullptr, want_grad = p.grad != nullptr;
    double sums[2] = {0.0, 0.0};                            // phi over the valid pixels, the valid pixels
    const int j = x0 + (tid & (FC_TW - 1));
    if (j < p.W) {
#pragma unroll
        for (int o = 0; o < FC_ROWS; ++o) {
            const int i = y0 + (tid / FC_TW) + o * (FC_THREADS / FC_TW);
            if (i >= p.H) break;
            const int64_t pix = (int64_t)i * p.W + j;
            const float2 f = fc_load(own + pix * p.flow_ld, p.flow_vec);
            FcPixel e;
            float2 g = make_float2(0.f, 0.f);
            if (fc_pixel(p, partner, i, j, f, e)) {
                sums[0] += (double)e.phi;
                sums[1] += 1.0;
                g.x = (e.psi0 + e.gx) * p.k;
                g.y = (e.psi1 + e.gy) * p.k;
            }
            if (want_grad) {
                const int64_t at = (int64_t)n * plane + pix;
                *reinterpret_cast<ulonglong2*>(p.acc + at * 2) = make_ulonglong2(0ull, 0ull);
                *reinterpret_cast<float2*>(p.gath + at * 2) = g;
            }
        }
    }
    if (!want_value) return;                                // uniform over the workgroup
    block_sum(sums, s_red, tid);
    if (tid == 0) {
        p.part[2 * (int64_t)blockIdx.x] = block_total(s_red, 0);
        p.part[2 * (int64_t)blockIdx.x + 1] = block_total(s_red, 1);
    }
}

__device__ __forceinline__ void fc_add(unsigned long long* dst, float w, float psi, double scale) {
    const double t = (double)w * (double)psi * scale;                          // the product of two floats is exact in double
    if (!(fabs(t) <= scale)) return;           // |w psi| < 1 for finite operands; a NaN or inf (a non-finite partner flow) is dropped
    const long long v = __double2ll_rn(t);
    if (v) atomicAdd(dst, (unsigned long long)v);
}

__global__ __launch_bounds__(FC_THREADS) void flow_consist_scatter_kernel(const FcArgs p) {
    const int tiles = p.tx * p.ty;
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int y0 = (t / p.tx) * FC_TH, x0 = (t % p.tx) * FC_TW;
    const int tid = threadIdx.x;
    const int m = n >= p.N / 2 ? n - p.N / 2 : n + p.N / 2;
    const int64_t plane = (int64_t)p.H * p.W;
    const float* own = p.flow + (int64_t)n * plane * p.flow_ld;
    const float* partner = p.flow + (int64_t)m * plane * p.flow_ld;
    unsigned long long* acc = p.acc + (int64_t)m * plane * 2;
    // The tile is walked TRANSPOSED (H == W): lanes run along the rows i, so the columns x ~ i of a wave's taps are neighbours in
    // one row y ~ j of the partner and an atomic instruction covers a few contiguous segments, not one word in each of 64 rows.
    const int i = x0 + (tid & (FC_TW - 1));
    if (i >= p.H) return;
#pragma unroll
    for (int o = 0; o < FC_ROWS; ++o) {
        const int j = y0 + (tid / FC_TW) + o * (FC_THREADS / FC_TW);
        if (j >= p.W) break;
        const float2 f = fc_load(own + ((int64_t)i * p.W + j) * p.flow_ld, p.flow_vec);
        FcPixel e;
        if (!fc_pixel(p, partner, i, j, f, e)) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!e.ok[q]) continue;
            fc_add(acc + e.tap[q] * 2, e.w[q], e.psi1, p.scale);
            fc_add(acc + e.tap[q] * 2 + 1, e.w[q], e.psi0, p.scale);
        }
    }
}

__global__ __launch_bounds__(FC_THREADS) void flow_consist_final_kernel(const FcArgs p) {
    if (p.grad) {
        const int64_t total = (int64_t)p.N * p.H * p.W, stride = (int64_t)gridDim.x * FC_THREADS;
        for (int64_t at = (int64_t)blockIdx.x * FC_THREADS + threadIdx.x; at < total; at += stride) {
            const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(p.acc + at * 2);
            const float t0 = (float)((double)(long long)a.x * p.inv_scale), t1 = (float)((double)(long long)a.y * p.inv_scale);
            float2 g = *reinterpret_cast<const float2*>(p.gath + at * 2);
            g.x = g.x + t0 * p.k;
            g.y = g.y + t1 * p.k;
            float* dst = p.grad + at * p.grad_ld;
            if (p.grad_vec) {
                float2* d2 = reinterpret_cast<float2*>(dst);
                if (p.accumulate) { const float2 old = *d2; g.x = old.x + g.x; g.y = old.y + g.y; }
                *d2 = g;
            } else {
                if (p.accumulate) { g.x = dst[0] + g.x; g.y = dst[1] + g.y; }
                dst[0] = g.x;
                dst[1] = g.y;
            }
        }
    }
    if (!p.loss || blockIdx.x != 0) return;                 // uniform over the workgroup
    tile_sums_final<2>(p.part, (int64_t)p.N * p.tx * p.ty, p.loss, p.overwrite, [&](const double (&sum)[2]) {
        const double c = sum[0] / p.npix;
        if (p.stats) {                                      // thread 0 alone evaluates the term
            p.stats[0] = (float)c;
            p.stats[1] = (float)(sum[1] / p.npix);
        }
        return (float)((double)p.weight * c);
    });
}

// 0 when the shape is outside what the entry takes
int64_t fc_tile_count(int N, int H, int W) {
    if (N < 2 || (N & 1) || H != W || H < 2 || H > IMG_MAX_SIDE) return 0;
    return image_tile_count(N, H, W, FC_TH, FC_TW);
}
size_t fc_plane_bytes(int N, int H, int W) {
    return (size_t)cdiv64((int64_t)N * H * W * 2 * (int64_t)sizeof(unsigned long long), 256) * 256;
}
size_t fc_gath_bytes(int N, int H, int W) {
    return (size_t)cdiv64((int64_t)N * H * W * 2 * (int64_t)sizeof(float), 256) * 256;
}
// ceil(log2(H W))
int fc_bits(int H, int W) {
    int bits = 0;
    while ((int64_t(1) << bits) < (int64_t)H * W) ++bits;
    return bits;
}

}  // namespace
}  // namespace mv3d

using namespace mv3d;

extern "C" {

size_t mv3d_flow_consistency_workspace_bytes(int N, int H, int W) {
    const int64_t total = fc_tile_count(N, H, W);
    return total ? fc_plane_bytes(N, H, W) + fc_gath_bytes(N, H, W) + tile_workspace_bytes(total, 2) : 0;
}

int mv3d_flow_consistency(int N, int H, int W, const void* flow, int flow_ld, float eps, float weight, void* loss_accum, void* stats,
                          void* grad, int grad_ld, int grad_accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mv3d_flow_consistency";
    if (N < 2 || (N & 1)) return fail(MV3D_E_INVAL, "%s: N (%d) must be even and at least 2 (the second half holds the reversed pairs)", fn, N);
    if (H != W) return fail(MV3D_E_INVAL, "%s: H (%d) and W (%d) differ (the transposed sampler convention needs square images)", fn, H, W);
    if (H < 2) return fail(MV3D_E_INVAL, "%s: H (%d) must be at least 2", fn, H);
    if (H > IMG_MAX_SIDE) return fail(MV3D_E_INVAL, "%s: H (%d) above %d", fn, H, IMG_MAX_SIDE);
    const int64_t total = fc_tile_count(N, H, W);
    if (!total) return fail_tiles(fn, N, H, W);
    if (flow_ld < 2) return fail(MV3D_E_INVAL, "%s: flow_ld (%d) smaller than 2", fn, flow_ld);
    if (grad_ld < 2) return fail(MV3D_E_INVAL, "%s: grad_ld (%d) smaller than 2", fn, grad_ld);
    {   // the largest element index of any operand, formed in int64 by the kernels
        const int ld = flow_ld > grad_ld ? flow_ld : grad_ld;
        if ((double)N * (double)H * (double)W * (double)ld >= 4.0e18)
            return fail(MV3D_E_INVAL, "%s: N (%d) images of %d x %d at pixel stride %d overflow the element index", fn, N, H, W, ld);
    }
    if (int rc = check_grad_accumulate(fn, grad_accumulate)) return rc;
    if (int rc = check_finite(fn, "eps", eps, true)) return rc;
    if (!(eps * eps >= FLT_MIN))                // a denormal or zero eps^2 has no root that is eps again: r == 0 would give 0 / 0
        return fail(MV3D_E_INVAL, "%s: eps (%g) is below 2^-63: eps * eps underflows in fp32", fn, (double)eps);
    if (int rc = check_finite(fn, "weight", weight, false)) return rc;
    if (int rc = check_not_null(fn, {{"flow", flow}})) return rc;
    if (!loss_accum && !grad) return fail(MV3D_E_INVAL, "%s: loss_accum and grad are both null", fn);
    if (stats && !loss_accum) return fail(MV3D_E_INVAL, "%s: stats without loss_accum", fn);
    const size_t plane_bytes = fc_plane_bytes(N, H, W), gath_bytes = fc_gath_bytes(N, H, W);
    if (int rc = check_buffers(fn, "flow, loss_accum, stats or grad", (uintptr_t)flow | (uintptr_t)loss_accum | (uintptr_t)stats | (uintptr_t)grad,
                               workspace, workspace_bytes, plane_bytes + gath_bytes + tile_workspace_bytes(total, 2))) return rc;

    FcArgs p = {};
    p.flow = (const float*)flow;
    p.acc = (unsigned long long*)workspace;
    p.gath = (float*)((char*)workspace + plane_bytes);
    p.part = (double*)((char*)workspace + plane_bytes + gath_bytes);
    p.loss = (float*)loss_accum; p.stats = (float*)stats; p.grad = (float*)grad;
    p.N = N; p.H = H; p.W = W; p.flow_ld = flow_ld; p.grad_ld = grad_ld;
    p.tx = cdiv(W, FC_TW); p.ty = cdiv(H, FC_TH);
    p.accumulate = grad_accumulate;
    // mv3d_loss_overwrite_next(): consumed by a call that writes the loss word (kept by a recorded one); a gradient-only call
    // is no loss entry and leaves it pending
    p.overwrite = (loss_accum && take_loss_overwrite()) ? 1 : 0;
    p.flow_vec = (flow_ld % 2 == 0 && ((uintptr_t)flow & 7) == 0) ? 1 : 0;
    p.grad_vec = (grad && grad_ld % 2 == 0 && ((uintptr_t)grad & 7) == 0) ? 1 : 0;
    // the constants of the numpy twin, each formed in double and rounded to fp32 once
    p.weight = weight;
    p.eps = eps;
    p.eps2 = eps * eps;                                   // fp32 product, normal (checked above): its correctly rounded root is eps again
    p.npix = (double)N * (double)H * (double)W;
    p.k = (float)((double)weight / p.npix);
    p.xmax = (float)(W - 1);
    p.ymax = (float)(H - 1);
    const int K = 62 - fc_bits(H, W);
    p.scale = std::ldexp(1.0, K);
    p.inv_scale = std::ldexp(1.0, -K);

    const double px = p.npix;
    // algorithmic bytes: the flow once as itself and once as a partner, the gathered part written, the plane cleared, the tile sums.  FLOPs per pixel: the bilinear sample of two channels ~22, the residual, root and
    // quotients ~10, the warp gradient ~28.
    const OpInfo tile_info{intern_label("flow_consist_tile"), px * (grad ? 60.0 : 32.0),
                           px * (16.0 + (grad ? 8.0 + 16.0 : 0.0)) + (loss_accum ? (double)total * 16.0 : 0.0)};
    const int grid = (int)total;
    int rc = dispatch(stream, tile_info, [=](hipStream_t s) {
        flow_consist_tile_kernel<<<grid, FC_THREADS, 0, s>>>(p);
        return launched("flow_consist_tile_kernel");
    });
    if (rc) return rc;
    if (grad) {
        // the flows again, and 8 integer atomics of 8 bytes per pixel
        const OpInfo scatter_info{intern_label("flow_consist_scatter"), px * 48.0, px * (16.0 + 64.0)};
        rc = dispatch(stream, scatter_info, [=](hipStream_t s) {
            flow_consist_scatter_kernel<<<grid, FC_THREADS, 0, s>>>(p);
            return launched("flow_consist_scatter_kernel");
        });
        if (rc) return rc;
    }
    const int final_grid = grad ? (int)std::min<int64_t>(cdiv64((int64_t)N * H * W, FC_THREADS), FC_MAX_GRID) : 1;
    const OpInfo final_info{intern_label("flow_consist_final"), grad ? px * 4.0 : 0.0,
                            (grad ? px * (32.0 + (grad_accumulate ? 8.0 : 0.0)) : 0.0) + (loss_accum ? (double)total * 16.0 + 16.0 : 0.0)};
    return dispatch(stream, final_info, [=](hipStream_t s) {
        flow_consist_final_kernel<<<final_grid, FC_THREADS, 0, s>>>(p);
        return launched("flow_consist_final_kernel");
    });
}

}  // extern "C"
