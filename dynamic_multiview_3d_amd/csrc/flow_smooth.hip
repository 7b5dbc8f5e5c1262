// Edge-aware first-order smoothness of a two-channel flow field: value and gradient with respect to the flow (its second-order
// sibling, mv3d_flow_smoothness2, follows the first-order kernel below and states its own definition there).
//
//   dx[n,i,j,c] = f[n,i,j+1,c] - f[n,i,j,c]  (j < W-1)        dy[n,i,j,c] = f[n,i+1,j,c] - f[n,i,j,c]  (i < H-1)
//   wx[n,i,j]   = exp(-(alpha/Cg) * sum_k |I[n,i,j+1,k] - I[n,i,j,k]|),  wy the same along rows;  1 without a guide
//   phi(d) = sqrt(d^2 + eps^2) - eps  (Charbonnier)            phi'(d) = d / sqrt(d^2 + eps^2)
//   S = sum wx phi(dx) / Zx + sum wy phi(dy) / Zy,   Zx = N H (W-1) 2,   Zy = N (H-1) W 2
//   dS/df[n,i,j,c] = (ex[i,j-1] - ex[i,j]) / Zx + (ey[i-1,j] - ey[i,j]) / Zy,   ex = wx phi'(dx),  ey = wy phi'(dy),  0 out of range
//
// Built with -ffp-contract=off: every step is fp32 in the order of the numpy twin (metrics.py flow_smoothness_host at float32),
// up to expf.  sqrt and the division are the correctly rounded ones, so sqrt(eps * eps) == eps: a constant flow gives d == 0,
// phi == 0 and phi' == 0 exactly, whatever the guide.  Only the two sums behind S are kept in double, in a fixed order.
//
// Two launches, no atomics, no device state outside the caller's workspace:
//   tile    one workgroup of 256 threads per 16 x 64 pixel tile of one image (a wave covers one 64-pixel row: 512 contiguous
//           bytes of a dense flow).  It stages the 18 x 66 halo of the flow (as float2) and of the guide's channels (one plane
//           each) in LDS, zeros outside the image.  Then every edge the tile's pixels touch is evaluated ONCE: 16 x 65 horizontal
//           edges (origins one column left of the tile up to its last column) and 17 x 64 vertical ones; an edge's weight, its
//           root, phi and phi' serve both channels and both pixels it joins.  ex / ey go to LDS; phi counts in the value only for
//           an edge whose ORIGIN pixel lies in the tile, so every difference counts once.  Last, every pixel combines its four
//           edges and writes (or adds to) its two gradient channels: one writer per element.
//   final   one workgroup adds the tiles' two sums in a fixed order and adds (or stores) weight * S into loss_accum.
// A call without loss_accum skips the sums and the final launch; one without grad skips ex / ey and the last phase.
//
// LDS: lanes run along the columns in every phase (consecutive float2 / float addresses), so no pitch needs padding against the
// 64 banks.  9.5 KB flow halo + 4.75 KB per guide channel + 8.3 KB ex + 8.7 KB ey: 26.5 KB unguided, 45.5 KB with four channels.
#include "image_common.h"

namespace mv3d {
namespace {

constexpr int FS_TW = 64;                          // tile width in pixels: one wave per row
constexpr int FS_TH = 16;                          // tile height
constexpr int FS_HW = FS_TW + 2;                   // halo width
constexpr int FS_HH = FS_TH + 2;                   // halo height
constexpr int FS_THREADS = IMG_THREADS;
constexpr int FS_ROWS = FS_TH / (FS_THREADS / FS_TW);      // pixel rows per thread in the last phase (4)

static_assert(FS_THREADS % FS_TW == 0 && FS_TH % (FS_THREADS / FS_TW) == 0, "the last phase covers the tile without a remainder");

struct FsArgs {
    const float* flow; const float* guide;
    double* part; float* loss; float* grad;
    int N, H, W, flow_ld, guide_ld, grad_ld, tx, ty, accumulate, overwrite, flow_vec, guide_vec, grad_vec;
    float alpha_c, eps, eps2, cx, cy, weight;
    double zx, zy;
};

// one edge of one channel: d the difference, w the edge weight.  e = w * phi'(d); returns w * phi(d).
__device__ __forceinline__ float fs_edge(float d, float w, float eps, float eps2, float& e) {
    const float r = sqrtf(d * d + eps2);               // plain sqrtf and / are the correctly rounded ones (the __f*_rn forms map to the
    e = w * (d / r);                                    // native 1-ulp root here); tests/test_gpu_flow_smooth.py holds the kernel to that
    return w * (r - eps);
}

template <int GC>
__global__ __launch_bounds__(FS_THREADS) void flow_smooth_tile_kernel(const FsArgs p) {
    __shared__ float2 s_f[FS_HH * FS_HW];
    __shared__ float s_g[(GC ? GC : 1) * FS_HH * FS_HW];
    __shared__ float2 s_ex[FS_TH * (FS_TW + 1)];            // [r][q]: the edge with origin (y0 + r, x0 - 1 + q)
    __shared__ float2 s_ey[(FS_TH + 1) * FS_TW];            // [r][q]: the edge with origin (y0 - 1 + r, x0 + q)
    __shared__ double s_red[2 * (FS_THREADS / 64)];
    const int tiles = p.tx * p.ty;
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int y0 = (t / p.tx) * FS_TH, x0 = (t % p.tx) * FS_TW;
    const int tid = threadIdx.x;
    const int64_t img = (int64_t)n * p.H * p.W;

    for (int i = tid; i < FS_HH * FS_HW; i += FS_THREADS) {
        const int r = i / FS_HW, q = i - r * FS_HW;
        const int y = y0 - 1 + r, x = x0 - 1 + q;
        float2 f = make_float2(0.f, 0.f);
        float g[GC ? GC : 1] = {};
        if (y >= 0 && y < p.H && x >= 0 && x < p.W) {       // outside the image: zeros, which only reach edges that are dropped
            const int64_t pix = img + (int64_t)y * p.W + x;
            const float* src = p.flow + pix * p.flow_ld;
            if (p.flow_vec) f = *reinterpret_cast<const float2*>(src);
            else { f.x = src[0]; f.y = src[1]; }
            if (GC) {
                const float* gs = p.guide + pix * p.guide_ld;
                bool done = false;
                if constexpr (GC == 4) {
                    if (p.guide_vec) {
                        const float4 v = *reinterpret_cast<const float4*>(gs);
                        g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w;
                        done = true;
                    }
                }
                if constexpr (GC == 2) {
                    if (p.guide_vec) {
                        const float2 v = *reinterpret_cast<const float2*>(gs);
                        g[0] = v.x; g[1] = v.y;
                        done = true;
                    }
                }
                if (!done) {
#pragma unroll
                    for (int k = 0; k < GC; ++k) g[k] = gs[k];
                }
            }
        }
        s_f[i] = f;
#pragma unroll
        for (int k = 0; k < GC; ++k) s_g[k * FS_HH * FS_HW + i] = g[k];
    }
    __syncthreads();

    const bool want_value = p.loss != nullptr, want_grad = p.grad != nullptr;
    double sums[2] = {0.0, 0.0};                            // over the horizontal edges, over the vertical ones
    double &sx = sums[0], &sy = sums[1];
    // horizontal edges: halo row r + 1, between halo columns q and q + 1
    for (int i = tid; i < FS_TH * (FS_TW + 1); i += FS_THREADS) {
        const int r = i / (FS_TW + 1), q = i - r * (FS_TW + 1);
        const int y = y0 + r, x = x0 - 1 + q;
        float2 e = make_float2(0.f, 0.f);
        if (y < p.H && x >= 0 && x + 1 < p.W) {
            const int at = (r + 1) * FS_HW + q;
            const float2 f0 = s_f[at], f1 = s_f[at + 1];
            float w = 1.0f;
            if (GC) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < GC; ++k) s = s + fabsf(s_g[k * FS_HH * FS_HW + at + 1] - s_g[k * FS_HH * FS_HW + at]);
                w = expf(-(p.alpha_c * s));
            }
            const float v0 = fs_edge(f1.x - f0.x, w, p.eps, p.eps2, e.x);
            const float v1 = fs_edge(f1.y - f0.y, w, p.eps, p.eps2, e.y);
            if (q >= 1) sx += (double)v0 + (double)v1;          // origin in the tile: counted here and only here
        }
        if (want_grad) s_ex[i] = e;
    }
    // vertical edges: halo column q + 1, between halo rows r and r + 1
    for (int i = tid; i < (FS_TH + 1) * FS_TW; i += FS_THREADS) {
        const int r = i / FS_TW, q = i - r * FS_TW;
        const int y = y0 - 1 + r, x = x0 + q;
        float2 e = make_float2(0.f, 0.f);
        if (x < p.W && y >= 0 && y + 1 < p.H) {
            const int at = r * FS_HW + q + 1;
            const float2 f0 = s_f[at], f1 = s_f[at + FS_HW];
            float w = 1.0f;
            if (GC) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < GC; ++k) s = s + fabsf(s_g[k * FS_HH * FS_HW + at + FS_HW] - s_g[k * FS_HH * FS_HW + at]);
                w = expf(-(p.alpha_c * s));
            }
            const float v0 = fs_edge(f1.x - f0.x, w, p.eps, p.eps2, e.x);
            const float v1 = fs_edge(f1.y - f0.y, w, p.eps, p.eps2, e.y);
            if (r >= 1) sy += (double)v0 + (double)v1;
        }
        if (want_grad) s_ey[i] = e;
    }

    if (want_value) block_sum(sums, s_red, tid);            // uniform: either way one barrier, which ex / ey need as well
    else __syncthreads();
    if (want_value && tid == 0) {
        p.part[2 * (int64_t)blockIdx.x] = block_total(s_red, 0);
        p.part[2 * (int64_t)blockIdx.x + 1] = block_total(s_red, 1);
    }
    if (!want_grad) return;

    const int px = tid & (FS_TW - 1), x = x0 + px;
    if (x >= p.W) return;
#pragma unroll
    for (int o = 0; o < FS_ROWS; ++o) {
        const int pr = (tid / FS_TW) + o * (FS_THREADS / FS_TW), y = y0 + pr;
        if (y >= p.H) break;
        const float2 el = s_ex[pr * (FS_TW + 1) + px], er = s_ex[pr * (FS_TW + 1) + px + 1];
        const float2 eu = s_ey[pr * FS_TW + px], ed = s_ey[(pr + 1) * FS_TW + px];
        float2 g;
        g.x = (el.x - er.x) * p.cx + (eu.x - ed.x) * p.cy;
        g.y = (el.y - er.y) * p.cx + (eu.y - ed.y) * p.cy;
        float* dst = p.grad + (img + (int64_t)y * p.W + x) * p.grad_ld;
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

__global__ __launch_bounds__(FS_THREADS) void flow_smooth_final_kernel(const FsArgs p) {
    tile_sums_final<2>(p.part, (int64_t)p.N * p.tx * p.ty, p.loss, p.overwrite, [&](const double (&sum)[2]) {
        return (float)((double)p.weight * (sum[0] / p.zx + sum[1] / p.zy));
    });
}

// 0 when the shape is outside what the entry takes
int64_t fs_tile_count(int N, int H, int W) {
    return (H < 2 || W < 2) ? 0 : image_tile_count(N, H, W, FS_TH, FS_TW);
}

template <int GC>
int fs_launch_tile(const FsArgs& p, int grid, hipStream_t s) {
    flow_smooth_tile_kernel<GC><<<grid, FS_THREADS, 0, s>>>(p);
    return launched("flow_smooth_tile_kernel");
}

// ---- second order -----------------------------------------------------------------------------------------------------------
//   d[c]  = (f[+] - f[c]) - (f[c] - f[-])  per flow channel, along x for the centres j = 1..W-2, along y for i = 1..H-2
//   w     = exp(-(alpha/Cg) * s),  s = sum_k (|I[c,k] - I[-,k]| + |I[+,k] - I[c,k]|) added in that order;  1 without a guide
//   S2    = sum w phi(dx) / Z2x + sum w phi(dy) / Z2y,   Z2x = N H (W-2) 2,   Z2y = N (H-2) W 2
//   dS2/df[i,j] = ((ex[i,j-1] - ex[i,j]) - (ex[i,j] - ex[i,j+1])) / Z2x + ((ey[i-1,j] - ey[i,j]) - (ey[i,j] - ey[i+1,j])) / Z2y,
//   e = w phi'(d), 0 where no stencil is centred.  The numpy twin is metrics.py flow_smoothness_host(order=2) at float32.
// A flow whose first differences are exact and equal along an axis (constant, affine with dyadic coefficients) gives d == 0 and
// with it exactly 0 and zeros.  The same two launches; the tile stages a 20 x 68 halo and evaluates every stencil its pixels touch
// once: 16 x 66 horizontal centres (columns x0 - 1 .. x0 + 64) and 18 x 64 vertical ones (rows y0 - 1 .. y0 + 16); phi counts in
// the value only for a stencil whose CENTRE lies in the tile.  Each pixel then combines its three ex and three ey.
// LDS: 10 880 B flow halo + 5 440 B per guide channel + 8 448 B ex + 9 216 B ey: 27.9 KB unguided, 49.1 KB with four channels.
// Lanes run along the columns in every phase, as in the first-order kernel: no pitch needs padding.
constexpr int FS2_HW = FS_TW + 4;                  // halo width
constexpr int FS2_HH = FS_TH + 4;                  // halo height
constexpr int FS2_EXW = FS_TW + 2;                 // horizontal centres per tile row
constexpr int FS2_EYH = FS_TH + 2;                 // vertical centres per tile column

template <int GC>
__global__ __launch_bounds__(FS_THREADS) void flow_smooth2_tile_kernel(const FsArgs p) {
    __shared__ float2 s_f[FS2_HH * FS2_HW];
    __shared__ float s_g[(GC ? GC : 1) * FS2_HH * FS2_HW];
    __shared__ float2 s_ex[FS_TH * FS2_EXW];                // [r][q]: the stencil centred at (y0 + r, x0 - 1 + q)
    __shared__ float2 s_ey[FS2_EYH * FS_TW];                // [r][q]: the stencil centred at (y0 - 1 + r, x0 + q)
    __shared__ double s_red[2 * (FS_THREADS / 64)];
    constexpr int PLANE = FS2_HH * FS2_HW;
    const int tiles = p.tx * p.ty;
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int y0 = (t / p.tx) * FS_TH, x0 = (t % p.tx) * FS_TW;
    const int tid = threadIdx.x;
    const int64_t img = (int64_t)n * p.H * p.W;

    for (int i = tid; i < PLANE; i += FS_THREADS) {
        const int r = i / FS2_HW, q = i - r * FS2_HW;
        const int y = y0 - 2 + r, x = x0 - 2 + q;
        float2 f = make_float2(0.f, 0.f);
        float g[GC ? GC : 1] = {};
        if (y >= 0 && y < p.H && x >= 0 && x < p.W) {       // outside the image: zeros, which only reach stencils that are dropped
            const int64_t pix = img + (int64_t)y * p.W + x;
            const float* src = p.flow + pix * p.flow_ld;
            if (p.flow_vec) f = *reinterpret_cast<const float2*>(src);
            else { f.x = src[0]; f.y = src[1]; }
            if (GC) {
                const float* gs = p.guide + pix * p.guide_ld;
                bool done = false;
                if constexpr (GC == 4) {
                    if (p.guide_vec) {
                        const float4 v = *reinterpret_cast<const float4*>(gs);
                        g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w;
                        done = true;
                    }
                }
                if constexpr (GC == 2) {
                    if (p.guide_vec) {
                        const float2 v = *reinterpret_cast<const float2*>(gs);
                        g[0] = v.x; g[1] = v.y;
                        done = true;
                    }
                }
                if (!done) {
#pragma unroll
                    for (int k = 0; k < GC; ++k) g[k] = gs[k];
                }
            }
        }
        s_f[i] = f;
#pragma unroll
        for (int k = 0; k < GC; ++k) s_g[k * PLANE + i] = g[k];
    }
    __syncthreads();

    const bool want_value = p.loss != nullptr, want_grad = p.grad != nullptr;
    double sums[2] = {0.0, 0.0};                            // over the horizontal stencils, over the vertical ones
    double &sx = sums[0], &sy = sums[1];
    // one stencil: the halo pixels at - arm, at, at + arm
    auto stencil = [&](int at, int arm, float2& e, double& sum, bool counts) {
        const float2 fm = s_f[at - arm], fc = s_f[at], fp = s_f[at + arm];
        float w = 1.0f;
        if (GC) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < GC; ++k) {
                const float gm = s_g[k * PLANE + at - arm], gc = s_g[k * PLANE + at], gp = s_g[k * PLANE + at + arm];
                s = s + fabsf(gc - gm);
                s = s + fabsf(gp - gc);
            }
            w = expf(-(p.alpha_c * s));
        }
        const float v0 = fs_edge((fp.x - fc.x) - (fc.x - fm.x), w, p.eps, p.eps2, e.x);
        const float v1 = fs_edge((fp.y - fc.y) - (fc.y - fm.y), w, p.eps, p.eps2, e.y);
        if (counts) sum += (double)v0 + (double)v1;
    };
    // horizontal stencils: halo row r + 2, centred at halo column q + 1
    for (int i = tid; i < FS_TH * FS2_EXW; i += FS_THREADS) {
        const int r = i / FS2_EXW, q = i - r * FS2_EXW;
        const int y = y0 + r, x = x0 - 1 + q;
        float2 e = make_float2(0.f, 0.f);
        if (y < p.H && x >= 1 && x + 1 < p.W)
            stencil((r + 2) * FS2_HW + q + 1, 1, e, sx, q >= 1 && q <= FS_TW);       // centre in the tile: counted here and only here
        if (want_grad) s_ex[i] = e;
    }
    // vertical stencils: halo column q + 2, centred at halo row r + 1
    for (int i = tid; i < FS2_EYH * FS_TW; i += FS_THREADS) {
        const int r = i / FS_TW, q = i - r * FS_TW;
        const int y = y0 - 1 + r, x = x0 + q;
        float2 e = make_float2(0.f, 0.f);
        if (x < p.W && y >= 1 && y + 1 < p.H)
            stencil((r + 1) * FS2_HW + q + 2, FS2_HW, e, sy, r >= 1 && r <= FS_TH);
        if (want_grad) s_ey[i] = e;
    }

    if (want_value) block_sum(sums, s_red, tid);            // uniform: either way one barrier, which ex / ey need as well
    else __syncthreads();
    if (want_value && tid == 0) {
        p.part[2 * (int64_t)blockIdx.x] = block_total(s_red, 0);
        p.part[2 * (int64_t)blockIdx.x + 1] = block_total(s_red, 1);
    }
    if (!want_grad) return;

    const int px = tid & (FS_TW - 1), x = x0 + px;
    if (x >= p.W) return;
#pragma unroll
    for (int o = 0; o < FS_ROWS; ++o) {
        const int pr = (tid / FS_TW) + o * (FS_THREADS / FS_TW), y = y0 + pr;
        if (y >= p.H) break;
        const float2 el = s_ex[pr * FS2_EXW + px], ec = s_ex[pr * FS2_EXW + px + 1], er = s_ex[pr * FS2_EXW + px + 2];
        const float2 eu = s_ey[pr * FS_TW + px], em = s_ey[(pr + 1) * FS_TW + px], ed = s_ey[(pr + 2) * FS_TW + px];
        float2 g;
        g.x = ((el.x - ec.x) - (ec.x - er.x)) * p.cx + ((eu.x - em.x) - (em.x - ed.x)) * p.cy;
        g.y = ((el.y - ec.y) - (ec.y - er.y)) * p.cx + ((eu.y - em.y) - (em.y - ed.y)) * p.cy;
        float* dst = p.grad + (img + (int64_t)y * p.W + x) * p.grad_ld;
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

// 0 when the shape is outside what the second-order entry takes
int64_t fs2_tile_count(int N, int H, int W) {
    return (H < 3 || W < 3) ? 0 : image_tile_count(N, H, W, FS_TH, FS_TW);
}

template <int GC>
int fs2_launch_tile(const FsArgs& p, int grid, hipStream_t s) {
    flow_smooth2_tile_kernel<GC><<<grid, FS_THREADS, 0, s>>>(p);
    return launched("flow_smooth2_tile_kernel");
}

}  // namespace
}  // namespace mv3d

using namespace mv3d;

extern "C" {

size_t mv3d_flow_smoothness_workspace_bytes(int N, int H, int W) {
    return tile_workspace_bytes(fs_tile_count(N, H, W), 2);
}

int mv3d_flow_smoothness(int N, int H, int W, const void* flow, int flow_ld, const void* guide, int guide_c, int guide_ld,
                         float edge_alpha, float eps, float weight, void* loss_accum, void* grad, int grad_ld, int grad_accumulate,
                         void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mv3d_flow_smoothness";
    if (N < 1) return fail(MV3D_E_INVAL, "%s: N (%d) must be at least 1", fn, N);
    if (H < 2) return fail(MV3D_E_INVAL, "%s: H (%d) must be at least 2", fn, H);
    if (W < 2) return fail(MV3D_E_INVAL, "%s: W (%d) must be at least 2", fn, W);
    const int64_t total = fs_tile_count(N, H, W);
    if (!total) return fail_tiles(fn, N, H, W);
    if (flow_ld < 2) return fail(MV3D_E_INVAL, "%s: flow_ld (%d) smaller than 2", fn, flow_ld);
    if (guide_c < 0 || guide_c > 4) return fail(MV3D_E_INVAL, "%s: guide_c (%d) outside 0..4", fn, guide_c);
    if (guide_c && !guide) return fail(MV3D_E_INVAL, "%s: guide_c (%d) without a guide", fn, guide_c);
    if (guide_c && guide_ld < guide_c) return fail(MV3D_E_INVAL, "%s: guide_ld (%d) smaller than guide_c (%d)", fn, guide_ld, guide_c);
    if (grad_ld < 2) return fail(MV3D_E_INVAL, "%s: grad_ld (%d) smaller than 2", fn, grad_ld);
    {   // the largest element index of any operand, formed in int64 by the kernel
        int ld = flow_ld > grad_ld ? flow_ld : grad_ld;
        if (guide_c && guide_ld > ld) ld = guide_ld;
        if ((double)N * (double)H * (double)W * (double)ld >= 4.0e18)
            return fail(MV3D_E_INVAL, "%s: N (%d) images of %d x %d at pixel stride %d overflow the element index", fn, N, H, W, ld);
    }
    if (int rc = check_grad_accumulate(fn, grad_accumulate)) return rc;
    if (int rc = check_finite(fn, "eps", eps, true)) return rc;
    if (!std::isfinite(edge_alpha) || edge_alpha < 0.f) return fail(MV3D_E_INVAL, "%s: edge_alpha (%g) must be finite and not negative", fn, (double)edge_alpha);
    if (int rc = check_finite(fn, "weight", weight, false)) return rc;
    if (int rc = check_not_null(fn, {{"flow", flow}})) return rc;
    if (!loss_accum && !grad) return fail(MV3D_E_INVAL, "%s: loss_accum and grad are both null", fn);
    if (int rc = check_buffers(fn, "flow, guide, loss_accum or grad",
                               (uintptr_t)flow | (guide_c ? (uintptr_t)guide : 0) | (uintptr_t)loss_accum | (uintptr_t)grad, workspace,
                               workspace_bytes, tile_workspace_bytes(total, 2))) return rc;

    FsArgs p = {};
    p.flow = (const float*)flow; p.guide = guide_c ? (const float*)guide : nullptr; p.part = (double*)workspace;
    p.loss = (float*)loss_accum; p.grad = (float*)grad;
    p.N = N; p.H = H; p.W = W; p.flow_ld = flow_ld; p.guide_ld = guide_ld; p.grad_ld = grad_ld;
    p.tx = cdiv(W, FS_TW); p.ty = cdiv(H, FS_TH);
    p.accumulate = grad_accumulate;
    // mv3d_loss_overwrite_next(): consumed by a call that writes the loss word (kept by a recorded one); a gradient-only call
    // is no loss entry and leaves it pending
    p.overwrite = (loss_accum && take_loss_overwrite()) ? 1 : 0;
    // one vector load / store per pixel where stride and address allow it
    p.flow_vec = (flow_ld % 2 == 0 && ((uintptr_t)flow & 7) == 0) ? 1 : 0;
    p.grad_vec = (grad && grad_ld % 2 == 0 && ((uintptr_t)grad & 7) == 0) ? 1 : 0;
    p.guide_vec = ((guide_c == 4 && guide_ld % 4 == 0 && ((uintptr_t)guide & 15) == 0) ||
                   (guide_c == 2 && guide_ld % 2 == 0 && ((uintptr_t)guide & 7) == 0)) ? 1 : 0;
    // the constants of the numpy twin, each formed in double and rounded to fp32 once
    p.weight = weight;
    p.eps = eps;
    p.eps2 = eps * eps;                                   // fp32 product: its correctly rounded root is eps again
    p.alpha_c = guide_c ? (float)((double)edge_alpha / (double)guide_c) : 0.f;
    p.zx = (double)N * (double)H * (double)(W - 1) * 2.0;
    p.zy = (double)N * (double)(H - 1) * (double)W * 2.0;
    p.cx = (float)((double)weight / p.zx);
    p.cy = (float)((double)weight / p.zy);

    const double px = (double)N * H * W;
    // algorithmic bytes: the flow and the guide once, the gradient written once (and read once when it accumulates), the tile
    // sums.  FLOPs per pixel: 2 edges x 2 channels x ~8 (difference, square, add, root, quotient, products) + the guide's
    // 2 x (2 Cg + 3) + the combination's 12.
    const double grad_bytes = grad ? (grad_accumulate ? 16.0 : 8.0) : 0.0;
    const double flops = px * (32.0 + (guide_c ? 2.0 * (2.0 * guide_c + 3.0) : 0.0) + (grad ? 12.0 : 0.0));
    const OpInfo tile_info{intern_label("flow_smooth_tile"), flops,
                           px * (8.0 + 4.0 * guide_c + grad_bytes) + (loss_accum ? (double)total * 16.0 : 0.0)};
    const int grid = (int)total;
    int rc = dispatch(stream, tile_info, [=](hipStream_t s) {
        switch (guide_c) {
            case 0: return fs_launch_tile<0>(p, grid, s);
            case 1: return fs_launch_tile<1>(p, grid, s);
            case 2: return fs_launch_tile<2>(p, grid, s);
            case 3: return fs_launch_tile<3>(p, grid, s);
            default: return fs_launch_tile<4>(p, grid, s);
        }
    });
    if (rc || !loss_accum) return rc;
    const OpInfo final_info{intern_label("flow_smooth_final"), 0.0, (double)total * 16.0 + 8.0};
    return dispatch(stream, final_info, [=](hipStream_t s) {
        flow_smooth_final_kernel<<<1, FS_THREADS, 0, s>>>(p);
        return launched("flow_smooth_final_kernel");
    });
}

size_t mv3d_flow_smoothness2_workspace_bytes(int N, int H, int W) {
    return tile_workspace_bytes(fs2_tile_count(N, H, W), 2);
}

int mv3d_flow_smoothness2(int N, int H, int W, const void* flow, int flow_ld, const void* guide, int guide_c, int guide_ld,
                          float edge_alpha, float eps, float weight, void* loss_accum, void* grad, int grad_ld, int grad_accumulate,
                          void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mv3d_flow_smoothness2";
    if (N < 1) return fail(MV3D_E_INVAL, "%s: N (%d) must be at least 1", fn, N);
    if (H < 3) return fail(MV3D_E_INVAL, "%s: H (%d) must be at least 3", fn, H);
    if (W < 3) return fail(MV3D_E_INVAL, "%s: W (%d) must be at least 3", fn, W);
    const int64_t total = fs2_tile_count(N, H, W);
    if (!total) return fail_tiles(fn, N, H, W);
    if (flow_ld < 2) return fail(MV3D_E_INVAL, "%s: flow_ld (%d) smaller than 2", fn, flow_ld);
    if (guide_c < 0 || guide_c > 4) return fail(MV3D_E_INVAL, "%s: guide_c (%d) outside 0..4", fn, guide_c);
    if (guide_c && !guide) return fail(MV3D_E_INVAL, "%s: guide_c (%d) without a guide", fn, guide_c);
    if (guide_c && guide_ld < guide_c) return fail(MV3D_E_INVAL, "%s: guide_ld (%d) smaller than guide_c (%d)", fn, guide_ld, guide_c);
    if (grad_ld < 2) return fail(MV3D_E_INVAL, "%s: grad_ld (%d) smaller than 2", fn, grad_ld);
    {   // the largest element index of any operand, formed in int64 by the kernel
        int ld = flow_ld > grad_ld ? flow_ld : grad_ld;
        if (guide_c && guide_ld > ld) ld = guide_ld;
        if ((double)N * (double)H * (double)W * (double)ld >= 4.0e18)
            return fail(MV3D_E_INVAL, "%s: N (%d) images of %d x %d at pixel stride %d overflow the element index", fn, N, H, W, ld);
    }
    if (int rc = check_grad_accumulate(fn, grad_accumulate)) return rc;
    if (int rc = check_finite(fn, "eps", eps, true)) return rc;
    if (!std::isfinite(edge_alpha) || edge_alpha < 0.f) return fail(MV3D_E_INVAL, "%s: edge_alpha (%g) must be finite and not negative", fn, (double)edge_alpha);
    if (int rc = check_finite(fn, "weight", weight, false)) return rc;
    if (int rc = check_not_null(fn, {{"flow", flow}})) return rc;
    if (!loss_accum && !grad) return fail(MV3D_E_INVAL, "%s: loss_accum and grad are both null", fn);
    if (int rc = check_buffers(fn, "flow, guide, loss_accum or grad",
                               (uintptr_t)flow | (guide_c ? (uintptr_t)guide : 0) | (uintptr_t)loss_accum | (uintptr_t)grad, workspace,
                               workspace_bytes, tile_workspace_bytes(total, 2))) return rc;

    const int gc = edge_alpha > 0.f ? guide_c : 0;         // alpha == 0: every weight is 1 and no guide is read
    FsArgs p = {};
    p.flow = (const float*)flow; p.guide = gc ? (const float*)guide : nullptr; p.part = (double*)workspace;
    p.loss = (float*)loss_accum; p.grad = (float*)grad;
    p.N = N; p.H = H; p.W = W; p.flow_ld = flow_ld; p.guide_ld = guide_ld; p.grad_ld = grad_ld;
    p.tx = cdiv(W, FS_TW); p.ty = cdiv(H, FS_TH);
    p.accumulate = grad_accumulate;
    p.overwrite = (loss_accum && take_loss_overwrite()) ? 1 : 0;          // as in mv3d_flow_smoothness
    p.flow_vec = (flow_ld % 2 == 0 && ((uintptr_t)flow & 7) == 0) ? 1 : 0;
    p.grad_vec = (grad && grad_ld % 2 == 0 && ((uintptr_t)grad & 7) == 0) ? 1 : 0;
    p.guide_vec = ((gc == 4 && guide_ld % 4 == 0 && ((uintptr_t)guide & 15) == 0) ||
                   (gc == 2 && guide_ld % 2 == 0 && ((uintptr_t)guide & 7) == 0)) ? 1 : 0;
    // the constants of the numpy twin, each formed in double and rounded to fp32 once
    p.weight = weight;
    p.eps = eps;
    p.eps2 = eps * eps;                                   // fp32 product: its correctly rounded root is eps again
    p.alpha_c = gc ? (float)((double)edge_alpha / (double)gc) : 0.f;
    p.zx = (double)N * (double)H * (double)(W - 2) * 2.0;
    p.zy = (double)N * (double)(H - 2) * (double)W * 2.0;
    p.cx = (float)((double)weight / p.zx);
    p.cy = (float)((double)weight / p.zy);

    const double px = (double)N * H * W;
    // algorithmic bytes: those of mv3d_flow_smoothness (the flow and the guide once, the gradient written once and read once when
    // it accumulates, the tile sums).  FLOPs per pixel: 2 stencils x 2 channels x ~10 (two differences and their difference,
    // square, add, root, quotient, products) + the guide's 2 x (4 Cg + 3) + the combination's 18.
    const double grad_bytes = grad ? (grad_accumulate ? 16.0 : 8.0) : 0.0;
    const double flops = px * (40.0 + (gc ? 2.0 * (4.0 * gc + 3.0) : 0.0) + (grad ? 18.0 : 0.0));
    const OpInfo tile_info{intern_label("flow_smooth2_tile"), flops,
                           px * (8.0 + 4.0 * gc + grad_bytes) + (loss_accum ? (double)total * 16.0 : 0.0)};
    const int grid = (int)total;
    int rc = dispatch(stream, tile_info, [=](hipStream_t s) {
        switch (gc) {
            case 0: return fs2_launch_tile<0>(p, grid, s);
            case 1: return fs2_launch_tile<1>(p, grid, s);
            case 2: return fs2_launch_tile<2>(p, grid, s);
            case 3: return fs2_launch_tile<3>(p, grid, s);
            default: return fs2_launch_tile<4>(p, grid, s);
        }
    });
    if (rc || !loss_accum) return rc;
    // the final launch is the first-order term's: weight * (sum[0] / zx + sum[1] / zy) of the two tile sums
    const OpInfo final_info{intern_label("flow_smooth2_final"), 0.0, (double)total * 16.0 + 8.0};
    return dispatch(stream, final_info, [=](hipStream_t s) {
        flow_smooth_final_kernel<<<1, FS_THREADS, 0, s>>>(p);
        return launched("flow_smooth_final_kernel");
    });
}

}  // extern "C"
