// Occlusion masking of the appearance-flow head over pair-swapped batches: the mask from the forward-backward residual, and the
// sampler + masked pixel loss + flow gradient of the head in one tiled pass that makes the mask on the way.
//
// The conventions are those of flow_consist.hip.  The partner of sample n is m = (n + N/2) mod N.  With the sampler's transposed
// convention (channel 0 + the ROW index is x, the column; channel 1 + the COLUMN index is y, the row), for pixel (i, j) of sample
// n, f = flow[n,i,j]:
//   x = f0 + i,  y = f1 + j               inside iff 0 <= x <= W-1 and 0 <= y <= H-1 (NaN and inf are not): the consistency term's
//                                         strict window, not the sampler's -1 < x < W
//   s  = bilinear sample of flow[m] at (row y, column x), the sampler's taps ff cc fc cf and its weight expressions
//        w = (dx dy, (1-dx)(1-dy), dx (1-dy), (1-dx) dy),  s = ((w0 ff + w1 cc) + w2 fc) + w3 cf; a tap at index W or H occurs only
//        with weight 0 and reads 0
//   r0 = f0 + s1,  r1 = f1 + s0           the channel swap belongs to the transposed convention
//   lhs = r0 r0 + r1 r1,   rhs = alpha1 ((f0 f0 + f1 f1) + (s0 s0 + s1 s1)) + alpha2
//   visible iff inside and lhs < rhs      a NaN on either side fails the comparison: the pixel counts as occluded
//   mask = 1 where visible, 0 where inside and not visible, outside_visible ? 1 : 0 where not inside
// Built with -ffp-contract=off: every step is fp32 in the order of the numpy twin (metrics.py flow_occlusion_mask_host at float32).
// The three pixel counts are integer-valued doubles (below 2^53: exact), reduced in a fixed order; so is the loss sum, whose terms
// are the fp32 products of pixel_loss_kernel (elem.hip), each widened to double before it is added.
//
// One kernel, two instances.  A workgroup of 256 threads owns a 32 x 32 output tile and goes through LDS (pitch 33) like
// resample_tile_kernel of elem.hip:
//   A (j fastest)  coalesced reads of flow (+ target) -> LDS, warp_pts written
//   B (i fastest)  lanes run along the rows of the source and of the partner flow: the image taps and the partner-flow taps of a
//                  pixel sit at the same (row y, column x), so both gathers are (nearly) contiguous over 32 lanes; mask, gen, the
//                  loss terms and the flow gradient are computed here, gen and the gradient with the expressions of
//                  resample_tile_kernel, the loss and d(gen) with those of pixel_loss_kernel with a mask
//   C (j fastest)  coalesced stores of gen / dflow / mask from LDS
// and leaves the tile's loss sum and counts in the workspace; a one-workgroup final launch adds the tiles in index order.
// No float atomics, no device state outside the caller's workspace.
#include "image_common.h"
#include <algorithm>

namespace mv3d {
namespace {

constexpr int OC_TILE = 32;
constexpr int OC_P = 33;                           // LDS pitch: transposed reads hit 32 different banks
constexpr int OC_THREADS = IMG_THREADS;
constexpr int OC_SUMS = 4;                         // per tile: loss sum, visible, occluded, outside

struct OcclParams {
    const float* src; const float* flow; const float* tgt;
    float* warp; float* gen; float* dflow; float* mask; float* loss; float* stats; double* part;
    int N, H, W, flow_ld, tgt_ld, dflow_ld, mask_ld, kind, outside_visible, overwrite, flow_vec;
    float weight, alpha1, alpha2, xmax, ymax;
    int tiles_i, tiles_j;
    int64_t n_tiles;
    double npix;
};

__device__ __forceinline__ float2 oc_load(const float* q, int vec) {
    if (vec) return *reinterpret_cast<const float2*>(q);
    return make_float2(q[0], q[1]);
}

// One bilinear tap of the image: an unconditional load from a clamped (always valid) address, the bounds test selects the result.
__device__ __forceinline__ float oc_tap(const float* img, int W, int H, int C, int y, int x, int c) {
    const bool ok = (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H;
    const int xc = min(max(x, 0), W - 1), yc = min(max(y, 0), H - 1);
    const float v = img[((int64_t)yc * W + xc) * C + c];
    return ok ? v : 0.f;
}

// HEAD false: the mask alone (C is 1 and unused).  HEAD true: the occlusion-aware head over C image channels.
template <bool HEAD, int C>
__global__ __launch_bounds__(OC_THREADS) void occl_tile_kernel(const OcclParams p) {
    constexpr int P = OC_P;
    __shared__ float s_f[2][OC_TILE * P];                                   // f0, f1; then gx, gy
    __shared__ float s_m[OC_TILE * P];                                      // the mask
    __shared__ float s_c[HEAD ? C : 1][HEAD ? OC_TILE * P : 1];             // target; then gen
    __shared__ double s_red[OC_SUMS * 4];
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
    const float gscale = (p.kind == 2 ? 2.0f : 1.0f) * p.weight / (float)((int64_t)p.N * p.H * p.W);
    int b = blockIdx.x;
    const int tj = b % p.tiles_j; b /= p.tiles_j;
    const int ti = b % p.tiles_i;
    const int n = b / p.tiles_i;
    const int m = n >= p.N / 2 ? n - p.N / 2 : n + p.N / 2;
    const int i0 = ti * OC_TILE, j0 = tj * OC_TILE;
    const int64_t plane = (int64_t)p.H * p.W;
    const float* img = HEAD ? p.src + (int64_t)n * plane * C : nullptr;
    const float* partner = p.flow + (int64_t)m * plane * p.flow_ld;
    double sums[OC_SUMS] = {0.0, 0.0, 0.0, 0.0};
    // ---- A: all loads first (clamped indices, no branches), then the LDS writes
    {
        float f0_[4], f1_[4], av[4][C];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = min(i0 + hi + 8 * k, p.H - 1), j = min(j0 + lo, p.W - 1);
            const int64_t pix = ((int64_t)n * p.H + i) * p.W + j;
            const float* fl = p.flow + pix * p.flow_ld;
            f0_[k] = fl[0]; f1_[k] = fl[1];
            if (HEAD) {
#pragma unroll
                for (int c = 0; c < C; ++c) av[k][c] = p.tgt[pix * p.tgt_ld + c];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = hi + 8 * k, i = i0 + r, j = j0 + lo;
            s_f[0][r * P + lo] = f0_[k]; s_f[1][r * P + lo] = f1_[k];
            if (HEAD) {
#pragma unroll
                for (int c = 0; c < C; ++c) s_c[c][r * P + lo] = av[k][c];
                if (p.warp && i < p.H && j < p.W) {
                    const int64_t pix = ((int64_t)n * p.H + i) * p.W + j;
                    p.warp[pix * 2] = f0_[k] + (float)i; p.warp[pix * 2 + 1] = f1_[k] + (float)j;
                }
            }
        }
    }
    __syncthreads();
    // ---- B: every tap of a thread's four pixels is requested before any of them is used
    {
        float tp[4][4][C];          // [pixel][ff, cc, fc, cf][channel]
        float2 pt[4][4];            // the partner flow at the same four taps
        float f0s[4], f1s[4], dxs[4], dys[4];
        bool vld[4], ins[4], okt[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q = hi + 8 * k;
            const float f0 = s_f[0][lo * P + q], f1 = s_f[1][lo * P + q];
            const float x = f0 + (float)min(i0 + lo, p.H - 1), y = f1 + (float)min(j0 + q, p.W - 1);
            f0s[k] = f0; f1s[k] = f1;
            ins[k] = x >= 0.0f && y >= 0.0f && x <= p.xmax && y <= p.ymax;             // a NaN fails every comparison
            vld[k] = x > -1.0f && y > -1.0f && x < (float)p.W && y < (float)p.H;
            const float fxf = floorf(x), fyf = floorf(y);
            // the clamp keeps the int conversion defined for far-away / non-finite sample points (they are neither valid nor inside)
            const int fx = (int)fminf(fmaxf(fxf, -2.0f), (float)p.W), fy = (int)fminf(fmaxf(fyf, -2.0f), (float)p.H);
            const int cx = fx + 1, cy = fy + 1;
            dxs[k] = (fxf + 1.0f) - x; dys[k] = (fyf + 1.0f) - y;
            const int xs[4] = {fx, cx, fx, cx}, ys[4] = {fy, cy, cy, fy};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                okt[k][t] = ins[k] && xs[t] < p.W && ys[t] < p.H;                       // index W or H: weight 0, reads 0
                const int xc = min(max(xs[t], 0), p.W - 1), yc = min(max(ys[t], 0), p.H - 1);   // an address is only formed from clamped indices
                pt[k][t] = oc_load(partner + ((int64_t)yc * p.W + xc) * p.flow_ld, p.flow_vec);
            }
            if (HEAD) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    tp[k][0][c] = oc_tap(img, p.W, p.H, C, fy, fx, c); tp[k][1][c] = oc_tap(img, p.W, p.H, C, cy, cx, c);
                    tp[k][2][c] = oc_tap(img, p.W, p.H, C, cy, fx, c); tp[k][3][c] = oc_tap(img, p.W, p.H, C, fy, cx, c);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = lo, q = hi + 8 * k;
            const bool inr = i0 + r < p.H && j0 + q < p.W;
            const float dx = dxs[k], dy = dys[k], f0 = f0s[k], f1 = f1s[k];
            // the mask
            float2 t[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] = okt[k][e] ? pt[k][e] : make_float2(0.f, 0.f);
            const float w0 = dx * dy, w1 = (1.0f - dx) * (1.0f - dy), w2 = dx * (1.0f - dy), w3 = (1.0f - dx) * dy;
            const float s0 = ((w0 * t[0].x + w1 * t[1].x) + w2 * t[2].x) + w3 * t[3].x;
            const float s1 = ((w0 * t[0].y + w1 * t[1].y) + w2 * t[2].y) + w3 * t[3].y;
            const float r0 = f0 + s1, r1 = f1 + s0;
            const float lhs = r0 * r0 + r1 * r1;
            const float rhs = p.alpha1 * ((f0 * f0 + f1 * f1) + (s0 * s0 + s1 * s1)) + p.alpha2;
            const bool inside = ins[k];
            const bool visible = inside && lhs < rhs;
            const float mk = inside ? (visible ? 1.0f : 0.0f) : (p.outside_visible ? 1.0f : 0.0f);
            s_m[r * P + q] = mk;
            if (inr) {
                sums[1] += visible ? 1.0 : 0.0;
                sums[2] += (inside && !visible) ? 1.0 : 0.0;
                sums[3] += inside ? 0.0 : 1.0;
            }
            if (HEAD) {
                const bool valid = vld[k];
                float gx = 0.f, gy = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float iff = valid ? tp[k][0][c] : 0.f, icc = valid ? tp[k][1][c] : 0.f;
                    const float ifc = valid ? tp[k][2][c] : 0.f, icf = valid ? tp[k][3][c] : 0.f;
                    const float v = valid ? ((dx * dy * iff + (1.0f - dx) * (1.0f - dy) * icc) + dx * (1.0f - dy) * ifc) + (1.0f - dx) * dy * icf : 0.f;
                    const float d = (v - s_c[c][r * P + q]) * mk;
                    float g;
                    if (p.kind == 2) { sums[0] += inr ? (double)(d * d) : 0.0; g = d * mk * gscale; }
                    else { sums[0] += inr ? (double)fabsf(d) : 0.0; g = ((d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f)) * mk * gscale; }
                    s_c[c][r * P + q] = v;                                              // gen goes out unmasked
                    const float tx = g * (dy * (icf - iff) + (1.0f - dy) * (icc - ifc));
                    const float ty = g * (dx * (ifc - iff) + (1.0f - dx) * (icc - icf));
                    gx += valid ? tx : 0.f;
                    gy += valid ? ty : 0.f;
                }
                s_f[0][r * P + q] = gx; s_f[1][r * P + q] = gy;
            }
        }
    }
    __syncthreads();
    // ---- C
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = hi + 8 * k, i = i0 + r, j = j0 + lo;
        if (i < p.H && j < p.W) {
            const int64_t pix = ((int64_t)n * p.H + i) * p.W + j;
            if (HEAD) {
#pragma unroll
                for (int c = 0; c < C; ++c) p.gen[pix * C + c] = s_c[c][r * P + lo];
                if (p.dflow) { p.dflow[pix * p.dflow_ld] = s_f[0][r * P + lo]; p.dflow[pix * p.dflow_ld + 1] = s_f[1][r * P + lo]; }
            }
            if (p.mask) p.mask[pix * p.mask_ld] = s_m[r * P + lo];
        }
    }
    if (!p.part) return;                                    // uniform over the workgroup
    block_sum(sums, s_red, threadIdx.x);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < OC_SUMS; ++q) p.part[OC_SUMS * (int64_t)blockIdx.x + q] = block_total(s_red, q);
    }
}

// One workgroup: the tiles' sums in index order, then the loss word and / or the three shares.
__global__ __launch_bounds__(OC_THREADS) void occl_final_kernel(const OcclParams p) {
    __shared__ double s_red[OC_SUMS * 4];
    double s[OC_SUMS] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t t = threadIdx.x; t < p.n_tiles; t += OC_THREADS)
#pragma unroll
        for (int q = 0; q < OC_SUMS; ++q) s[q] += p.part[t * OC_SUMS + q];
    block_sum(s, s_red, threadIdx.x);
    if (threadIdx.x != 0) return;
    if (p.stats) {
#pragma unroll
        for (int q = 1; q < OC_SUMS; ++q) p.stats[q - 1] = (float)(block_total(s_red, q) / p.npix);
    }
    if (p.loss) {
        const float t = (float)((double)p.weight * (block_total(s_red, 0) / p.npix));
        p.loss[0] = p.overwrite ? t : p.loss[0] + t;
    }
}

template <bool HEAD>
void launch_occl_tile(const OcclParams& p, int C, int blocks, hipStream_t s) {
    if (!HEAD) { occl_tile_kernel<false, 1><<<blocks, OC_THREADS, 0, s>>>(p); return; }
    switch (C) {
        case 1: occl_tile_kernel<true, 1><<<blocks, OC_THREADS, 0, s>>>(p); break;
        case 2: occl_tile_kernel<true, 2><<<blocks, OC_THREADS, 0, s>>>(p); break;
        case 3: occl_tile_kernel<true, 3><<<blocks, OC_THREADS, 0, s>>>(p); break;
        default: occl_tile_kernel<true, 4><<<blocks, OC_THREADS, 0, s>>>(p); break;
    }
}

// 0 when the shape is outside what the entries take
int64_t oc_tile_count(int N, int H, int W) {
    if (N < 2 || (N & 1) || H != W || H < 2 || H > IMG_MAX_SIDE) return 0;
    return image_tile_count(N, H, W, OC_TILE, OC_TILE);
}

// the checks both entries share, in the order of mv3d_flow_consistency
int oc_check_shape(const char* fn, int N, int H, int W, int64_t* total) {
    if (N < 2 || (N & 1)) return fail(MV3D_E_INVAL, "%s: N (%d) must be even and at least 2 (the second half holds the reversed pairs)", fn, N);
    if (H != W) return fail(MV3D_E_INVAL, "%s: H (%d) and W (%d) differ (the transposed sampler convention needs square images)", fn, H, W);
    if (H < 2) return fail(MV3D_E_INVAL, "%s: H (%d) must be at least 2", fn, H);
    if (H > IMG_MAX_SIDE) return fail(MV3D_E_INVAL, "%s: H (%d) above %d", fn, H, IMG_MAX_SIDE);
    *total = oc_tile_count(N, H, W);
    if (!*total) return fail_tiles(fn, N, H, W);
    return MV3D_OK;
}
int oc_check_alphas(const char* fn, float alpha1, float alpha2, int outside_visible) {
    if (!std::isfinite(alpha1) || alpha1 < 0.f) return fail(MV3D_E_INVAL, "%s: alpha1 (%g) must be finite and >= 0", fn, (double)alpha1);
    if (int rc = check_finite(fn, "alpha2", alpha2, true)) return rc;
    if (outside_visible != 0 && outside_visible != 1) return fail(MV3D_E_INVAL, "%s: outside_visible (%d) must be 0 or 1", fn, outside_visible);
    return MV3D_OK;
}

void oc_fill(OcclParams& p, int N, int H, int W, const void* flow, int flow_ld, float alpha1, float alpha2, int outside_visible,
             int64_t total) {
    p.flow = (const float*)flow;
    p.N = N; p.H = H; p.W = W; p.flow_ld = flow_ld;
    p.alpha1 = alpha1; p.alpha2 = alpha2; p.outside_visible = outside_visible;
    p.flow_vec = (flow_ld % 2 == 0 && ((uintptr_t)flow & 7) == 0) ? 1 : 0;
    p.xmax = (float)(W - 1);
    p.ymax = (float)(H - 1);
    p.tiles_i = cdiv(H, OC_TILE); p.tiles_j = cdiv(W, OC_TILE);
    p.n_tiles = total;
    p.npix = (double)N * (double)H * (double)W;
}

}  // namespace
}  // namespace mv3d

using namespace mv3d;

extern "C" {

size_t mv3d_flow_occlusion_mask_workspace_bytes(int N, int H, int W) {
    const int64_t total = oc_tile_count(N, H, W);
    return total ? tile_workspace_bytes(total, OC_SUMS) : 0;
}

int mv3d_flow_occlusion_mask(int N, int H, int W, const void* flow, int flow_ld, float alpha1, float alpha2, int outside_visible,
                             void* mask_out, int mask_ld, void* stats, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mv3d_flow_occlusion_mask";
    int64_t total = 0;
    if (int rc = oc_check_shape(fn, N, H, W, &total)) return rc;
    if (flow_ld < 2) return fail(MV3D_E_INVAL, "%s: flow_ld (%d) smaller than 2", fn, flow_ld);
    if (mask_ld < 1) return fail(MV3D_E_INVAL, "%s: mask_ld (%d) smaller than 1", fn, mask_ld);
    {   // the largest element index of any operand, formed in int64 by the kernel
        const int ld = flow_ld > mask_ld ? flow_ld : mask_ld;
        if ((double)N * (double)H * (double)W * (double)ld >= 4.0e18)
            return fail(MV3D_E_INVAL, "%s: N (%d) images of %d x %d at pixel stride %d overflow the element index", fn, N, H, W, ld);
    }
    if (int rc = oc_check_alphas(fn, alpha1, alpha2, outside_visible)) return rc;
    if (int rc = check_not_null(fn, {{"flow", flow}})) return rc;
    if (!mask_out && !stats) return fail(MV3D_E_INVAL, "%s: mask_out and stats are both null", fn);
    if (((uintptr_t)flow | (uintptr_t)mask_out | (uintptr_t)stats) & 3)
        return fail(MV3D_E_INVAL, "%s: flow, mask_out or stats not 4-byte aligned", fn);
    if (stats) {        // the workspace holds the tiles' counts: only a call with stats needs one
        if (int rc = check_buffers(fn, "flow, mask_out or stats", 0, workspace, workspace_bytes, tile_workspace_bytes(total, OC_SUMS))) return rc;
    }

    OcclParams p = {};
    oc_fill(p, N, H, W, flow, flow_ld, alpha1, alpha2, outside_visible, total);
    p.mask = (float*)mask_out; p.mask_ld = mask_ld;
    p.stats = (float*)stats;
    p.part = stats ? (double*)workspace : nullptr;

    const double px = p.npix;
    // algorithmic bytes: the flow once as itself and once as a partner, the mask written.  FLOPs per pixel: the bilinear sample of
    // two channels ~22, the residual and the two sides of the test ~16.
    const OpInfo info{intern_label("occl_mask"), px * 38.0, px * (16.0 + (mask_out ? 4.0 : 0.0)) + (stats ? (double)total * 32.0 : 0.0)};
    const int grid = (int)total;
    int rc = dispatch(stream, info, [=](hipStream_t s) {
        launch_occl_tile<false>(p, 1, grid, s);
        return launched("occl_tile_kernel<mask>");
    });
    if (rc || !stats) return rc;
    const OpInfo final_info{intern_label("occl_mask_stats"), 0.0, (double)total * 32.0 + 12.0};
    return dispatch(stream, final_info, [=](hipStream_t s) {
        occl_final_kernel<<<1, OC_THREADS, 0, s>>>(p);
        return launched("occl_final_kernel<mask>");
    });
}

size_t mv3d_warp_resample_occlusion_loss_workspace_bytes(int N, int H, int W) {
    return mv3d_flow_occlusion_mask_workspace_bytes(N, H, W);
}

int mv3d_warp_resample_occlusion_loss(int N, int H, int W, int Hs, int Ws, int C, const void* src, const void* flow, int flow_ld,
                                      const void* target, int target_ld, int kind, float weight, float alpha1, float alpha2,
                                      int outside_visible, void* warp_out, void* gen, void* dflow, int dflow_ld, void* mask_out,
                                      int mask_ld, void* loss_accum, void* stats, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mv3d_warp_resample_occlusion_loss";
    int64_t total = 0;
    if (int rc = oc_check_shape(fn, N, H, W, &total)) return rc;
    if (Hs != H || Ws != W)
        return fail(MV3D_E_INVAL, "%s: the source (%d x %d) must have the size of the flow (%d x %d): the partner flow is sampled where the image is", fn, Hs, Ws, H, W);
    if (C < 1 || C > 4) return fail(MV3D_E_INVAL, "%s: C (%d) outside 1..4", fn, C);
    if (flow_ld < 2) return fail(MV3D_E_INVAL, "%s: flow_ld (%d) smaller than 2", fn, flow_ld);
    if (target_ld < C) return fail(MV3D_E_INVAL, "%s: target_ld (%d) smaller than C (%d)", fn, target_ld, C);
    if (dflow && dflow_ld < 2) return fail(MV3D_E_INVAL, "%s: dflow_ld (%d) smaller than 2", fn, dflow_ld);
    if (mask_out && mask_ld < 1) return fail(MV3D_E_INVAL, "%s: mask_ld (%d) smaller than 1", fn, mask_ld);
    {
        int ld = std::max(std::max(flow_ld, target_ld), std::max(dflow ? dflow_ld : 0, mask_out ? mask_ld : 0));
        if ((double)N * (double)H * (double)W * (double)ld >= 4.0e18)
            return fail(MV3D_E_INVAL, "%s: N (%d) images of %d x %d at pixel stride %d overflow the element index", fn, N, H, W, ld);
    }
    if (kind != 1 && kind != 2) return fail(MV3D_E_INVAL, "%s: kind (%d) must be 1 (l1) or 2 (euclidean)", fn, kind);
    if (int rc = check_finite(fn, "weight", weight, false)) return rc;
    if (int rc = oc_check_alphas(fn, alpha1, alpha2, outside_visible)) return rc;
    if (int rc = check_not_null(fn, {{"src", src}, {"flow", flow}, {"target", target}, {"gen", gen}, {"loss_accum", loss_accum}})) return rc;
    if (int rc = check_buffers(fn, "src, flow, target, warp_out, gen, dflow, mask_out, loss_accum or stats",
                               (uintptr_t)src | (uintptr_t)flow | (uintptr_t)target | (uintptr_t)warp_out | (uintptr_t)gen | (uintptr_t)dflow |
                                   (uintptr_t)mask_out | (uintptr_t)loss_accum | (uintptr_t)stats,
                               workspace, workspace_bytes, tile_workspace_bytes(total, OC_SUMS))) return rc;

    OcclParams p = {};
    oc_fill(p, N, H, W, flow, flow_ld, alpha1, alpha2, outside_visible, total);
    p.src = (const float*)src; p.tgt = (const float*)target; p.tgt_ld = target_ld;
    p.warp = (float*)warp_out; p.gen = (float*)gen; p.dflow = (float*)dflow; p.dflow_ld = dflow_ld;
    p.mask = (float*)mask_out; p.mask_ld = mask_ld;
    p.loss = (float*)loss_accum; p.stats = (float*)stats;
    p.part = (double*)workspace;
    p.kind = kind; p.weight = weight;
    p.overwrite = take_loss_overwrite() ? 1 : 0;           // mv3d_loss_overwrite_next(): consumed here (kept by a recorded call)

    const double px = p.npix;
    // algorithmic bytes: flow as itself and as a partner, target, the four image taps' worth of source, gen, dflow, warp_pts, mask
    const OpInfo tile_info{intern_label("occl_head_tile"), px * (38.0 + 30.0 * C),
                           px * (16.0 + 8.0 * C + 4.0 * C + (dflow ? 8.0 : 0.0) + (warp_out ? 8.0 : 0.0) + (mask_out ? 4.0 : 0.0)) + (double)total * 32.0};
    const int grid = (int)total;
    int rc = dispatch(stream, tile_info, [=](hipStream_t s) {
        launch_occl_tile<true>(p, C, grid, s);
        return launched("occl_tile_kernel<head>");
    });
    if (rc) return rc;
    const OpInfo final_info{intern_label("occl_head_final"), 0.0, (double)total * 32.0 + 16.0};
    return dispatch(stream, final_info, [=](hipStream_t s) {
        occl_final_kernel<<<1, OC_THREADS, 0, s>>>(p);
        return launched("occl_final_kernel<head>");
    });
}

}  // extern "C"
