// Multi-scale (coarse-to-fine) photometric loss of a flow: value and gradient with respect to the full-resolution flow.
//
// For level l = 1..L, f = 2^l.  pool_l halves level l-1 (level 0 = the input) in fp32: 0.25 * ((p00 + p01) + (p10 + p11)) of the
// 2 x 2 block p00 p01 / p10 p11 (row-major); it applies to src, to target and to both channels of the flow.
//   flow_l = pool_l(flow) * (1 / f)                          (exact: a power of two)
//   warp_l[n,I,J] = flow_l[n,I,J] + (I, J)                   channel 0 + ROW index, read by the sampler as x (column); channel 1 +
//                                                            column index, read as y (row): the transposed convention of
//                                                            mv3d_warp_resample_* (SURVEY A.3/A.4).  Pooling with aligned pixel centres
//                                                            maps x to (x - (f-1)/2) / f, so the block mean IS the coarse flow
//   gen_l  = resample(pool_l(src), warp_l), zero outside     valid iff -1 < x < Ws/f and -1 < y < Hs/f; the expressions of resample_kernel
//   T_l    = mean over (n,I,J) of sum_c phi(gen_l - pool_l(target)),   phi = square (kind 2) or absolute value (kind 1)
//   term   = sum_l w_l T_l
//   d term / d flow[n,i,j,k] = sum_l w_l G_l[n, i >> l, j >> l, k] / f^3,   G_l = d T_l / d warp_l (the sampler's warp gradient);
//                              1 / f^2 from the block mean, 1 / f from the scaling.  src and target are not differentiated.
//
// Built with -ffp-contract=off: every step is fp32 in the order of the numpy twin (metrics.py multiscale_warp_loss_host at
// float32).  s_l = w_l k / (N H_l W_l) / f^3 (k = 2 for the square, 1 for the absolute value) is formed in double and rounded to
// fp32 once; a coarse pixel's dgen is d * s_l (or sign(d) * s_l), its warp gradient adds the channels in index order, and a
// full-resolution pixel adds its levels' contributions in level order before the one addition onto what grad holds.  Only the
// sums behind T_l are kept in double, in a fixed order.  gen_l == pool_l(target) gives d == 0: value and gradient exactly 0.
//
// Three launches, no atomics, no device state outside the caller's workspace:
//   pyramid  one workgroup of 256 per 32 x 32 tile of src or of target (one grid over both).  Lanes run along the (column,
//            channel) index of level 1, so a row pair is read as contiguous segments; level 1 is kept in LDS and halved into
//            levels 2 and 3 there.  Every level goes to the workspace as a dense [N, H/f, W/f, C] image.  Skipped with pyramid_ready.
//   tile     one workgroup per 32 x 32 tile of the flow.  A: the flow tile into LDS, lanes along columns.  B: halved in LDS, one
//            thread per coarse pixel: 256, 64, 16.  C: the tile's at most 336 coarse pixels are evaluated, lanes along coarse ROWS
//            (the sampler's x): four taps from the pooled src, the difference against the pooled target, phi into the level's
//            sum, the scaled warp gradient into LDS.  D: every flow pixel adds its levels from LDS and writes (or adds to) its
//            two gradient channels: one writer per element, the flow read and grad touched once whatever L is.
//   final    one workgroup adds the tiles' three sums in a fixed order, writes T_l and adds (or stores) the term.
// H and W are multiples of 2^L and tile origins multiples of 32, so a coarse block lies wholly inside the image or wholly outside.
//
// The masked form (mv3d_multiscale_warp_loss_masked, MASKED = true) weighs every coarse pixel by a mask m [N,H,W,1] over the flow's
// grid that is not differentiated: m_l = pool_l(m), the same pooling, so a coarse pixel counts by its visible share and a 0/1 mask
// pools exactly.  T_l = (1 / (N H_l W_l)) sum m_l sum_c phi(d_c), the count unchanged; a coarse pixel's channel sum is formed in
// double as before and the level sum adds (double)m_l * s; the scaled dgen becomes (d * s_l) * m_l (or (sign(d) * s_l) * m_l), the
// mask multiplying last.  Everything behind it is the unmasked code: m == 1 gives the unmasked bits, m == 0 gives +0 and zeros.
// The mask lies on the flow's grid, which the tile kernel already stages and halves: stage A loads the mask tile beside the flow
// tile, stage B halves it beside the flow, stage C reads m_l from LDS (4096 + 1344 B more).  The pyramid launch and the workspace
// know nothing of it; a call with pyramid_ready pools the mask again from its 4 B per pixel.
#include "image_common.h"

namespace mv3d {
namespace {

constexpr int MS_TILE = 32;
constexpr int MS_THREADS = IMG_THREADS;
constexpr int MS_LEVELS = 3;                                // most levels: 32 / 2^3 = 4 coarse pixels per tile side
constexpr int MS_L1 = 16, MS_L2 = 8, MS_L3 = 4;             // coarse pixels per tile side
constexpr int MS_OFF2 = MS_L1 * MS_L1, MS_OFF3 = MS_OFF2 + MS_L2 * MS_L2, MS_COARSE = MS_OFF3 + MS_L3 * MS_L3;      // 256, 320, 336

struct MsArgs {
    const float* src; const float* flow; const float* target; const float* mask;    // mask: the masked form only
    float* psrc[MS_LEVELS]; float* ptgt[MS_LEVELS];         // the pyramids in the workspace, dense
    double* part; float* loss; float* level_values; float* grad;
    int N, H, W, Hs, Ws, levels, kind, src_ld, flow_ld, target_ld, mask_ld, grad_ld, accumulate, overwrite, flow_vec, grad_vec;
    int tx, ty, sx, sy, src_tiles;                          // tiles of the flow / target, of src, N * sx * sy
    float gscale[MS_LEVELS];                                // s_l
    double weight[MS_LEVELS], count[MS_LEVELS];             // w_l, N H_l W_l
};

__device__ __forceinline__ float pool4(float p00, float p01, float p10, float p11) { return 0.25f * ((p00 + p01) + (p10 + p11)); }

// one level from the one below, both in LDS: out[r][q][c] over an n x n tile from in (2n x 2n)
template <int C>
__device__ __forceinline__ void ms_halve_image(const float* in, float* out, int n, float* dst, int Hl, int Wl, int img_n, int y0, int x0) {
    for (int idx = threadIdx.x; idx < n * n * C; idx += MS_THREADS) {
        const int r = idx / (n * C), rem = idx - r * (n * C), q = rem / C, c = rem - q * C;
        const float* a = in + ((2 * r) * (2 * n) + 2 * q) * C + c;
        const float v = pool4(a[0], a[C], a[2 * n * C], a[2 * n * C + C]);
        out[idx] = v;
        const int y = y0 + r, x = x0 + q;                   // coarse coordinates
        if (y < Hl && x < Wl) dst[(((int64_t)img_n * Hl + y) * Wl + x) * C + c] = v;
    }
}

template <int C>
__global__ __launch_bounds__(MS_THREADS) void ms_pyramid_kernel(const MsArgs p) {
    __shared__ float s1[MS_L1 * MS_L1 * C], s2[MS_L2 * MS_L2 * C], s3[MS_L3 * MS_L3 * C];
    const bool tgt = (int)blockIdx.x >= p.src_tiles;
    const int b = tgt ? blockIdx.x - p.src_tiles : blockIdx.x;
    const float* img = tgt ? p.target : p.src;
    const int ld = tgt ? p.target_ld : p.src_ld, Hi = tgt ? p.H : p.Hs, Wi = tgt ? p.W : p.Ws;
    const int tw = tgt ? p.tx : p.sx, th = tgt ? p.ty : p.sy;
    const int n = b / (tw * th), t = b - n * (tw * th);
    const int y0 = (t / tw) * MS_TILE, x0 = (t % tw) * MS_TILE;
    float* const* out = tgt ? p.ptgt : p.psrc;
    const int H1 = Hi >> 1, W1 = Wi >> 1;
    for (int idx = threadIdx.x; idx < MS_L1 * MS_L1 * C; idx += MS_THREADS) {
        const int r = idx / (MS_L1 * C), rem = idx - r * (MS_L1 * C), q = rem / C, c = rem - q * C;
        const int y = y0 + 2 * r, x = x0 + 2 * q;
        float v = 0.f;
        if (y < Hi && x < Wi) {                             // Hi, Wi even: the whole block is inside
            const float* a = img + (((int64_t)n * Hi + y) * Wi + x) * ld + c;
            const int64_t row = (int64_t)Wi * ld;
            v = pool4(a[0], a[ld], a[row], a[row + ld]);
            out[0][(((int64_t)n * H1 + (y >> 1)) * W1 + (x >> 1)) * C + c] = v;
        }
        s1[idx] = v;
    }
    __syncthreads();
    if (p.levels >= 2) ms_halve_image<C>(s1, s2, MS_L2, out[1], Hi >> 2, Wi >> 2, n, y0 >> 2, x0 >> 2);
    __syncthreads();
    if (p.levels >= 3) ms_halve_image<C>(s2, s3, MS_L3, out[2], Hi >> 3, Wi >> 3, n, y0 >> 3, x0 >> 3);
}

__device__ __forceinline__ float2 pool4(float2 a, float2 b, float2 c, float2 d) {
    return make_float2(pool4(a.x, b.x, c.x, d.x), pool4(a.y, b.y, c.y, d.y));
}

// One bilinear tap of a dense C-channel image: the load is unconditional from a clamped address, the bounds test selects.
template <int C>
__device__ __forceinline__ void ms_tap(const float* img, int Ws, int Hs, int y, int x, float (&v)[C]) {
    const bool ok = (unsigned)x < (unsigned)Ws && (unsigned)y < (unsigned)Hs;
    const int xc = min(max(x, 0), Ws - 1), yc = min(max(y, 0), Hs - 1);
    const float* a = img + ((int64_t)yc * Ws + xc) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) { const float t = a[c]; v[c] = ok ? t : 0.f; }
}

template <int C, bool MASKED>
__global__ __launch_bounds__(MS_THREADS) void ms_loss_tile_kernel(const MsArgs p) {
    __shared__ float2 s_f0[MS_TILE * MS_TILE];              // the flow tile
    __shared__ float2 s_f[MS_COARSE];                       // its levels 1, 2, 3 at 0, 256, 320
    __shared__ float s_m0[MASKED ? MS_TILE * MS_TILE : 1];  // the mask tile and its levels, laid out like s_f0 and s_f; the
    __shared__ float s_m[MASKED ? MS_COARSE : 1];           // unmasked kernel never names them
    __shared__ float2 s_g[MS_COARSE];                       // the scaled warp gradients, same layout
    __shared__ double s_red[MS_LEVELS * (MS_THREADS / 64)];
    const int tiles = p.tx * p.ty;
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int i0 = (t / p.tx) * MS_TILE, j0 = (t % p.tx) * MS_TILE;
    const int tid = threadIdx.x, lo = tid & 31, hi = tid >> 5;
    const int64_t img = (int64_t)n * p.H * p.W;
    const bool want_value = p.loss != nullptr, want_grad = p.grad != nullptr;

    // ---- A: the flow tile, zeros outside the image (they only reach coarse pixels that are dropped)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = hi + 8 * k, i = i0 + r, j = j0 + lo;
        float2 f = make_float2(0.f, 0.f);
        if (i < p.H && j < p.W) {
            const float* a = p.flow + (img + (int64_t)i * p.W + j) * p.flow_ld;
            if (p.flow_vec) f = *reinterpret_cast<const float2*>(a);
            else { f.x = a[0]; f.y = a[1]; }
        }
        s_f0[r * MS_TILE + lo] = f;
        if constexpr (MASKED) {
            float m = 0.f;
            if (i < p.H && j < p.W) m = p.mask[(img + (int64_t)i * p.W + j) * p.mask_ld];
            s_m0[r * MS_TILE + lo] = m;
        }
    }
    __syncthreads();
    // ---- B: halved three times, one thread per coarse pixel
    {
        const int r = tid >> 4, q = tid & 15;
        const float2* a = s_f0 + (2 * r) * MS_TILE + 2 * q;
        s_f[tid] = pool4(a[0], a[1], a[MS_TILE], a[MS_TILE + 1]);
        if constexpr (MASKED) {
            const float* m = s_m0 + (2 * r) * MS_TILE + 2 * q;
            s_m[tid] = pool4(m[0], m[1], m[MS_TILE], m[MS_TILE + 1]);
        }
    }
    __syncthreads();
    if (tid < MS_L2 * MS_L2) {
        const int r = tid >> 3, q = tid & 7;
        const float2* a = s_f + (2 * r) * MS_L1 + 2 * q;
        s_f[MS_OFF2 + tid] = pool4(a[0], a[1], a[MS_L1], a[MS_L1 + 1]);
        if constexpr (MASKED) {
            const float* m = s_m + (2 * r) * MS_L1 + 2 * q;
            s_m[MS_OFF2 + tid] = pool4(m[0], m[1], m[MS_L1], m[MS_L1 + 1]);
        }
    }
    __syncthreads();
    if (tid < MS_L3 * MS_L3) {
        const int r = tid >> 2, q = tid & 3;
        const float2* a = s_f + MS_OFF2 + (2 * r) * MS_L2 + 2 * q;
        s_f[MS_OFF3 + tid] = pool4(a[0], a[1], a[MS_L2], a[MS_L2 + 1]);
        if constexpr (MASKED) {
            const float* m = s_m + MS_OFF2 + (2 * r) * MS_L2 + 2 * q;
            s_m[MS_OFF3 + tid] = pool4(m[0], m[1], m[MS_L2], m[MS_L2 + 1]);
        }
    }
    __syncthreads();
    // ---- C: the coarse pixels; lanes along coarse rows, which the transposed convention makes the source's columns
    double sums[MS_LEVELS] = {0.0, 0.0, 0.0};
    for (int item = tid; item < MS_COARSE; item += MS_THREADS) {
        const int l = item < MS_OFF2 ? 1 : (item < MS_OFF3 ? 2 : 3);
        if (l > p.levels) continue;
        const int off = l == 1 ? 0 : (l == 2 ? MS_OFF2 : MS_OFF3), nl = MS_TILE >> l;
        const int k = item - off, r = k & (nl - 1), q = k >> (5 - l);
        const int ci = (i0 >> l) + r, cj = (j0 >> l) + q;
        const int Hl = p.H >> l, Wl = p.W >> l, Hsl = p.Hs >> l, Wsl = p.Ws >> l;
        float2 g = make_float2(0.f, 0.f);
        if (ci < Hl && cj < Wl) {
            const float inv_f = l == 1 ? 0.5f : (l == 2 ? 0.25f : 0.125f);
            const float gscale = l == 1 ? p.gscale[0] : (l == 2 ? p.gscale[1] : p.gscale[2]);
            const float* ps = (l == 1 ? p.psrc[0] : (l == 2 ? p.psrc[1] : p.psrc[2])) + (int64_t)n * Hsl * Wsl * C;
            const float* pt = (l == 1 ? p.ptgt[0] : (l == 2 ? p.ptgt[1] : p.ptgt[2])) + (((int64_t)n * Hl + ci) * Wl + cj) * C;
            const float2 fl = s_f[off + r * nl + q];
            [[maybe_unused]] float ml = 1.f;                // m_l of this coarse pixel
            if constexpr (MASKED) ml = s_m[off + r * nl + q];
            const float x = fl.x * inv_f + (float)ci, y = fl.y * inv_f + (float)cj;
            const bool valid = x > -1.0f && y > -1.0f && x < (float)Wsl && y < (float)Hsl;
            const float fxf = floorf(x), fyf = floorf(y);
            // the clamp keeps the int conversion defined for far-away / non-finite sample points (they are not valid)
            const int fx = (int)fminf(fmaxf(fxf, -2.0f), (float)Wsl), fy = (int)fminf(fmaxf(fyf, -2.0f), (float)Hsl);
            const int cx = fx + 1, cy = fy + 1;
            const float dx = (fxf + 1.0f) - x, dy = (fyf + 1.0f) - y;
            float tff[C], tcc[C], tfc[C], tcf[C], tt[C];
            ms_tap<C>(ps, Wsl, Hsl, fy, fx, tff); ms_tap<C>(ps, Wsl, Hsl, cy, cx, tcc);
            ms_tap<C>(ps, Wsl, Hsl, cy, fx, tfc); ms_tap<C>(ps, Wsl, Hsl, fy, cx, tcf);
#pragma unroll
            for (int c = 0; c < C; ++c) tt[c] = pt[c];
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float iff = valid ? tff[c] : 0.f, icc = valid ? tcc[c] : 0.f, ifc = valid ? tfc[c] : 0.f, icf = valid ? tcf[c] : 0.f;
                const float v = valid ? ((dx * dy * iff + (1.0f - dx) * (1.0f - dy) * icc) + dx * (1.0f - dy) * ifc) + (1.0f - dx) * dy * icf : 0.f;
                const float d = v - tt[c];
                float gc;
                if (p.kind == 2) { s += (double)(d * d); gc = d * gscale; }
                else { s += (double)fabsf(d); gc = ((d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f)) * gscale; }
                if constexpr (MASKED) gc = gc * ml;         // the mask multiplies last
                const float gx = gc * (dy * (icf - iff) + (1.0f - dy) * (icc - ifc));
                const float gy = gc * (dx * (ifc - iff) + (1.0f - dx) * (icc - icf));
                g.x += valid ? gx : 0.f;
                g.y += valid ? gy : 0.f;
            }
            if constexpr (MASKED) s = (double)ml * s;
            if (l == 1) sums[0] += s; else if (l == 2) sums[1] += s; else sums[2] += s;
        }
        s_g[off + r * nl + q] = g;
    }
    if (want_value) block_sum(sums, s_red, tid);            // uniform: either way one barrier, which s_g needs as well
    else __syncthreads();
    if (want_value && tid == 0) {
#pragma unroll
        for (int q = 0; q < MS_LEVELS; ++q) p.part[MS_LEVELS * (int64_t)blockIdx.x + q] = block_total(s_red, q);
    }
    if (!want_grad) return;
    // ---- D: every flow pixel adds its levels in level order; one writer per element
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = hi + 8 * k, i = i0 + r, j = j0 + lo;
        if (i >= p.H || j >= p.W) continue;
        float2 g = s_g[(r >> 1) * MS_L1 + (lo >> 1)];
        if (p.levels >= 2) { const float2 a = s_g[MS_OFF2 + (r >> 2) * MS_L2 + (lo >> 2)]; g.x = g.x + a.x; g.y = g.y + a.y; }
        if (p.levels >= 3) { const float2 a = s_g[MS_OFF3 + (r >> 3) * MS_L3 + (lo >> 3)]; g.x = g.x + a.x; g.y = g.y + a.y; }
        float* dst = p.grad + (img + (int64_t)i * p.W + j) * p.grad_ld;
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

__global__ __launch_bounds__(MS_THREADS) void ms_loss_final_kernel(const MsArgs p) {
    tile_sums_final<MS_LEVELS>(p.part, (int64_t)p.N * p.tx * p.ty, p.loss, p.overwrite, [&](const double (&sum)[MS_LEVELS]) {
        double term = 0.0;
        for (int l = 0; l < p.levels; ++l) {                // level order, in double; rounded once
            const double T = sum[l] / p.count[l];
            if (p.level_values) p.level_values[l] = (float)T;
            term += p.weight[l] * T;
        }
        return (float)term;
    });
}

bool ms_shape_ok(int N, int H, int W, int Hs, int Ws, int C, int levels) {
    if (N < 1 || C < 1 || C > 4 || levels < 1 || levels > MS_LEVELS) return false;
    const int f = 1 << levels;
    for (int v : {H, W, Hs, Ws})
        if (v < f || v % f || v > IMG_MAX_SIDE) return false;
    const int64_t a = image_tile_count(N, H, W, MS_TILE, MS_TILE), b = image_tile_count(N, Hs, Ws, MS_TILE, MS_TILE);
    return a && b && a + b <= INT32_MAX;
}

// the workspace: the tile sums, then src's levels, then target's; every piece 256-byte aligned
struct MsLayout { size_t src[MS_LEVELS], tgt[MS_LEVELS], total; };
MsLayout ms_layout(int N, int H, int W, int Hs, int Ws, int C, int levels) {
    MsLayout m = {};
    size_t at = tile_workspace_bytes(image_tile_count(N, H, W, MS_TILE, MS_TILE), MS_LEVELS);
    auto piece = [&](int h, int w, int l) {
        const size_t here = at;
        at += (size_t)cdiv64((int64_t)N * (h >> l) * (w >> l) * C * (int64_t)sizeof(float), 256) * 256;
        return here;
    };
    for (int l = 1; l <= levels; ++l) m.src[l - 1] = piece(Hs, Ws, l);
    for (int l = 1; l <= levels; ++l) m.tgt[l - 1] = piece(H, W, l);
    m.total = at;
    return m;
}

template <int C>
int ms_launch_pyramid(const MsArgs& p, int grid, hipStream_t s) {
    ms_pyramid_kernel<C><<<grid, MS_THREADS, 0, s>>>(p);
    return launched("ms_pyramid_kernel");
}
template <int C, bool MASKED>
int ms_launch_tile(const MsArgs& p, int grid, hipStream_t s) {
    ms_loss_tile_kernel<C, MASKED><<<grid, MS_THREADS, 0, s>>>(p);
    return launched("ms_loss_tile_kernel");
}

}  // namespace
}  // namespace mv3d

using namespace mv3d;

// Both entries: `mask` is null for mv3d_multiscale_warp_loss (fn names the entry in the messages).
template <bool MASKED>
static int ms_entry(const char* fn, int N, int H, int W, int Hs, int Ws, int C, const void* src, int src_ld, const void* flow, int flow_ld,
                    const void* target, int target_ld, const void* mask, int mask_ld, int levels, const float* level_weights, int kind,
                    void* loss_accum, void* level_values, void* grad, int grad_ld, int grad_accumulate, int pyramid_ready, void* workspace,
                    size_t workspace_bytes, void* stream) {
    if (N < 1) return fail(MV3D_E_INVAL, "%s: N (%d) must be at least 1", fn, N);
    if (C < 1 || C > 4) return fail(MV3D_E_INVAL, "%s: C (%d) outside 1..4", fn, C);
    if (levels < 1 || levels > MS_LEVELS) return fail(MV3D_E_INVAL, "%s: levels (%d) outside 1..%d", fn, levels, MS_LEVELS);
    {
        const int f = 1 << levels, sides[4] = {H, W, Hs, Ws};
        const char* names[4] = {"H", "W", "Hs", "Ws"};
        for (int k = 0; k < 4; ++k) {
            if (sides[k] < f || sides[k] % f)
                return fail(MV3D_E_INVAL, "%s: %s (%d) must be a positive multiple of 2^levels = %d", fn, names[k], sides[k], f);
            if (sides[k] > IMG_MAX_SIDE) return fail(MV3D_E_INVAL, "%s: %s (%d) above %d", fn, names[k], sides[k], IMG_MAX_SIDE);
        }
    }
    if (!ms_shape_ok(N, H, W, Hs, Ws, C, levels)) return fail_tiles(fn, N, H > Hs ? H : Hs, W > Ws ? W : Ws);
    if (src_ld < C) return fail(MV3D_E_INVAL, "%s: src_ld (%d) smaller than C (%d)", fn, src_ld, C);
    if (flow_ld < 2) return fail(MV3D_E_INVAL, "%s: flow_ld (%d) smaller than 2", fn, flow_ld);
    if (target_ld < C) return fail(MV3D_E_INVAL, "%s: target_ld (%d) smaller than C (%d)", fn, target_ld, C);
    if (MASKED && mask_ld < 1) return fail(MV3D_E_INVAL, "%s: mask_ld (%d) smaller than 1", fn, mask_ld);
    if (grad_ld < 2) return fail(MV3D_E_INVAL, "%s: grad_ld (%d) smaller than 2", fn, grad_ld);
    {   // the largest element index of any operand, formed in int64 by the kernels
        int ld = flow_ld > grad_ld ? (flow_ld > target_ld ? flow_ld : target_ld) : (grad_ld > target_ld ? grad_ld : target_ld);
        if (MASKED && mask_ld > ld) ld = mask_ld;
        if ((double)N * (double)H * (double)W * (double)ld >= 4.0e18 || (double)N * (double)Hs * (double)Ws * (double)src_ld >= 4.0e18)
            return fail(MV3D_E_INVAL, "%s: N (%d) images at these pixel strides overflow the element index", fn, N);
    }
    if (kind != 1 && kind != 2) return fail(MV3D_E_INVAL, "%s: kind (%d) must be 1 (absolute value) or 2 (square)", fn, kind);
    if (int rc = check_grad_accumulate(fn, grad_accumulate)) return rc;
    if (pyramid_ready != 0 && pyramid_ready != 1) return fail(MV3D_E_INVAL, "%s: pyramid_ready (%d) must be 0 or 1", fn, pyramid_ready);
    if (int rc = check_not_null(fn, {{"src", src}, {"flow", flow}, {"target", target}, {"level_weights", level_weights}})) return rc;
    if (MASKED)
        if (int rc = check_not_null(fn, {{"mask", mask}})) return rc;
    for (int l = 0; l < levels; ++l)
        if (!std::isfinite(level_weights[l]))
            return fail(MV3D_E_INVAL, "%s: level_weights[%d] (%g) must be finite", fn, l, (double)level_weights[l]);
    if (!loss_accum && !grad) return fail(MV3D_E_INVAL, "%s: loss_accum and grad are both null", fn);
    if (level_values && !loss_accum) return fail(MV3D_E_INVAL, "%s: level_values without loss_accum", fn);
    const MsLayout lay = ms_layout(N, H, W, Hs, Ws, C, levels);
    if (int rc = check_buffers(fn, MASKED ? "src, flow, target, mask, loss_accum, level_values or grad"
                                          : "src, flow, target, loss_accum, level_values or grad",
                               (uintptr_t)src | (uintptr_t)flow | (uintptr_t)target | (uintptr_t)mask | (uintptr_t)loss_accum |
                               (uintptr_t)level_values | (uintptr_t)grad, workspace, workspace_bytes, lay.total)) return rc;

    MsArgs p = {};
    p.src = (const float*)src; p.flow = (const float*)flow; p.target = (const float*)target; p.mask = (const float*)mask;
    p.part = (double*)workspace; p.loss = (float*)loss_accum; p.level_values = (float*)level_values; p.grad = (float*)grad;
    p.N = N; p.H = H; p.W = W; p.Hs = Hs; p.Ws = Ws; p.levels = levels; p.kind = kind;
    p.src_ld = src_ld; p.flow_ld = flow_ld; p.target_ld = target_ld; p.mask_ld = mask_ld; p.grad_ld = grad_ld;
    p.accumulate = grad_accumulate;
    // mv3d_loss_overwrite_next(): consumed by a call that writes the loss word (kept by a recorded one); a gradient-only call
    // is no loss entry and leaves it pending
    p.overwrite = (loss_accum && take_loss_overwrite()) ? 1 : 0;
    p.flow_vec = (flow_ld % 2 == 0 && ((uintptr_t)flow & 7) == 0) ? 1 : 0;
    p.grad_vec = (grad && grad_ld % 2 == 0 && ((uintptr_t)grad & 7) == 0) ? 1 : 0;
    p.tx = cdiv(W, MS_TILE); p.ty = cdiv(H, MS_TILE); p.sx = cdiv(Ws, MS_TILE); p.sy = cdiv(Hs, MS_TILE);
    p.src_tiles = N * p.sx * p.sy;
    double pyr_px = 0.0;                                    // pixels of both pyramids
    for (int l = 1; l <= levels; ++l) {
        p.psrc[l - 1] = (float*)((char*)workspace + lay.src[l - 1]);
        p.ptgt[l - 1] = (float*)((char*)workspace + lay.tgt[l - 1]);
        const double f = (double)(1 << l);
        p.weight[l - 1] = (double)level_weights[l - 1];
        p.count[l - 1] = (double)N * (double)(H >> l) * (double)(W >> l);
        // the twin's constant, formed in double and rounded to fp32 once
        p.gscale[l - 1] = (float)((double)level_weights[l - 1] * (kind == 2 ? 2.0 : 1.0) / p.count[l - 1] / (f * f * f));
        pyr_px += (double)N * ((double)(H >> l) * (W >> l) + (double)(Hs >> l) * (Ws >> l));
    }

    const double px = (double)N * H * W, spx = (double)N * Hs * Ws;
    const int tiles = N * p.tx * p.ty;
    int rc = MV3D_OK;
    if (!pyramid_ready) {
        // algorithmic bytes: src and target read once, every level written once
        const OpInfo info{intern_label("multiscale_pyramid"), pyr_px * C * 4.0, (px + spx + pyr_px) * 4.0 * C};
        const int grid = p.src_tiles + tiles;
        rc = dispatch(stream, info, [=](hipStream_t s) {
            switch (C) {
                case 1: return ms_launch_pyramid<1>(p, grid, s);
                case 2: return ms_launch_pyramid<2>(p, grid, s);
                case 3: return ms_launch_pyramid<3>(p, grid, s);
                default: return ms_launch_pyramid<4>(p, grid, s);
            }
        });
        if (rc) return rc;
    }
    {
        // algorithmic bytes: the flow once, the gradient written once (and read once when it accumulates), both pyramids once, the
        // tile sums (and the mask's 4 B per flow pixel).  FLOPs: 12 per flow pixel to pool and combine, ~(30 + 20 C) per coarse pixel
        const double grad_bytes = grad ? (grad_accumulate ? 16.0 : 8.0) : 0.0;
        const double coarse = px * (levels == 1 ? 0.25 : (levels == 2 ? 0.3125 : 0.328125));
        const OpInfo info{intern_label(MASKED ? "multiscale_loss_masked_tile" : "multiscale_loss_tile"), px * 12.0 + coarse * (30.0 + 20.0 * C),
                          px * (8.0 + grad_bytes + (MASKED ? 4.0 : 0.0)) + pyr_px * 4.0 * C + (loss_accum ? (double)tiles * 24.0 : 0.0)};
        rc = dispatch(stream, info, [=](hipStream_t s) {
            switch (C) {
                case 1: return ms_launch_tile<1, MASKED>(p, tiles, s);
                case 2: return ms_launch_tile<2, MASKED>(p, tiles, s);
                case 3: return ms_launch_tile<3, MASKED>(p, tiles, s);
                default: return ms_launch_tile<4, MASKED>(p, tiles, s);
            }
        });
    }
    if (rc || !loss_accum) return rc;
    const OpInfo final_info{intern_label("multiscale_loss_final"), 0.0, (double)tiles * 24.0 + 8.0 + 4.0 * levels};
    return dispatch(stream, final_info, [=](hipStream_t s) {
        ms_loss_final_kernel<<<1, MS_THREADS, 0, s>>>(p);
        return launched("ms_loss_final_kernel");
    });
}

extern "C" {

size_t mv3d_multiscale_warp_loss_workspace_bytes(int N, int H, int W, int Hs, int Ws, int C, int levels) {
    return ms_shape_ok(N, H, W, Hs, Ws, C, levels) ? ms_layout(N, H, W, Hs, Ws, C, levels).total : 0;
}

int mv3d_multiscale_warp_loss(int N, int H, int W, int Hs, int Ws, int C, const void* src, int src_ld, const void* flow, int flow_ld,
                              const void* target, int target_ld, int levels, const float* level_weights, int kind, void* loss_accum,
                              void* level_values, void* grad, int grad_ld, int grad_accumulate, int pyramid_ready, void* workspace,
                              size_t workspace_bytes, void* stream) {
    return ms_entry<false>("mv3d_multiscale_warp_loss", N, H, W, Hs, Ws, C, src, src_ld, flow, flow_ld, target, target_ld, nullptr, 1, levels,
                           level_weights, kind, loss_accum, level_values, grad, grad_ld, grad_accumulate, pyramid_ready, workspace,
                           workspace_bytes, stream);
}

int mv3d_multiscale_warp_loss_masked(int N, int H, int W, int Hs, int Ws, int C, const void* src, int src_ld, const void* flow, int flow_ld,
                                     const void* target, int target_ld, const void* mask, int mask_ld, int levels,
                                     const float* level_weights, int kind, void* loss_accum, void* level_values, void* grad, int grad_ld,
                                     int grad_accumulate, int pyramid_ready, void* workspace, size_t workspace_bytes, void* stream) {
    return ms_entry<true>("mv3d_multiscale_warp_loss_masked", N, H, W, Hs, Ws, C, src, src_ld, flow, flow_ld, target, target_ld, mask, mask_ld,
                          levels, level_weights, kind, loss_accum, level_values, grad, grad_ld, grad_accumulate, pyramid_ready, workspace,
                          workspace_bytes, stream);
}

}  // extern "C"
