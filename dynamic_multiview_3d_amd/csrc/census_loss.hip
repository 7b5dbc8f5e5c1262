// The soft census (ternary) loss of Meister et al. ("UnFlow") / Liu et al. ("DDFlow") between a prediction a and a target b, and
// its gradient with respect to a.
//
// a, b [N,H,W,C], C in 1..4; radius r in {1, 2, 3}; K = (2r+1)^2 - 1 offsets o of the (2r+1)^2 patch, centre excluded, row-major
// (dy outer, dx inner); Hv = H - 2r, Wv = W - 2r; a pixel is valid when its whole patch is inside the image.
//   g_x(p)   = (255 / max_val) (1/C) sum_c x(p,c)        intensity on the 0..255 scale: the constants mean what they mean in the
//                                                        literature
//   d_x(p,o) = g_x(p+o) - g_x(p)       R_x(p,o) = sqrt(0.81 + d_x^2)       t_x(p,o) = d_x / R_x
//   u(p,o)   = t_a - t_b               e = u^2
//   dist(p)  = (1/K) sum_o e / (0.1 + e)                 in [0, 1)
//   root(p)  = sqrt(dist + eps^2)      rho(p) = dist / (root + eps)        the Charbonnier penalty root - eps, written so that
//                                                                          dist == 0 gives exactly 0 whatever the rounding
//   census_loss = (1 / (N Hv Wv)) sum over n and the valid p of rho(p)
// Gradient:
//   phi(p,o) = [0.1 / (0.1 + e)^2] 2 u 0.81 / R_a^3      rho'(p) = 1 / (2 root(p))
//   dL/dg_a(q) = (1 / (K N Hv Wv)) ( sum_{o : q-o valid} rho'(q-o) phi(q-o, o) - [q valid] rho'(q) sum_o phi(q, o) )
//   grad(q,c)  = weight (255 / (max_val C)) dL/dg_a(q)   the same for every channel c
// Pixels outside the valid region still receive a gradient as neighbours.  a == b gives a loss of exactly 0 and a gradient of
// exactly 0, because u == 0.
//
// The kernel gathers: t is odd in d, so phi(q-o, o) == -phi(q, -o) exactly, and with o' = -o the first sum of the bracket is
// -sum_o' rho'(q+o') [q+o' valid] phi(q, o'): one K-loop per output pixel gives both sums once rho' is known on the tile plus a
// halo of r.  Built with -ffp-contract=off: every step is fp32 in the order of the numpy twin (metrics.py census_loss_host at
// float32, which states the order; o' running row-major is the twin's reverse offset order), sqrt and division correctly rounded.
// Only the sum of rho is kept in double, in a fixed order.
//
// Two launches, no atomics, no device state outside the caller's workspace:
//   tile    one workgroup of 256 per 32x32 PIXEL tile of one image, so that every gradient element has exactly one writer.  It
//           stages g_a and g_b of the tile plus a halo of 2r in LDS (0 outside the image, which only reaches terms whose
//           coefficient is 0).  Pass 1: every valid pixel of the tile gets dist, adds rho to its thread's double partial and, when
//           a gradient is asked for, leaves rho' in LDS; then the ring of r around the tile gets rho' the same way (0 for a pixel
//           that is not valid).  The tile's pixels keep one thread mapping with and without a gradient, so the value's bits do
//           not depend on it.  Pass 2: the K-loop above for each pixel of the tile, then the C gradient channels.  The patch of a
//           pixel is recomputed in pass 2 (2 roots and 3 divisions per offset and pass): K values per pixel do not fit in LDS.
//   final   one workgroup adds the tile sums in a fixed order and adds (or stores) weight * sum / (N Hv Wv) into loss_accum.
//
// The offset loop is unrolled over dx with compile-time LDS offsets; dy stays a loop: the correctly rounded roots and divisions
// of one row of offsets are already a few hundred instructions.  A thread's 32 lanes of one tile row read consecutive floats,
// so any pitch is free of bank conflicts in the passes over the tile; the pitches are odd for the ring, whose lanes run down
// columns.  LDS at r = 3: 2 * 44 * 45 * 4 + 38 * 39 * 4 = 21.8 KB static.
//
// The masked form (mv3d_census_loss_masked, MASKED = true) weighs every valid pixel by a mask m [N,H,W,1] that is not
// differentiated: census_loss_masked = (1 / (N Hv Wv)) sum m(p) rho(p), the count unchanged.  Pass 1 reads m(p) from global memory
// once per tile or ring pixel, and only at valid pixels: the product m(p) * rho(p) is formed in fp32 and added into the double sum,
// and the stored rho'(p) becomes (0.5 / root) * m(p), one fp32 multiply.  Everything behind it is the unmasked code, so a masked
// pixel still receives a gradient as the neighbour of a visible one, m == 1 gives the unmasked bits and m == 0 gives zeros.  No
// LDS is added.
#include "image_common.h"

namespace mv3d {
namespace {

constexpr int CL_TILE = IMG_TILE;                  // pixels per tile side
constexpr int CL_THREADS = IMG_THREADS;
constexpr int CL_ROWS = CL_TILE * CL_TILE / CL_THREADS;    // tile pixels per thread (4): rows py, py + 8, py + 16, py + 24 of column px

static_assert(CL_TILE == 32 && CL_THREADS == 256, "the thread mapping below: 32 lanes per tile row, 8 rows per round");

struct ClArgs {
    const float* a; const float* b; const float* mask;      // mask: the masked form only
    double* part; float* loss; float* grad;
    int N, H, W, C, a_ld, b_ld, mask_ld, grad_ld, tx, ty, accumulate, overwrite;
    float gs, inv_k, eps, eps2, gscale, weight;
    double count;
};

template <int R> struct ClGeom {
    static constexpr int HALO = CL_TILE + 4 * R;   // g is staged on the tile plus 2r
    static constexpr int GP = HALO + 1;            // its row pitch
    static constexpr int RING = CL_TILE + 2 * R;   // rho' lives on the tile plus r
    static constexpr int DP = RING + 1;
};

// sum over the offsets of e / (0.1 + e) at the pixel whose staged g_a, g_b are ga[0], gb[0]
template <int R>
__device__ __forceinline__ float census_sum(const float* ga, const float* gb) {
    constexpr int GP = ClGeom<R>::GP;
    const float ca = ga[0], cb = gb[0];
    float acc = 0.f;
#pragma unroll 1
    for (int dy = -R; dy <= R; ++dy) {
        const float* ra_ = ga + dy * GP;
        const float* rb_ = gb + dy * GP;
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const float da = ra_[dx] - ca, db = rb_[dx] - cb;
            const float ra = sqrtf(da * da + 0.81f), rb = sqrtf(db * db + 0.81f);      // plain sqrtf and / are the correctly rounded ones
            const float u = da / ra - db / rb;
            const float e = u * u;
            acc = acc + e / (0.1f + e);
        }
    }
    return acc;
}

// rho'(p) from the offset sum; *rho = rho(p)
__device__ __forceinline__ float census_root(float acc, const ClArgs& p, float* rho) {
    const float dist = acc * p.inv_k;
    const float root = sqrtf(dist + p.eps2);
    *rho = dist / (root + p.eps);
    return 0.5f / root;
}

template <int R, bool MASKED>
__global__ __launch_bounds__(CL_THREADS) void census_loss_tile_kernel(const ClArgs p) {
    using G = ClGeom<R>;
    __shared__ float s_ga[G::HALO * G::GP];
    __shared__ float s_gb[G::HALO * G::GP];
    __shared__ float s_dr[G::RING * G::DP];                // rho' on the tile plus r, 0 where the pixel is not valid
    __shared__ double s_red[CL_THREADS / 64];
    const int tiles = p.tx * p.ty;
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int y0 = (t / p.tx) * CL_TILE, x0 = (t % p.tx) * CL_TILE;
    const int tid = threadIdx.x;
    const int64_t img = (int64_t)n * p.H * p.W;
    const int px = tid & 31, py = tid >> 5;
    const bool want_grad = p.grad != nullptr;               // uniform
    double sum[1] = {0.0};

    for (int i = tid; i < G::HALO * G::HALO; i += CL_THREADS) {
        const int r = i / G::HALO, q = i - r * G::HALO;
        const int y = y0 - 2 * R + r, x = x0 - 2 * R + q;
        float va = 0.f, vb = 0.f;
        if (y >= 0 && y < p.H && x >= 0 && x < p.W) {
            const int64_t pix = img + (int64_t)y * p.W + x;
            const float* pa = p.a + pix * p.a_ld;
            const float* pb = p.b + pix * p.b_ld;
            va = pa[0];
            vb = pb[0];
            for (int c = 1; c < p.C; ++c) {                 // channels added in index order
                va = va + pa[c];
                vb = vb + pb[c];
            }
            va = va * p.gs;
            vb = vb * p.gs;
        }
        s_ga[r * G::GP + q] = va;
        s_gb[r * G::GP + q] = vb;
    }
    __syncthreads();

    // pass 1, the tile's own pixels: rho into the sum, rho' into LDS
#pragma unroll 1
    for (int k = 0; k < CL_ROWS; ++k) {
        const int ly = py + 8 * k;
        const int y = y0 + ly, x = x0 + px;
        float dr = 0.f;
        if (y >= R && y < p.H - R && x >= R && x < p.W - R) {
            const int at = (ly + 2 * R) * G::GP + px + 2 * R;
            float rho;
            dr = census_root(census_sum<R>(s_ga + at, s_gb + at), p, &rho);
            if (MASKED) {
                const float m = p.mask[(img + (int64_t)y * p.W + x) * p.mask_ld];
                rho = m * rho;
                dr = dr * m;
            }
            sum[0] += (double)rho;
        }
        if (want_grad) s_dr[(ly + R) * G::DP + px + R] = dr;
    }

    if (want_grad) {
        // pass 1, the ring of r around the tile: top and bottom bands of RING pixels per row, then the left and right bands
        constexpr int BAND = R * G::RING, RING_PIXELS = G::RING * G::RING - CL_TILE * CL_TILE;
#pragma unroll 1
        for (int i = tid; i < RING_PIXELS; i += CL_THREADS) {
            int ry, rx;
            if (i < 2 * BAND) {
                const int j = i < BAND ? i : i - BAND;
                ry = j / G::RING + (i < BAND ? 0 : CL_TILE + R);
                rx = j % G::RING;
            } else {
                const int j = i - 2 * BAND, cc = j % (2 * R);
                ry = R + j / (2 * R);
                rx = cc < R ? cc : cc + CL_TILE;
            }
            const int y = y0 - R + ry, x = x0 - R + rx;
            float dr = 0.f;
            if (y >= R && y < p.H - R && x >= R && x < p.W - R) {
                const int at = (ry + R) * G::GP + rx + R;
                float rho;
                dr = census_root(census_sum<R>(s_ga + at, s_gb + at), p, &rho);
                if (MASKED) dr = dr * p.mask[(img + (int64_t)y * p.W + x) * p.mask_ld];
            }
            s_dr[ry * G::DP + rx] = dr;
        }
        __syncthreads();

        // pass 2: both sums of the bracket at every pixel of the tile that lies in the image
#pragma unroll 1
        for (int k = 0; k < CL_ROWS; ++k) {
            const int ly = py + 8 * k;
            const int y = y0 + ly, x = x0 + px;
            if (y >= p.H || x >= p.W) continue;
            const float* ga = s_ga + (ly + 2 * R) * G::GP + px + 2 * R;
            const float* gb = s_gb + (ly + 2 * R) * G::GP + px + 2 * R;
            const float* drp = s_dr + (ly + R) * G::DP + px + R;
            const float ca = ga[0], cb = gb[0];
            float first = 0.f, second = 0.f;
#pragma unroll 1
            for (int dy = -R; dy <= R; ++dy) {
                const float* ra_ = ga + dy * G::GP;
                const float* rb_ = gb + dy * G::GP;
                const float* rd_ = drp + dy * G::DP;
#pragma unroll
                for (int dx = -R; dx <= R; ++dx) {
                    if (dx == 0 && dy == 0) continue;
                    const float da = ra_[dx] - ca, db = rb_[dx] - cb;
                    const float ra = sqrtf(da * da + 0.81f), rb = sqrtf(db * db + 0.81f);
                    const float u = da / ra - db / rb;
                    const float e = u * u;
                    const float den = 0.1f + e;
                    const float phi = (u * 0.162f) / ((den * den) * ((ra * ra) * ra));
                    second = second + phi;
                    first = first - rd_[dx] * phi;           // + rho'(q+o') phi(q+o', -o')
                }
            }
            const float g = (first - drp[0] * second) * p.gscale;
            float* dst = p.grad + (img + (int64_t)y * p.W + x) * p.grad_ld;
            for (int c = 0; c < p.C; ++c) dst[c] = p.accumulate ? dst[c] + g : g;
        }
    }

    block_sum(sum, s_red, tid);
    if (tid == 0) p.part[blockIdx.x] = block_total(s_red, 0);
}

__global__ __launch_bounds__(CL_THREADS) void census_loss_final_kernel(const ClArgs p) {
    tile_sums_final<1>(p.part, (int64_t)p.N * p.tx * p.ty, p.loss, p.overwrite, [&](const double (&sum)[1]) {
        return (float)((double)p.weight * (sum[0] / p.count));
    });
}

template <int R, bool MASKED>
int launch_tile(const ClArgs& p, int grid, hipStream_t s) {
    census_loss_tile_kernel<R, MASKED><<<grid, CL_THREADS, 0, s>>>(p);
    return launched("census_loss_tile_kernel");
}

// Both entries: `mask` is null for mv3d_census_loss (fn names the entry in the messages).
template <bool MASKED>
int census_loss_entry(const char* fn, int N, int H, int W, int C, const void* a, int a_ld, const void* b, int b_ld, const void* mask,
                      int mask_ld, int radius, float max_val, float eps, float weight, void* loss_accum, void* grad, int grad_ld,
                      int grad_accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    int64_t total;
    if (N < 1) return fail(MV3D_E_INVAL, "%s: N (%d) must be at least 1", fn, N);
    if (radius < 1 || radius > 3) return fail(MV3D_E_INVAL, "%s: radius (%d) outside 1..3", fn, radius);
    if (int rc = check_patch_image_pair(fn, N, H, W, C, a_ld, b_ld, 2 * radius + 1, &total)) return rc;
    if (MASKED && mask_ld < 1) return fail(MV3D_E_INVAL, "%s: mask_ld (%d) smaller than 1", fn, mask_ld);
    if (grad && grad_ld < C) return fail(MV3D_E_INVAL, "%s: grad_ld (%d) smaller than C (%d)", fn, grad_ld, C);
    if (int rc = check_grad_accumulate(fn, grad_accumulate)) return rc;
    if (int rc = check_finite(fn, "max_val", max_val, true)) return rc;
    if (int rc = check_finite(fn, "eps", eps, true)) return rc;
    if (int rc = check_finite(fn, "weight", weight, false)) return rc;
    if (int rc = check_not_null(fn, {{"a", a}, {"b", b}, {"loss_accum", loss_accum}})) return rc;
    if (MASKED)
        if (int rc = check_not_null(fn, {{"mask", mask}})) return rc;
    if (int rc = check_buffers(fn, MASKED ? "a, b, mask, loss_accum or grad" : "a, b, loss_accum or grad",
                               (uintptr_t)a | (uintptr_t)b | (uintptr_t)mask | (uintptr_t)loss_accum | (uintptr_t)grad,
                               workspace, workspace_bytes, tile_workspace_bytes(total, 1))) return rc;

    const int K = (2 * radius + 1) * (2 * radius + 1) - 1;
    ClArgs p = {};
    p.a = (const float*)a; p.b = (const float*)b; p.mask = (const float*)mask; p.part = (double*)workspace;
    p.loss = (float*)loss_accum; p.grad = (float*)grad;
    p.N = N; p.H = H; p.W = W; p.C = C; p.a_ld = a_ld; p.b_ld = b_ld; p.mask_ld = mask_ld; p.grad_ld = grad_ld;
    p.tx = cdiv(W, CL_TILE); p.ty = cdiv(H, CL_TILE);
    p.accumulate = grad_accumulate;
    p.overwrite = take_loss_overwrite() ? 1 : 0;          // mv3d_loss_overwrite_next(): consumed by this call, kept by a recorded one
    p.weight = weight;
    p.count = (double)N * (double)(H - 2 * radius) * (double)(W - 2 * radius);
    // the constants of the numpy twin, each formed in double and rounded to fp32 once
    p.gs = (float)(255.0 / ((double)max_val * C));
    p.inv_k = (float)(1.0 / K);
    p.eps = eps;
    p.eps2 = eps * eps;
    p.gscale = (float)((double)weight * 255.0 / ((double)max_val * C) / ((double)K * p.count));

    const double pixels = (double)N * H * W, elems = pixels * C;
    // algorithmic bytes: both images once (and the mask's 4 B per pixel), the gradient written once (and read once when it
    // accumulates), the tile sums written and read once.  FLOPs per pixel and offset: ~14 for the value (2 roots and 3 divisions
    // counted as one each), ~22 more for the gradient, whose pass also repeats the value's on the ring.
    const double grad_bytes = grad ? (grad_accumulate ? 8.0 : 4.0) : 0.0;
    const double flops = pixels * K * (grad ? 14.0 * 1.4 + 22.0 : 14.0) + elems * 2.0;
    const OpInfo tile_info{intern_label(MASKED ? "census_loss_masked_tile" : "census_loss_tile"), flops,
                           elems * (8.0 + grad_bytes) + (MASKED ? pixels * 4.0 : 0.0) + (double)total * 8.0};
    const int grid = (int)total;
    int rc = dispatch(stream, tile_info, [=](hipStream_t s) {
        return radius == 1 ? launch_tile<1, MASKED>(p, grid, s) : radius == 2 ? launch_tile<2, MASKED>(p, grid, s)
                                                                              : launch_tile<3, MASKED>(p, grid, s);
    });
    if (rc) return rc;
    const OpInfo final_info{intern_label(MASKED ? "census_loss_masked_final" : "census_loss_final"), 0.0, (double)total * 8.0 + 8.0};
    return dispatch(stream, final_info, [=](hipStream_t s) {
        census_loss_final_kernel<<<1, CL_THREADS, 0, s>>>(p);
        return launched("census_loss_final_kernel");
    });
}

}  // namespace
}  // namespace mv3d

using namespace mv3d;

extern "C" {

size_t mv3d_census_loss_workspace_bytes(int N, int H, int W, int C, int radius) {
    if (radius < 1 || radius > 3) return 0;
    return tile_workspace_bytes(patch_tile_count(N, H, W, C, 2 * radius + 1), 1);
}

int mv3d_census_loss(int N, int H, int W, int C, const void* a, int a_ld, const void* b, int b_ld, int radius, float max_val,
                     float eps, float weight, void* loss_accum, void* grad, int grad_ld, int grad_accumulate, void* workspace,
                     size_t workspace_bytes, void* stream) {
    return census_loss_entry<false>("mv3d_census_loss", N, H, W, C, a, a_ld, b, b_ld, nullptr, 1, radius, max_val, eps, weight, loss_accum,
                                    grad, grad_ld, grad_accumulate, workspace, workspace_bytes, stream);
}

int mv3d_census_loss_masked(int N, int H, int W, int C, const void* a, int a_ld, const void* b, int b_ld, const void* mask, int mask_ld,
                            int radius, float max_val, float eps, float weight, void* loss_accum, void* grad, int grad_ld,
                            int grad_accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    return census_loss_entry<true>("mv3d_census_loss_masked", N, H, W, C, a, a_ld, b, b_ld, mask, mask_ld, radius, max_val, eps, weight,
                                   loss_accum, grad, grad_ld, grad_accumulate, workspace, workspace_bytes, stream);
}

}  // extern "C"
