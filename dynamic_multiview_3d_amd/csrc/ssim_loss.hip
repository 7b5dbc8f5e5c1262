// SSIM as a training loss: loss = 1 - mean over images, windows and channels of the SSIM map S that mv3d_image_metrics averages
// (metrics.hip: both take the taps, c1 / c2, the window pass and the terms of S from image_common.h), and its gradient with respect
// to the prediction.
//
// Per window, with mx = F(a), my = F(b), sab = F(a b), s2 = F(a a + b b):
//   A1 = 2 mx my + c1    B1 = mx^2 + my^2 + c1    A2 = 2 sab - 2 mx my + c2    B2 = s2 - (mx^2 + my^2) + c2    S = (A1/B1)(A2/B2)
//   Dm = dS/dmx  = 2 (my (A2 - A1) - mx S (B2 - B1)) / (B1 B2)
//   Ds = dS/dsab = 2 (A1/B1) / B2
//   Dq = dS/ds2  = -S / B2
//   dS_total/da(q) = Ft(Dm)(q) + b(q) Ft(Ds)(q) + 2 a(q) Ft(Dq)(q),    grad(q) = -weight / (N Hv Wv C) * dS_total/da(q)
// Ft, the transpose of the valid window pass, is the same separable filter over the Hv x Wv map zero-padded by 10 on every
// side (the window is symmetric).  The three coefficients are written so that a == b gives Dm == 0 and Ds == -2 Dq exactly.
//
// Built with -ffp-contract=off: every step is fp32 in the order of the numpy twin (metrics.py ssim_loss_host at float32): in both
// directions the horizontal pass runs before the vertical one, each in the order image_common.h states.  Only the sum of S is
// kept in double, in a fixed order.
//
// Two launches, no atomics, no device state outside the caller's workspace:
//   tile    one workgroup per 32x32 PIXEL tile of one image, so that every gradient element has exactly one writer.  Per channel
//           it stages the 52x52 halo of a and b (origin 10 above and left of the tile, zeros outside the image), runs the
//           forward horizontal pass (52 rows x 42 columns x 4 quantities) and the vertical pass: the 42x42 windows that touch the
//           tile.  Each window's S, Dm, Ds, Dq are formed in registers (zero for a window outside [0,Hv) x [0,Wv)); S counts
//           only for a window whose origin lies in the tile's own 32x32, so every window counts once.  The three coefficient maps
//           go to LDS over the horizontal buffers, the transposed horizontal pass (42 x 32 x 3) overlays the staged images, and
//           the transposed vertical pass ends with the combination at the pixel.  The forward pass is recomputed about
//           (52/32)^2 = 2.6 times; in exchange the coefficient maps never travel through HBM.
//   final   one workgroup adds the tile sums in a fixed order and adds (or stores) weight * (1 - sum / count) into loss_accum.
//
// LDS: staged rows are 53 floats apart, forward horizontal rows and coefficient rows 43, transposed horizontal rows 33: odd
// pitches, because in the horizontal passes the lanes of a wave run down the rows.  2*52*53*4 + 4*52*43*4 = 57.8 KB static.
//
// The masked form (mv3d_ssim_loss_masked, MASKED = true) weighs every window by the mask m [N,H,W,1] at its centre, m_w =
// m(oy + 5, ox + 5) for the window with origin (oy, ox); the mask is not differentiated.  Two double sums per tile, M = sum of m_w
// and Sm = sum of fp32(m_w * S) over the channels and the tile's own windows, and loss = weight * (M / count - Sm / count) with the
// count unchanged.  Dm, Ds, Dq of a window are each multiplied by m_w (one fp32 multiply each) before the transposed passes.
// m_w is read from global memory in the vertical pass's thread mapping, where the lanes run along a window row: once per window, in
// front of the channel loop, and kept in 7 registers over the channels.  No LDS is added.  m == 1 gives the unmasked bits (M == count exactly) and m == 0 gives zeros.
#include "image_common.h"

namespace mv3d {
namespace {

constexpr int SL_TAPS = IMG_TAPS;
constexpr int SL_PAD = SL_TAPS - 1;                // 10
constexpr int SL_TILE = IMG_TILE;                  // pixels per tile side
constexpr int SL_WIN = SL_TILE + SL_PAD;           // 42 windows per side touch a tile
constexpr int SL_HALO = SL_WIN + SL_PAD;           // 52 pixels per side feed them
constexpr int SL_APITCH = SL_HALO + 1;             // 53
constexpr int SL_HPITCH = SL_WIN + 1;              // 43
constexpr int SL_TPITCH = SL_TILE + 1;             // 33
constexpr int SL_HG = 3;                           // forward horizontal pass: columns per item (42 = 14 * 3)
constexpr int SL_VR = 7;                           // forward vertical pass: rows per item (42 = 6 * 7; 42 * 6 = 252 items, one round)
constexpr int SL_THREADS = IMG_THREADS;

static_assert(SL_WIN % SL_HG == 0 && SL_WIN % SL_VR == 0, "the forward passes cover the 42 windows without a remainder");
static_assert(SL_WIN * (SL_WIN / SL_VR) <= SL_THREADS, "one vertical item per thread");
static_assert(3 * SL_WIN * SL_TPITCH <= 2 * SL_HALO * SL_APITCH, "the transposed horizontal results fit over the staged images");
static_assert(3 * SL_WIN * SL_HPITCH <= 4 * SL_HALO * SL_HPITCH, "the coefficient maps fit over the horizontal results");

struct SlArgs {
    const float* a; const float* b; const float* mask;      // mask: the masked form only
    double* part; float* loss; float* grad;
    int N, H, W, C, a_ld, b_ld, mask_ld, grad_ld, tx, ty, accumulate, overwrite;
    float c1, c2, gscale, weight;
    float w[SL_TAPS];
};

template <bool MASKED>
__global__ __launch_bounds__(SL_THREADS) void ssim_loss_tile_kernel(const SlArgs p) {
    constexpr int SUMS = MASKED ? 2 : 1;                   // the sum of S; masked: M, then Sm
    __shared__ float s_ab[2 * SL_HALO * SL_APITCH];        // a, b staged; later the transposed horizontal results
    __shared__ float s_h[4 * SL_HALO * SL_HPITCH];         // forward horizontal results; later Dm, Ds, Dq
    __shared__ double s_red[SUMS * (SL_THREADS / 64)];
    float* const s_a = s_ab;
    float* const s_b = s_ab + SL_HALO * SL_APITCH;
    const int tiles = p.tx * p.ty;
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int y0 = (t / p.tx) * SL_TILE, x0 = (t % p.tx) * SL_TILE;
    const int tid = threadIdx.x;
    const int Hv = p.H - SL_PAD, Wv = p.W - SL_PAD;
    const int64_t img = (int64_t)n * p.H * p.W;
    const int px = tid & 31, py = (tid >> 5) * 4;          // this thread's 4 pixels: rows py .. py+3 of column px
    const int wx = tid % SL_WIN, wy = (tid / SL_WIN) * SL_VR;      // its 7 windows: rows wy .. wy+6 of column wx (tid < 252)
    double ssim[SUMS] = {};
    float mw[SL_VR];                                       // masked: the mask at the centres of this thread's 7 windows
    if (MASKED && tid < SL_WIN * (SL_WIN / SL_VR)) {
        const int ox = x0 - SL_PAD + wx;
#pragma unroll
        for (int o = 0; o < SL_VR; ++o) {
            const int oy = y0 - SL_PAD + wy + o;
            mw[o] = 0.f;
            if (oy >= 0 && oy < Hv && ox >= 0 && ox < Wv)
                mw[o] = p.mask[(img + (int64_t)(oy + SL_TAPS / 2) * p.W + ox + SL_TAPS / 2) * p.mask_ld];
        }
    }

    for (int c = 0; c < p.C; ++c) {
        for (int i = tid; i < SL_HALO * SL_HALO; i += SL_THREADS) {
            const int r = i / SL_HALO, q = i - r * SL_HALO;
            const int y = y0 - SL_PAD + r, x = x0 - SL_PAD + q;
            float va = 0.f, vb = 0.f;
            if (y >= 0 && y < p.H && x >= 0 && x < p.W) {  // outside the image: zeros, which only reach windows that do not count
                const int64_t pix = img + (int64_t)y * p.W + x;
                va = p.a[pix * p.a_ld + c];
                vb = p.b[pix * p.b_ld + c];
            }
            s_a[r * SL_APITCH + q] = va;
            s_b[r * SL_APITCH + q] = vb;
        }
        __syncthreads();
        float pa[4], pb[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            pa[o] = s_a[(py + o + SL_PAD) * SL_APITCH + px + SL_PAD];
            pb[o] = s_b[(py + o + SL_PAD) * SL_APITCH + px + SL_PAD];
        }
        // forward horizontal pass: item = (row, group of 3 columns); lanes run down the rows
        for (int i = tid; i < SL_HALO * (SL_WIN / SL_HG); i += SL_THREADS) {
            const int cg = i / SL_HALO, r = i - cg * SL_HALO;
            const float* ra = s_a + r * SL_APITCH + cg * SL_HG;
            const float* rb = s_b + r * SL_APITCH + cg * SL_HG;
            float acc[4][SL_HG];
            window_pass(p.w, acc, [&](int j, float (&v)[4]) { ssim_operands(ra[j], rb[j], v); });
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int o = 0; o < SL_HG; ++o) s_h[q * SL_HALO * SL_HPITCH + r * SL_HPITCH + cg * SL_HG + o] = acc[q][o];
        }
        __syncthreads();
        // forward vertical pass: 7 rows of one window column per lane, then S and the three coefficients
        float dm[SL_VR], ds[SL_VR], dq[SL_VR];
        if (tid < SL_WIN * (SL_WIN / SL_VR)) {
            float acc[4][SL_VR];
            window_pass(p.w, acc, [&](int j, float (&v)[4]) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = s_h[q * SL_HALO * SL_HPITCH + (wy + j) * SL_HPITCH + wx];
            });
            const int ox = x0 - SL_PAD + wx;                              // window origin, image coordinates
#pragma unroll
            for (int o = 0; o < SL_VR; ++o) {
                const int oy = y0 - SL_PAD + wy + o;
                dm[o] = ds[o] = dq[o] = 0.f;
                if (oy >= 0 && oy < Hv && ox >= 0 && ox < Wv) {
                    const float mx = acc[0][o], my = acc[1][o];
                    const SsimTerms t = ssim_terms(mx, my, acc[2][o], acc[3][o], p.c1, p.c2);
                    const float lum = t.A1 / t.B1;
                    const float S = lum * (t.A2 / t.B2);
                    dm[o] = ((my * (t.A2 - t.A1) - (mx * S) * (t.B2 - t.B1)) * 2.0f) / (t.B1 * t.B2);
                    ds[o] = (lum / t.B2) * 2.0f;
                    dq[o] = -(S / t.B2);
                    if (MASKED) {
                        dm[o] = dm[o] * mw[o];
                        ds[o] = ds[o] * mw[o];
                        dq[o] = dq[o] * mw[o];
                    }
                    if (oy >= y0 && ox >= x0) {                            // origin in the tile's own 32x32: counted here and only here
                        if (MASKED) {
                            ssim[0] += (double)mw[o];
                            ssim[SUMS - 1] += (double)(mw[o] * S);
                        } else {
                            ssim[0] += (double)S;
                        }
                    }
                }
            }
        }
        __syncthreads();                                                   // every read of the horizontal results is done
        if (!p.grad) continue;                                             // value only (uniform): the next barrier is the one after staging
        float* const s_c = s_h;
        if (tid < SL_WIN * (SL_WIN / SL_VR)) {
#pragma unroll
            for (int o = 0; o < SL_VR; ++o) {
                const int at = (wy + o) * SL_HPITCH + wx;
                s_c[at] = dm[o];
                s_c[SL_WIN * SL_HPITCH + at] = ds[o];
                s_c[2 * SL_WIN * SL_HPITCH + at] = dq[o];
            }
        }
        __syncthreads();
        // transposed horizontal pass: item = (window row, group of 4 pixel columns); lanes run down the rows
        float* const s_t = s_ab;
        for (int i = tid; i < SL_WIN * (SL_TILE / 4); i += SL_THREADS) {
            const int cg = i / SL_WIN, r = i - cg * SL_WIN;
            float acc[3][4];
            window_pass(p.w, acc, [&](int j, float (&v)[3]) {
#pragma unroll
                for (int q = 0; q < 3; ++q) v[q] = s_c[q * SL_WIN * SL_HPITCH + r * SL_HPITCH + cg * 4 + j];
            });
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int o = 0; o < 4; ++o) s_t[q * SL_WIN * SL_TPITCH + r * SL_TPITCH + cg * 4 + o] = acc[q][o];
        }
        __syncthreads();
        // transposed vertical pass: 4 rows of one pixel column per lane, then the combination at the pixel
        {
            float acc[3][4];
            window_pass(p.w, acc, [&](int j, float (&v)[3]) {
#pragma unroll
                for (int q = 0; q < 3; ++q) v[q] = s_t[q * SL_WIN * SL_TPITCH + (py + j) * SL_TPITCH + px];
            });
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const int y = y0 + py + o, x = x0 + px;
                if (y < p.H && x < p.W) {
                    const float g = ((acc[0][o] + pb[o] * acc[1][o]) + (pa[o] * 2.0f) * acc[2][o]) * p.gscale;
                    float* dst = p.grad + (img + (int64_t)y * p.W + x) * p.grad_ld + c;
                    *dst = p.accumulate ? *dst + g : g;
                }
            }
        }
        __syncthreads();                                                   // the staging of the next channel overwrites s_t
    }

    block_sum(ssim, s_red, tid);
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < SUMS; ++q) p.part[(int64_t)blockIdx.x * SUMS + q] = block_total(s_red, q);
    }
}

__global__ __launch_bounds__(SL_THREADS) void ssim_loss_masked_final_kernel(const SlArgs p) {
    tile_sums_final<2>(p.part, (int64_t)p.N * p.tx * p.ty, p.loss, p.overwrite, [&](const double (&sum)[2]) {
        const double windows = (double)p.N * (double)(p.H - SL_PAD) * (double)(p.W - SL_PAD) * (double)p.C;
        return (float)((double)p.weight * (sum[0] / windows - sum[1] / windows));
    });
}

__global__ __launch_bounds__(SL_THREADS) void ssim_loss_final_kernel(const SlArgs p) {
    tile_sums_final<1>(p.part, (int64_t)p.N * p.tx * p.ty, p.loss, p.overwrite, [&](const double (&sum)[1]) {
        const double windows = (double)p.N * (double)(p.H - SL_PAD) * (double)(p.W - SL_PAD) * (double)p.C;
        return (float)((double)p.weight * (1.0 - sum[0] / windows));
    });
}

// Both entries: `mask` is null for mv3d_ssim_loss (fn names the entry in the messages).
template <bool MASKED>
int ssim_loss_entry(const char* fn, int N, int H, int W, int C, const void* a, int a_ld, const void* b, int b_ld, const void* mask,
                    int mask_ld, float max_val, float weight, void* loss_accum, void* grad, int grad_ld, int grad_accumulate,
                    void* workspace, size_t workspace_bytes, void* stream) {
    constexpr int SUMS = MASKED ? 2 : 1;
    int64_t total;
    if (int rc = check_image_pair(fn, N, H, W, C, a_ld, b_ld, &total)) return rc;
    if (MASKED && mask_ld < 1) return fail(MV3D_E_INVAL, "%s: mask_ld (%d) smaller than 1", fn, mask_ld);
    if (grad && grad_ld < C) return fail(MV3D_E_INVAL, "%s: grad_ld (%d) smaller than C (%d)", fn, grad_ld, C);
    if (int rc = check_grad_accumulate(fn, grad_accumulate)) return rc;
    if (int rc = check_finite(fn, "max_val", max_val, true)) return rc;
    if (int rc = check_finite(fn, "weight", weight, false)) return rc;
    if (int rc = check_not_null(fn, {{"a", a}, {"b", b}, {"loss_accum", loss_accum}})) return rc;
    if (MASKED)
        if (int rc = check_not_null(fn, {{"mask", mask}})) return rc;
    if (int rc = check_buffers(fn, MASKED ? "a, b, mask, loss_accum or grad" : "a, b, loss_accum or grad",
                               (uintptr_t)a | (uintptr_t)b | (uintptr_t)mask | (uintptr_t)loss_accum | (uintptr_t)grad,
                               workspace, workspace_bytes, tile_workspace_bytes(total, SUMS))) return rc;

    SlArgs p = {};
    p.a = (const float*)a; p.b = (const float*)b; p.mask = (const float*)mask; p.part = (double*)workspace; p.loss = (float*)loss_accum; p.grad = (float*)grad;
    p.N = N; p.H = H; p.W = W; p.C = C; p.a_ld = a_ld; p.b_ld = b_ld; p.mask_ld = mask_ld; p.grad_ld = grad_ld;
    p.tx = cdiv(W, SL_TILE); p.ty = cdiv(H, SL_TILE);
    p.accumulate = grad_accumulate;
    p.overwrite = take_loss_overwrite() ? 1 : 0;          // mv3d_loss_overwrite_next(): consumed by this call, kept by a recorded one
    p.weight = weight;
    const double windows = (double)N * (double)(H - SL_PAD) * (double)(W - SL_PAD) * (double)C;
    p.gscale = (float)(-(double)weight / windows);
    ssim_constants(max_val, &p.c1, &p.c2, p.w);

    const double elems = (double)N * H * W * C;
    // algorithmic bytes: both images once (and the mask's 4 B per pixel), the gradient written once (and read once when it accumulates), the tile sums written
    // and read once.  FLOPs per element: 4 quantities x 2 passes x 11 taps x 2 forward, 3 x 2 x 11 x 2 transposed, ~40 for the
    // window expression and the combination.
    const double grad_bytes = grad ? (grad_accumulate ? 8.0 : 4.0) : 0.0;
    const double flops = elems * (4.0 * 2 * SL_TAPS * 2 + (grad ? 3.0 * 2 * SL_TAPS * 2 + 40.0 : 12.0));
    const OpInfo tile_info{intern_label(MASKED ? "ssim_loss_masked_tile" : "ssim_loss_tile"), flops,
                           elems * (8.0 + grad_bytes) + (MASKED ? (double)N * H * W * 4.0 : 0.0) + (double)total * 8.0 * SUMS};
    const int grid = (int)total;
    int rc = dispatch(stream, tile_info, [=](hipStream_t s) {
        ssim_loss_tile_kernel<MASKED><<<grid, SL_THREADS, 0, s>>>(p);
        return launched("ssim_loss_tile_kernel");
    });
    if (rc) return rc;
    const OpInfo final_info{intern_label(MASKED ? "ssim_loss_masked_final" : "ssim_loss_final"), 0.0, (double)total * 8.0 * SUMS + 8.0};
    return dispatch(stream, final_info, [=](hipStream_t s) {
        if (MASKED) ssim_loss_masked_final_kernel<<<1, SL_THREADS, 0, s>>>(p);
        else ssim_loss_final_kernel<<<1, SL_THREADS, 0, s>>>(p);
        return launched("ssim_loss_final_kernel");
    });
}


}  // namespace
}  // namespace mv3d

using namespace mv3d;

extern "C" {

size_t mv3d_ssim_loss_workspace_bytes(int N, int H, int W, int C) {
    return tile_workspace_bytes(ssim_tile_count(N, H, W, C), 1);
}

size_t mv3d_ssim_loss_masked_workspace_bytes(int N, int H, int W, int C) {
    return tile_workspace_bytes(ssim_tile_count(N, H, W, C), 2);
}

int mv3d_ssim_loss(int N, int H, int W, int C, const void* a, int a_ld, const void* b, int b_ld, float max_val, float weight,
                   void* loss_accum, void* grad, int grad_ld, int grad_accumulate, void* workspace, size_t workspace_bytes,
                   void* stream) {
    return ssim_loss_entry<false>("mv3d_ssim_loss", N, H, W, C, a, a_ld, b, b_ld, nullptr, 1, max_val, weight, loss_accum, grad, grad_ld,
                                  grad_accumulate, workspace, workspace_bytes, stream);
}

int mv3d_ssim_loss_masked(int N, int H, int W, int C, const void* a, int a_ld, const void* b, int b_ld, const void* mask, int mask_ld,
                          float max_val, float weight, void* loss_accum, void* grad, int grad_ld, int grad_accumulate, void* workspace,
                          size_t workspace_bytes, void* stream) {
    return ssim_loss_entry<true>("mv3d_ssim_loss_masked", N, H, W, C, a, a_ld, b, b_ld, mask, mask_ld, max_val, weight, loss_accum, grad,
                                 grad_ld, grad_accumulate, workspace, workspace_bytes, stream);
}

}  // extern "C"
