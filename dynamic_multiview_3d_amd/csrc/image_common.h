// The SSIM window core, the fixed-order tile sums and the entry checks shared by the image kernels: metrics.hip, ssim_loss.hip
// flow_smooth.hip and census_loss.hip (the sums and the checks).  The device side of what ssim_window, _valid_filter, _ssim_operands and _ssim_parts are in metrics.py.
//
// Operation order is the contract (the three units are built with -ffp-contract=off; the fp32 helpers here switch contraction off
// themselves as well).  It is what makes the window results the float32 results of the numpy twins, and it is stated here once:
//   window pass   inputs outer, outputs inner, acc = acc + w[k] * v: an output's 11 taps are added in index order, every product
//                 and every sum rounded on its own
//   SSIM terms    num0 = (mx my) 2, den0 = mx mx + my my, A1 = num0 + c1, B1 = den0 + c1, A2 = (sab 2 - num0) + c2,
//                 B2 = (s2 - den0) + c2.  mv3d_image_metrics and mv3d_ssim_loss form S = (A1 / B1) (A2 / B2) from this one
//                 expression, so their S is the same number
//   sums          double.  A wave adds its lanes as a butterfly (offsets 32, 16 .. 1), a workgroup of four waves adds the wave sums
//                 as ((w0 + w1) + w2) + w3 (wave_sum / block_sum / block_total, in sum_common.h since the gradient-norm unit shares
//                 them), a final kernel strides over the tiles: fixed orders, the same bits on every run
#pragma once
#include "common.h"
#include "sum_common.h"
#include <cmath>
#include <initializer_list>
#include <utility>

namespace mv3d {

constexpr int IMG_TAPS = 11;                       // Gaussian window, sigma 1.5
constexpr int IMG_TILE = 32;                       // tile side of the two SSIM entries
constexpr int IMG_MAX_SIDE = 32768;                // ... and their largest H, W: H * W < 2^31 pixels per image
constexpr int IMG_THREADS = SUM_THREADS;           // four waves: what block_sum (sum_common.h) and tile_sums_final are written for

// ---- device ---------------------------------------------------------------------------------------------------------------

// One item of a window pass: G neighbouring outputs of Q quantities from G + 10 inputs.  load(j, v) fills v with the Q values at
// input j; acc[q][o] becomes the window sum whose first input is o.  Fully unrolled: acc and the taps stay in registers.
template <int Q, int G, class LOAD>
__device__ __forceinline__ void window_pass(const float (&w)[IMG_TAPS], float (&acc)[Q][G], LOAD load) {
#pragma clang fp contract(off)
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int o = 0; o < G; ++o) acc[q][o] = 0.f;
#pragma unroll
    for (int j = 0; j < G + IMG_TAPS - 1; ++j) {
        float v[Q];
        load(j, v);
#pragma unroll
        for (int o = 0; o < G; ++o) {
            const int k = j - o;
            if (k >= 0 && k < IMG_TAPS) {
                const float wk = w[k];
#pragma unroll
                for (int q = 0; q < Q; ++q) acc[q][o] = acc[q][o] + wk * v[q];
            }
        }
    }
}

// the four quantities the forward window pass filters, from one pixel of a and b
__device__ __forceinline__ void ssim_operands(float va, float vb, float (&v)[4]) {
#pragma clang fp contract(off)
    v[0] = va;
    v[1] = vb;
    v[2] = va * vb;
    v[3] = va * va + vb * vb;
}

struct SsimTerms { float A1, B1, A2, B2; };           // S = (A1 / B1) * (A2 / B2)
__device__ __forceinline__ SsimTerms ssim_terms(float mx, float my, float sab, float s2, float c1, float c2) {
#pragma clang fp contract(off)
    const float num0 = (mx * my) * 2.0f, den0 = mx * mx + my * my;
    return {num0 + c1, den0 + c1, (sab * 2.0f - num0) + c2, (s2 - den0) + c2};
}

// Body of a loss's final kernel (one workgroup of 256): adds the K sums of every tile, part[t * K + q], and adds (or stores)
// term(sums) into loss[0].
template <int K, class TERM>
__device__ __forceinline__ void tile_sums_final(const double* part, int64_t total, float* loss, int overwrite, TERM term) {
    __shared__ double s_red[K * 4];
    double s[K] = {};
    for (int64_t t = threadIdx.x; t < total; t += IMG_THREADS)
#pragma unroll
        for (int q = 0; q < K; ++q) s[q] += part[t * K + q];
    block_sum(s, s_red, threadIdx.x);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < K; ++q) s[q] = block_total(s_red, q);
        const float t = term(s);
        loss[0] = overwrite ? t : loss[0] + t;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------

// the constants of the numpy twin, rounded to fp32 once: c = (k * max_val)^2 and the normalised Gaussian, both from doubles
inline void ssim_constants(float max_val, float* c1, float* c2, float (&w)[IMG_TAPS]) {
    const double k1 = 0.01 * (double)max_val, k2 = 0.03 * (double)max_val;
    *c1 = (float)(k1 * k1);
    *c2 = (float)(k2 * k2);
    double g[IMG_TAPS], sum = 0.0;
    for (int k = 0; k < IMG_TAPS; ++k) {
        const double d = (double)(k - IMG_TAPS / 2);
        g[k] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += g[k];
    }
    for (int k = 0; k < IMG_TAPS; ++k) w[k] = (float)(g[k] / sum);
}

// workgroups of one tile each over N images; 0 for an empty shape or a count that is no launch grid (2^31 or more)
inline int64_t image_tile_count(int N, int H, int W, int tile_h, int tile_w) {
    if (N < 1 || H < 1 || W < 1) return 0;
    const int64_t per_image = cdiv64(H, tile_h) * cdiv64(W, tile_w);
    if (per_image > INT32_MAX) return 0;
    const int64_t total = (int64_t)N * per_image;
    return total <= INT32_MAX ? total : 0;
}
// ... of the two SSIM entries; 0 as well when the shape is outside what they take
inline int64_t ssim_tile_count(int N, int H, int W, int C) {
    if (H < IMG_TAPS || W < IMG_TAPS || C < 1 || C > 4 || H > IMG_MAX_SIDE || W > IMG_MAX_SIDE) return 0;
    return image_tile_count(N, H, W, IMG_TILE, IMG_TILE);
}
inline size_t tile_workspace_bytes(int64_t total, int doubles_per_tile) {
    return (size_t)cdiv64(total * doubles_per_tile * (int64_t)sizeof(double), 256) * 256;
}

// The entries' argument checks, in the order the entries make them; each returns MV3D_OK or what fail() returned.
inline int fail_tiles(const char* fn, int N, int H, int W) {
    return fail(MV3D_E_INVAL, "%s: N (%d) images of %d x %d need 2^31 or more tiles", fn, N, H, W);
}
// shape and pixel strides of an image pair (the two SSIM entries); *total = ssim_tile_count
inline int check_image_pair(const char* fn, int N, int H, int W, int C, int a_ld, int b_ld, int64_t* total) {
    if (N < 1) return fail(MV3D_E_INVAL, "%s: N (%d) must be at least 1", fn, N);
    if (H < IMG_TAPS) return fail(MV3D_E_INVAL, "%s: H (%d) smaller than the 11-tap window", fn, H);
    if (W < IMG_TAPS) return fail(MV3D_E_INVAL, "%s: W (%d) smaller than the 11-tap window", fn, W);
    if (C < 1 || C > 4) return fail(MV3D_E_INVAL, "%s: C (%d) outside 1..4", fn, C);
    if (H > IMG_MAX_SIDE) return fail(MV3D_E_INVAL, "%s: H (%d) above %d", fn, H, IMG_MAX_SIDE);
    if (W > IMG_MAX_SIDE) return fail(MV3D_E_INVAL, "%s: W (%d) above %d", fn, W, IMG_MAX_SIDE);
    *total = ssim_tile_count(N, H, W, C);
    if (!*total) return fail_tiles(fn, N, H, W);
    if (a_ld < C) return fail(MV3D_E_INVAL, "%s: a_ld (%d) smaller than C (%d)", fn, a_ld, C);
    if (b_ld < C) return fail(MV3D_E_INVAL, "%s: b_ld (%d) smaller than C (%d)", fn, b_ld, C);
    return MV3D_OK;
}
// ... of an entry over (2 radius + 1)^2 patches (census_loss.hip): the same limits with the patch side as the smallest H, W
inline int64_t patch_tile_count(int N, int H, int W, int C, int side) {
    if (H < side || W < side || C < 1 || C > 4 || H > IMG_MAX_SIDE || W > IMG_MAX_SIDE) return 0;
    return image_tile_count(N, H, W, IMG_TILE, IMG_TILE);
}
inline int check_patch_image_pair(const char* fn, int N, int H, int W, int C, int a_ld, int b_ld, int side, int64_t* total) {
    if (N < 1) return fail(MV3D_E_INVAL, "%s: N (%d) must be at least 1", fn, N);
    if (H < side) return fail(MV3D_E_INVAL, "%s: H (%d) smaller than the %d x %d patch", fn, H, side, side);
    if (W < side) return fail(MV3D_E_INVAL, "%s: W (%d) smaller than the %d x %d patch", fn, W, side, side);
    if (C < 1 || C > 4) return fail(MV3D_E_INVAL, "%s: C (%d) outside 1..4", fn, C);
    if (H > IMG_MAX_SIDE) return fail(MV3D_E_INVAL, "%s: H (%d) above %d", fn, H, IMG_MAX_SIDE);
    if (W > IMG_MAX_SIDE) return fail(MV3D_E_INVAL, "%s: W (%d) above %d", fn, W, IMG_MAX_SIDE);
    *total = patch_tile_count(N, H, W, C, side);
    if (!*total) return fail_tiles(fn, N, H, W);
    if (a_ld < C) return fail(MV3D_E_INVAL, "%s: a_ld (%d) smaller than C (%d)", fn, a_ld, C);
    if (b_ld < C) return fail(MV3D_E_INVAL, "%s: b_ld (%d) smaller than C (%d)", fn, b_ld, C);
    return MV3D_OK;
}
inline int check_grad_accumulate(const char* fn, int v) {
    if (v != 0 && v != 1) return fail(MV3D_E_INVAL, "%s: grad_accumulate (%d) must be 0 or 1", fn, v);
    return MV3D_OK;
}
// max_val and eps are finite and positive, weight is finite
inline int check_finite(const char* fn, const char* name, float v, bool positive) {
    if (!std::isfinite(v) || (positive && !(v > 0.f)))
        return fail(MV3D_E_INVAL, "%s: %s (%g) must be finite%s", fn, name, (double)v, positive ? " and positive" : "");
    return MV3D_OK;
}
inline int check_not_null(const char* fn, std::initializer_list<std::pair<const char*, const void*>> ptrs) {
    for (const auto& p : ptrs)
        if (!p.second) return fail(MV3D_E_INVAL, "%s: %s is null", fn, p.first);
    return MV3D_OK;
}
// the workspace is there, the operands (their addresses or-ed, `names` for the message) are floats, the workspace is large enough
// and holds doubles
inline int check_buffers(const char* fn, const char* names, uintptr_t operands, const void* workspace, size_t workspace_bytes,
                         size_t need) {
    if (!workspace) return fail(MV3D_E_INVAL, "%s: workspace is null", fn);
    if (operands & 3) return fail(MV3D_E_INVAL, "%s: %s not 4-byte aligned", fn, names);
    if (workspace_bytes < need) return fail(MV3D_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    if ((uintptr_t)workspace & 15) return fail(MV3D_E_WORKSPACE, "%s: workspace not 16-byte aligned", fn);
    return MV3D_OK;
}

}  // namespace mv3d
