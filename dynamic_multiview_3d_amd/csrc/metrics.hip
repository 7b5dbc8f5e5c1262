// Per-image quality metrics of a prediction against its target: L1 (the per-image form of l1_loss, tf_utils.py:22-23), the mean
// squared error (PSNR = 10 log10(max_val^2 / mse) is a host one-liner) and SSIM (Wang et al. 2004) in the form tf.image.ssim
// computes it: 11-tap Gaussian window (sigma 1.5, normalised), applied separably, fully-inside ("valid") windows only.
//
// Built with -ffp-contract=off.  The window pass and the SSIM expression are fp32 with the operation order of the numpy twin
// (metrics.py image_metrics_host): horizontal pass, then vertical pass, taps added in index order, products and sums rounded
// one by one.  The SSIM map is therefore the map numpy computes in float32; only the sums over it differ, and those are kept in
// double here.  L1 and MSE take the difference in double, which is exact for fp32 inputs.
//
// Two launches, no atomics, no device state outside the caller's workspace:
//   tile    one workgroup per 32x32 tile of one image.  Per channel it stages the 42x42 halo tile of a and b in LDS, runs the
//           horizontal pass for F(a), F(b), F(a*b), F(a*a+b*b) (42 rows x 32 columns each), then the vertical pass with the SSIM
//           expression in registers, and adds up its three sums; the tile's own 32x32 pixels feed L1 and MSE while they are staged.
//           Every input element reaches HBM once (halo re-reads and the channel loop hit the caches).  The three sums of a tile
//           go to workspace[(n * tiles + tile) * 3] as doubles, reduced in a fixed order.
//   final   one wave per image adds the tile sums in a fixed order and writes out[n] = {L1, MSE, SSIM}.
// A fixed order everywhere: two runs on the same inputs give the same bits.
//
// LDS: rows of the staged tiles are 43 floats apart and rows of the horizontal results 33: in the horizontal pass the lanes of a
// wave run down the rows (each lane computes 4 neighbouring columns from 14 loads per image instead of 44), and an odd row pitch
// spreads them over the banks; in the vertical pass the lanes run along a row (each computes 4 rows of one column from 14 loads
// per quantity).  2 * 42 * 43 * 4 + 4 * 42 * 33 * 4 = 36.6 KB per workgroup, independent of C: four workgroups per CU.
#include "common.h"
#include <cmath>

namespace mv3d {
namespace {

constexpr int IM_TAPS = 11;
constexpr int IM_TILE = 32;                        // SSIM positions (and L1/MSE pixels) per tile side
constexpr int IM_HALO = IM_TILE + IM_TAPS - 1;     // 42
constexpr int IM_SPAN = 4 + IM_TAPS - 1;           // 14 inputs feed 4 neighbouring outputs
constexpr int IM_APITCH = IM_HALO + 1;             // 43
constexpr int IM_HPITCH = IM_TILE + 1;             // 33
constexpr int IM_THREADS = 256;
constexpr int IM_MAX_SIDE = 32768;                 // H * W < 2^31 pixels per image, tile counts fit an int

struct ImArgs {
    const float* a; const float* b;
    double* part; float* out;
    int N, H, W, C, a_ld, b_ld, tx, ty;
    float c1, c2;
    float w[IM_TAPS];
};

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(IM_THREADS) void image_metrics_tile_kernel(const ImArgs p) {
    __shared__ float s_a[IM_HALO * IM_APITCH], s_b[IM_HALO * IM_APITCH];
    __shared__ float s_h[4][IM_HALO * IM_HPITCH];
    __shared__ double s_red[IM_THREADS / 64][3];
    const int tiles = p.tx * p.ty;
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int y0 = (t / p.tx) * IM_TILE, x0 = (t % p.tx) * IM_TILE;
    const int tid = threadIdx.x;
    const int Hv = p.H - (IM_TAPS - 1), Wv = p.W - (IM_TAPS - 1);
    const int64_t img = (int64_t)n * p.H * p.W;
    const bool has_windows = y0 < Hv && x0 < Wv;          // uniform over the workgroup
    const int vx = tid & 31, vy = (tid >> 5) * 4;
    double ssim = 0.0, l1 = 0.0, mse = 0.0;

    for (int c = 0; c < p.C; ++c) {
        // every thread is past the barrier that follows the horizontal pass of channel c-1, the last reader of s_a / s_b
        for (int i = tid; i < IM_HALO * IM_HALO; i += IM_THREADS) {
            const int r = i / IM_HALO, q = i - r * IM_HALO;
            const int y = y0 + r, x = x0 + q;
            float va = 0.f, vb = 0.f;
            if (y < p.H && x < p.W) {                     // outside the image: zeros, which only reach windows that do not count
                const int64_t pix = img + (int64_t)y * p.W + x;
                va = p.a[pix * p.a_ld + c];
                vb = p.b[pix * p.b_ld + c];
                if (r < IM_TILE && q < IM_TILE) {
                    const double d = (double)va - (double)vb;
                    l1 += fabs(d);
                    mse += d * d;
                }
            }
            s_a[r * IM_APITCH + q] = va;
            s_b[r * IM_APITCH + q] = vb;
        }
        if (!has_windows) continue;
        __syncthreads();
        // horizontal pass: item = (row, group of 4 columns); lanes run down the rows
        for (int i = tid; i < IM_HALO * (IM_TILE / 4); i += IM_THREADS) {
            const int cg = i / IM_HALO, r = i - cg * IM_HALO;
            const float* ra = s_a + r * IM_APITCH + cg * 4;
            const float* rb = s_b + r * IM_APITCH + cg * 4;
            float acc[4][4] = {};
#pragma unroll
            for (int j = 0; j < IM_SPAN; ++j) {
                const float va = ra[j], vb = rb[j];
                const float ab = va * vb, ss = va * va + vb * vb;
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    const int k = j - o;
                    if (k >= 0 && k < IM_TAPS) {
                        const float wk = p.w[k];
                        acc[0][o] = acc[0][o] + wk * va;
                        acc[1][o] = acc[1][o] + wk * vb;
                        acc[2][o] = acc[2][o] + wk * ab;
                        acc[3][o] = acc[3][o] + wk * ss;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int o = 0; o < 4; ++o) s_h[q][r * IM_HPITCH + cg * 4 + o] = acc[q][o];
        }
        __syncthreads();
        // vertical pass: 4 rows of one column per lane, then the SSIM expression
        {
            float acc[4][4] = {};
#pragma unroll
            for (int j = 0; j < IM_SPAN; ++j) {
                float v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = s_h[q][(vy + j) * IM_HPITCH + vx];
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    const int k = j - o;
                    if (k >= 0 && k < IM_TAPS) {
                        const float wk = p.w[k];
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[q][o] = acc[q][o] + wk * v[q];
                    }
                }
            }
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                if (y0 + vy + o < Hv && x0 + vx < Wv) {
                    const float mx = acc[0][o], my = acc[1][o], sab = acc[2][o], s2 = acc[3][o];
                    const float num0 = (mx * my) * 2.0f, den0 = mx * mx + my * my;
                    const float lum = (num0 + p.c1) / (den0 + p.c1);
                    const float cs = ((sab * 2.0f - num0) + p.c2) / ((s2 - den0) + p.c2);
                    ssim += (double)(lum * cs);
                }
            }
        }
    }

    ssim = wave_sum(ssim);
    l1 = wave_sum(l1);
    mse = wave_sum(mse);
    if ((tid & 63) == 0) {
        s_red[tid >> 6][0] = l1;
        s_red[tid >> 6][1] = mse;
        s_red[tid >> 6][2] = ssim;
    }
    __syncthreads();
    if (tid < 3) p.part[(int64_t)blockIdx.x * 3 + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
}

__global__ __launch_bounds__(64) void image_metrics_final_kernel(const ImArgs p) {
    const int tiles = p.tx * p.ty, n = blockIdx.x;
    const double* part = p.part + (int64_t)n * tiles * 3;
    double s[3] = {0.0, 0.0, 0.0};
    for (int t = threadIdx.x; t < tiles; t += 64)
#pragma unroll
        for (int q = 0; q < 3; ++q) s[q] += part[(int64_t)t * 3 + q];
#pragma unroll
    for (int q = 0; q < 3; ++q) s[q] = wave_sum(s[q]);
    if (threadIdx.x == 0) {
        const double pixels = (double)p.H * (double)p.W;
        const double windows = (double)(p.H - (IM_TAPS - 1)) * (double)(p.W - (IM_TAPS - 1)) * (double)p.C;
        p.out[(int64_t)n * 3 + 0] = (float)(s[0] / pixels);
        p.out[(int64_t)n * 3 + 1] = (float)(s[1] / (pixels * (double)p.C));
        p.out[(int64_t)n * 3 + 2] = (float)(s[2] / windows);
    }
}

// 0 when the shape is outside what the entry takes
int64_t tile_count(int N, int H, int W, int C) {
    if (N < 1 || H < IM_TAPS || W < IM_TAPS || C < 1 || C > 4 || H > IM_MAX_SIDE || W > IM_MAX_SIDE) return 0;
    const int64_t total = (int64_t)N * cdiv(H, IM_TILE) * cdiv(W, IM_TILE);
    return total <= INT32_MAX ? total : 0;
}

}  // namespace
}  // namespace mv3d

using namespace mv3d;

extern "C" {

size_t mv3d_image_metrics_workspace_bytes(int N, int H, int W, int C) {
    const int64_t total = tile_count(N, H, W, C);
    return (size_t)cdiv64(total * 3 * (int64_t)sizeof(double), 256) * 256;
}

int mv3d_image_metrics(int N, int H, int W, int C, const void* a, int a_ld, const void* b, int b_ld, float max_val, void* out,
                       void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mv3d_image_metrics";
    if (N < 1) return fail(MV3D_E_INVAL, "%s: N (%d) must be at least 1", fn, N);
    if (H < IM_TAPS) return fail(MV3D_E_INVAL, "%s: H (%d) smaller than the 11-tap window", fn, H);
    if (W < IM_TAPS) return fail(MV3D_E_INVAL, "%s: W (%d) smaller than the 11-tap window", fn, W);
    if (C < 1 || C > 4) return fail(MV3D_E_INVAL, "%s: C (%d) outside 1..4", fn, C);
    if (H > IM_MAX_SIDE) return fail(MV3D_E_INVAL, "%s: H (%d) above %d", fn, H, IM_MAX_SIDE);
    if (W > IM_MAX_SIDE) return fail(MV3D_E_INVAL, "%s: W (%d) above %d", fn, W, IM_MAX_SIDE);
    const int64_t total = tile_count(N, H, W, C);
    if (!total) return fail(MV3D_E_INVAL, "%s: N (%d) images of %d x %d need 2^31 or more tiles", fn, N, H, W);
    if (a_ld < C) return fail(MV3D_E_INVAL, "%s: a_ld (%d) smaller than C (%d)", fn, a_ld, C);
    if (b_ld < C) return fail(MV3D_E_INVAL, "%s: b_ld (%d) smaller than C (%d)", fn, b_ld, C);
    if (!std::isfinite(max_val) || !(max_val > 0.f)) return fail(MV3D_E_INVAL, "%s: max_val (%g) must be finite and positive", fn, (double)max_val);
    if (!a) return fail(MV3D_E_INVAL, "%s: a is null", fn);
    if (!b) return fail(MV3D_E_INVAL, "%s: b is null", fn);
    if (!out) return fail(MV3D_E_INVAL, "%s: out is null", fn);
    if (!workspace) return fail(MV3D_E_INVAL, "%s: workspace is null", fn);
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 3) return fail(MV3D_E_INVAL, "%s: a, b or out not 4-byte aligned", fn);
    const size_t need = mv3d_image_metrics_workspace_bytes(N, H, W, C);
    if (workspace_bytes < need) return fail(MV3D_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    if ((uintptr_t)workspace & 15) return fail(MV3D_E_WORKSPACE, "%s: workspace not 16-byte aligned", fn);

    ImArgs p = {};
    p.a = (const float*)a; p.b = (const float*)b; p.part = (double*)workspace; p.out = (float*)out;
    p.N = N; p.H = H; p.W = W; p.C = C; p.a_ld = a_ld; p.b_ld = b_ld;
    p.tx = cdiv(W, IM_TILE); p.ty = cdiv(H, IM_TILE);
    // the constants of the numpy twin, rounded to fp32 once: c = (k * max_val)^2 and the normalised Gaussian, both from doubles
    const double k1 = 0.01 * (double)max_val, k2 = 0.03 * (double)max_val;
    p.c1 = (float)(k1 * k1);
    p.c2 = (float)(k2 * k2);
    double g[IM_TAPS], sum = 0.0;
    for (int k = 0; k < IM_TAPS; ++k) {
        const double d = (double)(k - IM_TAPS / 2);
        g[k] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += g[k];
    }
    for (int k = 0; k < IM_TAPS; ++k) p.w[k] = (float)(g[k] / sum);

    const double elems = (double)N * H * W * C;
    // algorithmic bytes: both images once, the tile sums written and read once; FLOPs: 4 quantities x 2 passes x 11 taps x 2
    const OpInfo tile_info{intern_label("image_metrics_tile"), elems * (4.0 * 2 * IM_TAPS * 2 + 20.0), elems * 8.0 + (double)total * 24.0};
    const int grid = (int)total;
    int rc = dispatch(stream, tile_info, [=](hipStream_t s) {
        image_metrics_tile_kernel<<<grid, IM_THREADS, 0, s>>>(p);
        return launched("image_metrics_tile_kernel");
    });
    if (rc) return rc;
    const OpInfo final_info{intern_label("image_metrics_final"), 0.0, (double)total * 24.0 + (double)N * 12.0};
    return dispatch(stream, final_info, [=](hipStream_t s) {
        image_metrics_final_kernel<<<N, 64, 0, s>>>(p);
        return launched("image_metrics_final_kernel");
    });
}

}  // extern "C"
