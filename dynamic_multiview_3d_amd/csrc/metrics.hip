// Per-image quality metrics of a prediction against its target: L1 (the per-image form of l1_loss, tf_utils.py:22-23), the mean
// squared error (PSNR = 10 log10(max_val^2 / mse) is a host one-liner) and SSIM (Wang et al. 2004) in the form tf.image.ssim
// computes it: 11-tap Gaussian window (sigma 1.5, normalised), applied separably, fully-inside ("valid") windows only.
//
// Built with -ffp-contract=off.  The window pass and the SSIM expression are fp32 with the operation order of the numpy twin
// (metrics.py image_metrics_host): horizontal pass, then vertical pass, each in the order image_common.h states.  The SSIM map is
// therefore the map numpy computes in float32; only the sums over it differ, and those are kept in double here.  L1 and MSE take
// the difference in double, which is exact for fp32 inputs.
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
#include "image_common.h"

namespace mv3d {
namespace {

constexpr int IM_TAPS = IMG_TAPS;
constexpr int IM_TILE = IMG_TILE;                  // SSIM positions (and L1/MSE pixels) per tile side
constexpr int IM_HALO = IM_TILE + IM_TAPS - 1;     // 42
constexpr int IM_APITCH = IM_HALO + 1;             // 43
constexpr int IM_HPITCH = IM_TILE + 1;             // 33
constexpr int IM_THREADS = IMG_THREADS;

struct ImArgs {
    const float* a; const float* b;
    double* part; float* out;
    int N, H, W, C, a_ld, b_ld, tx, ty;
    float c1, c2;
    float w[IM_TAPS];
};

__global__ __launch_bounds__(IM_THREADS) void image_metrics_tile_kernel(const ImArgs p) {
    __shared__ float s_a[IM_HALO * IM_APITCH], s_b[IM_HALO * IM_APITCH];
    __shared__ float s_h[4][IM_HALO * IM_HPITCH];
    __shared__ double s_red[3 * (IM_THREADS / 64)];
    const int tiles = p.tx * p.ty;
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int y0 = (t / p.tx) * IM_TILE, x0 = (t % p.tx) * IM_TILE;
    const int tid = threadIdx.x;
    const int Hv = p.H - (IM_TAPS - 1), Wv = p.W - (IM_TAPS - 1);
    const int64_t img = (int64_t)n * p.H * p.W;
    const bool has_windows = y0 < Hv && x0 < Wv;          // uniform over the workgroup
    const int vx = tid & 31, vy = (tid >> 5) * 4;
    double sums[3] = {0.0, 0.0, 0.0};                     // L1, MSE, SSIM: the columns of a metrics row
    double &l1 = sums[0], &mse = sums[1], &ssim = sums[2];

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
            float acc[4][4];
            window_pass(p.w, acc, [&](int j, float (&v)[4]) { ssim_operands(ra[j], rb[j], v); });
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int o = 0; o < 4; ++o) s_h[q][r * IM_HPITCH + cg * 4 + o] = acc[q][o];
        }
        __syncthreads();
        // vertical pass: 4 rows of one column per lane, then the SSIM expression
        {
            float acc[4][4];
            window_pass(p.w, acc, [&](int j, float (&v)[4]) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = s_h[q][(vy + j) * IM_HPITCH + vx];
            });
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                if (y0 + vy + o < Hv && x0 + vx < Wv) {
                    const SsimTerms t = ssim_terms(acc[0][o], acc[1][o], acc[2][o], acc[3][o], p.c1, p.c2);
                    ssim += (double)((t.A1 / t.B1) * (t.A2 / t.B2));
                }
            }
        }
    }

    block_sum(sums, s_red, tid);
    if (tid < 3) p.part[(int64_t)blockIdx.x * 3 + tid] = block_total(s_red, tid);
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

}  // namespace
}  // namespace mv3d

using namespace mv3d;

extern "C" {

size_t mv3d_image_metrics_workspace_bytes(int N, int H, int W, int C) {
    return tile_workspace_bytes(ssim_tile_count(N, H, W, C), 3);
}

int mv3d_image_metrics(int N, int H, int W, int C, const void* a, int a_ld, const void* b, int b_ld, float max_val, void* out,
                       void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mv3d_image_metrics";
    int64_t total;
    if (int rc = check_image_pair(fn, N, H, W, C, a_ld, b_ld, &total)) return rc;
    if (int rc = check_finite(fn, "max_val", max_val, true)) return rc;
    if (int rc = check_not_null(fn, {{"a", a}, {"b", b}, {"out", out}})) return rc;
    if (int rc = check_buffers(fn, "a, b or out", (uintptr_t)a | (uintptr_t)b | (uintptr_t)out, workspace, workspace_bytes,
                               tile_workspace_bytes(total, 3))) return rc;

    ImArgs p = {};
    p.a = (const float*)a; p.b = (const float*)b; p.part = (double*)workspace; p.out = (float*)out;
    p.N = N; p.H = H; p.W = W; p.C = C; p.a_ld = a_ld; p.b_ld = b_ld;
    p.tx = cdiv(W, IM_TILE); p.ty = cdiv(H, IM_TILE);
    ssim_constants(max_val, &p.c1, &p.c2, p.w);

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
