// The reader's process_image on the device (multi_view_model/utils/read_tf_records.py:88-112): raw uint8 record image ->
// central square crop -> TensorFlow 1.3 ResizeBicubic (align_corners = False) -> / 255, float32 NHWC, one launch per
// feature per batch.  Built with -ffp-contract=off: every product and sum below rounds on its own, in the order DESIGN.md
// (input path) pins, so the result is bitwise the numpy float32 restatement's (read_tf_records.process_image).
//
// Per axis: scale = (float)S / (float)out, loc = scale * (float)o (no half-pixel offset), fl = floor(loc),
// off = rint((loc - fl) * 1024); taps fl-1 .. fl+2 clamped to [0, S-1] with the weights of TF's 1025-entry coefficient
// table (A = -0.75), which is a pure function of off and is evaluated here instead of being stored.  Horizontal pass first,
// then the vertical one, each ((v0*w0 + v1*w1) + v2*w2) + v3*w3.  No clipping: bicubic overshoots and so does the reference.
#include "common.h"
#include <algorithm>

namespace mv3d {

constexpr int PI_MAX_SIDE = 4096;            // largest record / output side the entry point admits
constexpr int PI_MAX_TILE = 16;              // output rows per workgroup of the tiled kernel, at most
constexpr size_t PI_LDS_BUDGET = 48 * 1024;  // per workgroup: three workgroups per CU at the least

// TF's table: tab[2i] at x = i/1024 in [0, 1], tab[2i+1] at x + 1 in [1, 2]
__host__ __device__ __forceinline__ float bicubic_near(int i) {
    const float A = -0.75f;
    const float x = (float)i * (1.0f / 1024.0f);             // exact: i <= 1024
    return ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
}
__host__ __device__ __forceinline__ float bicubic_far(int i) {
    const float A = -0.75f;
    const float x = (float)i * (1.0f / 1024.0f) + 1.0f;      // exact
    return ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
}

__host__ __device__ __forceinline__ int axis_floor(float scale, int o) { return (int)floorf(scale * (float)o); }

// first tap (unclamped: fl - 1) and the four weights of output coordinate o
__device__ __forceinline__ int axis_taps(float scale, int o, float4* w) {
    const float loc = scale * (float)o;
    const float fl = floorf(loc);
    const int off = __float2int_rn((loc - fl) * 1024.0f);   // round half to even, as lrintf
    *w = make_float4(bicubic_far(off), bicubic_near(off), bicubic_near(1024 - off), bicubic_far(1024 - off));
    return (int)fl - 1;
}

__device__ __forceinline__ float cubic4(float v0, float v1, float v2, float v3, const float4& w) {
    return ((v0 * w.x + v1 * w.y) + v2 * w.z) + v3 * w.w;
}

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

// ---------------------------------------------------------------- tiled kernel
// One workgroup = `th` output rows of one image, full width.  LDS: the x taps of every output column and the y taps of
// the tile's rows, the source window the tile needs as float (rows fl(first) - 1 .. fl(last) + 2, already cropped and
// row-clamped), and the horizontal pass of that window.  The vertical pass reads the horizontal one 16 bytes per lane and
// stores the NHWC output through a flat (x, c) index, 16 bytes per lane whatever C is (the host checks wo * C % 4 == 0).
// Dynamic LDS layout, every part a multiple of 16 bytes: wx[wo] float4 | wy[th] float4 | hrow[rmax * wo * C] | window
// [rmax * S * C] | ix[wo] int | iy[th] int.
template <int C>
__global__ __launch_bounds__(256) void process_image_tiled_kernel(const unsigned char* __restrict__ src, int hs, int ws, int S,
                                                                int crop_y, int crop_x, float* __restrict__ dst, int ho, int wo,
                                                                float sy, float sx, int th, int rmax, int tiles, int vec) {
    extern __shared__ float4 s_mem[];
    const int woC = wo * C, sC = S * C;
    float4* s_wx = s_mem;
    float4* s_wy = s_wx + wo;
    float* s_h = reinterpret_cast<float*>(s_wy + th);
    float* s_win = s_h + (size_t)rmax * woC;
    int* s_ix = reinterpret_cast<int*>(s_win + (((size_t)rmax * sC + 3) & ~(size_t)3));
    int* s_iy = s_ix + wo;

    const int n = blockIdx.x / tiles, y0 = (blockIdx.x - n * tiles) * th;
    const int trows = min(th, ho - y0);
    const int lo = axis_floor(sy, y0) - 1;                                   // first source row of the window (may be -1)
    const int rows = min(axis_floor(sy, y0 + trows - 1) + 2 - lo + 1, rmax);  // the host sized rmax with the same arithmetic
    const int tid = threadIdx.x;

    for (int x = tid; x < wo; x += 256) s_ix[x] = axis_taps(sx, x, &s_wx[x]);
    if (tid < trows) s_iy[tid] = axis_taps(sy, y0 + tid, &s_wy[tid]) - lo;

    // the window: uint8 -> float, one read of the source per workgroup
    const unsigned char* img = src + (size_t)n * hs * ws * C;
    if (vec) {
        const int sC4 = sC >> 2;
        int r = tid / sC4, j = tid - r * sC4;
        while (r < rows) {
            const int sr = clampi(lo + r, S - 1) + crop_y;
            const uchar4 b = reinterpret_cast<const uchar4*>(img + ((size_t)sr * ws + crop_x) * C)[j];
            reinterpret_cast<float4*>(s_win + (size_t)r * sC)[j] = make_float4((float)b.x, (float)b.y, (float)b.z, (float)b.w);
            j += 256;
            while (j >= sC4) { j -= sC4; ++r; }
        }
    } else {
        int r = tid / sC, j = tid - r * sC;
        while (r < rows) {
            const int sr = clampi(lo + r, S - 1) + crop_y;
            s_win[(size_t)r * sC + j] = (float)img[((size_t)sr * ws + crop_x) * C + j];
            j += 256;
            while (j >= sC) { j -= sC; ++r; }
        }
    }
    __syncthreads();

    {   // horizontal pass over every row of the window
        int r = tid / woC, j = tid - r * woC;
        while (r < rows) {
            const int x = j / C, c = j - x * C;
            const int t = s_ix[x];
            const float* row = s_win + (size_t)r * sC + c;
            s_h[(size_t)r * woC + j] = cubic4(row[clampi(t, S - 1) * C], row[clampi(t + 1, S - 1) * C], row[clampi(t + 2, S - 1) * C],
                                              row[clampi(t + 3, S - 1) * C], s_wx[x]);
            j += 256;
            while (j >= woC) { j -= woC; ++r; }
        }
    }
    __syncthreads();

    {   // vertical pass, / 255, 16-byte stores
        const int woC4 = woC >> 2;
        float4* out = reinterpret_cast<float4*>(dst + ((size_t)n * ho + y0) * woC);
        int t = tid / woC4, j = tid - t * woC4;
        while (t < trows) {
            const float4 w = s_wy[t];
            const float4* h = reinterpret_cast<const float4*>(s_h + (size_t)s_iy[t] * woC) + j;
            const float4 a = h[0], b = h[woC4], c = h[2 * woC4], d = h[3 * woC4];
            out[(size_t)t * woC4 + j] = make_float4(cubic4(a.x, b.x, c.x, d.x, w) / 255.0f, cubic4(a.y, b.y, c.y, d.y, w) / 255.0f,
                                                    cubic4(a.z, b.z, c.z, d.z, w) / 255.0f, cubic4(a.w, b.w, c.w, d.w, w) / 255.0f);
            j += 256;
            while (j >= woC4) { j -= woC4; ++t; }
        }
    }
}

// ---------------------------------------------------------------- fallback: one thread per output element
// Every size the entry point admits (rows that are no multiple of 16 bytes, windows beyond the LDS budget): taps computed per
// thread, sixteen byte loads, the same arithmetic in the same order.
__global__ __launch_bounds__(256) void process_image_plain_kernel(const unsigned char* __restrict__ src, int hs, int ws, int C, int S,
                                                                int crop_y, int crop_x, float* __restrict__ dst, int ho, int wo,
                                                                float sy, float sx, int total) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {       // total < 2^31 - 2^21: no wrap
        const int p = i / C, c = i - p * C;
        const int q = p / wo, x = p - q * wo;
        const int n = q / ho, y = q - n * ho;
        float4 wx, wy;
        const int tx = axis_taps(sx, x, &wx), ty = axis_taps(sy, y, &wy);
        const unsigned char* img = src + (size_t)n * hs * ws * C + ((size_t)crop_y * ws + crop_x) * C + c;
        const int x0 = clampi(tx, S - 1) * C, x1 = clampi(tx + 1, S - 1) * C, x2 = clampi(tx + 2, S - 1) * C, x3 = clampi(tx + 3, S - 1) * C;
        float h[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned char* row = img + (size_t)clampi(ty + k, S - 1) * ws * C;
            h[k] = cubic4((float)row[x0], (float)row[x1], (float)row[x2], (float)row[x3], wx);
        }
        dst[i] = cubic4(h[0], h[1], h[2], h[3], wy) / 255.0f;
    }
}

// rows of the source window the widest tile of `th` output rows needs (same fp32 products as the kernel's)
static int window_rows(float sy, int ho, int th) {
    int rmax = 0;
    for (int y0 = 0; y0 < ho; y0 += th) rmax = std::max(rmax, axis_floor(sy, std::min(y0 + th, ho) - 1) - axis_floor(sy, y0) + 4);
    return rmax;
}

static size_t tiled_lds_bytes(int S, int C, int wo, int th, int rmax) {
    return (size_t)20 * (wo + th) + 4 * ((size_t)rmax * wo * C + (((size_t)rmax * S * C + 3) & ~(size_t)3));
}

}  // namespace mv3d

using namespace mv3d;

extern "C" int mv3d_u8_process_image(const void* src, int n, int hs, int ws, int c, void* dst, int ho, int wo, void* stream) {
    if (!src || !dst) return fail(MV3D_E_INVAL, "mv3d_u8_process_image: null pointer");
    if (n < 1 || hs < 1 || ws < 1 || ho < 1 || wo < 1) return fail(MV3D_E_INVAL, "mv3d_u8_process_image: bad shape");
    if (c < 1 || c > 4) return fail(MV3D_E_INVAL, "mv3d_u8_process_image: %d channels, 1 .. 4 supported", c);
    if (hs > PI_MAX_SIDE || ws > PI_MAX_SIDE || ho > PI_MAX_SIDE || wo > PI_MAX_SIDE)
        return fail(MV3D_E_INVAL, "mv3d_u8_process_image: a side is larger than %d", PI_MAX_SIDE);
    if ((uintptr_t)dst & 15) return fail(MV3D_E_INVAL, "mv3d_u8_process_image: dst must be 16-byte aligned");
    const int64_t in_count = (int64_t)n * hs * ws * c, out_count = (int64_t)n * ho * wo * c, lim = ((int64_t)1 << 31) - ((int64_t)1 << 21);
    if (in_count >= lim || out_count >= lim) return fail(MV3D_E_INVAL, "mv3d_u8_process_image: more than 2^31 - 2^21 elements (32-bit indices)");

    const int S = std::min(hs, ws), crop_y = (hs - S) / 2, crop_x = (ws - S) / 2;
    const float sy = (float)S / (float)ho, sx = (float)S / (float)wo;
    const OpInfo info{"u8_process_image", 0.0, (double)n * S * S * c + 4.0 * (double)out_count};

    int th = 0, rmax = 0;
    size_t lds = 0;
    if ((wo * c) % 4 == 0)
        for (th = PI_MAX_TILE; th >= 1; th >>= 1) {
            rmax = window_rows(sy, ho, th);
            lds = tiled_lds_bytes(S, c, wo, th, rmax);
            if (lds <= PI_LDS_BUDGET) break;
        }
    if (th >= 1) {
        const int tiles = cdiv(ho, th);
        // 4 bytes per lane from the source when every cropped row starts on and spans a multiple of 4 bytes
        const int vec = ((uintptr_t)src & 3) == 0 && (ws * c) % 4 == 0 && (crop_x * c) % 4 == 0 && (S * c) % 4 == 0;
        return dispatch(stream, info, [=](hipStream_t s) {
            const unsigned char* in = (const unsigned char*)src;
            float* out = (float*)dst;
            const dim3 grid((unsigned)(n * tiles));                          // <= out_count < 2^31
#define MV3D_PI_LAUNCH(CH) process_image_tiled_kernel<CH><<<grid, 256, lds, s>>>(in, hs, ws, S, crop_y, crop_x, out, ho, wo, sy, sx, th, rmax, tiles, vec)
            switch (c) {
                case 1: MV3D_PI_LAUNCH(1); break;
                case 2: MV3D_PI_LAUNCH(2); break;
                case 3: MV3D_PI_LAUNCH(3); break;
                default: MV3D_PI_LAUNCH(4); break;
            }
#undef MV3D_PI_LAUNCH
            return launched("process_image_tiled_kernel");
        });
    }
    return dispatch(stream, info, [=](hipStream_t s) {
        const int blocks = (int)std::min<int64_t>(cdiv64(out_count, 256), 8192);
        process_image_plain_kernel<<<blocks, 256, 0, s>>>((const unsigned char*)src, hs, ws, c, S, crop_y, crop_x, (float*)dst, ho, wo, sy, sx,
                                                        (int)out_count);
        return launched("process_image_plain_kernel");
    });
}
