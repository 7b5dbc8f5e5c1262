// Geometric augmentation on the reader's stream: per sample ONE left-right flip, centred zoom-in and window shift, applied out of
// place to all of the sample's views (3-channel views bilinearly, 1-channel views -- masks, depth maps -- by the nearest pixel), and
// the sign of disp[:, 1] under a flip.  include/mv3d_hip.h states the contract; augment.geom_augment_host is the numpy twin and the
// authority: the reference has no augmentation and TensorFlow was never run against this.  Built with -ffp-contract=off like
// color_augment.hip: every difference, product and sum below rounds on its own.
//
// Ownership, a constant of the unit whatever the grid and the device: a row of w pixels is cut into quads of 4 consecutive pixels
// (the last one short when w & 3); the h * ceil(w / 4) quads of an image are numbered row-major and cut into chunks of GG_CHUNK_QUADS;
// thread t of the workgroup owns the quads t + 256 k, k = 0 .. GG_QUADS - 1, of its chunk.  A work item is one (sample, view, chunk),
// numbered sample-major; a workgroup takes the items blockIdx.x + r * gridDim.x.  A lane writes its quad as 16-byte stores (three
// for a 3-channel view, one for a 1-channel view) when the quad is whole and its row starts on a 16-byte boundary, else as scalars.
// The gathers go through the caches: with a zoom s >= 1 the source footprint of a wave is no wider than what it writes.
#include "common.h"
#include <algorithm>

namespace mv3d {

constexpr int GG_THREADS = 256;
constexpr int GG_QUADS = 2;                               // quads a lane owns per chunk
constexpr int GG_CHUNK_QUADS = GG_QUADS * GG_THREADS;     // 512 quads = 2048 pixels
constexpr int GG_MAX_VIEWS = 16;
constexpr int GG_MAX_BLOCKS = 2048;                       // 8 workgroups per CU, beyond that a grid stride (as CA_MAX_BLOCKS)

struct GgViews {                                          // by value: a recorded launch keeps its own copy
    const float* src[GG_MAX_VIEWS];
    float* dst[GG_MAX_VIEWS];
    unsigned rgb;                                         // bit v: view v has 3 channels (else 1)
};

struct GgPixel { float r, g, b; };                        // 4-byte aligned: one 12-byte load per tap

// select chains, not an index: the kernel argument stays in scalar registers
__device__ __forceinline__ const float* gg_src(const GgViews& V, int v) {
    const float* p = V.src[0];
#pragma unroll
    for (int k = 1; k < GG_MAX_VIEWS; ++k) p = (v == k) ? V.src[k] : p;
    return p;
}
__device__ __forceinline__ float* gg_dst(const GgViews& V, int v) {
    float* p = V.dst[0];
#pragma unroll
    for (int k = 1; k < GG_MAX_VIEWS; ++k) p = (v == k) ? V.dst[k] : p;
    return p;
}

// the clamped source coordinate of output coordinate p (already mirrored): fmaxf / fminf give 0 for a NaN, so it is in [0, hi]
// whatever the parameters hold
__device__ __forceinline__ float gg_coord(float p, float c, float inv, float co, float hi) {
#pragma clang fp contract(off)
    const float s = (p - c) * inv + co;
    return fminf(fmaxf(s, 0.0f), hi);
}

__device__ __forceinline__ float gg_lerp(float a, float b, float f) {
#pragma clang fp contract(off)
    return a + (b - a) * f;
}

__global__ __launch_bounds__(GG_THREADS) void geom_augment_kernel(GgViews V, int views, int h, int w, int qpr, int nquad, int nchunk,
                                                                  int items, const float* __restrict__ params, float* disp) {
    const int tid = threadIdx.x;
    const float cx = 0.5f * (float)(w - 1), cy = 0.5f * (float)(h - 1);       // exact
    const float xhi = (float)(w - 1), yhi = (float)(h - 1);
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        const int iv = item / nchunk;
        const int chunk = item - iv * nchunk;
        const int sample = iv / views, view = iv - sample * views;
        const float4 pv = *reinterpret_cast<const float4*>(params + (size_t)sample * 4);
        const bool flip = pv.x != 0.0f;
        const float inv = pv.y, cxo = pv.z, cyo = pv.w;
        if (disp && view == 0 && chunk == 0 && tid == 0) {                    // one lane per sample
            const float d = disp[2 * (size_t)sample + 1];
            disp[2 * (size_t)sample + 1] = flip ? -d : d;
        }
        const bool rgb = (V.rgb >> view) & 1u;
        const size_t first = (size_t)sample * h * w;                          // in pixels
        const float* src = gg_src(V, view);
        float* dst = gg_dst(V, view);
#pragma unroll
        for (int k = 0; k < GG_QUADS; ++k) {
            const int Q = chunk * GG_CHUNK_QUADS + k * GG_THREADS + tid;
            if (Q >= nquad) continue;
            const int y = Q / qpr;
            const int x4 = (Q - y * qpr) * 4;
            const size_t row = first + (size_t)y * w;                         // the output row, in pixels
            const bool vec = x4 + 3 < w && (row & 3) == 0;
            const float ys = gg_coord((float)y, cy, inv, cyo, yhi);
            if (rgb) {
                const float fy0 = floorf(ys);
                const int y0 = (int)fy0, y1 = min(y0 + 1, h - 1);
                const float fy = ys - fy0;
                const GgPixel* r0 = reinterpret_cast<const GgPixel*>(src) + first + (size_t)y0 * w;
                const GgPixel* r1 = reinterpret_cast<const GgPixel*>(src) + first + (size_t)y1 * w;
                GgPixel a[4], b[4], c[4], d[4];
                float fx[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {                                 // 16 loads issued before the first use
                    const int x = min(x4 + j, w - 1);                         // a pixel past the row repeats the last one; not stored
                    const float xs = gg_coord((float)(flip ? (w - 1) - x : x), cx, inv, cxo, xhi);
                    const float fx0 = floorf(xs);
                    const int x0 = (int)fx0, x1 = min(x0 + 1, w - 1);
                    fx[j] = xs - fx0;
                    a[j] = r0[x0];
                    b[j] = r0[x1];
                    c[j] = r1[x0];
                    d[j] = r1[x1];
                }
                float px[12];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    px[3 * j] = gg_lerp(gg_lerp(a[j].r, b[j].r, fx[j]), gg_lerp(c[j].r, d[j].r, fx[j]), fy);
                    px[3 * j + 1] = gg_lerp(gg_lerp(a[j].g, b[j].g, fx[j]), gg_lerp(c[j].g, d[j].g, fx[j]), fy);
                    px[3 * j + 2] = gg_lerp(gg_lerp(a[j].b, b[j].b, fx[j]), gg_lerp(c[j].b, d[j].b, fx[j]), fy);
                }
                float* o = dst + (row + x4) * 3;
                if (vec) {
                    float4* o4 = reinterpret_cast<float4*>(o);
                    o4[0] = make_float4(px[0], px[1], px[2], px[3]);
                    o4[1] = make_float4(px[4], px[5], px[6], px[7]);
                    o4[2] = make_float4(px[8], px[9], px[10], px[11]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x4 + j < w) {
                            o[3 * j] = px[3 * j];
                            o[3 * j + 1] = px[3 * j + 1];
                            o[3 * j + 2] = px[3 * j + 2];
                        }
                }
            } else {
                const int yi = min((int)floorf(ys + 0.5f), h - 1);
                const float* r = src + first + (size_t)yi * w;
                float px[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int x = min(x4 + j, w - 1);
                    const float xs = gg_coord((float)(flip ? (w - 1) - x : x), cx, inv, cxo, xhi);
                    px[j] = r[min((int)floorf(xs + 0.5f), w - 1)];
                }
                float* o = dst + row + x4;
                if (vec) {
                    *reinterpret_cast<float4*>(o) = make_float4(px[0], px[1], px[2], px[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x4 + j < w) o[j] = px[j];
                }
            }
        }
    }
}

}  // namespace mv3d

using namespace mv3d;

extern "C" {

int mv3d_geom_augment(const void* const* src, void* const* dst, const int* channels, int views, int n, int h, int w,
                      const void* params, void* disp, void* stream) {
    const char* fn = "mv3d_geom_augment";
    if (!src || !dst || !channels || !params) return fail(MV3D_E_INVAL, "%s: src, dst, channels or params is null", fn);
    if (views < 1 || views > GG_MAX_VIEWS) return fail(MV3D_E_INVAL, "%s: %d views, 1 .. %d supported", fn, views, GG_MAX_VIEWS);
    if (n < 1 || h < 1 || w < 1) return fail(MV3D_E_INVAL, "%s: bad shape (n %d, h %d, w %d)", fn, n, h, w);
    const int64_t P = (int64_t)h * w, count = (int64_t)n * P * 3, lim = ((int64_t)1 << 31) - ((int64_t)1 << 21);
    if (P >= lim || count >= lim) return fail(MV3D_E_INVAL, "%s: more than 2^31 - 2^21 elements per view (32-bit indices)", fn);
    if ((uintptr_t)params & 15) return fail(MV3D_E_INVAL, "%s: params must be 16-byte aligned", fn);
    if ((uintptr_t)disp & 15) return fail(MV3D_E_INVAL, "%s: disp must be 16-byte aligned", fn);
    GgViews V;
    V.rgb = 0;
    for (int v = 0; v < GG_MAX_VIEWS; ++v) {
        V.src[v] = nullptr;
        V.dst[v] = nullptr;
    }
    uintptr_t at[2 * GG_MAX_VIEWS];                       // sources, then destinations
    uint64_t bytes[2 * GG_MAX_VIEWS];
    double elems = 0.0;
    for (int v = 0; v < views; ++v) {
        if (channels[v] != 1 && channels[v] != 3) return fail(MV3D_E_INVAL, "%s: view %d has %d channels, 1 or 3 supported", fn, v, channels[v]);
        if (!src[v] || !dst[v]) return fail(MV3D_E_INVAL, "%s: view %d is null", fn, v);
        if (((uintptr_t)src[v] | (uintptr_t)dst[v]) & 15) return fail(MV3D_E_INVAL, "%s: view %d must be 16-byte aligned", fn, v);
        at[v] = (uintptr_t)src[v];
        at[views + v] = (uintptr_t)dst[v];
        bytes[v] = bytes[views + v] = 4 * (uint64_t)n * (uint64_t)P * (uint64_t)channels[v];
        elems += (double)n * (double)P * channels[v];
        V.src[v] = (const float*)src[v];
        V.dst[v] = (float*)dst[v];
        if (channels[v] == 3) V.rgb |= 1u << v;
    }
    for (int i = 0; i < 2 * views; ++i)
        for (int j = i + 1; j < 2 * views; ++j) {
            const uintptr_t a = at[i], b = at[j];
            if (a == b || (a < b ? b - a < bytes[i] : a - b < bytes[j]))
                return fail(MV3D_E_INVAL, "%s: %s %d and %s %d are equal or overlap", fn, i < views ? "source" : "destination",
                            i < views ? i : i - views, j < views ? "source" : "destination", j < views ? j : j - views);
        }
    const int qpr = (w + 3) / 4;
    const int64_t nquad64 = (int64_t)h * qpr;             // <= P
    const int nchunk = (int)cdiv64(nquad64, GG_CHUNK_QUADS);
    const int64_t items64 = (int64_t)n * views * nchunk;  // <= 16 * (count / 3 / 512 + n): fits an int
    if (items64 >= lim) return fail(MV3D_E_INVAL, "%s: too many work items", fn);
    const int items = (int)items64, nquad = (int)nquad64;
    // the grid: one workgroup per item up to GG_MAX_BLOCKS, beyond that every workgroup walks the same number of items
    const int rounds = (int)cdiv64(items64, GG_MAX_BLOCKS);
    const int blocks = (int)cdiv64(items64, rounds);
    const float* par = (const float*)params;
    float* dsp = (float*)disp;
    return dispatch(stream, OpInfo{"geom_augment_kernel", 0.0, 8.0 * elems}, [=](hipStream_t s) {
        geom_augment_kernel<<<blocks, GG_THREADS, 0, s>>>(V, views, h, w, qpr, nquad, nchunk, items, par, dsp);
        return launched("geom_augment_kernel");
    });
}

}  // extern "C"
