// Colour augmentation on the reader's stream: one pointwise colour map per sample (brightness, saturation + hue through one HSV
// round trip, contrast about the sample's joint channel means, clip) applied in place to all colour views of the sample.
// include/mv3d_hip.h states the contract and the summation order; augment.color_augment_host is the numpy twin and the authority:
// the reference has no augmentation and TensorFlow was never run against this.  Built with -ffp-contract=off like
// process_image.hip: every product, sum and (correctly rounded) quotient below rounds on its own.
//
// Ownership, a constant of the unit whatever the grid and the device: an image of P = h * w pixels is cut into chunks of CA_CHUNK =
// 4096 pixels; thread t of the workgroup owns the pixel quads t + 256 k, k = 0 .. CA_QUADS - 1, of its chunk (a quad = 4 RGB pixels =
// three float4s); the P & 3 pixels behind the last whole quad belong to the thread that would own that quad and are scalar.  A
// work item is one (sample, view, chunk), numbered sample-major; a workgroup takes the items blockIdx.x + r * gridDim.x.  A sample
// whose first float is not on a 16-byte boundary (P & 3 != 0, sample > 0) has its quads read and written as scalars, too.
#include "sum_common.h"
#include <algorithm>

namespace mv3d {

constexpr int CA_QUADS = 4;                               // pixel quads a lane owns per chunk: 12 x 16 bytes in flight per lane
constexpr int CA_CHUNK_QUADS = CA_QUADS * SUM_THREADS;    // 1024
constexpr int CA_CHUNK = 4 * CA_CHUNK_QUADS;              // pixels per chunk (4096): fixed
constexpr int CA_MAX_VIEWS = 8;
constexpr int CA_MAX_BLOCKS = 2048;                       // 8 workgroups per CU, beyond that a grid stride (as GN_MAX_BLOCKS)
constexpr unsigned CA_ALL = MV3D_AUG_BRIGHTNESS | MV3D_AUG_SATURATION | MV3D_AUG_HUE | MV3D_AUG_CONTRAST;

struct CaViews { float* p[CA_MAX_VIEWS]; };               // by value: a recorded launch keeps its own copy

// a select chain, not an index: the kernel argument stays in scalar registers
__device__ __forceinline__ float* view_ptr(const CaViews& V, int v) {
    float* p = V.p[0];
#pragma unroll
    for (int k = 1; k < CA_MAX_VIEWS; ++k) p = (v == k) ? V.p[k] : p;
    return p;
}

struct CaItem { int sample, view, chunk; };
__device__ __forceinline__ CaItem item_of(int item, int views, int nchunk) {
    const int iv = item / nchunk;
    return CaItem{iv / views, iv % views, item - iv * nchunk};
}

// the 12 floats of quad q of an image (q < P / 4); vec: the image starts on a 16-byte boundary
__device__ __forceinline__ void load_quad(const float* img, int q, bool vec, float (&px)[12]) {
    const float* s = img + (size_t)q * 12;
    if (vec) {
        const float4* s4 = reinterpret_cast<const float4*>(s);
        const float4 a = s4[0], b = s4[1], c = s4[2];
        px[0] = a.x; px[1] = a.y; px[2] = a.z; px[3] = a.w;
        px[4] = b.x; px[5] = b.y; px[6] = b.z; px[7] = b.w;
        px[8] = c.x; px[9] = c.y; px[10] = c.z; px[11] = c.w;
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) px[j] = s[j];
    }
}
__device__ __forceinline__ void store_quad(float* img, int q, bool vec, const float (&px)[12]) {
    float* d = img + (size_t)q * 12;
    if (vec) {
        float4* d4 = reinterpret_cast<float4*>(d);
        d4[0] = make_float4(px[0], px[1], px[2], px[3]);
        d4[1] = make_float4(px[4], px[5], px[6], px[7]);
        d4[2] = make_float4(px[8], px[9], px[10], px[11]);
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) d[j] = px[j];
    }
}

// ---------------------------------------------------------------- chunk sums (MV3D_AUG_CONTRAST only)
// part[item * 3 + ch] = the double sum of channel ch over the item's chunk, in the header's order.  Pixels past the image add 0.
__global__ __launch_bounds__(SUM_THREADS) void color_augment_sums_kernel(CaViews V, int views, int P, int nchunk, int items,
                                                                         double* __restrict__ part) {
    __shared__ double s_red[12];
    const int tid = threadIdx.x;
    const int nquad = P >> 2, tail = P & 3;
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        const CaItem it = item_of(item, views, nchunk);
        const size_t first = (size_t)it.sample * P * 3;
        const float* img = view_ptr(V, it.view) + first;
        const bool vec = (first & 3) == 0;
        float px[CA_QUADS][12];
#pragma unroll
        for (int k = 0; k < CA_QUADS; ++k) {
            const int q = it.chunk * CA_CHUNK_QUADS + k * SUM_THREADS + tid;
#pragma unroll
            for (int j = 0; j < 12; ++j) px[k][j] = 0.0f;
            if (q < nquad) {
                load_quad(img, q, vec, px[k]);
            } else if (q == nquad && tail) {
                const float* s = img + (size_t)q * 12;
#pragma unroll
                for (int j = 0; j < 9; ++j)
                    if (j < 3 * tail) px[k][j] = s[j];
            }
        }
        double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < CA_QUADS; ++k)
#pragma unroll
            for (int j = 0; j < 12; j += 3) {
                acc[0] += (double)px[k][j];
                acc[1] += (double)px[k][j + 1];
                acc[2] += (double)px[k][j + 2];
            }
        block_sum(acc, s_red, tid);
        if (tid < 3) part[(size_t)item * 3 + tid] = block_total(s_red, tid);
        __syncthreads();                                  // s_red is written again by the next item
    }
}

// ---------------------------------------------------------------- the map
struct CaParams { float db, fs, dh, fc; };

// The contract's x < 0 ? 0 : x > 1 ? 1 : x by value for every finite x (a zero may come out with the other sign); the compiler folds
// the median into the clamp modifier of the instruction that produced x, so a clip costs no instruction of its own.
__device__ __forceinline__ float clip01(float x) { return __builtin_amdgcn_fmed3f(x, 0.0f, 1.0f); }

// Straight-line code, selects only: the stage mask is a template argument, so the four pixels of a quad interleave and no lane
// ever branches.  max / min of clipped (finite) values as v_max3 / v_min3: the contract's a > b ? a : b by value.
template <unsigned ST>
__device__ __forceinline__ void color_map(float& r, float& g, float& b, const CaParams& p, float pr, float pg, float pb) {
#pragma clang fp contract(off)
    if (ST & MV3D_AUG_BRIGHTNESS) {
        r = r + p.db;
        g = g + p.db;
        b = b + p.db;
    }
    if (ST & (MV3D_AUG_SATURATION | MV3D_AUG_HUE)) {
        r = clip01(r);
        g = clip01(g);
        b = clip01(b);
        const float v = __builtin_fmaxf(__builtin_fmaxf(r, g), b);
        const float mn = __builtin_fminf(__builtin_fminf(r, g), b);
        const float range = v - mn;
        float s = v > 0.0f ? range / v : 0.0f;
        const float norm = 1.0f / (6.0f * range);
        // h = r == v ? (g - b) * norm : g == v ? (b - r) * norm + 2/6 : (r - g) * norm + 4/6 with the operands selected first
        // (the r branch adds 0: the same value)
        const bool isr = r == v, isg = g == v;
        const float ha = isr ? g : isg ? b : r;
        const float hb = isr ? b : isg ? r : g;
        const float ho = isr ? 0.0f : isg ? 2.0f / 6.0f : 4.0f / 6.0f;
        float h = (ha - hb) * norm + ho;
        h = range <= 0.0f ? 0.0f : h;
        h = h < 0.0f ? h + 1.0f : h;
        if (ST & MV3D_AUG_SATURATION) s = clip01(s * p.fs);
        if (ST & MV3D_AUG_HUE) h = h + p.dh;
        h = h - floorf(h);
        const float c = s * v;
        const float m = v - c;
        const float d = h * 6.0f;
        int k = (int)d;
        k = k < 5 ? k : 5;                                // h can round to exactly 1.0
        const float f = d - 2.0f * floorf(d / 2.0f);
        const float x = c * (1.0f - fabsf(f - 1.0f));
        r = m + ((k == 0 || k == 5) ? c : (k == 1 || k == 4) ? x : 0.0f);
        g = m + ((k == 1 || k == 2) ? c : (k == 0 || k == 3) ? x : 0.0f);
        b = m + ((k == 3 || k == 4) ? c : (k == 2 || k == 5) ? x : 0.0f);
    }
    if (ST & MV3D_AUG_CONTRAST) {
        r = (r - pr) * p.fc + pr;
        g = (g - pg) * p.fc + pg;
        b = (b - pb) * p.fc + pb;
    }
    r = clip01(r);
    g = clip01(g);
    b = clip01(b);
}

// One pass, in place: 4 bytes read and 4 written per element, 16 bytes per lane and access, the 12 loads of a lane's four quads
// issued before the first use.  No LDS traffic but the pivot's three floats, rebuilt from the chunk sums whenever the workgroup meets
// a new sample: threads 0 .. 2 add their channel's partials views ascending, chunks ascending within a view, divide by views * P in
// double and round to float once.  Which lane maps which pixel does not matter to the result; the items are the sums kernel's.
template <unsigned ST>
__global__ __launch_bounds__(SUM_THREADS) void color_augment_apply_kernel(CaViews V, int views, int P, int nchunk, int items,
                                                                          const float* __restrict__ params,
                                                                          const double* __restrict__ part) {
    __shared__ float s_piv[3];
    const int tid = threadIdx.x;
    const int nquad = P >> 2, tail = P & 3;
    int have = -1;                                        // the sample s_piv belongs to
    float pr = 0.0f, pg = 0.0f, pb = 0.0f;
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        const CaItem it = item_of(item, views, nchunk);
        if ((ST & MV3D_AUG_CONTRAST) && it.sample != have) {
            if (have >= 0) __syncthreads();               // everyone has read the previous pivot
            if (tid < 3) {
                const double* ps = part + (size_t)it.sample * views * nchunk * 3 + tid;
                double s = 0.0;
                for (int j = 0; j < views * nchunk; ++j) s += ps[(size_t)j * 3];
                s_piv[tid] = (float)(s / ((double)views * (double)P));
            }
            __syncthreads();
            pr = s_piv[0];
            pg = s_piv[1];
            pb = s_piv[2];
            have = it.sample;
        }
        const float4 pv = *reinterpret_cast<const float4*>(params + (size_t)it.sample * 4);
        const CaParams p{pv.x, pv.y, pv.z, pv.w};
        const size_t first = (size_t)it.sample * P * 3;
        float* img = view_ptr(V, it.view) + first;
        const bool vec = (first & 3) == 0;
        const int q0 = it.chunk * CA_CHUNK_QUADS + tid;
        float px[CA_QUADS][12];
        if (vec && (it.chunk + 1) * CA_CHUNK_QUADS <= nquad) {            // a whole chunk on 16-byte accesses: the hot path
#pragma unroll
            for (int k = 0; k < CA_QUADS; ++k) load_quad(img, q0 + k * SUM_THREADS, true, px[k]);
#pragma unroll
            for (int k = 0; k < CA_QUADS; ++k) {
#pragma unroll
                for (int j = 0; j < 12; j += 3) color_map<ST>(px[k][j], px[k][j + 1], px[k][j + 2], p, pr, pg, pb);
                store_quad(img, q0 + k * SUM_THREADS, true, px[k]);
            }
            continue;
        }
        for (int k = 0; k < CA_QUADS; ++k) {
            const int q = q0 + k * SUM_THREADS;
            if (q < nquad) {
                load_quad(img, q, vec, px[0]);
#pragma unroll
                for (int j = 0; j < 12; j += 3) color_map<ST>(px[0][j], px[0][j + 1], px[0][j + 2], p, pr, pg, pb);
                store_quad(img, q, vec, px[0]);
            } else if (q == nquad && tail) {
                float* s = img + (size_t)q * 12;
                for (int j = 0; j < tail; ++j) {
                    float r = s[3 * j], g = s[3 * j + 1], b = s[3 * j + 2];
                    color_map<ST>(r, g, b, p, pr, pg, pb);
                    s[3 * j] = r;
                    s[3 * j + 1] = g;
                    s[3 * j + 2] = b;
                }
            }
        }
    }
}

static inline int ca_chunks(int64_t P) { return (int)cdiv64(P, CA_CHUNK); }

}  // namespace mv3d

using namespace mv3d;

extern "C" {

size_t mv3d_color_augment_workspace_bytes(int n, int views, int h, int w) {
    if (n < 1 || views < 1 || views > CA_MAX_VIEWS || h < 1 || w < 1) return 0;
    return (size_t)n * views * ca_chunks((int64_t)h * w) * 3 * sizeof(double);
}

int mv3d_color_augment(void* const* images, int views, int n, int h, int w, const void* params, unsigned stages, void* workspace,
                       size_t workspace_bytes, void* stream) {
    const char* fn = "mv3d_color_augment";
    if (!images || !params || !workspace) return fail(MV3D_E_INVAL, "%s: images, params or workspace is null", fn);
    if (views < 1 || views > CA_MAX_VIEWS) return fail(MV3D_E_INVAL, "%s: %d views, 1 .. %d supported", fn, views, CA_MAX_VIEWS);
    if (n < 1 || h < 1 || w < 1) return fail(MV3D_E_INVAL, "%s: bad shape (n %d, h %d, w %d)", fn, n, h, w);
    const int64_t P = (int64_t)h * w, count = (int64_t)n * P * 3, lim = ((int64_t)1 << 31) - ((int64_t)1 << 21);
    if (P >= lim || count >= lim) return fail(MV3D_E_INVAL, "%s: more than 2^31 - 2^21 elements per view (32-bit indices)", fn);
    if (stages == 0 || (stages & ~CA_ALL)) return fail(MV3D_E_INVAL, "%s: stage mask 0x%x (no stage, or unknown bits)", fn, stages);
    if ((uintptr_t)params & 15) return fail(MV3D_E_INVAL, "%s: params must be 16-byte aligned", fn);
    CaViews V;
    for (int v = 0; v < CA_MAX_VIEWS; ++v) V.p[v] = nullptr;
    const uint64_t bytes = 4 * (uint64_t)count;
    for (int v = 0; v < views; ++v) {
        if (!images[v]) return fail(MV3D_E_INVAL, "%s: view %d is null", fn, v);
        if ((uintptr_t)images[v] & 15) return fail(MV3D_E_INVAL, "%s: view %d must be 16-byte aligned", fn, v);
        for (int u = 0; u < v; ++u) {
            const uintptr_t a = (uintptr_t)images[u], b = (uintptr_t)images[v];
            if (a == b || (a < b ? b - a < bytes : a - b < bytes))
                return fail(MV3D_E_INVAL, "%s: views %d and %d are equal or overlap", fn, u, v);
        }
        V.p[v] = (float*)images[v];
    }
    const size_t need = mv3d_color_augment_workspace_bytes(n, views, h, w);
    if (workspace_bytes < need) return fail(MV3D_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    if ((uintptr_t)workspace & 15) return fail(MV3D_E_WORKSPACE, "%s: workspace not 16-byte aligned", fn);
    const int nchunk = ca_chunks(P);
    const int64_t items64 = (int64_t)n * views * nchunk;          // <= 8 * count / 3 / 4096 + 8 n: fits an int
    const int items = (int)items64;
    // the grid: one workgroup per item up to CA_MAX_BLOCKS, beyond that every workgroup walks the same number of items
    const int rounds = (int)cdiv64(items64, CA_MAX_BLOCKS);
    const int blocks = (int)cdiv64(items64, rounds);
    const int Pi = (int)P;
    const float* par = (const float*)params;
    double* part = (double*)workspace;
    const double elems = (double)count * views;
    if (stages & MV3D_AUG_CONTRAST) {
        int rc = dispatch(stream, OpInfo{"color_augment_sums_kernel", elems, 4.0 * elems}, [=](hipStream_t s) {
            color_augment_sums_kernel<<<blocks, SUM_THREADS, 0, s>>>(V, views, Pi, nchunk, items, part);
            return launched("color_augment_sums_kernel");
        });
        if (rc != MV3D_OK) return rc;
    }
    return dispatch(stream, OpInfo{"color_augment_apply_kernel", 0.0, 8.0 * elems}, [=](hipStream_t s) {
#define MV3D_CA_LAUNCH(ST) case ST: color_augment_apply_kernel<ST><<<blocks, SUM_THREADS, 0, s>>>(V, views, Pi, nchunk, items, par, part); break;
        switch (stages) {                                 // one instance per stage mask
            MV3D_CA_LAUNCH(1) MV3D_CA_LAUNCH(2) MV3D_CA_LAUNCH(3) MV3D_CA_LAUNCH(4) MV3D_CA_LAUNCH(5)
            MV3D_CA_LAUNCH(6) MV3D_CA_LAUNCH(7) MV3D_CA_LAUNCH(8) MV3D_CA_LAUNCH(9) MV3D_CA_LAUNCH(10)
            MV3D_CA_LAUNCH(11) MV3D_CA_LAUNCH(12) MV3D_CA_LAUNCH(13) MV3D_CA_LAUNCH(14) MV3D_CA_LAUNCH(15)
        }
#undef MV3D_CA_LAUNCH
        return launched("color_augment_apply_kernel");
    });
}

}  // extern "C"
