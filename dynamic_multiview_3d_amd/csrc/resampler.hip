// The plain bilinear resampler: tf.contrib.resampler.resampler(data, warp) for ANY warp tensor (tf_utils.py:40-42), with
// the gradients w.r.t. both inputs.  The warp + resampler kernels of elem.hip cover only warp = flow + coords; these take
// the warp as it is (channel 0 = x = column, channel 1 = y = row).
//
// Built with -ffp-contract=off: the expressions and their operation order are those of resample_kernel (elem.hip), so
// the fp32 results round like the unfused TF kernels and the numpy oracle (oracle/ops.py resampler_fwd / resampler_bwd).
//
// The data gradient is a scatter-add.  It is accumulated in 64-bit fixed point so that it is the same bit for bit from run
// to run: integer addition is associative, so the order in which the atomics arrive cannot change the sum (float atomics
// could).  Three launches:
//   prep   zero the int64 accumulator and write one max|dout| per workgroup into a partial row
//   bwd    every workgroup reduces that row to gmax and picks k with N*P*gmax*2^k <= 2^62; every tap of a valid point adds
//          llrint(g * w * 2^k) to its destination (a point's four weights sum to <= 1, so no destination can overflow);
//          the warp gradient is computed in the same pass
//   final  ddata = acc * 2^-k into the strided fp32 output
// The accumulator is channel-planar, [N,C,Hs,Ws]: neighbouring points scatter to neighbouring 8-byte words, so one wave's atomics
// cover a few contiguous segments instead of one word every C*8 bytes.
// A max is order-independent too, and k is a function of the row alone, so every launch sees the same k.  No value ever
// comes back to the host: the sequence records into plans (mv3d_plan_*).
#include "common.h"
#include <algorithm>

namespace mv3d {
namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_PARTS = 1024;          // workgroups of the prep launch = length of the partial row
constexpr int RS_MAX_GRID = 4096;       // grid-stride loops beyond this
constexpr int64_t RS_MAX_ELEMS = int64_t(1) << 40;
constexpr int RS_MAX_SIDE = 1 << 24;    // Hs, Ws: exact as fp32, so the validity test x < Ws is exact

struct RsArgs {
    const float* data; const float* warp; const float* g;     // g: dout (bwd)
    float* out; float* dwarp; float* ddata;                    // out: fwd only
    unsigned long long* acc; float* part;
    int64_t NP, P, nacc;                                       // nacc = N*C*Hs*Ws (the accumulator)
    int Hs, Ws, C, data_ld, warp_ld, g_ld, dwarp_ld, ddata_ld; // g_ld: out_ld (fwd) / dout_ld (bwd)
    int nparts;
    bool w2;                                                   // warp (and dwarp) rows are 8-byte aligned float2
};

struct Cell {
    float dx, dy;
    int fx, fy;
    bool valid;
};

// A point is valid iff -1 < x < Ws and -1 < y < Hs (NaN and +-inf are not).  The clamp keeps the int conversion defined
// for far-away and non-finite coordinates; it cannot move a valid point, whose floor lies in [-1, W-1].
__device__ __forceinline__ Cell cell_of(float x, float y, int Hs, int Ws) {
    Cell k;
    k.valid = x > -1.0f && y > -1.0f && x < (float)Ws && y < (float)Hs;
    const float fxf = floorf(x), fyf = floorf(y);
    k.fx = (int)fminf(fmaxf(fxf, -2.0f), (float)Ws);
    k.fy = (int)fminf(fmaxf(fyf, -2.0f), (float)Hs);
    k.dx = (fxf + 1.0f) - x;
    k.dy = (fyf + 1.0f) - y;
    return k;
}

__device__ __forceinline__ float2 load_xy(const float* w, int64_t p, int ld, bool w2) {
    const float* q = w + p * ld;
    if (w2) return *reinterpret_cast<const float2*>(q);
    return make_float2(q[0], q[1]);
}

// The four taps ff (fy,fx), cc (cy,cx), fc (cy,fx), cf (fy,cx): pixel index inside the image from CLAMPED coordinates (an
// address is never formed from an unclamped one) and whether the tap lies inside the image.
__device__ __forceinline__ void taps_of(const Cell& k, int Hs, int Ws, int64_t pix[4], bool ok[4]) {
    const int cx = k.fx + 1, cy = k.fy + 1;
    const int xs[4] = {k.fx, cx, k.fx, cx}, ys[4] = {k.fy, cy, cy, k.fy};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        ok[q] = (unsigned)xs[q] < (unsigned)Ws && (unsigned)ys[q] < (unsigned)Hs;
        const int xc = min(max(xs[q], 0), Ws - 1), yc = min(max(ys[q], 0), Hs - 1);
        pix[q] = (int64_t)yc * Ws + xc;
    }
}

__device__ __forceinline__ float bilerp(const Cell& k, float iff, float icc, float ifc, float icf) {
    const float dx = k.dx, dy = k.dy;
    return ((dx * dy * iff + (1.0f - dx) * (1.0f - dy) * icc) + dx * (1.0f - dy) * ifc) + (1.0f - dx) * dy * icf;
}

__device__ __forceinline__ float4 keep(bool ok, float4 v) {
    return make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
}

// ---------------------------------------------------------------- forward
// One point per lane; taps of all C <= 4 channels are loaded (unconditionally, from clamped addresses) before any is used.
// CT = 0: any channel count, one channel at a time.
template <int CT>
__global__ __launch_bounds__(RS_THREADS) void rs_fwd_kernel(const RsArgs a) {
    const int C = CT > 0 ? CT : a.C;
    const int64_t img = (int64_t)a.Hs * a.Ws * a.data_ld;
    for (int64_t p = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; p < a.NP; p += (int64_t)gridDim.x * RS_THREADS) {
        const float2 xy = load_xy(a.warp, p, a.warp_ld, a.w2);
        const Cell k = cell_of(xy.x, xy.y, a.Hs, a.Ws);
        int64_t pix[4];
        bool ok[4];
        taps_of(k, a.Hs, a.Ws, pix, ok);
        const float* src = a.data + (p / a.P) * img;
        float* o = a.out + p * a.g_ld;
        if constexpr (CT > 0) {
            float t[4][CT > 0 ? CT : 1];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int c = 0; c < (CT > 0 ? CT : 1); ++c) t[q][c] = src[pix[q] * a.data_ld + c];
#pragma unroll
            for (int c = 0; c < (CT > 0 ? CT : 1); ++c) {
                const float v = bilerp(k, ok[0] ? t[0][c] : 0.f, ok[1] ? t[1][c] : 0.f, ok[2] ? t[2][c] : 0.f, ok[3] ? t[3][c] : 0.f);
                o[c] = k.valid ? v : 0.f;
            }
        } else {
            for (int c = 0; c < C; ++c) {
                const float t0 = src[pix[0] * a.data_ld + c], t1 = src[pix[1] * a.data_ld + c];
                const float t2 = src[pix[2] * a.data_ld + c], t3 = src[pix[3] * a.data_ld + c];
                const float v = bilerp(k, ok[0] ? t0 : 0.f, ok[1] ? t1 : 0.f, ok[2] ? t2 : 0.f, ok[3] ? t3 : 0.f);
                o[c] = k.valid ? v : 0.f;
            }
        }
    }
}

// C % 4 == 0 (feature maps): lanes run along the channels of a point, 16-byte loads and stores.
__global__ __launch_bounds__(RS_THREADS) void rs_fwd_vec4_kernel(const RsArgs a) {
    const int C4 = a.C >> 2;
    const int64_t total = a.NP * C4, img = (int64_t)a.Hs * a.Ws * a.data_ld;
    for (int64_t t = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; t < total; t += (int64_t)gridDim.x * RS_THREADS) {
        const int64_t p = t / C4;
        const int c = (int)(t - p * C4) * 4;
        const float2 xy = load_xy(a.warp, p, a.warp_ld, a.w2);
        const Cell k = cell_of(xy.x, xy.y, a.Hs, a.Ws);
        int64_t pix[4];
        bool ok[4];
        taps_of(k, a.Hs, a.Ws, pix, ok);
        const float* src = a.data + (p / a.P) * img + c;
        const float4 l0 = *reinterpret_cast<const float4*>(src + pix[0] * a.data_ld), l1 = *reinterpret_cast<const float4*>(src + pix[1] * a.data_ld);
        const float4 l2 = *reinterpret_cast<const float4*>(src + pix[2] * a.data_ld), l3 = *reinterpret_cast<const float4*>(src + pix[3] * a.data_ld);
        const float4 v0 = keep(ok[0], l0), v1 = keep(ok[1], l1), v2 = keep(ok[2], l2), v3 = keep(ok[3], l3);
        float4 r;
        r.x = bilerp(k, v0.x, v1.x, v2.x, v3.x);
        r.y = bilerp(k, v0.y, v1.y, v2.y, v3.y);
        r.z = bilerp(k, v0.z, v1.z, v2.z, v3.z);
        r.w = bilerp(k, v0.w, v1.w, v2.w, v3.w);
        *reinterpret_cast<float4*>(a.out + p * a.g_ld + c) = keep(k.valid, r);
    }
}

// ---------------------------------------------------------------- backward
// every thread of the workgroup calls this
__device__ __forceinline__ float block_max(float v) {
    __shared__ float s_w[RS_THREADS / 64];
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(s_w[0], s_w[1]), fmaxf(s_w[2], s_w[3]));
}

// k such that NP * gmax * 2^k <= 2^62 (0 when every |dout| is 0 or gmax is not finite).  Every thread of the workgroup calls it.
__device__ __forceinline__ int block_shift(const float* part, int nparts, int64_t NP) {
    float m = 0.f;
    for (int i = threadIdx.x; i < nparts; i += RS_THREADS) m = fmaxf(m, part[i]);
    m = block_max(m);
    if (!(m > 0.f) || !isfinite(m)) return 0;
    int e;
    frexp((double)m * (double)NP, &e);          // NP * gmax < 2^e (a rounded product stays in that binade or moves up)
    return 62 - e;
}

__global__ __launch_bounds__(RS_THREADS) void rs_prep_kernel(const RsArgs a) {
    const int64_t stride = (int64_t)gridDim.x * RS_THREADS, i0 = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    ulonglong2* acc2 = reinterpret_cast<ulonglong2*>(a.acc);
    for (int64_t i = i0; i < a.nacc / 2; i += stride) acc2[i] = make_ulonglong2(0ull, 0ull);
    if (i0 == 0 && (a.nacc & 1)) a.acc[a.nacc - 1] = 0ull;
    float m = 0.f;
    const int64_t total = a.NP * a.C;
    if (a.g_ld == a.C) {
        for (int64_t t = i0; t < total; t += stride) m = fmaxf(m, fabsf(a.g[t]));
    } else {
        for (int64_t t = i0; t < total; t += stride) {
            const int64_t p = t / a.C;
            m = fmaxf(m, fabsf(a.g[p * a.g_ld + (t - p * a.C)]));
        }
    }
    m = block_max(m);
    if (threadIdx.x == 0) a.part[blockIdx.x] = m;
}

// One point per lane.  The warp gradient sums the channels in order c = 0..C-1 (V4: four at a time, still in order), so it
// is deterministic and the same with and without the data gradient.  acc != nullptr: scatter the data gradient.
template <int CT, bool V4>
__global__ __launch_bounds__(RS_THREADS) void rs_bwd_kernel(const RsArgs a) {
    const int C = CT > 0 ? CT : a.C;
    double scale = 0.0;
    if (a.acc) scale = ldexp(1.0, block_shift(a.part, a.nparts, a.NP));
    const int64_t img = (int64_t)a.Hs * a.Ws;
    for (int64_t p = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; p < a.NP; p += (int64_t)gridDim.x * RS_THREADS) {
        const float2 xy = load_xy(a.warp, p, a.warp_ld, a.w2);
        const Cell k = cell_of(xy.x, xy.y, a.Hs, a.Ws);
        float gx = 0.f, gy = 0.f;
        if (k.valid) {
            int64_t pix[4];
            bool ok[4];
            taps_of(k, a.Hs, a.Ws, pix, ok);
            const int64_t n = p / a.P;
            const float* src = a.data + n * img * a.data_ld;
            const float* g = a.g + p * a.g_ld;
            const float dx = k.dx, dy = k.dy;
            const float w[4] = {dx * dy, (1.0f - dx) * (1.0f - dy), dx * (1.0f - dy), (1.0f - dx) * dy};
            unsigned long long* acc = a.acc ? a.acc + n * img * C : nullptr;
            auto one = [&](int c, float gc, float iff, float icc, float ifc, float icf) {
                gx += gc * (dy * (icf - iff) + (1.0f - dy) * (icc - ifc));
                gy += gc * (dx * (ifc - iff) + (1.0f - dx) * (icc - icf));
                if (acc) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (ok[q]) atomicAdd(acc + c * img + pix[q], (unsigned long long)__double2ll_rn((double)gc * (double)w[q] * scale));
                }
            };
            const bool need_taps = a.dwarp != nullptr;
            if (V4) {
                for (int c = 0; c < C; c += 4) {
                    const float4 g4 = *reinterpret_cast<const float4*>(g + c);
                    float4 t[4] = {};
                    if (need_taps) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            t[q] = keep(ok[q], *reinterpret_cast<const float4*>(src + pix[q] * a.data_ld + c));
                        }
                    }
                    one(c, g4.x, t[0].x, t[1].x, t[2].x, t[3].x);
                    one(c + 1, g4.y, t[0].y, t[1].y, t[2].y, t[3].y);
                    one(c + 2, g4.z, t[0].z, t[1].z, t[2].z, t[3].z);
                    one(c + 3, g4.w, t[0].w, t[1].w, t[2].w, t[3].w);
                }
            } else {
                for (int c = 0; c < C; ++c) {
                    float t[4] = {0.f, 0.f, 0.f, 0.f};
                    if (need_taps) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float v = src[pix[q] * a.data_ld + c];
                            t[q] = ok[q] ? v : 0.f;
                        }
                    }
                    one(c, g[c], t[0], t[1], t[2], t[3]);
                }
            }
        }
        if (a.dwarp) {
            float* d = a.dwarp + p * a.dwarp_ld;
            if (a.w2) *reinterpret_cast<float2*>(d) = make_float2(gx, gy);
            else { d[0] = gx; d[1] = gy; }
        }
    }
}

// reads the planar accumulator in order, writes the NHWC output (pixel stride ddata_ld)
__global__ __launch_bounds__(RS_THREADS) void rs_final_kernel(const RsArgs a) {
    const double inv = ldexp(1.0, -block_shift(a.part, a.nparts, a.NP));
    const int64_t stride = (int64_t)gridDim.x * RS_THREADS, img = (int64_t)a.Hs * a.Ws;
    for (int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; i < a.nacc; i += stride) {
        const int64_t plane = i / img, pix = i - plane * img;           // plane = n*C + c
        const int64_t n = plane / a.C;
        const int c = (int)(plane - n * a.C);
        a.ddata[(n * img + pix) * a.ddata_ld + c] = (float)((double)(long long)a.acc[i] * inv);
    }
}

int grid_of(int64_t work) { return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(work, RS_THREADS), RS_MAX_GRID)); }

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

size_t acc_bytes(int64_t nacc) { return (size_t)cdiv64(nacc * 8, 256) * 256; }

// shared validation of fwd / bwd; 0 = fine
int check_common(const char* fn, int N, int P, int Hs, int Ws, int C, const void* data, int data_ld, const void* warp, int warp_ld,
                 const void* g, int g_ld) {
    if (N <= 0 || P <= 0 || Hs <= 0 || Ws <= 0 || C <= 0) return fail(MV3D_E_INVAL, "%s: bad shape", fn);
    if (data_ld < C || warp_ld < 2 || g_ld < C) return fail(MV3D_E_INVAL, "%s: pixel stride smaller than the channel count", fn);
    if (!data || !warp || !g) return fail(MV3D_E_INVAL, "%s: null pointer", fn);
    if (!aligned(data, 4) || !aligned(warp, 4) || !aligned(g, 4)) return fail(MV3D_E_INVAL, "%s: pointer not 4-byte aligned", fn);
    if (Hs > RS_MAX_SIDE || Ws > RS_MAX_SIDE) return fail(MV3D_E_UNSUPPORTED, "%s: image side above 2^24", fn);
    const int64_t NP = (int64_t)N * P, NI = (int64_t)N * Hs * Ws;
    if (NP > RS_MAX_ELEMS / 64 || NI > RS_MAX_ELEMS / 64 || NP * std::max(warp_ld, g_ld) > RS_MAX_ELEMS || NI * data_ld > RS_MAX_ELEMS ||
        NI * C > RS_MAX_ELEMS / 8)
        return fail(MV3D_E_UNSUPPORTED, "%s: an operand spans 2^40 elements or more", fn);
    return MV3D_OK;
}

const char* ch_tag(int C, bool v4) {
    static const char* t[5] = {"generic", "C1", "C2", "C3", "C4"};
    return C <= 4 ? t[C] : (v4 ? "vec4" : "generic");
}

}  // namespace
}  // namespace mv3d

using namespace mv3d;

extern "C" {

int mv3d_resampler_fwd(int N, int P, int Hs, int Ws, int C, const void* data, int data_ld, const void* warp, int warp_ld, void* out,
                       int out_ld, void* stream) {
    if (int rc = check_common("mv3d_resampler_fwd", N, P, Hs, Ws, C, data, data_ld, warp, warp_ld, out, out_ld)) return rc;
    RsArgs a = {};
    a.data = (const float*)data; a.warp = (const float*)warp; a.out = (float*)out;
    a.NP = (int64_t)N * P; a.P = P; a.Hs = Hs; a.Ws = Ws; a.C = C;
    a.data_ld = data_ld; a.warp_ld = warp_ld; a.g_ld = out_ld;
    a.w2 = warp_ld % 2 == 0 && aligned(warp, 8);
    const bool v4 = C > 4 && C % 4 == 0 && data_ld % 4 == 0 && out_ld % 4 == 0 && aligned(data, 16) && aligned(out, 16);
    // algorithmic bytes: warp + output per point, every source element once
    const OpInfo info{intern_label("resampler_fwd<%s>", ch_tag(C, v4)), 0.0,
                      (double)a.NP * (8.0 + 4.0 * C) + (double)N * Hs * Ws * 4.0 * C};
    const int grid = grid_of(v4 ? a.NP * (C / 4) : a.NP);
    return dispatch(stream, info, [=](hipStream_t s) {
        switch (v4 ? -1 : (C <= 4 ? C : 0)) {
            case -1: rs_fwd_vec4_kernel<<<grid, RS_THREADS, 0, s>>>(a); break;
            case 1: rs_fwd_kernel<1><<<grid, RS_THREADS, 0, s>>>(a); break;
            case 2: rs_fwd_kernel<2><<<grid, RS_THREADS, 0, s>>>(a); break;
            case 3: rs_fwd_kernel<3><<<grid, RS_THREADS, 0, s>>>(a); break;
            case 4: rs_fwd_kernel<4><<<grid, RS_THREADS, 0, s>>>(a); break;
            default: rs_fwd_kernel<0><<<grid, RS_THREADS, 0, s>>>(a); break;
        }
        return launched("rs_fwd_kernel");
    });
}

size_t mv3d_resampler_bwd_workspace_bytes(int N, int P, int Hs, int Ws, int C) {
    if (N <= 0 || P <= 0 || Hs <= 0 || Ws <= 0 || C <= 0) return 0;
    return acc_bytes((int64_t)N * Hs * Ws * C) + RS_PARTS * sizeof(float);
}

int mv3d_resampler_bwd(int N, int P, int Hs, int Ws, int C, const void* data, int data_ld, const void* warp, int warp_ld,
                       const void* dout, int dout_ld, void* dwarp, int dwarp_ld, void* ddata, int ddata_ld, void* workspace,
                       size_t workspace_bytes, void* stream) {
    const char* fn = "mv3d_resampler_bwd";
    if (int rc = check_common(fn, N, P, Hs, Ws, C, data, data_ld, warp, warp_ld, dout, dout_ld)) return rc;
    if (!dwarp && !ddata) return fail(MV3D_E_INVAL, "%s: neither dwarp nor ddata requested", fn);
    if (dwarp && (dwarp_ld < 2 || !aligned(dwarp, 4))) return fail(MV3D_E_INVAL, "%s: bad dwarp stride or alignment", fn);
    if (ddata && (ddata_ld < C || !aligned(ddata, 4))) return fail(MV3D_E_INVAL, "%s: bad ddata stride or alignment", fn);
    if (dwarp && (int64_t)N * P * dwarp_ld > RS_MAX_ELEMS) return fail(MV3D_E_UNSUPPORTED, "%s: dwarp spans 2^40 elements or more", fn);
    if (ddata && (int64_t)N * Hs * Ws * ddata_ld > RS_MAX_ELEMS) return fail(MV3D_E_UNSUPPORTED, "%s: ddata spans 2^40 elements or more", fn);
    RsArgs a = {};
    a.data = (const float*)data; a.warp = (const float*)warp; a.g = (const float*)dout;
    a.dwarp = (float*)dwarp; a.ddata = (float*)ddata;
    a.NP = (int64_t)N * P; a.P = P; a.nacc = (int64_t)N * Hs * Ws * C;
    a.Hs = Hs; a.Ws = Ws; a.C = C;
    a.data_ld = data_ld; a.warp_ld = warp_ld; a.g_ld = dout_ld; a.dwarp_ld = dwarp_ld; a.ddata_ld = ddata_ld;
    a.w2 = warp_ld % 2 == 0 && aligned(warp, 8) && (!dwarp || (dwarp_ld % 2 == 0 && aligned(dwarp, 8)));
    if (ddata) {
        const size_t need = mv3d_resampler_bwd_workspace_bytes(N, P, Hs, Ws, C);
        if (!workspace || workspace_bytes < need) return fail(MV3D_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
        if (!aligned(workspace, 16)) return fail(MV3D_E_INVAL, "%s: workspace not 16-byte aligned", fn);
        a.acc = (unsigned long long*)workspace;
        a.part = (float*)((char*)workspace + acc_bytes(a.nacc));
        a.nparts = (int)std::min<int64_t>(RS_PARTS, std::max<int64_t>(cdiv64(std::max(a.nacc / 2, a.NP * C), RS_THREADS), 1));
    }
    const bool v4 = C > 4 && C % 4 == 0 && data_ld % 4 == 0 && dout_ld % 4 == 0 && aligned(data, 16) && aligned(dout, 16);
    const char* what = dwarp && ddata ? "dwarp+ddata" : (dwarp ? "dwarp" : "ddata");
    const double np = (double)a.NP, acc8 = 8.0 * (double)a.nacc;
    int rc;
    if (ddata) {
        const RsArgs pa = a;
        const int grid = a.nparts;
        rc = dispatch(stream, OpInfo{intern_label("resampler_ddata_prep"), 0.0, np * 4.0 * C + acc8}, [=](hipStream_t s) {
            rs_prep_kernel<<<grid, RS_THREADS, 0, s>>>(pa);
            return launched("rs_prep_kernel");
        });
        if (rc) return rc;
    }
    {
        // algorithmic bytes: warp + dout per point, dwarp per point, source elements once (dwarp), accumulator read + written once (ddata)
        const double bytes = np * (8.0 + 4.0 * C) + (dwarp ? np * 8.0 + (double)N * Hs * Ws * 4.0 * C : 0.0) + (ddata ? 2.0 * acc8 : 0.0);
        const OpInfo info{intern_label("resampler_bwd<%s,%s>", ch_tag(C, v4), what), 0.0, bytes};
        const int grid = grid_of(a.NP);
        rc = dispatch(stream, info, [=](hipStream_t s) {
            switch (v4 ? -1 : (C <= 4 ? C : 0)) {
                case -1: rs_bwd_kernel<0, true><<<grid, RS_THREADS, 0, s>>>(a); break;
                case 1: rs_bwd_kernel<1, false><<<grid, RS_THREADS, 0, s>>>(a); break;
                case 2: rs_bwd_kernel<2, false><<<grid, RS_THREADS, 0, s>>>(a); break;
                case 3: rs_bwd_kernel<3, false><<<grid, RS_THREADS, 0, s>>>(a); break;
                case 4: rs_bwd_kernel<4, false><<<grid, RS_THREADS, 0, s>>>(a); break;
                default: rs_bwd_kernel<0, false><<<grid, RS_THREADS, 0, s>>>(a); break;
            }
            return launched("rs_bwd_kernel");
        });
        if (rc) return rc;
    }
    if (ddata) {
        const int grid = grid_of(a.nacc);
        rc = dispatch(stream, OpInfo{intern_label("resampler_ddata_final"), 0.0, acc8 + 4.0 * (double)a.nacc}, [=](hipStream_t s) {
            rs_final_kernel<<<grid, RS_THREADS, 0, s>>>(a);
            return launched("rs_final_kernel");
        });
    }
    return rc;
}

}  // extern "C"
