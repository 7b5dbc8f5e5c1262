// Decoupled weight decay behind the optimiser (p -= p * f over a table of flat index ranges), alone or with the EMA of the
// weights fused behind it.  Built with -ffp-contract=off: both forms are bit-exact against numpy (graph.weight_decay_rule).
#include "ema_common.h"
#include <algorithm>
#include <cmath>

namespace mv3d {

// t = p * f;  p = p - t, two roundings.  Where t == 0 (p is +-0, f is 0, or the product underflows to 0) the element keeps its
// bits: p - 0 is p anyway, and the one case that would differ, -0 - -0 = +0, keeps its sign.
__device__ __forceinline__ float decay_elem(float p, float f) {
#pragma clang fp contract(off)
    const float t = p * f;
    return t == 0.0f ? p : p - t;
}

__device__ __forceinline__ float4 decay4(float4 p, float f) {
    return make_float4(decay_elem(p.x, f), decay_elem(p.y, f), decay_elem(p.z, f), decay_elem(p.w, f));
}

// first index in [a, b) whose value is > x (UPPER) or >= x (!UPPER); b when there is none.  v is sorted ascending.
template <bool UPPER>
__device__ __forceinline__ int first_above(const int64_t* v, int a, int b, int64_t x) {
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (UPPER ? v[mid] > x : v[mid] >= x) b = mid; else a = mid + 1;
    }
    return a;
}

// ema_kernel's walk over [lo, hi) of the flat buffers: chunks of EMA_UNROLL x 256 float4s with a grid stride, every load of a
// chunk issued before the first use.  The table (sorted, disjoint, every bound a multiple of 4: a float4 lies wholly inside one
// range or outside all of them) is staged in LDS once per workgroup, 16 KiB at the cap.  Per chunk ONE lookup, the same in every
// lane, finds the ranges [r0, r1) that meet the chunk; a float4 then searches those alone -- nothing when there is none, one
// comparison when there is one, which is every chunk but the handful at a variable's border in the model's table.
//   !FUSED: a chunk that meets no range is skipped without a load; elements outside the ranges are neither read nor written.
//   FUSED:  s = ema(s, p_new) for every element of [lo, hi), p_new the decayed value inside the ranges and p outside them.
template <bool FUSED>
__global__ __launch_bounds__(256) void weight_decay_kernel(float* __restrict__ p, float* __restrict__ s, int64_t lo, int64_t hi,
                                                          const int64_t* __restrict__ ranges, int nranges, float f, float w) {
    __shared__ int64_t rb[MV3D_DECAY_MAX_RANGES], re[MV3D_DECAY_MAX_RANGES];
    for (int i = threadIdx.x; i < nranges; i += 256) { rb[i] = ranges[2 * i]; re[i] = ranges[2 * i + 1]; }
    __syncthreads();
    const int64_t nvec = (hi - lo) >> 2;
    const int64_t nchunk = (nvec + EMA_CHUNK - 1) / EMA_CHUNK;
    float4* p4 = reinterpret_cast<float4*>(p + lo);
    float4* s4 = FUSED ? reinterpret_cast<float4*>(s + lo) : nullptr;
    for (int64_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
        const int64_t cb = lo + c * (4 * EMA_CHUNK);                                    // the chunk's elements, absolute
        const int64_t ce = std::min<int64_t>(cb + 4 * EMA_CHUNK, lo + (nvec << 2));
        const int r0 = first_above<true>(re, 0, nranges, cb);                           // first range that ends behind the chunk's start
        const int r1 = first_above<false>(rb, r0, nranges, ce);                         // first range that begins at or behind its end
        if (!FUSED && r0 == r1) continue;
        const int64_t base = c * EMA_CHUNK + threadIdx.x;
        bool live[EMA_UNROLL], in[EMA_UNROLL];
        float4 pv[EMA_UNROLL], sv[EMA_UNROLL];
#pragma unroll
        for (int k = 0; k < EMA_UNROLL; ++k) {
            const int64_t i = base + k * 256;
            live[k] = i < nvec;
            const int64_t e = lo + (i << 2);
            const int r = first_above<true>(re, r0, r1, e);
            in[k] = live[k] && r < r1 && rb[r] <= e;
            pv[k] = sv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < EMA_UNROLL; ++k)
            if (FUSED ? live[k] : in[k]) pv[k] = p4[base + k * 256];
        if (FUSED) {
#pragma unroll
            for (int k = 0; k < EMA_UNROLL; ++k)
                if (live[k]) sv[k] = s4[base + k * 256];
        }
#pragma unroll
        for (int k = 0; k < EMA_UNROLL; ++k) {
            if (in[k]) { pv[k] = decay4(pv[k], f); p4[base + k * 256] = pv[k]; }
            if (FUSED && live[k]) s4[base + k * 256] = ema4(sv[k], pv[k], w);
        }
    }
    // hi is the unaligned end of the buffer: its last (hi - lo) & 3 floats, one lane each
    if (blockIdx.x == 0 && threadIdx.x < ((hi - lo) & 3)) {
        const int64_t e = lo + (nvec << 2);
        const int64_t i = e + threadIdx.x;
        const int r = first_above<true>(re, 0, nranges, e);
        const bool in = r < nranges && rb[r] <= e;
        float pv = 0.0f;
        if (FUSED || in) pv = p[i];                 // the pure form reads nothing outside the ranges
        if (in) { pv = decay_elem(pv, f); p[i] = pv; }
        if (FUSED) s[i] = ema_elem(s[i], pv, w);
    }
}

}  // namespace mv3d

using namespace mv3d;

extern "C" {

int mv3d_weight_decay_step(void* params, void* shadow, int64_t lo, int64_t hi, const void* ranges, int nranges, float f,
                           float one_minus_decay, void* stream) {
    if (!params || lo < 0 || hi <= lo) return fail(MV3D_E_INVAL, "mv3d_weight_decay_step: bad arguments");
    if (((uintptr_t)params | (uintptr_t)shadow) & 15) return fail(MV3D_E_INVAL, "mv3d_weight_decay_step: buffers must be 16-byte aligned");
    if (lo & 3) return fail(MV3D_E_INVAL, "mv3d_weight_decay_step: lo must be a multiple of 4");
    if ((hi & 3) && !shadow)
        return fail(MV3D_E_INVAL, "mv3d_weight_decay_step: hi must be a multiple of 4 (the unaligned end of the buffers: the fused form only)");
    if (nranges < 0 || nranges > MV3D_DECAY_MAX_RANGES)
        return fail(MV3D_E_INVAL, "mv3d_weight_decay_step: nranges must be in 0..%d", MV3D_DECAY_MAX_RANGES);
    if ((nranges && !ranges) || ((uintptr_t)ranges & 7)) return fail(MV3D_E_INVAL, "mv3d_weight_decay_step: the range table is NULL or misaligned");
    if (!(f >= 0.0f && f < 1.0f)) return fail(MV3D_E_INVAL, "mv3d_weight_decay_step: f must be in [0, 1)");      // also refuses NaN
    if (shadow && !(one_minus_decay >= 0.0f && one_minus_decay <= 1.0f))
        return fail(MV3D_E_INVAL, "mv3d_weight_decay_step: one_minus_decay must be in [0, 1]");
    const int64_t count = hi - lo;
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(count >> 2, EMA_CHUNK), EMA_MAX_BLOCKS));
    const int64_t* tb = (const int64_t*)ranges;
    // algorithmic bytes: the table lives on the device, so the host knows only the bound (every element of [lo, hi) decays)
    if (shadow)
        return dispatch(stream, OpInfo{"weight_decay_ema", 0.0, 16.0 * count}, [=](hipStream_t s) {
            weight_decay_kernel<true><<<blocks, 256, 0, s>>>((float*)params, (float*)shadow, lo, hi, tb, nranges, f, one_minus_decay);
            return launched("weight_decay_kernel<fused>");
        });
    return dispatch(stream, OpInfo{"weight_decay", 0.0, 8.0 * count}, [=](hipStream_t s) {
        weight_decay_kernel<false><<<blocks, 256, 0, s>>>((float*)params, nullptr, lo, hi, tb, nranges, f, 0.0f);
        return launched("weight_decay_kernel");
    });
}

}  // extern "C"
