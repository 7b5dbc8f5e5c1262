// Exponential moving average of the weights (tf.train.ExponentialMovingAverage, TF 1.3) and the in-place exchange that puts
// the averaged weights where the forward pass reads them.  Built with -ffp-contract=off: the update is bit-exact against numpy.
#include "ema_common.h"
#include <algorithm>
#include <cmath>

namespace mv3d {

// (ema_elem, ema4 and the chunk geometry: ema_common.h, shared with weight_decay.hip)
// A pure HBM stream, 12 B/param (loads s, p; stores s), no LDS.  A workgroup takes chunks of EMA_UNROLL x 256 float4s; every
// lane issues its EMA_UNROLL 16-byte loads of BOTH buffers before the first use, so a workgroup has 2 x 4 x 4 KiB = 32 KiB of
// loads in flight and a CU with several resident workgroups a multiple of that.  The grid is 8 workgroups per CU (256 CUs),
// each walking the chunks with a grid stride; the last, partial chunk is bounds-checked, the count & 3 tail is scalar.

__global__ __launch_bounds__(256) void ema_kernel(int64_t count, float* __restrict__ s, const float* __restrict__ p, float w) {
    const int64_t nvec = count >> 2;
    const int64_t nchunk = (nvec + EMA_CHUNK - 1) / EMA_CHUNK;
    float4* s4 = reinterpret_cast<float4*>(s);
    const float4* p4 = reinterpret_cast<const float4*>(p);
    for (int64_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
        const int64_t base = c * EMA_CHUNK + threadIdx.x;
        float4 sv[EMA_UNROLL], pv[EMA_UNROLL];
        if (base - threadIdx.x + EMA_CHUNK <= nvec) {
#pragma unroll
            for (int k = 0; k < EMA_UNROLL; ++k) sv[k] = s4[base + k * 256];
#pragma unroll
            for (int k = 0; k < EMA_UNROLL; ++k) pv[k] = p4[base + k * 256];
#pragma unroll
            for (int k = 0; k < EMA_UNROLL; ++k) s4[base + k * 256] = ema4(sv[k], pv[k], w);
        } else {
#pragma unroll
            for (int k = 0; k < EMA_UNROLL; ++k) {
                const int64_t i = base + k * 256;
                if (i < nvec) s4[i] = ema4(s4[i], p4[i], w);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (count & 3)) {
        const int64_t i = (nvec << 2) + threadIdx.x;
        s[i] = ema_elem(s[i], p[i], w);
    }
}

// a <-> b, bit for bit (integer lanes: no float operation ever sees the values); same walk as ema_kernel, 16 B/element of traffic
__global__ __launch_bounds__(256) void swap_kernel(int64_t count, uint32_t* __restrict__ a, uint32_t* __restrict__ b) {
    const int64_t nvec = count >> 2;
    const int64_t nchunk = (nvec + EMA_CHUNK - 1) / EMA_CHUNK;
    uint4* a4 = reinterpret_cast<uint4*>(a);
    uint4* b4 = reinterpret_cast<uint4*>(b);
    for (int64_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
        const int64_t base = c * EMA_CHUNK + threadIdx.x;
        if (base - threadIdx.x + EMA_CHUNK <= nvec) {
            uint4 av[EMA_UNROLL], bv[EMA_UNROLL];
#pragma unroll
            for (int k = 0; k < EMA_UNROLL; ++k) av[k] = a4[base + k * 256];
#pragma unroll
            for (int k = 0; k < EMA_UNROLL; ++k) bv[k] = b4[base + k * 256];
#pragma unroll
            for (int k = 0; k < EMA_UNROLL; ++k) { a4[base + k * 256] = bv[k]; b4[base + k * 256] = av[k]; }
        } else {
#pragma unroll
            for (int k = 0; k < EMA_UNROLL; ++k) {
                const int64_t i = base + k * 256;
                if (i < nvec) { const uint4 av = a4[i], bv = b4[i]; a4[i] = bv; b4[i] = av; }
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (count & 3)) {
        const int64_t i = (nvec << 2) + threadIdx.x;
        const uint32_t av = a[i], bv = b[i];
        a[i] = bv; b[i] = av;
    }
}

static inline int ema_blocks(int64_t count) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(count >> 2, EMA_CHUNK), EMA_MAX_BLOCKS));
}

}  // namespace mv3d

using namespace mv3d;

extern "C" {

int mv3d_ema_step(int64_t count, void* shadow, const void* params, float one_minus_decay, void* stream) {
    if (count < 1 || !shadow || !params) return fail(MV3D_E_INVAL, "mv3d_ema_step: bad arguments");
    if (((uintptr_t)shadow | (uintptr_t)params) & 15) return fail(MV3D_E_INVAL, "mv3d_ema_step: buffers must be 16-byte aligned");
    if (!(one_minus_decay >= 0.0f && one_minus_decay <= 1.0f))      // also refuses NaN
        return fail(MV3D_E_INVAL, "mv3d_ema_step: one_minus_decay must be in [0, 1]");
    const int blocks = ema_blocks(count);
    return dispatch(stream, OpInfo{"ema", 0.0, 12.0 * count}, [=](hipStream_t s) {
        ema_kernel<<<blocks, 256, 0, s>>>(count, (float*)shadow, (const float*)params, one_minus_decay);
        return launched("ema_kernel");
    });
}

int mv3d_swap_f32(int64_t count, void* a, void* b, void* stream) {
    if (count < 1 || !a || !b) return fail(MV3D_E_INVAL, "mv3d_swap_f32: bad arguments");
    if (((uintptr_t)a | (uintptr_t)b) & 15) return fail(MV3D_E_INVAL, "mv3d_swap_f32: buffers must be 16-byte aligned");
    const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b;
    const uint64_t bytes = 4 * (uint64_t)count;
    if (ua == ub || (ua < ub ? ub - ua < bytes : ua - ub < bytes)) return fail(MV3D_E_INVAL, "mv3d_swap_f32: the buffers overlap");
    const int blocks = ema_blocks(count);
    return dispatch(stream, OpInfo{"swap_f32", 0.0, 16.0 * count}, [=](hipStream_t s) {
        swap_kernel<<<blocks, 256, 0, s>>>(count, (uint32_t*)a, (uint32_t*)b);
        return launched("swap_kernel");
    });
}

}  // extern "C"
