// The EMA update of one element and the chunked walk's geometry, shared by ema.hip (mv3d_ema_step) and weight_decay.hip (the
// EMA fused behind the decay).  Both units are built with -ffp-contract=off.
#pragma once
#include "common.h"

namespace mv3d {

// moving_averages.assign_moving_average(shadow, var, decay, zero_debias=False) on one element, in TF's order:
//   d = s - p;  u = d * w;  s = s - u      (w = 1 - decay, rounded once on the host).  s == p gives d = 0 and leaves s as it is.
__device__ __forceinline__ float ema_elem(float s, float p, float w) {
#pragma clang fp contract(off)
    const float d = s - p;
    const float u = d * w;
    return s - u;
}

__device__ __forceinline__ float4 ema4(float4 s, float4 p, float w) {
    return make_float4(ema_elem(s.x, p.x, w), ema_elem(s.y, p.y, w), ema_elem(s.z, p.z, w), ema_elem(s.w, p.w, w));
}

constexpr int EMA_UNROLL = 4;
constexpr int EMA_CHUNK = EMA_UNROLL * 256;      // float4s per workgroup per pass
constexpr int EMA_MAX_BLOCKS = 2048;

}  // namespace mv3d
