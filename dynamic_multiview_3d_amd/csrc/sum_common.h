// The fixed-order double sums of a workgroup of 256 threads (four waves), shared by the image units (through image_common.h) and
// by the gradient-norm and gradient-accumulation units (grad_norm.hip, grad_accum.hip).  The order is a contract, stated once here: a wave adds its lanes as an xor butterfly
// (offsets 32, 16 .. 1), the workgroup adds the four wave sums as ((w0 + w1) + w2) + w3 -- the same bits on every run and on every
// grid, and what the numpy twins restate.
#pragma once
#include "common.h"

namespace mv3d {

constexpr int SUM_THREADS = 256;                   // four waves: what block_sum and block_total are written for

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// K sums over the workgroup's 256 threads: the wave sums land in s_red[q * 4 + wave] (K * 4 doubles), then a barrier; any thread
// may then read block_total(s_red, q).
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* s_red, int tid) {
#pragma unroll
    for (int q = 0; q < K; ++q) {
        const double s = wave_sum(v[q]);
        if ((tid & 63) == 0) s_red[q * 4 + (tid >> 6)] = s;
    }
    __syncthreads();
}
__device__ __forceinline__ double block_total(const double* s_red, int q) {
    return ((s_red[q * 4] + s_red[q * 4 + 1]) + s_red[q * 4 + 2]) + s_red[q * 4 + 3];
}

// The chunking of the flat-gradient sums of squares (grad_sumsq_kernel of grad_norm.hip and the FINISH mode of grad_accum.hip write
// the same partials; include/mv3d_hip.h states the order): one double per chunk of GN_CHUNK floats, thread t of the workgroup owns
// float4s t + 256 k, k = 0 .. GN_UNROLL - 1, of the chunk.
constexpr int GN_UNROLL = 16;                        // float4s a lane owns per chunk
constexpr int GN_CHUNK4 = GN_UNROLL * SUM_THREADS;   // float4s per chunk
constexpr int GN_CHUNK = 4 * GN_CHUNK4;              // floats per chunk (16384): fixed, whatever the device and the grid
// The grid: one workgroup per chunk up to 8 per CU (256 CUs), beyond that the workgroups walk the chunks with a grid stride.  The
// chunk sums do not depend on it.
constexpr int GN_MAX_BLOCKS = 2048;

__device__ __forceinline__ double sq(float x) {
    const double d = (double)x;
    return d * d;                                    // exact: 24 x 24 bits
}

static inline int64_t gn_chunks(int64_t count) { return cdiv64(count, GN_CHUNK); }

}  // namespace mv3d
