// Global-norm gradient clipping over one flat gradient buffer: the norm in two launches (chunk sums, then one workgroup), and the
// scale written into the gradient-scale slot of the optimiser records, so the optimiser launch behind it applies the clip and no
// gradient is rewritten.  include/mv3d_hip.h states the order contract; graph.grad_clip_rule is its numpy twin.  Built with
// -ffp-contract=off: the fp32 end of the final kernel is bit-exact against numpy.
#include "sum_common.h"
#include <algorithm>
#include <cmath>

namespace mv3d {

// GN_UNROLL (float4s a lane loads per chunk, all issued before the first use), GN_CHUNK, GN_MAX_BLOCKS and sq(): sum_common.h, which
// grad_accum.hip shares.

// Pass 1, a pure 4 B/element read stream, no LDS traffic but the four wave sums.  A lane has GN_UNROLL 16-byte loads (256 B) in
// flight, a workgroup 64 KiB.  part[c] = the chunk's sum of squares, in the header's order.
__global__ __launch_bounds__(SUM_THREADS) void grad_sumsq_kernel(int64_t count, const float* __restrict__ g, double* __restrict__ part) {
    __shared__ double s_red[4];
    const int64_t nvec = count >> 2;
    const int tail = (int)(count & 3);
    const int64_t nchunk = (count + GN_CHUNK - 1) / GN_CHUNK;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    for (int64_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
        const int64_t base = c * GN_CHUNK4 + threadIdx.x;
        float4 v[GN_UNROLL];
        if ((c + 1) * GN_CHUNK4 <= nvec) {
#pragma unroll
            for (int k = 0; k < GN_UNROLL; ++k) v[k] = g4[base + k * SUM_THREADS];
        } else {
#pragma unroll
            for (int k = 0; k < GN_UNROLL; ++k) {
                const int64_t i = base + k * SUM_THREADS;
                v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (i < nvec) {
                    v[k] = g4[i];
                } else if (i == nvec && tail) {      // the count & 3 floats behind the last whole float4
                    const float* t = g + (nvec << 2);
                    v[k].x = t[0];
                    if (tail > 1) v[k].y = t[1];
                    if (tail > 2) v[k].z = t[2];
                }
            }
        }
        double acc[1] = {0.0};
#pragma unroll
        for (int k = 0; k < GN_UNROLL; ++k) {
            acc[0] += sq(v[k].x);
            acc[0] += sq(v[k].y);
            acc[0] += sq(v[k].z);
            acc[0] += sq(v[k].w);
        }
        block_sum(acc, s_red, threadIdx.x);
        if (threadIdx.x == 0) part[c] = block_total(s_red, 0);
        __syncthreads();                             // s_red is written again by the next chunk
    }
}

// Pass 2, one workgroup: S = the chunk sums in the header's order; thread 0 turns S into the norm, the scale and the records' slot.
__global__ __launch_bounds__(SUM_THREADS) void grad_clip_final_kernel(int64_t nchunk, const double* __restrict__ part, float pre_scale,
                                                                      float clip_norm, float* __restrict__ out, float* state_a,
                                                                      float* state_b) {
#pragma clang fp contract(off)
    __shared__ double s_red[4];
    double acc[1] = {0.0};
    for (int64_t t = threadIdx.x; t < nchunk; t += SUM_THREADS) acc[0] += part[t];
    block_sum(acc, s_red, threadIdx.x);
    if (threadIdx.x == 0) {
        const double S = block_total(s_red, 0);
        const float n = (float)__dsqrt_rn(S) * pre_scale;
        const float s = (n > clip_norm) ? clip_norm / n : 1.0f;      // NaN compares false: scale 1; n = inf: scale 0
        out[0] = n;
        out[1] = s;
        const float gscale = pre_scale * s;
        if (state_a) state_a[MV3D_ADAM_GSCALE] = gscale;
        if (state_b) state_b[MV3D_ADAM_GSCALE] = gscale;
    }
}

}  // namespace mv3d

using namespace mv3d;

static_assert(MV3D_ADAM_GSCALE == MV3D_SGD_GSCALE, "one gradient-scale slot for every optimiser record");

extern "C" {

size_t mv3d_grad_clip_workspace_bytes(int64_t count) {
    if (count < 1) return 0;
    return (size_t)cdiv64(gn_chunks(count) * (int64_t)sizeof(double), 256) * 256;
}

// The checks mv3d_grad_clip_scale and mv3d_grad_clip_finish share (everything but g).
static int clip_args(const char* fn, int64_t count, float pre_scale, float clip_norm, const void* out, const void* state_a,
                     const void* state_b, const void* workspace, size_t workspace_bytes) {
    if (count < 1) return fail(MV3D_E_INVAL, "%s: count (%lld) must be at least 1", fn, (long long)count);
    if (!out || !workspace) return fail(MV3D_E_INVAL, "%s: out or workspace is null", fn);
    if (((uintptr_t)out | (uintptr_t)state_a | (uintptr_t)state_b) & 3)
        return fail(MV3D_E_INVAL, "%s: out, state_a or state_b not 4-byte aligned", fn);
    if (!std::isfinite(pre_scale) || !(pre_scale > 0.f))
        return fail(MV3D_E_INVAL, "%s: pre_scale (%g) must be finite and positive", fn, (double)pre_scale);
    if (!(clip_norm > 0.f))                          // also refuses NaN; +inf = measure only
        return fail(MV3D_E_INVAL, "%s: clip_norm (%g) must be positive (+inf: measure only)", fn, (double)clip_norm);
    const size_t need = mv3d_grad_clip_workspace_bytes(count);
    if (workspace_bytes < need) return fail(MV3D_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    if ((uintptr_t)workspace & 15) return fail(MV3D_E_WORKSPACE, "%s: workspace not 16-byte aligned", fn);
    return MV3D_OK;
}

static int clip_final(int64_t count, float pre_scale, float clip_norm, void* out, void* state_a, void* state_b, const void* workspace,
                      void* stream) {
    const int64_t nchunk = gn_chunks(count);
    const double* part = (const double*)workspace;
    return dispatch(stream, OpInfo{"grad_clip_final_kernel", 0.0, 8.0 * nchunk}, [=](hipStream_t s) {
        grad_clip_final_kernel<<<1, SUM_THREADS, 0, s>>>(nchunk, part, pre_scale, clip_norm, (float*)out, (float*)state_a, (float*)state_b);
        return launched("grad_clip_final_kernel");
    });
}

int mv3d_grad_clip_scale(int64_t count, const void* g, float pre_scale, float clip_norm, void* out, void* state_a, void* state_b,
                         void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mv3d_grad_clip_scale";
    if (count >= 1 && !g) return fail(MV3D_E_INVAL, "%s: g is null", fn);
    if (count >= 1 && ((uintptr_t)g & 15)) return fail(MV3D_E_INVAL, "%s: g must be 16-byte aligned", fn);
    int rc = clip_args(fn, count, pre_scale, clip_norm, out, state_a, state_b, workspace, workspace_bytes);
    if (rc != MV3D_OK) return rc;
    const int64_t nchunk = gn_chunks(count);
    const int blocks = (int)std::min<int64_t>(nchunk, GN_MAX_BLOCKS);
    double* part = (double*)workspace;
    rc = dispatch(stream, OpInfo{"grad_sumsq_kernel", 2.0 * count, 4.0 * count}, [=](hipStream_t s) {
        grad_sumsq_kernel<<<blocks, SUM_THREADS, 0, s>>>(count, (const float*)g, part);
        return launched("grad_sumsq_kernel");
    });
    if (rc != MV3D_OK) return rc;
    return clip_final(count, pre_scale, clip_norm, out, state_a, state_b, workspace, stream);
}

int mv3d_grad_clip_finish(int64_t count, float pre_scale, float clip_norm, void* out, void* state_a, void* state_b,
                          const void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = clip_args("mv3d_grad_clip_finish", count, pre_scale, clip_norm, out, state_a, state_b, workspace, workspace_bytes);
    if (rc != MV3D_OK) return rc;
    return clip_final(count, pre_scale, clip_norm, out, state_a, state_b, workspace, stream);
}

}  // extern "C"
