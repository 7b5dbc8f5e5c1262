// Gradient accumulation over one flat gradient buffer: N micro-batches' gradients summed into a second flat buffer, the last
// sum written back into the gradient buffer itself, so the norm and every optimiser kernel behind it read what they always read.
// The last launch can write the chunk sums of squares of what it stored, in grad_sumsq_kernel's order (grad_norm.hip), which
// saves the norm its read pass.  include/mv3d_hip.h states the modes and the order contract; graph.grad_accum_rule is the numpy
// twin.  Built with -ffp-contract=off like its neighbours (the unit holds additions only; the loss scale is one product).
#include "sum_common.h"
#include <algorithm>

namespace mv3d {

// float4s of EACH buffer a lane loads before its first use: a chunk (GN_UNROLL float4s per lane) is walked in GN_UNROLL / GA_SUB
// rounds.  ADD and FINISH have 2 x GA_SUB 16-byte loads (256 B) in flight per lane, a workgroup 64 KiB -- what grad_sumsq_kernel
// has for its one buffer -- of which 64 VGPRs hold the loaded data.  Whole kernels (hipcc -O3, gfx950, no scratch): STORE 60 VGPRs
// (7 waves per SIMD), ADD and FINISH 78 (6), FINISH with partials 90 (5): five to seven workgroups stay resident per CU.
constexpr int GA_SUB = 8;
static_assert(GN_UNROLL % GA_SUB == 0, "a chunk is a whole number of rounds");

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// A pure HBM stream, no LDS traffic but the four wave sums of PART.  dst[i] = src[i] (ADD false: MV3D_ACCUM_STORE, dst = sum, src = g,
// 8 B/element, dst is not read) or dst[i] = dst[i] + src[i] (12 B/element; MV3D_ACCUM_ADD: dst = sum, src = g; MV3D_ACCUM_FINISH:
// dst = g, src = sum -- an fp32 addition gives the same number either way round).  src is only read.  One writer per element, no
// atomics: the same bits on every run and every grid.  PART (FINISH only): part[c] = the sum of squares of the values chunk c
// stored, in the header's order -- thread t adds its float4s t + 256 k to one double in the order k = 0 .. 15, x, y, z, w, whatever
// the round they were loaded in.  The last, partial chunk is bounds-checked; the count & 3 floats behind the last whole float4 are
// scalar and belong to the lane that owns that float4.  Thread 0 of workgroup 0 carries the loss scalar along (`mode` is its alone).
template <bool ADD, bool PART>
__global__ __launch_bounds__(SUM_THREADS) void grad_accum_kernel(int64_t count, float* __restrict__ dst, const float* __restrict__ src,
                                                                 int mode, const float* loss, float* loss_sum, float loss_scale,
                                                                 double* __restrict__ part) {
    __shared__ double s_red[4];
    const int64_t nvec = count >> 2;
    const int tail = (int)(count & 3);
    const int64_t nchunk = (count + GN_CHUNK - 1) / GN_CHUNK;
    float4* d4 = reinterpret_cast<float4*>(dst);
    const float4* s4 = reinterpret_cast<const float4*>(src);
    for (int64_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
        const int64_t base = c * GN_CHUNK4 + threadIdx.x;
        const bool whole = (c + 1) * GN_CHUNK4 <= nvec;
        double acc[1] = {0.0};
#pragma unroll
        for (int h = 0; h < GN_UNROLL; h += GA_SUB) {
            if (whole) {
                float4 dv[GA_SUB], sv[GA_SUB];
                if (ADD) {
#pragma unroll
                    for (int k = 0; k < GA_SUB; ++k) dv[k] = d4[base + (h + k) * SUM_THREADS];
                }
#pragma unroll
                for (int k = 0; k < GA_SUB; ++k) sv[k] = s4[base + (h + k) * SUM_THREADS];
#pragma unroll
                for (int k = 0; k < GA_SUB; ++k) {
                    const float4 r = ADD ? add4(dv[k], sv[k]) : sv[k];
                    d4[base + (h + k) * SUM_THREADS] = r;
                    if (PART) {
                        acc[0] += sq(r.x);
                        acc[0] += sq(r.y);
                        acc[0] += sq(r.z);
                        acc[0] += sq(r.w);
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < GA_SUB; ++k) {
                    const int64_t i = base + (h + k) * SUM_THREADS;
                    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);      // elements at or past count: 0 in the sum of squares
                    if (i < nvec) {
                        r = ADD ? add4(d4[i], s4[i]) : s4[i];
                        d4[i] = r;
                    } else if (i == nvec && tail) {
                        float* dt = dst + (nvec << 2);
                        const float* st = src + (nvec << 2);
                        r.x = ADD ? dt[0] + st[0] : st[0];
                        dt[0] = r.x;
                        if (tail > 1) { r.y = ADD ? dt[1] + st[1] : st[1]; dt[1] = r.y; }
                        if (tail > 2) { r.z = ADD ? dt[2] + st[2] : st[2]; dt[2] = r.z; }
                    }
                    if (PART) {
                        acc[0] += sq(r.x);
                        acc[0] += sq(r.y);
                        acc[0] += sq(r.z);
                        acc[0] += sq(r.w);
                    }
                }
            }
        }
        if (PART) {
            block_sum(acc, s_red, threadIdx.x);
            if (threadIdx.x == 0) part[c] = block_total(s_red, 0);
            __syncthreads();                         // s_red is written again by the next chunk
        }
    }
    if (loss && blockIdx.x == 0 && threadIdx.x == 0) {
#pragma clang fp contract(off)
        const float l = loss[0];
        if (mode == MV3D_ACCUM_STORE) loss_sum[0] = l;
        else if (mode == MV3D_ACCUM_ADD) loss_sum[0] = loss_sum[0] + l;
        else loss_sum[0] = (loss_sum[0] + l) * loss_scale;
    }
}

}  // namespace mv3d

using namespace mv3d;

extern "C" {

int mv3d_grad_accumulate(int64_t count, void* sum, void* g, int mode, const void* loss, void* loss_sum, float loss_scale,
                         void* sumsq_part, size_t sumsq_bytes, void* stream) {
    const char* fn = "mv3d_grad_accumulate";
    if (count < 1) return fail(MV3D_E_INVAL, "%s: count (%lld) must be at least 1", fn, (long long)count);
    if (!sum || !g) return fail(MV3D_E_INVAL, "%s: sum or g is null", fn);
    if (((uintptr_t)sum | (uintptr_t)g) & 15) return fail(MV3D_E_INVAL, "%s: sum and g must be 16-byte aligned", fn);
    const uintptr_t us = (uintptr_t)sum, ug = (uintptr_t)g;
    const uint64_t bytes = 4 * (uint64_t)count;
    if (us == ug || (us < ug ? ug - us < bytes : us - ug < bytes)) return fail(MV3D_E_INVAL, "%s: sum and g overlap", fn);
    if (mode != MV3D_ACCUM_STORE && mode != MV3D_ACCUM_ADD && mode != MV3D_ACCUM_FINISH)
        return fail(MV3D_E_INVAL, "%s: unknown mode %d", fn, mode);
    if ((loss == nullptr) != (loss_sum == nullptr)) return fail(MV3D_E_INVAL, "%s: loss and loss_sum go together (both or neither)", fn);
    if (((uintptr_t)loss | (uintptr_t)loss_sum) & 3) return fail(MV3D_E_INVAL, "%s: loss or loss_sum not 4-byte aligned", fn);
    if (sumsq_part && mode != MV3D_ACCUM_FINISH) return fail(MV3D_E_INVAL, "%s: sumsq_part is written by MV3D_ACCUM_FINISH only", fn);
    if (sumsq_part) {
        const size_t need = mv3d_grad_clip_workspace_bytes(count);
        if (sumsq_bytes < need) return fail(MV3D_E_WORKSPACE, "%s: sumsq_part of %zu bytes, %zu needed", fn, sumsq_bytes, need);
        if ((uintptr_t)sumsq_part & 15) return fail(MV3D_E_WORKSPACE, "%s: sumsq_part not 16-byte aligned", fn);
    }
    // The grid: one workgroup per chunk up to GN_MAX_BLOCKS; beyond that every workgroup walks the same number of chunks (the last
    // one may be short) with a grid stride, so that no workgroup is left streaming alone behind the others (with min(chunks,
    // GN_MAX_BLOCKS) 148 of the 2048 workgroups would walk a third chunk at 69.5 M floats).  DESIGN.md has what was measured of
    // the grid: no gain beyond the spread from process to process.  The results do not depend on the grid.
    const int64_t rounds = cdiv64(gn_chunks(count), GN_MAX_BLOCKS);
    const int blocks = (int)cdiv64(gn_chunks(count), rounds);
    float* s_ = (float*)sum;
    float* g_ = (float*)g;
    const float* l_ = (const float*)loss;
    float* ls_ = (float*)loss_sum;
    double* part = (double*)sumsq_part;
    if (mode == MV3D_ACCUM_STORE)
        return dispatch(stream, OpInfo{"grad_accum_store_kernel", 0.0, 8.0 * count}, [=](hipStream_t s) {
            grad_accum_kernel<false, false><<<blocks, SUM_THREADS, 0, s>>>(count, s_, g_, mode, l_, ls_, loss_scale, nullptr);
            return launched("grad_accum_store_kernel");
        });
    if (mode == MV3D_ACCUM_ADD)
        return dispatch(stream, OpInfo{"grad_accum_add_kernel", 1.0 * count, 12.0 * count}, [=](hipStream_t s) {
            grad_accum_kernel<true, false><<<blocks, SUM_THREADS, 0, s>>>(count, s_, g_, mode, l_, ls_, loss_scale, nullptr);
            return launched("grad_accum_add_kernel");
        });
    if (!part)
        return dispatch(stream, OpInfo{"grad_accum_finish_kernel", 1.0 * count, 12.0 * count}, [=](hipStream_t s) {
            grad_accum_kernel<true, false><<<blocks, SUM_THREADS, 0, s>>>(count, g_, s_, mode, l_, ls_, loss_scale, nullptr);
            return launched("grad_accum_finish_kernel");
        });
    return dispatch(stream, OpInfo{"grad_accum_finish_sumsq_kernel", 3.0 * count, 12.0 * count}, [=](hipStream_t s) {
        grad_accum_kernel<true, true><<<blocks, SUM_THREADS, 0, s>>>(count, g_, s_, mode, l_, ls_, loss_scale, part);
        return launched("grad_accum_finish_sumsq_kernel");
    });
}

}  // extern "C"
