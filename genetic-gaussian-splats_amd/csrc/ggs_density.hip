// Density control of the Adam refiner: the fixed-N form, relocation.
// Every `every` steps a candidate's dead splats (alpha below alpha_dead) are re-used
// as clones or split halves of its live splats with the largest accumulated
// positional gradient.  ggs/refine.py density_accumulate / relocate state all of it
// in numpy; the kernels are held to them bit for bit.
//   density_acc_kernel    one thread per (candidate, splat): acc += |d fit / d (x, y)|
//                         per pixel
//   density_rank_kernel   one thread per (candidate, splat): classifies its splat
//                         (dead / source / neither), ranks it among its class by
//                         counting smaller 64-bit keys, tiled through LDS, and writes
//                         the first max_moves of either list
//   density_apply_kernel  one thread per (candidate, pair): clone or split, the two
//                         rows' moments zeroed, the pair logged
// Float32, one rounding per operation (-ffp-contract=off), division and sqrt
// correctly rounded, exp / sin / cos those of ggs_detmath.h.  The only atomics are
// integer counters; every index is bounded by N or max_moves before it is used.
#include <hip/hip_runtime.h>

#include "ggs_detmath.h"
#include "ggs_internal.h"

namespace ggs {
namespace {

using namespace detmath;

constexpr int DT = 256;            // threads per workgroup; the rank kernel's tile

// order-preserving 32-bit key of a float (NaN excluded by the callers): -0.0 is +0.0
__device__ __forceinline__ uint32_t float_key(float f) {
    const uint32_t u = __builtin_bit_cast(uint32_t, f + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The splat's 64-bit key: class (0 neither, 1 dead, 2 source) in the top two bits,
// the float key in the next 32, the index (below 2^25: check_dims) in the low 30.
// Within a class the keys are unique and ascend as the class's list does: dead by
// (alpha, index), sources by (-acc, index).  Neither: 0.
__device__ __forceinline__ uint64_t classify(const float* __restrict__ x, const float* __restrict__ acc, int64_t row0,
                                             int s, float n_acc, float alpha_dead, float grad_min) {
    const float alpha = x[(row0 + s) * 9 + 8];
    const float a = acc[row0 + s];
    uint64_t cls;
    uint32_t k;
    if (alpha < alpha_dead) {
        cls = 1;
        k = float_key(alpha);
    } else if (ggs_div_rn(a, n_acc) > grad_min) {      // false for a NaN
        cls = 2;
        k = ~float_key(a);
    } else {
        return 0;
    }
    return (cls << 62) | ((uint64_t)k << 30) | (uint32_t)s;
}

__global__ void __launch_bounds__(DT)
density_acc_kernel(const float* __restrict__ g, float* __restrict__ acc, int64_t n, float wm, float hm) {
    const int64_t i = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (i >= n) return;
    const float px = ggs_div_rn(g[i * 9 + 0], wm);
    const float py = ggs_div_rn(g[i * 9 + 1], hm);
    acc[i] = acc[i] + ggs_sqrt_rn(px * px + py * py);
}

// grid (ceil(N / DT), B).  counts [B][2]: dead, sources (zero on entry).
__global__ void __launch_bounds__(DT)
density_rank_kernel(const float* __restrict__ x, const float* __restrict__ acc, int N, int M, float n_acc,
                    float alpha_dead, float grad_min, int* __restrict__ dead_list, int* __restrict__ src_list,
                    int* __restrict__ counts) {
    __shared__ uint64_t t_key[DT];
    const int b = (int)blockIdx.y;
    const int64_t row0 = (int64_t)b * N;
    const int s = (int)blockIdx.x * DT + (int)threadIdx.x;
    const uint64_t key = s < N ? classify(x, acc, row0, s, n_acc, alpha_dead, grad_min) : 0;
    const int cls = (int)(key >> 62);
    // keys of my class below mine: k - base < key - base in unsigned arithmetic (a key
    // of a lower class wraps round, one of a higher class is 2^62 or more above base)
    const uint64_t base = (uint64_t)cls << 62, span = key - base;
    int rank = 0;
    for (int t0 = 0; t0 < N; t0 += DT) {
        const int o = t0 + (int)threadIdx.x;
        const uint64_t k = o < N ? classify(x, acc, row0, o, n_acc, alpha_dead, grad_min) : 0;
        __syncthreads();                       // the previous tile has been counted
        t_key[threadIdx.x] = k;
        __syncthreads();
        // the whole tile, branch-free, so that many reads are in flight: an entry past N
        // is 0, which is nobody's
        if (cls != 0) {
#pragma unroll 16
            for (int j = 0; j < DT; ++j) rank += (t_key[j] - base < span) ? 1 : 0;
        }
    }
    // one atomic per wave and class (every lane is still here)
    const uint64_t dead_lanes = __ballot(cls == 1), src_lanes = __ballot(cls == 2);
    if ((threadIdx.x & 63) == 0) {
        if (dead_lanes) atomicAdd(&counts[2 * b], __popcll(dead_lanes));
        if (src_lanes) atomicAdd(&counts[2 * b + 1], __popcll(src_lanes));
    }
    if (cls != 0 && rank < M) (cls == 1 ? dead_list : src_list)[(int64_t)b * M + rank] = s;
}

struct DensityApplyDev {
    float split_log, log_shrink, split_offset;
    float wm, hm;                 // float(max(W - 1, 1)), float(max(H - 1, 1))
    float log_lo, log_hi;
};

__device__ __forceinline__ float clip(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// One thread per (candidate, pair slot j < M).  pairs [B][M][2] = (dead, source) or
// (-1, -1), is_split [B][M], last_n [B]; moves / splits [B] cumulative (may be null).
__global__ void __launch_bounds__(DT)
density_apply_kernel(float* __restrict__ x, float* __restrict__ m, float* __restrict__ v, int B, int N, int M,
                     const int* __restrict__ dead_list, const int* __restrict__ src_list,
                     const int* __restrict__ counts, DensityApplyDev p, int* __restrict__ pairs,
                     int* __restrict__ is_split, int* __restrict__ last_n, unsigned long long* __restrict__ moves,
                     unsigned long long* __restrict__ splits) {
    const int64_t i = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (i >= (int64_t)B * M) return;
    const int b = (int)(i / M), j = (int)(i % M);
    const int n = min(min(counts[2 * b], counts[2 * b + 1]), M);
    if (j == 0) {
        last_n[b] = n;
        if (moves) moves[b] += (unsigned long long)n;
    }
    if (j >= n) {
        pairs[2 * i] = -1;
        pairs[2 * i + 1] = -1;
        is_split[i] = 0;
        return;
    }
    const int d = dead_list[i], s = src_list[i];
    pairs[2 * i] = d;
    pairs[2 * i + 1] = s;
    if ((unsigned)d >= (unsigned)N || (unsigned)s >= (unsigned)N) return;     // ranks are unique: never taken
    float* __restrict__ xs = x + ((int64_t)b * N + s) * 9;
    float* __restrict__ xd = x + ((int64_t)b * N + d) * 9;
    float r[9];
    for (int c = 0; c < 9; ++c) r[c] = xs[c];
    const float L = r[2] >= r[3] ? r[2] : r[3];
    const bool split = !(L <= p.split_log);
    is_split[i] = split ? 1 : 0;
    if (split) {
        float sn, cs;
        det_sincosf(r[4], &sn, &cs);
        const bool major_a = r[2] >= r[3];
        const float ux = major_a ? cs : -sn, uy = major_a ? sn : cs;
        const float dlt = p.split_offset * det_expf(L);
        const float dx = ggs_div_rn(dlt * ux, p.wm), dy = ggs_div_rn(dlt * uy, p.hm);
        const float la = clip(r[2] - p.log_shrink, p.log_lo, p.log_hi);
        const float lb = clip(r[3] - p.log_shrink, p.log_lo, p.log_hi);
        xs[0] = clip(r[0] + dx, 0.0f, 1.0f);
        xs[1] = clip(r[1] + dy, 0.0f, 1.0f);
        xs[2] = la;
        xs[3] = lb;
        r[0] = clip(r[0] - dx, 0.0f, 1.0f);
        r[1] = clip(r[1] - dy, 0.0f, 1.0f);
        r[2] = la;
        r[3] = lb;
        float* __restrict__ ms = m + ((int64_t)b * N + s) * 9;
        float* __restrict__ vs = v + ((int64_t)b * N + s) * 9;
        for (int c = 0; c < 9; ++c) {
            ms[c] = 0.0f;
            vs[c] = 0.0f;
        }
        if (splits) atomicAdd(&splits[b], 1ull);
    }
    float* __restrict__ md = m + ((int64_t)b * N + d) * 9;
    float* __restrict__ vd = v + ((int64_t)b * N + d) * 9;
    for (int c = 0; c < 9; ++c) {
        xd[c] = r[c];
        md[c] = 0.0f;
        vd[c] = 0.0f;
    }
}

}  // namespace

hipError_t launch_density_acc(hipStream_t st, const float* grad, float* acc, int B, int N, int H, int W) {
    const int64_t n = (int64_t)B * N;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(density_acc_kernel, dim3((unsigned)((n + DT - 1) / DT)), dim3(DT), 0, st, grad, acc, n,
                       (float)(W > 1 ? W - 1 : 1), (float)(H > 1 ? H - 1 : 1));
    return hipGetLastError();
}

hipError_t launch_density_event(hipStream_t st, float* x, float* m, float* v, const float* acc, int n_acc, int B, int N,
                                int H, int W, float log_lo, float log_hi, const ggs_refine_density& d, int M,
                                int* dead_list, int* src_list, int* counts, int* pairs, int* is_split, int* last_n,
                                unsigned long long* moves, unsigned long long* splits) {
    if (B <= 0 || N <= 0 || M <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(int) * 2 * (size_t)B, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(density_rank_kernel, dim3((unsigned)((N + DT - 1) / DT), (unsigned)B), dim3(DT), 0, st, x, acc,
                       N, M, (float)n_acc, d.alpha_dead, d.grad_min, dead_list, src_list, counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    DensityApplyDev p;
    p.split_log = d.split_log;
    p.log_shrink = d.log_shrink;
    p.split_offset = d.split_offset;
    p.wm = (float)(W > 1 ? W - 1 : 1);
    p.hm = (float)(H > 1 ? H - 1 : 1);
    p.log_lo = log_lo;
    p.log_hi = log_hi;
    const int64_t n = (int64_t)B * M;
    hipLaunchKernelGGL(density_apply_kernel, dim3((unsigned)((n + DT - 1) / DT)), dim3(DT), 0, st, x, m, v, B, N, M,
                       dead_list, src_list, counts, p, pairs, is_split, last_n, moves, splits);
    return hipGetLastError();
}

}  // namespace ggs
