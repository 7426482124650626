// Device-resident differential evolution (ggs_de_*): the variation and select
// kernels.  Session in ggs_sess_de.cpp.
#include "ggs_prep.h"
#include "ggs_variation.h"

namespace ggs {

// ---------------------------------------------------------------------------
// differential evolution (ggs_de_*): variation and select
// ---------------------------------------------------------------------------
// Generation gen >= 1 is synchronous: the P trials are built from the population
// as it stood at the start of the generation (ggs/de.py: de_trials states the
// arithmetic, DESIGN.md the algorithm).  Draws of target row i: Philox counter
// (gen, i, what, S_DE), key = seed:
//   what 0          x, y, z -> r1, r2, r3 (mod P-1, P-2, P-3, then de-collided);
//                   w -> jrand (mod 9 N per gene, mod N per splat)
//   what 1          x -> f_u
//   what 2 + 3s + k x, y, z, w -> crossover uniforms of splat s, genes 4k .. 4k+3
//                   (k = 2: x only; per-splat crossover: word x of k = 0 only)
enum : uint32_t { S_DE = 9 };

// r avoids the excluded value e (walked in ascending order of e)
__device__ __forceinline__ int de_skip(int r, int e) { return r + (r >= e ? 1 : 0); }

struct DeIdx {
    int r1, r2, r3;
};
__device__ __forceinline__ DeIdx de_indices(const U4& w, int i, int P) {
    const int r1 = de_skip((int)(w.x % (uint32_t)(P - 1)), i);
    const int r2 = de_skip(de_skip((int)(w.y % (uint32_t)(P - 2)), min(i, r1)), max(i, r1));
    const int lo = min(i, min(r1, r2)), hi = max(i, max(r1, r2)), mid = i + r1 + r2 - lo - hi;
    const int r3 = de_skip(de_skip(de_skip((int)(w.z % (uint32_t)(P - 3)), lo), mid), hi);
    return {r1, r2, r3};
}

// One workgroup per trial, one splat per thread (N > blockDim: several).  No
// draw depends on another splat, so there is no barrier; a splat's nine genes
// stay in statically indexed registers from the loads to the record.
__global__ void __launch_bounds__(1024)
de_variation_kernel(const float* __restrict__ pop, int P, int N, DeParamsDev prm, uint32_t k0, uint32_t k1, int gen,
                    const int* __restrict__ best_row, float* __restrict__ trials, SplatRec* __restrict__ recs,
                    int4* __restrict__ bnds, int H, int W, float k_sigma) {
    const int i = blockIdx.x;
    const Rng rng{k0, k1, (uint32_t)gen};
    const U4 w0 = rng.block(S_DE, (uint32_t)i, 0);
    const DeIdx ix = de_indices(w0, i, P);
    const int jrand = (int)(w0.w % (uint32_t)(prm.crossover ? N : 9 * N));
    const float fspan = prm.f_hi - prm.f_lo;
    const float fmul = u01(rng.block(S_DE, (uint32_t)i, 1).x) * fspan;
    const float F = prm.f_lo + fmul;
    // strategy 0: v = x[r1] + F (x[r2] - x[r3]); 1: v = x[best] + F (x[r1] - x[r2]);
    // 2: v = (x[i] + F (x[best] - x[i])) + F (x[r1] - x[r2])
    const int64_t row = (int64_t)N * 9;
    const int b = prm.strategy == 0 ? ix.r1 : *best_row;
    const float* __restrict__ X = pop + i * row;
    const float* __restrict__ B = pop + b * row;
    const float* __restrict__ Da = pop + (prm.strategy == 0 ? ix.r2 : ix.r1) * row;
    const float* __restrict__ Db = pop + (prm.strategy == 0 ? ix.r3 : ix.r2) * row;
    float* __restrict__ T = trials + i * row;
    for (int s = threadIdx.x; s < N; s += blockDim.x) {
        float cu[9];                            // crossover uniforms of the splat's genes
        const U4 c0 = rng.block(S_DE, (uint32_t)i, (uint32_t)(2 + 3 * s));
        if (prm.crossover) {
#pragma unroll
            for (int c = 0; c < 9; ++c) cu[c] = u01(c0.x);
        } else {
            const U4 c1 = rng.block(S_DE, (uint32_t)i, (uint32_t)(3 + 3 * s));
            const U4 c2 = rng.block(S_DE, (uint32_t)i, (uint32_t)(4 + 3 * s));
            cu[0] = u01(c0.x); cu[1] = u01(c0.y); cu[2] = u01(c0.z); cu[3] = u01(c0.w);
            cu[4] = u01(c1.x); cu[5] = u01(c1.y); cu[6] = u01(c1.z); cu[7] = u01(c1.w);
            cu[8] = u01(c2.x);
        }
        const int j0 = prm.crossover ? (s == jrand ? 0 : -9) : jrand - 9 * s;   // per splat: all nine or none
        float g[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            const float xi = X[(int64_t)s * 9 + c];
            float d = Da[(int64_t)s * 9 + c] - Db[(int64_t)s * 9 + c];
            if (c == 4) d = wrap_angle(d);
            const float fd = F * d;
            float v;
            if (prm.strategy == 2) {
                float d0 = B[(int64_t)s * 9 + c] - xi;
                if (c == 4) d0 = wrap_angle(d0);
                const float fd0 = F * d0;
                const float t = xi + fd0;
                v = t + fd;
            } else {
                v = B[(int64_t)s * 9 + c] + fd;
            }
            // clamp_genome's rule of the column, on genes taken from the mutant only
            if (c < 2) v = clip(v, 0.0f, 1.0f);
            else if (c < 4) v = clip(v, prm.log_lo, prm.log_hi);
            else if (c == 4) v = wrap_angle(v);
            else v = clip(v, 0.0f, 255.0f);
            const bool take = (cu[c] < prm.cr) || (prm.crossover ? j0 == 0 : j0 == c);
            g[c] = take ? v : xi;               // inherited genes: the parent's bits
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) T[(int64_t)s * 9 + c] = g[c];
        float enc[9];
        encode_row(g, enc);
        const SplatRec r = make_rec(preprocess_row(enc, H, W, k_sigma));
        recs[(int64_t)i * N + s] = r;
        bnds[(int64_t)i * N + s] = rec_bounds(r);
    }
}

// grid P + 1.  Workgroup i < P: trial i replaces row i iff f_trial[i] <= f[i]
// (float32 compare: a NaN keeps the parent).  Workgroup P: the new fitness
// vector (fits -> fits_next, never the same buffer: the row workgroups read
// fits), best so far, the curves row and the best row, with the arithmetic of
// breed_stats / the survivors kernel.  init: no trials; statistics of the
// initial population, best set unconditionally (ggs_ga_create's init launch).
__global__ void __launch_bounds__(256)
de_select_kernel(DeSelectDev d, int P, int N, int init) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int64_t row = (int64_t)N * 9;
    if ((int)blockIdx.x < P) {
        const int i = blockIdx.x;
        if (init || !(d.trial_fits[i] <= d.fits[i])) return;
        const float* __restrict__ from = d.trials + i * row;
        float* __restrict__ to = d.pop + i * row;
        for (int64_t q = tid; q < row; q += nt) to[q] = from[q];
        return;
    }
    __shared__ float nf[RANKMAX];
    __shared__ float med[2];
    __shared__ int s_g, s_upd;
    for (int r = tid; r < P; r += nt) {
        float f = d.fits[r];
        if (!init) {
            const float t = d.trial_fits[r];
            if (t <= f) f = t;
            d.fits_next[r] = f;
        }
        nf[r] = f;
    }
    __syncthreads();
    if (tid == 0) {
        int g = 0;
        double sum = (double)nf[0];
        for (int r = 1; r < P; ++r) {
            if (nf[r] < nf[g]) g = r;
            sum += (double)nf[r];
        }
        const double fg = (double)nf[g];
        const int upd = init || fg + 1e-10 < *d.best_fit;
        if (upd) *d.best_fit = fg;
        d.curves_row[0] = *d.best_fit;
        d.curves_row[1] = sum / (double)P;
        *d.best_row = g;                        // the next generation's x[best]
        s_g = g;
        s_upd = upd;
    }
    for (int r = tid; r < P; r += nt) {         // statistics.median
        const float f = nf[r];
        int rank = 0;
        for (int j = 0; j < P; ++j) rank += (nf[j] < f) | ((nf[j] == f) & (j < r));
        if (rank == P / 2) med[1] = f;
        if (rank == P / 2 - 1) med[0] = f;
    }
    __syncthreads();
    if (tid == 0) d.curves_row[2] = (P & 1) ? (double)med[1] : ((double)med[0] + (double)med[1]) / 2.0;
    if (s_upd) {
        // row g of the new population: the trial where it was taken (workgroup g is
        // writing it into pop meanwhile), else the untouched parent
        const int g = s_g;
        const bool taken = !init && d.trial_fits[g] <= d.fits[g];
        const float* __restrict__ from = (taken ? d.trials : d.pop) + g * row;
        for (int64_t q = tid; q < row; q += nt) d.best_ind[q] = from[q];
    }
}

hipError_t launch_de_variation(hipStream_t st, const float* pop, int P, int N, const DeParamsDev& prm, uint64_t seed,
                               int gen, const int* best_row, float* trials, SplatRec* recs, int4* bnds, int H, int W,
                               float k_sigma) {
    if (P < 4 || P > RANKMAX || N < 1) return hipErrorInvalidValue;
    const int nt = N >= 1024 ? 1024 : (N + 63) / 64 * 64;
    hipLaunchKernelGGL(de_variation_kernel, dim3(P), dim3(nt), 0, st, pop, P, N, prm, (uint32_t)seed,
                       (uint32_t)(seed >> 32), gen, best_row, trials, recs, bnds, H, W, k_sigma);
    return hipGetLastError();
}

hipError_t launch_de_select(hipStream_t st, const DeSelectDev& d, int P, int N, int init) {
    if (P < 1 || P > RANKMAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(de_select_kernel, dim3(P + 1), dim3(256), 0, st, d, P, N, init);
    return hipGetLastError();
}

}  // namespace ggs
