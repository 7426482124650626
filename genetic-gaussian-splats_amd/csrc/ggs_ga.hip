// Device-resident genetic algorithm around the fitness pipeline (SURVEY.md §8f
// next #1: algorithm.py:85-141, genetic.py:8-91, utils.py:10-45 on the GPU).
//
// Per generation (all on one stream, no host round trip):
//   variation  1 workgroup / offspring: tournament (genetic.py:8-14), uniform
//              row crossover (:17-21), masked Gaussian mutation with the >=1-flag
//              guarantees (:32-77), wrap/clamp (utils.py:35-45), size-ordered
//              splat swap (:79-91).  Same float32 operation order as ggs/ga.py,
//              which is replay-verified against the reference.
//   fitness    prep + raster + finalize (ggs_kernels.hip) on the offspring
//   survivors  1 workgroup: stable sort of the parents' fitness -> elites,
//              next population = elites + offspring[:P-E] (algorithm.py:129-141),
//              best-so-far (:144-150) and the curves (:153-155)
//   gather     1 workgroup / individual: builds the next population buffer
// Draws come either from explicit per-generation arrays (replay / parity with the
// host path) or from a counter-based Philox4x32-10 generator keyed by
// (seed, generation, individual, splat), which needs no state between launches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ggs_internal.h"
#include "ggs_prep.h"
#include "ggs_variation.h"

namespace ggs {

// ---------------------------------------------------------------------------
// variation
// ---------------------------------------------------------------------------
__device__ int tournament_pick(const float* __restrict__ fits, const GaDrawsDev& d, const Rng& rng,
                               int q, int P, int k) {
    int best = -1;
    for (int j = 0; j < k; ++j) {
        int i;
        if (d.tour_idx) {
            i = d.tour_idx[q * k + j];
        } else {
            const U4 r = rng.block(S_TOUR, (uint32_t)q, (uint32_t)j);
            i = min((int)(u01(r.x) * (float)P), P - 1);
        }
        if (best < 0 || fits[i] < fits[best]) best = i;        // genetic.py:11-13: strict <
    }
    return best;
}

// ---------------------------------------------------------------------------
// breed: survivors + gather of the previous generation fused into the variation
// ---------------------------------------------------------------------------
constexpr int ST = 1024;   // max threads; the launch uses min(ST, pow2 >= P) (cheap barriers at P=128)

// Every breed workgroup rebuilds, in LDS, the next population P_g of
// algorithm.py:129-141 as a row map: row r < E is the parent of rank r (stable
// order of the parents' fitness: elite_prev, written by whoever produced that
// fitness vector — the survivors kernel or the previous breed's stats
// workgroup, from the same counting rank), row r >= E is offspring r - E of the
// generation just evaluated.  s_src[r] follows the survivors kernel's index
// space (parents 0..P-1, offspring P + q), s_nf[r] is the row's fitness.  The
// rows themselves are read from where they are (no gather in front of the
// tournament).
__device__ __forceinline__ int breed_src(const BreedDev& br, int r, int P, int E) {
    return r < E ? br.elite_prev[r] : P + (r - E);
}
__device__ __forceinline__ float breed_fit(const BreedDev& br, int src, int P) {
    return src < P ? br.fits_prev[src] : br.off_fits[src - P];
}
__device__ void breed_rows(const BreedDev& br, int P, float* s_nf, int* s_src) {
    const int E = br.elite_k < 1 ? 1 : br.elite_k;                      // algorithm.py:129
    for (int r = threadIdx.x; r < P; r += blockDim.x) {
        const int src = breed_src(br, r, P, E);
        s_src[r] = src;
        s_nf[r] = breed_fit(br, src, P);
    }
    __syncthreads();
}
__device__ __forceinline__ const float* breed_row(const BreedDev& br, int src, int P, int N) {
    return src < P ? br.pop_prev + (int64_t)src * N * 9 : br.off_prev + (int64_t)(src - P) * N * 9;
}
// The breed grid's extra workgroup: best so far (algorithm.py:143-150), the curves
// row (:153-155; sequential float64 mean, statistics.median), the best row — the
// survivors kernel's arithmetic on the same row map, so the same bits — and the
// next breed's elite list (the median's ranks, rank < E).
__device__ void breed_stats(const BreedDev& br, int P, int N, const float* s_nf, const int* s_src) {
    __shared__ float med[2];
    __shared__ int s_g, s_upd;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int E = br.elite_k < 1 ? 1 : br.elite_k;
    if (tid == 0) {
        int g = 0;
        double sum = (double)s_nf[0];
        for (int r = 1; r < P; ++r) {
            if (s_nf[r] < s_nf[g]) g = r;
            sum += (double)s_nf[r];
        }
        const double fg = (double)s_nf[g];
        const int upd = fg + 1e-10 < *br.best.fit;
        if (upd) {
            *br.best.fit = fg;
            *br.best.src = s_src[g];
        }
        *br.best.updated = upd;
        br.curves_row[0] = *br.best.fit;
        br.curves_row[1] = sum / (double)P;
        s_g = g;
        s_upd = upd;
    }
    for (int r = tid; r < P; r += nt) {
        const float f = s_nf[r];
        int rank = 0;
        for (int j = 0; j < P; ++j) rank += (s_nf[j] < f) | ((s_nf[j] == f) & (j < r));
        if (rank == P / 2) med[1] = f;
        if (rank == P / 2 - 1) med[0] = f;
        if (rank < E) br.elite_next[rank] = r;
    }
    __syncthreads();
    if (tid == 0) br.curves_row[2] = (P & 1) ? (double)med[1] : ((double)med[0] + (double)med[1]) / 2.0;
    if (s_upd) {
        const float* from = breed_row(br, s_src[s_g], P, N);
        for (int64_t i = tid; i < (int64_t)N * 9; i += nt) br.best.ind[i] = from[i];
    }
}

#ifndef GGS_VTIMING
#define GGS_VTIMING 0             // diagnostic build: per-workgroup phase clocks (tools/probe/breed_timing.py)
#endif
#if GGS_VTIMING
__device__ unsigned long long g_ggs_vtiming[8 * 4096];
#define GGS_VMARK(k) do { if (threadIdx.x == 0 && blockIdx.x < 4096) \
    g_ggs_vtiming[8 * blockIdx.x + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define GGS_VMARK(k) do { } while (0)
#endif

// Threads per variation workgroup (one workgroup per offspring): the smallest of
// 256 / 512 / 1024 that gives every splat its own thread up to 1,024 splats (the
// register-resident path below); 256 past that, and 1024 when a few large
// offspring are bred (SA tries at configs[4]: 4,096 splats each), which otherwise
// leave 16 splats per thread on a handful of CUs.  Results do not depend on VT
// (per-splat work, an OR, a sum and an in-order search).
//
// BREED: the generation's survivors and gather run inside this kernel (one extra
// workgroup, o == n_off, keeps best and curves): the parents are the rows of the
// next population P_g (breed_rows), each workgroup o also writes row o of P_g
// (and its fitness) for the generation after.  pop / fits are unused then.
//
// The body is shared by the single-population kernel (o = blockIdx.x) and the
// island kernel (ga_variation_islands_kernel: the same body on island
// blockIdx.y's slices), so an island breeds with a session's exact operations.
template <int VT, bool BREED>
__device__ __forceinline__ void
ga_variation_body(const int o, const float* __restrict__ pop, const float* __restrict__ fits, int P, int N,
                  GaParamsDev prm, GaDrawsDev d, uint32_t k0, uint32_t k1, int gen,
                  float* __restrict__ off, int n_off, SplatRec* __restrict__ recs, int4* __restrict__ bnds,
                  int H, int W, float k_sigma,
                  const SaLoopDev* __restrict__ sl, const SaItDev* __restrict__ sit, BreedDev br) {
    __shared__ int s_a, s_b, s_cx, s_any;
    __shared__ float s_nf[BREED ? RANKMAX : 1];
    __shared__ int s_src[BREED ? RANKMAX : 1];
    __shared__ float s_sizei;
    __shared__ int s_j, s_count;
    __shared__ int s_scan[VT / 64];
    GGS_VMARK(0);                              // o: offspring index
    const int pair = o >> 1;
    const bool first = (o & 1) == 0;
    const int tid = threadIdx.x;

    uint32_t og = (uint32_t)(o + prm.o_base);   // Philox identity of this offspring
    if (sl) {   // SA loop round: neighbour o is global try pos + o = (it, k); it's sigmas from sit
        if (o >= sl->live) return;
        const int64_t g = sl->pos + o;
        const int it = (int)(g / sl->tries);
        og = (uint32_t)(g % sl->tries);
        gen = it;
        const SaItDev& q = sit[it - sl->first_it];
        prm.sig_xy = q.sig[0]; prm.sig_alog = q.sig[1]; prm.sig_blog = q.sig[2];
        prm.sig_theta = q.sig[3]; prm.sig_rgb = q.sig[4]; prm.sig_alpha = q.sig[5];
    }
    if (BREED && o == n_off) {                 // the stats workgroup
        breed_rows(br, P, s_nf, s_src);
        breed_stats(br, P, N, s_nf, s_src);
        return;
    }
    const Rng rng{k0, k1, (uint32_t)gen};
    float* __restrict__ O = off + (int64_t)o * N * 9;
    const float p = prm.mutpb;
    const int64_t ob = (int64_t)o * N;
    const int E = br.elite_k < 1 ? 1 : br.elite_k;

    if (N <= VT) {
        // One splat per thread (s = tid).  Phase A issues everything that does not
        // depend on the parents' fitness — the row-map and gather loads (BREED),
        // the tournament's candidate indices, the crossover decision, every
        // per-splat draw — with no barrier in between, so the loads' latency
        // hides behind the Philox / Box-Muller arithmetic; after one barrier
        // thread 0 only compares fitness values.  The row, its draws and its size
        // then stay in registers / LDS from mutation to swap to prep.  Same
        // operations on the same values as the generic path, so the same bits.
        constexpr int KT = 32;                 // tournament picks precomputed when 2k <= 2*KT
        __shared__ int s_tour[2 * KT];
        __shared__ float s_size[VT];
        __shared__ float s_rowi[9], s_rowj[9];
        const int sp = tid;
        const bool act = sp < N;
        const int k = prm.tour_k;
        const bool pre = !prm.mutate_only && 2 * k <= 2 * KT;
        // --- phase A
        int msrc[(RANKMAX + VT - 1) / VT];               // BREED: row map entries r = tid + VT*i
        float mfit[(RANKMAX + VT - 1) / VT];
        float cp[9];                           // BREED: this thread's part of row o of P_g
        if (BREED) {
#pragma unroll
            for (int i = 0; i < (RANKMAX + VT - 1) / VT; ++i) {
                const int r = tid + VT * i;
                msrc[i] = r < P ? breed_src(br, r, P, E) : 0;
                mfit[i] = r < P ? breed_fit(br, msrc[i], P) : 0.0f;
            }
            const float* __restrict__ from = breed_row(br, breed_src(br, o, P, E), P, N);
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                const int i = tid + VT * c;
                cp[c] = i < N * 9 ? from[i] : 0.0f;
            }
        }
        if (tid == 0) {
            s_any = 0;
            s_j = -1;
            if (prm.mutate_only) {
                s_a = 0;                       // annealing.py:122-128: mutate the current state
                s_b = 0;
                s_cx = 0;
            } else {
                s_cx = d.cx ? d.cx[pair] : (u01(rng.block(S_CX, (uint32_t)pair, 0).x) < prm.cxpb);
            }
        }
        if (pre && tid < 2 * k) {              // candidate j of parent h's tournament (genetic.py:11)
            const int h = tid / k, j = tid % k;
            const int q = h == 0 ? (d.perm ? d.perm[2 * pair] : 2 * pair)
                                 : (d.perm ? d.perm[(2 * pair + 1) % P] : (2 * pair + 1) % P);
            s_tour[tid] = d.tour_idx ? d.tour_idx[q * k + j]
                                     : min((int)(u01(rng.block(S_TOUR, (uint32_t)q, (uint32_t)j).x) * (float)P), P - 1);
        }
        MaskU u{};
        NormD nd{};
        float cxu = 0.0f;
        int any = 0;
        if (act) {
            u = mask_draws(d, rng, og, ob, sp);
            any = mask_any(u, p);
            if (!prm.mutate_only)
                cxu = d.cx_u ? d.cx_u[(int64_t)pair * N + sp]
                             : u01(rng.block(S_CX, (uint32_t)pair, (uint32_t)(sp + 1)).x);   // shared by the pair
            nd = normal_draws(d, rng, og, ob, sp, N);
        }
        if (BREED) {
#pragma unroll
            for (int i = 0; i < (RANKMAX + VT - 1) / VT; ++i) {
                const int r = tid + VT * i;
                if (r < P) {
                    s_src[r] = msrc[i];
                    s_nf[r] = mfit[i];
                }
            }
            fits = s_nf;
        }
        __syncthreads();
        GGS_VMARK(1);
        // --- tournament (genetic.py:8-14, strict <) on the fitness now in place;
        //     the mask groups' any() (genetic.py:24-29) meanwhile
        if (tid == 0 && !prm.mutate_only) {
            if (pre) {
                int best = -1;
                for (int j = 0; j < k; ++j) {
                    const int i = s_tour[j];
                    if (best < 0 || fits[i] < fits[best]) best = i;
                }
                s_a = best;
                best = -1;
                for (int j = 0; j < k; ++j) {
                    const int i = s_tour[k + j];
                    if (best < 0 || fits[i] < fits[best]) best = i;
                }
                s_b = best;
            } else {
                const int qa = d.perm ? d.perm[2 * pair] : 2 * pair;
                const int qb = d.perm ? d.perm[(2 * pair + 1) % P] : (2 * pair + 1) % P;
                s_a = tournament_pick(fits, d, rng, qa, P, k);
                s_b = tournament_pick(fits, d, rng, qb, P, k);
            }
        }
        {
            const int wa = (__ballot(any & ANY_COLOR) ? ANY_COLOR : 0) | (__ballot(any & ANY_XY) ? ANY_XY : 0) |
                           (__ballot(any & ANY_AB) ? ANY_AB : 0) | (__ballot(any & ANY_T) ? ANY_T : 0);
            if ((tid & 63) == 0 && wa) atomicOr(&s_any, wa);
        }
        __syncthreads();
        GGS_VMARK(2);
        any = s_any;
        const Fallback fb = fallbacks(d, rng, og, o, N, any);
        const float* __restrict__ A = BREED ? breed_row(br, s_src[s_a], P, N) : pop + (int64_t)s_a * N * 9;
        const float* __restrict__ Bp = BREED ? breed_row(br, s_src[s_b], P, N) : pop + (int64_t)s_b * N * 9;
        GGS_VMARK(3);
        float g[9];
        if (act) {
            // genetic.py:17-21 (c1 = where(m, a, b), c2 = where(m, b, a)) / duplicate
            const bool m = cxu < 0.5f;
            const bool takeA = s_cx ? (first ? m : !m) : first;
            const float* src = (takeA ? A : Bp) + (int64_t)sp * 9;
#pragma unroll
            for (int c = 0; c < 9; ++c) g[c] = src[c];
            mutate_row(g, u, nd, fb, sp, prm);
            s_size[sp] = expf(g[2]) * expf(g[3]);
        }
        if (N >= 2) {
            // genetic.py:79-91: pick i, then the pick-th later splat bigger than i
            const int i = d.swap_i ? d.swap_i[o] : (int)(rng.block(S_IND, og, 4).x % (uint32_t)(N - 1));
            __syncthreads();
            GGS_VMARK(4);
            const float sizei = s_size[i];
            const bool c = act && sp > i && s_size[sp] > sizei;
            const uint64_t bal = __ballot(c);
            const int lane = tid & 63, w = tid >> 6;
            if (lane == 0) s_scan[w] = __popcll(bal);
            __syncthreads();
            int count = 0, before = 0;
            for (int q = 0; q < VT / 64; ++q) {
                before += q < w ? s_scan[q] : 0;
                count += s_scan[q];
            }
            if (count > 0) {
                int pick;
                if (d.swap_pick && d.swap_pick[o] >= 0) pick = d.swap_pick[o];
                else {
                    const double uu = d.swap_u ? d.swap_u[o] : (double)u01(rng.block(S_IND, og, 5).x);
                    pick = (int)(uu * (double)count);
                    if (pick > count - 1) pick = count - 1;
                }
                const int inwave = __popcll(bal & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
                if (c && before + inwave == pick) s_j = sp;       // the (pick+1)-th in splat order
                __syncthreads();
                const int j = s_j;
                if (sp == i) {
#pragma unroll
                    for (int q = 0; q < 9; ++q) s_rowi[q] = g[q];
                }
                if (sp == j) {
#pragma unroll
                    for (int q = 0; q < 9; ++q) s_rowj[q] = g[q];
                }
                __syncthreads();
                if (sp == i) {
#pragma unroll
                    for (int q = 0; q < 9; ++q) g[q] = s_rowj[q];
                }
                if (sp == j) {
#pragma unroll
                    for (int q = 0; q < 9; ++q) g[q] = s_rowi[q];
                }
            }
        }
        GGS_VMARK(5);
        if (act) {
#pragma unroll
            for (int c = 0; c < 9; ++c) O[(int64_t)sp * 9 + c] = g[c];
            if (recs) {         // prep fused in (ggs_prep.h): the raster's record of this splat
                float row[9];
                encode_row(g, row);
                const SplatRec r = make_rec(preprocess_row(row, H, W, k_sigma));
                recs[ob + sp] = r;
                bnds[ob + sp] = rec_bounds(r);
            }
        }
        if (BREED) {            // gather: row o of P_g and its fitness, for the generation after
            float* __restrict__ to = br.pop_next + (int64_t)o * N * 9;
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                const int i = tid + VT * c;
                if (i < N * 9) to[i] = cp[c];
            }
            if (tid == 0) br.fits_next[o] = s_nf[o];
        }
#if GGS_VTIMING
        __syncthreads();
#endif
        GGS_VMARK(6);
        return;
    }

    // ---- generic path (N > VT: several splats per thread) ------------------------
    if (BREED) {
        breed_rows(br, P, s_nf, s_src);
        const float* __restrict__ from = breed_row(br, s_src[o], P, N);     // gather: row o of P_g
        float* __restrict__ to = br.pop_next + (int64_t)o * N * 9;
        for (int64_t i = tid; i < (int64_t)N * 9; i += VT) to[i] = from[i];
        if (tid == 0) br.fits_next[o] = s_nf[o];
        fits = s_nf;
    }
    if (tid == 0 && prm.mutate_only) {
        s_a = 0;                               // annealing.py:122-128: mutate the current state
        s_b = 0;
        s_cx = 0;
    } else if (tid == 0) {
        // parents 2*pair and 2*pair+1 of the (shuffled) tournament winners
        const int qa = d.perm ? d.perm[2 * pair] : 2 * pair;
        const int qb = d.perm ? d.perm[(2 * pair + 1) % P] : (2 * pair + 1) % P;
        s_a = tournament_pick(fits, d, rng, qa, P, prm.tour_k);
        s_b = tournament_pick(fits, d, rng, qb, P, prm.tour_k);
        if (d.cx) s_cx = d.cx[pair];
        else s_cx = u01(rng.block(S_CX, (uint32_t)pair, 0).x) < prm.cxpb;
    }
    __syncthreads();
    const float* __restrict__ A = BREED ? breed_row(br, s_src[s_a], P, N) : pop + (int64_t)s_a * N * 9;
    const float* __restrict__ Bp = BREED ? breed_row(br, s_src[s_b], P, N) : pop + (int64_t)s_b * N * 9;

    // pass 1: crossover + mask flags, any() per mask group
    int any = 0;
    for (int s = tid; s < N; s += VT) any |= mask_any(mask_draws(d, rng, og, ob, s), p);
    any = (__syncthreads_or(any & ANY_COLOR) ? ANY_COLOR : 0) | (__syncthreads_or(any & ANY_XY) ? ANY_XY : 0) |
          (__syncthreads_or(any & ANY_AB) ? ANY_AB : 0) | (__syncthreads_or(any & ANY_T) ? ANY_T : 0);
    // genetic.py:24-29: fallback flat indices (k into [N,2] or [N,1] row-major)
    const Fallback fb = fallbacks(d, rng, og, o, N, any);

    // pass 2: build the child row, mutate, wrap, clamp -> off
    for (int s = tid; s < N; s += VT) {
        const MaskU u = mask_draws(d, rng, og, ob, s);
        const NormD nd = normal_draws(d, rng, og, ob, s, N);
        float cxu = 0.0f;
        if (s_cx) cxu = d.cx_u ? d.cx_u[(int64_t)pair * N + s]
                               : u01(rng.block(S_CX, (uint32_t)pair, (uint32_t)(s + 1)).x);   // shared by the pair
        // genetic.py:17-21 (c1 = where(m, a, b), c2 = where(m, b, a)) / duplicate
        const bool m = cxu < 0.5f;
        const bool takeA = s_cx ? (first ? m : !m) : first;
        const float* src = (takeA ? A : Bp) + (int64_t)s * 9;
        float g[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) g[c] = src[c];
        mutate_row(g, u, nd, fb, s, prm);      // flags with the one-true fallbacks, mutation, clamp
#pragma unroll
        for (int c = 0; c < 9; ++c) O[(int64_t)s * 9 + c] = g[c];
    }
    if (N >= 2) {
    __syncthreads();   // workgroup-scope ordering of the rows just written

    // genetic.py:79-91: pick i, then the pick-th later splat bigger than i
    int i;
    if (d.swap_i) i = d.swap_i[o];
    else i = (int)(rng.block(S_IND, og, 4).x % (uint32_t)(N - 1));
    if (tid == 0) {
        s_sizei = expf(O[(int64_t)i * 9 + 2]) * expf(O[(int64_t)i * 9 + 3]);
        s_j = -1;
    }
    __syncthreads();
    const float sizei = s_sizei;
    int cnt = 0;
    for (int s = tid; s < N; s += VT)
        cnt += (s > i) && (expf(O[(int64_t)s * 9 + 2]) * expf(O[(int64_t)s * 9 + 3]) > sizei);
    {   // total candidates: workgroup sum
        const int lane = tid & 63, w = tid >> 6;
        int v = cnt;
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) s_scan[w] = v;
        __syncthreads();
        if (tid == 0) {
            int tot = 0;
            for (int k = 0; k < VT / 64; ++k) tot += s_scan[k];
            s_count = tot;
        }
        __syncthreads();
    }
    const int count = s_count;
    if (count > 0) {
    int pick;
    if (d.swap_pick && d.swap_pick[o] >= 0) pick = d.swap_pick[o];
    else {
        const double u = d.swap_u ? d.swap_u[o] : (double)u01(rng.block(S_IND, og, 5).x);
        pick = (int)(u * (double)count);
        if (pick > count - 1) pick = count - 1;
    }
    // find the (pick+1)-th candidate in splat order: walk 256-splat chunks
    int seen = 0;
    for (int base = 0; base < N; base += VT) {
        const int s = base + tid;
        const bool c = s < N && s > i &&
                       (expf(O[(int64_t)s * 9 + 2]) * expf(O[(int64_t)s * 9 + 3]) > sizei);
        // exclusive prefix of c across the workgroup (in s order)
        const uint64_t bal = __ballot(c);
        const int lane = tid & 63, w = tid >> 6;
        const int inwave = __popcll(bal & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
        __syncthreads();
        if (lane == 0) s_scan[w] = __popcll(bal);
        __syncthreads();
        int before = seen;
        for (int k = 0; k < w; ++k) before += s_scan[k];
        if (c && before + inwave == pick) s_j = s;
        int tot = 0;
        for (int k = 0; k < VT / 64; ++k) tot += s_scan[k];
        seen += tot;
        __syncthreads();
        if (s_j >= 0) break;
    }
    const int j = s_j;
    if (tid < 9 && j >= 0) {
        const float a = O[(int64_t)i * 9 + tid], b = O[(int64_t)j * 9 + tid];
        O[(int64_t)i * 9 + tid] = b;
        O[(int64_t)j * 9 + tid] = a;
    }
    }   // count > 0
    }   // N >= 2
    if (recs) {             // prep fused in (ggs_prep.h): the raster's records of this offspring
        __syncthreads();    // swapped rows visible to the workgroup
        for (int s = tid; s < N; s += VT) {
            float row[9];
            encode_row(O + (int64_t)s * 9, row);
            const SplatRec r = make_rec(preprocess_row(row, H, W, k_sigma));
            recs[(int64_t)o * N + s] = r;
            bnds[(int64_t)o * N + s] = rec_bounds(r);
        }
    }
}

template <int VT, bool BREED>
__global__ void __launch_bounds__(VT)
ga_variation_kernel(const float* __restrict__ pop, const float* __restrict__ fits, int P, int N,
                    GaParamsDev prm, GaDrawsDev d, uint32_t k0, uint32_t k1, int gen,
                    float* __restrict__ off, int n_off, SplatRec* __restrict__ recs, int4* __restrict__ bnds,
                    int H, int W, float k_sigma,
                    const SaLoopDev* __restrict__ sl, const SaItDev* __restrict__ sit, BreedDev br) {
    ga_variation_body<VT, BREED>(blockIdx.x, pop, fits, P, N, prm, d, k0, k1, gen, off, n_off, recs, bnds, H, W,
                                 k_sigma, sl, sit, br);
}

// Island group: grid (offspring [+ stats workgroup], island).  Every pointer is
// the group's base; island k's slice starts k strides in (IslandStride).  The
// offspring's raster records are compact: only offspring o < P - E of an island
// are evaluated, and island k's go to candidates k (P - E) + o of one batch.
struct IslandStride {
    int64_t pop;                // P * N * 9 floats: populations, offspring
    int rows;                   // P: fits, elite lists, src
    int evals;                  // P - E: offspring fitness, raster records (in candidates)
    int64_t ind;                // N * 9: best individual
};
__device__ __forceinline__ IslandStride island_stride(int P, int N, int elite_k) {
    return {(int64_t)P * N * 9, P, P - (elite_k < 1 ? 1 : elite_k), (int64_t)N * 9};
}
__device__ __forceinline__ GaBestDev island_best(GaBestDev b, int k, const IslandStride& is) {
    return {b.fit + k, b.src + k, b.updated + k, b.ind + k * is.ind};
}

template <int VT, bool BREED>
__global__ void __launch_bounds__(VT)
ga_variation_islands_kernel(const float* __restrict__ pop, const float* __restrict__ fits, int P, int N,
                            GaParamsDev prm, const uint64_t* __restrict__ seeds, int gen,
                            float* __restrict__ off, SplatRec* __restrict__ recs, int4* __restrict__ bnds,
                            int H, int W, float k_sigma, BreedDev br) {
    const int o = blockIdx.x, k = blockIdx.y;
    const IslandStride is = island_stride(P, N, br.elite_k);
    const uint64_t seed = seeds[k];
    if (BREED) {
        br.pop_prev += k * is.pop;
        br.fits_prev += k * is.rows;
        br.off_prev += k * is.pop;
        br.off_fits += k * is.evals;
        br.elite_prev += k * is.rows;
        br.elite_next += k * is.rows;
        br.pop_next += k * is.pop;
        br.fits_next += k * is.rows;
        br.curves_row += 3 * k;
        br.best = island_best(br.best, k, is);
    } else {
        pop += k * is.pop;
        fits += k * is.rows;
    }
    // the last E offspring are bred (their draws keep the trajectory) but get no record
    const bool rec = o < is.evals;
    ga_variation_body<VT, BREED>(o, pop, fits, P, N, prm, GaDrawsDev{}, (uint32_t)seed, (uint32_t)(seed >> 32), gen,
                                 off + k * is.pop, P, rec ? recs + (int64_t)k * is.evals * N : nullptr,
                                 rec ? bnds + (int64_t)k * is.evals * N : nullptr, H, W, k_sigma, nullptr, nullptr,
                                 br);
}

// ---------------------------------------------------------------------------
// survivors: elites by stable fitness order, next fitness vector, best, curves
// ---------------------------------------------------------------------------

// bitonic sort of n2 (power of two) LDS keys (+ optional indices), ascending;
// ties by index: lexicographic (key, idx) == Python's stable sorted()
__device__ void bitonic(float* key, int* idx, int n2) {
    const int nt = blockDim.x;
    for (int k = 2; k <= n2; k <<= 1) {
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            for (int i = threadIdx.x; i < n2; i += nt) {
                const int l = i ^ jj;
                if (l > i) {
                    const bool up = (i & k) == 0;
                    const bool gt = key[i] > key[l] || (idx && key[i] == key[l] && idx[i] > idx[l]);
                    if (gt == up) {
                        const float tk = key[i]; key[i] = key[l]; key[l] = tk;
                        if (idx) { const int ti = idx[i]; idx[i] = idx[l]; idx[l] = ti; }
                    }
                }
            }
            __syncthreads();
        }
    }
}

// RANKED: the counting-rank path only (P <= RANKMAX; the island kernel), with
// LDS arrays of that size.
template <bool RANKED>
__device__ __forceinline__ void
ga_survivors_body(const float* __restrict__ fits, const float* __restrict__ off_fits, int P,
                  int elite_k, int* __restrict__ src, float* __restrict__ new_fits,
                  GaBestDev best, double* __restrict__ curves_row, int init, FitReduce fr,
                  int* __restrict__ elite_next) {
    constexpr int SMAX = RANKED ? RANKMAX : ggs::SMAX;
    // The surviving offspring's fitness (rows E..P-1 of the next generation):
    // given, or reduced here from the raster's strip partials, one wave per
    // candidate (finalize_wave: the same bits as finalize_kernel).
    const int E0 = elite_k < 1 ? 1 : elite_k;
    __shared__ float nf[SMAX];           // the next generation's fitness vector
    if (!init && fr.partials) {          // one wave per candidate
        const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
        for (int q = wave; q < P - E0; q += nw) {
            const float f = finalize_wave(fr.partials, fr.wpartials, fr.nT, fr.mode, fr.hw, q);
            if ((threadIdx.x & 63) == 0) {
                nf[E0 + q] = f;
                new_fits[E0 + q] = f;
                src[E0 + q] = P + q;                                // offspring q
            }
        }
    } else if (!init) {                  // one thread per candidate
        for (int q = threadIdx.x; q < P - E0; q += blockDim.x) {
            const float f = off_fits[q];
            nf[E0 + q] = f;
            new_fits[E0 + q] = f;
            src[E0 + q] = P + q;
        }
    }
    __shared__ float key[SMAX];
    __shared__ int idx[SMAX];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int E = elite_k < 1 ? 1 : elite_k;                      // algorithm.py:129
    if (RANKED || P <= RANKMAX) {
        // Small populations: ranks by counting (one LDS pass per element, 3
        // barriers) instead of two bitonic sorts (~60 barriers).  rank(r) = #{j:
        // (f_j, j) < (f_r, r)} is the position in Python's stable sorted().
        __shared__ float med[2];
        for (int r = tid; r < P; r += nt) key[r] = fits[r];
        __syncthreads();
        if (!init) {
            for (int r = tid; r < P; r += nt) {
                const float f = key[r];
                int rank = 0;
                for (int j = 0; j < P; ++j) rank += (key[j] < f) | ((key[j] == f) & (j < r));
                if (rank < E) {                                   // an elite, from the parents
                    src[rank] = r;
                    new_fits[rank] = f;
                    nf[rank] = f;
                }
            }
            // rows E..P-1 (the offspring) were written above
        } else {
            for (int r = tid; r < P; r += nt) nf[r] = key[r];
        }
        __syncthreads();
        if (tid == 0) {
            int g = 0;
            double sum = (double)nf[0];                           // sum(fitnesses) / len, in order
            for (int r = 1; r < P; ++r) {
                if (nf[r] < nf[g]) g = r;
                sum += (double)nf[r];
            }
            const double fg = (double)nf[g];
            if (init || fg + 1e-10 < *best.fit) {
                *best.fit = fg;
                *best.src = init ? g : src[g];
                *best.updated = 1;
            } else {
                *best.updated = 0;
            }
            curves_row[0] = *best.fit;
            curves_row[1] = sum / (double)P;
        }
        for (int r = tid; r < P; r += nt) {                       // statistics.median
            const float f = nf[r];
            int rank = 0;
            for (int j = 0; j < P; ++j) rank += (nf[j] < f) | ((nf[j] == f) & (j < r));
            if (rank == P / 2) med[1] = f;
            if (rank == P / 2 - 1) med[0] = f;
            if (elite_next && rank < E) elite_next[rank] = r;    // the fused breed's row map
        }
        __syncthreads();
        if (tid == 0)
            curves_row[2] = (P & 1) ? (double)med[1] : ((double)med[0] + (double)med[1]) / 2.0;
        return;
    }
    int n2 = 1;
    while (n2 < P) n2 <<= 1;
    if (!init) {
        for (int i = tid; i < n2; i += nt) {
            key[i] = i < P ? fits[i] : __builtin_inff();
            idx[i] = i < P ? i : 0x7fffffff;
        }
        __syncthreads();
        bitonic(key, idx, n2);
        for (int r = tid; r < E; r += nt) {                       // the elites, from the parents
            src[r] = idx[r];
            new_fits[r] = key[r];
            nf[r] = key[r];
        }
    } else {
        for (int r = tid; r < P; r += nt) nf[r] = fits[r];
    }
    __syncthreads();
    // best so far (algorithm.py:64-67, 143-150) and curves (:71-75, 153-155)
    if (tid == 0) {
        int g = 0;
        double sum = (double)nf[0];                               // sum(fitnesses) / len, in order
        for (int r = 1; r < P; ++r) {
            if (nf[r] < nf[g]) g = r;
            sum += (double)nf[r];
        }
        const double fg = (double)nf[g];
        if (init || fg + 1e-10 < *best.fit) {
            *best.fit = fg;
            *best.src = init ? g : src[g];
            *best.updated = 1;
        } else {
            *best.updated = 0;
        }
        curves_row[0] = *best.fit;
        curves_row[1] = sum / (double)P;
    }
    // median: sort the new fitness values (statistics.median on the list)
    for (int i = tid; i < n2; i += nt) key[i] = i < P ? nf[i] : __builtin_inff();
    __syncthreads();
    bitonic(key, nullptr, n2);
    if (tid == 0)
        curves_row[2] = (P & 1) ? (double)key[P / 2] : ((double)key[P / 2 - 1] + (double)key[P / 2]) / 2.0;
}

__global__ void __launch_bounds__(ST)
ga_survivors_kernel(const float* __restrict__ fits, const float* __restrict__ off_fits, int P,
                    int elite_k, int* __restrict__ src, float* __restrict__ new_fits,
                    GaBestDev best, double* __restrict__ curves_row, int init, FitReduce fr,
                    int* __restrict__ elite_next) {
    ga_survivors_body<false>(fits, off_fits, P, elite_k, src, new_fits, best, curves_row, init, fr, elite_next);
}

// one workgroup per island (P <= RANKMAX), on island blockIdx.x's slices
__global__ void __launch_bounds__(RANKMAX)
ga_survivors_islands_kernel(const float* __restrict__ fits, const float* __restrict__ off_fits, int P, int N,
                            int elite_k, int* __restrict__ src, float* __restrict__ new_fits,
                            GaBestDev best, double* __restrict__ curves_row, int init,
                            int* __restrict__ elite_next) {
    const int k = blockIdx.x;
    const IslandStride is = island_stride(P, N, elite_k);
    ga_survivors_body<true>(fits + k * is.rows, init ? nullptr : off_fits + k * is.evals, P, elite_k,
                            src + k * is.rows, init ? nullptr : new_fits + k * is.rows, island_best(best, k, is),
                            curves_row + 3 * k, init, FitReduce{}, elite_next + k * is.rows);
}

// next population rows from (parents | offspring) by src; best row if improved
__device__ __forceinline__ void
ga_gather_body(const int r, const float* __restrict__ pop, const float* __restrict__ off, int P, int N,
               const int* __restrict__ src, float* __restrict__ next, GaBestDev best, int init) {
    const int sidx = init ? r : src[r];
    const float* from = sidx < P ? pop + (int64_t)sidx * N * 9 : off + (int64_t)(sidx - P) * N * 9;
    float* to = next + (int64_t)r * N * 9;
    const int64_t n = (int64_t)N * 9;
    if (!init)
        for (int64_t i = threadIdx.x; i < n; i += 256) to[i] = from[i];
    if (*best.updated && *best.src == sidx)      // the new best individual
        for (int64_t i = threadIdx.x; i < n; i += 256) best.ind[i] = from[i];
}

__global__ void __launch_bounds__(256)
ga_gather_kernel(const float* __restrict__ pop, const float* __restrict__ off, int P, int N,
                 const int* __restrict__ src, float* __restrict__ next, GaBestDev best, int init) {
    ga_gather_body(blockIdx.x, pop, off, P, N, src, next, best, init);
}

// grid (row, island)
__global__ void __launch_bounds__(256)
ga_gather_islands_kernel(const float* __restrict__ pop, const float* __restrict__ off, int P, int N, int elite_k,
                         const int* __restrict__ src, float* __restrict__ next, GaBestDev best, int init) {
    const int k = blockIdx.y;
    const IslandStride is = island_stride(P, N, elite_k);
    ga_gather_body(blockIdx.x, pop + k * is.pop, init ? nullptr : off + k * is.pop, P, N,
                   init ? nullptr : src + k * is.rows, init ? nullptr : next + k * is.pop,
                   island_best(best, k, is), init);
}

// ---------------------------------------------------------------------------
// ring migration between islands (K >= 2, 0 < m <= P / 2)
// ---------------------------------------------------------------------------
// All islands act at once on the pre-migration state: the row of rank j < m of
// island (k - 1 + K) mod K overwrites the row of rank P - 1 - j of island k
// (genome and fitness; ranks by the stable counting rank: ascending fitness,
// ties by lower row).  Two launches keep the ranking off the rows being
// written: ga_migrate_rank_kernel lists every island's m best and m worst rows
// from the untouched fitness vectors; ga_migrate_apply_kernel then copies.  It
// reads only best-m rows and writes only worst-m rows, which are disjoint
// within an island for m <= P / 2, so no workgroup reads what another writes.
__global__ void __launch_bounds__(RANKMAX)
ga_migrate_rank_kernel(const float* __restrict__ fits, int P, int m, int* __restrict__ mig) {
    __shared__ float key[RANKMAX];
    const int k = blockIdx.x;
    const float* __restrict__ f = fits + (int64_t)k * P;
    int* __restrict__ out = mig + (int64_t)k * 2 * m;   // [0, m): row of rank j; [m, 2m): row of rank P-1-j
    for (int r = threadIdx.x; r < P; r += blockDim.x) key[r] = f[r];
    __syncthreads();
    for (int r = threadIdx.x; r < P; r += blockDim.x) {
        const float v = key[r];
        int rank = 0;
        for (int j = 0; j < P; ++j) rank += (key[j] < v) | ((key[j] == v) & (j < r));
        if (rank < m) out[rank] = r;
        if (P - 1 - rank < m) out[m + (P - 1 - rank)] = r;
    }
}

// grid (m + 1, island).  Workgroup j < m copies emigrant j's genome; workgroup m
// installs the immigrants' fitness and recomputes the island's elite list (the
// breed's row map) from its new fitness vector.
// Islands with a target each (ggs_ga_islands_create_targets) run it as two
// launches around the immigrants' re-evaluation: grid (m, island) with `stage`
// ([K][m][N][9]: the genomes also go there, compact, for the grouped fitness
// launch), then grid (1, island) with j0 = m and `refit` ([K][m]: the immigrants'
// fitness against island k's target, installed instead of the source island's).
__global__ void __launch_bounds__(RANKMAX)
ga_migrate_apply_kernel(float* __restrict__ pop, float* __restrict__ fits, int P, int N, int m, int elite_k,
                        const int* __restrict__ mig, int* __restrict__ elite, int j0, float* __restrict__ stage,
                        const float* __restrict__ refit) {
    const int j = blockIdx.x + j0, k = blockIdx.y, K = gridDim.y;
    const int from_k = (k - 1 + K) % K;
    const int* __restrict__ best_from = mig + (int64_t)from_k * 2 * m;
    const int* __restrict__ worst_to = mig + (int64_t)k * 2 * m + m;
    const int64_t row = (int64_t)N * 9;
    if (j < m) {
        const float* __restrict__ from = pop + ((int64_t)from_k * P + best_from[j]) * row;
        float* __restrict__ to = pop + ((int64_t)k * P + worst_to[j]) * row;
        if (stage) {
            float* __restrict__ sg = stage + ((int64_t)k * m + j) * row;
            for (int64_t i = threadIdx.x; i < row; i += blockDim.x) {
                const float v = from[i];
                to[i] = v;
                sg[i] = v;
            }
            return;
        }
        for (int64_t i = threadIdx.x; i < row; i += blockDim.x) to[i] = from[i];
        return;
    }
    __shared__ float key[RANKMAX];
    float* __restrict__ f = fits + (int64_t)k * P;
    for (int r = threadIdx.x; r < P; r += blockDim.x) key[r] = f[r];
    __syncthreads();
    // the emigrants' fitness: best-m rows of the neighbour, which nobody writes
    for (int q = threadIdx.x; q < m; q += blockDim.x) {
        const float v = refit ? refit[(int64_t)k * m + q] : fits[(int64_t)from_k * P + best_from[q]];
        key[worst_to[q]] = v;
        f[worst_to[q]] = v;
    }
    __syncthreads();
    const int E = elite_k < 1 ? 1 : elite_k;
    int* __restrict__ el = elite + (int64_t)k * P;
    for (int r = threadIdx.x; r < P; r += blockDim.x) {
        const float v = key[r];
        int rank = 0;
        for (int q = 0; q < P; ++q) rank += (key[q] < v) | ((key[q] == v) & (q < r));
        if (rank < E) el[rank] = r;
    }
}

// ---------------------------------------------------------------------------
hipError_t launch_ga_variation(hipStream_t st, const float* pop, const float* fits, int P, int N,
                               const GaParamsDev& prm, const GaDrawsDev& d, uint64_t seed, int gen,
                               float* off, int n_off, SplatRec* recs, int4* bnds, int H, int W, float k_sigma,
                               const SaLoopDev* sl, const SaItDev* sit, const BreedDev* br) {
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    // The smallest workgroup that holds one splat per thread (the register-resident
    // path, N <= VT) up to 1,024 splats: the shipped GA run (config.py: 512 splats)
    // on the generic path (two splats per thread, the child rows round-tripping
    // through HBM between the passes) bred in 21.6 us per generation.
    // Past 1,024 splats (the generic path, several splats per thread) 256 threads,
    // unless the launch is too small to fill the chip (< 64 workgroups): the same
    // rule for the breed (+ stats workgroup) and the plain variation launch.
    const int vt = N <= 256 ? 256 : N <= 512 ? 512 : (N <= 1024 || n_off < 64) ? 1024 : 256;
#define GGS_VAR(VTT, BR, NB, BD)                                                                  \
    hipLaunchKernelGGL((ga_variation_kernel<VTT, BR>), dim3(NB), dim3(VTT), 0, st, pop, fits, P, N, prm, d, k0, \
                       k1, gen, off, n_off, recs, bnds, H, W, k_sigma, sl, sit, BD)
    if (br) {       // + the stats workgroup
        if (P > RANKMAX || n_off != P) return hipErrorInvalidValue;
        if (vt == 256) GGS_VAR(256, true, n_off + 1, *br);
        else if (vt == 512) GGS_VAR(512, true, n_off + 1, *br);
        else GGS_VAR(1024, true, n_off + 1, *br);
    } else {
        if (vt == 256) GGS_VAR(256, false, n_off, BreedDev{});
        else if (vt == 512) GGS_VAR(512, false, n_off, BreedDev{});
        else GGS_VAR(1024, false, n_off, BreedDev{});
    }
#undef GGS_VAR
    return hipGetLastError();
}

hipError_t launch_ga_survivors(hipStream_t st, const float* fits, const float* off_fits, int P,
                               int elite_k, int* src, float* new_fits, const GaBestDev& best,
                               double* curves_row, int init, const FitReduce& fr, int* elite_next) {
    int nt = fr.partials ? 512 : 64;   // 8 waves for the fused per-candidate reductions
    while (nt < P && nt < ST) nt <<= 1;
    hipLaunchKernelGGL(ga_survivors_kernel, dim3(1), dim3(nt), 0, st, fits, off_fits, P, elite_k,
                       src, new_fits, best, curves_row, init, fr, elite_next);
    return hipGetLastError();
}

hipError_t launch_ga_gather(hipStream_t st, const float* pop, const float* off, int P, int N,
                            const int* src, float* next, const GaBestDev& best, int init) {
    hipLaunchKernelGGL(ga_gather_kernel, dim3(P), dim3(256), 0, st, pop, off, P, N, src, next, best,
                       init);
    return hipGetLastError();
}

// ---- island groups: the same launches with an island grid dimension ----------
hipError_t launch_ga_variation_islands(hipStream_t st, int K, const float* pop, const float* fits, int P, int N,
                                       const GaParamsDev& prm, const uint64_t* seeds, int gen, float* off,
                                       SplatRec* recs, int4* bnds, int H, int W, float k_sigma, int elite_k,
                                       const BreedDev* br) {
    if (K < 1 || P > RANKMAX) return hipErrorInvalidValue;
    // launch_ga_variation's rule, on the launch's total workgroup count
    const int vt = N <= 256 ? 256 : N <= 512 ? 512 : (N <= 1024 || (int64_t)K * P < 64) ? 1024 : 256;
    BreedDev b = br ? *br : BreedDev{};
    b.elite_k = elite_k;
#define GGS_VARI(VTT, BR)                                                                                     \
    hipLaunchKernelGGL((ga_variation_islands_kernel<VTT, BR>), dim3(BR ? P + 1 : P, K), dim3(VTT), 0, st, pop, \
                       fits, P, N, prm, seeds, gen, off, recs, bnds, H, W, k_sigma, b)
    if (br) {       // + the stats workgroup of every island
        if (vt == 256) GGS_VARI(256, true);
        else if (vt == 512) GGS_VARI(512, true);
        else GGS_VARI(1024, true);
    } else {
        if (vt == 256) GGS_VARI(256, false);
        else if (vt == 512) GGS_VARI(512, false);
        else GGS_VARI(1024, false);
    }
#undef GGS_VARI
    return hipGetLastError();
}

hipError_t launch_ga_survivors_islands(hipStream_t st, int K, const float* fits, const float* off_fits, int P, int N,
                                       int elite_k, int* src, float* new_fits, const GaBestDev& best,
                                       double* curves_row, int init, int* elite_next) {
    if (K < 1 || P > RANKMAX) return hipErrorInvalidValue;
    int nt = 64;
    while (nt < P && nt < RANKMAX) nt <<= 1;
    hipLaunchKernelGGL(ga_survivors_islands_kernel, dim3(K), dim3(nt), 0, st, fits, off_fits, P, N, elite_k, src,
                       new_fits, best, curves_row, init, elite_next);
    return hipGetLastError();
}

hipError_t launch_ga_gather_islands(hipStream_t st, int K, const float* pop, const float* off, int P, int N,
                                    int elite_k, const int* src, float* next, const GaBestDev& best, int init) {
    hipLaunchKernelGGL(ga_gather_islands_kernel, dim3(P, K), dim3(256), 0, st, pop, off, P, N, elite_k, src, next,
                       best, init);
    return hipGetLastError();
}

hipError_t launch_ga_migrate(hipStream_t st, int K, float* pop, float* fits, int P, int N, int m, int elite_k,
                             int* mig, int* elite) {
    if (K < 2 || m < 1 || 2 * m > P || P > RANKMAX) return hipErrorInvalidValue;
    int nt = 64;
    while (nt < P && nt < RANKMAX) nt <<= 1;
    hipLaunchKernelGGL(ga_migrate_rank_kernel, dim3(K), dim3(nt), 0, st, fits, P, m, mig);
    hipLaunchKernelGGL(ga_migrate_apply_kernel, dim3(m + 1, K), dim3(nt < 256 ? 256 : nt), 0, st, pop, fits, P, N, m,
                       elite_k, mig, elite, 0, (float*)nullptr, (const float*)nullptr);
    return hipGetLastError();
}

hipError_t launch_ga_migrate_copy(hipStream_t st, int K, float* pop, const float* fits, int P, int N, int m,
                                  int* mig, float* stage) {
    if (K < 2 || m < 1 || 2 * m > P || P > RANKMAX || !stage) return hipErrorInvalidValue;
    int nt = 64;
    while (nt < P && nt < RANKMAX) nt <<= 1;
    hipLaunchKernelGGL(ga_migrate_rank_kernel, dim3(K), dim3(nt), 0, st, fits, P, m, mig);
    hipLaunchKernelGGL(ga_migrate_apply_kernel, dim3(m, K), dim3(nt < 256 ? 256 : nt), 0, st, pop, (float*)nullptr, P,
                       N, m, 0, mig, (int*)nullptr, 0, stage, (const float*)nullptr);
    return hipGetLastError();
}

hipError_t launch_ga_migrate_install(hipStream_t st, int K, float* fits, int P, int m, int elite_k, const int* mig,
                                     const float* refit, int* elite) {
    if (K < 2 || m < 1 || 2 * m > P || P > RANKMAX || !refit) return hipErrorInvalidValue;
    int nt = 64;
    while (nt < P && nt < RANKMAX) nt <<= 1;
    hipLaunchKernelGGL(ga_migrate_apply_kernel, dim3(1, K), dim3(nt < 256 ? 256 : nt), 0, st, (float*)nullptr, fits, P,
                       0, m, elite_k, mig, elite, m, (float*)nullptr, refit);
    return hipGetLastError();
}

int ga_max_population() { return SMAX; }
#if GGS_VTIMING
extern "C" int ggs_debug_vtiming_read(void* host, size_t bytes) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_ggs_vtiming), bytes, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}
#endif
int ga_breed_max_population() { return RANKMAX; }

// ---------------------------------------------------------------------------
// stage export (ggs_ga_philox_draws): the Philox-mode draws as explicit arrays
// ---------------------------------------------------------------------------
// What the variation kernels draw in Philox mode for generation `gen` (SA:
// iteration), offspring first .. first+n_off-1 (SA: tries), written in the
// explicit-draw layout (GaDrawsDev), every slot filled whether or not a kernel
// would consume it.  The per-splat and per-offspring draws come from the helpers
// the kernels call (mask_draws, normal_draws, fallbacks with no flag set, u01,
// rng.block); the expressions ga_variation_body writes inline (crossover
// decision and mask uniform, tournament index, swap_i, swap_u) are restated.
// `first` moves only the offspring identity og (S_MASK, S_NORM_*, S_IND): pairs
// and tournament slots are counted from the launch's offspring 0, as the
// kernels count them.  One thread per output element of the largest array.
__global__ void __launch_bounds__(256)
ga_philox_draws_kernel(uint32_t k0, uint32_t k1, int gen, int first, int n_off, int P, int N, int tour_k, float cxpb,
                       GaDrawsOut out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const Rng rng{k0, k1, (uint32_t)gen};
    const GaDrawsDev d{};
    const int npairs = (n_off + 1) / 2;
    if (t < (int64_t)n_off * N) {              // per offspring and splat: mask uniforms, normals
        const int o = (int)(t / N), s = (int)(t % N);
        const uint32_t og = (uint32_t)(o + first);
        const MaskU u = mask_draws(d, rng, og, 0, s);
        const NormD n = normal_draws(d, rng, og, 0, s, N);
        out.u_xy[t * 2] = u.ux0; out.u_xy[t * 2 + 1] = u.ux1;
        out.u_ab[t * 2] = u.ua0; out.u_ab[t * 2 + 1] = u.ua1;
        out.u_t[t] = u.ut; out.u_rgb[t] = u.urgb; out.u_a[t] = u.ua;
        out.n_xy[t * 2] = n.nx0; out.n_xy[t * 2 + 1] = n.nx1;
        out.n_ab[t * 2] = n.na0; out.n_ab[t * 2 + 1] = n.na1;
        out.n_t[t] = n.nt;
        out.n_rgba[t * 4] = n.nr0; out.n_rgba[t * 4 + 1] = n.nr1;
        out.n_rgba[t * 4 + 2] = n.nr2; out.n_rgba[t * 4 + 3] = n.nr3;
    }
    if (t < (int64_t)npairs * N) {             // crossover mask uniform of (pair, splat), shared by the pair
        const int pair = (int)(t / N), s = (int)(t % N);
        out.cx_u[t] = u01(rng.block(S_CX, (uint32_t)pair, (uint32_t)(s + 1)).x);
    }
    if (t < (int64_t)P * tour_k) {             // candidate j of tournament slot q
        const int q = (int)(t / tour_k), j = (int)(t % tour_k);
        out.tour_idx[t] = min((int)(u01(rng.block(S_TOUR, (uint32_t)q, (uint32_t)j).x) * (float)P), P - 1);
    }
    if (t < P) out.perm[t] = (int)t;           // Philox mode does not shuffle
    if (t < npairs) out.cx[t] = u01(rng.block(S_CX, (uint32_t)t, 0).x) < cxpb;
    if (t < n_off) {                           // per offspring: fallbacks, swap
        const int o = (int)t;
        const uint32_t og = (uint32_t)(o + first);
        const Fallback f = fallbacks(d, rng, og, o, N, 0);
        out.k_color[o] = f.kc; out.k_xy[o] = f.kx; out.k_ab[o] = f.kb; out.k_t[o] = f.kt;
        out.swap_i[o] = N >= 2 ? (int)(rng.block(S_IND, og, 4).x % (uint32_t)(N - 1)) : 0;
        out.swap_pick[o] = -1;
        out.swap_u[o] = (double)u01(rng.block(S_IND, og, 5).x);
    }
}

hipError_t launch_ga_philox_draws(hipStream_t st, uint64_t seed, int gen, int first, int n_off, int P, int N,
                                  int tour_k, float cxpb, const GaDrawsOut& out) {
    // the largest array: [n_off*N] (>= npairs*N, n_off, npairs) or [P*tour_k] (>= P)
    const int64_t a = (int64_t)n_off * N, b = (int64_t)P * tour_k, n = a > b ? a : b;
    hipLaunchKernelGGL(ga_philox_draws_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (uint32_t)seed,
                       (uint32_t)(seed >> 32), gen, first, n_off, P, N, tour_k, cxpb, out);
    return hipGetLastError();
}

}  // namespace ggs
