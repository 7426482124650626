// Device-resident simulated annealing: the round kernels of the lone loop
// (ggs_sa_run) and of chain groups (ggs_sa_chains_*), and replica exchange.
// Sessions in ggs_sess_sa.cpp.
#include "ggs_prep.h"
#include "ggs_variation.h"

namespace ggs {

double sa_accept_uniform(uint64_t seed, uint32_t it, uint32_t k) { return accept_u(seed, it, k); }
double sa_exchange_uniform(uint64_t seed, uint32_t it, uint32_t k) { return exchange_u(seed, it, k); }

// ---------------------------------------------------------------------------
// device SA loop (ggs_sa_run): chunk start, and one round's acceptance walk
// ---------------------------------------------------------------------------
// Round width: the host loop's rule (ggs/annealing.py) without its iteration
// boundary — 1/acceptance rate, or the capacity while acceptances are rarer than that.
// gcap: the width of the batch of rounds the host enqueued (their launch width,
// <= cap): the host applies sa_width_rule at each sync, so every launched
// neighbour slot is used (an unused slot's early-exit strip waves are not free)
__device__ __forceinline__ int sa_width(const SaLoopDev& s, int gcap) {
    int w = gcap > 0 ? gcap : s.width;
    if (w <= 0) w = sa_width_rule(s.acc_rate, s.cap, s.width_r);
    w = min(w, s.cap);
    return (int)min((int64_t)w, max(s.end - s.pos, (int64_t)0));
}

// The round's neighbours, spread over the GPU: ga_variation_kernel gives each
// neighbour one workgroup, so a round of a few 4,096-splat neighbours ran on a
// few CUs (40 us + a 5-us prep launch).  Here three kernels of one workgroup per
// (neighbour, 256 splats) — flags, mutate + prep, swap — do the same per-splat
// work with the same helpers (the same bits as ggs_sa_propose's variation).
constexpr int SA_VT = 256;

struct SaTry {                  // neighbour o of the round -> its Philox identity and sigmas
    uint32_t og;
    int gen;
};
__device__ __forceinline__ SaTry sa_try(const SaLoopDev& s, const SaItDev* sit, int o, GaParamsDev& prm) {
    const int64_t g = s.pos + o;
    const int it = (int)(g / s.tries);
    const SaItDev& q = sit[it - s.first_it];
    prm.sig_xy = q.sig[0]; prm.sig_alog = q.sig[1]; prm.sig_blog = q.sig[2];
    prm.sig_theta = q.sig[3]; prm.sig_rgb = q.sig[4]; prm.sig_alpha = q.sig[5];
    return {(uint32_t)(g % s.tries), it};
}

// pass 1, for every try of the chunk at once (the mask uniforms do not depend on
// the state, so a try re-proposed after an acceptance keeps its flags): any() of
// each mask group over try t's splats -> tflags[t] (OR; zeroed by the caller)
__device__ __forceinline__ void
sa_flags_body(int64_t pos0, int tries, uint32_t k0, uint32_t k1, float mutpb, int N, int nch,
              int* __restrict__ tflags) {
    const int t = blockIdx.x / nch, s = (blockIdx.x % nch) * SA_VT + threadIdx.x;
    const int64_t g = pos0 + t;
    const Rng rng{k0, k1, (uint32_t)(g / tries)};
    const int any = s < N ? mask_any(mask_draws(GaDrawsDev{}, rng, (uint32_t)(g % tries), 0, s), mutpb) : 0;
    const int wave_any = (__ballot(any & ANY_COLOR) ? ANY_COLOR : 0) | (__ballot(any & ANY_XY) ? ANY_XY : 0) |
                         (__ballot(any & ANY_AB) ? ANY_AB : 0) | (__ballot(any & ANY_T) ? ANY_T : 0);
    if ((threadIdx.x & 63) == 0 && wave_any) atomicOr(&tflags[t], wave_any);
}
__global__ void __launch_bounds__(SA_VT)
sa_flags_kernel(int64_t pos0, int tries, uint32_t k0, uint32_t k1, float mutpb, int N, int nch,
                int* __restrict__ tflags) {
    sa_flags_body(pos0, tries, k0, k1, mutpb, N, nch, tflags);
}

hipError_t launch_sa_flags(hipStream_t st, int64_t pos0, int n_tries, int tries, uint64_t seed, float mutpb, int N,
                           int* tflags) {
    const int nch = (N + SA_VT - 1) / SA_VT;
    hipError_t e = hipMemsetAsync(tflags, 0, sizeof(int) * (size_t)n_tries, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sa_flags_kernel, dim3((unsigned)((int64_t)n_tries * nch)), dim3(SA_VT), 0, st, pos0, tries,
                       (uint32_t)seed, (uint32_t)(seed >> 32), mutpb, N, nch, tflags);
    return hipGetLastError();
}

// pass 2: mutate each splat of the current state into neighbour o, its raster
// record, and its size exp(a)exp(b) for the swap
// (o: the neighbour's slot in its chain's round; ob: its candidate in the launch,
// where its genome, sizes and records go.  A lone session has ob = o.)
__device__ __forceinline__ void
sa_mutate_body(int o, int ob, int s, const SaLoopDev* __restrict__ sl, const SaItDev* __restrict__ sit,
               GaParamsDev prm, uint32_t k0, uint32_t k1, int N, const int* __restrict__ tflags,
               const float* __restrict__ curr, float* __restrict__ off, float* __restrict__ sizes,
               SplatRec* __restrict__ recs, int4* __restrict__ bnds, int H, int W, float k_sigma) {
    if (o >= sl->live || s >= N) return;
    const SaTry t = sa_try(*sl, sit, o, prm);
    const Rng rng{k0, k1, (uint32_t)t.gen};
    const GaDrawsDev d{};
    const SaLoopDev& sv = *sl;
    const Fallback fb = fallbacks(d, rng, t.og, o, N, tflags[sv.pos + o - (int64_t)sv.first_it * sv.tries]);
    const MaskU u = mask_draws(d, rng, t.og, 0, s);
    const NormD nd = normal_draws(d, rng, t.og, 0, s, N);
    float g[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) g[c] = curr[(int64_t)s * 9 + c];
    mutate_row(g, u, nd, fb, s, prm);
    const int64_t os = (int64_t)ob * N + s;
#pragma unroll
    for (int c = 0; c < 9; ++c) off[os * 9 + c] = g[c];
    sizes[os] = expf(g[2]) * expf(g[3]);
    float row[9];
    encode_row(g, row);
    const SplatRec r = make_rec(preprocess_row(row, H, W, k_sigma));
    recs[os] = r;
    bnds[os] = rec_bounds(r);
}
__global__ void __launch_bounds__(SA_VT)
sa_mutate_kernel(const SaLoopDev* __restrict__ sl, const SaItDev* __restrict__ sit, GaParamsDev prm, uint32_t k0,
                 uint32_t k1, int N, int nch, const int* __restrict__ tflags, const float* __restrict__ curr,
                 float* __restrict__ off, float* __restrict__ sizes, SplatRec* __restrict__ recs,
                 int4* __restrict__ bnds, int H, int W, float k_sigma) {
    const int o = blockIdx.x / nch, s = (blockIdx.x % nch) * SA_VT + threadIdx.x;
    sa_mutate_body(o, o, s, sl, sit, prm, k0, k1, N, tflags, curr, off, sizes, recs, bnds, H, W, k_sigma);
}

// genetic.py:79-91 on neighbour o: the pick-th later splat bigger than a random
// splat i trades rows (and raster records) with it.  Thread t owns the contiguous
// run of splats [t*per, (t+1)*per) (splat order = thread order), counts its
// candidates in one read of the sizes, one workgroup scan of the counts gives the
// total (-> pick) and each run's rank offset, and the thread whose run holds the
// pick walks its run again to name j.  Two barriers (the first version counted,
// then walked the sizes in 1024-splat chunks with three barriers per chunk: 8.4 us
// per round at 4,096 splats).
constexpr int SW_THREADS = 1024;
__device__ __forceinline__ void
sa_swap_body(int o, int ob, const SaLoopDev* __restrict__ sl, uint32_t k0, uint32_t k1, int N,
             const float* __restrict__ sizes, float* __restrict__ off, SplatRec* __restrict__ recs,
             int4* __restrict__ bnds) {
    __shared__ int s_wsum[SW_THREADS / 64], s_j;
    const int tid = threadIdx.x;
    const SaLoopDev& sv = *sl;
    if (o >= sv.live || N < 2) return;
    const int64_t g = sv.pos + o;
    const uint32_t og = (uint32_t)(g % sv.tries);
    const Rng rng{k0, k1, (uint32_t)(g / sv.tries)};
    const float* __restrict__ sz = sizes + (int64_t)ob * N;
    const int i = (int)(rng.block(S_IND, og, 4).x % (uint32_t)(N - 1));
    const float sizei = sz[i];
    const int lane = tid & 63, w = tid >> 6;
    const int per = (N + SW_THREADS - 1) / SW_THREADS;
    const int r0 = min(tid * per, N), r1 = min(r0 + per, N);
    int cnt = 0;
    for (int sk = max(r0, i + 1); sk < r1; ++sk) cnt += sz[sk] > sizei;
    int v = cnt;                                       // inclusive wave scan
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    if (lane == 63) s_wsum[w] = v;
    if (tid == 0) s_j = -1;
    __syncthreads();
    int before = v - cnt, count = 0;
#pragma unroll
    for (int q = 0; q < SW_THREADS / 64; ++q) {
        const int t = s_wsum[q];
        before += q < w ? t : 0;
        count += t;
    }
    if (count == 0) return;                            // (uniform)
    int pick = (int)((double)u01(rng.block(S_IND, og, 5).x) * (double)count);
    if (pick > count - 1) pick = count - 1;
    if (pick >= before && pick < before + cnt) {       // this run holds the (pick+1)-th candidate
        int left = pick - before;
        for (int sk = max(r0, i + 1); sk < r1; ++sk)
            if (sz[sk] > sizei && left-- == 0) {
                s_j = sk;
                break;
            }
    }
    __syncthreads();
    const int j = s_j;
    float* __restrict__ O = off + (int64_t)ob * N * 9;
    if (tid < 9) {
        const float a = O[(int64_t)i * 9 + tid], b = O[(int64_t)j * 9 + tid];
        O[(int64_t)i * 9 + tid] = b;
        O[(int64_t)j * 9 + tid] = a;
    } else if (tid >= 64 && tid < 64 + 4) {           // a record is a function of its row alone
        float4* ri = reinterpret_cast<float4*>(recs + (int64_t)ob * N + i) + (tid - 64);
        float4* rj = reinterpret_cast<float4*>(recs + (int64_t)ob * N + j) + (tid - 64);
        const float4 a = *ri, b = *rj;
        *ri = b;
        *rj = a;
    } else if (tid == 128) {
        int4* bi = bnds + (int64_t)ob * N + i;
        int4* bj = bnds + (int64_t)ob * N + j;
        const int4 a = *bi, b = *bj;
        *bi = b;
        *bj = a;
    }
}
__global__ void __launch_bounds__(SW_THREADS)
sa_swap_kernel(const SaLoopDev* __restrict__ sl, uint32_t k0, uint32_t k1, int N, const float* __restrict__ sizes,
               float* __restrict__ off, SplatRec* __restrict__ recs, int4* __restrict__ bnds) {
    sa_swap_body(blockIdx.x, blockIdx.x, sl, k0, k1, N, sizes, off, recs, bnds);
}

hipError_t launch_sa_mutate(hipStream_t st, const SaLoopDev* sl, const SaItDev* sit, const GaParamsDev& prm,
                            uint64_t seed, int N, int cap, const int* tflags, const float* curr, float* off,
                            float* sizes, SplatRec* recs, int4* bnds, int H, int W, float k_sigma) {
    const int nch = (N + SA_VT - 1) / SA_VT;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    hipLaunchKernelGGL(sa_mutate_kernel, dim3(cap * nch), dim3(SA_VT), 0, st, sl, sit, prm, k0, k1, N, nch, tflags,
                       curr, off, sizes, recs, bnds, H, W, k_sigma);
    hipLaunchKernelGGL(sa_swap_kernel, dim3(cap), dim3(SW_THREADS), 0, st, sl, k0, k1, N, sizes, off, recs, bnds);
    return hipGetLastError();
}

__global__ void sa_begin_kernel(SaLoopDev* sl, int64_t pos, int64_t end, int tries, int first_it, int cap,
                                int width, double width_r, int gcap) {
    SaLoopDev s = *sl;
    s.pos = pos;
    s.end = end;
    s.tries = tries;
    s.first_it = first_it;
    s.cap = cap;
    s.width = width;
    s.width_r = width_r;
    s.acc_j = -1;
    s.new_best = 0;
    s.live = sa_width(s, gcap);
    *sl = s;
}

// The end of a round, one workgroup: the neighbours' fitness (finalize_wave, the
// bits of finalize_kernel), then annealing.py:130-150 over them in try order by
// one thread, then the workgroup installs the accepted neighbour.  Same arithmetic as the
// host loop (ggs/annealing.py): dE in float64 from the float32 energies, the
// Metropolis test u < exp(-dE/T) (device exp; the host's math.exp agrees to the
// last ulp in all but rare cases, and u would have to fall between the two),
// the 1e-12 best margin.
// (cb: the launch candidate of the round's neighbour 0 — 0 for a lone session, the
// chain's base in the compact list for a chain group)
__device__ __forceinline__ void
sa_accept_body(SaLoopDev* __restrict__ sl, const SaItDev* __restrict__ sit, SaRoundDev r, int cb) {
    __shared__ int s_j, s_nb;
    __shared__ float fits[SMAX];
    const int N = r.N;
    {
        const int live = sl->live, nw = blockDim.x >> 6;
        for (int b = threadIdx.x >> 6; b < live; b += nw) {
            const float v = finalize_wave(r.partials, r.wpartials, r.nslots, r.mode, r.hw, cb + b);
            if ((threadIdx.x & 63) == 0) {
                fits[b] = v;
                r.fits_out[cb + b] = v;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint64_t seed = r.seed;
        double* __restrict__ curves = r.curves;
        SaLoopDev s = *sl;
        int jacc = -1, nbest = 0;
        if (s.live > 0) {
            int used = s.live;
            for (int j = 0; j < s.live; ++j) {
                const int64_t g = s.pos + j;
                const int it = (int)(g / s.tries), k = (int)(g % s.tries);
                const double T = sit[it - s.first_it].T;
                const double e_new = (double)fits[j];
                const double dE = e_new - s.curr_fit;                       // annealing.py:133
                bool acc = dE <= 0.0;
                if (!acc && T > 0.0) acc = accept_u(seed, (uint32_t)it, (uint32_t)k) < exp(-dE / T);
                s.acc_rate = 0.9 * s.acc_rate + 0.1 * (acc ? 1.0 : 0.0);
                if (acc) s.curr_fit = e_new;
                const bool nbst = s.curr_fit + 1e-12 < s.best_fit;            // annealing.py:148-150
                if (nbst) s.best_fit = s.curr_fit;
                if (k == s.tries - 1) {                                     // end of iteration `it`
                    curves[2 * (int64_t)(it - s.first_it)] = s.best_fit;
                    curves[2 * (int64_t)(it - s.first_it) + 1] = s.curr_fit;
                }
                if (acc) {          // the later tries were mutated from the old state
                    jacc = j;
                    nbest = nbst;
                    used = j + 1;
                    s.accepted += 1;
                    break;
                }
            }
            s.evaluated += (uint64_t)s.live;
            s.rounds += 1;
            s.pos += used;
        }
        s.acc_j = jacc;
        s.new_best = nbest;
        s.live = sa_width(s, r.gcap);
        *sl = s;
        s_j = jacc;
        s_nb = nbest;
    }
    __syncthreads();
    const int j = s_j;
    if (j < 0) return;
    float* __restrict__ curr = r.curr;
    float* __restrict__ best = r.best;
    // install: 16-B copies (the genome is 36 N bytes: N % 4 floats of tail)
    const int64_t n9 = (int64_t)N * 9, n4 = n9 >> 2;
    const float* __restrict__ src = r.nb + (cb + j) * n9;
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src);
    float4* __restrict__ c4 = reinterpret_cast<float4*>(curr);
    float4* __restrict__ b4 = reinterpret_cast<float4*>(best);
    const bool nbst = s_nb;
    if ((((cb + j) * n9) & 3) == 0) {
        // distinct buffers (restrict): the unrolled loads go out together instead of
        // one load-store round trip per iteration
#pragma unroll 8
        for (int64_t i = threadIdx.x; i < n4; i += blockDim.x) {
            const float4 v = s4[i];
            c4[i] = v;
            if (nbst) b4[i] = v;
        }
        for (int64_t i = 4 * n4 + threadIdx.x; i < n9; i += blockDim.x) {
            curr[i] = src[i];
            if (nbst) best[i] = src[i];
        }
    } else {
        for (int64_t i = threadIdx.x; i < n9; i += blockDim.x) {
            const float v = src[i];
            curr[i] = v;
            if (nbst) best[i] = v;
        }
    }
    if (r.cur_recs) {       // incremental evaluation keeps the state's records and partials
        const float4* rs = reinterpret_cast<const float4*>(r.nb_recs + (cb + j) * (int64_t)N);
        float4* rd = reinterpret_cast<float4*>(r.cur_recs);
        for (int64_t i = threadIdx.x; i < 4 * (int64_t)N; i += blockDim.x) rd[i] = rs[i];
        for (int i = threadIdx.x; i < r.nslots; i += blockDim.x)
            r.cur_part[i] = r.partials[(int64_t)(cb + j) * r.nslots + i];
    }
}
__global__ void __launch_bounds__(1024)
sa_accept_kernel(SaLoopDev* __restrict__ sl, const SaItDev* __restrict__ sit, SaRoundDev r) {
    sa_accept_body(sl, sit, r, 0);
}

hipError_t launch_sa_begin(hipStream_t st, SaLoopDev* sl, int64_t pos, int64_t end, int tries, int first_it,
                           int cap, int width, double width_r, int gcap) {
    hipLaunchKernelGGL(sa_begin_kernel, dim3(1), dim3(1), 0, st, sl, pos, end, tries, first_it, cap, width,
                       width_r, gcap);
    return hipGetLastError();
}

hipError_t launch_sa_accept(hipStream_t st, SaLoopDev* sl, const SaItDev* sit, const SaRoundDev& r) {
    hipLaunchKernelGGL(sa_accept_kernel, dim3(1), dim3(1024), 0, st, sl, sit, r);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// SA chain groups (ggs_sa_chains_*): K chains' rounds in one set of launches
// ---------------------------------------------------------------------------
// Every pointer is the group's base; chain k's slice starts k strides in (its
// SaLoopDev, its rows of the iteration table and of the flags, its genomes, its
// curves).  The chains run out of step, so a round's neighbours are named by the
// compact candidate list (SaChainsDev): candidate b is slot `slot[b]` of chain
// `chain[b]`, chain k's candidates are base[k] .. base[k] + live_k - 1, and the
// grids past `total` exit at once.  The per-try and per-splat work is the lone
// session's (sa_*_body), so chain k follows the session of seeds[k] bit for bit.

// the next round's list from the K live counts (one workgroup, after a barrier
// that follows the writes of sl[k].live by this workgroup, or in a launch of its own)
__device__ __forceinline__ void sa_list_build(const SaChainsDev& g, const SaLoopDev* __restrict__ sl) {
    __shared__ int s_base[kSaMaxChains + 1];
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int k = 0; k < g.K; ++k) {
            s_base[k] = acc;
            g.base[k] = acc;
            acc += sl[k].live;
        }
        s_base[g.K] = acc;
        *g.total = acc;
    }
    __syncthreads();
    for (int k = 0; k < g.K; ++k) {
        const int b0 = s_base[k], n = s_base[k + 1] - b0;
        for (int j = threadIdx.x; j < n; j += blockDim.x) {
            g.chain[b0 + j] = k;
            g.slot[b0 + j] = j;
        }
    }
}

__global__ void __launch_bounds__(256)
sa_chains_list_kernel(SaChainsDev g, const SaLoopDev* __restrict__ sl) { sa_list_build(g, sl); }

__global__ void __launch_bounds__(256)
sa_chains_begin_kernel(SaChainsDev g, SaLoopDev* sl, int64_t pos, int64_t end, int tries, int first_it, int width,
                       double width_r, int gcap) {
    for (int k = threadIdx.x; k < g.K; k += blockDim.x) {
        SaLoopDev s = sl[k];
        s.pos = pos;
        s.end = end;
        s.tries = tries;
        s.first_it = first_it;
        s.cap = g.cap;
        s.width = width;
        s.width_r = width_r;
        s.acc_j = -1;
        s.new_best = 0;
        s.live = sa_width(s, gcap);
        sl[k] = s;
    }
    __threadfence_block();
    __syncthreads();
    sa_list_build(g, sl);
}

__global__ void __launch_bounds__(SA_VT)
sa_chains_flags_kernel(SaChainsDev g, int64_t pos0, int tries, float mutpb, int N, int nch,
                       int* __restrict__ tflags) {
    const int k = blockIdx.y;
    const uint64_t seed = g.seeds[k];
    sa_flags_body(pos0, tries, (uint32_t)seed, (uint32_t)(seed >> 32), mutpb, N, nch, tflags + (int64_t)k * g.n_tries);
}

__global__ void __launch_bounds__(SA_VT)
sa_chains_mutate_kernel(SaChainsDev g, const SaLoopDev* __restrict__ sl, const SaItDev* __restrict__ sit,
                        GaParamsDev prm, int N, int nch, const int* __restrict__ tflags,
                        const float* __restrict__ curr, float* __restrict__ off, float* __restrict__ sizes,
                        SplatRec* __restrict__ recs, int4* __restrict__ bnds, int H, int W, float k_sigma) {
    const int b = blockIdx.x / nch, s = (blockIdx.x % nch) * SA_VT + threadIdx.x;
    if (b >= *g.total) return;
    const int k = g.chain[b];
    const uint64_t seed = g.seeds[k];
    sa_mutate_body(g.slot[b], b, s, sl + k, sit + (int64_t)k * g.n_its, prm, (uint32_t)seed, (uint32_t)(seed >> 32), N,
                   tflags + (int64_t)k * g.n_tries, curr + k * g.gstride, off, sizes, recs, bnds, H, W, k_sigma);
}

__global__ void __launch_bounds__(SW_THREADS)
sa_chains_swap_kernel(SaChainsDev g, const SaLoopDev* __restrict__ sl, int N, const float* __restrict__ sizes,
                      float* __restrict__ off, SplatRec* __restrict__ recs, int4* __restrict__ bnds) {
    const int b = blockIdx.x;
    if (b >= *g.total) return;          // (uniform)
    const int k = g.chain[b];
    const uint64_t seed = g.seeds[k];
    sa_swap_body(g.slot[b], b, sl + k, (uint32_t)seed, (uint32_t)(seed >> 32), N, sizes, off, recs, bnds);
}

// one workgroup per chain: its neighbours' fitness against its plan's weights,
// its acceptance walk, its install
__global__ void __launch_bounds__(1024)
sa_chains_accept_kernel(SaChainsDev g, SaLoopDev* __restrict__ sl, const SaItDev* __restrict__ sit, SaRoundDev r) {
    const int k = blockIdx.x;
    r.wpartials += k * g.wstride;
    r.seed = g.seeds[k];
    r.curves += 2 * (int64_t)k * g.n_its;
    r.curr += k * g.gstride;
    r.best += k * g.gstride;
    sa_accept_body(sl + k, sit + (int64_t)k * g.n_its, r, g.base[k]);
}

// Replica exchange number e after iteration `it` (row ii of the iteration table):
// pairs (k, k + 1), k % 2 == e % 2, all decided by one thread from the
// pre-exchange energies (annealing.replica_exchange); then the workgroup trades
// the pairs' current genomes and applies annealing.py:148-150 to both chains.
__global__ void __launch_bounds__(1024)
sa_chains_exchange_kernel(SaChainsDev g, SaLoopDev* __restrict__ sl, const SaItDev* __restrict__ sit, int ii, int it,
                          uint64_t xseed, int e, int N, float* __restrict__ curr, float* __restrict__ best,
                          unsigned long long* __restrict__ swaps) {
    __shared__ int s_swap[kSaMaxChains], s_best[kSaMaxChains];
    if (threadIdx.x == 0) {
        unsigned long long tried = 0, done = 0;
        for (int k = 0; k < g.K; ++k) s_swap[k] = s_best[k] = 0;
        for (int k = e & 1; k + 1 < g.K; k += 2) {
            const double Ta = sit[(int64_t)k * g.n_its + ii].T, Tb = sit[(int64_t)(k + 1) * g.n_its + ii].T;
            if (!(Ta > 0.0) || !(Tb > 0.0)) continue;
            const double Ea = sl[k].curr_fit, Eb = sl[k + 1].curr_fit;
            const double d = (Ea - Eb) * (1.0 / Ta - 1.0 / Tb);
            tried += 1;
            if (exchange_u(xseed, (uint32_t)it, (uint32_t)k) < exp(d)) {
                done += 1;
                s_swap[k] = 1;
                sl[k].curr_fit = Eb;
                sl[k + 1].curr_fit = Ea;
                for (int q = k; q <= k + 1; ++q)
                    if (sl[q].curr_fit + 1e-12 < sl[q].best_fit) {
                        sl[q].best_fit = sl[q].curr_fit;
                        s_best[q] = 1;
                    }
            }
        }
        swaps[0] += tried;
        swaps[1] += done;
    }
    __syncthreads();
    const int64_t n9 = (int64_t)N * 9;
    for (int k = e & 1; k + 1 < g.K; k += 2) {
        if (!s_swap[k]) continue;       // (uniform)
        float* __restrict__ a = curr + k * g.gstride;
        float* __restrict__ b = a + g.gstride;
        for (int64_t i = threadIdx.x; i < n9; i += blockDim.x) {
            const float va = a[i], vb = b[i];
            a[i] = vb;
            b[i] = va;
            if (s_best[k]) best[k * g.gstride + i] = vb;
            if (s_best[k + 1]) best[(k + 1) * g.gstride + i] = va;
        }
    }
}

hipError_t launch_sa_chains_begin(hipStream_t st, const SaChainsDev& g, SaLoopDev* sl, int64_t pos, int64_t end,
                                  int tries, int first_it, int width, double width_r, int gcap) {
    hipLaunchKernelGGL(sa_chains_begin_kernel, dim3(1), dim3(256), 0, st, g, sl, pos, end, tries, first_it, width,
                       width_r, gcap);
    return hipGetLastError();
}

hipError_t launch_sa_chains_flags(hipStream_t st, const SaChainsDev& g, int64_t pos0, int tries, float mutpb, int N,
                                  int* tflags) {
    const int nch = (N + SA_VT - 1) / SA_VT;
    hipError_t e = hipMemsetAsync(tflags, 0, sizeof(int) * (size_t)g.n_tries * g.K, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sa_chains_flags_kernel, dim3((unsigned)((int64_t)g.n_tries * nch), g.K), dim3(SA_VT), 0, st, g,
                       pos0, tries, mutpb, N, nch, tflags);
    return hipGetLastError();
}

hipError_t launch_sa_chains_mutate(hipStream_t st, const SaChainsDev& g, const SaLoopDev* sl, const SaItDev* sit,
                                   const GaParamsDev& prm, int N, int B, const int* tflags, const float* curr,
                                   float* off, float* sizes, SplatRec* recs, int4* bnds, int H, int W,
                                   float k_sigma) {
    const int nch = (N + SA_VT - 1) / SA_VT;
    hipLaunchKernelGGL(sa_chains_mutate_kernel, dim3(B * nch), dim3(SA_VT), 0, st, g, sl, sit, prm, N, nch, tflags,
                       curr, off, sizes, recs, bnds, H, W, k_sigma);
    hipLaunchKernelGGL(sa_chains_swap_kernel, dim3(B), dim3(SW_THREADS), 0, st, g, sl, N, sizes, off, recs, bnds);
    return hipGetLastError();
}

hipError_t launch_sa_chains_accept(hipStream_t st, const SaChainsDev& g, SaLoopDev* sl, const SaItDev* sit,
                                   const SaRoundDev& r) {
    hipLaunchKernelGGL(sa_chains_accept_kernel, dim3(g.K), dim3(1024), 0, st, g, sl, sit, r);
    hipLaunchKernelGGL(sa_chains_list_kernel, dim3(1), dim3(256), 0, st, g, sl);
    return hipGetLastError();
}

hipError_t launch_sa_chains_exchange(hipStream_t st, const SaChainsDev& g, SaLoopDev* sl, const SaItDev* sit, int ii,
                                     int it, uint64_t xseed, int e, int N, float* curr, float* best,
                                     unsigned long long* swaps) {
    hipLaunchKernelGGL(sa_chains_exchange_kernel, dim3(1), dim3(1024), 0, st, g, sl, sit, ii, it, xseed, e, N, curr,
                       best, swaps);
    return hipGetLastError();
}

}  // namespace ggs
