// Internal declarations shared by the kernels (*.hip) and the host layer (ggs_host.h, ggs_capi.cpp, ggs_sess_*.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ggs.h"

// Diagnostic knobs (per-wave clocks, a plan-less traffic probe that computes the
// wrong fitness, saturation / cull / chunk overrides) compile only into the probe
// library (`make probe` -> libggs_probe.so, which ggs/_lib.py refuses unless
// GGS_PROBE=1), never into libggs.so.
#if !defined(GGS_PROBE_BUILD) &&                                                         \
    (defined(GGS_NOPLAN) || defined(GGS_TIMING) || defined(GGS_VTIMING) || defined(GGS_SATURATE) || \
     defined(GGS_SAT_EVERY) || defined(GGS_SAT_BATCH) || defined(GGS_SAT_AHEAD) ||             \
     defined(GGS_CULL_AHEAD) || defined(GGS_CHUNK_MB) || defined(GGS_NO_RATIO_CLAMP) ||               \
     defined(GGS_DEPTH_SPLIT) || defined(GGS_TILE_H))
#error "GGS_* diagnostic knobs are for the probe build only: make probe PROBE=\"-D...\""
#endif
#ifdef GGS_PROBE_BUILD
#define GGS_BUILD_KIND "probe"
#else
#define GGS_BUILD_KIND "product"
#endif

namespace ggs {

// One preprocessed splat as the raster kernel consumes it (64 B, HBM + LDS).
// cx, cy: centre in pixels (render.py:15-16); A, Bc, Cc, la: exp2-domain
// coefficients of the Gaussian (render.py:189-192 folded with log2(a));
// r, g, b: colour in [0,1] (render.py:40-42); x0..y1: inclusive integer AABB
// (render.py:27-30).
struct __attribute__((aligned(16))) SplatRec {
    // C64, r, g, b and rho sit in EVEN dwords: a 16-dword s_load lands them in
    // even SGPRs, the low half of an aligned SGPR pair, which the raster's v_pk_*
    // ops broadcast to both halves (op_sel_hi) with no per-visit copy (round 3:
    // raster -2.8 % vs odd dwords, which the compiler copied into even SGPRs).
    // (A, B8) is one aligned pair: one v_pk_mul forms (A qx, 8 Bc qx) per visit.
    // The raster works with qy / 8 (cy8): C64 = 64 Cc, B8 = 8 Bc and c128 = 128 Cc
    // are the exponent's y-terms rescaled by powers of two (exact), so the
    // recurrence ratio needs no separate 8 * bx (see make_rec).
    float C64, cx, r, cy8;
    float g, la, b, c128;
    float rho, rho4, A, B8;    // row-recurrence constants: 2^(128 Cc), 2^(64 Cc) (8-row step)
    int x0, x1, y0, y1;
};
static_assert(sizeof(SplatRec) == 64, "SplatRec must be 64 bytes");

// live (device, may be null): only the first *live candidates of N splats each are
// live (the device SA loop sizes its grids for the session's capacity and sets the
// round's neighbour count on the device); the other threads / waves exit at once.
// recs [S] and bnds [S] (the records' AABBs, compact for the raster's cull) go together.
// Strip words (optional): with both buffers set, N splats per candidate (S = B * N)
// and strip_words_ok(N), prep also makes the raster's integer cull tests, once per
// candidate (words [B][nTY][N], masks: see prep_strip_words), and a launch_raster of
// the same batch that is handed the same buffers only compacts its strip lists from
// them: the same lists, so the same bits.  Anything else (null buffers, other N, a
// live count, dirty strips, the saturation and folded-finalize instances) culls
// from bnds as before.
struct StripWords {
    int* words = nullptr;         // strip_words_bytes
    uint64_t* masks = nullptr;    // strip_masks_bytes
    const int* table = nullptr;   // the canvas's strip table (strip_table_entry per dispatch group)
};

// ---- the strip-words raster's launch descriptor ---------------------------------
// Every strip wave of a launch used to derive its (candidate, strip) from the
// block index with three runtime divisions and a chain of argument loads, on
// identical inputs.  The host does that once per launch: the divisions become
// multiply-shifts by constants it builds, and the dispatch-order table carries
// the decoded strip.
//
// n / d == ((uint64_t)n * mul) >> shift for every n <= the nmax it was built for.
struct GridDiv {
    uint32_t mul = 0, shift = 0;   // (0, 0): the quotient 0
};
__host__ __device__ inline uint32_t grid_div(uint32_t n, GridDiv g) {
    return (uint32_t)(((uint64_t)n * g.mul) >> g.shift);
}
// Round-up magic: mul = ceil(2^k / d) at the smallest k whose error e = mul * d - 2^k
// satisfies e * nmax < 2^k.  (mul n / 2^k = n / d + e n / (d 2^k): the floor is that
// of n / d while the excess stays below 1 / d, the least distance of n / d to the
// next integer.)  k = 31 + ceil(log2 d) always does for nmax < 2^31, with mul < 2^32.
// False: no 32-bit constant is exact up to nmax (or d == 0).
inline bool grid_div_make(uint32_t d, uint32_t nmax, GridDiv* out) {
    if (d == 0) return false;
    for (uint32_t k = 0; k < 64; ++k) {
        const uint64_t p = (uint64_t)1 << k;
        const uint64_t m = p / d + (p % d != 0);
        if (m >> 32) break;
        const uint64_t e = m * d - p;                 // < d: e * nmax fits 64 bits
        if (e * (uint64_t)nmax < p) {
            out->mul = (uint32_t)m;
            out->shift = k;
            return true;
        }
    }
    return false;
}
// One entry of the strip table: dispatch group grp (raster_tile_order's numbering,
// tile * 4 + strip of the tile) as the strip's column index over the canvas,
// tx * 4 + strip (bits 0-15; its low two bits are the strip of the tile) and the
// row tile ty (bits 16-30).  False: the canvas has more strips than the fields hold.
constexpr int kStripsPerTile = 4;
inline bool strip_table_entry(int grp, int nTX, int* out) {
    const int t = grp / kStripsPerTile, s = grp % kStripsPerTile;
    const int cs = (t % nTX) * kStripsPerTile + s, ty = t / nTX;
    if (cs > 0xFFFF || ty > 0x7FFF) return false;
    *out = cs | (ty << 16);
    return true;
}
__host__ __device__ inline int strip_entry_column(int e) { return e & 0xFFFF; }   // tx * 4 + strip of the tile
__host__ __device__ inline int strip_entry_row(int e) { return e >> 16; }         // ty
// The by-value block that is raster_kernel's first argument and all that the
// strip-words instances, raster_kernel<MODE, false, false>, read (launch_raster
// fills it).  The grid decode's fields come first.
struct StripLaunch {
    const int* table = nullptr;        // strip_table_entry per dispatch group
    const uint64_t* masks = nullptr;   // StripWords
    const int* words = nullptr;
    // blocks [flip_lo, flip_lo + flip_n) run as block flip_sum - index (the single-round
    // boustrophedon; flip_n = 0: none)
    uint32_t flip_lo = 0, flip_n = 0, flip_sum = 0;
    // candidate chunks: chunk c = index / per has chunk_b candidates (the last one
    // last_b), c * chunk_b being its first; one chunk: per_div = (0, 0), c_last = 0
    uint32_t per = 0, c_last = 0, chunk_b = 0, last_b = 0;
    GridDiv per_div, chunk_div, last_div;
    int N = 0, ncols = 0;              // splats per candidate; column strips of the canvas (4 nTX)
    int ncp = 0;                       // strip_mask_chunks(N)
    int words_b = 0, masks_b = 0;      // per candidate: ints of words (nTY N), mask words ((2 ncols + nTY) ncp)
    int nslots = 0;                    // strips per candidate (4 nTiles)
    const SplatRec* recs = nullptr;
    const float4* plan = nullptr;      // MODE 1
    float* partials = nullptr;
    float* img = nullptr;              // MODE 0
    int H = 0, W = 0;
    float bg_r = 0.f, bg_g = 0.f, bg_b = 0.f;
};
// Fills the grid decode of a launch of B candidates over nTiles tiles in chunks of CH
// (raster_chunk) on a device of `simds` SIMDs.  False: some constant does not exist
// (the launch then goes to the instance that divides).
inline bool strip_launch_grid(int64_t B, int nTiles, int CH, int simds, StripLaunch* d) {
    const int64_t nG = (int64_t)nTiles * kStripsPerTile, grid = B * nG;
    if (B <= 0 || nG <= 0 || CH <= 0 || grid >= ((int64_t)1 << 31)) return false;
    d->flip_lo = d->flip_n = d->flip_sum = 0;
    if (simds > 0 && grid > 2 * (int64_t)simds && grid <= 3 * (int64_t)simds) {
        d->flip_lo = (uint32_t)simds;
        d->flip_n = (uint32_t)simds;
        d->flip_sum = 3u * (uint32_t)simds - 1u;
    }
    const bool chunks = B > CH;
    const int64_t c_last = chunks ? (B - 1) / CH : 0;
    d->per = chunks ? (uint32_t)(CH * nG) : 0u;
    d->c_last = (uint32_t)c_last;
    d->chunk_b = (uint32_t)(chunks ? CH : B);
    d->last_b = (uint32_t)(B - c_last * CH);
    d->per_div = GridDiv{};
    if (chunks && !grid_div_make(d->per, (uint32_t)(grid - 1), &d->per_div)) return false;
    // dividends: a block's index in its chunk, then (its remainder + its group), below b + nG
    const int64_t in_chunk = (chunks ? (int64_t)d->per : grid) - 1;
    const auto lim = [&](uint32_t b) {
        const int64_t x = (int64_t)b + nG - 2;
        return (uint32_t)(x > in_chunk ? x : in_chunk);
    };
    return grid_div_make(d->chunk_b, lim(d->chunk_b), &d->chunk_div) &&
           grid_div_make(d->last_b, lim(d->last_b), &d->last_div);
}
// The candidate and dispatch group of block `index` (device and host: the tests
// restate today's divisions against it).
struct StripBlock { uint32_t b, group; };
__host__ __device__ inline StripBlock strip_launch_block(const StripLaunch& d, uint32_t index) {
    if (index - d.flip_lo < d.flip_n) index = d.flip_sum - index;
    const uint32_t c = grid_div(index, d.per_div);
    index -= c * d.per;
    const bool last = c == d.c_last;
    const uint32_t nb = last ? d.last_b : d.chunk_b;
    const GridDiv dv = last ? d.last_div : d.chunk_div;
    const uint32_t gi = grid_div(index, dv);
    const uint32_t x = index - gi * nb + gi;           // (index + gi) mod nb == x mod nb
    return {c * d.chunk_b + (x - grid_div(x, dv) * nb), gi};
}
bool strip_words_ok(int N);       // N % 64 == 0 and at most the no-saturation-check limit
size_t strip_words_bytes(int64_t B, int N, int H, int W);
size_t strip_masks_bytes(int64_t B, int N, int H, int W);
hipError_t launch_prep(hipStream_t st, bool encode, const float* genomes, int64_t S, int C, int H,
                       int W, float k, SplatRec* recs, int4* bnds, float* f9, int* i4, float* enc9,
                       const int* live = nullptr, int n_per = 0, const StripWords& sw = StripWords{}, int N = 0);
int raster_tiles(int H, int W, int* nTX);
// The fitness finalize folded into the raster (MODE 1): each strip wave counts
// itself in ctr[b] after storing its partial, and the candidate's last strip
// wave reduces the candidate's partials (finalize_wave, so the same bits as
// finalize_kernel) into out[b] and resets ctr[b] to 0 for the next launch.
// ctr: one int per candidate of the launch, all zero before the first launch
// (ensure_zeroed); the counters are per workspace, so launches that may run at
// the same time (other streams) never share them.
struct FinFused {
    int* ctr = nullptr;               // null: no fusion (launch_finalize follows)
    const float* wpartials = nullptr;  // the plan's weight block
    float* out = nullptr;             // [B] fitness scalars
    double hw = 0.0;                  // H * W
    int mode = 0;                     // GGS_FIT_*
};
// simds: SIMDs of the launch's device (DevCtx::simds; 0 = unknown: no single-round
// reordering).
// group > 0: a plan set (launch_plan_set).  `plan` and fin->wpartials are those of
// plan 0 and candidate b is scored against plan b / group; fitness only (mode 1),
// without dirty / clean / live.
hipError_t launch_raster(hipStream_t st, int mode, const SplatRec* recs, const int4* bnds, int B, int N, int H, int W,
                         const float bg[3], float* img, const float4* plan, float* partials,
                         const int* tile_order, const unsigned char* dirty = nullptr,
                         const float* clean = nullptr, const int* live = nullptr, const FinFused* fin = nullptr,
                         int simds = 0, int group = 0, const StripWords& sw = StripWords{});
// SIMDs (CUs x 4) of HIP device `dev`, 0 if unknown.
int device_simds(int dev);

// Strips touched by splats that differ between the neighbours and the current
// state (old AABB from cur_recs, new from nb_recs) -> dirty [n][tiles][4] (zeroed
// first).  rule 1: a splat differs when its raster record does (nb_recs [n][N] vs
// cur_recs [N]); rule 0: when its genes do (nb [n][N][9] vs curr [N][9]).
hipError_t launch_dirty(hipStream_t st, const float* curr, const float* nb, const SplatRec* cur_recs,
                        const SplatRec* nb_recs, int n, int N, int H, int W, unsigned char* dirty,
                        unsigned* n_changed, const int* live = nullptr, int rule = 1);
// Target plan for the fitness epilogue (built once per target/mask/mode/beta).
// wblock (plan_wsum_bytes): the plan's Sum w as a double, then per-wave sums.
hipError_t launch_plan(hipStream_t st, const float* target, const float* mask, int mode, float beta,
                       int H, int W, float4* plan, float* wblock);
// K plans of one (H, W, mode, beta) in one launch: targets [K][H][W][3], masks
// [K][H][W] (or null), plans K * plan_bytes and wblocks K * plan_wsum_bytes, plan
// k at those strides (launch_plan is K = 1).
hipError_t launch_plan_set(hipStream_t st, const float* targets, const float* masks, int mode, float beta,
                           int H, int W, int K, float4* plans, float* wblocks);
size_t plan_bytes(int H, int W);
size_t plan_wsum_bytes(int H, int W);
// Tile visiting order for the raster grid: tiles sorted by distance of their
// centre from the image centre (central tiles carry the most splats; running
// them first shortens the tail of the launch).
void raster_tile_order(int H, int W, int* order);   // raster_order_len(H, W) entries
int raster_order_len(int H, int W);
hipError_t launch_detmath(hipStream_t st, const float* x, const float* y, int64_t n, int fn,
                          float* out);
hipError_t launch_finalize(hipStream_t st, const float* partials, const float* wpartials, int B,
                           int nTiles, int mode, int H, int W, float* out, const int* live = nullptr,
                           int group = 0);   // group > 0: wpartials of plan set entry b / group

// ---- the device searches' size limits (ggs_ga.hip, ggs_sa.hip, ggs_de.hip, ggs_grad.hip) --
constexpr int SMAX = 4096;     // largest pop_size (ga_max_population): a GA population, an SA session's neighbours
constexpr int RANKMAX = 512;   // counting ranks below this population size (and the fused breed's limit)

// ---- device GA (ggs_ga.hip; shared draw helpers in ggs_variation.h) -----------
struct GaParamsDev {            // one generation's operator parameters (float32 as the host path)
    float sig_xy, sig_alog, sig_blog, sig_theta, sig_rgb, sig_alpha;   // build_mut_sigma
    float mutpb, cxpb;
    int tour_k;
    int mutate_only;            // SA neighbours: every offspring = mutation of pop[0], no selection
    int o_base;                 // Philox key offset of offspring 0 (SA: index of the first try)
    float log_lo, log_hi;       // clamp_genome scale bounds (utils.py:38-39)
};
struct GaDrawsDev {             // explicit draws (device pointers); all NULL -> Philox in-kernel
    const int* tour_idx;        // [P*k]
    const int* perm;            // [P]
    const int* cx;              // [npairs]
    const float* cx_u;          // [npairs*N]
    const float *u_xy, *u_ab;   // [P*N*2]
    const float *u_t, *u_rgb, *u_a;   // [P*N]
    const int *k_color, *k_xy, *k_ab, *k_t;   // [P]
    const float *n_xy, *n_ab;   // [P*N*2]
    const float* n_t;           // [P*N]
    const float* n_rgba;        // [P*N*4]
    const int *swap_i, *swap_pick;    // [P]
    const double* swap_u;       // [P]
};
struct GaDrawsOut {             // GaDrawsDev's mutable twin (device pointers): the stage export's outputs
    int* tour_idx;              // [P*k]
    int* perm;                  // [P]
    int* cx;                    // [npairs], npairs = ceil(n_off / 2)
    float* cx_u;                // [npairs*N]
    float *u_xy, *u_ab;         // [n_off*N*2]
    float *u_t, *u_rgb, *u_a;   // [n_off*N]
    int *k_color, *k_xy, *k_ab, *k_t;   // [n_off]
    float *n_xy, *n_ab;         // [n_off*N*2]
    float* n_t;                 // [n_off*N]
    float* n_rgba;              // [n_off*N*4]
    int *swap_i, *swap_pick;    // [n_off]
    double* swap_u;             // [n_off]
};
// The draws the variation kernels take in Philox mode for generation `gen` (SA:
// iteration), offspring first .. first+n_off-1 (SA: tries), as explicit arrays
// (ggs_ga_philox_draws; one small kernel built from the kernels' own draw helpers).
hipError_t launch_ga_philox_draws(hipStream_t st, uint64_t seed, int gen, int first, int n_off, int P, int N,
                                  int tour_k, float cxpb, const GaDrawsOut& out);
struct GaBestDev {
    double* fit;
    int* src;
    int* updated;
    float* ind;                 // [N*9]
};
// ---- device SA loop (ggs_sa_run; kernels in ggs_sa.hip) ------------------------
// Tries are numbered globally, g = it * tries + k.  A round mutates the next
// `live` tries from the current state (Philox keyed by (seed, it, k), as
// ggs_sa_propose), evaluates them, and the accept kernel walks them in order
// (annealing.py:133-150): the first acceptance installs that neighbour and ends
// the round (the later tries came from the old state and are re-proposed by the
// next round); without one the round consumes all `live` tries.
struct SaLoopDev {
    int64_t pos, end;           // next try / one past the chunk's last try
    int32_t live;               // neighbours of the current round (0: chunk done)
    int32_t acc_j;              // neighbour the last round accepted (-1: none)
    int32_t new_best;           // ... and whether it became the best
    int32_t tries, first_it;    // tries per iteration; iteration of sit[0]
    int32_t cap, width;         // neighbour capacity; fixed width (0: adaptive)
    int32_t pad_;
    double acc_rate;            // EWMA of acceptances per try (ggs/annealing.py)
    double best_fit;
    double curr_fit;            // float32 energy of the current state, widened
    uint64_t evaluated, rounds, accepted;
    double width_r;             // adaptive width: a round's fixed cost / its cost per neighbour
};
// Adaptive round width: the w in [1, cap] with the least expected cost per consumed
// try.  A round of w neighbours costs ~ (r + w) neighbour-evaluations and consumes
// E(w) = (1 - (1 - p)^w) / p tries at acceptance rate p (it ends at the first
// acceptance); p -> 0: E = w, so w = cap.  Only the cost depends on w: the
// trajectory is the same at every width.
__host__ __device__ inline int sa_width_rule(double p, int cap, double r) {
    if (cap <= 1) return 1;
    if (!(p > 1e-9)) return cap;
    int best_w = 1;
    double best = 0.0, qw = 1.0;
    for (int w = 1; w <= cap; ++w) {
        qw *= 1.0 - p;
        const double cost = (r + w) * p / (1.0 - qw);
        if (w == 1 || cost < best) { best = cost; best_w = w; }
    }
    return best_w;
}
struct SaItDev {                // one iteration of the chunk
    float sig[6];               // build_mut_sigma at this iteration
    float pad_[2];
    double T;                   // temperature (annealing.py:29-44)
};
// The end of a device round (one workgroup): the neighbours' fitness from their
// strip partials (finalize_wave), the acceptance walk, the install of the
// accepted neighbour (genome; records and strip partials too when cur_recs is
// set, for the incremental path), curves[(it - first_it)*2 + {0,1}] = best,
// current after each iteration, and the next round's mask-group flags.
struct SaRoundDev {
    const float* partials;      // [cap][nslots] the round's strip partials
    const float* wpartials;     // [nslots] plan weight sums
    int nslots, mode, N;
    double hw;
    float* fits_out;            // [cap] the round's energies (kept for inspection)
    uint64_t seed;
    float mutpb;
    double* curves;
    float *curr, *best;         // [N][9] state
    const float* nb;            // [cap][N][9] the round's neighbours
    SplatRec* cur_recs;         // incremental only (else null)
    const SplatRec* nb_recs;
    float* cur_part;
    int gcap;                   // the next round's neighbour limit: the batch's launch width
};
hipError_t launch_sa_accept(hipStream_t st, SaLoopDev* sl, const SaItDev* sit, const SaRoundDev& r);
// Start a chunk: pos/end/tries/first_it and the first round's width (at most gcap).
hipError_t launch_sa_begin(hipStream_t st, SaLoopDev* sl, int64_t pos, int64_t end, int tries, int first_it,
                           int cap, int width, double width_r, int gcap);
// Mask-group flags of the chunk's n_tries tries from pos0 (state-independent):
// tflags [n_tries], zeroed here.
hipError_t launch_sa_flags(hipStream_t st, int64_t pos0, int n_tries, int tries, uint64_t seed, float mutpb, int N,
                           int* tflags);
// The round's neighbours (Philox draws; the bits of ga_variation_kernel's
// mutate-only mode) with their raster records: tflags of the chunk's tries,
// sizes [cap][N] scratch, off [cap][N][9], recs [cap][N].
hipError_t launch_sa_mutate(hipStream_t st, const SaLoopDev* sl, const SaItDev* sit, const GaParamsDev& prm,
                            uint64_t seed, int N, int cap, const int* tflags, const float* curr, float* off,
                            float* sizes, SplatRec* recs, int4* bnds, int H, int W, float k_sigma);
// The acceptance uniform of try (it, k): Philox4x32-10 keyed by seed, 53-bit double
// in [0, 1).  Host and device compute the same bits.
double sa_accept_uniform(uint64_t seed, uint32_t it, uint32_t k);

// ---- SA chain groups (ggs_sa_chains_*; kernels in ggs_sa.hip) -------------------
// K chains, each the device SA loop above with its own SaLoopDev, Philox seed,
// temperatures and (optionally) target plan.  Every array gains a leading chain
// dimension: loop state [K], iteration table [K][n_its], flags [K][n_tries],
// curves [K][n_its][2], current / best genomes [K] rows of gstride floats.  The
// round's neighbours of all chains are one raster batch, named by the compact
// candidate list: a chain at high acceptance has one live neighbour while a cold
// one has the batch width, and a chain that finished the chunk has none.
constexpr int kSaMaxChains = GGS_SA_MAX_CHAINS;
struct SaChainsDev {
    int K, n_its, n_tries, cap; // chains; iterations and tries of the chunk; neighbour capacity per chain
    int64_t gstride;            // floats between the chains' genomes (N * 9 rounded up to 4: 16-B rows)
    int64_t wstride;            // floats between the chains' plan weight blocks (0: one shared plan)
    const uint64_t* seeds;      // [K]
    int* total;                 // candidates of the round (the raster's `live`)
    int* base;                  // [K] chain k's first candidate
    int* chain;                 // [K * cap] candidate b's chain (per-target: its plan)
    int* slot;                  // [K * cap] candidate b's slot in its chain's round
};
// Start a chunk for every chain and write the first round's list.
hipError_t launch_sa_chains_begin(hipStream_t st, const SaChainsDev& g, SaLoopDev* sl, int64_t pos, int64_t end,
                                  int tries, int first_it, int width, double width_r, int gcap);
hipError_t launch_sa_chains_flags(hipStream_t st, const SaChainsDev& g, int64_t pos0, int tries, float mutpb, int N,
                                  int* tflags);
// The listed neighbours (launch_sa_mutate per candidate): off [B][N][9], sizes [B][N],
// recs / bnds [B][N], B = the launch's candidate capacity (grid size).
hipError_t launch_sa_chains_mutate(hipStream_t st, const SaChainsDev& g, const SaLoopDev* sl, const SaItDev* sit,
                                   const GaParamsDev& prm, int N, int B, const int* tflags, const float* curr,
                                   float* off, float* sizes, SplatRec* recs, int4* bnds, int H, int W,
                                   float k_sigma);
// launch_sa_accept for every chain (r: the group's base pointers; r.seed is
// replaced by the chain's), then the next round's list.
hipError_t launch_sa_chains_accept(hipStream_t st, const SaChainsDev& g, SaLoopDev* sl, const SaItDev* sit,
                                   const SaRoundDev& r);
// Replica exchange e after iteration `it` (row ii of the iteration table), in
// place; swaps [2] accumulates pairs tried / swapped.
hipError_t launch_sa_chains_exchange(hipStream_t st, const SaChainsDev& g, SaLoopDev* sl, const SaItDev* sit, int ii,
                                     int it, uint64_t xseed, int e, int N, float* curr, float* best,
                                     unsigned long long* swaps);
// The exchange uniform of pair (k, k + 1) after iteration it: accept_u's Philox
// block with what = 1.  Host and device compute the same bits.
double sa_exchange_uniform(uint64_t seed, uint32_t it, uint32_t k);
// The fitness raster of a chain group with a target per chain: candidate b < *live
// is scored against plan plan_of[b] of a plan set (unfused: partials only).
hipError_t launch_chain_strips(hipStream_t st, const SplatRec* recs, const int4* bnds, int B, int N, int H, int W,
                               const float4* plans, float* partials, const int* tile_order, const int* live,
                               const int* plan_of, int simds);

struct BreedDev {               // the fused breed (launch_ga_variation with br != null)
    const float* pop_prev;      // [P][N][9] population P_{g-1} (materialised)
    const float* fits_prev;     // [P] its fitness
    const float* off_prev;      // [P][N][9] offspring of generation g-1
    const float* off_fits;      // [P] their fitness (finalize / all-gather)
    const int* elite_prev;      // [E] rows of P_{g-1} by rank (survivors / the previous breed)
    int* elite_next;            // [E] the same for P_g (written by the stats workgroup)
    float* pop_next;            // [P][N][9] P_g, row o written by workgroup o
    float* fits_next;           // [P]
    double* curves_row;         // [3] best, mean, median of P_g
    GaBestDev best;
    int elite_k;
};
hipError_t launch_ga_variation(hipStream_t st, const float* pop, const float* fits, int P, int N,
                               const GaParamsDev& prm, const GaDrawsDev& d, uint64_t seed, int gen,
                               float* off, int n_off,    // n_off offspring (GA: P; SA: tries)
                               SplatRec* recs = nullptr, int4* bnds = nullptr, int H = 0, int W = 0,
                               float k_sigma = 3.0f,
                               const SaLoopDev* sl = nullptr, const SaItDev* sit = nullptr,
                               const BreedDev* br = nullptr);
                               // recs != null: also prep the offspring (records [n_off][N]);
                               // sl != null: SA loop round (neighbour o = try sl->pos + o, its
                               // iteration's sigmas from sit; o >= sl->live exits)
struct FitReduce {               // survivors reduces the offspring's strip partials itself
    const float* partials = nullptr; // [P][nT] (null: use off_fits)
    const float* wpartials = nullptr;
    int nT = 0, mode = 0;
    double hw = 0.0;
};
hipError_t launch_ga_survivors(hipStream_t st, const float* fits, const float* off_fits, int P,
                               int elite_k, int* src, float* new_fits, const GaBestDev& best,
                               double* curves_row, int init, const FitReduce& fr = FitReduce{},
                               int* elite_next = nullptr);   // P <= 512: rows of the output by rank, rank < E
hipError_t launch_ga_gather(hipStream_t st, const float* pop, const float* off, int P, int N,
                            const int* src, float* next, const GaBestDev& best, int init);
int ga_max_population();
int ga_breed_max_population();   // the fused breed's population limit

// ---- island groups (ggs_ga_islands_*) ------------------------------------------
// K populations of P <= ga_breed_max_population() rows in one launch: every array
// above gains a leading island dimension ([K][P][N][9], [K][P], best [K], curves
// row [K][3]), seeds [K] (device) keys island k's Philox stream, and island k
// runs exactly the single-population kernel's operations on its slices.  Only
// offspring o < Pe = P - max(1, elite_k) of an island get raster records, at
// candidate k * Pe + o of one batch (recs / bnds [K * Pe][N]); their fitness
// (BreedDev::off_fits, the survivors' off_fits) is laid out the same way, [K][Pe].
hipError_t launch_ga_variation_islands(hipStream_t st, int K, const float* pop, const float* fits, int P, int N,
                                       const GaParamsDev& prm, const uint64_t* seeds, int gen, float* off,
                                       SplatRec* recs, int4* bnds, int H, int W, float k_sigma, int elite_k,
                                       const BreedDev* br = nullptr);   // br: group base pointers
hipError_t launch_ga_survivors_islands(hipStream_t st, int K, const float* fits, const float* off_fits, int P, int N,
                                       int elite_k, int* src, float* new_fits, const GaBestDev& best,
                                       double* curves_row, int init, int* elite_next);
hipError_t launch_ga_gather_islands(hipStream_t st, int K, const float* pop, const float* off, int P, int N,
                                    int elite_k, const int* src, float* next, const GaBestDev& best, int init);
// Ring migration on the materialised state (in place): the row of fitness rank
// j < m of island (k - 1 + K) % K replaces the row of rank P - 1 - j of island k,
// all islands at once from the pre-migration state; elite [K][P] is recomputed.
// mig: [K][2 m] ints of scratch.  K >= 2, 1 <= m <= P / 2.
hipError_t launch_ga_migrate(hipStream_t st, int K, float* pop, float* fits, int P, int N, int m, int elite_k,
                             int* mig, int* elite);
// The same migration for islands with a target each, in two steps around the
// immigrants' re-evaluation: _copy moves the genomes (and stages them compactly,
// stage [K][m][N][9], immigrant j of island k at k * m + j); _install writes
// refit [K][m], their fitness against island k's target, into the rows they
// took and recomputes elite.
hipError_t launch_ga_migrate_copy(hipStream_t st, int K, float* pop, const float* fits, int P, int N, int m,
                                  int* mig, float* stage);
hipError_t launch_ga_migrate_install(hipStream_t st, int K, float* fits, int P, int m, int elite_k, const int* mig,
                                     const float* refit, int* elite);

// ---- differential evolution (ggs_de_*; kernels in ggs_de.hip) -------------------
struct DeParamsDev {
    int strategy;               // 0 rand/1, 1 best/1, 2 current-to-best/1
    int crossover;              // 0 per gene, 1 per splat
    float f_lo, f_hi, cr;
    float log_lo, log_hi;       // clamp_genome scale bounds, as GaParamsDev
};
// Trial i of generation gen from pop [P][N][9] (4 <= P <= ga_breed_max_population(),
// N >= 1): trials [P][N][9] with their raster records recs / bnds [P][N].
// best_row (device): the row of lowest fitness, written by launch_de_select.
hipError_t launch_de_variation(hipStream_t st, const float* pop, int P, int N, const DeParamsDev& prm, uint64_t seed,
                               int gen, const int* best_row, float* trials, SplatRec* recs, int4* bnds, int H, int W,
                               float k_sigma);
struct DeSelectDev {
    float* pop;                 // [P][N][9], rows replaced in place
    const float* trials;        // [P][N][9]
    const float* fits;          // [P] the population's fitness
    const float* trial_fits;    // [P]
    float* fits_next;           // [P] the new fitness vector (another buffer than fits)
    int* best_row;
    double* best_fit;
    float* best_ind;            // [N][9]
    double* curves_row;         // [3] best, mean, median
};
// One-to-one selection, best so far and the curves row.  init: the statistics of
// the population as it is (trials, trial_fits and fits_next unused).
hipError_t launch_de_select(hipStream_t st, const DeSelectDev& d, int P, int N, int init);

// ---- target preparation and importance mask (ggs_mask.hip) ---------------------
// K images [K][H0][W0][3] -> targets [K][H][W][3] (prepare_target) and, with prm,
// masks [K][H][W] (compute_importance_mask of each prepared target), enqueued on
// st with no host synchronisation.  ws: targets_prepare_ws_bytes of scratch that
// stays valid until the work has run.  The arguments are validated by the caller.
constexpr int kMaxQuantiles = 8;
size_t targets_prepare_ws_bytes(int K, int H, int W, bool masks);
hipError_t launch_targets_prepare(hipStream_t st, const float* imgs, int K, int H0, int W0, int H, int W,
                                  const ggs_mask_params* prm, float* targets, float* masks, void* ws);
// numpy's 'linear' quantiles q [nq] (host array, nq <= kMaxQuantiles) of each of A
// arrays of n floats at x + a * n, by exact radix select -> d_out [A][nq] float32.
size_t quantile_ws_bytes(int A, int nq);
hipError_t launch_quantiles(hipStream_t st, const float* x, int A, int64_t n, const double* q, int nq, void* ws,
                            float* d_out);

// ---- fitness gradients and the Adam refiner (ggs_grad.hip) -----------------------
// d fitness / d genome [B][N][9].  f9 / i4: launch_prep's stage outputs of the whole
// batch (S = B * N columns); the call handles candidates b0 .. b0+nb-1 of it, with
// partials of nb * grad_partial_bytes (one wave per candidate and 16 x 32 pixel
// strip writes nine sums per splat it visits, padded to 48 B).  target [H][W][3]
// and mask [H][W] (or null) as the caller passed them; wblock: the target plan's
// weight block (launch_plan), whose leading double is the mode's Sum w.
int grad_strips(int H, int W, int* nSX);
size_t grad_partial_bytes(int N, int H, int W);
hipError_t launch_grad(hipStream_t st, const float* genomes, int C, const float* f9, const int* i4, int64_t B,
                       int64_t b0, int nb, int N, int H, int W, const float* target, const float* mask, int mode,
                       float beta, const float* wblock, void* partials, float* grad);
// A target per candidate: candidate b of the batch against image b / group of
// targets [K][H][W][3] / masks [K][H][W] (or null), wblocks the plan set's weight
// blocks wstride floats apart.  The rest as launch_grad, whose bits a candidate gets.
hipError_t launch_grad_set(hipStream_t st, const float* genomes, int C, const float* f9, const int* i4, int64_t B,
                           int64_t b0, int nb, int N, int H, int W, const float* targets, const float* masks,
                           int mode, float beta, const float* wblocks, int64_t wstride, int group, void* partials,
                           float* grad);
// The renderer's vector-Jacobian product: grad [B][N][9] = sum over pixels
// of cot [B][H][W][3] . d image / d rows, the rows in `layout` (GGS_LAYOUT_*), against
// the background bg (host).  f9 / i4, the candidates b0 .. b0+nb-1 and the partials as
// launch_grad.
hipError_t launch_render_vjp(hipStream_t st, int layout, const float* genomes, int C, const float* f9, const int* i4,
                             int64_t B, int64_t b0, int nb, int N, int H, int W, const float* cot, const float bg[3],
                             void* partials, float* grad);
// Memetic generations (ggs_ga_islands_set_polish): island k's R best-ranked rows
// staged as refine candidates k * R + j (x, best_x, best_fit = +inf, rows), and
// their refined best installed where strictly lower, the elite lists re-ranked and
// the islands' best so far updated.  P <= polish_max_population().
int polish_max_population();
hipError_t launch_polish_stage(hipStream_t st, int K, const float* pop, const float* fits, int P, int N, int R,
                               int* rows, float* x, float* best_x, double* best_fit);
hipError_t launch_polish_install(hipStream_t st, int K, float* pop, float* fits, int P, int N, int R, int elite_k,
                                 const int* rows, const float* best_x, const double* best_fit, int* elite,
                                 double* gbest_fit, float* gbest_ind);
struct RefineStepDev {          // one Adam step's constants (ggs/refine.py adam_step)
    float lr[9];
    float beta1, beta2, eps;
    float c1, c2;               // 1 - beta1^t, 1 - beta2^t: float64 on the host, rounded once
    float log_lo, log_hi;       // clamp_genome scale bounds, as GaParamsDev
};
// x [B][N][9] becomes best_x / best_fit [B] where fits[b] + 1e-10 < best_fit[b] (float64).
hipError_t launch_refine_best(hipStream_t st, const float* x, const float* fits, int B, int N, double* best_fit,
                              float* best_x);
hipError_t launch_refine_adam(hipStream_t st, float* x, float* m, float* v, const float* g, int B, int N,
                              const RefineStepDev& p);

// ---- image losses (ggs_loss.hip) ---------------------------------------
// loss [B] = w[0] mean|x - y| + w[1] mean (x - y)^2 + w[2] (1 - mean SSIM) of img
// [B][H][W][3] against targets [K][H][W][3] (candidate b against image b / group) and,
// unless cot is null, cot [B][H][W][3] = d loss / d img.  partials:
// image_loss_partial_bytes of scratch.  B * image_loss_tiles must stay below 2^31.
int64_t image_loss_tiles(int H, int W);
size_t image_loss_partial_bytes(int64_t B, int H, int W);
hipError_t launch_image_loss(hipStream_t st, const float* img, int64_t B, const float* targets, int group, int H, int W,
                             const float w[3], void* partials, float* loss, float* cot);

// ---- density control of the refiner (ggs_density.hip) --------------------
// acc [B][N] += the per-pixel norm of grad [B][N][9]'s position columns.
hipError_t launch_density_acc(hipStream_t st, const float* grad, float* acc, int B, int N, int H, int W);
// One event on x, m, v [B][N][9]: counts [B][2] zeroed, rank, apply.  M = the
// effective max_moves (<= N / 2; 0: nothing is launched); dead_list / src_list
// [B][M], pairs [B][M][2], is_split [B][M], last_n [B]; moves / splits [B] cumulative,
// may be null.  B <= 65535 (the rank kernel's grid is (ceil(N / 256), B)).
hipError_t launch_density_event(hipStream_t st, float* x, float* m, float* v, const float* acc, int n_acc, int B, int N,
                                int H, int W, float log_lo, float log_hi, const ggs_refine_density& d, int M,
                                int* dead_list, int* src_list, int* counts, int* pairs, int* is_split, int* last_n,
                                unsigned long long* moves, unsigned long long* splits);

// ---- residual-driven placement (ggs_seed.hip) ---------------------------
inline int seed_cells(int H, int W, int cell) { return ((H + cell - 1) / cell) * ((W + cell - 1) / cell); }
// bytes of launch_seed_sites's scratch (own_err: the error grid is not the caller's)
size_t seed_scratch_bytes(int B, int H, int W, int cell, int M, bool own_err);
// One placement: cell, rank (its counters zeroed first) and apply on `st`.  img [B][H][W][3]
// or null (the constant bg), targets [K][H][W][3], weights [K][H][W] or null, candidate b
// against image b / group; rows [B][M] or null (prm.first_row + j); x [B][N][9] or null
// (sites only); err [B][G] or null (kept in the scratch); sites [B][M], n_out [B];
// M = prm.max_sites.  B <= 65535 (the rank kernel's grid is (ceil(G / 256), B)).
hipError_t launch_seed_sites(hipStream_t st, const float* img, const float bg[3], const float* targets,
                             const float* weights, int B, int group, int H, int W, const ggs_seed_params& prm,
                             const int* rows, float* x, int N, void* scratch, float* err, int* sites, int* n_out);

// ---- RCCL (ggs_comm.cpp) ----------------------------------------------------
// Grouped in-place all-gather over single-process communicators (ggs_comm_init_local):
// buf[d] holds shard d at buf[d] + d*per; afterwards every buf[d] holds all n shards.
int comm_group_allgather_inplace(void* const* comms, int n, hipStream_t const* streams, float* const* bufs,
                                 int64_t per);

}  // namespace ggs
