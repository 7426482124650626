/*
 * ggs.h — C ABI of libggs.so, the MI355X (gfx950) 2D Gaussian-splat renderer and
 * fitness evaluator.  Plain pointers and sizes only; no torch/HIP types in any
 * signature (device streams are passed as void*).
 *
 * It is the drop-in boundary for the reference's hot path
 * (josedelrey/genetic-gaussian-splats):
 *
 *   ggs_render          <- modules/render.py:203-252  render_splats_rgb_triton
 *                          (with render.py:8-47 _preprocess_genome,
 *                           render.py:50-118 _gpu_bin_splats_to_tiles,
 *                           render.py:121-200 _render_tile_over_kernel)
 *   ggs_fitness         <- modules/fitness.py:7-31  fitness_many
 *                          (with modules/encode.py:62-79 genome_to_renderer_batched;
 *                           fitness.py:34-47 fitness_population is a host-side loop)
 *   ggs_encode          <- modules/encode.py:27-79  genome_to_renderer(_batched)
 *   ggs_preprocess      <- modules/render.py:8-47   _preprocess_genome
 *   ggs_*_device        the same two operations on caller-owned device memory
 *                        (inputs already resident in HBM, caller's HIP stream)
 *
 * Genome layouts (row-major float32, C >= 9 columns per splat, extra columns
 * ignored as render.py:222-223 does):
 *   axes-angle (fitness input, population.py:43):  x, y, a_log, b_log, theta, r, g, b, alpha
 *   renderer   (render input,  encode.py:37-57):   x, y, log l11, log l22, l21, r, g, b, alpha
 *
 * Ownership: all pointers are caller-owned and only used during the call (host
 * API: the call is synchronous; device API: the work is enqueued on `stream`
 * and the pointers must stay valid until it completes).  The library keeps
 * pooled device workspaces and a cache of the last target/mask uploaded per
 * device (keyed by size + a 64-bit content hash).
 *
 * Errors: 0 on success, a negative GGS_E* code otherwise; ggs_last_error()
 * returns a thread-local message.  The reference's assertion failures
 * (render.py:217 CUDA device, :219 ndim, :223 C >= 9) map to GGS_ENODEV and
 * GGS_EINVAL.  Thread safety: calls may come from any thread; each device
 * context is guarded by its own mutex.
 */
#ifndef GGS_H_
#define GGS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GGS_OK 0
#define GGS_EINVAL (-1) /* bad argument (reference asserts render.py:219,223) */
#define GGS_ENODEV (-2) /* no usable HIP device (reference assert render.py:217) */
#define GGS_EHIP (-3)   /* HIP runtime / launch failure */
#define GGS_ENOMEM (-4) /* device or pinned host allocation failed */

/* fitness modes (fitness.py:17-31) */
#define GGS_FIT_NONE 0     /* weight_mask is None:  mean over H*W*3 of d^2          */
#define GGS_FIT_WEIGHTED 1 /* default GA path:      sum(w*d^2) / (sum(w) + 1e-12)   */
#define GGS_FIT_BOOST 2    /* boost_only=True:      mean(d^2*wb) / (mean(wb)+1e-12), wb = 1+beta*clamp(w,0,1) */

/* Library version string. */
const char* ggs_version(void);

/* Initialise up to max_devices HIP devices (<=0: all).  Returns the number of
 * usable devices (>0) or a negative error.  Idempotent; called lazily by every
 * entry point. */
int ggs_init(int32_t max_devices);

/* Number of HIP devices the library sees (0 before ggs_init / without GPUs). */
int ggs_device_count(void);

/* Restrict the host API's fan-out to the listed device ids, in order (n == 0:
 * all devices).  One process per GPU calls this with its local rank.  Device
 * contexts are created lazily on first use.  Returns the active count. */
int ggs_select_devices(const int32_t* ids, int32_t n);

/* Thread-local message describing the last error on this thread ("" if none). */
const char* ggs_last_error(void);

/* Free every device buffer, stream and pinned host buffer. */
void ggs_shutdown(void);

/* ---- host-pointer API (drop-in path) ----------------------------------------
 * render: genomes [B,N,C] renderer layout -> out [B,H,W,3] in [0,1].
 *   bg: background RGB (render.py:209, default 1,1,1); NULL means (1,1,1).
 * fitness: genomes [B,N,C] axes-angle layout, target [H,W,3], mask [H,W]
 *   (NULL iff mode == GGS_FIT_NONE) -> out [B] float32.
 * n_devices: shard the B candidates contiguously over the first n_devices of
 *   the active device list (<=0: all of them; see ggs_select_devices). */
int ggs_render(const float* genomes, int64_t B, int32_t N, int32_t C, int32_t H, int32_t W,
               float k_sigma, const float* bg, float* out_bhw3, int32_t n_devices);
int ggs_fitness(const float* genomes_axes, int64_t B, int32_t N, int32_t C, const float* target_hw3,
                const float* mask_hw, int32_t mode, float boost_beta, int32_t H, int32_t W,
                float k_sigma, float* out_B, int32_t n_devices);

/* ---- stage exports (host pointers; parity tests) ----------------------------
 * encode: S splat rows (stride C) axes-angle -> renderer rows [S,9].
 * preprocess: S renderer rows (stride C) -> out_f9 [9][S] = cx, cy, sxx, sxy,
 *   syy, rc, gc, bc, a and out_i4 [4][S] = x0, x1, y0, y1 (render.py:45-47). */
int ggs_encode(const float* genomes_axes, int64_t S, int32_t C, float* out_S9);
int ggs_preprocess(const float* genomes, int64_t S, int32_t C, int32_t H, int32_t W, float k_sigma,
                   float* out_f9, int32_t* out_i4);

/* Deterministic-math probe (parity tests of csrc/ggs_detmath.h against
 * oracle/detmath.py): out[i] = f(x[i]) for fn 0 exp, 1 log, 2 sin, 3 cos,
 * 4 sqrt (correctly rounded), 5 x[i] / y[i] (correctly rounded). */
int ggs_detmath_eval(int32_t fn, const float* x, const float* y, int64_t n, float* out);

/* ---- device-pointer API (inputs resident in HBM) ----------------------------
 * Same semantics as the host API on one device; all pointers are device
 * pointers on `device`; work is enqueued on `stream` (a hipStream_t, NULL =
 * the null stream) and the call returns without synchronising. */
int ggs_render_device(int32_t device, void* stream, const float* d_genomes, int64_t B, int32_t N,
                      int32_t C, int32_t H, int32_t W, float k_sigma, const float* bg,
                      float* d_out_bhw3);
int ggs_fitness_device(int32_t device, void* stream, const float* d_genomes_axes, int64_t B,
                       int32_t N, int32_t C, const float* d_target_hw3, const float* d_mask_hw,
                       int32_t mode, float boost_beta, int32_t H, int32_t W, float k_sigma,
                       float* d_out_B);

/* Target plan: the fitness epilogue's inputs (target, mask, mode, beta) laid out
 * once in the raster's lane order — what ggs_fitness_device rebuilds on every
 * call.  A caller whose target/mask stay fixed over a run (a GA loop) builds it
 * once (enqueued on `stream`; the inputs must stay valid until it has run) and
 * evaluates generations with ggs_fitness_device_planned (same results). */
int ggs_plan_create(int32_t device, void* stream, const float* d_target_hw3, const float* d_mask_hw,
                    int32_t mode, float boost_beta, int32_t H, int32_t W, void** plan);
int ggs_fitness_device_planned(void* plan, void* stream, const float* d_genomes_axes, int64_t B,
                               int32_t N, int32_t C, float k_sigma, float* d_out_B);
void ggs_plan_destroy(void* plan);

/* Plan set: K target plans of one (H, W, mode, beta), built in one launch from
 * d_targets_khw3 [K,H,W,3] and d_masks_khw [K,H,W] (required unless mode is
 * GGS_FIT_NONE).  ggs_fitness_device_planset scores candidate b against plan
 * b / group in one prep / raster / finalize: group >= 1, B % group == 0 and
 * B / group <= K (fewer groups than plans use the first plans).  A candidate's
 * fitness has the bits ggs_fitness_device_planned gives it against that plan
 * alone.  Invalid arguments (those, K < 1, null pointers) are reported
 * (GGS_EINVAL) before any device is touched. */
int ggs_planset_create(int32_t device, void* stream, const float* d_targets_khw3, const float* d_masks_khw,
                       int32_t mode, float boost_beta, int32_t H, int32_t W, int32_t K, void** planset);
int ggs_fitness_device_planset(void* planset, void* stream, const float* d_genomes_axes, int64_t B,
                               int32_t N, int32_t C, int32_t group, float k_sigma, float* d_out_B);
void ggs_planset_destroy(void* planset);

/* ---- target preparation and importance mask (K images at once) ---------------
 * The inputs of the weighted fitness, made on the device from K images of one
 * size: targets [K,H,W,3] as algorithm.py:33-39 prepares them (float32, /255
 * when the image's maximum is > 1.5, bilinear resize to (H, W), align_corners
 * False; the identity when the sizes match) and masks [K,H,W] as
 * modules/mask.py:29-83 computes them from each prepared target (the range rule
 * once more on the prepared target, as the reference applies it; luma;
 * multi-scale Sobel edges; 9x9 local variance; _norm01 with exact 2 % / 98 %
 * quantiles; optional smoothing; gamma, floor and strength).  Every launch covers
 * all K images; image k's result has the bits a K = 1 call gives it, and two runs
 * agree bit for bit (integer atomics only).
 *
 * The outputs are what ggs_planset_create (d_targets_khw3, d_masks_khw) and, for
 * K = 1, ggs_plan_create (d_target_hw3, d_mask_hw) take: prepare on a stream,
 * create the plan or plan set on the same stream, and no host code touches the
 * pixels in between.
 *
 * params: edge_scales[0..n_scales) are summed in the order given (1 <= n_scales
 * <= 4, each scale s >= 1 with H / s >= 1 and W / s >= 1); smooth <= 0: no
 * smoothing, otherwise an odd window (an even one changes the array's size in
 * the reference); the reference's defaults are scales 1, 2, 4, w_edge 0.7, w_var
 * 0.3, gamma 0.7, floor 0.15, smooth 3 (algorithm.py:42-49).  params == NULL:
 * targets only, and d_masks_khw must be NULL.
 * Reported as GGS_EINVAL before any device is touched: K < 1 (or > 65535), null
 * pointers, sizes < 1, min(H, W) < 4 and the parameter rules above. */
typedef struct ggs_mask_params {
    int32_t n_scales;
    int32_t edge_scales[4];
    float w_edge, w_var, gamma, floor, strength;
    int32_t smooth;
} ggs_mask_params;

/* Device form: d_images [K,H0,W0,3], d_targets_khw3 and d_masks_khw are device
 * pointers on `device`; the work is enqueued on `stream` (scratch comes from the
 * library's pooled per-stream workspace) and the call returns without
 * synchronising. */
int ggs_targets_prepare_device(int32_t device, void* stream, const float* d_images, int32_t K, int32_t H0,
                               int32_t W0, int32_t H, int32_t W, const ggs_mask_params* params,
                               float* d_targets_khw3, float* d_masks_khw);
/* Host-pointer form (synchronous) on HIP device `device`. */
int ggs_targets_prepare(const float* images, int32_t K, int32_t H0, int32_t W0, int32_t H, int32_t W,
                        const ggs_mask_params* params, float* targets, float* masks, int32_t device);
/* Stage export (host pointers; parity tests): out[i] = numpy's 'linear' quantile
 * q[i] of x[0..n), float32 of the double interpolation between the two order
 * statistics around q[i] (n - 1), found by the radix select _norm01 uses.
 * 1 <= n < 2^31, 1 <= nq <= 8, 0 <= q[i] <= 1; -0 counts as +0, no NaNs. */
int ggs_quantiles(const float* x, int64_t n, const double* q, int32_t nq, float* out);

/* ---- device-resident GA ------------------------------
 * genetic_approx's generation loop (algorithm.py:85-155) on one device: the
 * population, fitness, elites, best individual and curves stay in HBM; a
 * generation is variation -> fitness -> survivors -> gather, no host sync.
 * Up to pop_size 512 the survivors/gather of a generation run inside the next
 * generation's variation launch ("breed"), and the fitness finalize inside the
 * raster launch (its last strip wave per candidate reduces): 2 launches per
 * generation instead of 5; ggs_ga_read applies the last generation's survivors
 * first, so what it returns is the same either way (GGS_GA_UNFUSED=1: separate
 * survivors/gather launches; GGS_UNFUSED_FINALIZE=1: a separate finalize launch).
 * Draws: explicit arrays (ggs_ga_step with draws != NULL; replay / parity) or a
 * counter-based Philox4x32-10 stream keyed by (seed, generation, individual). */
typedef struct ggs_ga_config {
    int32_t pop_size, n_splats, H, W, tour_k, elite_k;
    float cxpb, mutpb, k_sigma, min_scale_splats, max_scale_splats;
    float scale_log_lo, scale_log_hi; /* clamp bounds log(min), log(max*max(H,W)); 0,0 = compute */
    int32_t fitness_mode;             /* GGS_FIT_* */
    float boost_beta;
    int32_t schedule;                 /* 0 linear, 1 cosine, 2 exp (utils.py:14-27) */
    double sig_max[6], sig_min[6];    /* xy, alog, blog, theta, rgb, alpha (config.py:22-43) */
    uint64_t seed;
} ggs_ga_config;

typedef struct ggs_ga_draws {         /* host arrays for ONE generation (ggs/ga.py layout) */
    const int32_t* tour_idx;          /* [P*k]   random.randrange draws (genetic.py:11) */
    const int32_t* perm;              /* [P]     random.shuffle (algorithm.py:90) */
    const int32_t* cx;                /* [ceil(P/2)] crossover decisions (algorithm.py:97) */
    const float* cx_u;                /* [ceil(P/2)*N] crossover masks (genetic.py:18) */
    const float *u_xy, *u_ab;         /* [P*N*2] mask uniforms (genetic.py:37-38) */
    const float *u_t, *u_rgb, *u_a;   /* [P*N] */
    const int32_t *k_color, *k_xy, *k_ab, *k_t;   /* [P] one-true fallbacks (genetic.py:24-29) */
    const float *n_xy, *n_ab;         /* [P*N*2] normals (genetic.py:57-70) */
    const float* n_t;                 /* [P*N] */
    const float* n_rgba;              /* [P*N*4] */
    const int32_t *swap_i, *swap_pick;/* [P] swap draws (genetic.py:79-91); pick < 0 -> swap_u */
    const double* swap_u;             /* [P] */
} ggs_ga_draws;

/* init_pop [P,N,9] axes-angle (required); mask may be NULL iff fitness_mode is
 * GGS_FIT_NONE.  Evaluates the initial population. */
int ggs_ga_create(int32_t device, const ggs_ga_config* cfg, const float* target_hw3,
                  const float* mask_hw, const float* init_pop, void** handle);
/* Shard the device GA's fitness evaluation over the ranks of `comm` (one
 * process per GPU; every rank created its session with the same config, target,
 * mask, initial population and seed, and steps it with the same arguments —
 * checked: the ranks exchange a 64-bit fingerprint of those inputs and the call
 * fails with GGS_EINVAL on every rank if any differ):
 * each generation every rank breeds all P offspring (same draws), rasterises its
 * contiguous block of ceil(P/nranks), and one in-place RCCL all-gather of the
 * offspring fitness scalars lets every rank run the same survivors step, so the
 * populations stay identical without exchanging genomes (north_star: shard the
 * generation's candidates across the GPUs of a node).  comm = NULL: one GPU.
 * The communicator must outlive the session's use of it. */
int ggs_ga_set_comm(void* handle, void* comm);
int ggs_ga_step(void* handle, int32_t gen, int32_t total_gens, const ggs_ga_draws* draws);
int ggs_ga_run(void* handle, int32_t first_gen, int32_t n_gens, int32_t total_gens);
/* Synchronises; any output may be NULL.  curves: [n_curves][3] = best, mean, median. */
int ggs_ga_read(void* handle, float* pop, float* fits, float* best_ind, double* best_fit,
                double* curves, int32_t* n_curves);
void ggs_ga_destroy(void* handle);

/* ---- island groups: K device GA populations with ring migration ---------------
 * K independent populations ("islands") of cfg->pop_size rows each, one target,
 * in one session: one stream, one target plan, and per generation one breed
 * launch for all islands (grid: offspring x island) and one raster launch over
 * the K (P - E) evaluated offspring (E = max(1, elite_k)).  Island k draws from
 * the Philox stream of seeds[k] and, without migration, follows bit for bit the
 * trajectory of a ggs_ga_create session with that seed and init_pops[k].
 * Migration (ring, n_migrants = m): after the survivors of every generation g
 * with g % migrate_every == 0 (generations count absolutely, as passed to
 * ggs_ga_islands_run), all islands at once and from the pre-migration state,
 * the row of fitness rank j < m of island (k - 1 + K) % K (ascending, ties by
 * lower row) overwrites the row of rank P - 1 - j of island k, genome and
 * fitness; island k's elites are re-ranked.  Best-so-far and curves are not
 * touched: the next generation's statistics pick an immigrant up.  K == 1,
 * migrate_every == 0 or m == 0: no migration.  pop_size <= 512.  Explicit draws
 * and ggs_ga_set_comm are not offered for groups.  Invalid arguments are
 * reported (GGS_EINVAL) before any device is touched. */
typedef struct ggs_ga_islands {
    int32_t n_islands;        /* K >= 1 */
    int32_t migrate_every;    /* generations between migrations, 0 = never */
    int32_t n_migrants;       /* m, 0 <= m <= pop_size / 2 */
    int32_t topology;         /* 0 = ring (the only one) */
    const uint64_t* seeds;    /* [K] Philox seed of each island (cfg->seed is ignored) */
} ggs_ga_islands;
int ggs_ga_islands_create(int32_t device, const ggs_ga_config* cfg, const ggs_ga_islands* isl,
                          const float* target_hw3, const float* mask_hw,
                          const float* init_pops /* [K,P,N,9] */, void** handle);
/* A target per island: targets_khw3 [K,H,W,3], masks_khw [K,H,W] (NULL iff
 * fitness_mode is GGS_FIT_NONE); island k is fitted to image k (K images, the
 * frames of a clip, the tiles of a picture in one session).  One plan set, and
 * still one breed and one raster launch per generation: candidate k (P - E) + o
 * is scored against plan k.  Without migration island k follows bit for bit
 * the ggs_ga_create session on (targets[k], masks[k], seeds[k], init_pops[k]).
 * Migration moves the same rows as above, but an immigrant's fitness was
 * measured against its SOURCE island's image, so it is RE-SCORED: the genome
 * is copied, the K m immigrants are evaluated against their destination
 * island's target and mask (one prep and one grouped raster launch), that
 * fitness is installed in the rows they took, and only then are island k's
 * elites re-ranked from the new fitness vector.  (With K copies of one target
 * this installs exactly the fitness the shared-target group copies.)
 * Best-so-far and curves are not touched, as above.  Run, read and destroy are
 * ggs_ga_islands_run / _read / _destroy. */
int ggs_ga_islands_create_targets(int32_t device, const ggs_ga_config* cfg, const ggs_ga_islands* isl,
                                  const float* targets_khw3, const float* masks_khw,
                                  const float* init_pops /* [K,P,N,9] */, void** handle);
int ggs_ga_islands_run(void* handle, int32_t first_gen, int32_t n_gens, int32_t total_gens);
/* Synchronises; any output may be NULL: pop [K,P,N,9], fits [K,P], best_ind [K,N,9],
 * best_fit [K], curves [K][n_curves][3], n_curves (the same for every island). */
int ggs_ga_islands_read(void* handle, float* pop, float* fits, float* best_ind, double* best_fit,
                        double* curves, int32_t* n_curves);
void ggs_ga_islands_destroy(void* handle);

/* ---- device-resident simulated-annealing neighbours (annealing.py:121-150) ---
 * The current state stays on the GPU.  ggs_sa_propose mutates it into n
 * neighbours — tries first_try .. first_try+n-1 of iteration `it`, draws either
 * explicit (ggs_ga_draws layout, mutation fields only, indexed by local try) or
 * Philox keyed by (seed, it, try), so a try's neighbour does not depend on how
 * the tries are batched — evaluates them in one launch and returns their
 * energies.  The host runs the acceptance test (annealing.py:133-146) and
 * ggs_sa_commit installs the accepted neighbour j (and/or snapshots the best).
 * cfg: pop_size = the largest n per propose call; tour_k/elite_k/cxpb unused.
 * Replaces: annealing.py:122-131 (duplicate + mutate_individual + fitness). */
int ggs_sa_create(int32_t device, const ggs_ga_config* cfg, const float* target_hw3,
                  const float* mask_hw, const float* init_ind, void** handle, float* init_fit);
int ggs_sa_propose(void* handle, int32_t it, int32_t total_iters, int32_t first_try, int32_t n,
                   const ggs_ga_draws* draws, float* fits_out);
/* j >= 0: current <- neighbour j of the last propose; update_best: best <- current. */
int ggs_sa_commit(void* handle, int32_t j, int32_t update_best);
/* Synchronises; any output may be NULL.  neighbours: [n of the last propose][N][9]. */
int ggs_sa_read(void* handle, float* current, float* best, float* neighbours);
/* The SA loop itself on the device (annealing.py:117-155 for iterations
 * first_it .. first_it+n_its-1): each round mutates the next tries from the
 * current state (Philox keyed by (seed, it, try), as ggs_sa_propose), evaluates
 * them in one launch and walks them in order with the Metropolis test of
 * annealing.py:133-146 — acceptance uniform ggs_sa_accept_uniform(seed, it, try)
 * — installing the first accepted neighbour (and the best, :148-150) on the GPU;
 * the host syncs once per batch of rounds, not per try.  temps[i]: temperature of
 * iteration first_it+i (annealing.py:29-44, the caller's float64); width:
 * neighbours per round, 0 = adaptive (1 / acceptance rate, at most pop_size);
 * results do not depend on it.  curves_out[i] = {best, current} energy after
 * iteration first_it+i (annealing.py:152-155).  A session is driven either by
 * ggs_sa_run or by ggs_sa_propose/commit, not both. */
int ggs_sa_run(void* handle, int32_t first_it, int32_t n_its, int32_t total_iters, int32_t tries,
               const double* temps, int32_t width, double* curves_out);
/* ggs_sa_run's batching rule (pure host arithmetic, no device): rounds enqueued
 * before the next host sync when `remaining` tries of the chunk are left and a
 * round is expected to consume `est` of them — ceil(remaining / est), at least
 * 1, at most GGS_SA_MAX_ROUNDS_PER_SYNC (a bound on the dispatches queued
 * between syncs: 4 per round, 6 with incremental evaluation). */
#define GGS_SA_MAX_ROUNDS_PER_SYNC 64
int64_t ggs_sa_rounds_per_sync(int64_t remaining, int32_t est);
/* The device loop's state after the last ggs_sa_run (any output may be NULL). */
int ggs_sa_loop_state(void* handle, double* best_fit, double* curr_fit, uint64_t* rounds,
                      uint64_t* evaluated, uint64_t* accepted);
/* The acceptance uniform in [0, 1) ggs_sa_run draws for try k of iteration it
 * (lets a host loop reproduce the device loop's trajectory). */
int ggs_sa_accept_uniform(uint64_t seed, int32_t it, int32_t k, double* u);
/* Stage export (host pointers; parity tests): the draws the GA / SA variation
 * kernels take from their in-kernel Philox4x32-10 stream (counter (gen, who,
 * what, stream), key = seed; DESIGN.md has the layout) for generation `gen`
 * (SA: iteration `it`) and offspring first .. first+n_off-1 (SA: tries; `first`
 * is ggs_sa_propose's first_try, 0 for the GA), computed on `device` by the
 * kernels' own draw functions and written into caller-owned host arrays in the
 * ggs_ga_draws layout: per-offspring arrays are indexed by the local offspring
 * 0 .. n_off-1 ([n_off*N*2] ..., [n_off]), cx / cx_u by the local pair
 * ([ceil(n_off/2)], [ceil(n_off/2)*N]), tour_idx [P*tour_k] and perm [P] by the
 * tournament slot.  Every slot is filled, also those a kernel would not consume
 * (a fallback index when a mask flag is set, ...).  Philox mode's conventions:
 * perm is the identity, cx = (u01 < cxpb), swap_pick = -1 with swap_u the
 * uniform, swap_i = 0 when N < 2.  ggs_ga_step / ggs_sa_propose fed these
 * arrays compute what the Philox run computes, bit for bit.
 * n_off, P, N, tour_k < 1, gen or first < 0, a null array and sizes past 2^27
 * draws per array are reported (GGS_EINVAL) before any device is touched. */
typedef struct ggs_ga_draws_out {     /* ggs_ga_draws with writable arrays, same order */
    int32_t *tour_idx, *perm, *cx;
    float* cx_u;
    float *u_xy, *u_ab, *u_t, *u_rgb, *u_a;
    int32_t *k_color, *k_xy, *k_ab, *k_t;
    float *n_xy, *n_ab, *n_t, *n_rgba;
    int32_t *swap_i, *swap_pick;
    double* swap_u;
} ggs_ga_draws_out;
int ggs_ga_philox_draws(int32_t device, uint64_t seed, int32_t gen, int32_t first, int32_t n_off, int32_t P,
                        int32_t N, int32_t tour_k, float cxpb, const ggs_ga_draws_out* out);
/* Incremental evaluation (default off): a neighbour's 16-column strips that no
 * changed splat touches (old or new AABB) keep the current state's partial sums —
 * bit-identical to a full re-render; off = every strip is rasterised.  Turning
 * it on re-evaluates the current state's records and strip partials (the device
 * loop keeps them only while it is on), so it may be toggled between calls. */
int ggs_sa_set_incremental(void* handle, int32_t on);
/* Neighbours proposed and splats found changed (summed over proposals). */
int ggs_sa_stats(void* handle, uint64_t* proposed, uint64_t* changed_splats);
void ggs_sa_destroy(void* handle);

/* ---- SA chain groups: K annealing chains in one session ---------------------
 * K chains of the device loop above (ggs_sa_run) in one session: one set of
 * launches per round for all chains (grid: neighbour x chain) and one raster
 * launch over exactly the neighbours the chains have live in that round (a
 * compact candidate list written on the device; a chain at high acceptance has
 * one, a cold chain the round's width, a chain that finished the chunk none).
 * Chain k draws from the Philox stream of seeds[k] and, without exchange,
 * follows bit for bit the ggs_sa_create + ggs_sa_run session with that seed on
 * init_inds[k] and temps[k]: current and best genome, both energies, curves and
 * the accepted count.  Its trajectory does not depend on K, on the other
 * chains, on `width`, or on how many rounds are queued between host syncs.
 * cfg: pop_size = the neighbour capacity PER CHAIN.  Only the ggs_sa_run driver
 * exists for groups: no propose/commit, explicit draws or incremental evaluation.
 * Replica exchange (exchange_every = M > 0, shared target only): ggs_sa_chains_run
 * splits its range after every iteration `it` with (it + 1) % M == 0 (iterations
 * count absolutely, as passed in); once all chains have finished it, exchange
 * e = (it + 1) / M - 1 considers the pairs (k, k + 1), k % 2 == e % 2, k + 1 < K,
 * all from the pre-exchange energies: with T_k chain k's temperature of
 * iteration `it` and d = (E_k - E_{k+1}) (1 / T_k - 1 / T_{k+1}) in float64, the
 * pair trades current genome and energy iff u < exp(d),
 * u = ggs_sa_exchange_uniform(exchange_seed, it, k) (equal temperatures: always;
 * a pair with a temperature <= 0 is skipped and not counted).  Each chain of a
 * swapped pair then applies annealing.py:148-150 (curr + 1e-12 < best: that state
 * becomes its best).  Curves already written are not touched.
 * K < 1 or K > GGS_SA_MAX_CHAINS, null pointers, exchange_every < 0,
 * exchange_every > 0 with _create_targets (an energy measured on another image
 * means nothing) and ggs_sa_run's argument rules are reported (GGS_EINVAL)
 * before any device is touched. */
#define GGS_SA_MAX_CHAINS 64
typedef struct ggs_sa_chains {
    int32_t n_chains;          /* K >= 1 */
    int32_t exchange_every;    /* M iterations between replica exchanges, 0 = never */
    const uint64_t* seeds;     /* [K] Philox seed of each chain (cfg->seed is ignored) */
    uint64_t exchange_seed;    /* key of the exchange uniforms */
} ggs_sa_chains;
/* One target and mask for all chains (ONE target plan); init_fits [K] may be NULL. */
int ggs_sa_chains_create(int32_t device, const ggs_ga_config* cfg, const ggs_sa_chains* chains,
                         const float* target_hw3, const float* mask_hw, const float* init_inds /* [K,N,9] */,
                         void** handle, float* init_fits /* [K] */);
/* A target per chain: targets_khw3 [K,H,W,3], masks_khw [K,H,W] (NULL iff
 * fitness_mode is GGS_FIT_NONE), one plan set; chain k anneals image k. */
int ggs_sa_chains_create_targets(int32_t device, const ggs_ga_config* cfg, const ggs_sa_chains* chains,
                                 const float* targets_khw3, const float* masks_khw,
                                 const float* init_inds /* [K,N,9] */, void** handle, float* init_fits /* [K] */);
/* ggs_sa_run for every chain: temps [K][n_its], curves_out [K][n_its][2]. */
int ggs_sa_chains_run(void* handle, int32_t first_it, int32_t n_its, int32_t total_iters, int32_t tries,
                      const double* temps, int32_t width, double* curves_out);
/* The chains' loop state after the last run, arrays of K (any output may be NULL),
 * and the session's exchange counts. */
int ggs_sa_chains_state(void* handle, double* best_fit, double* curr_fit, uint64_t* rounds, uint64_t* evaluated,
                        uint64_t* accepted, uint64_t* swaps_tried, uint64_t* swaps_accepted);
/* Synchronises; any output may be NULL: current, best [K,N,9]. */
int ggs_sa_chains_read(void* handle, float* current, float* best);
void ggs_sa_chains_destroy(void* handle);
/* The exchange uniform in [0, 1) of pair (k, k + 1) after iteration it: the Philox
 * block of ggs_sa_accept_uniform with counter word what = 1. */
int ggs_sa_exchange_uniform(uint64_t exchange_seed, int32_t it, int32_t k, double* u);

/* ---- differential evolution: a third device-resident optimiser ----------------
 * A population of cfg->pop_size axes-angle genomes evolved by DE on one GPU, three
 * launches per generation on the session's own stream: variation (P trials with
 * their raster records), the fitness raster over the P trials, select.  Generation
 * gen >= 1 is synchronous (every trial is built from the population as it stood
 * at the start of the generation).  Target row i draws from the Philox block
 * (gen, i, what, 9) keyed by cfg->seed: three distinct rows r1, r2, r3 != i, a
 * forced crossover position jrand, F_i = f_lo + u (f_hi - f_lo) and one uniform
 * per gene (crossover 0) or per splat (crossover 1).  Mutant v (float32, one
 * rounding per operation, angle differences through wrap_angle):
 *   strategy 0  rand/1             x[r1] + F (x[r2] - x[r3])
 *   strategy 1  best/1             x[best] + F (x[r1] - x[r2])
 *   strategy 2  current-to-best/1  (x[i] + F (x[best] - x[i])) + F (x[r1] - x[r2])
 * with best the row of lowest fitness (ties: the lowest row).  A gene (all nine
 * genes of a splat, crossover 1) comes from the mutant iff its uniform < cr or it
 * is the jrand gene (splat), and is then clamped by clamp_genome's rule of its
 * column; every other gene is the parent's, bit for bit.  Trial i replaces row i
 * iff f_trial[i] <= f[i] (float32: a NaN keeps the parent).  Best so far and the
 * curves follow ggs_ga_*'s arithmetic.  ggs/de.py restates all of it in numpy and
 * DESIGN.md has the counter layout; a run is held to that restatement bit for bit.
 * From cfg: pop_size, n_splats, H, W, k_sigma, the scale bounds, fitness_mode,
 * boost_beta and seed; the rest is ignored.  pop_size < 4 or > 512, n_splats < 1,
 * cr outside [0, 1], f_lo > f_hi or not finite, an unknown strategy or crossover,
 * null required pointers and a mask missing for the mode are reported
 * (GGS_EINVAL) before any device is touched. */
typedef struct ggs_de_params {
    int32_t strategy;     /* 0 rand/1, 1 best/1, 2 current-to-best/1 */
    int32_t crossover;    /* 0 per gene, 1 per splat */
    float f_lo, f_hi;     /* F per trial uniform in [f_lo, f_hi]; equal = fixed F */
    float cr;             /* [0, 1] */
} ggs_de_params;
/* init_pop [P,N,9] (required); mask may be NULL iff fitness_mode is GGS_FIT_NONE.
 * Evaluates the initial population (curves row 0). */
int ggs_de_create(int32_t device, const ggs_ga_config* cfg, const ggs_de_params* de,
                  const float* target_hw3, const float* mask_hw, const float* init_pop, void** handle);
/* New parameters for the generations run from now on (F / CR schedules from the host). */
int ggs_de_set_params(void* handle, const ggs_de_params* de);
int ggs_de_run(void* handle, int32_t first_gen, int32_t n_gens);
/* Synchronises; any output may be NULL.  pop, trials [P,N,9]; fits, trial_fits [P];
 * curves [n_curves][3] = best, mean, median.  trials / trial_fits are those of the
 * last generation run (unspecified before the first). */
int ggs_de_read(void* handle, float* pop, float* fits, float* trials, float* trial_fits,
                float* best_ind, double* best_fit, double* curves, int32_t* n_curves);
void ggs_de_destroy(void* handle);

/* ---- fitness gradients ----------------------------------------
 * out [B]: the fitness, by the same prep -> raster -> finalize launches as
 * ggs_fitness_device (the same bits).  grad [B,N,9], whatever the input stride
 * C >= 9: d out[b] / d genomes[b,s,0:9], the derivative of the composition encode
 * (encode.py:4-59) -> preprocess (render.py:8-47) -> "over" blend in ascending
 * splat order (render.py:189-196) -> clip to [0,1] -> fitness.py:7-31, with the
 * integer AABB held constant, clip(x, lo, hi) passing the gradient iff
 * lo <= x <= hi and max(x, eps) iff x > eps.  Deterministic: reruns and other
 * batches give a candidate the same bits.  One device.  B, N, H or W < 1, C < 9,
 * null pointers (out may be NULL in the device call), an unknown mode and a mask
 * missing for the mode are reported (GGS_EINVAL) before any device is touched;
 * a candidate whose strip partials (48 B per splat and 16 x 32 pixel strip)
 * exceed the 40 MiB workspace budget is refused with GGS_ENOMEM.  The host call
 * synchronises every stream it queued work on before returning, errors included. */
int ggs_fitness_grad(const float* genomes_axes, int64_t B, int32_t N, int32_t C, const float* target_hw3,
                     const float* mask_hw, int32_t mode, float boost_beta, int32_t H, int32_t W,
                     float k_sigma, float* out_B, float* grad_BN9);
int ggs_fitness_grad_device(int32_t device, void* stream, const float* d_genomes_axes, int64_t B, int32_t N,
                            int32_t C, const float* d_target_hw3, const float* d_mask_hw, int32_t mode,
                            float boost_beta, int32_t H, int32_t W, float k_sigma,
                            float* d_out_B, float* d_grad_BN9);
/* A target per candidate: out and grad of candidate b are the bits
 * ggs_fitness_grad_device gives it against d_targets_khw3[b / group],
 * d_masks_khw[b / group] alone.  The plan set keeps the pixels only in the raster's
 * lane order, so the call also takes the raw arrays the set was created from (the
 * caller's responsibility); the set supplies the fitness and each image's Sum w.
 * Rules of ggs_fitness_device_planset (group >= 1, B % group == 0, B / group <= K)
 * and of ggs_fitness_grad_device, all GGS_EINVAL / GGS_ENOMEM before any device is
 * touched. */
int ggs_fitness_grad_device_planset(void* planset, void* stream, const float* d_genomes_axes, int64_t B, int32_t N,
                                    int32_t C, int32_t group, const float* d_targets_khw3,
                                    const float* d_masks_khw, float k_sigma, float* d_out_B, float* d_grad_BN9);
/* host pointers, synchronous, one device: builds its own plan set of the K images */
int ggs_fitness_grad_targets(const float* genomes_axes, int64_t B, int32_t N, int32_t C,
                             const float* targets_khw3, const float* masks_khw, int32_t K, int32_t group,
                             int32_t mode, float boost_beta, int32_t H, int32_t W, float k_sigma,
                             float* out_B, float* grad_BN9);

/* ---- differentiable render -------------------------------------
 * The renderer's vector-Jacobian product.  With img[b] = clip(blend(preprocess(
 * rows[b])), 0, 1) against the background bg, exactly what ggs_render_device
 * writes, and a cotangent cot [B,H,W,3] (d loss / d img of any loss),
 *   grad[b,s,0:9] = sum over y, x, ch of cot[b,y,x,ch] * d img[b,y,x,ch] / d rows[b,s,0:9]
 * grad is [B,N,9] whatever the input stride C >= 9.  layout names what the rows
 * are: GGS_LAYOUT_RENDERER, ggs_render's input (x, y, log l11, log l22, l21, r, g,
 * b, alpha), or GGS_LAYOUT_AXES, axes-angle rows that encode (encode.py:4-59)
 * turns into renderer rows first, as the fitness path does.  The derivative's
 * conventions are those of the fitness gradient above (constant integer AABB,
 * clip passes iff lo <= x <= hi, max(x, eps) iff x > eps, the image clip per
 * channel on the unclipped float32 colour); there is no gradient with respect to
 * bg (host pointer to three floats, NULL = 1, 1, 1).  Deterministic: reruns and
 * other batches give a candidate the same bits.  One device.  B, N, H or W < 1,
 * C < 9, B * N >= 2^31, a null genome, cotangent or gradient pointer and an unknown
 * layout are reported (GGS_EINVAL) before any device is touched; a candidate whose
 * strip partials exceed the 40 MiB workspace budget is refused with GGS_ENOMEM.
 * The device call enqueues on `stream` and returns; the host call synchronises
 * every stream it queued work on before returning, errors included.
 * ggs_render_layout_device is ggs_render_device with the rows in `layout`: layout
 * 0 issues ggs_render_device's launches (the same bits), layout 1 gives the bits
 * of ggs_render on ggs_encode's rows. */
#define GGS_LAYOUT_RENDERER 0
#define GGS_LAYOUT_AXES 1
int ggs_render_vjp_device(int32_t device, void* stream, const float* d_genomes, int64_t B, int32_t N, int32_t C,
                          int32_t layout, int32_t H, int32_t W, float k_sigma, const float* bg /* host, NULL = 1,1,1 */,
                          const float* d_cot_bhw3, float* d_grad_BN9);
int ggs_render_vjp(const float* genomes, int64_t B, int32_t N, int32_t C, int32_t layout, int32_t H, int32_t W,
                   float k_sigma, const float* bg, const float* cot_bhw3, float* grad_BN9, int32_t device);
int ggs_render_layout_device(int32_t device, void* stream, const float* d_genomes, int64_t B, int32_t N, int32_t C,
                             int32_t layout, int32_t H, int32_t W, float k_sigma, const float* bg, float* d_out_bhw3);

/* ---- image losses ------------------------------------------------
 * For candidate b with image x = img[b] [H,W,3] (what ggs_render_device writes) and
 * target y = targets[b / group],
 *   loss[b] = w_l1 mean|x - y| + w_mse mean (x - y)^2 + w_ssim (1 - mean SSIM(x, y))
 * the means over all 3 H W values; SSIM per channel with the 11 x 11 separable
 * Gaussian window (sigma 1.5, taps normalised in float64), zero padding, C1 = 0.01^2,
 * C2 = 0.03^2 (the 3DGS / GaussianImage loss is w = (1 - lambda, 0, lambda)).
 * cot[b] = d loss[b] / d x [H,W,3], with d|d|/dd = sign(d), sign(0) = 0.  Everything
 * between the float32 inputs and the float32 outputs is float64.  Deterministic:
 * reruns, other batches and a NULL cotangent give a candidate's loss the same bits.
 * The group rule of ggs_fitness_device_planset (group >= 1, B % group == 0,
 * B / group <= K), B, H or W < 1, null pointers (the cotangent may be NULL) and weights
 * that are negative, not finite or all zero are GGS_EINVAL before any device is
 * touched.  The device calls enqueue on `stream` and return; the host calls
 * synchronise every stream they queued work on before returning, errors included. */
typedef struct ggs_loss_params {
    float w_l1, w_mse, w_ssim;       /* each >= 0 and finite, not all 0 */
} ggs_loss_params;
int ggs_image_loss_device(int32_t device, void* stream, const float* d_img_bhw3, int64_t B,
                          const float* d_targets_khw3, int32_t K, int32_t group, int32_t H, int32_t W,
                          const ggs_loss_params* p, float* d_loss_B, float* d_cot_bhw3 /* may be NULL */);
int ggs_image_loss(const float* img_bhw3, int64_t B, const float* targets_khw3, int32_t K, int32_t group, int32_t H,
                   int32_t W, const ggs_loss_params* p, float* loss_B, float* cot_bhw3 /* may be NULL */,
                   int32_t device);
/* loss [B] and d loss / d rows [B,N,9] in one call: ggs_render_layout_device, the image
 * loss and ggs_render_vjp_device, issued as those entry points issue them (bytewise what
 * the three calls give), the image and the cotangent in scratch the library owns
 * (24 B per pixel of the batch).  Argument rules of ggs_render_vjp_device (GGS_ENOMEM
 * for its 40 MiB partial budget) and of ggs_image_loss_device. */
int ggs_loss_grad_device(int32_t device, void* stream, const float* d_genomes, int64_t B, int32_t N, int32_t C,
                         int32_t layout, const float* d_targets_khw3, int32_t K, int32_t group, int32_t H, int32_t W,
                         float k_sigma, const float* bg /* host, NULL = 1,1,1 */, const ggs_loss_params* p,
                         float* d_loss_B, float* d_grad_BN9);
int ggs_loss_grad(const float* genomes, int64_t B, int32_t N, int32_t C, int32_t layout, const float* targets_khw3,
                  int32_t K, int32_t group, int32_t H, int32_t W, float k_sigma, const float* bg,
                  const ggs_loss_params* p, float* loss_B, float* grad_BN9, int32_t device);

/* ---- Adam refiner --------------------------------------------------------------
 * B candidates [B,N,9] refined side by side on the session's own stream.  Step t
 * (from 1) evaluates fitness and gradient g of the state x_t, makes x_t the
 * candidate's best so far iff fit + 1e-10 < best (float64), and updates in
 * float32, every operation rounded once in this order (division and sqrt
 * correctly rounded):
 *   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) (g g)
 *   x = x - (lr[c] (m / c1)) / (sqrt(v / c2) + eps),  c1 = float(1 - beta1^t), c2 likewise
 * (the powers in float64), then clamp_genome's rule of column c (utils.py:35-45;
 * an angle already in [-pi, pi) keeps its bits).  ggs/refine.py adam_step is the
 * numpy statement a run is held to bit for bit.  From cfg: n_splats, H, W, k_sigma,
 * the scale bounds, fitness_mode and boost_beta; the rest is ignored.  Argument
 * errors as ggs_fitness_grad, plus lr < 0 or not finite, beta outside [0, 1) and
 * eps <= 0 (GGS_EINVAL, before any device is touched). */
typedef struct ggs_refine_params {
    float lr[9];          /* per gene column: x, y, log a, log b, theta, r, g, b, alpha */
    float beta1, beta2, eps;
} ggs_refine_params;
int ggs_refine_create(int32_t device, const ggs_ga_config* cfg, const ggs_refine_params* p,
                      const float* target_hw3, const float* mask_hw, const float* genomes_BN9, int32_t B,
                      void** handle);
int ggs_refine_run(void* handle, int32_t n_steps);      /* enqueues; no host synchronisation */
/* Evaluates the current state (so fits belongs to genomes, and may become the best
 * so far) and synchronises; any output may be NULL.  genomes, best, last_grad
 * [B,N,9]; fits, best_fits [B].  last_grad: the gradient of the last step run. */
int ggs_refine_read(void* handle, float* genomes, float* fits, float* best, float* best_fits, float* last_grad);
void ggs_refine_destroy(void* handle);
/* K images in one session: targets_khw3 [K,H,W,3], masks_khw [K,H,W] (NULL iff
 * fitness_mode is GGS_FIT_NONE), one plan set built at create; candidate b is
 * refined against image b / group (group >= 1, B % group == 0, B / group <= K).
 * Run, read and destroy are the calls above.  Every array read returns for
 * candidate b carries the bits of a ggs_refine_create session on that genome and
 * image alone.  Argument errors as ggs_refine_create and
 * ggs_fitness_grad_device_planset (GGS_EINVAL / GGS_ENOMEM before any device is
 * touched). */
int ggs_refine_create_targets(int32_t device, const ggs_ga_config* cfg, const ggs_refine_params* p,
                              const float* targets_khw3, const float* masks_khw, int32_t K,
                              const float* genomes_BN9, int32_t B, int32_t group, void** handle);
/* The refiner on the image loss above: step t evaluates ggs_loss_grad_device's loss and
 * gradient of the axes-angle state (GGS_LAYOUT_AXES) against image b / group and the
 * background bg (host, NULL = 1, 1, 1); fits is the loss.  The Adam update, the best-so-far
 * rule and run / read / destroy are those above; cfg's fitness_mode and boost_beta are
 * not read.  Argument errors as ggs_refine_create_targets and ggs_loss_grad_device. */
int ggs_refine_create_loss(int32_t device, const ggs_ga_config* cfg, const ggs_refine_params* p,
                           const ggs_loss_params* loss, const float* bg, const float* targets_khw3, int32_t K,
                           const float* genomes_BN9, int32_t B, int32_t group, void** handle);

/* ---- density control of a refine session: relocation ---------------
 * The genome keeps its N splats; every `every` steps a candidate's dead splats are
 * re-used as clones or split halves of its live splats with the largest accumulated
 * positional gradient.  ggs/refine.py density_accumulate / relocate are the numpy
 * statement the device is held to bit for bit.  Float32, every operation rounded once
 * in the written order, division and sqrt correctly rounded.
 *   accumulate, on every step while on, after the gradient g of x_t and before the Adam
 *     update: acc[b,s] += sqrt(px px + py py), px = g[b,s,0] / float(max(W - 1, 1)),
 *     py = g[b,s,1] / float(max(H - 1, 1)); n_acc counts the steps accumulated.
 *   event, after the Adam update of step t when t % every == 0, t >= start and
 *     (stop == 0 or t <= stop), per candidate on the updated x:
 *     dead[s] = x[s,8] < alpha_dead; src[s] = !dead[s] && acc[s] / float(n_acc) > grad_min
 *     (a NaN is not a source); the dead list ascending by (alpha, index), the source
 *     list descending by acc, ties to the lower index, -0.0 equal to +0.0;
 *     n = min(|dead|, |src|, max_moves); pair j < n is (d = dead[j], s = src[j]).
 *     Clone, when max(x[s,2], x[s,3]) <= split_log: row d becomes row s's nine genes,
 *     m[d] = v[d] = 0, row s keeps everything.  Split otherwise, from row s's values
 *     before the event: L = max(x[s,2], x[s,3]), the major axis is a iff
 *     x[s,2] >= x[s,3]; (ux, uy) = (cos th, sin th) for a, else (-sin th, cos th);
 *     dlt = split_offset exp(L); dx = (dlt ux) / float(max(W - 1, 1)),
 *     dy = (dlt uy) / float(max(H - 1, 1)); row s gets x0 = clip(x0 + dx, 0, 1),
 *     x1 = clip(x1 + dy, 0, 1) and x2, x3 = clip(. - log_shrink, scale_log_lo,
 *     scale_log_hi), row d the same with - dx, - dy; angle, colour and alpha are copied;
 *     m and v are zeroed for both rows.  exp, sin and cos are ggs_detmath_eval's.
 *     Then acc and n_acc are zeroed for every candidate, moved or not.
 * best, best_fit, last_grad and t are untouched, and the Adam bias corrections stay
 * global in t.  Genomes that are not finite are not a supported input. */
typedef struct ggs_refine_density {
    int32_t every;        /* steps between events; 0 = off */
    int32_t start;        /* no event before step start */
    int32_t stop;         /* no event after step stop; 0 = no end */
    int32_t max_moves;    /* pairs per candidate and event; the effective value is min(max_moves, N / 2) */
    float alpha_dead;     /* in [0, 255] */
    float grad_min;       /* >= 0 */
    float split_log;
    float log_shrink;     /* >= 0 */
    float split_offset;
} ggs_refine_density;
/* Works on a session of any of the three creates and holds for the steps run after the
 * call; allocates what it needs and starts acc, n_acc and the event log from zero.
 * NULL or every == 0: off, and a session that never had it on keeps its bits.
 * GGS_EINVAL, the session left as it was: negative every, start, stop or max_moves,
 * max_moves == 0 with every > 0, floats that are not finite, alpha_dead outside
 * [0, 255], grad_min < 0, log_shrink < 0, more than 65535 candidates. */
int ggs_refine_set_density(void* handle, const ggs_refine_density* density /* NULL = off */);
/* Synchronises.  acc_BN [B,N] and *n_acc as they stand; moves_B / splits_B [B]: pairs
 * moved / of them split since ggs_refine_set_density; last_pairs_B_M_2 [B,M,2]
 * (M = min(max_moves, N / 2)): the last event's (dead, source) rows, (-1, -1) past
 * last_n_B[b].  Any pointer may be NULL.  GGS_EINVAL while density control is off. */
int ggs_refine_density_read(void* handle, float* acc_BN, int32_t* n_acc, int64_t* moves_B, int64_t* splits_B,
                            int32_t* last_pairs_B_M_2, int32_t* last_n_B);
/* Stage export (host arrays): one event's rank and apply kernels on x, m, v [B,N,9]
 * and acc [B,N] -> x_out, m_out, v_out [B,N,9], pairs [B,M,2] ((-1, -1) past
 * n_pairs[b]), n_pairs [B], is_split [B,M], M = min(max_moves, N / 2).  every == 0:
 * the identity.  GGS_EINVAL before any device is touched: ggs_refine_set_density's
 * parameter rules, a NULL params or array (pairs and is_split may be NULL when M is 0),
 * B or N < 1, B > 65535, B * N * 9 >= 2^31, H or W < 1, n_acc < 0, log_lo > log_hi or
 * either a NaN. */
int ggs_density_relocate(int32_t device, const float* x, const float* m, const float* v, const float* acc,
                         int32_t n_acc, int32_t B, int32_t N, int32_t H, int32_t W, float log_lo, float log_hi,
                         const ggs_refine_density* params, float* x_out, float* m_out, float* v_out,
                         int32_t* pairs, int32_t* n_pairs, int32_t* is_split);

/* ---- residual-driven placement: seeding from the target ------------
 * Where a render misses its target, and the splat to put there.  ggs/seed.py cell_grid /
 * place_sites are the numpy statement the device is held to bit for bit.  Float32, every
 * operation rounded once in the written order, division correctly rounded.
 *   pixel   d = img[b] - targets[b / group] per channel (img NULL: the constant bg);
 *           e = (dr dr + dg dg) + db db, then e = w e with w = weights[b / group] when
 *           weights are given.
 *   cell    the canvas in cells of c x c pixels, Gy = ceil(H / c) by Gx = ceil(W / c),
 *           cell index gy Gx + gx.  A pixel past the image contributes +0.0 and is not
 *           counted.  Each of the cell's c pixel columns is summed over y ascending from
 *           +0.0; the c column sums are reduced by the balanced tree v = v[0::2] + v[1::2]
 *           repeated (adjacent pairs, then pairs of pairs), which is what a lane
 *           xor-butterfly with strides 1, 2, 4, ... computes.  err is that sum of e; the
 *           three target channels are summed in the same order; count is the number of
 *           in-image pixels; the peak is the cell's pixel of largest e, ties to the
 *           smaller (y, x).
 *   sites   a cell is eligible iff err > err_min (a NaN is not); the eligible cells
 *           descending by err, ties to the lower cell index; the first
 *           n = min(max_sites, #eligible) are the sites.  A perfect render gives none.
 *   rows    site j < n writes axes-angle row rows[b][j] (rows NULL: first_row + j):
 *           x = float(px) / float(max(W - 1, 1)), y = float(py) / float(max(H - 1, 1)),
 *           log a = log b = log_sigma (the caller clips it to the scale bounds),
 *           theta = 0, colour c = clip(255 (sum_c / float(count)), 0, 255), alpha = alpha.
 *           Slots j >= n leave their rows untouched; sites[b][j] is the cell, -1 past n.
 *           Two slots of one candidate naming the same row is not a supported input.
 * Images that are not finite are not a supported input.  Deterministic: reruns and other
 * batches give a candidate the same bits. */
typedef struct ggs_seed_params {
    int32_t cell;         /* c: 2, 4, 8, 16, 32 or 64 */
    int32_t max_sites;    /* M >= 1: sites per candidate */
    int32_t first_row;    /* first row written when no row list is given; first_row + M <= N */
    float err_min;        /* >= 0 */
    float log_sigma;
    float alpha;          /* in [0, 255] */
} ggs_seed_params;
/* One placement on device arrays, enqueued on `stream` with no host synchronisation:
 * d_img_bhw3 [B,H,W,3] or NULL (bg: host, three floats, NULL = 1, 1, 1), d_targets_khw3
 * [K,H,W,3], d_weights_khw [K,H,W] or NULL (1), d_rows_BM int32 [B,M] or NULL,
 * d_genomes_BN9 [B,N,9] updated in place or NULL (sites only; N is then not read),
 * d_sites_BM int32 [B,M], d_n_B int32 [B], d_err_BG [B, Gy Gx] or NULL.  GGS_EINVAL
 * before any device is touched: a NULL params, targets, sites or n, a cell size not
 * listed, max_sites < 1, first_row < 0 or first_row + max_sites > N (with genomes and no
 * row list), floats that are not finite, err_min < 0, alpha outside [0, 255], the group
 * rule of ggs_fitness_device_planset (group >= 1, B % group == 0, B / group <= K), B, K,
 * H or W < 1, N < 1 with genomes, B > 65535, B N 9, B Gy Gx or B max_sites >= 2^31.  A
 * row of a device row list outside [0, N) is skipped on the device. */
int ggs_seed_sites_device(int32_t device, void* stream, const float* d_img_bhw3, const float* bg,
                          const float* d_targets_khw3, const float* d_weights_khw, int32_t B, int32_t K,
                          int32_t group, int32_t H, int32_t W, const ggs_seed_params* params,
                          const int32_t* d_rows_BM, float* d_genomes_BN9, int32_t N, int32_t* d_sites_BM,
                          int32_t* d_n_B, float* d_err_BG);
/* Stage export (host arrays): one placement on genomes [B,N,9] -> genomes_out [B,N,9]
 * (both may be NULL together: sites only), sites [B,M], n [B], err [B, Gy Gx] (may be
 * NULL).  The rules above, and a row of rows_BM outside [0, N) or one of genomes and
 * genomes_out NULL alone, are GGS_EINVAL before any device is touched; a refused call
 * leaves its outputs alone. */
int ggs_seed_sites(int32_t device, const float* img_bhw3, const float* bg, const float* targets_khw3,
                   const float* weights_khw, int32_t B, int32_t K, int32_t group, int32_t H, int32_t W,
                   const ggs_seed_params* params, const int32_t* rows_BM, const float* genomes_BN9, int32_t N,
                   float* genomes_out_BN9, int32_t* sites_BM, int32_t* n_B, float* err_BG);
/* Greedy coarse-to-fine seeding of K images at once.  Every genome starts as N empty
 * rows (0.5, 0.5, scale_log_lo, scale_log_lo, 0, 0, 0, 0, 0): alpha 0 blends as the
 * identity, so N empty rows render exactly the background.  Round r renders the genomes
 * as they stand (axes layout, k_sigma, bg), finds up to count sites of cell size cell
 * against image k (err_min) and writes them to the next count rows, the rounds' rows
 * following one another from row 0; rows a round could not place stay empty.  Coarse
 * rounds first put the fine splats on top in compositing order.  All rounds are enqueued
 * on one stream with one synchronisation at the end.  genomes_KN9 [K,N,9]; placed_RK
 * int32 [n_rounds, K]: the rows each round wrote (may be NULL).  A round with count 0 is
 * skipped (placed 0).  GGS_EINVAL before any device is touched: NULL targets, rounds
 * or genomes, n_rounds < 1, a round with a cell size not listed, a negative count, a
 * log_sigma that is not finite or an alpha outside [0, 255], counts that do not sum to
 * N, err_min < 0 or not finite, scale_log_lo not finite, K, N, H or W < 1, K > 65535 and
 * ggs_render's size limits. */
typedef struct ggs_seed_round {
    int32_t cell;
    int32_t count;
    float log_sigma;
    float alpha;
} ggs_seed_round;
int ggs_seed_genomes(int32_t device, const float* targets_khw3, const float* weights_khw, int32_t K, int32_t H,
                     int32_t W, int32_t N, const ggs_seed_round* rounds, int32_t n_rounds, float err_min,
                     float scale_log_lo, float k_sigma, const float* bg, float* genomes_KN9, int32_t* placed_RK);

/* ---- memetic generations of an island group ----------------------
 * After the survivors of every generation g with g % every == 0 (g counts
 * absolutely, as migrate_every does), and after that generation's migration if
 * one is due, every island's n_rows best-ranked rows (ascending fitness, ties by
 * lower row, from the fitness as it stands then) are polished at once: row of
 * rank j of island k is refine candidate k * n_rows + j, started from the row with
 * zero moments and t from 1, taken through n_steps steps exactly as ggs_refine_run
 * takes them and ggs_refine_read's closing evaluation, against island k's image
 * (the one target of a shared-target group).  The candidate's best individual and
 * best fitness overwrite the row and its fitness iff that fitness is strictly
 * lower than the row's; otherwise the row keeps its bits.  A polished row is, bit
 * for bit, best / best_fits of a refine session started on it; moments do not
 * survive from one polish to the next.  Then the island's elite list is re-ranked
 * from the new fitness vector and its best so far updated by the GA's rule
 * (fit + 1e-10 < best in float64, the first lowest row); curves already written
 * are not touched.  All of it is enqueued on the session's stream, one prep ->
 * raster -> finalize -> strip -> finish chain per step for all K * n_rows
 * candidates, with no host synchronisation.  A generation followed by a polish is
 * closed unfused, like one followed by a migration (GGS_GA_UNFUSED=1: the same
 * bits).  A setting holds for the generations run after the call: one already run
 * and not yet closed is closed first, under the setting it ran with.
 * every == 0, n_steps == 0 or polish == NULL: off, the session's bits
 * are those of one that never called this.  The buffers are allocated here.  A
 * negative field, n_rows outside [1, max(1, elite_k)] and ggs_refine_create's
 * parameter rules are GGS_EINVAL, a candidate's strip partials above the gradient's
 * workspace budget GGS_ENOMEM; the session is then left as it was.  ggs/ga.py
 * polish_elites is the numpy statement the device is held to bit for bit. */
typedef struct ggs_ga_polish {
    int32_t every;      /* generations between polishes (absolute count, like migrate_every); 0 = never */
    int32_t n_steps;    /* Adam steps per polish; 0 = never */
    int32_t n_rows;     /* best-ranked rows per island, 1 <= n_rows <= max(1, elite_k) */
    ggs_refine_params adam;
} ggs_ga_polish;
int ggs_ga_islands_set_polish(void* handle, const ggs_ga_polish* polish /* NULL = off */);

/* ---- multi-GPU fitness gather -------------------------------
 * One process per GPU; candidates are sharded in contiguous blocks and the only
 * exchange is an all-gather of each rank's fitness scalars over RCCL (xGMI).
 * Replaces nothing in the reference (single-device, render.py:4); it is the
 * collective of the sharded fitness_population (fitness.py:34-47).  RCCL is
 * loaded at first use (the copy already in the process, else $GGS_RCCL, else the
 * one beside the HIP runtime, by absolute path) and must come from the HIP
 * runtime's directory.  Rank 0 makes the id, every rank passes the same bytes. */
#define GGS_COMM_ID_BYTES 128
int ggs_comm_unique_id(uint8_t* id128);
int ggs_comm_create(int32_t device, int32_t nranks, int32_t rank, const uint8_t* id128, void** comm);
/* recv[r*count + i] = rank r's send[i] (device pointers).  overlap = 0: enqueued
 * on `stream` after the work already there; *ticket = -1.  overlap = 1: runs on
 * the communicator's own stream once the work already on `stream` is done, and
 * `stream` continues at once; *ticket names it for ggs_comm_wait (the caller
 * must not overwrite d_send or read d_recv before waiting). */
int ggs_comm_allgather(void* comm, void* stream, const float* d_send, float* d_recv, int64_t count,
                       int32_t overlap, int64_t* ticket);
/* Make `stream` wait (on the device, no host sync) for the gather `ticket`;
 * valid for the 64 most recent tickets. */
int ggs_comm_wait(void* comm, void* stream, int64_t ticket);
int ggs_comm_size(void* comm, int32_t* nranks, int32_t* rank);
/* What RCCL itself reports for `comm` (ncclCommCount, ncclCommUserRank,
 * ncclCommCuDevice); GGS_EINVAL for a loopback communicator (no RCCL). */
int ggs_comm_info(void* comm, int32_t* nranks, int32_t* rank, int32_t* device);
/* Provenance of the runtimes in this process, as JSON into buf[cap]: the HIP
 * runtime libggs is bound to (path, version), the RCCL libggs loaded (path,
 * version; null before the first communicator) and whether both come from one
 * directory.  RCCL is always loaded from the HIP runtime's directory and a mixed
 * pair is refused (ggs_comm_* fail with GGS_ENODEV).  Returns 0, or the buffer
 * size needed (> 0) when cap is too small. */
int ggs_runtime_info(char* buf, int32_t cap);
void ggs_comm_destroy(void* comm);
/* Single-process communicators over the n listed devices (ncclCommInitAll; no id
 * exchange): comms[i] is rank i on devices[i].  The host API uses this for its
 * own multi-device fan-out (ggs_fitness with n_devices > 1). */
int ggs_comm_init_local(int32_t n, const int32_t* devices, void** comms);
/* Loopback group (test rig, no RCCL): n communicators on ONE device of this
 * process acting as ranks 0..n-1 of one job, so a one-GPU box runs the sharded
 * paths (rank != 0, uneven and empty shards, ggs_ga_set_comm's fingerprint
 * check).  Device all-gathers are matched by call order: every rank calls once
 * per gather (lockstep; a second call before all ranks called fails), the last
 * call enqueues the shard copies on every rank's stream — so d_recv on rank r's
 * stream is defined only after EVERY rank has called for that gather (work a
 * rank queues on its stream before then does not see it).  A HIP failure while
 * the last call enqueues poisons the group (every later call fails).  Host all-gathers /
 * barriers block until all n ranks (on their own host threads) arrived, at most
 * GGS_LOOPBACK_TIMEOUT_S seconds (default 60), then fail. */
int ggs_comm_init_loopback(int32_t device, int32_t n, void** comms);
/* Host-pointer all-gather (synchronous): recv[r*count + i] = rank r's send[i].
 * Staged through the communicator's own device buffer and stream; for small
 * control values (timings, session fingerprints).  count = 0: a barrier. */
int ggs_comm_allgather_host(void* comm, const float* send, float* recv, int64_t count);
/* Returns once every rank of `comm` has called it (host-side barrier). */
int ggs_comm_barrier(void* comm);

/* ---- per-kernel timing (HIP events on the launch stream) --------------------
 * When enabled, every launch of "prep", "raster" and "finalize" is bracketed
 * by hipEvents; ggs_profile_read synchronises those events and returns the
 * accumulated milliseconds and launch count for the named kernel (a finalize
 * folded into the raster counts as raster time, no finalize launch).  A DE
 * session's variation counts as "prep" and its select launch as "select"; one
 * density-control event of a refine session (rank, apply, accumulator reset) as "density";
 * one placement (ggs_seed_*: cell, rank and apply, not the render before it) as "seed". */
int ggs_profile_enable(int32_t on);
int ggs_profile_read(const char* kernel, double* total_ms, int64_t* launches);
void ggs_profile_reset(void);

/* The number of pooled per-stream pipeline workspaces that device's context holds,
 * or a negative GGS_E* code.  A session's stream has one while the session lives and
 * none after its destroy: a leak check that does not depend on free device memory,
 * which other processes on the same GPU change. */
int ggs_workspace_count(int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* GGS_H_ */
