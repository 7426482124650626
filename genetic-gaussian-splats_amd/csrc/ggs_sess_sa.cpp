// Device-resident simulated annealing: lone sessions (ggs_sa_*) and chain groups
// (ggs_sa_chains_*); kernels in ggs_sa.hip.  Declared in include/ggs.h.
#include "ggs_host.h"

namespace ggs {
namespace {

// The SA state keeps, besides the current genome, its splat records and its
// per-strip partials: a neighbour is then evaluated incrementally — only the
// strips a changed splat (old or new AABB) touches are rasterised, the others
// keep the current partial (bit-identical to a full evaluation: same cull list,
// same blend order).  annealing.py:121-146 re-renders the whole canvas per try.
struct SaSession : Session {
    using Session::Session;
    int N = 0, cap = 0, last_n = 0, nTiles = 0;
    bool incremental = false;   // measured slower at every SA config tried
    int dirty_rule = 1;         // 1: a splat is changed when its raster record is; 0: its genes (GGS_SA_DIRTY_RULE)
    // cur_recs / cur_part describe the current state (create evaluates them, commit and
    // an incremental device run install them); a non-incremental ggs_sa_run may
    // accept neighbours without installing them
    bool cur_cache_valid = true;
    DevBuf curr, best, nb, nb_fits, draws;
    DevBuf cur_recs, nb_recs, nb_bnds, cur_part, nb_part, dirty, counters;
    DevBuf loop, sit, curves;       // device SA loop (ggs_sa_run): state, per-iteration table, curves
    DevBuf flags, sizes;            // ... and its mutation scratch (per-try mask-group flags, splat sizes)
    PinBuf pin_fits, pin_counters, pin_loop;
    float* h_fits() const { return (float*)pin_fits.p; }
    unsigned* h_counters() const { return (unsigned*)pin_counters.p; }   // [0] changed splats (last propose)
    SaLoopDev* h_loop() const { return (SaLoopDev*)pin_loop.p; }         // copy of the loop state
    uint64_t n_changed = 0, n_proposed = 0;
    int driver = 0;                 // 1: ggs_sa_propose/commit, 2: ggs_sa_run (not mixed)
};

// prep -> [dirty] -> raster -> finalize for n genomes G; records / partials / fitness
// land in recs / part / fits.  dirty != null: incremental against the current state.
// bnds: the records' cull bounds (scratch for the current state's evaluation).
int sa_eval(SaSession* s, const float* G, int n, SplatRec* recs, int4* bnds, float* part, float* fits, bool dirty,
            bool have_recs = false) {
    const ggs_ga_config& c = s->cfg;
    if (!have_recs) {
        ProfScope ps(s->st, 0);
        GGS_HIP(launch_prep(s->st, true, G, (int64_t)n * s->N, 9, c.H, c.W, c.k_sigma, recs, bnds, nullptr,
                            nullptr, nullptr));
    }
    if (dirty)
        GGS_HIP(launch_dirty(s->st, (const float*)s->curr.p, G, (const SplatRec*)s->cur_recs.p, recs, n,
                             s->N, c.H, c.W, (unsigned char*)s->dirty.p, (unsigned*)s->counters.p, nullptr,
                             s->dirty_rule));
    return raster_fitness(s->st, s->c->simds, recs, bnds, n, s->N, c.H, c.W, (const float4*)s->plan.p, part,
                          (const float*)s->wpart.p, c.fitness_mode, (const int*)s->order.p, s->fctr, fits, false,
                          dirty ? (const unsigned char*)s->dirty.p : nullptr, (const float*)s->cur_part.p);
}

// ---- the round driver of ggs_sa_run and ggs_sa_chains_run ---------------------------
int sa_check_run(int first_it, int n_its, int tries, const double* temps, int width, int cap,
                 const double* curves_out) {
    if (first_it < 0 || n_its < 0 || tries < 1) return fail(GGS_EINVAL, "need first_it >= 0, n_its >= 0, tries >= 1");
    if (n_its > 0 && (!temps || !curves_out)) return fail(GGS_EINVAL, "null temps / curves");
    if (width < 0 || width > cap) return fail(GGS_EINVAL, "width=%d outside [0, %d]", width, cap);
    if ((int64_t)(first_it + (int64_t)n_its) * tries > INT32_MAX)
        return fail(GGS_EINVAL, "iterations x tries must stay below 2^31");
    return GGS_OK;
}

int64_t sa_rounds(int64_t remaining, int32_t est, int64_t cap) {   // ceil(remaining / est) in [1, cap]
    const int64_t e = std::max<int64_t>(1, est);
    return std::min<int64_t>(cap, std::max<int64_t>(1, (std::max<int64_t>(remaining, 0) + e - 1) / e));
}
// Diagnostic override of the bound (tools/probe/sa_pmc_r03b.sh reproduces the
// round-2 crash with it lifted); not part of the C ABI.
int64_t sa_rounds_per_sync(int64_t remaining, int32_t est) {
    static const int64_t cap = [] {
        const char* v = getenv("GGS_SA_MAX_ROUNDS_PER_SYNC");
        return v ? std::max<int64_t>(1, atoll(v)) : (int64_t)GGS_SA_MAX_ROUNDS_PER_SYNC;
    }();
    return sa_rounds(remaining, est, cap);
}

// Adaptive width (sa_width_rule): a round's fixed cost in neighbour evaluations,
// half the number of candidates whose strip waves fit in the GPU's raster wave
// slots (CUs x 4 SIMDs x 3 waves): small canvases add neighbours almost for free
// until the chip fills.  2048^2 (2,048 strips): 0.75 — measured at configs[4],
// start of a run, a round of 1 neighbour costs 191 us and of 2 297 us (r = 0.81);
// 512^2 (128 strips): 12
double sa_width_r(int nTiles) {
    static const double wave_slots = [] {
        int dev = 0, cus = 256;
        if (hipGetDevice(&dev) == hipSuccess)
            (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        return 12.0 * (double)cus;
    }();
    return std::max(0.25, 0.5 * wave_slots / (double)(4 * nTiles));
}

struct SaChunk {                // what the driver hands a session's launches
    const SaItDev* sit;         // [K][n] the iteration table (device)
    int64_t pos0, end;          // the chunk's tries, the same for every chain
    double width_r;
    GaParamsDev prm;            // mutate-only; sigmas replaced per neighbour from sit
    SaRoundDev rd;              // what every session sets; gcap is the driver's
};

// One chunk of iterations [first_it, first_it + n) over the K loop states of session
// s (SaSession: K = 1; SaChains), temps[k * tstride + i] and curves_out[(k * tstride
// + i) * 2 + {0, 1}].  The session supplies its launches: begin(x, bw), the chunk's
// start and flags (bw: the first round's width); round(x, gcap), one round in grids
// of gcap neighbours per chain; finish(), its read-backs ahead of the final sync.
// est_with_width: after a sync the lone loop sizes a batch by the remaining tries
// over the pending round's live count, the group over max(batch width, live).  The
// sync cadence and the `rounds` / `evaluated` counters follow, so each keeps its own.
template <class S, class Begin, class Round, class Finish>
int sa_drive(S* s, int K, int first_it, int n, int total_iters, int tries, const double* temps, int tstride,
             int width, double* curves_out, bool est_with_width, Begin begin, Round round, Finish finish) {
    const ggs_ga_config& c = s->cfg;
    std::vector<SaItDev> tab((size_t)K * n);
    for (int i = 0; i < n; ++i) {
        const GaParamsDev q = ga_params(c, first_it + i, total_iters);
        for (int k = 0; k < K; ++k)
            tab[(size_t)k * n + i] = SaItDev{{q.sig_xy, q.sig_alog, q.sig_blog, q.sig_theta, q.sig_rgb, q.sig_alpha},
                                             {0.f, 0.f}, temps[(size_t)k * tstride + i]};
    }
    SaChunk x{};
    x.pos0 = (int64_t)first_it * tries;
    x.end = x.pos0 + (int64_t)n * tries;
    const int64_t end = x.end;
    int rc;
    if ((rc = ensure(s->sit, sizeof(SaItDev) * tab.size(), s->st)) ||
        (rc = ensure(s->curves, sizeof(double) * 2 * tab.size(), s->st)) ||
        (rc = ensure(s->flags, sizeof(int) * (size_t)(end - x.pos0) * K, s->st)))
        return rc;
    x.sit = (const SaItDev*)s->sit.p;
    GGS_HIP(hipMemcpyAsync(s->sit.p, tab.data(), sizeof(SaItDev) * tab.size(), hipMemcpyHostToDevice, s->st));
    x.width_r = sa_width_r(s->nTiles);
    // Width of a batch of rounds: the rule's width at the acceptance rates of the
    // last sync, used by every round of the batch and the size of their mutation
    // and raster grids — not the session capacity with the width chosen per round
    // on the device: unused neighbour slots are not free (a lone 2048^2 neighbour in
    // a 16-slot grid ran 216 us per round instead of 191: the early-exit strip waves
    // of the other slots stream through the free wave slots beside it).  The
    // unfinished chains share a round, so its fixed cost is divided among them, at
    // their mean acceptance rate.  The pending round (computed by the
    // previous batch) keeps its width.
    SaLoopDev* h = s->h_loop();
    bool fresh = true;              // before the chunk's first sync: every chain is unfinished
    auto unfinished = [&](int k) { return fresh || h[k].pos < end; };
    auto batch_width = [&]() {
        if (width > 0) return std::min(s->cap, width);
        double p = 0.0;
        int u = 0;
        for (int k = 0; k < K; ++k)
            if (unfinished(k)) { p += h[k].acc_rate; ++u; }
        u = std::max(u, 1);
        return std::min(s->cap, std::max(1, sa_width_rule(p / u, s->cap, x.width_r / u)));
    };
    int bw = batch_width(), gcap = bw;
    x.prm = ga_params(c, first_it, total_iters);
    x.prm.mutate_only = 1;
    x.prm.o_base = 0;
    x.rd.partials = (const float*)s->nb_part.p;
    x.rd.wpartials = (const float*)s->wpart.p;
    x.rd.nslots = 4 * s->nTiles;
    x.rd.mode = c.fitness_mode;
    x.rd.N = s->N;
    x.rd.hw = (double)c.H * (double)c.W;
    x.rd.fits_out = (float*)s->nb_fits.p;
    x.rd.mutpb = c.mutpb;
    x.rd.curves = (double*)s->curves.p;
    x.rd.curr = (float*)s->curr.p;
    x.rd.best = (float*)s->best.p;
    x.rd.nb = (const float*)s->nb.p;
    if ((rc = begin(x, bw))) return rc;
    // Rounds are enqueued in batches with one host sync between batches: a round
    // consumes at most its width of a chain's tries, so ceil(longest remaining /
    // width) rounds never overshoot the chunk (rounds past its end would be empty
    // launches anyway).  A batch holds at most GGS_SA_MAX_ROUNDS_PER_SYNC rounds
    // (ggs_sa_rounds_per_sync): unbounded, a 256-iteration chunk at high acceptance
    // queued ~1,000 rounds = 4,000 dispatches behind one sync, and rocprofv3's PMC
    // dispatch interception crashed the host thread inside the launch call
    // (docs/EXPERIMENTS.md §9).
    int64_t remaining = end - x.pos0;
    int est = gcap;
    for (;;) {
        int64_t R = sa_rounds_per_sync(remaining, est);
        // the batch width comes from the acceptance rates at this sync: while a
        // rate has little history (a session's first tries) sync every 2 rounds
        uint64_t ev = UINT64_MAX;
        for (int k = 0; k < K; ++k)
            if (unfinished(k)) ev = std::min<uint64_t>(ev, h[k].evaluated);
        if (ev < 64) R = std::min<int64_t>(R, 2);
        x.rd.gcap = bw;
        for (int64_t r = 0; r < R; ++r) {
            if ((rc = round(x, gcap))) return rc;
            gcap = bw;                  // after the pending round: every round has width bw
        }
        GGS_HIP(hipMemcpyAsync(h, s->loop.p, sizeof(SaLoopDev) * K, hipMemcpyDeviceToHost, s->st));
        GGS_HIP(hipStreamSynchronize(s->st));
        fresh = false;
        remaining = 0;
        int live = 1;
        for (int k = 0; k < K; ++k) {
            remaining = std::max<int64_t>(remaining, end - h[k].pos);
            live = std::max(live, (int)h[k].live);
        }
        if (remaining <= 0) break;
        bw = batch_width();
        gcap = std::max(bw, live);      // the grids also hold the pending round
        est = est_with_width ? gcap : live;
    }
    std::vector<double> hc(2 * tab.size());
    GGS_HIP(hipMemcpyAsync(hc.data(), s->curves.p, sizeof(double) * hc.size(), hipMemcpyDeviceToHost, s->st));
    if ((rc = finish())) return rc;
    GGS_HIP(hipStreamSynchronize(s->st));
    for (int k = 0; k < K; ++k)
        memcpy(curves_out + 2 * (size_t)k * tstride, hc.data() + 2 * (size_t)k * n, sizeof(double) * 2 * (size_t)n);
    return GGS_OK;
}


}  // namespace
}  // namespace ggs

using namespace ggs;

extern "C" {

// ---- simulated annealing ------------------------------------------------------
int ggs_sa_create(int32_t device, const ggs_ga_config* cfg, const float* target_hw3,
                  const float* mask_hw, const float* init_ind, void** handle, float* init_fit) {
    if (!cfg || !target_hw3 || !init_ind || !handle) return fail(GGS_EINVAL, "null argument");
    int rc = ga_check_config(*cfg, mask_hw, true);
    if (rc) return rc;
    DevCtx* ctx = nullptr;
    if ((rc = get_ctx(device, &ctx))) return rc;
    auto s = std::make_unique<SaSession>(ctx, *cfg);
    s->N = cfg->n_splats;
    s->cap = cfg->pop_size;
    if (const char* v = getenv("GGS_SA_DIRTY_RULE")) s->dirty_rule = atoi(v) != 0;   // A/B: 0 = genes
    const size_t ib = sizeof(float) * 9 * (size_t)s->N;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg(ctx->dev);
    auto bail = [&](int code) { return fail_session(s, code); };
    if ((rc = s->open(target_hw3, mask_hw, 1, 1, true))) return bail(rc);
    int nTX;
    s->nTiles = raster_tiles(cfg->H, cfg->W, &nTX);
    const size_t slots = 4 * (size_t)s->nTiles, rb = sizeof(SplatRec) * (size_t)std::max(s->N, 1);
    if ((rc = ensure(s->curr, std::max<size_t>(ib, 4), s->st)) || (rc = ensure(s->best, std::max<size_t>(ib, 4), s->st)) ||
        (rc = ensure(s->nb, std::max<size_t>(ib * s->cap, 4), s->st)) ||
        (rc = ensure(s->nb_fits, sizeof(float) * s->cap, s->st)) ||
        (rc = ensure(s->cur_recs, rb, s->st)) || (rc = ensure(s->nb_recs, rb * s->cap, s->st)) ||
        (rc = ensure(s->nb_bnds, rb / 4 * s->cap, s->st)) ||
        (rc = ensure(s->cur_part, sizeof(float) * slots, s->st)) ||
        (rc = ensure(s->nb_part, sizeof(float) * slots * s->cap, s->st)) ||
        (rc = ensure(s->dirty, slots * s->cap, s->st)) ||
        (rc = ensure(s->counters, sizeof(unsigned) * 4, s->st)) || (rc = ensure(s->loop, sizeof(SaLoopDev), s->st)) ||
        (rc = ensure(s->sizes, sizeof(float) * (size_t)std::max(s->N, 1) * s->cap, s->st)) ||
        (rc = ensure_pinned(s->pin_fits, sizeof(float) * s->cap)) ||
        (rc = ensure_pinned(s->pin_counters, sizeof(unsigned) * 4)) ||
        (rc = ensure_pinned(s->pin_loop, sizeof(SaLoopDev))))
        return bail(rc);
    if (hipMemcpyAsync(s->curr.p, init_ind, ib, hipMemcpyHostToDevice, s->st) ||
        hipMemcpyAsync(s->best.p, init_ind, ib, hipMemcpyHostToDevice, s->st) ||
        hipMemsetAsync(s->counters.p, 0, sizeof(unsigned) * 4, s->st))
        return bail(fail(GGS_EHIP, "upload failed"));
    if ((rc = sa_eval(s.get(), (const float*)s->curr.p, 1, (SplatRec*)s->cur_recs.p, (int4*)s->nb_bnds.p,
                      (float*)s->cur_part.p,
                      (float*)s->nb_fits.p, false)))
        return bail(rc);
    if (hipMemcpyAsync(s->h_fits(), s->nb_fits.p, sizeof(float), hipMemcpyDeviceToHost, s->st) ||
        hipStreamSynchronize(s->st))
        return bail(fail(GGS_EHIP, "initial evaluation failed"));
    if (init_fit) *init_fit = s->h_fits()[0];
    // the device loop's state: current = best = the initial energy, no acceptances yet
    *s->h_loop() = SaLoopDev{};
    s->h_loop()->acc_j = -1;
    s->h_loop()->curr_fit = s->h_loop()->best_fit = (double)s->h_fits()[0];
    if (hipMemcpy(s->loop.p, s->h_loop(), sizeof(SaLoopDev), hipMemcpyHostToDevice) != hipSuccess)
        return bail(fail(GGS_EHIP, "upload failed"));
    *handle = s.release();
    return GGS_OK;
}

int ggs_sa_propose(void* handle, int32_t it, int32_t total_iters, int32_t first_try, int32_t n,
                   const ggs_ga_draws* draws, float* fits_out) {
    if (!handle || !fits_out) return fail(GGS_EINVAL, "null argument");
    SaSession* s = (SaSession*)handle;
    if (n < 1 || n > s->cap) return fail(GGS_EINVAL, "n=%d outside [1, %d]", n, s->cap);
    if (first_try < 0) return fail(GGS_EINVAL, "first_try must be >= 0");
    if (s->driver == 2) return fail(GGS_EINVAL, "this SA session is driven by ggs_sa_run");
    std::lock_guard<std::mutex> lk(s->c->mu);
    s->driver = 1;
    DeviceGuard dg(s->c->dev);
    GaDrawsDev d{};
    int rc;
    if (draws && (rc = ga_upload_draws(s->draws, s->st, n, s->N, 1, true, draws, &d))) return rc;
    GaParamsDev prm = ga_params(s->cfg, it, total_iters);
    prm.mutate_only = 1;
    prm.o_base = first_try;
    // The neighbours and their raster records.  The variation kernel runs one
    // workgroup per neighbour; fusing the prep into it pays while that leaves few
    // splats per thread, but a handful of 4,096-splat neighbours (configs[4]) would
    // prep 16 splats per thread on a few CUs (99 us): then the prep kernel runs
    // separately, one thread per splat (same ggs_prep.h math, same bits).
    const bool fuse_prep = s->N <= 1024 || n >= 64;
    {
        ProfScope ps(s->st, 0);
        GGS_HIP(launch_ga_variation(s->st, (const float*)s->curr.p, nullptr, 1, s->N, prm, d, s->cfg.seed, it,
                                    (float*)s->nb.p, n, fuse_prep ? (SplatRec*)s->nb_recs.p : nullptr,
                                    (int4*)s->nb_bnds.p,
                                    s->cfg.H, s->cfg.W, s->cfg.k_sigma));
    }
    if ((rc = sa_eval(s, (const float*)s->nb.p, n, (SplatRec*)s->nb_recs.p, (int4*)s->nb_bnds.p,
                      (float*)s->nb_part.p,
                      (float*)s->nb_fits.p, s->incremental, fuse_prep)))
        return rc;
    GGS_HIP(hipMemcpyAsync(s->h_fits(), s->nb_fits.p, sizeof(float) * n, hipMemcpyDeviceToHost, s->st));
    GGS_HIP(hipMemcpyAsync(s->h_counters(), s->counters.p, sizeof(unsigned), hipMemcpyDeviceToHost, s->st));
    GGS_HIP(hipMemsetAsync(s->counters.p, 0, sizeof(unsigned), s->st));
    GGS_HIP(hipStreamSynchronize(s->st));
    memcpy(fits_out, s->h_fits(), sizeof(float) * n);
    s->n_changed += s->h_counters()[0];
    s->n_proposed += (uint64_t)n;
    s->last_n = n;
    return GGS_OK;
}

int ggs_sa_commit(void* handle, int32_t j, int32_t update_best) {
    if (!handle) return fail(GGS_EINVAL, "null handle");
    SaSession* s = (SaSession*)handle;
    if (j >= s->last_n) return fail(GGS_EINVAL, "neighbour %d not proposed (last n=%d)", j, s->last_n);
    if (s->driver == 2) return fail(GGS_EINVAL, "this SA session is driven by ggs_sa_run");
    std::lock_guard<std::mutex> lk(s->c->mu);
    DeviceGuard dg(s->c->dev);
    const size_t ib = sizeof(float) * 9 * (size_t)s->N;
    if (j >= 0) {   // the accepted neighbour becomes the state: genome, records, strip partials
        const size_t rb = sizeof(SplatRec) * (size_t)s->N, pb = sizeof(float) * 4 * (size_t)s->nTiles;
        GGS_HIP(hipMemcpyAsync(s->curr.p, (const char*)s->nb.p + ib * j, ib, hipMemcpyDeviceToDevice, s->st));
        GGS_HIP(hipMemcpyAsync(s->cur_recs.p, (const char*)s->nb_recs.p + rb * j, rb, hipMemcpyDeviceToDevice,
                               s->st));
        GGS_HIP(hipMemcpyAsync(s->cur_part.p, (const char*)s->nb_part.p + pb * j, pb, hipMemcpyDeviceToDevice,
                               s->st));
    }
    if (update_best) GGS_HIP(hipMemcpyAsync(s->best.p, s->curr.p, ib, hipMemcpyDeviceToDevice, s->st));
    return GGS_OK;
}

int64_t ggs_sa_rounds_per_sync(int64_t remaining, int32_t est) {
    return sa_rounds(remaining, est, GGS_SA_MAX_ROUNDS_PER_SYNC);
}

int ggs_sa_run(void* handle, int32_t first_it, int32_t n_its, int32_t total_iters, int32_t tries,
               const double* temps, int32_t width, double* curves_out) {
    if (!handle) return fail(GGS_EINVAL, "null handle");
    SaSession* s = (SaSession*)handle;
    int rc = sa_check_run(first_it, n_its, tries, temps, width, s->cap, curves_out);
    if (rc) return rc;
    if (s->driver == 1) return fail(GGS_EINVAL, "this SA session is driven by ggs_sa_propose/commit");
    if (n_its == 0) return GGS_OK;
    std::lock_guard<std::mutex> lk(s->c->mu);
    DeviceGuard dg(s->c->dev);
    s->driver = 2;
    if (!s->incremental) s->cur_cache_valid = false;
    const ggs_ga_config& c = s->cfg;
    SaLoopDev* loop = (SaLoopDev*)s->loop.p;
    const float bg[3] = {1.f, 1.f, 1.f};
    const int* live = &loop->live;
    const uint64_t evaluated0 = s->h_loop()->evaluated;
    auto begin = [&](const SaChunk& x, int bw) -> int {
        GGS_HIP(launch_sa_begin(s->st, loop, x.pos0, x.end, tries, first_it, s->cap, width, x.width_r, bw));
        GGS_HIP(launch_sa_flags(s->st, x.pos0, (int)(x.end - x.pos0), tries, c.seed, c.mutpb, s->N, (int*)s->flags.p));
        return GGS_OK;
    };
    // one round: mutate (+ records) and swap, [dirty strips], raster, then one
    // workgroup for fitness, acceptance, install and the next round's flags
    auto round = [&](const SaChunk& x, int gcap) -> int {
        {
            ProfScope ps(s->st, 0);
            GGS_HIP(launch_sa_mutate(s->st, loop, x.sit, x.prm, c.seed, s->N, gcap, (int*)s->flags.p,
                                     (const float*)s->curr.p, (float*)s->nb.p, (float*)s->sizes.p,
                                     (SplatRec*)s->nb_recs.p, (int4*)s->nb_bnds.p, c.H, c.W, c.k_sigma));
        }
        if (s->incremental)
            GGS_HIP(launch_dirty(s->st, (const float*)s->curr.p, (const float*)s->nb.p,
                                 (const SplatRec*)s->cur_recs.p, (const SplatRec*)s->nb_recs.p, gcap, s->N, c.H,
                                 c.W, (unsigned char*)s->dirty.p, (unsigned*)s->counters.p, live, s->dirty_rule));
        {
            ProfScope ps(s->st, 1);
            GGS_HIP(launch_raster(s->st, 1, (const SplatRec*)s->nb_recs.p, (const int4*)s->nb_bnds.p, gcap, s->N,
                                  c.H, c.W, bg, nullptr,
                                  (const float4*)s->plan.p, (float*)s->nb_part.p, (const int*)s->order.p,
                                  s->incremental ? (const unsigned char*)s->dirty.p : nullptr,
                                  (const float*)s->cur_part.p, live, nullptr, s->c->simds));
        }
        SaRoundDev rd = x.rd;       // + the one chain's seed and the incremental path's state
        rd.seed = c.seed;
        rd.cur_recs = s->incremental ? (SplatRec*)s->cur_recs.p : nullptr;
        rd.nb_recs = (const SplatRec*)s->nb_recs.p;
        rd.cur_part = (float*)s->cur_part.p;
        GGS_HIP(launch_sa_accept(s->st, loop, x.sit, rd));
        return GGS_OK;
    };
    auto finish = [&]() -> int {
        if (s->incremental) {
            GGS_HIP(hipMemcpyAsync(s->h_counters(), s->counters.p, sizeof(unsigned), hipMemcpyDeviceToHost, s->st));
            GGS_HIP(hipMemsetAsync(s->counters.p, 0, sizeof(unsigned), s->st));
        }
        return GGS_OK;
    };
    if ((rc = sa_drive(s, 1, first_it, n_its, total_iters, tries, temps, n_its, width, curves_out, false, begin, round,
                       finish)))
        return rc;
    if (s->incremental) s->n_changed += s->h_counters()[0];
    s->n_proposed += s->h_loop()->evaluated - evaluated0;
    return GGS_OK;
}

int ggs_sa_loop_state(void* handle, double* best_fit, double* curr_fit, uint64_t* rounds, uint64_t* evaluated,
                      uint64_t* accepted) {
    if (!handle) return fail(GGS_EINVAL, "null handle");
    SaSession* s = (SaSession*)handle;
    std::lock_guard<std::mutex> lk(s->c->mu);
    const SaLoopDev& l = *s->h_loop();     // as of the end of the last ggs_sa_run (or creation)
    if (best_fit) *best_fit = l.best_fit;
    if (curr_fit) *curr_fit = l.curr_fit;
    if (rounds) *rounds = l.rounds;
    if (evaluated) *evaluated = l.evaluated;
    if (accepted) *accepted = l.accepted;
    return GGS_OK;
}

int ggs_sa_accept_uniform(uint64_t seed, int32_t it, int32_t k, double* u) {
    if (!u || it < 0 || k < 0) return fail(GGS_EINVAL, "bad arguments");
    *u = sa_accept_uniform(seed, (uint32_t)it, (uint32_t)k);
    return GGS_OK;
}

int ggs_sa_set_incremental(void* handle, int32_t on) {
    if (!handle) return fail(GGS_EINVAL, "null handle");
    SaSession* s = (SaSession*)handle;
    std::lock_guard<std::mutex> lk(s->c->mu);
    if (on && !s->incremental && !s->cur_cache_valid) {
        // The device loop installs an accepted neighbour's records and strip
        // partials only while incremental evaluation is on (sa_accept_kernel), so
        // after an incremental-off ggs_sa_run they describe an older state:
        // re-evaluate the current state before the dirty-strip test relies on them.
        // (Right after create, or after propose/commit, they are current: no work.)
        DeviceGuard dg(s->c->dev);
        int rc = sa_eval(s, (const float*)s->curr.p, 1, (SplatRec*)s->cur_recs.p, (int4*)s->nb_bnds.p,
                         (float*)s->cur_part.p, (float*)s->nb_fits.p, false);
        if (rc) return rc;
        GGS_HIP(hipStreamSynchronize(s->st));
        s->cur_cache_valid = true;
    }
    s->incremental = on != 0;
    return GGS_OK;
}

int ggs_sa_stats(void* handle, uint64_t* proposed, uint64_t* changed_splats) {
    if (!handle) return fail(GGS_EINVAL, "null handle");
    SaSession* s = (SaSession*)handle;
    std::lock_guard<std::mutex> lk(s->c->mu);
    if (proposed) *proposed = s->n_proposed;
    if (changed_splats) *changed_splats = s->n_changed;
    return GGS_OK;
}

int ggs_sa_read(void* handle, float* current, float* best, float* neighbours) {
    if (!handle) return fail(GGS_EINVAL, "null handle");
    SaSession* s = (SaSession*)handle;
    std::lock_guard<std::mutex> lk(s->c->mu);
    DeviceGuard dg(s->c->dev);
    const size_t ib = sizeof(float) * 9 * (size_t)s->N;
    GGS_HIP(hipStreamSynchronize(s->st));
    if (current) GGS_HIP(hipMemcpy(current, s->curr.p, ib, hipMemcpyDeviceToHost));
    if (best) GGS_HIP(hipMemcpy(best, s->best.p, ib, hipMemcpyDeviceToHost));
    if (neighbours && s->last_n > 0)
        GGS_HIP(hipMemcpy(neighbours, s->nb.p, ib * s->last_n, hipMemcpyDeviceToHost));
    return GGS_OK;
}

void ggs_sa_destroy(void* handle) { destroy_session<SaSession>(handle); }

}  // extern "C"

// ---- SA chain groups -------------------------------------------------------------
namespace ggs {
namespace {

struct SaChains : Session {
    using Session::Session;
    int K = 0, N = 0, cap = 0, nTiles = 0, exchange_every = 0;
    bool multi = false;             // a target (plan) per chain
    uint64_t exchange_seed = 0;
    int64_t gstride = 0;            // floats between the chains' genomes in curr / best
    DevBuf curr, best, nb, nb_fits, nb_recs, nb_bnds, nb_part;
    DevBuf loop, sit, curves, flags, sizes, seeds, list, swaps;
    PinBuf pin_loop, pin_fits, pin_swaps;
    SaLoopDev* h_loop() const { return (SaLoopDev*)pin_loop.p; }    // [K]
    float* h_fits() const { return (float*)pin_fits.p; }            // [K]
    unsigned long long* h_swaps() const { return (unsigned long long*)pin_swaps.p; }   // [2]: exchange pairs tried / swapped
};

SaChainsDev sc_dev(const SaChains* s, int n_its, int n_tries) {
    SaChainsDev g{};
    g.K = s->K;
    g.n_its = n_its;
    g.n_tries = n_tries;
    g.cap = s->cap;
    g.gstride = s->gstride;
    g.wstride = s->multi ? (int64_t)(plan_wsum_bytes(s->cfg.H, s->cfg.W) / sizeof(float)) : 0;
    g.seeds = (const uint64_t*)s->seeds.p;
    int* l = (int*)s->list.p;       // total (+ 3 of padding), base [K], chain [K * cap], slot [K * cap]
    g.total = l;
    g.base = l + 4;
    g.chain = g.base + s->K;
    g.slot = g.chain + (size_t)s->K * s->cap;
    return g;
}

int sc_check(const ggs_ga_config* cfg, const ggs_sa_chains* ch, const float* target, const float* mask,
             const float* init_inds, void** handle, bool multi) {
    if (!cfg || !ch || !target || !init_inds || !handle) return fail(GGS_EINVAL, "null argument");
    int rc = ga_check_config(*cfg, mask, true);
    if (rc) return rc;
    if (ch->n_chains < 1 || ch->n_chains > GGS_SA_MAX_CHAINS)
        return fail(GGS_EINVAL, "n_chains must be in [1, %d], got %d", GGS_SA_MAX_CHAINS, ch->n_chains);
    if (!ch->seeds) return fail(GGS_EINVAL, "seeds is required ([n_chains])");
    if (ch->exchange_every < 0) return fail(GGS_EINVAL, "exchange_every must be >= 0, got %d", ch->exchange_every);
    if (multi && ch->exchange_every > 0)
        return fail(GGS_EINVAL, "replica exchange needs one shared target: an energy measured on another image "
                                "means nothing (exchange_every=%d)", ch->exchange_every);
    return check_dims((int64_t)ch->n_chains * cfg->pop_size, cfg->n_splats, 9, cfg->H, cfg->W);
}

int sc_create(int32_t device, const ggs_ga_config* cfg, const ggs_sa_chains* ch, const float* target,
              const float* mask, const float* init_inds, void** handle, float* init_fits, bool multi) {
    int rc = sc_check(cfg, ch, target, mask, init_inds, handle, multi);   // before any device call
    if (rc) return rc;
    const ggs_ga_config& c = *cfg;
    DevCtx* ctx = nullptr;
    if ((rc = get_ctx(device, &ctx))) return rc;
    auto s = std::make_unique<SaChains>(ctx, c);
    const int K = s->K = ch->n_chains, N = s->N = c.n_splats;
    s->cap = c.pop_size;
    s->multi = multi;
    s->exchange_every = ch->exchange_every;
    s->exchange_seed = ch->exchange_seed;
    const size_t n9 = 9 * (size_t)N;
    s->gstride = (int64_t)((n9 + 3) & ~(size_t)3);
    const int nplans = multi ? K : 1;
    const size_t B = (size_t)K * s->cap, BN = B * (size_t)std::max(N, 1);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg(ctx->dev);
    auto bail = [&](int code) { return fail_session(s, code); };
    if ((rc = s->open(target, mask, nplans, nplans, true))) return bail(rc);
    int nTX;
    s->nTiles = raster_tiles(c.H, c.W, &nTX);
    const size_t slots = 4 * (size_t)s->nTiles, gb = sizeof(float) * std::max<size_t>((size_t)s->gstride * K, 4);
    if ((rc = ensure(s->curr, gb, s->st)) || (rc = ensure(s->best, gb, s->st)) ||
        (rc = ensure(s->nb, sizeof(float) * std::max<size_t>(n9 * B, 4), s->st)) ||
        (rc = ensure(s->nb_fits, sizeof(float) * B, s->st)) ||
        (rc = ensure(s->nb_recs, sizeof(SplatRec) * BN, s->st)) || (rc = ensure(s->nb_bnds, sizeof(int4) * BN, s->st)) ||
        (rc = ensure(s->nb_part, sizeof(float) * slots * B, s->st)) ||
        (rc = ensure(s->loop, sizeof(SaLoopDev) * K, s->st)) || (rc = ensure(s->sizes, sizeof(float) * BN, s->st)) ||
        (rc = ensure(s->seeds, sizeof(uint64_t) * K, s->st)) ||
        (rc = ensure_zeroed(s->list, sizeof(int) * (4 + (size_t)K + 2 * B), s->st)) ||
        (rc = ensure_zeroed(s->swaps, sizeof(unsigned long long) * 2, s->st)) ||
        (rc = ensure_pinned(s->pin_fits, sizeof(float) * K)) ||
        (rc = ensure_pinned(s->pin_swaps, sizeof(unsigned long long) * 2)) ||
        (rc = ensure_pinned(s->pin_loop, sizeof(SaLoopDev) * K)))
        return bail(rc);
    s->h_swaps()[0] = s->h_swaps()[1] = 0;
    // the K initial individuals, contiguous in the neighbour buffer for their one evaluation
    if (hipMemcpyAsync(s->nb.p, init_inds, sizeof(float) * n9 * K, hipMemcpyHostToDevice, s->st) ||
        hipMemcpyAsync(s->seeds.p, ch->seeds, sizeof(uint64_t) * K, hipMemcpyHostToDevice, s->st))
        return bail(fail(GGS_EHIP, "upload failed"));
    for (int k = 0; k < K && n9; ++k)
        if (hipMemcpyAsync((float*)s->curr.p + k * s->gstride, init_inds + n9 * k, sizeof(float) * n9,
                           hipMemcpyHostToDevice, s->st) ||
            hipMemcpyAsync((float*)s->best.p + k * s->gstride, init_inds + n9 * k, sizeof(float) * n9,
                           hipMemcpyHostToDevice, s->st))
            return bail(fail(GGS_EHIP, "upload failed"));
    // one prep and one raster launch for the K initial energies (chain k against
    // plan k of a plan set: group 1); unfused, as ggs_sa_create evaluates its one
    if (launch_prep(s->st, true, (const float*)s->nb.p, (int64_t)K * N, 9, c.H, c.W, c.k_sigma, (SplatRec*)s->nb_recs.p,
                    (int4*)s->nb_bnds.p, nullptr, nullptr, nullptr) != hipSuccess)
        return bail(fail(GGS_EHIP, "prep launch failed"));
    if ((rc = raster_fitness(s->st, ctx->simds, (const SplatRec*)s->nb_recs.p, (const int4*)s->nb_bnds.p, K, N, c.H, c.W,
                             (const float4*)s->plan.p, (float*)s->nb_part.p, (const float*)s->wpart.p, c.fitness_mode,
                             (const int*)s->order.p, s->fctr, (float*)s->nb_fits.p, false, nullptr, nullptr,
                             multi ? 1 : 0)))
        return bail(rc);
    if (hipMemcpyAsync(s->h_fits(), s->nb_fits.p, sizeof(float) * K, hipMemcpyDeviceToHost, s->st) ||
        hipStreamSynchronize(s->st))
        return bail(fail(GGS_EHIP, "initial evaluation failed"));
    for (int k = 0; k < K; ++k) {
        if (init_fits) init_fits[k] = s->h_fits()[k];
        s->h_loop()[k] = SaLoopDev{};
        s->h_loop()[k].acc_j = -1;
        s->h_loop()[k].curr_fit = s->h_loop()[k].best_fit = (double)s->h_fits()[k];
    }
    if (hipMemcpy(s->loop.p, s->h_loop(), sizeof(SaLoopDev) * K, hipMemcpyHostToDevice) != hipSuccess)
        return bail(fail(GGS_EHIP, "upload failed"));
    *handle = s.release();
    return GGS_OK;
}

// One chunk of iterations [first_it, first_it + n) for every chain, no exchange
// inside it.  temps[k * tstride + i], curves_out[(k * tstride + i) * 2 + {0, 1}].
int sc_run_chunk(SaChains* s, int first_it, int n, int total_iters, int tries, const double* temps, int tstride,
                 int width, double* curves_out) {
    const ggs_ga_config& c = s->cfg;
    const SaChainsDev g = sc_dev(s, n, n * tries);
    SaLoopDev* loop = (SaLoopDev*)s->loop.p;
    const float bg[3] = {1.f, 1.f, 1.f};
    auto begin = [&](const SaChunk& x, int bw) -> int {
        GGS_HIP(launch_sa_chains_begin(s->st, g, loop, x.pos0, x.end, tries, first_it, width, x.width_r, bw));
        GGS_HIP(launch_sa_chains_flags(s->st, g, x.pos0, tries, c.mutpb, s->N, (int*)s->flags.p));
        return GGS_OK;
    };
    // one round: mutate + swap over the listed neighbours, one raster launch over
    // exactly that many candidates, the chains' accept workgroups, the next list
    auto round = [&](const SaChunk& x, int gcap) -> int {
        const int B = s->K * gcap;
        {
            ProfScope ps(s->st, 0);
            GGS_HIP(launch_sa_chains_mutate(s->st, g, loop, x.sit, x.prm, s->N, B, (const int*)s->flags.p,
                                            (const float*)s->curr.p, (float*)s->nb.p, (float*)s->sizes.p,
                                            (SplatRec*)s->nb_recs.p, (int4*)s->nb_bnds.p, c.H, c.W, c.k_sigma));
        }
        {
            ProfScope ps(s->st, 1);
            if (s->multi)
                GGS_HIP(launch_chain_strips(s->st, (const SplatRec*)s->nb_recs.p, (const int4*)s->nb_bnds.p, B, s->N,
                                            c.H, c.W, (const float4*)s->plan.p, (float*)s->nb_part.p,
                                            (const int*)s->order.p, g.total, g.chain, s->c->simds));
            else
                GGS_HIP(launch_raster(s->st, 1, (const SplatRec*)s->nb_recs.p, (const int4*)s->nb_bnds.p, B, s->N, c.H,
                                      c.W, bg, nullptr, (const float4*)s->plan.p, (float*)s->nb_part.p,
                                      (const int*)s->order.p, nullptr, nullptr, g.total, nullptr, s->c->simds));
        }
        GGS_HIP(launch_sa_chains_accept(s->st, g, loop, x.sit, x.rd));
        return GGS_OK;
    };
    return sa_drive(s, s->K, first_it, n, total_iters, tries, temps, tstride, width, curves_out, true, begin, round,
                    [] { return (int)GGS_OK; });
}

}  // namespace
}  // namespace ggs

extern "C" {

int ggs_sa_chains_create(int32_t device, const ggs_ga_config* cfg, const ggs_sa_chains* chains,
                         const float* target_hw3, const float* mask_hw, const float* init_inds, void** handle,
                         float* init_fits) {
    return ggs::sc_create(device, cfg, chains, target_hw3, mask_hw, init_inds, handle, init_fits, false);
}

int ggs_sa_chains_create_targets(int32_t device, const ggs_ga_config* cfg, const ggs_sa_chains* chains,
                                 const float* targets_khw3, const float* masks_khw, const float* init_inds,
                                 void** handle, float* init_fits) {
    return ggs::sc_create(device, cfg, chains, targets_khw3, masks_khw, init_inds, handle, init_fits, true);
}

int ggs_sa_chains_run(void* handle, int32_t first_it, int32_t n_its, int32_t total_iters, int32_t tries,
                      const double* temps, int32_t width, double* curves_out) {
    if (!handle) return fail(GGS_EINVAL, "null handle");
    SaChains* s = (SaChains*)handle;
    if (int rc = sa_check_run(first_it, n_its, tries, temps, width, s->cap, curves_out)) return rc;
    if (n_its == 0) return GGS_OK;
    std::lock_guard<std::mutex> lk(s->c->mu);
    DeviceGuard dg(s->c->dev);
    // the range in chunks that end where an exchange is due (all of it without exchange)
    const int M = s->K >= 2 ? s->exchange_every : 0;
    for (int done = 0; done < n_its;) {
        const int it0 = first_it + done;
        int n = n_its - done;
        if (M > 0) n = std::min(n, M - it0 % M);
        int rc = sc_run_chunk(s, it0, n, total_iters, tries, temps + done, n_its, width, curves_out + 2 * (size_t)done);
        if (rc) return rc;
        const int it = it0 + n - 1;
        if (M > 0 && (it + 1) % M == 0) {
            const SaChainsDev g = sc_dev(s, n, n * tries);
            GGS_HIP(launch_sa_chains_exchange(s->st, g, (SaLoopDev*)s->loop.p, (const SaItDev*)s->sit.p, n - 1, it,
                                              s->exchange_seed, (it + 1) / M - 1, s->N, (float*)s->curr.p,
                                              (float*)s->best.p, (unsigned long long*)s->swaps.p));
            GGS_HIP(hipMemcpyAsync(s->h_loop(), s->loop.p, sizeof(SaLoopDev) * s->K, hipMemcpyDeviceToHost, s->st));
            GGS_HIP(hipMemcpyAsync(s->h_swaps(), s->swaps.p, sizeof(unsigned long long) * 2, hipMemcpyDeviceToHost,
                                   s->st));
            GGS_HIP(hipStreamSynchronize(s->st));
        }
        done += n;
    }
    return GGS_OK;
}

int ggs_sa_chains_state(void* handle, double* best_fit, double* curr_fit, uint64_t* rounds, uint64_t* evaluated,
                        uint64_t* accepted, uint64_t* swaps_tried, uint64_t* swaps_accepted) {
    if (!handle) return fail(GGS_EINVAL, "null handle");
    SaChains* s = (SaChains*)handle;
    std::lock_guard<std::mutex> lk(s->c->mu);
    for (int k = 0; k < s->K; ++k) {    // as of the end of the last ggs_sa_chains_run (or creation)
        const SaLoopDev& l = s->h_loop()[k];
        if (best_fit) best_fit[k] = l.best_fit;
        if (curr_fit) curr_fit[k] = l.curr_fit;
        if (rounds) rounds[k] = l.rounds;
        if (evaluated) evaluated[k] = l.evaluated;
        if (accepted) accepted[k] = l.accepted;
    }
    if (swaps_tried) *swaps_tried = s->h_swaps()[0];
    if (swaps_accepted) *swaps_accepted = s->h_swaps()[1];
    return GGS_OK;
}

int ggs_sa_chains_read(void* handle, float* current, float* best) {
    if (!handle) return fail(GGS_EINVAL, "null handle");
    SaChains* s = (SaChains*)handle;
    std::lock_guard<std::mutex> lk(s->c->mu);
    DeviceGuard dg(s->c->dev);
    const size_t n9 = 9 * (size_t)s->N;
    GGS_HIP(hipStreamSynchronize(s->st));
    for (int k = 0; k < s->K && n9; ++k) {
        if (current)
            GGS_HIP(hipMemcpy(current + n9 * k, (const float*)s->curr.p + k * s->gstride, sizeof(float) * n9,
                              hipMemcpyDeviceToHost));
        if (best)
            GGS_HIP(hipMemcpy(best + n9 * k, (const float*)s->best.p + k * s->gstride, sizeof(float) * n9,
                              hipMemcpyDeviceToHost));
    }
    return GGS_OK;
}

void ggs_sa_chains_destroy(void* handle) { destroy_session<SaChains>(handle); }

int ggs_sa_exchange_uniform(uint64_t exchange_seed, int32_t it, int32_t k, double* u) {
    if (!u || it < 0 || k < 0) return fail(GGS_EINVAL, "bad arguments");
    *u = sa_exchange_uniform(exchange_seed, (uint32_t)it, (uint32_t)k);
    return GGS_OK;
}

}  // extern "C"
