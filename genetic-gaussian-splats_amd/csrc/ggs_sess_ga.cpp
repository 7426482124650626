// Device-resident GA sessions (ggs_ga_*) and island groups with their polish
// (ggs_ga_islands_*); kernels in ggs_ga.hip.  Declared in include/ggs.h.
#include "ggs_host.h"

namespace ggs {
namespace {

// What a GA session and an island group keep of the population(s): every array of
// the group has a leading island dimension.
struct GaState : Session {
    using Session::Session;
    int P = 0, N = 0, cur = 0;
    DevBuf pop[2], fits[2], off[2], off_fits, src, best_ind, best_fit, best_src, best_upd, curves;
    DevBuf elite[2];               // elite[cur]: rows of pop[cur] by fitness rank (the breed's row map)
    int ocur = 0;                  // off[ocur]: the offspring evaluated last
    bool pending = false;          // their survivors / gather not applied yet (ga_flush, gi_flush)
    DevBuf recs, bnds, partials;   // the generation's fused pipeline (with the base's plan, order, fctr)
    int64_t n_curves = 0, curves_cap = 0;
    GaBestDev best() { return {(double*)best_fit.p, (int*)best_src.p, (int*)best_upd.p, (float*)best_ind.p}; }

    // The buffers of K populations of P rows (P, N set) and of a raster batch of B candidates.
    int alloc(int K, size_t B) {
        const size_t KP = (size_t)K * P, pb = sizeof(float) * 9 * KP * N;
        int nTX, rc;
        const size_t slots = 4 * (size_t)raster_tiles(cfg.H, cfg.W, &nTX);
        for (DevBuf* b : {&pop[0], &pop[1], &off[0], &off[1]})
            if ((rc = ensure(*b, std::max<size_t>(pb, 4), st))) return rc;
        for (DevBuf* b : {&fits[0], &fits[1]})
            if ((rc = ensure(*b, sizeof(float) * KP, st))) return rc;
        for (DevBuf* b : {&src, &elite[0], &elite[1]})
            if ((rc = ensure(*b, sizeof(int) * KP, st))) return rc;
        if ((rc = ensure(off_fits, sizeof(float) * std::max<size_t>(B, 1), st)) ||
            (rc = ensure(best_ind, std::max<size_t>(sizeof(float) * 9 * (size_t)K * N, 4), st)) ||
            (rc = ensure(best_fit, sizeof(double) * K, st)) || (rc = ensure(best_src, sizeof(int) * K, st)) ||
            (rc = ensure(best_upd, sizeof(int) * K, st)) ||
            (rc = ensure(recs, sizeof(SplatRec) * std::max<size_t>(B * N, 1), st)) ||
            (rc = ensure(bnds, sizeof(int4) * std::max<size_t>(B * N, 1), st)) ||
            (rc = ensure(partials, sizeof(float) * slots * std::max<size_t>(B, 1), st)))
            return rc;
        return GGS_OK;
    }
    // The fused breed's view of the pending generation: it closes into the other
    // buffers, its statistics into `row` of the curves.
    BreedDev breed(double* row) {
        const int nxt = 1 - cur;
        return {(const float*)pop[cur].p, (const float*)fits[cur].p, (const float*)off[ocur].p,
                (const float*)off_fits.p, (const int*)elite[cur].p, (int*)elite[nxt].p, (float*)pop[nxt].p,
                (float*)fits[nxt].p, row, best(), cfg.elite_k};
    }
    // The pending generation's survivors and gather are enqueued (on their own or
    // inside a breed): the other buffers are current and the curves have its row.
    void closed() {
        cur = 1 - cur;
        n_curves += 1;
        pending = false;
    }
};

struct GaSession : GaState {
    using GaState::GaState;
    DevBuf draws;
    void* comm = nullptr;          // ggs_ga_set_comm: offspring fitness sharded over ranks
    int nranks = 1, rank = 0;
    uint64_t fingerprint = 0;      // hash of (config, target, mask, initial population)
};

}  // namespace

static double anneal_factor(int gen, int total, int kind) {          // utils.py:14-27
    const int g = std::max(0, std::min(gen, total));
    const double p = (double)g / (double)std::max(1, total);
    double raw;
    if (kind == 1) raw = 0.5 * (1.0 + cos(M_PI * p));
    else if (kind == 2) raw = pow(pow(0.2, 1.0 / (double)std::max(1, total)), (double)g);
    else raw = 1.0 - p;
    return std::max(0.0, raw);
}

GaParamsDev ga_params(const ggs_ga_config& c, int gen, int total) {   // build_mut_sigma
    const double f = anneal_factor(gen, total, c.schedule);
    float sig[6];
    for (int k = 0; k < 6; ++k)
        sig[k] = (float)(c.sig_min[k] + f * (c.sig_max[k] - c.sig_min[k]));
    GaParamsDev p{};
    p.sig_xy = sig[0]; p.sig_alog = sig[1]; p.sig_blog = sig[2]; p.sig_theta = sig[3];
    p.sig_rgb = sig[4]; p.sig_alpha = sig[5];
    p.mutpb = c.mutpb; p.cxpb = c.cxpb; p.tour_k = c.tour_k;
    p.log_lo = c.scale_log_lo; p.log_hi = c.scale_log_hi;
    return p;
}

int curves_row(DevBuf& curves, int64_t n, int64_t* cap_io, size_t row_bytes, hipStream_t st, double** row) {
    if (n >= *cap_io) {
        const int64_t cap = std::max<int64_t>(64, *cap_io * 2);
        DevBuf nb;              // freed on the error returns
        GGS_HIP(hipMalloc(&nb.p, row_bytes * cap));
        nb.cap = row_bytes * cap;
        if (curves.p) {
            GGS_HIP(hipMemcpyAsync(nb.p, curves.p, row_bytes * n, hipMemcpyDeviceToDevice, st));
            GGS_HIP(hipStreamSynchronize(st));
        }
        curves = std::move(nb);     // the old block is freed with nb, after the copy
        *cap_io = cap;
    }
    *row = (double*)((char*)curves.p + row_bytes * n);
    return GGS_OK;
}

// The fused breed (survivors + gather of the previous generation inside the
// variation kernel: 3 launches per generation instead of 5), unless GGS_GA_UNFUSED=1.
static bool breed_fused() {
    static const bool off = getenv("GGS_GA_UNFUSED") && atoi(getenv("GGS_GA_UNFUSED")) != 0;
    return !off;
}

namespace {

// One generation's row of a GA session's curves [generation][3] / a group's [generation][K][3].
int ga_curves_row(GaState* s, int K, double** row) {
    return curves_row(s->curves, s->n_curves, &s->curves_cap, sizeof(double) * 3 * (size_t)K, s->st, row);
}

}  // namespace

int ga_upload_draws(DevBuf& buf, hipStream_t st, int64_t P, int64_t N, int64_t K, bool mutation_only,
                    const ggs_ga_draws* h, GaDrawsDev* d) {
    const int64_t np2 = (P + 1) / 2;
    struct Seg { const void* src; int64_t bytes; const void** dst; };
    Seg segs[] = {
        {h->tour_idx, 4 * P * K, (const void**)&d->tour_idx}, {h->perm, 4 * P, (const void**)&d->perm},
        {h->cx, 4 * np2, (const void**)&d->cx}, {h->cx_u, 4 * np2 * N, (const void**)&d->cx_u},
        {h->u_xy, 8 * P * N, (const void**)&d->u_xy}, {h->u_ab, 8 * P * N, (const void**)&d->u_ab},
        {h->u_t, 4 * P * N, (const void**)&d->u_t}, {h->u_rgb, 4 * P * N, (const void**)&d->u_rgb},
        {h->u_a, 4 * P * N, (const void**)&d->u_a}, {h->k_color, 4 * P, (const void**)&d->k_color},
        {h->k_xy, 4 * P, (const void**)&d->k_xy}, {h->k_ab, 4 * P, (const void**)&d->k_ab},
        {h->k_t, 4 * P, (const void**)&d->k_t}, {h->n_xy, 8 * P * N, (const void**)&d->n_xy},
        {h->n_ab, 8 * P * N, (const void**)&d->n_ab}, {h->n_t, 4 * P * N, (const void**)&d->n_t},
        {h->n_rgba, 16 * P * N, (const void**)&d->n_rgba}, {h->swap_i, 4 * P, (const void**)&d->swap_i},
        {h->swap_pick, 4 * P, (const void**)&d->swap_pick}, {h->swap_u, 8 * P, (const void**)&d->swap_u},
    };
    const int first = mutation_only ? 4 : 0;   // SA: no selection / crossover draws
    int64_t total = 0;
    for (int k = first; k < (int)(sizeof segs / sizeof segs[0]); ++k) {
        if (!segs[k].src) return fail(GGS_EINVAL, "every draws array is required");
        total += (segs[k].bytes + 255) & ~(int64_t)255;
    }
    int rc;
    if ((rc = ensure(buf, (size_t)total, st))) return rc;
    GGS_HIP(hipStreamSynchronize(st));   // the previous launch may still read the buffer
    char* base = (char*)buf.p;
    for (int k = first; k < (int)(sizeof segs / sizeof segs[0]); ++k) {
        const Seg& g = segs[k];
        GGS_HIP(hipMemcpyAsync(base, g.src, (size_t)g.bytes, hipMemcpyHostToDevice, st));
        *g.dst = base;
        base += (g.bytes + 255) & ~(int64_t)255;
    }
    return GGS_OK;
}

namespace {

// Survivors + gather of the generation evaluated last (algorithm.py:129-155):
// population, fitness, best and curves as of the end of that generation.  A
// generation leaves them pending; the next generation's breed applies them
// itself (fused), anything reading the session state calls this first.
int ga_flush(GaSession* s) {
    if (!s->pending) return GGS_OK;
    const int P = s->P, N = s->N, nxt = 1 - s->cur;
    double* row;
    int rc;
    if ((rc = ga_curves_row(s, 1, &row))) return rc;
    // (FitReduce-fused survivors measured slower: 33.7 us vs 19 + 4.1 separately)
    GGS_HIP(launch_ga_survivors(s->st, (const float*)s->fits[s->cur].p, (const float*)s->off_fits.p, P,
                                s->cfg.elite_k, (int*)s->src.p, (float*)s->fits[nxt].p, s->best(), row, 0,
                                FitReduce{}, (int*)s->elite[nxt].p));
    GGS_HIP(launch_ga_gather(s->st, (const float*)s->pop[s->cur].p, (const float*)s->off[s->ocur].p, P, N,
                             (const int*)s->src.p, (float*)s->pop[nxt].p, s->best(), 0));
    s->closed();
    return GGS_OK;
}

int ga_generation(GaSession* s, int gen, int total, const ggs_ga_draws* hd) {
    GaDrawsDev d{};
    int rc;
    if (hd && (rc = ga_upload_draws(s->draws, s->st, s->P, s->N, s->cfg.tour_k, false, hd, &d))) return rc;
    const int P = s->P, N = s->N;
    const GaParamsDev prm = ga_params(s->cfg, gen, total);
    const ggs_ga_config& c = s->cfg;
    const int onew = 1 - s->ocur;
    // per generation: breed (survivors + gather of the previous generation, then
    // variation + prep of the offspring), raster, finalize [, all-gather]
    // Only offspring[:P - E] survive (algorithm.py:140-141: the next generation is the
    // E elites + the first P - E offspring, fitnesses likewise); the last E offspring's
    // fitness is never read (survivors, fused breed, best, curves), so they are bred
    // (their draws keep the trajectory) but not evaluated.
    const int Pe = P - (c.elite_k < 1 ? 1 : c.elite_k);
    // this rank's contiguous shard of the evaluated offspring (all of them on one GPU);
    // every rank bred all P offspring above with the same draws
    const int per = (Pe + s->nranks - 1) / s->nranks;
    const int b0 = std::min(Pe, s->rank * per), nb = std::min(Pe, b0 + per) - b0;
    if (s->pending && breed_fused() && P <= ga_breed_max_population()) {   // fused up to this population
        double* row;
        if ((rc = ga_curves_row(s, 1, &row))) return rc;
        const BreedDev br = s->breed(row);
        {
            ProfScope ps(s->st, 0);
            GGS_HIP(launch_ga_variation(s->st, nullptr, nullptr, P, N, prm, d, c.seed, gen, (float*)s->off[onew].p,
                                        P, (SplatRec*)s->recs.p, (int4*)s->bnds.p, c.H, c.W, c.k_sigma, nullptr,
                                        nullptr, &br));
        }
        s->closed();
    } else {
        if ((rc = ga_flush(s))) return rc;
        ProfScope ps(s->st, 0);
        GGS_HIP(launch_ga_variation(s->st, (const float*)s->pop[s->cur].p, (const float*)s->fits[s->cur].p,
                                    P, N, prm, d, c.seed, gen, (float*)s->off[onew].p, P, (SplatRec*)s->recs.p,
                                    (int4*)s->bnds.p, c.H, c.W, c.k_sigma));
    }
    s->ocur = onew;
    s->pending = true;
    if (nb > 0 && (rc = raster_fitness(s->st, s->c->simds, (const SplatRec*)s->recs.p + (int64_t)b0 * N,
                                       (const int4*)s->bnds.p + (int64_t)b0 * N, nb, N, c.H, c.W,
                                       (const float4*)s->plan.p, (float*)s->partials.p, (const float*)s->wpart.p,
                                       c.fitness_mode, (const int*)s->order.p, s->fctr,
                                       (float*)s->off_fits.p + b0, true)))
        return rc;
    if (s->comm && per > 0) {   // one in-place all-gather of the shards' fitness scalars (RCCL, same stream)
        float* of = (float*)s->off_fits.p;
        if ((rc = ggs_comm_allgather(s->comm, s->st, of + (int64_t)s->rank * per, of, per, 0, nullptr)))
            return rc;
    }
    return GGS_OK;
}

}  // namespace

int ga_check_config(const ggs_ga_config& c, const float* mask_hw, bool sa) {
    int rc = check_dims(c.pop_size, c.n_splats, 9, c.H, c.W);
    if (rc) return rc;
    if (c.pop_size < 1 || c.pop_size > ga_max_population())
        return fail(GGS_EINVAL, "pop_size must be in [1, %d]", ga_max_population());
    if (!sa && c.tour_k < 1) return fail(GGS_EINVAL, "tour_k must be >= 1");
    if (!sa && c.elite_k > c.pop_size) return fail(GGS_EINVAL, "elite_k must be <= pop_size");
    if (c.fitness_mode < GGS_FIT_NONE || c.fitness_mode > GGS_FIT_BOOST)
        return fail(GGS_EINVAL, "bad fitness mode %d", c.fitness_mode);
    if (c.fitness_mode != GGS_FIT_NONE && !mask_hw) return fail(GGS_EINVAL, "mode needs a mask");
    return GGS_OK;
}

}  // namespace ggs

using namespace ggs;

extern "C" {

int ggs_ga_create(int32_t device, const ggs_ga_config* cfg, const float* target_hw3,
                  const float* mask_hw, const float* init_pop, void** handle) {
    if (!cfg || !target_hw3 || !init_pop || !handle) return fail(GGS_EINVAL, "null argument");
    const ggs_ga_config& c = *cfg;
    int rc = ga_check_config(c, mask_hw, false);
    if (rc) return rc;
    DevCtx* ctx = nullptr;
    if ((rc = get_ctx(device, &ctx))) return rc;
    auto s = std::make_unique<GaSession>(ctx, c);
    s->P = c.pop_size;
    s->N = c.n_splats;
    const size_t pb = sizeof(float) * 9 * (size_t)s->P * s->N, hw = (size_t)c.H * c.W;
    // what every rank of a sharded session must agree on (ggs_ga_set_comm checks it)
    s->fingerprint = hash_bytes(&s->cfg, sizeof s->cfg) * 0x9E3779B97F4A7C15ull ^
                     hash_bytes(target_hw3, sizeof(float) * 3 * hw) * 0xC2B2AE3D27D4EB4Full ^
                     (mask_hw ? hash_bytes(mask_hw, sizeof(float) * hw) : 0x165667B19E3779F9ull) ^
                     rotl(hash_bytes(init_pop, pb), 29);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg(ctx->dev);
    auto bail = [&](int code) { return fail_session(s, code); };
    if ((rc = s->open(target_hw3, mask_hw, 1, 1, true))) return bail(rc);
    if ((rc = s->alloc(1, (size_t)s->P))) return bail(rc);     // all P offspring get records
    if (hipMemcpyAsync(s->pop[0].p, init_pop, pb, hipMemcpyHostToDevice, s->st))
        return bail(fail(GGS_EHIP, "upload failed"));
    if ((rc = run_fitness(ctx, s->st, (const float*)s->pop[0].p, s->P, s->N, 9, (const float*)s->target.p,
                          s->d_mask(), c.fitness_mode, c.boost_beta,
                          c.H, c.W, c.k_sigma, (float*)s->fits[0].p, s->plan_key)))
        return bail(rc);
    double* row;
    if ((rc = ga_curves_row(s.get(), 1, &row))) return bail(rc);
    if (launch_ga_survivors(s->st, (const float*)s->fits[0].p, nullptr, s->P, c.elite_k, (int*)s->src.p,
                            nullptr, s->best(), row, 1, FitReduce{}, (int*)s->elite[0].p) ||
        launch_ga_gather(s->st, (const float*)s->pop[0].p, nullptr, s->P, s->N, nullptr, nullptr,
                         s->best(), 1))
        return bail(fail(GGS_EHIP, "init launch failed"));
    if (hipStreamSynchronize(s->st) != hipSuccess)     // init_pop / target may be freed on return
        return bail(fail(GGS_EHIP, "initial evaluation failed"));
    s->n_curves = 1;
    *handle = s.release();
    return GGS_OK;
}

int ggs_ga_set_comm(void* handle, void* comm) {
    GaSession* s = (GaSession*)handle;
    if (!s) return fail(GGS_EINVAL, "null GA handle");
    int32_t n = 1, r = 0;
    if (comm) {
        int rc = ggs_comm_size(comm, &n, &r);
        if (rc) return rc;
        // the ranks must breed identical offspring: compare the sessions' fingerprints
        // (exchanged as two float32 bit patterns; an all-gather only moves bytes)
        float mine[2];
        memcpy(mine, &s->fingerprint, sizeof mine);
        std::vector<float> all(2 * (size_t)n);
        if ((rc = ggs_comm_allgather_host(comm, mine, all.data(), 2))) return rc;
        for (int k = 0; k < n; ++k) {
            uint64_t f;
            memcpy(&f, &all[2 * (size_t)k], sizeof f);
            if (f != s->fingerprint)
                return fail(GGS_EINVAL, "ggs_ga_set_comm: rank %d's session differs from rank %d's (config, "
                            "target, mask, initial population or seed): the shards would mix populations",
                            k, r);
        }
    }
    std::lock_guard<std::mutex> lk(s->c->mu);
    DeviceGuard dg(s->c->dev);
    const int per = (s->P + n - 1) / n;
    int rc = ensure(s->off_fits, sizeof(float) * (size_t)per * n, s->st);   // gather target: n shards
    if (rc) return rc;
    s->comm = comm;
    s->nranks = n;
    s->rank = r;
    return GGS_OK;
}

int ggs_ga_step(void* handle, int32_t gen, int32_t total_gens, const ggs_ga_draws* draws) {
    if (!handle) return fail(GGS_EINVAL, "null handle");
    GaSession* s = (GaSession*)handle;
    std::lock_guard<std::mutex> lk(s->c->mu);
    DeviceGuard dg(s->c->dev);
    const int rc = ga_generation(s, gen, total_gens, draws);
    if (rc || !draws) return rc;
    GGS_HIP(hipStreamSynchronize(s->st));   // the caller's draw arrays are released on return
    return GGS_OK;
}

int ggs_ga_run(void* handle, int32_t first_gen, int32_t n_gens, int32_t total_gens) {
    if (!handle || n_gens < 0) return fail(GGS_EINVAL, "bad arguments");
    GaSession* s = (GaSession*)handle;
    std::lock_guard<std::mutex> lk(s->c->mu);
    DeviceGuard dg(s->c->dev);
    for (int g = 0; g < n_gens; ++g) {
        const int rc = ga_generation(s, first_gen + g, total_gens, nullptr);
        if (rc) return rc;
    }
    return GGS_OK;
}

int ggs_ga_read(void* handle, float* pop, float* fits, float* best_ind, double* best_fit,
                double* curves, int32_t* n_curves) {
    if (!handle) return fail(GGS_EINVAL, "null handle");
    GaSession* s = (GaSession*)handle;
    std::lock_guard<std::mutex> lk(s->c->mu);
    DeviceGuard dg(s->c->dev);
    const int rc = ga_flush(s);   // the last generation's survivors
    if (rc) return rc;
    GGS_HIP(hipStreamSynchronize(s->st));
    if (pop) GGS_HIP(hipMemcpy(pop, s->pop[s->cur].p, sizeof(float) * 9 * (size_t)s->P * s->N, hipMemcpyDeviceToHost));
    if (fits) GGS_HIP(hipMemcpy(fits, s->fits[s->cur].p, sizeof(float) * s->P, hipMemcpyDeviceToHost));
    if (best_ind) GGS_HIP(hipMemcpy(best_ind, s->best_ind.p, sizeof(float) * 9 * (size_t)s->N, hipMemcpyDeviceToHost));
    if (best_fit) GGS_HIP(hipMemcpy(best_fit, s->best_fit.p, sizeof(double), hipMemcpyDeviceToHost));
    if (curves) GGS_HIP(hipMemcpy(curves, s->curves.p, sizeof(double) * 3 * s->n_curves, hipMemcpyDeviceToHost));
    if (n_curves) *n_curves = (int32_t)s->n_curves;
    return GGS_OK;
}

void ggs_ga_destroy(void* handle) { destroy_session<GaSession>(handle); }

}  // extern "C"

// ---- island groups (ggs_ga_islands_*) -------------------------------------------
namespace ggs {
namespace {

// K populations of P rows in one session: every per-population array of GaSession
// with a leading island dimension, one stream / plan / tile order / counter block.
// The evaluated offspring are compact: island k's offspring o < Pe = P - E is
// candidate k * Pe + o of the generation's one raster launch (recs, bnds,
// partials, off_fits).  curves: [generation][K][3] on the device.
struct GaIslands : GaState {
    using GaState::GaState;
    int K = 0, Pe = 0;
    int migrate_every = 0, n_migrants = 0;
    int pending_gen = 0;           // which generation is pending (migrations count absolutely)
    DevBuf seeds, mig;
    // a target per island (ggs_ga_islands_create_targets): target [K][H][W][3], mask
    // [K][H][W], plan / wpart a plan set of K; island k's candidates are scored
    // against plan k, and a migration re-scores the immigrants (mig_gen [K][m][N][9],
    // their genomes staged compactly; mig_fits [K][m])
    bool multi = false;
    DevBuf mig_gen, mig_fits;
    // memetic generations (ggs_ga_islands_set_polish; every or n_steps 0: off): island
    // k's n_rows best-ranked rows are refine candidates k * n_rows + j
    ggs_ga_polish polish{};
    DevBuf px, pm, pv, pgrad, pbest_x, pbest_fit, pfits, prows;
};

bool gi_migrates(const GaIslands* s, int gen) {
    return s->K >= 2 && s->migrate_every > 0 && s->n_migrants > 0 && gen % s->migrate_every == 0;
}

bool gi_polishes(const GaIslands* s, int gen) {
    return s->polish.every > 0 && s->polish.n_steps > 0 && gen % s->polish.every == 0;
}

// One polish of every island, all on the session's stream: the ranked rows staged
// as K * n_rows refine candidates (zero moments, t from 1), n_steps steps as
// ggs_refine_run takes them and ggs_refine_read's closing evaluation, each one
// chain of launches for all candidates against their island's image, then the
// install (strictly lower only), the elite lists and the best so far.
int gi_polish(GaIslands* s) {
    const ggs_ga_config& c = s->cfg;
    const int R = s->polish.n_rows, B = s->K * R, N = s->N, cur = s->cur;
    const size_t pb = sizeof(float) * 9 * (size_t)B * N;
    const float* d_mask = s->d_mask();
    const int group = s->multi ? R : 0;     // a shared target: the one plan, ggs_refine_create's path
    int rc;
    GGS_HIP(launch_polish_stage(s->st, s->K, (const float*)s->pop[cur].p, (const float*)s->fits[cur].p, s->P, N, R,
                                (int*)s->prows.p, (float*)s->px.p, (float*)s->pbest_x.p, (double*)s->pbest_fit.p));
    GGS_HIP(hipMemsetAsync(s->pm.p, 0, pb, s->st));
    GGS_HIP(hipMemsetAsync(s->pv.p, 0, pb, s->st));
    for (int t = 1; t <= s->polish.n_steps; ++t) {
        if ((rc = run_fitness_grad_planned(s->c, s->st, (const float*)s->px.p, B, N, 9, (const float4*)s->plan.p,
                                           (const float*)s->wpart.p, (const float*)s->target.p, d_mask,
                                           c.fitness_mode, c.boost_beta, c.H, c.W, group, c.k_sigma,
                                           (float*)s->pfits.p, (float*)s->pgrad.p)))
            return rc;
        GGS_HIP(launch_refine_best(s->st, (const float*)s->px.p, (const float*)s->pfits.p, B, N,
                                   (double*)s->pbest_fit.p, (float*)s->pbest_x.p));
        GGS_HIP(launch_refine_adam(s->st, (float*)s->px.p, (float*)s->pm.p, (float*)s->pv.p, (const float*)s->pgrad.p,
                                   B, N, refine_step_dev(s->polish.adam, c, t)));
    }
    if ((rc = run_fitness_planned(s->c, s->st, (const float*)s->px.p, B, N, 9, (const float4*)s->plan.p,
                                  (const float*)s->wpart.p, c.fitness_mode, c.H, c.W, c.k_sigma, (float*)s->pfits.p,
                                  group)))
        return rc;
    GGS_HIP(launch_refine_best(s->st, (const float*)s->px.p, (const float*)s->pfits.p, B, N, (double*)s->pbest_fit.p,
                               (float*)s->pbest_x.p));
    GGS_HIP(launch_polish_install(s->st, s->K, (float*)s->pop[cur].p, (float*)s->fits[cur].p, s->P, N, R, c.elite_k,
                                  (const int*)s->prows.p, (const float*)s->pbest_x.p, (const double*)s->pbest_fit.p,
                                  (int*)s->elite[cur].p, (double*)s->best_fit.p, (float*)s->best_ind.p));
    return GGS_OK;
}

// ga_flush for the group, then the pending generation's migration and polish if they are due.
int gi_flush(GaIslands* s) {
    if (!s->pending) return GGS_OK;
    const int nxt = 1 - s->cur;
    double* row;
    int rc;
    if ((rc = ga_curves_row(s, s->K, &row))) return rc;
    GGS_HIP(launch_ga_survivors_islands(s->st, s->K, (const float*)s->fits[s->cur].p, (const float*)s->off_fits.p,
                                        s->P, s->N, s->cfg.elite_k, (int*)s->src.p, (float*)s->fits[nxt].p,
                                        s->best(), row, 0, (int*)s->elite[nxt].p));
    GGS_HIP(launch_ga_gather_islands(s->st, s->K, (const float*)s->pop[s->cur].p, (const float*)s->off[s->ocur].p,
                                     s->P, s->N, s->cfg.elite_k, (const int*)s->src.p, (float*)s->pop[nxt].p,
                                     s->best(), 0));
    s->closed();
    if (gi_migrates(s, s->pending_gen) && !s->multi)
        GGS_HIP(launch_ga_migrate(s->st, s->K, (float*)s->pop[nxt].p, (float*)s->fits[nxt].p, s->P, s->N,
                                  s->n_migrants, s->cfg.elite_k, (int*)s->mig.p, (int*)s->elite[nxt].p));
    else if (gi_migrates(s, s->pending_gen)) {
        // A target per island: an immigrant's fitness was measured against its source
        // island's target, so the genomes move first, the K * m immigrants are scored
        // against their new island's plan (one prep + one grouped raster, group m; the
        // generation's records and partials are free by now), and only then are the
        // fitness rows installed and the elites re-ranked.
        const int m = s->n_migrants, Bm = s->K * m;
        const ggs_ga_config& c = s->cfg;
        GGS_HIP(launch_ga_migrate_copy(s->st, s->K, (float*)s->pop[nxt].p, (const float*)s->fits[nxt].p, s->P, s->N,
                                       m, (int*)s->mig.p, (float*)s->mig_gen.p));
        {
            ProfScope ps(s->st, 0);
            GGS_HIP(launch_prep(s->st, true, (const float*)s->mig_gen.p, (int64_t)Bm * s->N, 9, c.H, c.W, c.k_sigma,
                                (SplatRec*)s->recs.p, (int4*)s->bnds.p, nullptr, nullptr, nullptr));
        }
        if ((rc = raster_fitness(s->st, s->c->simds, (const SplatRec*)s->recs.p, (const int4*)s->bnds.p, Bm, s->N,
                                 c.H, c.W, (const float4*)s->plan.p, (float*)s->partials.p, (const float*)s->wpart.p,
                                 c.fitness_mode, (const int*)s->order.p, s->fctr, (float*)s->mig_fits.p, true,
                                 nullptr, nullptr, m)))
            return rc;
        GGS_HIP(launch_ga_migrate_install(s->st, s->K, (float*)s->fits[nxt].p, s->P, m, c.elite_k,
                                          (const int*)s->mig.p, (const float*)s->mig_fits.p, (int*)s->elite[nxt].p));
    }
    if (gi_polishes(s, s->pending_gen) && (rc = gi_polish(s))) return rc;
    return GGS_OK;
}

int gi_generation(GaIslands* s, int gen, int total) {
    const int K = s->K, P = s->P, N = s->N;
    const ggs_ga_config& c = s->cfg;
    const GaParamsDev prm = ga_params(c, gen, total);
    const int onew = 1 - s->ocur;
    int rc;
    // a generation whose survivors are followed by a migration or a polish is closed
    // unfused (flush, migrate, polish); the plain variation launch then breeds from pop / fits
    if (s->pending && breed_fused() && !gi_migrates(s, s->pending_gen) && !gi_polishes(s, s->pending_gen)) {
        double* row;
        if ((rc = ga_curves_row(s, s->K, &row))) return rc;
        const BreedDev br = s->breed(row);
        {
            ProfScope ps(s->st, 0);
            GGS_HIP(launch_ga_variation_islands(s->st, K, nullptr, nullptr, P, N, prm, (const uint64_t*)s->seeds.p,
                                                gen, (float*)s->off[onew].p, (SplatRec*)s->recs.p,
                                                (int4*)s->bnds.p, c.H, c.W, c.k_sigma, c.elite_k, &br));
        }
        s->closed();
    } else {
        if ((rc = gi_flush(s))) return rc;
        ProfScope ps(s->st, 0);
        GGS_HIP(launch_ga_variation_islands(s->st, K, (const float*)s->pop[s->cur].p,
                                            (const float*)s->fits[s->cur].p, P, N, prm,
                                            (const uint64_t*)s->seeds.p, gen, (float*)s->off[onew].p,
                                            (SplatRec*)s->recs.p, (int4*)s->bnds.p, c.H, c.W, c.k_sigma, c.elite_k));
    }
    s->ocur = onew;
    s->pending = true;
    s->pending_gen = gen;
    const int B = K * s->Pe;        // one contiguous batch: island k's offspring o at k * Pe + o
    if (B > 0 && (rc = raster_fitness(s->st, s->c->simds, (const SplatRec*)s->recs.p, (const int4*)s->bnds.p, B, N,
                                      c.H, c.W, (const float4*)s->plan.p, (float*)s->partials.p,
                                      (const float*)s->wpart.p, c.fitness_mode, (const int*)s->order.p, s->fctr,
                                      (float*)s->off_fits.p, true, nullptr, nullptr, s->multi ? s->Pe : 0)))
        return rc;
    return GGS_OK;
}

int gi_check(const ggs_ga_config* cfg, const ggs_ga_islands* isl, const float* target_hw3, const float* mask_hw,
             const float* init_pops, void** handle) {
    if (!cfg || !isl || !target_hw3 || !handle) return fail(GGS_EINVAL, "null argument");
    int rc = ga_check_config(*cfg, mask_hw, false);
    if (rc) return rc;
    if (isl->n_islands < 1 || isl->n_islands > 65535)
        return fail(GGS_EINVAL, "n_islands must be in [1, 65535], got %d", isl->n_islands);
    if (cfg->pop_size > ga_breed_max_population())
        return fail(GGS_EINVAL, "an island's pop_size must be <= %d, got %d", ga_breed_max_population(),
                    cfg->pop_size);
    if (isl->migrate_every < 0) return fail(GGS_EINVAL, "migrate_every must be >= 0, got %d", isl->migrate_every);
    if (isl->n_migrants < 0 || isl->n_migrants > cfg->pop_size / 2)
        return fail(GGS_EINVAL, "n_migrants must be in [0, pop_size / 2 = %d], got %d", cfg->pop_size / 2,
                    isl->n_migrants);
    if (isl->topology != 0) return fail(GGS_EINVAL, "topology %d: only 0 (ring) exists", isl->topology);
    if (!isl->seeds) return fail(GGS_EINVAL, "seeds is required ([n_islands])");
    if (!init_pops) return fail(GGS_EINVAL, "init_pops is required ([K, P, N, 9])");
    return check_dims((int64_t)isl->n_islands * cfg->pop_size, cfg->n_splats, 9, cfg->H, cfg->W);
}

// ggs_ga_islands_create (multi false: target_hw3 [H][W][3], mask_hw [H][W] shared by
// the islands) and ggs_ga_islands_create_targets (multi: [K][H][W][3], [K][H][W]).
int gi_create(int32_t device, const ggs_ga_config* cfg, const ggs_ga_islands* isl, const float* target_hw3,
              const float* mask_hw, const float* init_pops, void** handle, bool multi) {
    int rc = gi_check(cfg, isl, target_hw3, mask_hw, init_pops, handle);   // before any device call
    if (rc) return rc;
    const ggs_ga_config& c = *cfg;
    DevCtx* ctx = nullptr;
    if ((rc = get_ctx(device, &ctx))) return rc;
    auto s = std::make_unique<GaIslands>(ctx, c);
    const int K = s->K = isl->n_islands, P = s->P = c.pop_size, N = s->N = c.n_splats;
    s->Pe = P - (c.elite_k < 1 ? 1 : c.elite_k);
    s->migrate_every = isl->migrate_every;
    s->n_migrants = isl->n_migrants;
    s->multi = multi;
    const int nplans = multi ? K : 1;
    const size_t KP = (size_t)K * P;
    // the raster batch: the generation's K * Pe offspring, or a migration's K * m immigrants
    const size_t Bm = multi && K >= 2 && s->migrate_every > 0 ? (size_t)K * s->n_migrants : 0;
    const size_t B = std::max((size_t)K * s->Pe, Bm);
    const size_t pb = sizeof(float) * 9 * KP * N;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg(ctx->dev);
    auto bail = [&](int code) { return fail_session(s, code); };
    if ((rc = s->open(target_hw3, mask_hw, nplans, nplans, true))) return bail(rc);
    if ((rc = s->alloc(K, B))) return bail(rc);
    // migration scratch: row lists, zeroed so that an entry is a valid row whatever the fitness values
    if ((rc = ensure_zeroed(s->mig, sizeof(int) * 2 * (size_t)std::max(s->n_migrants, 1) * K, s->st)))
        return bail(rc);
    if ((rc = ensure(s->seeds, sizeof(uint64_t) * K, s->st))) return bail(rc);
    if (Bm && ((rc = ensure(s->mig_gen, std::max<size_t>(sizeof(float) * 9 * Bm * N, 4), s->st)) ||
               (rc = ensure(s->mig_fits, sizeof(float) * Bm, s->st))))
        return bail(rc);
    if (hipMemcpyAsync(s->pop[0].p, init_pops, pb, hipMemcpyHostToDevice, s->st) ||
        hipMemcpyAsync(s->seeds.p, isl->seeds, sizeof(uint64_t) * K, hipMemcpyHostToDevice, s->st))
        return bail(fail(GGS_EHIP, "upload failed"));
    if (multi) {    // the initial [K][P] population, island k's rows against plan k
        if ((rc = run_fitness_planned(ctx, s->st, (const float*)s->pop[0].p, (int64_t)KP, N, 9,
                                      (const float4*)s->plan.p, (const float*)s->wpart.p, c.fitness_mode, c.H, c.W,
                                      c.k_sigma, (float*)s->fits[0].p, P)))
            return bail(rc);
    } else if ((rc = run_fitness(ctx, s->st, (const float*)s->pop[0].p, (int64_t)KP, N, 9, (const float*)s->target.p,
                                 s->d_mask(), c.fitness_mode, c.boost_beta, c.H, c.W, c.k_sigma,
                                 (float*)s->fits[0].p, s->plan_key)))
        return bail(rc);
    double* row;
    if ((rc = ga_curves_row(s.get(), K, &row))) return bail(rc);
    if (launch_ga_survivors_islands(s->st, K, (const float*)s->fits[0].p, nullptr, P, N, c.elite_k, (int*)s->src.p,
                                    nullptr, s->best(), row, 1, (int*)s->elite[0].p) ||
        launch_ga_gather_islands(s->st, K, (const float*)s->pop[0].p, nullptr, P, N, c.elite_k, nullptr, nullptr,
                                 s->best(), 1))
        return bail(fail(GGS_EHIP, "init launch failed"));
    if (hipStreamSynchronize(s->st) != hipSuccess)     // init_pops / target / seeds may be freed on return
        return bail(fail(GGS_EHIP, "initial evaluation failed"));
    s->n_curves = 1;
    *handle = s.release();
    return GGS_OK;
}
}  // namespace
}  // namespace ggs
extern "C" {

int ggs_ga_islands_create(int32_t device, const ggs_ga_config* cfg, const ggs_ga_islands* isl,
                          const float* target_hw3, const float* mask_hw, const float* init_pops, void** handle) {
    return ggs::gi_create(device, cfg, isl, target_hw3, mask_hw, init_pops, handle, false);
}

int ggs_ga_islands_create_targets(int32_t device, const ggs_ga_config* cfg, const ggs_ga_islands* isl,
                                  const float* targets_khw3, const float* masks_khw, const float* init_pops,
                                  void** handle) {
    return ggs::gi_create(device, cfg, isl, targets_khw3, masks_khw, init_pops, handle, true);
}

int ggs_ga_islands_run(void* handle, int32_t first_gen, int32_t n_gens, int32_t total_gens) {
    if (!handle || n_gens < 0) return fail(GGS_EINVAL, "bad arguments");
    GaIslands* s = (GaIslands*)handle;
    std::lock_guard<std::mutex> lk(s->c->mu);
    DeviceGuard dg(s->c->dev);
    for (int g = 0; g < n_gens; ++g) {
        const int rc = gi_generation(s, first_gen + g, total_gens);
        if (rc) return rc;
    }
    return GGS_OK;
}

int ggs_ga_islands_set_polish(void* handle, const ggs_ga_polish* polish) {
    if (!handle) return fail(GGS_EINVAL, "null handle");
    GaIslands* s = (GaIslands*)handle;
    std::lock_guard<std::mutex> lk(s->c->mu);
    if (!polish) {
        DeviceGuard dg(s->c->dev);
        const int rc = gi_flush(s);     // a generation already run is closed under the setting it ran with
        if (rc) return rc;
        s->polish = ggs_ga_polish{};
        return GGS_OK;
    }
    const ggs_ga_polish& q = *polish;
    const int Emax = std::max(1, s->cfg.elite_k);
    if (q.every < 0 || q.n_steps < 0) return fail(GGS_EINVAL, "every=%d and n_steps=%d must be >= 0", q.every, q.n_steps);
    if (q.n_rows < 1 || q.n_rows > Emax)
        return fail(GGS_EINVAL, "n_rows must be in [1, max(1, elite_k) = %d], got %d", Emax, q.n_rows);
    int rc = refine_check_params(&q.adam);
    if (rc) return rc;
    if (s->P > polish_max_population())
        return fail(GGS_EINVAL, "an island's pop_size must be <= %d, got %d", polish_max_population(), s->P);
    const ggs_ga_config& c = s->cfg;
    const int64_t B = (int64_t)s->K * q.n_rows;
    // the candidates' batch limits and the partial budget (GGS_ENOMEM)
    if ((rc = check_grad_dims(B, s->N, 9, c.H, c.W, c.fitness_mode, s->mask.p))) return rc;
    DeviceGuard dg(s->c->dev);
    const size_t pb = sizeof(float) * 9 * (size_t)B * s->N;
    if ((rc = ensure(s->px, pb, s->st)) || (rc = ensure(s->pm, pb, s->st)) || (rc = ensure(s->pv, pb, s->st)) ||
        (rc = ensure(s->pgrad, pb, s->st)) || (rc = ensure(s->pbest_x, pb, s->st)) ||
        (rc = ensure(s->pbest_fit, sizeof(double) * (size_t)B, s->st)) ||
        (rc = ensure(s->pfits, sizeof(float) * (size_t)B, s->st)) ||
        (rc = ensure(s->prows, sizeof(int) * (size_t)B, s->st)) ||
        (rc = reserve_grad_workspace(s->c, s->st, B, s->N, c.H, c.W)))
        return rc;              // buffers only grew: the session's settings are as they were
    if ((rc = gi_flush(s))) return rc;  // a generation already run is closed under the setting it ran with
    s->polish = q;
    return GGS_OK;
}

int ggs_ga_islands_read(void* handle, float* pop, float* fits, float* best_ind, double* best_fit,
                        double* curves, int32_t* n_curves) {
    if (!handle) return fail(GGS_EINVAL, "null handle");
    GaIslands* s = (GaIslands*)handle;
    std::lock_guard<std::mutex> lk(s->c->mu);
    DeviceGuard dg(s->c->dev);
    const int rc = gi_flush(s);   // the last generation's survivors (and its migration)
    if (rc) return rc;
    GGS_HIP(hipStreamSynchronize(s->st));
    const size_t K = s->K, KP = K * s->P;
    if (pop) GGS_HIP(hipMemcpy(pop, s->pop[s->cur].p, sizeof(float) * 9 * KP * s->N, hipMemcpyDeviceToHost));
    if (fits) GGS_HIP(hipMemcpy(fits, s->fits[s->cur].p, sizeof(float) * KP, hipMemcpyDeviceToHost));
    if (best_ind) GGS_HIP(hipMemcpy(best_ind, s->best_ind.p, sizeof(float) * 9 * K * s->N, hipMemcpyDeviceToHost));
    if (best_fit) GGS_HIP(hipMemcpy(best_fit, s->best_fit.p, sizeof(double) * K, hipMemcpyDeviceToHost));
    if (curves) {               // device [generation][K][3] -> caller [K][generation][3]
        const size_t n = (size_t)s->n_curves;
        std::vector<double> h(3 * K * n);
        GGS_HIP(hipMemcpy(h.data(), s->curves.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
        for (size_t g = 0; g < n; ++g)
            for (size_t k = 0; k < K; ++k)
                for (int q = 0; q < 3; ++q) curves[(k * n + g) * 3 + q] = h[(g * K + k) * 3 + q];
    }
    if (n_curves) *n_curves = (int32_t)s->n_curves;
    return GGS_OK;
}

void ggs_ga_islands_destroy(void* handle) { destroy_session<GaIslands>(handle); }

int ggs_ga_philox_draws(int32_t device, uint64_t seed, int32_t gen, int32_t first, int32_t n_off, int32_t P,
                        int32_t N, int32_t tour_k, float cxpb, const ggs_ga_draws_out* out) {
    if (n_off < 1 || P < 1 || N < 1 || tour_k < 1)
        return fail(GGS_EINVAL, "n_off=%d, P=%d, N=%d, tour_k=%d must be >= 1", n_off, P, N, tour_k);
    if (gen < 0 || first < 0) return fail(GGS_EINVAL, "gen=%d, first=%d must be >= 0", gen, first);
    const int64_t on = (int64_t)n_off * N, np2 = (n_off + 1) / 2;
    if (on > ((int64_t)1 << 27) || (int64_t)P * tour_k > ((int64_t)1 << 27))
        return fail(GGS_EINVAL, "n_off*N=%lld, P*tour_k=%lld exceed the limit of 2^27 draws per array",
                    (long long)on, (long long)P * tour_k);
    if (!out) return fail(GGS_EINVAL, "null output");
    GaDrawsOut d{};
    struct Seg { void* host; int64_t bytes; void** dev; };
    Seg segs[] = {
        {out->tour_idx, 4 * (int64_t)P * tour_k, (void**)&d.tour_idx}, {out->perm, 4 * (int64_t)P, (void**)&d.perm},
        {out->cx, 4 * np2, (void**)&d.cx}, {out->cx_u, 4 * np2 * N, (void**)&d.cx_u},
        {out->u_xy, 8 * on, (void**)&d.u_xy}, {out->u_ab, 8 * on, (void**)&d.u_ab},
        {out->u_t, 4 * on, (void**)&d.u_t}, {out->u_rgb, 4 * on, (void**)&d.u_rgb},
        {out->u_a, 4 * on, (void**)&d.u_a}, {out->k_color, 4 * (int64_t)n_off, (void**)&d.k_color},
        {out->k_xy, 4 * (int64_t)n_off, (void**)&d.k_xy}, {out->k_ab, 4 * (int64_t)n_off, (void**)&d.k_ab},
        {out->k_t, 4 * (int64_t)n_off, (void**)&d.k_t}, {out->n_xy, 8 * on, (void**)&d.n_xy},
        {out->n_ab, 8 * on, (void**)&d.n_ab}, {out->n_t, 4 * on, (void**)&d.n_t},
        {out->n_rgba, 16 * on, (void**)&d.n_rgba}, {out->swap_i, 4 * (int64_t)n_off, (void**)&d.swap_i},
        {out->swap_pick, 4 * (int64_t)n_off, (void**)&d.swap_pick},
        {out->swap_u, 8 * (int64_t)n_off, (void**)&d.swap_u},
    };
    int64_t total = 0;
    for (const Seg& g : segs) {
        if (!g.host) return fail(GGS_EINVAL, "null output: every draws array is required");
        total += (g.bytes + 255) & ~(int64_t)255;
    }
    int rc;
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    DevBuf buf;      // exact-size scratch of this call, freed on return
    GGS_HIP(hipMalloc(&buf.p, (size_t)total));
    char* base = (char*)buf.p;
    for (const Seg& g : segs) {
        *g.dev = base;
        base += (g.bytes + 255) & ~(int64_t)255;
    }
    GGS_HIP(launch_ga_philox_draws(c->stream, seed, gen, first, n_off, P, N, tour_k, cxpb, d));
    GGS_HIP(hipStreamSynchronize(c->stream));
    for (const Seg& g : segs) GGS_HIP(hipMemcpy(g.host, *g.dev, (size_t)g.bytes, hipMemcpyDeviceToHost));
    return GGS_OK;
}

}  // extern "C"
