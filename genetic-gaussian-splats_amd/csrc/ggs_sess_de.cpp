// Device-resident differential evolution (ggs_de_*; kernels in ggs_de.hip).
// Declared in include/ggs.h.
#include "ggs_host.h"

namespace ggs {
namespace {

// Like a GA session: its own stream, pipeline buffers and finalize counters.
struct DeSession : Session {
    using Session::Session;
    ggs_de_params de{};
    int P = 0, N = 0, cur = 0;     // fits[cur]: the population's fitness
    DevBuf pop, trials, fits[2], trial_fits, best_ind, best_fit, best_row, curves;
    DevBuf recs, bnds, partials;
    int64_t n_curves = 0, curves_cap = 0;
};

int de_check_params(const ggs_de_params* de) {
    if (!de) return fail(GGS_EINVAL, "null ggs_de_params");
    if (de->strategy < 0 || de->strategy > 2)
        return fail(GGS_EINVAL, "unknown strategy %d (0 rand/1, 1 best/1, 2 current-to-best/1)", de->strategy);
    if (de->crossover < 0 || de->crossover > 1)
        return fail(GGS_EINVAL, "unknown crossover %d (0 per gene, 1 per splat)", de->crossover);
    if (!std::isfinite(de->f_lo) || !std::isfinite(de->f_hi))
        return fail(GGS_EINVAL, "f_lo and f_hi must be finite");
    if (de->f_lo > de->f_hi) return fail(GGS_EINVAL, "f_lo=%g must be <= f_hi=%g", de->f_lo, de->f_hi);
    if (!(de->cr >= 0.0f && de->cr <= 1.0f)) return fail(GGS_EINVAL, "cr=%g must be in [0, 1]", de->cr);
    return GGS_OK;
}

DeSelectDev de_select_args(DeSession* s, double* row) {
    return {(float*)s->pop.p, (const float*)s->trials.p, (const float*)s->fits[s->cur].p,
            (const float*)s->trial_fits.p, (float*)s->fits[1 - s->cur].p, (int*)s->best_row.p,
            (double*)s->best_fit.p, (float*)s->best_ind.p, row};
}

// variation (+ prep), raster (+ finalize), select
int de_generation(DeSession* s, int gen) {
    const ggs_ga_config& c = s->cfg;
    const int P = s->P, N = s->N;
    const DeParamsDev prm{s->de.strategy, s->de.crossover, s->de.f_lo, s->de.f_hi, s->de.cr, c.scale_log_lo,
                          c.scale_log_hi};
    int rc;
    double* row;
    if ((rc = curves_row(s->curves, s->n_curves, &s->curves_cap, sizeof(double) * 3, s->st, &row))) return rc;
    {
        ProfScope ps(s->st, 0);
        GGS_HIP(launch_de_variation(s->st, (const float*)s->pop.p, P, N, prm, c.seed, gen, (const int*)s->best_row.p,
                                    (float*)s->trials.p, (SplatRec*)s->recs.p, (int4*)s->bnds.p, c.H, c.W,
                                    c.k_sigma));
    }
    if ((rc = raster_fitness(s->st, s->c->simds, (const SplatRec*)s->recs.p, (const int4*)s->bnds.p, P, N, c.H, c.W,
                             (const float4*)s->plan.p, (float*)s->partials.p, (const float*)s->wpart.p,
                             c.fitness_mode, (const int*)s->order.p, s->fctr, (float*)s->trial_fits.p, true)))
        return rc;
    {
        ProfScope ps(s->st, 3);
        GGS_HIP(launch_de_select(s->st, de_select_args(s, row), P, N, 0));
    }
    s->cur = 1 - s->cur;
    s->n_curves += 1;
    return GGS_OK;
}

}  // namespace
}  // namespace ggs

using namespace ggs;

extern "C" {

int ggs_de_create(int32_t device, const ggs_ga_config* cfg, const ggs_de_params* de, const float* target_hw3,
                  const float* mask_hw, const float* init_pop, void** handle) {
    if (!cfg || !de || !target_hw3 || !init_pop || !handle) return fail(GGS_EINVAL, "null argument");
    const ggs_ga_config& c = *cfg;
    if (c.pop_size < 4 || c.pop_size > ga_breed_max_population())
        return fail(GGS_EINVAL, "pop_size must be in [4, %d] (three distinct rows besides the target), got %d",
                    ga_breed_max_population(), c.pop_size);
    if (c.n_splats < 1) return fail(GGS_EINVAL, "n_splats must be >= 1, got %d", c.n_splats);
    int rc = check_dims(c.pop_size, c.n_splats, 9, c.H, c.W);
    if (rc) return rc;
    if (c.fitness_mode < GGS_FIT_NONE || c.fitness_mode > GGS_FIT_BOOST)
        return fail(GGS_EINVAL, "bad fitness mode %d", c.fitness_mode);
    if (c.fitness_mode != GGS_FIT_NONE && !mask_hw) return fail(GGS_EINVAL, "mode needs a mask");
    if ((rc = de_check_params(de))) return rc;
    DevCtx* ctx = nullptr;
    if ((rc = get_ctx(device, &ctx))) return rc;
    auto s = std::make_unique<DeSession>(ctx, c);
    s->de = *de;
    s->P = c.pop_size;
    s->N = c.n_splats;
    const size_t pb = sizeof(float) * 9 * (size_t)s->P * s->N;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg(ctx->dev);
    auto bail = [&](int code) { return fail_session(s, code); };
    if ((rc = s->open(target_hw3, mask_hw, 1, 1, true))) return bail(rc);
    int nTX;
    const size_t slots = 4 * (size_t)raster_tiles(c.H, c.W, &nTX), rows = (size_t)s->P * s->N;
    if ((rc = ensure(s->pop, pb, s->st)) || (rc = ensure(s->trials, pb, s->st)) ||
        (rc = ensure(s->fits[0], sizeof(float) * s->P, s->st)) ||
        (rc = ensure(s->fits[1], sizeof(float) * s->P, s->st)) ||
        (rc = ensure(s->trial_fits, sizeof(float) * s->P, s->st)) ||
        (rc = ensure(s->best_ind, sizeof(float) * 9 * s->N, s->st)) ||
        (rc = ensure(s->best_fit, sizeof(double), s->st)) || (rc = ensure(s->best_row, sizeof(int), s->st)) ||
        (rc = ensure(s->recs, sizeof(SplatRec) * rows, s->st)) || (rc = ensure(s->bnds, sizeof(int4) * rows, s->st)) ||
        (rc = ensure(s->partials, sizeof(float) * slots * s->P, s->st)))
        return bail(rc);
    if (hipMemcpyAsync(s->pop.p, init_pop, pb, hipMemcpyHostToDevice, s->st))
        return bail(fail(GGS_EHIP, "upload failed"));
    // the initial population through the session's own pipeline
    {
        ProfScope ps(s->st, 0);
        if (launch_prep(s->st, true, (const float*)s->pop.p, (int64_t)rows, 9, c.H, c.W, c.k_sigma,
                        (SplatRec*)s->recs.p, (int4*)s->bnds.p, nullptr, nullptr, nullptr) != hipSuccess)
            return bail(fail(GGS_EHIP, "prep launch failed"));
    }
    if ((rc = raster_fitness(s->st, ctx->simds, (const SplatRec*)s->recs.p, (const int4*)s->bnds.p, s->P, s->N, c.H,
                             c.W, (const float4*)s->plan.p, (float*)s->partials.p, (const float*)s->wpart.p,
                             c.fitness_mode, (const int*)s->order.p, s->fctr, (float*)s->fits[0].p, true)))
        return bail(rc);
    double* row;
    if ((rc = curves_row(s->curves, 0, &s->curves_cap, sizeof(double) * 3, s->st, &row))) return bail(rc);
    if (launch_de_select(s->st, de_select_args(s.get(), row), s->P, s->N, 1) != hipSuccess)
        return bail(fail(GGS_EHIP, "init launch failed"));
    if (hipStreamSynchronize(s->st) != hipSuccess)     // init_pop / target may be freed on return
        return bail(fail(GGS_EHIP, "initial evaluation failed"));
    s->n_curves = 1;
    *handle = s.release();
    return GGS_OK;
}

int ggs_de_set_params(void* handle, const ggs_de_params* de) {
    if (!handle) return fail(GGS_EINVAL, "null handle");
    const int rc = de_check_params(de);
    if (rc) return rc;
    DeSession* s = (DeSession*)handle;
    std::lock_guard<std::mutex> lk(s->c->mu);
    s->de = *de;                     // a kernel argument of the launches from now on
    return GGS_OK;
}

int ggs_de_run(void* handle, int32_t first_gen, int32_t n_gens) {
    if (!handle || n_gens < 0 || first_gen < 0) return fail(GGS_EINVAL, "bad arguments");
    DeSession* s = (DeSession*)handle;
    std::lock_guard<std::mutex> lk(s->c->mu);
    DeviceGuard dg(s->c->dev);
    for (int g = 0; g < n_gens; ++g) {
        const int rc = de_generation(s, first_gen + g);
        if (rc) return rc;
    }
    return GGS_OK;
}

int ggs_de_read(void* handle, float* pop, float* fits, float* trials, float* trial_fits, float* best_ind,
                double* best_fit, double* curves, int32_t* n_curves) {
    if (!handle) return fail(GGS_EINVAL, "null handle");
    DeSession* s = (DeSession*)handle;
    std::lock_guard<std::mutex> lk(s->c->mu);
    DeviceGuard dg(s->c->dev);
    GGS_HIP(hipStreamSynchronize(s->st));
    const size_t pb = sizeof(float) * 9 * (size_t)s->P * s->N;
    if (pop) GGS_HIP(hipMemcpy(pop, s->pop.p, pb, hipMemcpyDeviceToHost));
    if (fits) GGS_HIP(hipMemcpy(fits, s->fits[s->cur].p, sizeof(float) * s->P, hipMemcpyDeviceToHost));
    if (trials) GGS_HIP(hipMemcpy(trials, s->trials.p, pb, hipMemcpyDeviceToHost));
    if (trial_fits) GGS_HIP(hipMemcpy(trial_fits, s->trial_fits.p, sizeof(float) * s->P, hipMemcpyDeviceToHost));
    if (best_ind) GGS_HIP(hipMemcpy(best_ind, s->best_ind.p, sizeof(float) * 9 * (size_t)s->N, hipMemcpyDeviceToHost));
    if (best_fit) GGS_HIP(hipMemcpy(best_fit, s->best_fit.p, sizeof(double), hipMemcpyDeviceToHost));
    if (curves) GGS_HIP(hipMemcpy(curves, s->curves.p, sizeof(double) * 3 * s->n_curves, hipMemcpyDeviceToHost));
    if (n_curves) *n_curves = (int32_t)s->n_curves;
    return GGS_OK;
}

void ggs_de_destroy(void* handle) { destroy_session<DeSession>(handle); }

}  // extern "C"
