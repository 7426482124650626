// Adam refiner sessions (ggs_refine_*), and what the island group's polish shares
// with them.  Kernels in ggs_grad.hip / ggs_loss.hip; declared in include/ggs.h.
#include "ggs_host.h"

namespace ggs {

int refine_check_params(const ggs_refine_params* p) {
    if (!p) return fail(GGS_EINVAL, "null ggs_refine_params");
    for (int c = 0; c < 9; ++c)
        if (!std::isfinite(p->lr[c]) || p->lr[c] < 0.0f) return fail(GGS_EINVAL, "lr[%d]=%g must be finite and >= 0", c, p->lr[c]);
    if (!(p->beta1 >= 0.0f && p->beta1 < 1.0f)) return fail(GGS_EINVAL, "beta1=%g must be in [0, 1)", p->beta1);
    if (!(p->beta2 >= 0.0f && p->beta2 < 1.0f)) return fail(GGS_EINVAL, "beta2=%g must be in [0, 1)", p->beta2);
    if (!(p->eps > 0.0f) || !std::isfinite(p->eps)) return fail(GGS_EINVAL, "eps=%g must be > 0", p->eps);
    return GGS_OK;
}

RefineStepDev refine_step_dev(const ggs_refine_params& prm, const ggs_ga_config& cfg, int64_t t) {
    RefineStepDev p;
    for (int c = 0; c < 9; ++c) p.lr[c] = prm.lr[c];
    p.beta1 = prm.beta1;
    p.beta2 = prm.beta2;
    p.eps = prm.eps;
    p.c1 = (float)(1.0 - pow((double)prm.beta1, (double)t));
    p.c2 = (float)(1.0 - pow((double)prm.beta2, (double)t));
    p.log_lo = cfg.scale_log_lo;
    p.log_hi = cfg.scale_log_hi;
    return p;
}

namespace {

// B candidates refined side by side on the session's own stream: per step one
// gradient call (fitness and gradient of the state x_t), the best-so-far update
// (x_t, its fitness) and one elementwise Adam update.  The pipeline buffers are the
// stream's pooled workspace, dropped with the session.
struct RefineSession : Session {
    using Session::Session;
    ggs_refine_params prm{};
    int B = 0, N = 0;
    int64_t t = 0;                 // Adam steps taken
    DevBuf x, m, v, grad, fits, best_x, best_fit;
    // ggs_refine_create_targets: target [K][H][W][3], mask [K][H][W], plan / wpart a plan
    // set of K made at create; candidate b against image b / group (0: the one target)
    int K = 1, group = 0;
    // ggs_refine_create_loss: fits is the image loss of the render against image b / group
    // (no plan, no mask); the render and its cotangent live in img / cot [B][H][W][3]
    bool use_loss = false;
    ggs_loss_params loss{};
    float bg[3] = {1.f, 1.f, 1.f};
    DevBuf img, cot;
};

// fitness (and, with grad, the gradient) of the current state into s->fits
int refine_eval(RefineSession* s, bool grad) {
    const ggs_ga_config& c = s->cfg;
    const float* d_mask = s->d_mask();
    if (s->use_loss) {
        if (grad)
            return run_loss_grad(s->c, s->st, (const float*)s->x.p, s->B, s->N, 9, GGS_LAYOUT_AXES,
                                 (const float*)s->target.p, s->group, c.H, c.W, c.k_sigma, s->bg, s->loss,
                                 (float*)s->fits.p, (float*)s->grad.p, (float*)s->img.p, (float*)s->cot.p);
        int rc = run_render(s->c, s->st, (const float*)s->x.p, s->B, s->N, 9, c.H, c.W, c.k_sigma, s->bg,
                            (float*)s->img.p, true);
        if (rc) return rc;
        return run_image_loss(s->c, s->st, (const float*)s->img.p, s->B, (const float*)s->target.p, s->group, c.H, c.W,
                              s->loss, (float*)s->fits.p, nullptr);
    }
    if (s->group > 0) {
        if (grad)
            return run_fitness_grad_planned(s->c, s->st, (const float*)s->x.p, s->B, s->N, 9, (const float4*)s->plan.p,
                                            (const float*)s->wpart.p, (const float*)s->target.p, d_mask,
                                            c.fitness_mode, c.boost_beta, c.H, c.W, s->group, c.k_sigma,
                                            (float*)s->fits.p, (float*)s->grad.p);
        return run_fitness_planned(s->c, s->st, (const float*)s->x.p, s->B, s->N, 9, (const float4*)s->plan.p,
                                   (const float*)s->wpart.p, c.fitness_mode, c.H, c.W, c.k_sigma, (float*)s->fits.p,
                                   s->group);
    }
    if (grad)
        return run_fitness_grad(s->c, s->st, (const float*)s->x.p, s->B, s->N, 9, (const float*)s->target.p, d_mask,
                                c.fitness_mode, c.boost_beta, c.H, c.W, c.k_sigma, (float*)s->fits.p,
                                (float*)s->grad.p, s->plan_key);
    return run_fitness(s->c, s->st, (const float*)s->x.p, s->B, s->N, 9, (const float*)s->target.p, d_mask,
                       c.fitness_mode, c.boost_beta, c.H, c.W, c.k_sigma, (float*)s->fits.p, s->plan_key);
}

// ggs_refine_create (group 0: one target and mask), ggs_refine_create_targets
// (group >= 1: targets [K][H][W][3], masks [K][H][W], one plan set) and
// ggs_refine_create_loss (loss set: group >= 1, targets [K][H][W][3], no mask and no plan)
int refine_create(int32_t device, const ggs_ga_config* cfg, const ggs_refine_params* p, const float* target,
                  const float* mask, int32_t K, const float* genomes_BN9, int32_t B, int32_t group, void** handle,
                  const ggs_loss_params* loss = nullptr, const float* bg = nullptr) {
    if (!cfg || !p || !target || !genomes_BN9 || !handle) return fail(GGS_EINVAL, "null argument");
    const ggs_ga_config& c = *cfg;
    int rc = loss ? check_loss_grad(B, c.n_splats, 9, GGS_LAYOUT_AXES, K, group, c.H, c.W, loss)
             : group == 0 ? check_grad_dims(B, c.n_splats, 9, c.H, c.W, c.fitness_mode, mask)
                          : check_grad_set(B, c.n_splats, 9, c.H, c.W, c.fitness_mode, mask, K, group);
    if (rc) return rc;
    if (!loss && group > 0 && (rc = check_dims(K, 1, 9, c.H, c.W))) return rc;
    if ((rc = refine_check_params(p))) return rc;
    DevCtx* ctx = nullptr;
    if ((rc = get_ctx(device, &ctx))) return rc;
    auto s = std::make_unique<RefineSession>(ctx, c);
    s->prm = *p;
    s->B = B;
    s->N = c.n_splats;
    s->K = K;
    s->group = group;
    if (loss) {
        s->use_loss = true;
        s->loss = *loss;
        if (bg) memcpy(s->bg, bg, sizeof s->bg);
    }
    const bool planned = group > 0 && !loss;
    const size_t pb = sizeof(float) * 9 * (size_t)B * s->N;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg(ctx->dev);
    auto bail = [&](int code) { return fail_session(s, code); };
    // no tile order of its own: every evaluation runs through the stream's workspace
    if ((rc = s->open(target, mask, K, planned ? K : 0, false))) return bail(rc);
    if ((rc = ensure(s->x, pb, s->st)) || (rc = ensure(s->m, pb, s->st)) || (rc = ensure(s->v, pb, s->st)) ||
        (rc = ensure(s->grad, pb, s->st)) || (rc = ensure(s->best_x, pb, s->st)) ||
        (rc = ensure(s->fits, sizeof(float) * (size_t)B, s->st)) ||
        (rc = ensure(s->best_fit, sizeof(double) * (size_t)B, s->st)) ||
        (loss && ((rc = ensure(s->img, sizeof(float) * 3 * (size_t)B * c.H * c.W, s->st)) ||
                  (rc = ensure(s->cot, sizeof(float) * 3 * (size_t)B * c.H * c.W, s->st)))))
        return bail(rc);
    std::vector<double> inf((size_t)B, (double)INFINITY);
    if (hipMemcpyAsync(s->x.p, genomes_BN9, pb, hipMemcpyHostToDevice, s->st) ||
        hipMemcpyAsync(s->best_x.p, genomes_BN9, pb, hipMemcpyHostToDevice, s->st) ||
        hipMemcpyAsync(s->best_fit.p, inf.data(), sizeof(double) * (size_t)B, hipMemcpyHostToDevice, s->st) ||
        hipMemsetAsync(s->m.p, 0, pb, s->st) || hipMemsetAsync(s->v.p, 0, pb, s->st) ||
        hipMemsetAsync(s->grad.p, 0, pb, s->st))
        return bail(fail(GGS_EHIP, "upload failed"));
    if (hipStreamSynchronize(s->st) != hipSuccess)     // the caller's arrays may be freed on return
        return bail(fail(GGS_EHIP, "upload failed"));
    *handle = s.release();
    return GGS_OK;
}
}  // namespace
}  // namespace ggs

using namespace ggs;

extern "C" {

int ggs_refine_create(int32_t device, const ggs_ga_config* cfg, const ggs_refine_params* p, const float* target_hw3,
                      const float* mask_hw, const float* genomes_BN9, int32_t B, void** handle) {
    return ggs::refine_create(device, cfg, p, target_hw3, mask_hw, 1, genomes_BN9, B, 0, handle);
}

int ggs_refine_create_targets(int32_t device, const ggs_ga_config* cfg, const ggs_refine_params* p,
                              const float* targets_khw3, const float* masks_khw, int32_t K, const float* genomes_BN9,
                              int32_t B, int32_t group, void** handle) {
    if (group < 1) return fail(GGS_EINVAL, "group=%d must be >= 1", group);
    return ggs::refine_create(device, cfg, p, targets_khw3, masks_khw, K, genomes_BN9, B, group, handle);
}

int ggs_refine_create_loss(int32_t device, const ggs_ga_config* cfg, const ggs_refine_params* p,
                           const ggs_loss_params* loss, const float* bg, const float* targets_khw3, int32_t K,
                           const float* genomes_BN9, int32_t B, int32_t group, void** handle) {
    if (!loss) return fail(GGS_EINVAL, "null ggs_loss_params");
    return ggs::refine_create(device, cfg, p, targets_khw3, nullptr, K, genomes_BN9, B, group, handle, loss, bg);
}

int ggs_refine_run(void* handle, int32_t n_steps) {
    if (!handle || n_steps < 0) return fail(GGS_EINVAL, "bad arguments");
    RefineSession* s = (RefineSession*)handle;
    std::lock_guard<std::mutex> lk(s->c->mu);
    DeviceGuard dg(s->c->dev);
    for (int i = 0; i < n_steps; ++i) {
        int rc;
        if ((rc = refine_eval(s, true))) return rc;
        GGS_HIP(launch_refine_best(s->st, (const float*)s->x.p, (const float*)s->fits.p, s->B, s->N,
                                   (double*)s->best_fit.p, (float*)s->best_x.p));
        s->t += 1;
        const RefineStepDev p = refine_step_dev(s->prm, s->cfg, s->t);
        GGS_HIP(launch_refine_adam(s->st, (float*)s->x.p, (float*)s->m.p, (float*)s->v.p, (const float*)s->grad.p,
                                   s->B, s->N, p));
    }
    return GGS_OK;
}

int ggs_refine_read(void* handle, float* genomes, float* fits, float* best, float* best_fits, float* last_grad) {
    if (!handle) return fail(GGS_EINVAL, "null handle");
    RefineSession* s = (RefineSession*)handle;
    std::lock_guard<std::mutex> lk(s->c->mu);
    DeviceGuard dg(s->c->dev);
    // the current state's own fitness, which may also be the best so far
    int rc;
    if ((rc = refine_eval(s, false))) return rc;
    GGS_HIP(launch_refine_best(s->st, (const float*)s->x.p, (const float*)s->fits.p, s->B, s->N,
                               (double*)s->best_fit.p, (float*)s->best_x.p));
    GGS_HIP(hipStreamSynchronize(s->st));
    const size_t pb = sizeof(float) * 9 * (size_t)s->B * s->N;
    if (genomes) GGS_HIP(hipMemcpy(genomes, s->x.p, pb, hipMemcpyDeviceToHost));
    if (fits) GGS_HIP(hipMemcpy(fits, s->fits.p, sizeof(float) * (size_t)s->B, hipMemcpyDeviceToHost));
    if (best) GGS_HIP(hipMemcpy(best, s->best_x.p, pb, hipMemcpyDeviceToHost));
    if (best_fits) {
        std::vector<double> bf((size_t)s->B);
        GGS_HIP(hipMemcpy(bf.data(), s->best_fit.p, sizeof(double) * (size_t)s->B, hipMemcpyDeviceToHost));
        for (int b = 0; b < s->B; ++b) best_fits[b] = (float)bf[b];   // float32 fitness values, widened: exact
    }
    if (last_grad) GGS_HIP(hipMemcpy(last_grad, s->grad.p, pb, hipMemcpyDeviceToHost));
    return GGS_OK;
}

void ggs_refine_destroy(void* handle) { destroy_session<RefineSession>(handle); }

}  // extern "C"
