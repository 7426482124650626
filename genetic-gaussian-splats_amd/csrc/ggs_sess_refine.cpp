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

int density_check_params(const ggs_refine_density& d) {
    if (d.every < 0 || d.start < 0 || d.stop < 0 || d.max_moves < 0)
        return fail(GGS_EINVAL, "density: every=%d, start=%d, stop=%d, max_moves=%d must be >= 0", d.every, d.start,
                    d.stop, d.max_moves);
    if (d.every > 0 && d.max_moves == 0) return fail(GGS_EINVAL, "density: max_moves must be >= 1 when every > 0");
    const float f[5] = {d.alpha_dead, d.grad_min, d.split_log, d.log_shrink, d.split_offset};
    for (float x : f)
        if (!std::isfinite(x)) return fail(GGS_EINVAL, "density: every float parameter must be finite");
    if (d.alpha_dead < 0.0f || d.alpha_dead > 255.0f)
        return fail(GGS_EINVAL, "density: alpha_dead=%g must be in [0, 255]", d.alpha_dead);
    if (d.grad_min < 0.0f) return fail(GGS_EINVAL, "density: grad_min=%g must be >= 0", d.grad_min);
    if (d.log_shrink < 0.0f) return fail(GGS_EINVAL, "density: log_shrink=%g must be >= 0", d.log_shrink);
    return GGS_OK;
}

constexpr int kDensityMaxB = 65535;     // the rank kernel's grid is (ceil(N / 256), B)

// What one event reads and writes beside x, m, v: the accumulator, the two lists, their
// counters and the event log.
struct DensityBufs {
    int M = 0;                     // the effective max_moves, min(max_moves, N / 2)
    DevBuf acc, dead, src, counts, pairs, is_split, last_n, moves, splits;
    size_t pair_bytes(int B) const { return sizeof(int) * 2 * (size_t)B * M; }

    // allocated and zeroed on st; `session`: with the accumulator and the cumulative counters
    int make(int B, int N, int max_moves, bool session, hipStream_t st) {
        M = std::min(max_moves, N / 2);
        const size_t lb = std::max<size_t>(sizeof(int) * (size_t)B * M, 4), ib = sizeof(int) * (size_t)B;
        int rc;
        if ((rc = ensure(dead, lb, st)) || (rc = ensure(src, lb, st)) || (rc = ensure(counts, 2 * ib, st)) ||
            (rc = ensure(pairs, 2 * lb, st)) || (rc = ensure(is_split, lb, st)) || (rc = ensure(last_n, ib, st)))
            return rc;
        if (session && ((rc = ensure(acc, sizeof(float) * (size_t)B * N, st)) ||
                        (rc = ensure(moves, 2 * ib, st)) || (rc = ensure(splits, 2 * ib, st))))
            return rc;
        // an event with M == 0 launches nothing: the log reads as "no pairs"
        GGS_HIP(hipMemsetAsync(pairs.p, 0xFF, 2 * lb, st));
        GGS_HIP(hipMemsetAsync(is_split.p, 0, lb, st));
        GGS_HIP(hipMemsetAsync(last_n.p, 0, ib, st));
        GGS_HIP(hipMemsetAsync(dead.p, 0, lb, st));
        GGS_HIP(hipMemsetAsync(src.p, 0, lb, st));
        if (session) {
            GGS_HIP(hipMemsetAsync(acc.p, 0, sizeof(float) * (size_t)B * N, st));
            GGS_HIP(hipMemsetAsync(moves.p, 0, 2 * ib, st));
            GGS_HIP(hipMemsetAsync(splits.p, 0, 2 * ib, st));
        }
        return GGS_OK;
    }
};

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
    // ggs_refine_set_density: off unless den.every > 0
    ggs_refine_density den{};
    DensityBufs db;
    int n_acc = 0;                 // steps accumulated since the last event
};

// one relocation event on the session's state, then the accumulator's reset
int refine_density_event(RefineSession* s) {
    DensityBufs& d = s->db;
    ProfScope ps(s->st, 4);
    GGS_HIP(launch_density_event(s->st, (float*)s->x.p, (float*)s->m.p, (float*)s->v.p, (const float*)d.acc.p, s->n_acc,
                                 s->B, s->N, s->cfg.H, s->cfg.W, s->cfg.scale_log_lo, s->cfg.scale_log_hi, s->den, d.M,
                                 (int*)d.dead.p, (int*)d.src.p, (int*)d.counts.p, (int*)d.pairs.p, (int*)d.is_split.p,
                                 (int*)d.last_n.p, (unsigned long long*)d.moves.p, (unsigned long long*)d.splits.p));
    GGS_HIP(hipMemsetAsync(d.acc.p, 0, sizeof(float) * (size_t)s->B * s->N, s->st));
    s->n_acc = 0;
    return GGS_OK;
}

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
        const ggs_refine_density& d = s->den;
        if (d.every > 0) {
            GGS_HIP(launch_density_acc(s->st, (const float*)s->grad.p, (float*)s->db.acc.p, s->B, s->N, s->cfg.H,
                                       s->cfg.W));
            s->n_acc += 1;
        }
        GGS_HIP(launch_refine_adam(s->st, (float*)s->x.p, (float*)s->m.p, (float*)s->v.p, (const float*)s->grad.p,
                                   s->B, s->N, p));
        if (d.every > 0 && s->t % d.every == 0 && s->t >= d.start && (d.stop == 0 || s->t <= d.stop) &&
            (rc = refine_density_event(s)))
            return rc;
    }
    return GGS_OK;
}

int ggs_refine_set_density(void* handle, const ggs_refine_density* density) {
    if (!handle) return fail(GGS_EINVAL, "null handle");
    RefineSession* s = (RefineSession*)handle;
    int rc;
    if (density && (rc = density_check_params(*density))) return rc;
    if (density && density->every > 0 && s->B > kDensityMaxB)
        return fail(GGS_EINVAL, "density: B=%d candidates exceed the limit %d", s->B, kDensityMaxB);
    std::lock_guard<std::mutex> lk(s->c->mu);
    DeviceGuard dg(s->c->dev);
    if (!density || density->every == 0) {
        s->den = ggs_refine_density{};
        return GGS_OK;
    }
    DensityBufs nb;                     // the session's own buffers stay until these are ready
    if ((rc = nb.make(s->B, s->N, density->max_moves, true, s->st))) {
        (void)hipStreamSynchronize(s->st);
        return rc;
    }
    GGS_HIP(hipStreamSynchronize(s->st));     // steps already queued are done with the old buffers
    s->db = std::move(nb);
    s->den = *density;
    s->n_acc = 0;
    return GGS_OK;
}

int ggs_refine_density_read(void* handle, float* acc_BN, int32_t* n_acc, int64_t* moves_B, int64_t* splits_B,
                            int32_t* last_pairs_B_M_2, int32_t* last_n_B) {
    if (!handle) return fail(GGS_EINVAL, "null handle");
    RefineSession* s = (RefineSession*)handle;
    std::lock_guard<std::mutex> lk(s->c->mu);
    DeviceGuard dg(s->c->dev);
    if (s->den.every == 0) return fail(GGS_EINVAL, "density control is off (ggs_refine_set_density)");
    const DensityBufs& d = s->db;
    const size_t ib = sizeof(int) * (size_t)s->B;
    GGS_HIP(hipStreamSynchronize(s->st));
    if (acc_BN) GGS_HIP(hipMemcpy(acc_BN, d.acc.p, sizeof(float) * (size_t)s->B * s->N, hipMemcpyDeviceToHost));
    if (n_acc) *n_acc = s->n_acc;
    if (moves_B) GGS_HIP(hipMemcpy(moves_B, d.moves.p, 2 * ib, hipMemcpyDeviceToHost));
    if (splits_B) GGS_HIP(hipMemcpy(splits_B, d.splits.p, 2 * ib, hipMemcpyDeviceToHost));
    if (last_pairs_B_M_2 && d.M > 0)
        GGS_HIP(hipMemcpy(last_pairs_B_M_2, d.pairs.p, d.pair_bytes(s->B), hipMemcpyDeviceToHost));
    if (last_n_B) GGS_HIP(hipMemcpy(last_n_B, d.last_n.p, ib, hipMemcpyDeviceToHost));
    return GGS_OK;
}

int ggs_density_relocate(int32_t device, const float* x, const float* m, const float* v, const float* acc,
                         int32_t n_acc, int32_t B, int32_t N, int32_t H, int32_t W, float log_lo, float log_hi,
                         const ggs_refine_density* params, float* x_out, float* m_out, float* v_out,
                         int32_t* pairs, int32_t* n_pairs, int32_t* is_split) {
    if (!params) return fail(GGS_EINVAL, "null ggs_refine_density");
    int rc = density_check_params(*params);
    if (rc) return rc;
    if (B < 1 || N < 1) return fail(GGS_EINVAL, "B=%d and N=%d must be >= 1", B, N);
    if (B > kDensityMaxB) return fail(GGS_EINVAL, "density: B=%d candidates exceed the limit %d", B, kDensityMaxB);
    if ((int64_t)B * N * 9 >= (int64_t)1 << 31)
        return fail(GGS_EINVAL, "B*N*9 = %lld genes exceeds the limit; split the batch", (long long)B * N * 9);
    if (H < 1 || W < 1) return fail(GGS_EINVAL, "H=%d, W=%d must be >= 1", H, W);
    if (n_acc < 0) return fail(GGS_EINVAL, "n_acc=%d must be >= 0", n_acc);
    if (!(log_lo <= log_hi)) return fail(GGS_EINVAL, "log bounds [%g, %g] are not an interval", log_lo, log_hi);
    const int M = params->every > 0 ? std::min(params->max_moves, N / 2) : 0;
    if (!x || !m || !v || !acc || !x_out || !m_out || !v_out || !n_pairs || (M > 0 && (!pairs || !is_split)))
        return fail(GGS_EINVAL, "null array");
    const size_t pb = sizeof(float) * 9 * (size_t)B * N, ab = sizeof(float) * (size_t)B * N;
    if (M == 0) {                       // off, or no pair fits: the identity
        if (x_out != x) memmove(x_out, x, pb);
        if (m_out != m) memmove(m_out, m, pb);
        if (v_out != v) memmove(v_out, v, pb);
        memset(n_pairs, 0, sizeof(int32_t) * (size_t)B);
        return GGS_OK;
    }
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    const hipStream_t st = c->stream;
    DevBuf dx, dm, dv, dacc;            // this call's own scratch, freed on return
    DensityBufs d;
    struct Sync {                       // ... after the stream has drained, errors included
        hipStream_t st;
        ~Sync() { (void)hipStreamSynchronize(st); }
    } sync{st};
    if ((rc = ensure(dx, pb, st)) || (rc = ensure(dm, pb, st)) || (rc = ensure(dv, pb, st)) ||
        (rc = ensure(dacc, ab, st)) || (rc = d.make(B, N, params->max_moves, false, st)))
        return rc;
    GGS_HIP(hipMemcpyAsync(dx.p, x, pb, hipMemcpyHostToDevice, st));
    GGS_HIP(hipMemcpyAsync(dm.p, m, pb, hipMemcpyHostToDevice, st));
    GGS_HIP(hipMemcpyAsync(dv.p, v, pb, hipMemcpyHostToDevice, st));
    GGS_HIP(hipMemcpyAsync(dacc.p, acc, ab, hipMemcpyHostToDevice, st));
    GGS_HIP(launch_density_event(st, (float*)dx.p, (float*)dm.p, (float*)dv.p, (const float*)dacc.p, n_acc, B, N, H, W,
                                 log_lo, log_hi, *params, d.M, (int*)d.dead.p, (int*)d.src.p, (int*)d.counts.p,
                                 (int*)d.pairs.p, (int*)d.is_split.p, (int*)d.last_n.p, nullptr, nullptr));
    GGS_HIP(hipMemcpyAsync(x_out, dx.p, pb, hipMemcpyDeviceToHost, st));
    GGS_HIP(hipMemcpyAsync(m_out, dm.p, pb, hipMemcpyDeviceToHost, st));
    GGS_HIP(hipMemcpyAsync(v_out, dv.p, pb, hipMemcpyDeviceToHost, st));
    GGS_HIP(hipMemcpyAsync(pairs, d.pairs.p, d.pair_bytes(B), hipMemcpyDeviceToHost, st));
    GGS_HIP(hipMemcpyAsync(is_split, d.is_split.p, sizeof(int) * (size_t)B * d.M, hipMemcpyDeviceToHost, st));
    GGS_HIP(hipMemcpyAsync(n_pairs, d.last_n.p, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, st));
    GGS_HIP(hipStreamSynchronize(st));
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
