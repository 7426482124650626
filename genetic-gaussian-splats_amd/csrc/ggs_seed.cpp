// Residual-driven placement, host side: ggs_seed_sites_device, its stage
// export ggs_seed_sites and the greedy coarse-to-fine seeding ggs_seed_genomes.  The
// kernels are ggs_seed.hip's; every argument is checked before a device is looked for.
#include "ggs_host.h"

namespace ggs {
namespace {

constexpr int kSeedMaxB = 65535;       // the rank kernel's grid is (ceil(G / 256), B)

bool seed_cell_ok(int c) { return c == 2 || c == 4 || c == 8 || c == 16 || c == 32 || c == 64; }

// The shape rules shared by the three entry points: B candidates, K images.
int seed_check_shape(int B, int K, int group, int H, int W) {
    if (B < 1) return fail(GGS_EINVAL, "B=%d must be >= 1", B);
    if (B > kSeedMaxB) return fail(GGS_EINVAL, "seed: B=%d candidates exceed the limit %d", B, kSeedMaxB);
    if (H < 1 || W < 1) return fail(GGS_EINVAL, "H=%d, W=%d must be >= 1", H, W);
    if (K < 1) return fail(GGS_EINVAL, "K=%d images: must be >= 1", K);
    if (group < 1) return fail(GGS_EINVAL, "group=%d must be >= 1", group);
    if (B % group != 0) return fail(GGS_EINVAL, "B=%d is not a multiple of group=%d", B, group);
    if (B / group > K) return fail(GGS_EINVAL, "B / group = %d images wanted, the set holds %d", B / group, K);
    return GGS_OK;
}

// ggs_seed_params and the sizes that follow from it.  with_x: the call writes rows of
// [B][N][9] genomes; row_list: it has a row list, so first_row is not read.
int seed_check_params(const ggs_seed_params* p, int B, int H, int W, bool with_x, int N, bool row_list) {
    if (!p) return fail(GGS_EINVAL, "null ggs_seed_params");
    if (!seed_cell_ok(p->cell)) return fail(GGS_EINVAL, "seed: cell=%d must be 2, 4, 8, 16, 32 or 64", p->cell);
    if (p->max_sites < 1) return fail(GGS_EINVAL, "seed: max_sites=%d must be >= 1", p->max_sites);
    if (!std::isfinite(p->err_min) || !std::isfinite(p->log_sigma) || !std::isfinite(p->alpha))
        return fail(GGS_EINVAL, "seed: err_min=%g, log_sigma=%g, alpha=%g must be finite", p->err_min, p->log_sigma,
                    p->alpha);
    if (p->err_min < 0.0f) return fail(GGS_EINVAL, "seed: err_min=%g must be >= 0", p->err_min);
    if (!(p->alpha >= 0.0f && p->alpha <= 255.0f))
        return fail(GGS_EINVAL, "seed: alpha=%g must be in [0, 255]", p->alpha);
    if ((int64_t)B * seed_cells(H, W, p->cell) >= (int64_t)1 << 31)
        return fail(GGS_EINVAL, "seed: B*cells = %lld exceeds the limit; split the batch",
                    (long long)B * seed_cells(H, W, p->cell));
    if ((int64_t)B * p->max_sites >= (int64_t)1 << 31)
        return fail(GGS_EINVAL, "seed: B*max_sites = %lld exceeds the limit", (long long)B * p->max_sites);
    if (with_x) {
        if (N < 1) return fail(GGS_EINVAL, "N=%d must be >= 1", N);
        if ((int64_t)B * N * 9 >= (int64_t)1 << 31)
            return fail(GGS_EINVAL, "B*N*9 = %lld genes exceeds the limit; split the batch", (long long)B * N * 9);
        if (!row_list && (p->first_row < 0 || (int64_t)p->first_row + p->max_sites > N))
            return fail(GGS_EINVAL, "seed: rows first_row=%d .. + max_sites=%d lie outside [0, N=%d)", p->first_row,
                        p->max_sites, N);
    }
    return GGS_OK;
}

// One placement on `st` (ctx locked, device set), bracketed as "seed" for the profiler.
int run_seed_sites(DevCtx* c, hipStream_t st, const float* d_img, const float bg[3], const float* d_targets,
                   const float* d_weights, int B, int group, int H, int W, const ggs_seed_params& prm,
                   const int* d_rows, float* d_x, int N, int* d_sites, int* d_n, float* d_err) {
    Workspace* w = workspace_for(c, st);
    int rc;
    if ((rc = ensure(w->seedws, seed_scratch_bytes(B, H, W, prm.cell, prm.max_sites, d_err == nullptr), st)))
        return rc;
    ProfScope ps(st, 5);
    GGS_HIP(launch_seed_sites(st, d_img, bg, d_targets, d_weights, B, group, H, W, prm, d_rows, d_x, N, w->seedws.p,
                              d_err, d_sites, d_n));
    return GGS_OK;
}

const float kWhite[3] = {1.f, 1.f, 1.f};

}  // namespace
}  // namespace ggs

using namespace ggs;

extern "C" {

int ggs_seed_sites_device(int32_t device, void* stream, const float* d_img_bhw3, const float* bg,
                          const float* d_targets_khw3, const float* d_weights_khw, int32_t B, int32_t K,
                          int32_t group, int32_t H, int32_t W, const ggs_seed_params* params,
                          const int32_t* d_rows_BM, float* d_genomes_BN9, int32_t N, int32_t* d_sites_BM,
                          int32_t* d_n_B, float* d_err_BG) {
    int rc = seed_check_shape(B, K, group, H, W);
    if (rc) return rc;
    if ((rc = seed_check_params(params, B, H, W, d_genomes_BN9 != nullptr, N, d_rows_BM != nullptr))) return rc;
    if (!d_targets_khw3 || !d_sites_BM || !d_n_B) return fail(GGS_EINVAL, "null targets/sites/n");
    if (bg && !(std::isfinite(bg[0]) && std::isfinite(bg[1]) && std::isfinite(bg[2])))
        return fail(GGS_EINVAL, "seed: the background must be finite");
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    return run_seed_sites(c, (hipStream_t)stream, d_img_bhw3, bg ? bg : kWhite, d_targets_khw3, d_weights_khw, B,
                          group, H, W, *params, d_rows_BM, d_genomes_BN9, N, d_sites_BM, d_n_B, d_err_BG);
}

int ggs_seed_sites(int32_t device, const float* img_bhw3, const float* bg, const float* targets_khw3,
                   const float* weights_khw, int32_t B, int32_t K, int32_t group, int32_t H, int32_t W,
                   const ggs_seed_params* params, const int32_t* rows_BM, const float* genomes_BN9, int32_t N,
                   float* genomes_out_BN9, int32_t* sites_BM, int32_t* n_B, float* err_BG) {
    int rc = seed_check_shape(B, K, group, H, W);
    if (rc) return rc;
    if ((genomes_BN9 == nullptr) != (genomes_out_BN9 == nullptr))
        return fail(GGS_EINVAL, "null genomes or genomes_out alone");
    const bool with_x = genomes_BN9 != nullptr;
    if ((rc = seed_check_params(params, B, H, W, with_x, N, rows_BM != nullptr))) return rc;
    if (!targets_khw3 || !sites_BM || !n_B) return fail(GGS_EINVAL, "null targets/sites/n");
    if (bg && !(std::isfinite(bg[0]) && std::isfinite(bg[1]) && std::isfinite(bg[2])))
        return fail(GGS_EINVAL, "seed: the background must be finite");
    const int M = params->max_sites;
    if (rows_BM && with_x)
        for (int64_t i = 0; i < (int64_t)B * M; ++i)
            if (rows_BM[i] < 0 || rows_BM[i] >= N)
                return fail(GGS_EINVAL, "seed: row %d of candidate %lld lies outside [0, N=%d)", rows_BM[i],
                            (long long)(i / M), N);
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    const hipStream_t st = c->stream;
    const size_t plane = (size_t)H * W, G = (size_t)seed_cells(H, W, params->cell);
    const size_t ib = sizeof(float) * 3 * plane * (size_t)B, tb = sizeof(float) * 3 * plane * (size_t)K;
    const size_t wb = sizeof(float) * plane * (size_t)K, xb = sizeof(float) * 9 * (size_t)B * (size_t)(with_x ? N : 0);
    const size_t sb = sizeof(int) * (size_t)B * M, eb = sizeof(float) * (size_t)B * G;
    DevBuf dimg, dtgt, dw, dx, drows, dsites, dn, derr;      // this call's own scratch, freed on return
    struct Sync {                       // ... after the stream has drained, errors included
        hipStream_t st;
        ~Sync() { (void)hipStreamSynchronize(st); }
    } sync{st};
    if ((img_bhw3 && (rc = ensure(dimg, ib, st))) || (rc = ensure(dtgt, tb, st)) ||
        (weights_khw && (rc = ensure(dw, wb, st))) || (with_x && (rc = ensure(dx, xb, st))) ||
        (rows_BM && (rc = ensure(drows, sb, st))) || (rc = ensure(dsites, sb, st)) ||
        (rc = ensure(dn, sizeof(int) * (size_t)B, st)) || (rc = ensure(derr, eb, st)))
        return rc;
    if (img_bhw3) GGS_HIP(hipMemcpyAsync(dimg.p, img_bhw3, ib, hipMemcpyHostToDevice, st));
    GGS_HIP(hipMemcpyAsync(dtgt.p, targets_khw3, tb, hipMemcpyHostToDevice, st));
    if (weights_khw) GGS_HIP(hipMemcpyAsync(dw.p, weights_khw, wb, hipMemcpyHostToDevice, st));
    if (with_x) GGS_HIP(hipMemcpyAsync(dx.p, genomes_BN9, xb, hipMemcpyHostToDevice, st));
    if (rows_BM) GGS_HIP(hipMemcpyAsync(drows.p, rows_BM, sb, hipMemcpyHostToDevice, st));
    if ((rc = run_seed_sites(c, st, (const float*)dimg.p, bg ? bg : kWhite, (const float*)dtgt.p, (const float*)dw.p,
                             B, group, H, W, *params, (const int*)drows.p, (float*)dx.p, N, (int*)dsites.p,
                             (int*)dn.p, (float*)derr.p)))
        return rc;
    if (with_x) GGS_HIP(hipMemcpyAsync(genomes_out_BN9, dx.p, xb, hipMemcpyDeviceToHost, st));
    GGS_HIP(hipMemcpyAsync(sites_BM, dsites.p, sb, hipMemcpyDeviceToHost, st));
    GGS_HIP(hipMemcpyAsync(n_B, dn.p, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, st));
    if (err_BG) GGS_HIP(hipMemcpyAsync(err_BG, derr.p, eb, hipMemcpyDeviceToHost, st));
    GGS_HIP(hipStreamSynchronize(st));
    return GGS_OK;
}

int ggs_seed_genomes(int32_t device, const float* targets_khw3, const float* weights_khw, int32_t K, int32_t H,
                     int32_t W, int32_t N, const ggs_seed_round* rounds, int32_t n_rounds, float err_min,
                     float scale_log_lo, float k_sigma, const float* bg, float* genomes_KN9, int32_t* placed_RK) {
    int rc = seed_check_shape(K, K, 1, H, W);
    if (rc) return rc;
    if (N < 1) return fail(GGS_EINVAL, "N=%d must be >= 1", N);
    if ((rc = check_dims(K, N, 9, H, W))) return rc;
    if (!targets_khw3 || !rounds || !genomes_KN9) return fail(GGS_EINVAL, "null targets/rounds/genomes");
    if (n_rounds < 1) return fail(GGS_EINVAL, "seed: n_rounds=%d must be >= 1", n_rounds);
    if (!std::isfinite(scale_log_lo) || !std::isfinite(k_sigma))
        return fail(GGS_EINVAL, "seed: scale_log_lo=%g and k_sigma=%g must be finite", scale_log_lo, k_sigma);
    if (bg && !(std::isfinite(bg[0]) && std::isfinite(bg[1]) && std::isfinite(bg[2])))
        return fail(GGS_EINVAL, "seed: the background must be finite");
    int64_t total = 0;
    int max_count = 1, min_cell = 64;
    for (int r = 0; r < n_rounds; ++r) {
        if (rounds[r].count < 0) return fail(GGS_EINVAL, "seed: round %d has count=%d < 0", r, rounds[r].count);
        // the round's parameters by the rules of one placement (a count of 0 is skipped)
        const ggs_seed_params p = {rounds[r].cell, std::max(rounds[r].count, 1), 0, err_min, rounds[r].log_sigma,
                                   rounds[r].alpha};
        if ((rc = seed_check_params(&p, K, H, W, false, N, false))) return rc;
        total += rounds[r].count;
        max_count = std::max(max_count, rounds[r].count);
        min_cell = std::min(min_cell, rounds[r].cell);
    }
    if (total != N) return fail(GGS_EINVAL, "seed: the rounds' counts sum to %lld, not N=%d", (long long)total, N);
    if ((int64_t)K * N * 9 >= (int64_t)1 << 31)
        return fail(GGS_EINVAL, "B*N*9 = %lld genes exceeds the limit; split the batch", (long long)K * N * 9);
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    const hipStream_t st = c->stream;
    const size_t plane = (size_t)H * W;
    const size_t ib = sizeof(float) * 3 * plane * (size_t)K, wb = sizeof(float) * plane * (size_t)K;
    const size_t xb = sizeof(float) * 9 * (size_t)K * N;
    std::vector<float> empty((size_t)K * N * 9, 0.0f);
    for (size_t i = 0; i < (size_t)K * N; ++i) {
        empty[i * 9 + 0] = 0.5f;
        empty[i * 9 + 1] = 0.5f;
        empty[i * 9 + 2] = scale_log_lo;
        empty[i * 9 + 3] = scale_log_lo;
    }
    DevBuf dimg, dtgt, dw, dx, dsites, dplaced;              // this call's own scratch, freed on return
    struct Sync {
        hipStream_t st;
        ~Sync() { (void)hipStreamSynchronize(st); }
    } sync{st};
    Workspace* w = workspace_for(c, st);
    // everything the rounds use is allocated before the first of them is enqueued
    if ((rc = ensure(dimg, ib, st)) || (rc = ensure(dtgt, ib, st)) || (weights_khw && (rc = ensure(dw, wb, st))) ||
        (rc = ensure(dx, xb, st)) || (rc = ensure(dsites, sizeof(int) * (size_t)K * max_count, st)) ||
        (rc = ensure(dplaced, sizeof(int) * (size_t)K * n_rounds, st)) ||
        (rc = ensure(w->seedws, seed_scratch_bytes(K, H, W, min_cell, max_count, true), st)))
        return rc;
    GGS_HIP(hipMemcpyAsync(dtgt.p, targets_khw3, ib, hipMemcpyHostToDevice, st));
    if (weights_khw) GGS_HIP(hipMemcpyAsync(dw.p, weights_khw, wb, hipMemcpyHostToDevice, st));
    GGS_HIP(hipMemcpyAsync(dx.p, empty.data(), xb, hipMemcpyHostToDevice, st));
    GGS_HIP(hipMemsetAsync(dplaced.p, 0, sizeof(int) * (size_t)K * n_rounds, st));
    int first = 0;
    for (int r = 0; r < n_rounds; ++r) {
        if (rounds[r].count == 0) continue;
        if ((rc = run_render(c, st, (const float*)dx.p, K, N, 9, H, W, k_sigma, bg ? bg : kWhite, (float*)dimg.p, true)))
            return rc;
        const ggs_seed_params p = {rounds[r].cell, rounds[r].count, first, err_min, rounds[r].log_sigma,
                                   rounds[r].alpha};
        if ((rc = run_seed_sites(c, st, (const float*)dimg.p, bg ? bg : kWhite, (const float*)dtgt.p,
                                 (const float*)dw.p, K, 1, H, W, p, nullptr, (float*)dx.p, N, (int*)dsites.p,
                                 (int*)dplaced.p + (size_t)r * K, nullptr)))
            return rc;
        first += rounds[r].count;
    }
    GGS_HIP(hipMemcpyAsync(genomes_KN9, dx.p, xb, hipMemcpyDeviceToHost, st));
    if (placed_RK)
        GGS_HIP(hipMemcpyAsync(placed_RK, dplaced.p, sizeof(int) * (size_t)K * n_rounds, hipMemcpyDeviceToHost, st));
    GGS_HIP(hipStreamSynchronize(st));
    return GGS_OK;
}

}  // extern "C"
