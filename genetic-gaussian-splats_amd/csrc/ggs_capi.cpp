// C-ABI of libggs.so (declared in include/ggs.h): device contexts, pooled
// workspaces, host<->device staging, multi-device fan-out, error reporting and
// per-kernel event timing.  The kernels live in ggs_kernels.hip, the shared host
// declarations in ggs_host.h, the device-resident sessions in ggs_sess_*.cpp.
//
// Reference boundary replaced here:
//   render_splats_rgb_triton  modules/render.py:203-252  -> ggs_render / ggs_render_device
//   fitness_many              modules/fitness.py:7-31    -> ggs_fitness / ggs_fitness_device
//   (fitness_population fitness.py:34-47 and the list/tensor plumbing stay in Python)
#include <stdarg.h>
#include <stdio.h>

#include <atomic>

#include "ggs_host.h"


namespace ggs {

thread_local std::string t_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    t_err = buf;
    return code;
}

// thread-local ggs_last_error() message, for the other translation units (ggs_comm.cpp)
int set_error(int code, const char* msg) {
    t_err = msg ? msg : "";
    return code;
}

// ---- device buffers ---------------------------------------------------------
int ensure(DevBuf& b, size_t bytes, hipStream_t st) {
    if (bytes <= b.cap) return GGS_OK;
    if (b.p) {
        GGS_HIP(hipStreamSynchronize(st));
        GGS_HIP(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    const size_t want = std::max<size_t>(bytes + bytes / 4, 4096);
    GGS_HIP(hipMalloc(&b.p, want));
    b.cap = want;
    return GGS_OK;
}

int ensure_zeroed(DevBuf& b, size_t bytes, hipStream_t st) {
    if (bytes <= b.cap) return GGS_OK;
    int rc = ensure(b, bytes, st);
    if (rc) return rc;
    GGS_HIP(hipMemsetAsync(b.p, 0, b.cap, st));
    return GGS_OK;
}

// The device GA folds the fitness finalize into the raster (FinFused: the last
// strip wave of each candidate reduces it): its generation is one breed and one
// raster launch, and the launch the fold saves is worth more than the per-wave
// count it adds (shipped run +1.3 %).  The fitness API keeps the separate
// finalize launch: with four streams of independent batches the fold measured
// -0.4 % and +17 MB of write traffic per launch, with one stream +0.1 %
// (docs/EXPERIMENTS.md §14).  GGS_UNFUSED_FINALIZE=1 unfuses the GA too (A/B
// switch, same bits).
static bool finalize_fused() {
    static const bool off = getenv("GGS_UNFUSED_FINALIZE") && atoi(getenv("GGS_UNFUSED_FINALIZE")) != 0;
    return !off;
}
// Test switch: GGS_FITNESS_FOLD=1 folds the finalize into the fitness API's raster
// too (read per call, so one test process can cover both paths; the GA's fold
// under concurrent, uneven load is otherwise exercised only through GA sessions).
static bool fitness_api_fold() {
    const char* v = getenv("GGS_FITNESS_FOLD");
    return v && atoi(v) != 0;
}
// A/B and test switch: GGS_STRIP_WORDS=0 keeps the raster's own cull from the bounds
// where prep would hand it strip words (read per call; the same bits either way).
static bool strip_words_on() {
    const char* v = getenv("GGS_STRIP_WORDS");
    return !(v && *v && atoi(v) == 0);
}

int ensure_pinned(PinBuf& b, size_t bytes) {
    if (bytes <= b.cap) return GGS_OK;
    if (b.p) {
        GGS_HIP(hipHostFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    const size_t want = std::max<size_t>(bytes + bytes / 4, 4096);
    GGS_HIP(hipHostMalloc(&b.p, want, hipHostMallocDefault));
    b.cap = want;
    return GGS_OK;
}

// Upload the centre-first raster dispatch order for (H, W) once per size.
static int ensure_tile_order(Workspace* w, int H, int W, hipStream_t st) {
    if (w->order_H == H && w->order_W == W) return GGS_OK;
    const int n = raster_order_len(H, W);
    int rc;
    // the order's n groups, then the same n groups as decoded strips (strip_table_entry:
    // the strip-words raster's table; zeros where the canvas does not fit its fields,
    // launch_raster then never reads them)
    if ((rc = ensure(w->order, sizeof(int) * 2 * (size_t)n, st))) return rc;
    std::vector<int> h(2 * (size_t)n);
    raster_tile_order(H, W, h.data());
#ifdef GGS_PROBE_BUILD
    // probe: a dispatch order from a file of n int32 group indices (order experiments)
    if (const char* f = getenv("GGS_PROBE_ORDER")) {
        FILE* fp = fopen(f, "rb");
        if (!fp || fread(h.data(), sizeof(int), n, fp) != (size_t)n) {
            if (fp) fclose(fp);
            return fail(GGS_EINVAL, "GGS_PROBE_ORDER: cannot read the order");
        }
        fclose(fp);
    }
#endif
    int nTX;
    raster_tiles(H, W, &nTX);
    w->strips_ok = true;
    for (int g = 0; g < n; ++g)
        if (!strip_table_entry(h[g], nTX, &h[(size_t)n + g])) w->strips_ok = false;
    GGS_HIP(hipStreamSynchronize(st));
    GGS_HIP(hipMemcpy(w->order.p, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice));
    w->order_H = H;
    w->order_W = W;
    return GGS_OK;
}

namespace {

std::mutex g_mu;
// Indexed by HIP device id.  The registry is immortal (never destroyed): a context
// owns device buffers, and no HIP call may run from a static destructor after
// main() returns.  ggs_shutdown is the only place that releases contexts.
auto& g_ctx = *new std::vector<std::unique_ptr<DevCtx>>;
std::vector<int> g_active;                    // devices the host API fans out over
bool g_inited = false;

// ---- profiling ----------------------------------------------------------------
constexpr int kProfKernels = 6;
struct ProfRec {
    int kernel;  // 0 prep, 1 raster, 2 finalize, 3 select (DE)
    hipEvent_t a, b;
};
std::mutex g_prof_mu;
bool g_prof_on = false;
std::vector<ProfRec> g_prof_pending;
double g_prof_ms[kProfKernels] = {};
int64_t g_prof_n[kProfKernels] = {};
const char* const kKernelNames[kProfKernels] = {"prep", "raster", "finalize", "select", "density", "seed"};

}  // namespace

ProfScope::ProfScope(hipStream_t s, int k) : st(s), kernel(k) {
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        on = g_prof_on;
    }
    if (on && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess)
        (void)hipEventRecord(a, st);
    else
        on = false;
}
ProfScope::~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(b, st);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_pending.push_back({kernel, a, b});
}

static void prof_drain_locked() {
    for (auto& r : g_prof_pending) {
        float ms = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            g_prof_ms[r.kernel] += ms;
            g_prof_n[r.kernel] += 1;
        }
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    g_prof_pending.clear();
}

int raster_fitness(hipStream_t st, int simds, const SplatRec* recs, const int4* bnds, int B, int N, int H, int W,
                   const float4* plan, float* partials, const float* wpartials, int mode, const int* order,
                   DevBuf& ctr, float* out, bool fuse, const unsigned char* dirty, const float* clean, int group,
                   const StripWords& sw) {
    const float bg[3] = {1.f, 1.f, 1.f};  // fitness renders with the default background (fitness.py:15)
    int nTX;
    const int nTiles = raster_tiles(H, W, &nTX);
    // fused only where every candidate's partials fill whole 128-B lines (4 * nTiles
    // a multiple of 32 floats: 512^2, 1024^2, 2048^2 ...): a line is then read, with
    // agent-scope loads, by one wave only, after every store to it, and never sits
    // in that XCD's L2 from an earlier read of a neighbour candidate's finalize
    if (fuse && finalize_fused() && (4 * nTiles) % 32 == 0) {
        int rc;
        if ((rc = ensure_zeroed(ctr, sizeof(int) * (size_t)std::max(B, 1), st))) return rc;
        FinFused ff;
        ff.ctr = (int*)ctr.p;
        ff.wpartials = wpartials;
        ff.out = out;
        ff.hw = (double)H * (double)W;
        ff.mode = mode;
        ProfScope ps(st, 1);
        GGS_HIP(launch_raster(st, 1, recs, bnds, B, N, H, W, bg, nullptr, plan, partials, order, dirty, clean,
                              nullptr, &ff, simds, group));
        return GGS_OK;
    }
    {
        ProfScope ps(st, 1);
        GGS_HIP(launch_raster(st, 1, recs, bnds, B, N, H, W, bg, nullptr, plan, partials, order, dirty, clean,
                              nullptr, nullptr, simds, group, sw));
    }
    ProfScope ps(st, 2);
    GGS_HIP(launch_finalize(st, partials, wpartials, B, nTiles, mode, H, W, out, nullptr, group));
    return GGS_OK;
}

// ---- helpers ----------------------------------------------------------------------
namespace {
// Host API: every stream this call has queued work on — copies from or into the
// caller's arrays included — is synchronised before the call returns, on error
// returns too, so the caller's arrays are never touched after the call
// (include/ggs.h: pointers are used only during the call).  Declared after the
// context locks, so it drains while they are held.
struct StreamDrain {
    std::vector<std::pair<int, hipStream_t>> s;
    void add(int dev, hipStream_t st) {
        for (auto& x : s)
            if (x.second == st) return;
        s.emplace_back(dev, st);
    }
    // returns the first failure (GGS_OK if none) and empties the list
    int drain() {
        int rc = GGS_OK;
        for (auto& x : s) {
            DeviceGuard dg(x.first);
            const hipError_t e = hipStreamSynchronize(x.second);
            if (e != hipSuccess && rc == GGS_OK)
                rc = fail(GGS_EHIP, "hipStreamSynchronize: %s", hipGetErrorString(e));
        }
        s.clear();
        return rc;
    }
    ~StreamDrain() {
        const std::string keep = t_err;          // an error return keeps its own message
        (void)drain();
        t_err = keep;
    }
};

// Test hook (GGS_TEST_FAIL_AFTER_ENQUEUE=d): the host API fails with GGS_EHIP
// right after queueing device d's work (d from 1), as a HIP failure on a later
// shard would; read per call.
bool inject_fail_after(int d) {
    const char* v = getenv("GGS_TEST_FAIL_AFTER_ENQUEUE");
    return v && atoi(v) == d;
}

int init_locked(int max_devices) {
    if (g_inited) return (int)g_ctx.size();
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(GGS_ENODEV, "no HIP device available (%s); the reference asserts a GPU too "
                                "(render.py:217)", e != hipSuccess ? hipGetErrorString(e) : "count=0");
    if (max_devices > 0) n = std::min(n, max_devices);
    g_ctx.resize(n);              // contexts are created on first use (ctx_locked)
    g_active.clear();
    for (int d = 0; d < n; ++d) g_active.push_back(d);
    g_inited = true;
    return n;
}

// Context of device d, created on first use (one stream per device).  g_mu held.
int ctx_locked(int d, DevCtx** out) {
    if (d < 0 || d >= (int)g_ctx.size())
        return fail(GGS_EINVAL, "device %d out of range (have %d)", d, (int)g_ctx.size());
    if (!g_ctx[d]) {
        auto c = std::make_unique<DevCtx>();
        c->dev = d;
        DeviceGuard dg(d);
        GGS_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->simds = device_simds(d);
        g_ctx[d] = std::move(c);
    }
    *out = g_ctx[d].get();
    return GGS_OK;
}

}  // namespace

int get_ctx(int device, DevCtx** out) {
    std::lock_guard<std::mutex> lk(g_mu);
    const int rc = init_locked(0);
    if (rc < 0) return rc;
    return ctx_locked(device, out);
}

namespace {

// The first n (<=0: all) devices of the active list, contexts created.
int active_ctxs(int32_t n_devices, std::vector<DevCtx*>* out) {
    std::lock_guard<std::mutex> lk(g_mu);
    int rc = init_locked(0);
    if (rc < 0) return rc;
    const int have = (int)g_active.size();
    const int n = n_devices <= 0 ? have : std::min<int>(n_devices, have);
    out->clear();
    for (int i = 0; i < n; ++i) {
        DevCtx* c;
        if ((rc = ctx_locked(g_active[i], &c))) return rc;
        out->push_back(c);
    }
    return GGS_OK;
}

}  // namespace

Workspace* workspace_for(DevCtx* c, hipStream_t st) {
    for (auto& w : c->ws)
        if (w->stream == st) return w.get();
    c->ws.push_back(std::make_unique<Workspace>());
    c->ws.back()->stream = st;
    return c->ws.back().get();
}

// xxhash64-style content hash (target/mask upload cache)
uint64_t hash_bytes(const void* data, size_t n) {
    const uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full, P3 = 0x165667B19E3779F9ull;
    const unsigned char* p = (const unsigned char*)data;
    uint64_t v[4] = {P1 + P2, P2, 0, 0 - P1};
    size_t i = 0;
    for (; i + 32 <= n; i += 32) {
        for (int k = 0; k < 4; ++k) {
            uint64_t w;
            memcpy(&w, p + i + 8 * k, 8);
            v[k] = rotl(v[k] + w * P2, 31) * P1;
        }
    }
    uint64_t h = rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18) + n;
    for (; i < n; ++i) h = rotl(h ^ (p[i] * P3), 11) * P1;
    h ^= h >> 33;
    h *= P2;
    h ^= h >> 29;
    h *= P3;
    h ^= h >> 32;
    return h;
}

int check_dims(int64_t B, int32_t N, int32_t C, int32_t H, int32_t W) {
    if (B < 0 || N < 0) return fail(GGS_EINVAL, "B=%lld and N=%d must be >= 0", (long long)B, N);
    if (C < 9) return fail(GGS_EINVAL, "expected at least 9 genome cols, got C=%d (render.py:223)", C);
    if (H < 1 || W < 1) return fail(GGS_EINVAL, "H=%d, W=%d must be >= 1", H, W);
    // the raster's cull list holds 32-bit byte offsets of 64-B records: N * 64 < 2^31
    // (N <= 512 launches pack the visit's control into the offset's free bits)
    if ((int64_t)N * (int64_t)sizeof(SplatRec) >= ((int64_t)1 << 31))
        return fail(GGS_EINVAL, "N=%d splats per candidate exceeds the limit %lld", N,
                    (long long)(((int64_t)1 << 31) / (int64_t)sizeof(SplatRec) - 1));
    int nTX;
    const int64_t nTiles = raster_tiles(H, W, &nTX);
    if (B * nTiles * 4 >= (int64_t)1 << 31)
        return fail(GGS_EINVAL, "B*tiles = %lld exceeds the grid limit; split the batch",
                    (long long)(B * nTiles * 4));
    return GGS_OK;
}

// ---- the device pipelines (ctx locked, device set) ----------------------------------
// The workspace's strip-word buffers for a batch of B x N splats where the batch
// qualifies and the switch is on (else *sw stays empty: the raster culls from bnds).
static int ensure_strip_words(Workspace* w, int64_t B, int N, int H, int W, hipStream_t st, StripWords* sw) {
    if (!strip_words_ok(N) || !strip_words_on()) return GGS_OK;
    int rc;
    if ((rc = ensure(w->swords, strip_words_bytes(B, N, H, W), st))) return rc;
    if ((rc = ensure(w->smasks, strip_masks_bytes(B, N, H, W), st))) return rc;
    sw->words = (int*)w->swords.p;
    sw->masks = (uint64_t*)w->smasks.p;
    // the strip table of the workspace's tile order (ensure_tile_order(w, H, W) came first)
    if (w->order_H == H && w->order_W == W && w->strips_ok)
        sw->table = (const int*)w->order.p + raster_order_len(H, W);
    return GGS_OK;
}

int run_fitness(DevCtx* c, hipStream_t st, const float* d_gen, int64_t B, int N, int C,
                const float* d_target, const float* d_mask, int mode, float beta, int H, int W,
                float k, float* d_out, uint64_t plan_key) {
    if (B == 0) return GGS_OK;
    Workspace* w = workspace_for(c, st);
    int nTX;
    const int nTiles = raster_tiles(H, W, &nTX);
    int rc;
    if ((rc = ensure(w->recs, sizeof(SplatRec) * (size_t)std::max<int64_t>(B * N, 1), st))) return rc;
    if ((rc = ensure(w->bnds, sizeof(int4) * (size_t)std::max<int64_t>(B * N, 1), st))) return rc;
    // one partial per (candidate, tile, 16-column strip)
    if ((rc = ensure(w->partials, sizeof(float) * 4 * (size_t)(B * nTiles), st))) return rc;
    if ((rc = ensure(w->wpartials, plan_wsum_bytes(H, W), st))) return rc;
    if ((rc = ensure_tile_order(w, H, W, st))) return rc;
    if (plan_key == 0 || plan_key != w->plan_key) {
        if ((rc = ensure(w->plan, plan_bytes(H, W), st))) return rc;
        GGS_HIP(launch_plan(st, d_target, d_mask, mode, beta, H, W, (float4*)w->plan.p,
                            (float*)w->wpartials.p));
        w->plan_key = plan_key;
    }
    return run_fitness_planned(c, st, d_gen, B, N, C, (const float4*)w->plan.p,
                               (const float*)w->wpartials.p, mode, H, W, k, d_out);
}

int run_fitness_planned(DevCtx* c, hipStream_t st, const float* d_gen, int64_t B, int N, int C,
                        const float4* plan, const float* wpartials, int mode, int H, int W, float k,
                        float* d_out, int group) {
    if (B == 0) return GGS_OK;
    Workspace* w = workspace_for(c, st);
    int nTX;
    const int nTiles = raster_tiles(H, W, &nTX);
    int rc;
    if ((rc = ensure(w->recs, sizeof(SplatRec) * (size_t)std::max<int64_t>(B * N, 1), st))) return rc;
    if ((rc = ensure(w->bnds, sizeof(int4) * (size_t)std::max<int64_t>(B * N, 1), st))) return rc;
    if ((rc = ensure(w->partials, sizeof(float) * 4 * (size_t)(B * nTiles), st))) return rc;
    if ((rc = ensure_tile_order(w, H, W, st))) return rc;
    SplatRec* recs = (SplatRec*)w->recs.p;
    const bool fold = fitness_api_fold();
    StripWords sw;   // for the single-plan raster without the fold (the instances with visit words)
    if (group == 0 && !fold && (rc = ensure_strip_words(w, B, N, H, W, st, &sw))) return rc;
    {
        ProfScope ps(st, 0);
        GGS_HIP(launch_prep(st, true, d_gen, B * N, C, H, W, k, recs, (int4*)w->bnds.p, nullptr, nullptr, nullptr,
                            nullptr, 0, sw, N));
    }
    return raster_fitness(st, c->simds, recs, (const int4*)w->bnds.p, (int)B, N, H, W, plan, (float*)w->partials.p,
                          wpartials, mode, (const int*)w->order.p, w->fctr, d_out, fold, nullptr,
                          nullptr, group, sw);
}

int run_render(DevCtx* c, hipStream_t st, const float* d_gen, int64_t B, int N, int C, int H, int W,
               float k, const float bg[3], float* d_img, bool encode) {
    if (B == 0) return GGS_OK;
    Workspace* w = workspace_for(c, st);
    int rc;
    if ((rc = ensure(w->recs, sizeof(SplatRec) * (size_t)std::max<int64_t>(B * N, 1), st))) return rc;
    if ((rc = ensure(w->bnds, sizeof(int4) * (size_t)std::max<int64_t>(B * N, 1), st))) return rc;
    if ((rc = ensure_tile_order(w, H, W, st))) return rc;
    SplatRec* recs = (SplatRec*)w->recs.p;
    StripWords sw;
    if ((rc = ensure_strip_words(w, B, N, H, W, st, &sw))) return rc;
    {
        ProfScope ps(st, 0);
        GGS_HIP(launch_prep(st, encode, d_gen, B * N, C, H, W, k, recs, (int4*)w->bnds.p, nullptr, nullptr, nullptr,
                            nullptr, 0, sw, N));
    }
    {
        ProfScope ps(st, 1);
        GGS_HIP(launch_raster(st, 0, recs, (const int4*)w->bnds.p, (int)B, N, H, W, bg, d_img, nullptr, nullptr,
                              (const int*)w->order.p, nullptr, nullptr, nullptr, nullptr, c->simds, 0, sw));
    }
    return GGS_OK;
}

// The strip partials of the gradient in flight per launch: candidates are chunked
// to this budget (the raster's chunk policy, 40 MiB), and one candidate above it
// is refused rather than given a second layout.
constexpr size_t kGradChunkBytes = (size_t)40 << 20;

// Argument errors (GGS_EINVAL) and the workspace budget (GGS_ENOMEM), before any device is touched.
int check_grad_dims(int64_t B, int32_t N, int32_t C, int32_t H, int32_t W, int32_t mode, const void* mask) {
    if (B < 1 || N < 1) return fail(GGS_EINVAL, "B=%lld and N=%d must be >= 1", (long long)B, N);
    int rc = check_dims(B, N, C, H, W);
    if (rc) return rc;
    if (mode < GGS_FIT_NONE || mode > GGS_FIT_BOOST) return fail(GGS_EINVAL, "bad fitness mode %d", mode);
    if (mode != GGS_FIT_NONE && !mask) return fail(GGS_EINVAL, "mode %d needs a weight mask", mode);
    if (B * N >= (int64_t)1 << 31) return fail(GGS_EINVAL, "B*N = %lld splats exceeds the limit; split the batch",
                                               (long long)(B * N));
    const size_t per = grad_partial_bytes(N, H, W);
    if (per > kGradChunkBytes)
        return fail(GGS_ENOMEM, "the gradient's strip partials of one candidate (%d x %d, %d splats: %.0f MB) exceed "
                                "the %.0f MB workspace budget", H, W, N, per / 1048576.0, kGradChunkBytes / 1048576.0);
    return GGS_OK;
}

// The gradient launches of a batch whose fitness has just run: prep's stage outputs,
// then the strip / finish pair per chunk of candidates.  group == 0: one target and
// mask, wblocks its plan's weight block; group > 0: candidate b against image
// b / group of targets [K][H][W][3] / masks [K][H][W], wblocks the set's blocks.
int run_grad_chunks(Workspace* w, hipStream_t st, const float* d_gen, int64_t B, int N, int C, const float* d_targets,
                    const float* d_masks, int mode, float beta, int H, int W, float k, const float* wblocks,
                    int group, float* d_grad) {
    const size_t per = grad_partial_bytes(N, H, W);     // within the budget: check_grad_dims
    const int64_t S = B * N;
    const int chunk = (int)std::min<int64_t>(B, (int64_t)(kGradChunkBytes / per));
    int rc;
    if ((rc = ensure(w->gf9, sizeof(float) * 9 * (size_t)S, st))) return rc;
    if ((rc = ensure(w->gi4, sizeof(int) * 4 * (size_t)S, st))) return rc;
    if ((rc = ensure(w->gpart, per * (size_t)chunk, st))) return rc;
    GGS_HIP(launch_prep(st, true, d_gen, S, C, H, W, k, nullptr, nullptr, (float*)w->gf9.p, (int*)w->gi4.p, nullptr));
    const int64_t wstride = (int64_t)(plan_wsum_bytes(H, W) / sizeof(float));
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int nb = (int)std::min<int64_t>(chunk, B - b0);
        if (group > 0)      // a chunk may begin inside a group: the kernel takes b / group of the absolute b
            GGS_HIP(launch_grad_set(st, d_gen, C, (const float*)w->gf9.p, (const int*)w->gi4.p, B, b0, nb, N, H, W,
                                    d_targets, d_masks, mode, beta, wblocks, wstride, group, w->gpart.p, d_grad));
        else
            GGS_HIP(launch_grad(st, d_gen, C, (const float*)w->gf9.p, (const int*)w->gi4.p, B, b0, nb, N, H, W,
                                d_targets, d_masks, mode, beta, wblocks, w->gpart.p, d_grad));
    }
    return GGS_OK;
}

// ggs_render_vjp*'s argument errors (GGS_EINVAL) and the workspace budget (GGS_ENOMEM):
// check_grad_dims' rules without mode and mask, before any device is touched.
int check_vjp_dims(int64_t B, int32_t N, int32_t C, int32_t layout, int32_t H, int32_t W) {
    if (layout != GGS_LAYOUT_RENDERER && layout != GGS_LAYOUT_AXES) return fail(GGS_EINVAL, "unknown layout %d", layout);
    return check_grad_dims(B, N, C, H, W, GGS_FIT_NONE, nullptr);
}

// The renderer's vector-Jacobian product: prep's stage outputs, then the
// strip / finish pair per chunk of candidates as run_grad_chunks; no fitness launch
// and no plan.  d_cot [B][H][W][3], d_grad [B][N][9].
int run_render_vjp(DevCtx* c, hipStream_t st, const float* d_gen, int64_t B, int N, int C, int layout, int H, int W,
                   float k, const float bg[3], const float* d_cot, float* d_grad) {
    Workspace* w = workspace_for(c, st);
    const size_t per = grad_partial_bytes(N, H, W);     // within the budget: check_vjp_dims
    const int64_t S = B * N;
    const int chunk = (int)std::min<int64_t>(B, (int64_t)(kGradChunkBytes / per));
    int rc;
    if ((rc = ensure(w->gf9, sizeof(float) * 9 * (size_t)S, st))) return rc;
    if ((rc = ensure(w->gi4, sizeof(int) * 4 * (size_t)S, st))) return rc;
    if ((rc = ensure(w->gpart, per * (size_t)chunk, st))) return rc;
    GGS_HIP(launch_prep(st, layout == GGS_LAYOUT_AXES, d_gen, S, C, H, W, k, nullptr, nullptr, (float*)w->gf9.p,
                        (int*)w->gi4.p, nullptr));
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int nb = (int)std::min<int64_t>(chunk, B - b0);
        GGS_HIP(launch_render_vjp(st, layout, d_gen, C, (const float*)w->gf9.p, (const int*)w->gi4.p, B, b0, nb, N, H,
                                  W, d_cot, bg, w->gpart.p, d_grad));
    }
    return GGS_OK;
}

// ---- image losses ----------------------------------------------------
int check_loss_params(const ggs_loss_params* p) {
    if (!p) return fail(GGS_EINVAL, "null ggs_loss_params");
    const float w[3] = {p->w_l1, p->w_mse, p->w_ssim};
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(w[i]) || w[i] < 0.0f)
            return fail(GGS_EINVAL, "loss weights (%g, %g, %g) must be finite and >= 0", w[0], w[1], w[2]);
    if (w[0] == 0.0f && w[1] == 0.0f && w[2] == 0.0f) return fail(GGS_EINVAL, "loss weights are all zero");
    return GGS_OK;
}

// ggs_image_loss*'s shape rules: the group rule of ggs_fitness_device_planset and a grid
// of B * tiles workgroups below 2^31.
int check_loss_dims(int64_t B, int32_t K, int32_t group, int32_t H, int32_t W) {
    if (B < 1) return fail(GGS_EINVAL, "B=%lld must be >= 1", (long long)B);
    if (H < 1 || W < 1) return fail(GGS_EINVAL, "H=%d, W=%d must be >= 1", H, W);
    if (group < 1) return fail(GGS_EINVAL, "group=%d must be >= 1", group);
    if (K < 1) return fail(GGS_EINVAL, "K=%d images: must be >= 1", K);
    if (B % group != 0) return fail(GGS_EINVAL, "B=%lld is not a multiple of group=%d", (long long)B, group);
    if (B / group > K)
        return fail(GGS_EINVAL, "B / group = %lld images wanted, the set holds %d", (long long)(B / group), K);
    if (B >= (int64_t)1 << 31 || B * image_loss_tiles(H, W) >= (int64_t)1 << 31)
        return fail(GGS_EINVAL, "B*tiles = %lld exceeds the grid limit; split the batch",
                    (long long)(B * image_loss_tiles(H, W)));
    return GGS_OK;
}

int run_image_loss(DevCtx* c, hipStream_t st, const float* d_img, int64_t B, const float* d_targets, int group, int H,
                   int W, const ggs_loss_params& p, float* d_loss, float* d_cot) {
    Workspace* w = workspace_for(c, st);
    int rc;
    if ((rc = ensure(w->lpart, image_loss_partial_bytes(B, H, W), st))) return rc;
    const float wt[3] = {p.w_l1, p.w_mse, p.w_ssim};
    GGS_HIP(launch_image_loss(st, d_img, B, d_targets, group, H, W, wt, w->lpart.p, d_loss, d_cot));
    return GGS_OK;
}

// ggs_loss_grad*'s argument errors: the VJP's, the loss's, the weights'.
int check_loss_grad(int64_t B, int32_t N, int32_t C, int32_t layout, int32_t K, int32_t group, int32_t H, int32_t W,
                    const ggs_loss_params* p) {
    int rc = check_vjp_dims(B, N, C, layout, H, W);
    if (rc == GGS_OK) rc = check_loss_dims(B, K, group, H, W);
    if (rc == GGS_OK) rc = check_loss_params(p);
    return rc;
}

int run_loss_grad(DevCtx* c, hipStream_t st, const float* d_gen, int64_t B, int N, int C, int layout,
                  const float* d_targets, int group, int H, int W, float k, const float bg[3],
                  const ggs_loss_params& p, float* d_loss, float* d_grad, float* d_img, float* d_cot) {
    int rc;
    if ((rc = run_render(c, st, d_gen, B, N, C, H, W, k, bg, d_img, layout == GGS_LAYOUT_AXES))) return rc;
    if ((rc = run_image_loss(c, st, d_img, B, d_targets, group, H, W, p, d_loss, d_cot))) return rc;
    return run_render_vjp(c, st, d_gen, B, N, C, layout, H, W, k, bg, d_cot, d_grad);
}

int run_fitness_grad(DevCtx* c, hipStream_t st, const float* d_gen, int64_t B, int N, int C, const float* d_target,
                     const float* d_mask, int mode, float beta, int H, int W, float k, float* d_out, float* d_grad,
                     uint64_t plan_key) {
    Workspace* w = workspace_for(c, st);
    int rc;
    if (!d_out) {
        if ((rc = ensure(w->gout, sizeof(float) * (size_t)B, st))) return rc;
        d_out = (float*)w->gout.p;
    }
    // first: it leaves the plan's weight block (the mode's Sum w) in the workspace
    if ((rc = run_fitness(c, st, d_gen, B, N, C, d_target, d_mask, mode, beta, H, W, k, d_out, plan_key))) return rc;
    return run_grad_chunks(w, st, d_gen, B, N, C, d_target, d_mask, mode, beta, H, W, k, (const float*)w->wpartials.p,
                           0, d_grad);
}

int run_fitness_grad_planned(DevCtx* c, hipStream_t st, const float* d_gen, int64_t B, int N, int C,
                             const float4* plan, const float* wblocks, const float* d_targets, const float* d_masks,
                             int mode, float beta, int H, int W, int group, float k, float* d_out, float* d_grad) {
    Workspace* w = workspace_for(c, st);
    int rc;
    if (!d_out) {
        if ((rc = ensure(w->gout, sizeof(float) * (size_t)B, st))) return rc;
        d_out = (float*)w->gout.p;
    }
    if ((rc = run_fitness_planned(c, st, d_gen, B, N, C, plan, wblocks, mode, H, W, k, d_out, group))) return rc;
    return run_grad_chunks(w, st, d_gen, B, N, C, d_targets, d_masks, mode, beta, H, W, k, wblocks, group, d_grad);
}

// ggs_fitness_device_planset's rules on top of check_grad_dims (K: the set's plans)
int check_grad_set(int64_t B, int32_t N, int32_t C, int32_t H, int32_t W, int32_t mode, const void* masks, int32_t K,
                   int32_t group) {
    if (group < 1) return fail(GGS_EINVAL, "group=%d must be >= 1", group);
    if (K < 1) return fail(GGS_EINVAL, "K=%d images: must be >= 1", K);
    int rc = check_grad_dims(B, N, C, H, W, mode, masks);
    if (rc) return rc;
    if (B % group != 0) return fail(GGS_EINVAL, "B=%lld is not a multiple of group=%d", (long long)B, group);
    if (B / group > K)
        return fail(GGS_EINVAL, "B / group = %lld images wanted, the set holds %d", (long long)(B / group), K);
    return GGS_OK;
}

namespace {

// Split [0, B) into n contiguous shards of ceil(B/n) (the last ones shorter or
// empty): equal-sized slots, so the fitness shards meet in one in-place RCCL
// all-gather (ggs/parallel.py shard_bounds: the same rule).
void shard(int64_t B, int n, int d, int64_t* b0, int64_t* nb) {
    const int64_t per = (B + n - 1) / n;
    *b0 = std::min<int64_t>(B, d * per);
    *nb = std::min<int64_t>(B, *b0 + per) - *b0;
}

// Single-process communicators over the active device list (host-API fan-out),
// made on first use with ggs_comm_init_local and remade when the list changes.
std::vector<int> g_comm_devs;
std::vector<void*> g_comms;

int local_comms_locked(const std::vector<DevCtx*>& cs, std::vector<void*>* out) {
    std::vector<int> devs;
    for (DevCtx* c : cs) devs.push_back(c->dev);
    if (devs != g_comm_devs) {
        for (void* c : g_comms) ggs_comm_destroy(c);
        g_comms.clear();
        g_comm_devs.clear();
        std::vector<void*> made(devs.size(), nullptr);
        const int rc = ggs_comm_init_local((int32_t)devs.size(), devs.data(), made.data());
        if (rc) return rc;
        g_comms = made;
        g_comm_devs = devs;
    }
    *out = g_comms;
    return GGS_OK;
}
std::mutex g_comm_mu;

}  // namespace
}  // namespace ggs

using namespace ggs;

extern "C" {

const char* ggs_version(void) { return "ggs-mi355x 0.4.0 (gfx950, " GGS_BUILD_KIND " build)"; }

int ggs_init(int32_t max_devices) {
    std::lock_guard<std::mutex> lk(g_mu);
    return init_locked(max_devices);
}

int ggs_device_count(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_inited ? (int)g_ctx.size() : 0;
}

int ggs_select_devices(const int32_t* ids, int32_t n) {
    std::lock_guard<std::mutex> lk(g_mu);
    int rc = init_locked(0);
    if (rc < 0) return rc;
    if (n < 0 || (n > 0 && !ids)) return fail(GGS_EINVAL, "bad device list");
    std::vector<int> act;
    for (int i = 0; i < n; ++i) {
        if (ids[i] < 0 || ids[i] >= (int)g_ctx.size())
            return fail(GGS_EINVAL, "device %d out of range (have %d)", ids[i], (int)g_ctx.size());
        if (std::find(act.begin(), act.end(), ids[i]) != act.end())
            return fail(GGS_EINVAL, "device %d listed twice", ids[i]);
        act.push_back(ids[i]);
    }
    if (act.empty())
        for (int d = 0; d < (int)g_ctx.size(); ++d) act.push_back(d);
    g_active = act;
    return (int)g_active.size();
}

const char* ggs_last_error(void) { return t_err.c_str(); }

void ggs_shutdown(void) {
    {
        std::lock_guard<std::mutex> cl(g_comm_mu);
        for (void* c : g_comms) ggs_comm_destroy(c);
        g_comms.clear();
        g_comm_devs.clear();
    }
    std::lock_guard<std::mutex> lk(g_mu);
    {
        std::lock_guard<std::mutex> pl(g_prof_mu);
        prof_drain_locked();
    }
    for (auto& c : g_ctx) {
        if (!c) continue;
        std::lock_guard<std::mutex> cl(c->mu);
        (void)hipSetDevice(c->dev);
        (void)hipStreamSynchronize(c->stream);
        for (auto& w : c->ws)
            if (w->stream) (void)hipStreamSynchronize(w->stream);
        // the workspaces and the staging free themselves here: device current, context locked
        static_cast<CtxBuffers&>(*c) = CtxBuffers{};
        (void)hipStreamDestroy(c->stream);
    }
    g_ctx.clear();      // the contexts own nothing by now
    g_active.clear();
    g_inited = false;
}

int ggs_fitness_device(int32_t device, void* stream, const float* d_genomes_axes, int64_t B, int32_t N,
                       int32_t C, const float* d_target_hw3, const float* d_mask_hw, int32_t mode,
                       float boost_beta, int32_t H, int32_t W, float k_sigma, float* d_out_B) {
    int rc = check_dims(B, N, C, H, W);
    if (rc) return rc;
    if (mode < GGS_FIT_NONE || mode > GGS_FIT_BOOST) return fail(GGS_EINVAL, "bad fitness mode %d", mode);
    if (mode != GGS_FIT_NONE && !d_mask_hw) return fail(GGS_EINVAL, "mode %d needs a weight mask", mode);
    if (B > 0 && (!d_genomes_axes && N > 0)) return fail(GGS_EINVAL, "null genomes");
    if (B > 0 && (!d_target_hw3 || !d_out_B)) return fail(GGS_EINVAL, "null target/out");
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    return run_fitness(c, (hipStream_t)stream, d_genomes_axes, B, N, C, d_target_hw3, d_mask_hw, mode,
                       boost_beta, H, W, k_sigma, d_out_B);
}

int ggs_fitness_grad_device(int32_t device, void* stream, const float* d_genomes_axes, int64_t B, int32_t N,
                            int32_t C, const float* d_target_hw3, const float* d_mask_hw, int32_t mode,
                            float boost_beta, int32_t H, int32_t W, float k_sigma, float* d_out_B, float* d_grad_BN9) {
    int rc = check_grad_dims(B, N, C, H, W, mode, d_mask_hw);
    if (rc) return rc;
    if (!d_genomes_axes || !d_target_hw3 || !d_grad_BN9) return fail(GGS_EINVAL, "null genomes/target/grad");
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    return run_fitness_grad(c, (hipStream_t)stream, d_genomes_axes, B, N, C, d_target_hw3, d_mask_hw, mode, boost_beta,
                            H, W, k_sigma, d_out_B, d_grad_BN9);
}

// ---- target plans (device API with a target prepared once) ------------------
}  // extern "C"
namespace ggs {
namespace {
struct TargetPlan {
    DevCtx* c = nullptr;
    int H = 0, W = 0, mode = 0;
    DevBuf plan, wpartials;
};
// K plans plan_bytes apart and K weight blocks plan_wsum_bytes apart (launch_plan_set)
struct PlanSet {
    DevCtx* c = nullptr;
    int H = 0, W = 0, mode = 0, K = 0;
    float beta = 0.0f;              // the gradient's strip kernel needs it in BOOST mode
    DevBuf plan, wpartials;
};
}  // namespace
}  // namespace ggs
extern "C" {

int ggs_plan_create(int32_t device, void* stream, const float* d_target_hw3, const float* d_mask_hw,
                    int32_t mode, float boost_beta, int32_t H, int32_t W, void** plan) {
    int rc = check_dims(1, 1, 9, H, W);
    if (rc) return rc;
    if (!plan || !d_target_hw3) return fail(GGS_EINVAL, "null argument");
    if (mode < GGS_FIT_NONE || mode > GGS_FIT_BOOST) return fail(GGS_EINVAL, "bad fitness mode %d", mode);
    if (mode != GGS_FIT_NONE && !d_mask_hw) return fail(GGS_EINVAL, "mode %d needs a weight mask", mode);
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    auto p = std::make_unique<TargetPlan>();
    p->c = c;
    p->H = H;
    p->W = W;
    p->mode = mode;
    const hipStream_t st = (hipStream_t)stream;
    // (an error return frees the plan's buffers with it, before the lock is released)
    if ((rc = ensure(p->plan, plan_bytes(H, W), st)) ||
        (rc = ensure(p->wpartials, plan_wsum_bytes(H, W), st)))
        return rc;
    if (launch_plan(st, d_target_hw3, d_mask_hw, mode, boost_beta, H, W, (float4*)p->plan.p,
                    (float*)p->wpartials.p) != hipSuccess)
        return fail(GGS_EHIP, "plan launch failed");
    *plan = p.release();
    return GGS_OK;
}

int ggs_fitness_device_planned(void* plan, void* stream, const float* d_genomes_axes, int64_t B,
                               int32_t N, int32_t C, float k_sigma, float* d_out_B) {
    if (!plan) return fail(GGS_EINVAL, "null plan");
    TargetPlan* p = (TargetPlan*)plan;
    int rc = check_dims(B, N, C, p->H, p->W);
    if (rc) return rc;
    if (B > 0 && ((!d_genomes_axes && N > 0) || !d_out_B)) return fail(GGS_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(p->c->mu);
    DeviceGuard dg(p->c->dev);
    return run_fitness_planned(p->c, (hipStream_t)stream, d_genomes_axes, B, N, C,
                               (const float4*)p->plan.p, (const float*)p->wpartials.p, p->mode, p->H,
                               p->W, k_sigma, d_out_B);
}

void ggs_plan_destroy(void* plan) {
    if (!plan) return;
    TargetPlan* p = (TargetPlan*)plan;
    std::lock_guard<std::mutex> lk(p->c->mu);
    DeviceGuard dg(p->c->dev);
    (void)hipDeviceSynchronize();    // streams that may still read the plan
    delete p;
}

// ---- plan sets: K target plans of one (H, W, mode, beta) ------------------------
int ggs_planset_create(int32_t device, void* stream, const float* d_targets_khw3, const float* d_masks_khw,
                       int32_t mode, float boost_beta, int32_t H, int32_t W, int32_t K, void** planset) {
    if (!planset || !d_targets_khw3) return fail(GGS_EINVAL, "null argument");
    if (K < 1) return fail(GGS_EINVAL, "K=%d plans: must be >= 1", K);
    if (mode < GGS_FIT_NONE || mode > GGS_FIT_BOOST) return fail(GGS_EINVAL, "bad fitness mode %d", mode);
    if (mode != GGS_FIT_NONE && !d_masks_khw) return fail(GGS_EINVAL, "mode %d needs the weight masks", mode);
    // (the set's strips are numbered through in 32 bits: K * tiles * 4 < 2^31)
    int rc = check_dims(K, 1, 9, H, W);
    if (rc) return rc;
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    auto p = std::make_unique<PlanSet>();
    p->c = c;
    p->H = H;
    p->W = W;
    p->mode = mode;
    p->K = K;
    p->beta = boost_beta;
    const hipStream_t st = (hipStream_t)stream;
    if ((rc = ensure(p->plan, (size_t)K * plan_bytes(H, W), st)) ||
        (rc = ensure(p->wpartials, (size_t)K * plan_wsum_bytes(H, W), st)))
        return rc;
    if (launch_plan_set(st, d_targets_khw3, d_masks_khw, mode, boost_beta, H, W, K, (float4*)p->plan.p,
                        (float*)p->wpartials.p) != hipSuccess)
        return fail(GGS_EHIP, "plan launch failed");
    *planset = p.release();
    return GGS_OK;
}

int ggs_fitness_device_planset(void* planset, void* stream, const float* d_genomes_axes, int64_t B, int32_t N,
                               int32_t C, int32_t group, float k_sigma, float* d_out_B) {
    if (group < 1) return fail(GGS_EINVAL, "group=%d must be >= 1", group);
    if (B % group != 0) return fail(GGS_EINVAL, "B=%lld is not a multiple of group=%d", (long long)B, group);
    if (!planset) return fail(GGS_EINVAL, "null plan set");
    PlanSet* p = (PlanSet*)planset;
    int rc = check_dims(B, N, C, p->H, p->W);
    if (rc) return rc;
    if (B / group > p->K)
        return fail(GGS_EINVAL, "B / group = %lld plans wanted, the set holds %d", (long long)(B / group), p->K);
    if (!d_out_B || (!d_genomes_axes && B > 0 && N > 0)) return fail(GGS_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(p->c->mu);
    DeviceGuard dg(p->c->dev);
    return run_fitness_planned(p->c, (hipStream_t)stream, d_genomes_axes, B, N, C, (const float4*)p->plan.p,
                               (const float*)p->wpartials.p, p->mode, p->H, p->W, k_sigma, d_out_B, group);
}

int ggs_fitness_grad_device_planset(void* planset, void* stream, const float* d_genomes_axes, int64_t B, int32_t N,
                                    int32_t C, int32_t group, const float* d_targets_khw3, const float* d_masks_khw,
                                    float k_sigma, float* d_out_B, float* d_grad_BN9) {
    if (!planset) return fail(GGS_EINVAL, "null plan set");
    PlanSet* p = (PlanSet*)planset;
    int rc = check_grad_set(B, N, C, p->H, p->W, p->mode, d_masks_khw, p->K, group);
    if (rc) return rc;
    if (!d_genomes_axes || !d_targets_khw3 || !d_grad_BN9) return fail(GGS_EINVAL, "null genomes/targets/grad");
    std::lock_guard<std::mutex> lk(p->c->mu);
    DeviceGuard dg(p->c->dev);
    return run_fitness_grad_planned(p->c, (hipStream_t)stream, d_genomes_axes, B, N, C, (const float4*)p->plan.p,
                                    (const float*)p->wpartials.p, d_targets_khw3, d_masks_khw, p->mode, p->beta,
                                    p->H, p->W, group, k_sigma, d_out_B, d_grad_BN9);
}

void ggs_planset_destroy(void* planset) {
    if (!planset) return;
    PlanSet* p = (PlanSet*)planset;
    std::lock_guard<std::mutex> lk(p->c->mu);
    DeviceGuard dg(p->c->dev);
    (void)hipDeviceSynchronize();    // streams that may still read the plans
    delete p;
}

// ---- target preparation and importance mask ------------------------------------
}  // extern "C"
namespace ggs {
namespace {
int check_prepare(const void* images, int32_t K, int32_t H0, int32_t W0, int32_t H, int32_t W,
                  const ggs_mask_params* p, const void* targets, const void* masks) {
    if (K < 1 || K > 65535) return fail(GGS_EINVAL, "K=%d images: must be in 1..65535", K);
    if (!images || !targets) return fail(GGS_EINVAL, "null images / targets pointer");
    if (p && !masks) return fail(GGS_EINVAL, "null masks pointer (params given)");
    if (!p && masks) return fail(GGS_EINVAL, "masks wanted without params (params == NULL: targets only)");
    if (H0 < 1 || W0 < 1 || H < 1 || W < 1)
        return fail(GGS_EINVAL, "H0=%d, W0=%d, H=%d, W=%d must be >= 1", H0, W0, H, W);
    if ((int64_t)H * W >= ((int64_t)1 << 29) || (int64_t)H0 * W0 >= ((int64_t)1 << 29))
        return fail(GGS_EINVAL, "image of %lld or %lld pixels exceeds the limit 2^29", (long long)H0 * W0,
                    (long long)H * W);
    if (!p) return GGS_OK;
    if (std::min(H, W) < 4) return fail(GGS_EINVAL, "min(H, W) = %d: the mask needs at least 4", std::min(H, W));
    if (p->n_scales < 1 || p->n_scales > 4) return fail(GGS_EINVAL, "n_scales=%d must be in 1..4", p->n_scales);
    for (int i = 0; i < p->n_scales; ++i) {
        const int s = p->edge_scales[i];
        if (s < 1) return fail(GGS_EINVAL, "edge scale %d must be >= 1", s);
        if (H / s < 1 || W / s < 1) return fail(GGS_EINVAL, "edge scale %d leaves no pixel of %dx%d", s, H, W);
    }
    if (p->smooth > 0 && p->smooth % 2 == 0)
        return fail(GGS_EINVAL, "smooth=%d must be odd (an even window changes the array's size)", p->smooth);
    return GGS_OK;
}

// ctx locked, device set
int run_targets_prepare(DevCtx* c, hipStream_t st, const float* d_images, int K, int H0, int W0, int H, int W,
                        const ggs_mask_params* p, float* d_targets, float* d_masks) {
    Workspace* w = workspace_for(c, st);
    int rc;
    if ((rc = ensure(w->maskws, targets_prepare_ws_bytes(K, H, W, p != nullptr), st))) return rc;
    GGS_HIP(launch_targets_prepare(st, d_images, K, H0, W0, H, W, p, d_targets, d_masks, w->maskws.p));
    return GGS_OK;
}
}  // namespace
}  // namespace ggs
extern "C" {

int ggs_targets_prepare_device(int32_t device, void* stream, const float* d_images, int32_t K, int32_t H0,
                               int32_t W0, int32_t H, int32_t W, const ggs_mask_params* params,
                               float* d_targets_khw3, float* d_masks_khw) {
    int rc = check_prepare(d_images, K, H0, W0, H, W, params, d_targets_khw3, d_masks_khw);
    if (rc) return rc;
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    return run_targets_prepare(c, (hipStream_t)stream, d_images, K, H0, W0, H, W, params, d_targets_khw3,
                               d_masks_khw);
}

int ggs_targets_prepare(const float* images, int32_t K, int32_t H0, int32_t W0, int32_t H, int32_t W,
                        const ggs_mask_params* params, float* targets, float* masks, int32_t device) {
    int rc = check_prepare(images, K, H0, W0, H, W, params, targets, masks);
    if (rc) return rc;
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    const hipStream_t st = c->stream;
    const size_t ib = sizeof(float) * 3 * (size_t)K * H0 * W0, tb = sizeof(float) * 3 * (size_t)K * H * W,
                 mb = sizeof(float) * (size_t)K * H * W;
    if ((rc = ensure(c->prep_in, ib, st)) || (rc = ensure(c->prep_tgt, tb, st)) ||
        (params && (rc = ensure(c->prep_mask, mb, st))))
        return rc;
    StreamDrain drain;
    drain.add(c->dev, st);
    GGS_HIP(hipMemcpyAsync(c->prep_in.p, images, ib, hipMemcpyHostToDevice, st));
    if ((rc = run_targets_prepare(c, st, (const float*)c->prep_in.p, K, H0, W0, H, W, params, (float*)c->prep_tgt.p,
                                  params ? (float*)c->prep_mask.p : nullptr)))
        return rc;
    GGS_HIP(hipMemcpyAsync(targets, c->prep_tgt.p, tb, hipMemcpyDeviceToHost, st));
    if (params) GGS_HIP(hipMemcpyAsync(masks, c->prep_mask.p, mb, hipMemcpyDeviceToHost, st));
    return drain.drain();
}

int ggs_quantiles(const float* x, int64_t n, const double* q, int32_t nq, float* out) {
    if (!x || !q || !out) return fail(GGS_EINVAL, "null pointer");
    if (n < 1 || n >= ((int64_t)1 << 31)) return fail(GGS_EINVAL, "n=%lld must be in 1..2^31-1", (long long)n);
    if (nq < 1 || nq > kMaxQuantiles) return fail(GGS_EINVAL, "nq=%d must be in 1..%d", nq, kMaxQuantiles);
    for (int i = 0; i < nq; ++i)
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return fail(GGS_EINVAL, "q[%d]=%g is outside [0, 1]", i, q[i]);
    int rc;
    std::vector<DevCtx*> cs;
    if ((rc = active_ctxs(1, &cs))) return rc;
    DevCtx* c = cs[0];
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    const hipStream_t st = c->stream;
    Workspace* w = workspace_for(c, st);
    const size_t xb = sizeof(float) * (size_t)n;
    if ((rc = ensure(c->prep_in, xb, st)) || (rc = ensure(c->prep_mask, sizeof(float) * kMaxQuantiles, st)) ||
        (rc = ensure(w->maskws, quantile_ws_bytes(1, nq), st)))
        return rc;
    StreamDrain drain;
    drain.add(c->dev, st);
    GGS_HIP(hipMemcpyAsync(c->prep_in.p, x, xb, hipMemcpyHostToDevice, st));
    GGS_HIP(launch_quantiles(st, (const float*)c->prep_in.p, 1, n, q, nq, w->maskws.p, (float*)c->prep_mask.p));
    GGS_HIP(hipMemcpyAsync(out, c->prep_mask.p, sizeof(float) * nq, hipMemcpyDeviceToHost, st));
    return drain.drain();
}

int ggs_render_device(int32_t device, void* stream, const float* d_genomes, int64_t B, int32_t N,
                      int32_t C, int32_t H, int32_t W, float k_sigma, const float* bg,
                      float* d_out_bhw3) {
    int rc = check_dims(B, N, C, H, W);
    if (rc) return rc;
    if (B > 0 && ((!d_genomes && N > 0) || !d_out_bhw3)) return fail(GGS_EINVAL, "null pointer");
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    const float bg1[3] = {1.f, 1.f, 1.f};
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    return run_render(c, (hipStream_t)stream, d_genomes, B, N, C, H, W, k_sigma, bg ? bg : bg1, d_out_bhw3);
}

int ggs_render_layout_device(int32_t device, void* stream, const float* d_genomes, int64_t B, int32_t N, int32_t C,
                             int32_t layout, int32_t H, int32_t W, float k_sigma, const float* bg,
                             float* d_out_bhw3) {
    if (layout != GGS_LAYOUT_RENDERER && layout != GGS_LAYOUT_AXES) return fail(GGS_EINVAL, "unknown layout %d", layout);
    int rc = check_dims(B, N, C, H, W);
    if (rc) return rc;
    if (B > 0 && ((!d_genomes && N > 0) || !d_out_bhw3)) return fail(GGS_EINVAL, "null pointer");
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    const float bg1[3] = {1.f, 1.f, 1.f};
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    return run_render(c, (hipStream_t)stream, d_genomes, B, N, C, H, W, k_sigma, bg ? bg : bg1, d_out_bhw3,
                      layout == GGS_LAYOUT_AXES);
}

int ggs_render_vjp_device(int32_t device, void* stream, const float* d_genomes, int64_t B, int32_t N, int32_t C,
                          int32_t layout, int32_t H, int32_t W, float k_sigma, const float* bg,
                          const float* d_cot_bhw3, float* d_grad_BN9) {
    int rc = check_vjp_dims(B, N, C, layout, H, W);
    if (rc) return rc;
    if (!d_genomes || !d_cot_bhw3 || !d_grad_BN9) return fail(GGS_EINVAL, "null genomes/cotangent/grad");
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    const float bg1[3] = {1.f, 1.f, 1.f};
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    return run_render_vjp(c, (hipStream_t)stream, d_genomes, B, N, C, layout, H, W, k_sigma, bg ? bg : bg1,
                          d_cot_bhw3, d_grad_BN9);
}

int ggs_image_loss_device(int32_t device, void* stream, const float* d_img_bhw3, int64_t B,
                          const float* d_targets_khw3, int32_t K, int32_t group, int32_t H, int32_t W,
                          const ggs_loss_params* p, float* d_loss_B, float* d_cot_bhw3) {
    int rc = check_loss_dims(B, K, group, H, W);
    if (rc) return rc;
    if ((rc = check_loss_params(p))) return rc;
    if (!d_img_bhw3 || !d_targets_khw3 || !d_loss_B) return fail(GGS_EINVAL, "null image/targets/loss");
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    return run_image_loss(c, (hipStream_t)stream, d_img_bhw3, B, d_targets_khw3, group, H, W, *p, d_loss_B,
                          d_cot_bhw3);
}

int ggs_loss_grad_device(int32_t device, void* stream, const float* d_genomes, int64_t B, int32_t N, int32_t C,
                         int32_t layout, const float* d_targets_khw3, int32_t K, int32_t group, int32_t H, int32_t W,
                         float k_sigma, const float* bg, const ggs_loss_params* p, float* d_loss_B,
                         float* d_grad_BN9) {
    int rc = check_loss_grad(B, N, C, layout, K, group, H, W, p);
    if (rc) return rc;
    if (!d_genomes || !d_targets_khw3 || !d_loss_B || !d_grad_BN9)
        return fail(GGS_EINVAL, "null genomes/targets/loss/grad");
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    const float bg1[3] = {1.f, 1.f, 1.f};
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    hipStream_t st = (hipStream_t)stream;
    Workspace* w = workspace_for(c, st);
    const size_t vbytes = sizeof(float) * 3 * (size_t)H * W * (size_t)B;
    if ((rc = ensure(w->limg, vbytes, st)) || (rc = ensure(w->lcot, vbytes, st))) return rc;
    return run_loss_grad(c, st, d_genomes, B, N, C, layout, d_targets_khw3, group, H, W, k_sigma, bg ? bg : bg1, *p,
                         d_loss_B, d_grad_BN9, (float*)w->limg.p, (float*)w->lcot.p);
}

}  // extern "C"

namespace ggs {
namespace {
uint64_t host_plan_key(uint64_t tkey, uint64_t mkey, float boost_beta, int mode, int H, int W) {
    uint32_t bb;
    memcpy(&bb, &boost_beta, 4);
    return (((tkey * 0x9E3779B97F4A7C15ull) ^ (mkey + 0x632BE59BD9B4E019ull) ^ ((uint64_t)bb << 8) ^
             ((uint64_t)mode << 2) ^ ((uint64_t)H << 40) ^ ((uint64_t)W << 20)) & ~(1ull << 63)) | 1;
}

// Upload the caller's target or mask into its staging buffer (large enough) when the
// content key or the byte count differs from what the buffer holds.
int upload_if_changed(DevBuf& buf, uint64_t* held_key, size_t* held_bytes, const float* src, uint64_t key,
                      size_t bytes, hipStream_t st) {
    if (key == *held_key && bytes == *held_bytes) return GGS_OK;
    GGS_HIP(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, st));
    *held_key = key;
    *held_bytes = bytes;
    return GGS_OK;
}

// A host call on one device: the context lock, the device guard, the context's stream
// and, declared after the lock so that it drains while the lock is held, the drain
// that synchronises the stream on every return.
struct HostCall {
    DevCtx* c;
    std::lock_guard<std::mutex> lk;
    DeviceGuard dg;
    hipStream_t st;
    StreamDrain drain;
    explicit HostCall(DevCtx* ctx) : c(ctx), lk(ctx->mu), dg(ctx->dev), st(ctx->stream) {}
    // the previous call's work is done with the staging; what follows is drained
    int begin() {
        GGS_HIP(hipStreamSynchronize(st));
        drain.add(c->dev, st);
        return GGS_OK;
    }
};

// One device, host arrays in and out.  The content hashes of target and mask
// (4 MB at 512^2: ~0.2 ms on one core) decide whether the device copies cached
// from an earlier call are still right.  A GA passes the same arrays every
// generation, so the evaluation is enqueued against the cached copies first and
// the arrays are hashed while the GPU runs; only if the contents changed is the
// result discarded and the evaluation redone with the new inputs (same bits as
// hashing first).  *done = 0: nothing cached yet, the caller takes the plain path.
int fitness_one_device_speculative(DevCtx* c, const float* genomes_axes, int64_t B, int N, int C,
                                   const float* target_hw3, const float* mask_hw, int mode, float boost_beta,
                                   int H, int W, float k_sigma, float* out_B, int* done) {
    *done = 0;
    const size_t tbytes = sizeof(float) * 3 * (size_t)H * W, mbytes = sizeof(float) * (size_t)H * W;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->target_key == 0 || c->target_bytes != tbytes || !c->target.p ||
        (mask_hw && (c->mask_key == 0 || c->mask_bytes != mbytes || !c->mask.p)))
        return GGS_OK;
    DeviceGuard dg(c->dev);
    hipStream_t st = c->stream;
    const size_t gbytes = sizeof(float) * (size_t)N * C * (size_t)B;
    int rc;
    if ((rc = ensure(c->out, sizeof(float) * (size_t)B, st))) return rc;
    if ((rc = ensure_pinned(c->h_out, sizeof(float) * (size_t)B))) return rc;
    if ((rc = ensure(c->gen, std::max<size_t>(gbytes, 4), st))) return rc;
    GGS_HIP(hipStreamSynchronize(st));  // the previous call's work is done with c->gen
    StreamDrain drain;                  // after the context lock: drained on every return
    drain.add(c->dev, st);
    // straight from the caller's (pageable) array: the runtime's own staged copy
    // beat a memcpy into our pinned buffer + its upload by ~25 us per call at
    // 512^2/256/128 (1.18 MB: 240 -> 215 us per call; docs/EXPERIMENTS.md §15).  The
    // array stays valid for the whole call, which syncs before returning.
    if (gbytes) GGS_HIP(hipMemcpyAsync(c->gen.p, genomes_axes, gbytes, hipMemcpyHostToDevice, st));
    const uint64_t mkey_c = mask_hw ? c->mask_key : 0;
    auto evaluate = [&](uint64_t tk, uint64_t mk) {
        int r = run_fitness(c, st, (const float*)c->gen.p, B, N, C, (const float*)c->target.p,
                            mask_hw ? (const float*)c->mask.p : nullptr, mode, boost_beta, H, W, k_sigma,
                            (float*)c->out.p, host_plan_key(tk, mk, boost_beta, mode, H, W));
        if (r) return r;
        GGS_HIP(hipMemcpyAsync(c->h_out.p, c->out.p, sizeof(float) * (size_t)B, hipMemcpyDeviceToHost, st));
        return GGS_OK;
    };
    if ((rc = evaluate(c->target_key, mkey_c))) return rc;
    if (inject_fail_after(1)) return fail(GGS_EHIP, "injected failure after device 1's work (test hook)");
    const uint64_t tkey = hash_bytes(target_hw3, tbytes);      // while the GPU runs
    const uint64_t mkey = mask_hw ? hash_bytes(mask_hw, mbytes) : 0;
    if ((rc = drain.drain())) return rc;
    if (tkey != c->target_key || mkey != mkey_c) {            // changed: redo with the new inputs
        drain.add(c->dev, st);
        if ((rc = upload_if_changed(c->target, &c->target_key, &c->target_bytes, target_hw3, tkey, tbytes, st)) ||
            (mask_hw &&
             (rc = upload_if_changed(c->mask, &c->mask_key, &c->mask_bytes, mask_hw, mkey, mbytes, st))))
            return rc;
        if ((rc = evaluate(tkey, mkey))) return rc;
        if ((rc = drain.drain())) return rc;
    }
    memcpy(out_B, c->h_out.p, sizeof(float) * (size_t)B);
    *done = 1;
    return GGS_OK;
}
}  // namespace
}  // namespace ggs

extern "C" {

int ggs_fitness(const float* genomes_axes, int64_t B, int32_t N, int32_t C, const float* target_hw3,
                const float* mask_hw, int32_t mode, float boost_beta, int32_t H, int32_t W,
                float k_sigma, float* out_B, int32_t n_devices) {
    int rc = check_dims(B, N, C, H, W);
    if (rc) return rc;
    if (mode < GGS_FIT_NONE || mode > GGS_FIT_BOOST) return fail(GGS_EINVAL, "bad fitness mode %d", mode);
    if (mode != GGS_FIT_NONE && !mask_hw) return fail(GGS_EINVAL, "mode %d needs a weight mask", mode);
    if (B == 0) return GGS_OK;
    if ((!genomes_axes && N > 0) || !target_hw3 || !out_B) return fail(GGS_EINVAL, "null pointer");
    std::vector<DevCtx*> cs;
    if ((rc = active_ctxs(n_devices, &cs))) return rc;
    const int nd = (int)cs.size();
    const size_t tbytes = sizeof(float) * 3 * (size_t)H * W, mbytes = sizeof(float) * (size_t)H * W;
    const size_t row = (size_t)N * C;
    // RCCL gather of the shards (GGS_FANOUT_RCCL=1 forces it at one device: tests)
    static const bool force_rccl = getenv("GGS_FANOUT_RCCL") && atoi(getenv("GGS_FANOUT_RCCL")) != 0;
    const bool gather = nd > 1 || force_rccl;
    if (!gather) {
        int done = 0;
        if ((rc = fitness_one_device_speculative(cs[0], genomes_axes, B, N, C, target_hw3, mask_hw, mode,
                                                 boost_beta, H, W, k_sigma, out_B, &done)) || done)
            return rc;
    }
    const uint64_t tkey = hash_bytes(target_hw3, tbytes);
    const uint64_t mkey = mask_hw ? hash_bytes(mask_hw, mbytes) : 0;
    const int64_t per = (B + nd - 1) / nd;

    std::vector<std::unique_lock<std::mutex>> locks;
    for (int d = 0; d < nd; ++d) locks.emplace_back(cs[d]->mu);
    StreamDrain drain;                  // every stream given work is synchronised on any return
    // enqueue on every device, then gather (nd > 1) and wait
    for (int d = 0; d < nd; ++d) {
        DevCtx* c = cs[d];
        int64_t b0, nb;
        shard(B, nd, d, &b0, &nb);
        DeviceGuard dg(c->dev);
        hipStream_t st = c->stream;
        // one slot per device for the in-place gather (nd == 1: just this shard);
        // devices without candidates still take part in the gather
        if ((rc = ensure(c->out, sizeof(float) * (size_t)per * nd, st))) return rc;
        if ((rc = ensure_pinned(c->h_out, sizeof(float) * (size_t)(gather ? B : nb)))) return rc;
        if (nb == 0) continue;
        if ((rc = ensure(c->target, tbytes, st)) ||
            (rc = upload_if_changed(c->target, &c->target_key, &c->target_bytes, target_hw3, tkey, tbytes, st)))
            return rc;
        if (mask_hw && ((rc = ensure(c->mask, mbytes, st)) ||
                        (rc = upload_if_changed(c->mask, &c->mask_key, &c->mask_bytes, mask_hw, mkey, mbytes, st))))
            return rc;
        const size_t gbytes = sizeof(float) * row * (size_t)nb;
        if ((rc = ensure(c->gen, std::max<size_t>(gbytes, 4), st))) return rc;
        GGS_HIP(hipStreamSynchronize(st));  // the previous call's work is done with c->gen
        drain.add(c->dev, st);
        if (gbytes)                         // straight from the caller's array (see above)
            GGS_HIP(hipMemcpyAsync(c->gen.p, genomes_axes + row * b0, gbytes, hipMemcpyHostToDevice, st));
        if ((rc = run_fitness(c, st, (const float*)c->gen.p, nb, N, C, (const float*)c->target.p,
                              mask_hw ? (const float*)c->mask.p : nullptr, mode, boost_beta, H, W,
                              k_sigma, (float*)c->out.p + (gather ? b0 : 0),
                              host_plan_key(tkey, mkey, boost_beta, mode, H, W))))
            return rc;
        if (!gather)
            GGS_HIP(hipMemcpyAsync(c->h_out.p, c->out.p, sizeof(float) * nb, hipMemcpyDeviceToHost, st));
        if (inject_fail_after(d + 1)) return fail(GGS_EHIP, "injected failure after device %d's work (test hook)", d + 1);
    }
    if (gather) {
        // north_star: one RCCL gather of the shards' fitness scalars (in place, every
        // device's out[] becomes the whole vector), then ONE D2H from the first device
        std::lock_guard<std::mutex> cl(g_comm_mu);
        std::vector<void*> comms;
        if ((rc = local_comms_locked(cs, &comms))) return rc;
        std::vector<hipStream_t> sts;
        std::vector<float*> bufs;
        for (DevCtx* c : cs) {
            sts.push_back(c->stream);
            bufs.push_back((float*)c->out.p);
        }
        for (DevCtx* c : cs) drain.add(c->dev, c->stream);    // devices without candidates gather too
        if ((rc = comm_group_allgather_inplace(comms.data(), nd, sts.data(), bufs.data(), per))) return rc;
        DeviceGuard dg(cs[0]->dev);
        GGS_HIP(hipMemcpyAsync(cs[0]->h_out.p, cs[0]->out.p, sizeof(float) * B, hipMemcpyDeviceToHost,
                               cs[0]->stream));
        if ((rc = drain.drain())) return rc;    // every device's gather done (the first: and its D2H)
        memcpy(out_B, cs[0]->h_out.p, sizeof(float) * B);
        return GGS_OK;
    }
    if ((rc = drain.drain())) return rc;
    memcpy(out_B, cs[0]->h_out.p, sizeof(float) * B);
    return GGS_OK;
}

int ggs_fitness_grad(const float* genomes_axes, int64_t B, int32_t N, int32_t C, const float* target_hw3,
                     const float* mask_hw, int32_t mode, float boost_beta, int32_t H, int32_t W, float k_sigma,
                     float* out_B, float* grad_BN9) {
    int rc = check_grad_dims(B, N, C, H, W, mode, mask_hw);
    if (rc) return rc;
    if (!genomes_axes || !target_hw3 || !out_B || !grad_BN9) return fail(GGS_EINVAL, "null pointer");
    std::vector<DevCtx*> cs;
    if ((rc = active_ctxs(1, &cs))) return rc;
    DevCtx* c = cs[0];
    const size_t tbytes = sizeof(float) * 3 * (size_t)H * W, mbytes = sizeof(float) * (size_t)H * W;
    const size_t gbytes = sizeof(float) * (size_t)N * C * (size_t)B, dbytes = sizeof(float) * 9 * (size_t)N * (size_t)B;
    const uint64_t tkey = hash_bytes(target_hw3, tbytes);
    const uint64_t mkey = mask_hw ? hash_bytes(mask_hw, mbytes) : 0;
    HostCall hc(c);
    const hipStream_t st = hc.st;
    if ((rc = ensure(c->out, sizeof(float) * (size_t)B, st)) || (rc = ensure(c->ggrad, dbytes, st)) ||
        (rc = ensure(c->target, tbytes, st)) || (mask_hw && (rc = ensure(c->mask, mbytes, st))) ||
        (rc = ensure(c->gen, gbytes, st)) || (rc = hc.begin()))
        return rc;
    if ((rc = upload_if_changed(c->target, &c->target_key, &c->target_bytes, target_hw3, tkey, tbytes, st)) ||
        (mask_hw && (rc = upload_if_changed(c->mask, &c->mask_key, &c->mask_bytes, mask_hw, mkey, mbytes, st))))
        return rc;
    GGS_HIP(hipMemcpyAsync(c->gen.p, genomes_axes, gbytes, hipMemcpyHostToDevice, st));
    if ((rc = run_fitness_grad(c, st, (const float*)c->gen.p, B, N, C, (const float*)c->target.p,
                               mask_hw ? (const float*)c->mask.p : nullptr, mode, boost_beta, H, W, k_sigma,
                               (float*)c->out.p, (float*)c->ggrad.p, host_plan_key(tkey, mkey, boost_beta, mode, H, W))))
        return rc;
    GGS_HIP(hipMemcpyAsync(out_B, c->out.p, sizeof(float) * (size_t)B, hipMemcpyDeviceToHost, st));
    GGS_HIP(hipMemcpyAsync(grad_BN9, c->ggrad.p, dbytes, hipMemcpyDeviceToHost, st));
    if (inject_fail_after(1)) return fail(GGS_EHIP, "injected failure after device 1's work (test hook)");
    return hc.drain.drain();
}

int ggs_render_vjp(const float* genomes, int64_t B, int32_t N, int32_t C, int32_t layout, int32_t H, int32_t W,
                   float k_sigma, const float* bg, const float* cot_bhw3, float* grad_BN9, int32_t device) {
    int rc = check_vjp_dims(B, N, C, layout, H, W);
    if (rc) return rc;
    if (!genomes || !cot_bhw3 || !grad_BN9) return fail(GGS_EINVAL, "null genomes/cotangent/grad");
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    const float bg1[3] = {1.f, 1.f, 1.f};
    const size_t vbytes = sizeof(float) * 3 * (size_t)H * W * (size_t)B;
    const size_t gbytes = sizeof(float) * (size_t)N * C * (size_t)B, dbytes = sizeof(float) * 9 * (size_t)N * (size_t)B;
    HostCall hc(c);
    const hipStream_t st = hc.st;
    // the cotangent is staged in c->out, the render host call's image buffer
    if ((rc = ensure(c->out, vbytes, st)) || (rc = ensure(c->ggrad, dbytes, st)) || (rc = ensure(c->gen, gbytes, st)) ||
        (rc = hc.begin()))
        return rc;
    GGS_HIP(hipMemcpyAsync(c->gen.p, genomes, gbytes, hipMemcpyHostToDevice, st));
    GGS_HIP(hipMemcpyAsync(c->out.p, cot_bhw3, vbytes, hipMemcpyHostToDevice, st));
    if ((rc = run_render_vjp(c, st, (const float*)c->gen.p, B, N, C, layout, H, W, k_sigma, bg ? bg : bg1,
                             (const float*)c->out.p, (float*)c->ggrad.p)))
        return rc;
    GGS_HIP(hipMemcpyAsync(grad_BN9, c->ggrad.p, dbytes, hipMemcpyDeviceToHost, st));
    return hc.drain.drain();
}

int ggs_image_loss(const float* img_bhw3, int64_t B, const float* targets_khw3, int32_t K, int32_t group, int32_t H,
                   int32_t W, const ggs_loss_params* p, float* loss_B, float* cot_bhw3, int32_t device) {
    int rc = check_loss_dims(B, K, group, H, W);
    if (rc) return rc;
    if ((rc = check_loss_params(p))) return rc;
    if (!img_bhw3 || !targets_khw3 || !loss_B) return fail(GGS_EINVAL, "null image/targets/loss");
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    const size_t plane = sizeof(float) * 3 * (size_t)H * W;
    const size_t vbytes = plane * (size_t)B, tbytes = plane * (size_t)K;
    HostCall hc(c);
    const hipStream_t st = hc.st;
    if ((rc = ensure(c->loss_img, vbytes, st)) || (cot_bhw3 && (rc = ensure(c->loss_cot, vbytes, st))) ||
        (rc = ensure(c->loss_out, sizeof(float) * (size_t)B, st)) || (rc = ensure(c->target, tbytes, st)) ||
        (rc = hc.begin()))
        return rc;
    // the staging no longer holds what the single-target calls' content keys describe
    c->target_key = 0;
    c->target_bytes = 0;
    GGS_HIP(hipMemcpyAsync(c->loss_img.p, img_bhw3, vbytes, hipMemcpyHostToDevice, st));
    GGS_HIP(hipMemcpyAsync(c->target.p, targets_khw3, tbytes, hipMemcpyHostToDevice, st));
    float* d_cot = cot_bhw3 ? (float*)c->loss_cot.p : nullptr;
    if ((rc = run_image_loss(c, st, (const float*)c->loss_img.p, B, (const float*)c->target.p, group, H, W, *p,
                             (float*)c->loss_out.p, d_cot)))
        return rc;
    GGS_HIP(hipMemcpyAsync(loss_B, c->loss_out.p, sizeof(float) * (size_t)B, hipMemcpyDeviceToHost, st));
    if (cot_bhw3) GGS_HIP(hipMemcpyAsync(cot_bhw3, d_cot, vbytes, hipMemcpyDeviceToHost, st));
    return hc.drain.drain();
}

int ggs_loss_grad(const float* genomes, int64_t B, int32_t N, int32_t C, int32_t layout, const float* targets_khw3,
                  int32_t K, int32_t group, int32_t H, int32_t W, float k_sigma, const float* bg,
                  const ggs_loss_params* p, float* loss_B, float* grad_BN9, int32_t device) {
    int rc = check_loss_grad(B, N, C, layout, K, group, H, W, p);
    if (rc) return rc;
    if (!genomes || !targets_khw3 || !loss_B || !grad_BN9) return fail(GGS_EINVAL, "null genomes/targets/loss/grad");
    DevCtx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    const float bg1[3] = {1.f, 1.f, 1.f};
    const size_t plane = sizeof(float) * 3 * (size_t)H * W;
    const size_t vbytes = plane * (size_t)B, tbytes = plane * (size_t)K;
    const size_t gbytes = sizeof(float) * (size_t)N * C * (size_t)B, dbytes = sizeof(float) * 9 * (size_t)N * (size_t)B;
    HostCall hc(c);
    const hipStream_t st = hc.st;
    if ((rc = ensure(c->loss_img, vbytes, st)) || (rc = ensure(c->loss_cot, vbytes, st)) ||
        (rc = ensure(c->loss_out, sizeof(float) * (size_t)B, st)) || (rc = ensure(c->target, tbytes, st)) ||
        (rc = ensure(c->gen, gbytes, st)) || (rc = ensure(c->ggrad, dbytes, st)) ||
        (rc = hc.begin()))
        return rc;
    c->target_key = 0;
    c->target_bytes = 0;
    GGS_HIP(hipMemcpyAsync(c->gen.p, genomes, gbytes, hipMemcpyHostToDevice, st));
    GGS_HIP(hipMemcpyAsync(c->target.p, targets_khw3, tbytes, hipMemcpyHostToDevice, st));
    if ((rc = run_loss_grad(c, st, (const float*)c->gen.p, B, N, C, layout, (const float*)c->target.p, group, H, W,
                            k_sigma, bg ? bg : bg1, *p, (float*)c->loss_out.p, (float*)c->ggrad.p,
                            (float*)c->loss_img.p, (float*)c->loss_cot.p)))
        return rc;
    GGS_HIP(hipMemcpyAsync(loss_B, c->loss_out.p, sizeof(float) * (size_t)B, hipMemcpyDeviceToHost, st));
    GGS_HIP(hipMemcpyAsync(grad_BN9, c->ggrad.p, dbytes, hipMemcpyDeviceToHost, st));
    return hc.drain.drain();
}

int ggs_fitness_grad_targets(const float* genomes_axes, int64_t B, int32_t N, int32_t C, const float* targets_khw3,
                             const float* masks_khw, int32_t K, int32_t group, int32_t mode, float boost_beta,
                             int32_t H, int32_t W, float k_sigma, float* out_B, float* grad_BN9) {
    int rc = check_grad_set(B, N, C, H, W, mode, masks_khw, K, group);
    if (rc) return rc;
    if (!genomes_axes || !targets_khw3 || !out_B || !grad_BN9) return fail(GGS_EINVAL, "null pointer");
    if ((rc = check_dims(K, 1, 9, H, W))) return rc;      // the set's strips are numbered through in 32 bits
    std::vector<DevCtx*> cs;
    if ((rc = active_ctxs(1, &cs))) return rc;
    DevCtx* c = cs[0];
    const size_t tbytes = sizeof(float) * 3 * (size_t)H * W * (size_t)K, mbytes = sizeof(float) * (size_t)H * W * (size_t)K;
    const size_t gbytes = sizeof(float) * (size_t)N * C * (size_t)B, dbytes = sizeof(float) * 9 * (size_t)N * (size_t)B;
    HostCall hc(c);
    const hipStream_t st = hc.st;
    if ((rc = ensure(c->out, sizeof(float) * (size_t)B, st)) || (rc = ensure(c->ggrad, dbytes, st)) ||
        (rc = ensure(c->target, tbytes, st)) || (masks_khw && (rc = ensure(c->mask, mbytes, st))) ||
        (rc = ensure(c->gen, gbytes, st)) || (rc = ensure(c->set_plan, (size_t)K * plan_bytes(H, W), st)) ||
        (rc = ensure(c->set_wpart, (size_t)K * plan_wsum_bytes(H, W), st)) || (rc = hc.begin()))
        return rc;
    // the staging no longer holds what the single-target calls' content keys describe
    c->target_key = c->mask_key = 0;
    c->target_bytes = c->mask_bytes = 0;
    GGS_HIP(hipMemcpyAsync(c->target.p, targets_khw3, tbytes, hipMemcpyHostToDevice, st));
    if (masks_khw) GGS_HIP(hipMemcpyAsync(c->mask.p, masks_khw, mbytes, hipMemcpyHostToDevice, st));
    GGS_HIP(hipMemcpyAsync(c->gen.p, genomes_axes, gbytes, hipMemcpyHostToDevice, st));
    const float* d_masks = masks_khw ? (const float*)c->mask.p : nullptr;
    GGS_HIP(launch_plan_set(st, (const float*)c->target.p, d_masks, mode, boost_beta, H, W, K,
                            (float4*)c->set_plan.p, (float*)c->set_wpart.p));
    if ((rc = run_fitness_grad_planned(c, st, (const float*)c->gen.p, B, N, C, (const float4*)c->set_plan.p,
                                       (const float*)c->set_wpart.p, (const float*)c->target.p, d_masks, mode,
                                       boost_beta, H, W, group, k_sigma, (float*)c->out.p, (float*)c->ggrad.p)))
        return rc;
    GGS_HIP(hipMemcpyAsync(out_B, c->out.p, sizeof(float) * (size_t)B, hipMemcpyDeviceToHost, st));
    GGS_HIP(hipMemcpyAsync(grad_BN9, c->ggrad.p, dbytes, hipMemcpyDeviceToHost, st));
    return hc.drain.drain();
}

int ggs_render(const float* genomes, int64_t B, int32_t N, int32_t C, int32_t H, int32_t W,
               float k_sigma, const float* bg, float* out_bhw3, int32_t n_devices) {
    int rc = check_dims(B, N, C, H, W);
    if (rc) return rc;
    if (B == 0) return GGS_OK;
    if ((!genomes && N > 0) || !out_bhw3) return fail(GGS_EINVAL, "null pointer");
    std::vector<DevCtx*> cs;
    if ((rc = active_ctxs(n_devices, &cs))) return rc;
    const float bg1[3] = {1.f, 1.f, 1.f};
    const float* bgp = bg ? bg : bg1;
    const int nd = (int)cs.size();
    const size_t row = (size_t)N * C;
    const size_t img1 = sizeof(float) * 3 * (size_t)H * W;
    std::vector<std::unique_lock<std::mutex>> locks;
    for (int d = 0; d < nd; ++d) locks.emplace_back(cs[d]->mu);
    StreamDrain drain;                  // every stream given work is synchronised on any return
    // uploads and renders on every device first, then the image copies: a D2H into
    // pageable memory may run synchronously, and queued before the next device's
    // upload it would serialise the fan-out
    for (int d = 0; d < nd; ++d) {
        DevCtx* c = cs[d];
        int64_t b0, nb;
        shard(B, nd, d, &b0, &nb);
        if (nb == 0) continue;
        DeviceGuard dg(c->dev);
        hipStream_t st = c->stream;
        const size_t gbytes = sizeof(float) * row * (size_t)nb;
        if ((rc = ensure(c->gen, std::max<size_t>(gbytes, 4), st))) return rc;
        if ((rc = ensure(c->out, img1 * nb, st))) return rc;
        GGS_HIP(hipStreamSynchronize(st));
        drain.add(c->dev, st);
        // straight from / to the caller's (pageable) arrays, as the fitness host API
        if (gbytes)
            GGS_HIP(hipMemcpyAsync(c->gen.p, genomes + row * b0, gbytes, hipMemcpyHostToDevice, st));
        if ((rc = run_render(c, st, (const float*)c->gen.p, nb, N, C, H, W, k_sigma, bgp, (float*)c->out.p)))
            return rc;
        if (inject_fail_after(d + 1)) return fail(GGS_EHIP, "injected failure after device %d's work (test hook)", d + 1);
    }
    for (int d = 0; d < nd; ++d) {
        DevCtx* c = cs[d];
        int64_t b0, nb;
        shard(B, nd, d, &b0, &nb);
        if (nb == 0) continue;
        DeviceGuard dg(c->dev);
        GGS_HIP(hipMemcpyAsync((char*)out_bhw3 + img1 * b0, c->out.p, img1 * nb, hipMemcpyDeviceToHost, c->stream));
    }
    return drain.drain();
}

static int stage_call(bool encode, const float* in, int64_t S, int32_t C, int32_t H, int32_t W, float k,
                      float* f9, int32_t* i4, float* enc9) {
    if (S < 0 || C < 9) return fail(GGS_EINVAL, "S=%lld must be >= 0 and C=%d >= 9", (long long)S, C);
    if (S == 0) return GGS_OK;
    if (!in) return fail(GGS_EINVAL, "null input");
    int rc;
    std::vector<DevCtx*> cs;
    if ((rc = active_ctxs(1, &cs))) return rc;
    DevCtx* c = cs[0];
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    hipStream_t st = c->stream;
    DevBuf din, dout;      // exact-size scratch of this call, freed on return
    const size_t ib = sizeof(float) * (size_t)S * C, ob = (f9 ? 13 : 9) * sizeof(float) * (size_t)S;
    GGS_HIP(hipMalloc(&din.p, ib));
    GGS_HIP(hipMalloc(&dout.p, ob));
    GGS_HIP(hipMemcpyAsync(din.p, in, ib, hipMemcpyHostToDevice, st));
    float* o = (float*)dout.p;
    GGS_HIP(launch_prep(st, encode, (const float*)din.p, S, C, H, W, k, nullptr, nullptr, f9 ? o : nullptr,
                        f9 ? (int*)(o + 9 * S) : nullptr, enc9 ? o : nullptr));
    GGS_HIP(hipStreamSynchronize(st));
    if (f9) {
        GGS_HIP(hipMemcpy(f9, o, 9 * sizeof(float) * S, hipMemcpyDeviceToHost));
        GGS_HIP(hipMemcpy(i4, o + 9 * S, 4 * sizeof(int) * S, hipMemcpyDeviceToHost));
    } else {
        GGS_HIP(hipMemcpy(enc9, o, 9 * sizeof(float) * S, hipMemcpyDeviceToHost));
    }
    return GGS_OK;
}

int ggs_encode(const float* genomes_axes, int64_t S, int32_t C, float* out_S9) {
    if (!out_S9 && S > 0) return fail(GGS_EINVAL, "null output");
    return stage_call(true, genomes_axes, S, C, 1, 1, 3.f, nullptr, nullptr, out_S9);
}

int ggs_preprocess(const float* genomes, int64_t S, int32_t C, int32_t H, int32_t W, float k_sigma,
                   float* out_f9, int32_t* out_i4) {
    if ((!out_f9 || !out_i4) && S > 0) return fail(GGS_EINVAL, "null output");
    if (H < 1 || W < 1) return fail(GGS_EINVAL, "H=%d, W=%d must be >= 1", H, W);
    return stage_call(false, genomes, S, C, H, W, k_sigma, out_f9, out_i4, nullptr);
}

int ggs_detmath_eval(int32_t fn, const float* x, const float* y, int64_t n, float* out) {
    if (fn < 0 || fn > 5) return fail(GGS_EINVAL, "bad detmath function %d", fn);
    if (n < 0 || (n > 0 && (!x || !out || (fn == 5 && !y)))) return fail(GGS_EINVAL, "bad arguments");
    if (n == 0) return GGS_OK;
    int rc;
    std::vector<DevCtx*> cs;
    if ((rc = active_ctxs(1, &cs))) return rc;
    DevCtx* c = cs[0];
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    DevBuf dx, dy, dout;      // exact-size scratch of this call, freed on return
    const size_t nb = sizeof(float) * (size_t)n;
    GGS_HIP(hipMalloc(&dx.p, nb));
    GGS_HIP(hipMalloc(&dout.p, nb));
    GGS_HIP(hipMemcpy(dx.p, x, nb, hipMemcpyHostToDevice));
    if (fn == 5) {
        GGS_HIP(hipMalloc(&dy.p, nb));
        GGS_HIP(hipMemcpy(dy.p, y, nb, hipMemcpyHostToDevice));
    }
    GGS_HIP(launch_detmath(c->stream, (const float*)dx.p, (const float*)dy.p, n, fn, (float*)dout.p));
    GGS_HIP(hipStreamSynchronize(c->stream));
    GGS_HIP(hipMemcpy(out, dout.p, nb, hipMemcpyDeviceToHost));
    return GGS_OK;
}

int ggs_profile_enable(int32_t on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_on = on != 0;
    return GGS_OK;
}

int ggs_profile_read(const char* kernel, double* total_ms, int64_t* launches) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    prof_drain_locked();
    for (int k = 0; k < kProfKernels; ++k) {
        if (kernel && strcmp(kernel, kKernelNames[k]) == 0) {
            if (total_ms) *total_ms = g_prof_ms[k];
            if (launches) *launches = g_prof_n[k];
            return GGS_OK;
        }
    }
    return fail(GGS_EINVAL, "unknown kernel name '%s' (prep|raster|finalize|select|density|seed)", kernel ? kernel : "(null)");
}

void ggs_profile_reset(void) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    prof_drain_locked();
    for (int k = 0; k < kProfKernels; ++k) {
        g_prof_ms[k] = 0;
        g_prof_n[k] = 0;
    }
}

int ggs_workspace_count(int32_t device) {
    DevCtx* c = nullptr;
    const int rc = get_ctx(device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    return (int)c->ws.size();
}

}  // extern "C"

// ---- what the session units share (ggs_host.h) --------------------------------------
namespace ggs {

void release_workspace(DevCtx* c, hipStream_t st) {
    for (auto it = c->ws.begin(); it != c->ws.end(); ++it)
        if ((*it)->stream == st) {
            c->ws.erase(it);
            return;
        }
}

uint64_t new_plan_key() {
    static std::atomic<uint64_t> g_session_ids{0};
    return (1ull << 63) | ++g_session_ids;
}

int Session::open(const float* target_host, const float* mask_host, int n_images, int n_plans, bool raster) {
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
        st = nullptr;
        return fail(GGS_EHIP, "stream creation failed");
    }
    const int H = cfg.H, W = cfg.W;
    const size_t hw = (size_t)n_images * H * W;
    int rc;
    if ((rc = ensure(target, sizeof(float) * 3 * hw, st)) ||
        (mask_host && (rc = ensure(mask, sizeof(float) * hw, st))) ||
        (n_plans && ((rc = ensure(plan, (size_t)n_plans * plan_bytes(H, W), st)) ||
                     (rc = ensure(wpart, (size_t)n_plans * plan_wsum_bytes(H, W), st)))) ||
        (raster && (rc = ensure(order, sizeof(int) * (size_t)raster_order_len(H, W), st))))
        return rc;
    if (hipMemcpyAsync(target.p, target_host, sizeof(float) * 3 * hw, hipMemcpyHostToDevice, st) ||
        (mask_host && hipMemcpyAsync(mask.p, mask_host, sizeof(float) * hw, hipMemcpyHostToDevice, st)))
        return fail(GGS_EHIP, "upload failed");
    if (raster) {
        order_host.resize(raster_order_len(H, W));
        raster_tile_order(H, W, order_host.data());
        if (hipMemcpyAsync(order.p, order_host.data(), sizeof(int) * order_host.size(), hipMemcpyHostToDevice, st))
            return fail(GGS_EHIP, "upload failed");
    }
    if (n_plans && launch_plan_set(st, (const float*)target.p, d_mask(), cfg.fitness_mode, cfg.boost_beta, H, W,
                                   n_plans, (float4*)plan.p, (float*)wpart.p) != hipSuccess)
        return fail(GGS_EHIP, "plan launch failed");
    return GGS_OK;
}

int reserve_grad_workspace(DevCtx* c, hipStream_t st, int64_t B, int N, int H, int W) {
    Workspace* w = workspace_for(c, st);
    int nTX;
    const int nTiles = raster_tiles(H, W, &nTX);
    const size_t per = grad_partial_bytes(N, H, W), S = (size_t)B * N;
    const int64_t chunk = std::min<int64_t>(B, (int64_t)(kGradChunkBytes / per));
    int rc;
    StripWords sw;
    if ((rc = ensure(w->recs, sizeof(SplatRec) * S, st)) || (rc = ensure(w->bnds, sizeof(int4) * S, st)) ||
        (rc = ensure(w->partials, sizeof(float) * 4 * (size_t)(B * nTiles), st)) ||
        (rc = ensure_tile_order(w, H, W, st)) || (rc = ensure_strip_words(w, B, N, H, W, st, &sw)) ||
        (rc = ensure(w->gf9, sizeof(float) * 9 * S, st)) || (rc = ensure(w->gi4, sizeof(int) * 4 * S, st)) ||
        (rc = ensure(w->gpart, per * (size_t)chunk, st)))
        return rc;
    return GGS_OK;
}

}  // namespace ggs
