// Host-only declarations shared by the units of libggs.so's host layer: ggs_capi.cpp
// (contexts, host and device API) and the session units ggs_sess_{ga,sa,de,refine}.cpp.
// Error reporting, owning buffers, pooled workspaces, device contexts, guards, the
// device pipelines (run_*), their argument checks (check_*) and the session base.
// The kernels include ggs_internal.h, never this file.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "ggs_internal.h"

namespace ggs {

extern thread_local std::string t_err;   // ggs_last_error()'s message
int fail(int code, const char* fmt, ...);

#define GGS_HIP(call)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return ::ggs::fail(e_ == hipErrorOutOfMemory ? GGS_ENOMEM : GGS_EHIP, "%s: %s (%s:%d)", \
                               #call, hipGetErrorString(e_), __FILE__, __LINE__);                \
    } while (0)

// ---- buffers ------------------------------------------------------------------
// A device (DevBuf) or pinned host (PinBuf) allocation that frees itself: move-only,
// so a struct of them needs no list of its members to be released.  The owner sees
// to it that the destructor runs with the buffer's device current, its context
// locked and the stream that used it synchronised, and never after main() returns.
template <hipError_t (*Free)(void*)>
struct OwnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    OwnedBuf& operator=(OwnedBuf&& o) noexcept {
        std::swap(p, o.p);          // o, a temporary or a buffer being replaced, frees the old block
        std::swap(cap, o.cap);
        return *this;
    }
    ~OwnedBuf() {
        if (p) (void)Free(p);
    }
};
inline hipError_t free_device(void* p) { return hipFree(p); }
inline hipError_t free_pinned(void* p) { return hipHostFree(p); }
using DevBuf = OwnedBuf<free_device>;
using PinBuf = OwnedBuf<free_pinned>;

// Grow `b` to at least `bytes`.  `st` is the stream that may still be using the
// old allocation; it is synchronised before the free.
int ensure(DevBuf& b, size_t bytes, hipStream_t st);
// ensure() for a counter block: a grown buffer is zeroed on `st` (the fused
// finalize's per-candidate counters start at zero and every launch leaves them
// at zero).
int ensure_zeroed(DevBuf& b, size_t bytes, hipStream_t st);
int ensure_pinned(PinBuf& b, size_t bytes);

// Per-(device, stream) scratch used by one render/fitness pipeline.
struct Workspace {
    hipStream_t stream = nullptr;
    DevBuf recs, bnds, partials, wpartials, order, plan, fctr;   // fctr: fused-finalize counters
    DevBuf maskws;                    // target preparation / importance mask scratch (ggs_mask.hip)
    DevBuf swords, smasks;            // strip words and masks, prep -> raster (StripWords)
    DevBuf gf9, gi4, gpart, gout;     // fitness gradient: prep's stage outputs, strip partials, unwanted fitness
    DevBuf lpart, limg, lcot;         // image loss: tile partials; ggs_loss_grad's image and cotangent
    DevBuf seedws;                    // residual-driven placement: launch_seed_sites's scratch
    int order_H = -1, order_W = -1;   // (H, W) the tile order was built for
    bool strips_ok = false;           // ... and whether its strip table holds that canvas
    uint64_t plan_key = 0;            // inputs the plan was built from (0: none / volatile)
};

// What a context owns on its device; ggs_shutdown releases it by assigning an empty one.
struct CtxBuffers {
    std::vector<std::unique_ptr<Workspace>> ws;
    // host-API staging
    DevBuf gen, out, target, mask, ggrad;   // ggrad: ggs_fitness_grad's [B,N,9]
    DevBuf set_plan, set_wpart;            // ggs_fitness_grad_targets' own plan set
    DevBuf prep_in, prep_tgt, prep_mask;   // ggs_targets_prepare / ggs_quantiles staging
    DevBuf loss_img, loss_cot, loss_out;   // ggs_image_loss / ggs_loss_grad staging
    PinBuf h_out;                  // the fitness scalars (render and genomes go straight to / from the caller)
    uint64_t target_key = 0, mask_key = 0;
    size_t target_bytes = 0, mask_bytes = 0;
};

struct DevCtx : CtxBuffers {
    int dev = 0;
    int simds = 0;                 // CUs x 4 of dev (single-round raster ordering)
    hipStream_t stream = nullptr;  // library-owned stream for the host API
    std::mutex mu;
};

// Context of `device`, created on first use.
int get_ctx(int device, DevCtx** out);
Workspace* workspace_for(DevCtx* c, hipStream_t st);
// A session's stream is about to be destroyed: the context's pipeline workspace of
// that stream goes with it (a later stream may get the same handle).
void release_workspace(DevCtx* c, hipStream_t st);
// The pipeline buffers a gradient call over B candidates takes from the stream's
// workspace, made now so that no later call allocates.
int reserve_grad_workspace(DevCtx* c, hipStream_t st, int64_t B, int N, int H, int W);

// ---- guards ---------------------------------------------------------------------
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// Event pair around one kernel while ggs_profile_enable is on (kernel: 0 prep,
// 1 raster, 2 finalize, 3 select, 4 one density-control event of a refine session,
// 5 one residual-driven placement).
struct ProfScope {
    bool on = false;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st;
    int kernel;
    ProfScope(hipStream_t s, int k);
    ~ProfScope();
};

// ---- the device pipelines (ctx locked, device set) --------------------------------
uint64_t hash_bytes(const void* data, size_t n);
inline uint64_t rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

int check_dims(int64_t B, int32_t N, int32_t C, int32_t H, int32_t W);
int check_grad_dims(int64_t B, int32_t N, int32_t C, int32_t H, int32_t W, int32_t mode, const void* mask);
int check_grad_set(int64_t B, int32_t N, int32_t C, int32_t H, int32_t W, int32_t mode, const void* masks, int32_t K,
                   int32_t group);
int check_loss_grad(int64_t B, int32_t N, int32_t C, int32_t layout, int32_t K, int32_t group, int32_t H, int32_t W,
                    const ggs_loss_params* p);

// raster (MODE 1) + finalize of B candidates: one launch when `fuse` (and allowed).
// group > 0: plan / wpartials are a plan set's and candidate b is scored against
// plan b / group.
int raster_fitness(hipStream_t st, int simds, const SplatRec* recs, const int4* bnds, int B, int N, int H, int W,
                   const float4* plan, float* partials, const float* wpartials, int mode, const int* order,
                   DevBuf& ctr, float* out, bool fuse, const unsigned char* dirty = nullptr,
                   const float* clean = nullptr, int group = 0, const StripWords& sw = StripWords{});
// plan_key: identifies (target contents, mask contents, mode, beta, H, W) when
// the caller knows them to be unchanged since a previous call with the same key
// (host API: content hashes; sessions: immutable inputs, new_plan_key); 0 = rebuild.
int run_fitness(DevCtx* c, hipStream_t st, const float* d_gen, int64_t B, int N, int C,
                const float* d_target, const float* d_mask, int mode, float beta, int H, int W,
                float k, float* d_out, uint64_t plan_key = 0);
// prep -> raster -> finalize against a ready target plan (group > 0: a plan set,
// candidate b against plan b / group).
int run_fitness_planned(DevCtx* c, hipStream_t st, const float* d_gen, int64_t B, int N, int C,
                        const float4* plan, const float* wpartials, int mode, int H, int W, float k,
                        float* d_out, int group = 0);
// encode: the rows are axes-angle rows, prep encodes them first (GGS_LAYOUT_AXES)
int run_render(DevCtx* c, hipStream_t st, const float* d_gen, int64_t B, int N, int C, int H, int W,
               float k, const float bg[3], float* d_img, bool encode = false);
// loss [B] and, unless d_cot is null, the cotangent [B][H][W][3]; the tile partials are
// the stream's workspace.
int run_image_loss(DevCtx* c, hipStream_t st, const float* d_img, int64_t B, const float* d_targets, int group, int H,
                   int W, const ggs_loss_params& p, float* d_loss, float* d_cot);
// render -> image loss -> VJP, the three stages as their own entry points issue them;
// d_img / d_cot [B][H][W][3] are the caller's scratch.
int run_loss_grad(DevCtx* c, hipStream_t st, const float* d_gen, int64_t B, int N, int C, int layout,
                  const float* d_targets, int group, int H, int W, float k, const float bg[3],
                  const ggs_loss_params& p, float* d_loss, float* d_grad, float* d_img, float* d_cot);
// Fitness (the existing prep -> raster -> finalize path, so ggs_fitness_device's
// bits) and its gradient [B][N][9].  d_out may be null.
int run_fitness_grad(DevCtx* c, hipStream_t st, const float* d_gen, int64_t B, int N, int C, const float* d_target,
                     const float* d_mask, int mode, float beta, int H, int W, float k, float* d_out, float* d_grad,
                     uint64_t plan_key = 0);
// The same against ready plans: group == 0 one plan (ggs_fitness_device_planned's
// bits), group > 0 a plan set (ggs_fitness_device_planset's).  d_targets / d_masks:
// the raw arrays the plans were made from.
int run_fitness_grad_planned(DevCtx* c, hipStream_t st, const float* d_gen, int64_t B, int N, int C,
                             const float4* plan, const float* wblocks, const float* d_targets, const float* d_masks,
                             int mode, float beta, int H, int W, int group, float k, float* d_out, float* d_grad);

// ---- sessions -------------------------------------------------------------------
// Target-plan cache keys of sessions (their target/mask never change): unique
// for the process lifetime, top bit set (host-API content keys have it clear).
uint64_t new_plan_key();

// What the six device-resident session types share: the context, their own stream,
// the config with the log bounds filled, the target(s) and the raster inputs made
// from them.  The buffers free themselves; the stream is closed by close_session.
struct Session {
    DevCtx* c;
    hipStream_t st = nullptr;
    ggs_ga_config cfg;
    const uint64_t plan_key = new_plan_key();
    DevBuf target, mask, plan, wpart, order, fctr;   // fctr: the fused finalize's counters
    std::vector<int> order_host;    // the tile order's upload reads it until the create synchronises

    Session(DevCtx* ctx, const ggs_ga_config& config) : c(ctx), cfg(config) {
        if (cfg.scale_log_lo == 0.0f && cfg.scale_log_hi == 0.0f) {   // utils.py:38-39 when the caller passed 0, 0
            cfg.scale_log_lo = logf(cfg.min_scale_splats);
            cfg.scale_log_hi = logf(cfg.max_scale_splats * (float)std::max(cfg.H, cfg.W));
        }
    }
    const float* d_mask() const { return (const float*)mask.p; }      // null without a mask

    // Creates the stream and queues on it: the upload of n_images targets (and masks,
    // unless null), the plan set of n_plans of them (0: none; the refiner's loss mode
    // has no plan and its single-target mode takes the workspace's) and, with
    // `raster`, the tile order of a session that launches the raster itself.
    // Context locked, device current; the caller synchronises before it returns.
    int open(const float* target_host, const float* mask_host, int n_images, int n_plans, bool raster);
};

// Synchronise, free the buffers, release the stream's workspace, destroy the stream
// (context locked, device current).
template <class T>
void close_session(T* s) {
    DevCtx* c = s->c;
    const hipStream_t st = s->st;
    if (st) (void)hipStreamSynchronize(st);     // copies from the caller's arrays included
    delete s;
    if (!st) return;
    release_workspace(c, st);
    (void)hipStreamDestroy(st);
}

// A create that fails after the session was made: the thread's error text is kept.
template <class T>
int fail_session(std::unique_ptr<T>& s, int code) {
    const std::string keep = t_err;
    close_session(s.release());
    t_err = keep;
    return code;
}

template <class T>
void destroy_session(void* handle) {
    if (!handle) return;
    DevCtx* c = ((T*)handle)->c;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->dev);
    close_session((T*)handle);
}

// ---- shared by the session units (ggs_sess_ga.cpp, ggs_sess_refine.cpp) -----------
GaParamsDev ga_params(const ggs_ga_config& c, int gen, int total);
// Shared validation of ggs_ga_create / ggs_sa_create.
int ga_check_config(const ggs_ga_config& c, const float* mask_hw, bool sa);
// Upload one generation's explicit draws into buf; returns device views.
int ga_upload_draws(DevBuf& buf, hipStream_t st, int64_t P, int64_t N, int64_t K, bool mutation_only,
                    const ggs_ga_draws* h, GaDrawsDev* d);
// Row n of a session's curves [cap][row_bytes] on the device, grown (doubling) when full.
int curves_row(DevBuf& curves, int64_t n, int64_t* cap_io, size_t row_bytes, hipStream_t st, double** row);
int refine_check_params(const ggs_refine_params* p);
// step t's constants (t from 1); cfg: the scale bounds, filled
RefineStepDev refine_step_dev(const ggs_refine_params& prm, const ggs_ga_config& cfg, int64_t t);

}  // namespace ggs
