// What the three device searches (ggs_ga.hip, ggs_sa.hip, ggs_de.hip) share: the
// counter-based Philox draws and the per-splat pieces of the variation.  Every
// function is __forceinline__, so each unit compiles its own copy into its kernels.
#pragma once
#include "ggs_internal.h"

namespace ggs {

// ---------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11), counter-based
// ---------------------------------------------------------------------------
struct U4 {
    uint32_t x, y, z, w;
};

__host__ __device__ __forceinline__ U4 philox(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
        c = {(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

__device__ __forceinline__ float u01(uint32_t v) { return (float)(v >> 8) * (1.0f / 16777216.0f); }

// stream ids: which draw a 4-word Philox block feeds
enum : uint32_t { S_MASK = 1, S_NORM_A = 2, S_NORM_B = 3, S_NORM_C = 4, S_IND = 5, S_TOUR = 6, S_CX = 7,
                  S_ACCEPT = 8 };

// SA acceptance uniform of try (it, k): 53 bits of one Philox block -> [0, 1)
// (the role of random.random() at annealing.py:140-142).  Host and device.
__host__ __device__ __forceinline__ double accept_u(uint64_t seed, uint32_t it, uint32_t k) {
    const U4 r = philox({it, k, 0u, S_ACCEPT}, (uint32_t)seed, (uint32_t)(seed >> 32));
    return ((double)(r.x >> 5) * 67108864.0 + (double)(r.y >> 6)) * (1.0 / 9007199254740992.0);
}
// Replica-exchange uniform of the pair (k, k + 1) after iteration `it`: accept_u's
// layout with what = 1, keyed by the group's exchange seed.
__host__ __device__ __forceinline__ double exchange_u(uint64_t seed, uint32_t it, uint32_t k) {
    const U4 r = philox({it, k, 1u, S_ACCEPT}, (uint32_t)seed, (uint32_t)(seed >> 32));
    return ((double)(r.x >> 5) * 67108864.0 + (double)(r.y >> 6)) * (1.0 / 9007199254740992.0);
}

struct Rng {
    uint32_t k0, k1, gen;
    __device__ U4 block(uint32_t stream, uint32_t who, uint32_t what) const {
        return philox({gen, who, what, stream}, k0, k1);
    }
};

// Box-Muller pair from two Philox words: r = sqrt(-2 ln u1) with u1 in (0, 1],
// angle 2*pi*u2.  The hardware transcendentals (v_log_f32 = log2, v_sqrt_f32,
// v_sin/v_cos_f32 in revolutions) are ample for mutation noise and keep the
// per-splat draw chain short; both outputs are used (5 pairs cover a splat's 9).
__device__ __forceinline__ float2 normal_pair(uint32_t a, uint32_t b) {
    const float u1 = ((float)(a >> 8) + 1.0f) * (1.0f / 16777216.0f);      // (0, 1]
    const float u2 = u01(b);                                               // [0, 1) revolutions
    const float r = __builtin_amdgcn_sqrtf(-1.38629436112f * __builtin_amdgcn_logf(u1));   // -2 ln 2 * log2
    return make_float2(r * __builtin_amdgcn_cosf(u2), r * __builtin_amdgcn_sinf(u2));
}

// ---------------------------------------------------------------------------
// float32 helpers with ggs/ga.py's exact semantics
// ---------------------------------------------------------------------------
constexpr float PI32 = 3.14159274101257324219f;     // float32(pi)
constexpr float TWO_PI32 = 6.28318548202514648438f; // float32(2*pi)

__device__ __forceinline__ float wrap_angle(float th) {      // np.remainder(th + pi, 2pi) - pi
    const float x = th + PI32;
    float r = fmodf(x, TWO_PI32);
    if (r != 0.0f && (r < 0.0f) != (TWO_PI32 < 0.0f)) r += TWO_PI32;
    return r - PI32;
}
__device__ __forceinline__ float clip(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// Per-splat pieces of the variation, shared by the GA variation kernel and the
// SA loop's split kernels (same code, so the same bits).
struct MaskU {                  // mask uniforms of one splat (genetic.py:37-54)
    float ux0, ux1, ua0, ua1, ut, urgb, ua;
};
__device__ __forceinline__ MaskU mask_draws(const GaDrawsDev& d, const Rng& rng, uint32_t og, int64_t ob, int s) {
    MaskU m;
    if (d.u_xy) {
        m.ux0 = d.u_xy[(ob + s) * 2]; m.ux1 = d.u_xy[(ob + s) * 2 + 1];
        m.ua0 = d.u_ab[(ob + s) * 2]; m.ua1 = d.u_ab[(ob + s) * 2 + 1];
        m.ut = d.u_t[ob + s]; m.urgb = d.u_rgb[ob + s]; m.ua = d.u_a[ob + s];
    } else {
        const U4 r1 = rng.block(S_MASK, og, (uint32_t)(2 * s));
        const U4 r2 = rng.block(S_MASK, og, (uint32_t)(2 * s + 1));
        m.ux0 = u01(r1.x); m.ux1 = u01(r1.y); m.ua0 = u01(r1.z); m.ua1 = u01(r1.w);
        m.ut = u01(r2.x); m.urgb = u01(r2.y); m.ua = u01(r2.z);
    }
    return m;
}
enum : int { ANY_COLOR = 1, ANY_XY = 2, ANY_AB = 4, ANY_T = 8 };
__device__ __forceinline__ int mask_any(const MaskU& m, float p) {
    return (((m.urgb < p) | (m.ua < p)) ? ANY_COLOR : 0) | (((m.ux0 < p) | (m.ux1 < p)) ? ANY_XY : 0) |
           (((m.ua0 < p) | (m.ua1 < p)) ? ANY_AB : 0) | ((m.ut < p) ? ANY_T : 0);
}
struct Fallback {               // genetic.py:24-29: one-true flat indices (-1: not needed)
    int kc, kx, kb, kt;
};
__device__ __forceinline__ Fallback fallbacks(const GaDrawsDev& d, const Rng& rng, uint32_t og, int o, int N,
                                              int any) {
    Fallback f{-1, -1, -1, -1};
    if (!(any & ANY_COLOR)) f.kc = d.k_color ? d.k_color[o] : (int)(rng.block(S_IND, og, 0).x % (uint32_t)(2 * N));
    if (!(any & ANY_XY)) f.kx = d.k_xy ? d.k_xy[o] : (int)(rng.block(S_IND, og, 1).x % (uint32_t)(2 * N));
    if (!(any & ANY_AB)) f.kb = d.k_ab ? d.k_ab[o] : (int)(rng.block(S_IND, og, 2).x % (uint32_t)(2 * N));
    if (!(any & ANY_T)) f.kt = d.k_t ? d.k_t[o] : (int)(rng.block(S_IND, og, 3).x % (uint32_t)N);
    return f;
}
struct NormD {                  // normals of one splat (genetic.py:57-70)
    float nx0, nx1, na0, na1, nt, nr0, nr1, nr2, nr3;
};
__device__ __forceinline__ NormD normal_draws(const GaDrawsDev& d, const Rng& rng, uint32_t og, int64_t ob, int s,
                                              int N) {
    NormD n;
    if (d.u_xy) {
        n.nx0 = d.n_xy[(ob + s) * 2]; n.nx1 = d.n_xy[(ob + s) * 2 + 1];
        n.na0 = d.n_ab[(ob + s) * 2]; n.na1 = d.n_ab[(ob + s) * 2 + 1];
        n.nt = d.n_t[ob + s];
        n.nr0 = d.n_rgba[(ob + s) * 4]; n.nr1 = d.n_rgba[(ob + s) * 4 + 1];
        n.nr2 = d.n_rgba[(ob + s) * 4 + 2]; n.nr3 = d.n_rgba[(ob + s) * 4 + 3];
    } else {
        const U4 g1 = rng.block(S_NORM_A, og, (uint32_t)s);
        const U4 g2 = rng.block(S_NORM_B, og, (uint32_t)s);
        const U4 g3 = rng.block(S_NORM_C, og, (uint32_t)s);
        const float2 p1 = normal_pair(g1.x, g1.y), p2 = normal_pair(g1.z, g1.w);
        const float2 p3 = normal_pair(g2.x, g2.y), p4 = normal_pair(g2.z, g2.w);
        const float2 p5 = normal_pair(g3.x, g3.y);
        n.nx0 = p1.x; n.nx1 = p1.y; n.na0 = p2.x; n.na1 = p2.y;
        n.nt = p3.x; n.nr0 = p3.y; n.nr1 = p4.x; n.nr2 = p4.y; n.nr3 = p5.x;
    }
    return n;
}
// genetic.py:37-70 + clamp_genome (utils.py:35-45) on one row, ggs/ga.py's float32 op order
__device__ __forceinline__ void mutate_row(float* g, const MaskU& u, const NormD& n, const Fallback& f, int s,
                                           const GaParamsDev& prm) {
    const float p = prm.mutpb;
    const bool mrgb = (u.urgb < p) || (f.kc == 2 * s), ma = (u.ua < p) || (f.kc == 2 * s + 1);
    const bool mx0 = (u.ux0 < p) || (f.kx == 2 * s), mx1 = (u.ux1 < p) || (f.kx == 2 * s + 1);
    const bool mb0 = (u.ua0 < p) || (f.kb == 2 * s), mb1 = (u.ua1 < p) || (f.kb == 2 * s + 1);
    const bool mt = (u.ut < p) || (f.kt == s);
    g[0] = g[0] + (n.nx0 * prm.sig_xy) * (float)mx0;
    g[1] = g[1] + (n.nx1 * prm.sig_xy) * (float)mx1;
    g[2] = g[2] + (n.na0 * prm.sig_alog) * (float)mb0;
    g[3] = g[3] + (n.na1 * prm.sig_blog) * (float)mb1;
    g[4] = g[4] + (n.nt * prm.sig_theta) * (float)mt;
    g[4] = wrap_angle(g[4]);
    g[5] = g[5] + (n.nr0 * prm.sig_rgb) * (float)mrgb;
    g[6] = g[6] + (n.nr1 * prm.sig_rgb) * (float)mrgb;
    g[7] = g[7] + (n.nr2 * prm.sig_rgb) * (float)mrgb;
    g[8] = g[8] + (n.nr3 * prm.sig_alpha) * (float)ma;
    g[0] = clip(g[0], 0.0f, 1.0f);
    g[1] = clip(g[1], 0.0f, 1.0f);
    g[2] = clip(g[2], prm.log_lo, prm.log_hi);
    g[3] = clip(g[3], prm.log_lo, prm.log_hi);
    g[4] = wrap_angle(g[4]);
#pragma unroll
    for (int c = 5; c < 9; ++c) g[c] = clip(g[c], 0.0f, 255.0f);
}

}  // namespace ggs
