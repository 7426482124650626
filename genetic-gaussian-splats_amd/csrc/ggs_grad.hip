// Fitness gradients: d fitness / d genome for the nine axes-angle
// genes of every splat, the Adam refiner's elementwise kernels and (§8d) the set
// kernel grad_set_strip_kernel with the island polish's polish_stage / _install.
//   grad_strip_kernel   one wave per (candidate, 16 x 32 pixel strip): the per-pixel
//                       backward of the "over" blend, reduced over the strip to nine
//                       sums per visited splat -> partials [b][strip][splat][12]
//   grad_finish_kernel  one thread per (candidate, splat): the strip partials summed
//                       in ascending strip order (float64), then the chain rule
//                       through preprocess (render.py:8-47) and encode
//                       (encode.py:4-59) -> grad [b][s][9]
//   refine_best_kernel / refine_adam_kernel   the refine session's step
//   vjp_strip_kernel / vjp_finish_kernel      (§8e) the same pair entered with a cotangent
//                       dL/d image instead of the fitness: the renderer's vector-
//                       Jacobian product, for renderer rows or axes-angle rows
//
// The forward values the clip decisions hang on (is x inside [0, 1], is exp(.)
// above 1e-6, ...) are prep's own float32 values: f9 / i4 are launch_prep's stage
// outputs and the finish kernel repeats encode_row's operations.  The integer
// AABB is a constant of the derivative.  Memory is indexed by candidate, strip
// and splat numbers only; the AABB integers are compared, never used as offsets.
#include <hip/hip_runtime.h>

#include "ggs_prep.h"

namespace ggs {
namespace {

constexpr int GS_W = 16;           // strip width: lane & 15 is the pixel column
constexpr int GS_H = 32;           // strip height: lane >> 4 is the row group, rows rg + 4 j
constexpr int GPL = GS_H / 4;      // pixels per lane
constexpr float K_EXP2 = -0.72134752044448170f;   // -0.5 * log2(e)
// 1 - f below this: the visit takes canvas_{i-1} from an exact ascending walk
// instead of (S - w gc) / (1 - f), whose rounding error grows as 1 / (1 - f)
constexpr float ONE_MINUS_F_MIN = 1.0f / 256.0f;

struct GSplat {
    float cx, cy, sxx, sxy2, syy, r, g, b, a;
    int x0, x1, y0, y1;
};

// k is wave-uniform: thirteen scalar loads
__device__ __forceinline__ GSplat load_splat(const float* __restrict__ f9, const int* __restrict__ i4, int64_t S,
                                             int64_t k) {
    GSplat s;
    s.cx = f9[0 * S + k];
    s.cy = f9[1 * S + k];
    s.sxx = f9[2 * S + k];
    s.sxy2 = 2.0f * f9[3 * S + k];
    s.syy = f9[4 * S + k];
    s.r = f9[5 * S + k];
    s.g = f9[6 * S + k];
    s.b = f9[7 * S + k];
    s.a = f9[8 * S + k];
    s.x0 = i4[0 * S + k];
    s.x1 = i4[1 * S + k];
    s.y0 = i4[2 * S + k];
    s.y1 = i4[3 * S + k];
    return s;
}

// Does the AABB touch strip (sx, sy)?  The strip kernel's cull and the finish
// kernel's walk both ask this, so the finish reads exactly the entries written.
__device__ __forceinline__ bool strip_hit(int x0, int x1, int y0, int y1, int sx, int sy) {
    const int px0 = sx * GS_W, py0 = sy * GS_H;
    return x1 >= px0 && x0 <= px0 + (GS_W - 1) && y1 >= py0 && y0 <= py0 + (GS_H - 1);
}

// the strip's splats among base + c * 64 .. + 63, bit l = splat c * 64 + l
__device__ __forceinline__ uint64_t cull_chunk(const int* __restrict__ i4, int64_t S, int64_t base, int N, int c,
                                               int lane, int sx, int sy) {
    const int i = c * 64 + lane;
    bool hit = false;
    if (i < N) {
        const int64_t k = base + i;
        hit = strip_hit(i4[0 * S + k], i4[1 * S + k], i4[2 * S + k], i4[3 * S + k], sx, sy);
    }
    return __builtin_amdgcn_ballot_w64(hit);
}

// The compiler hoists everything a visit computes from the pixel position alone
// (sixteen row numbers as floats, sixteen g . background) out of the splat loops
// and holds it in registers for the whole kernel; a value passed through here is
// recomputed per visit instead (a few conversions against ~40 operations a pixel).
__device__ __forceinline__ int opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ float opaque(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

// exp(-quad / 2) at the lane's pixel j, 0 outside the AABB (render.py:189-192)
__device__ __forceinline__ float gauss(const GSplat& s, bool in_x, float qx, float yf, int y, float* qy_out) {
    const float qy = yf - s.cy;
    *qy_out = qy;
    const float quad = (s.sxx * (qx * qx) + s.sxy2 * (qx * qy)) + s.syy * (qy * qy);
    const float e = __builtin_amdgcn_exp2f(K_EXP2 * quad);
    return (in_x && y >= s.y0 && y <= s.y1) ? e : 0.0f;
}

// The canvas of the strip's pixels after splats 0 .. limit-1, by the reference's
// own recurrence in ascending order (render.py:193-196); cr / cg / cb hold the
// background on entry.  Division-free.
__device__ __forceinline__ void canvas_upto(const float* __restrict__ f9, const int* __restrict__ i4, int64_t S,
                                            int64_t base, int N, int limit, int lane, int sx, int sy, int X,
                                            int Y0, float (&cr)[GPL], float (&cg)[GPL], float (&cb)[GPL]) {
    const float xf = (float)X;
    for (int c = 0; c * 64 < limit; ++c) {
        uint64_t m = cull_chunk(i4, S, base, N, c, lane, sx, sy);
        const int rest = limit - c * 64;
        if (rest < 64) m &= (1ull << rest) - 1ull;
        while (m) {
            const int bit = __builtin_ctzll(m);
            m &= m - 1ull;
            const GSplat s = load_splat(f9, i4, S, base + c * 64 + bit);
            const bool in_x = X >= s.x0 && X <= s.x1;
            const float qx = xf - s.cx;
            const int yb = opaque(Y0);
#pragma unroll
            for (int j = 0; j < GPL; ++j) {
                const int y = yb + 4 * j;
                float qy;
                const float f = gauss(s, in_x, qx, (float)y, y, &qy) * s.a;
                const float om = 1.0f - f;
                cr[j] = om * cr[j] + f * s.r;
                cg[j] = om * cg[j] + f * s.g;
                cb[j] = om * cb[j] + f * s.b;
            }
        }
    }
}

// g . canvas of the strip's pixels after splats 0 .. limit-1: the same ascending
// walk on u = g . canvas (g is fixed per pixel and the blend is linear in the
// canvas); u holds g . background on entry.  Division-free.
__device__ __forceinline__ void gdot_canvas_upto(const float* __restrict__ f9, const int* __restrict__ i4, int64_t S,
                                                 int64_t base, int N, int limit, int lane, int sx, int sy, int X,
                                                 int Y0, const float (&gr)[GPL], const float (&gg)[GPL],
                                                 const float (&gb)[GPL], float (&u)[GPL]) {
    const float xf = (float)X;
    for (int c = 0; c * 64 < limit; ++c) {
        uint64_t m = cull_chunk(i4, S, base, N, c, lane, sx, sy);
        const int rest = limit - c * 64;
        if (rest < 64) m &= (1ull << rest) - 1ull;
        while (m) {
            const int bit = __builtin_ctzll(m);
            m &= m - 1ull;
            const GSplat s = load_splat(f9, i4, S, base + c * 64 + bit);
            const bool in_x = X >= s.x0 && X <= s.x1;
            const float qx = xf - s.cx;
            const int yb = opaque(Y0);
#pragma unroll
            for (int j = 0; j < GPL; ++j) {
                const int y = yb + 4 * j;
                float qy;
                const float f = gauss(s, in_x, qx, (float)y, y, &qy) * s.a;
                const float gc = (gr[j] * s.r + gg[j] * s.g) + gb[j] * s.b;
                u[j] = (1.0f - f) * u[j] + f * gc;
            }
        }
    }
}

__device__ __forceinline__ float wave_add(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid: nb * nStrips one-wave workgroups, strip fastest.  f9 / i4: prep's stage
// outputs of the whole batch (S = B * N columns), b0: the chunk's first candidate.
// wsum: the plan's weight block (Sum w as a double first).  part: the chunk's
// partials [nb][nStrips][N] of three float4.
__global__ void __launch_bounds__(64, 3)
grad_strip_kernel(const float* __restrict__ f9, const int* __restrict__ i4, int64_t S, int64_t b0, int N, int H,
                  int W, const float* __restrict__ target, const float* __restrict__ mask, int mode, float beta,
                  const double* __restrict__ wsum, int nSX, int nStrips, float4* __restrict__ part) {
    const int lane = (int)threadIdx.x;
    const int bl = (int)(blockIdx.x / (unsigned)nStrips);
    const int strip = (int)(blockIdx.x % (unsigned)nStrips);
#include "ggs_grad_strip.inc"
}

// A target per candidate: candidate b = b0 + bl against image
// pk = b / group of targets [K][H][W][3], masks [K][H][W] (or null) and the set's
// weight blocks, wstride floats apart.  pk is wave-uniform, so the three base
// pointers move on the scalar side; the body is grad_strip_kernel's and a
// candidate's partials are its bits.
__global__ void __launch_bounds__(64, 3)
grad_set_strip_kernel(const float* __restrict__ f9, const int* __restrict__ i4, int64_t S, int64_t b0, int N, int H,
                      int W, const float* __restrict__ targets, const float* __restrict__ masks, int mode,
                      float beta, const float* __restrict__ wblocks, int64_t wstride, int group, int nSX,
                      int nStrips, float4* __restrict__ part) {
    const int lane = (int)threadIdx.x;
    const int bl = (int)(blockIdx.x / (unsigned)nStrips);
    const int strip = (int)(blockIdx.x % (unsigned)nStrips);
    const int64_t pk = (b0 + bl) / group;
    const int64_t px = (int64_t)H * W;
    const float* __restrict__ target = targets + pk * px * 3;
    const float* __restrict__ mask = masks ? masks + pk * px : nullptr;
    const double* __restrict__ wsum = reinterpret_cast<const double*>(wblocks + pk * wstride);
#include "ggs_grad_strip.inc"
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// genomes: the batch's axes-angle rows (stride C); grad [B][N][9].
__global__ void __launch_bounds__(64)
grad_finish_kernel(const float* __restrict__ genomes, int C, const float* __restrict__ f9,
                   const int* __restrict__ i4, int64_t S, int64_t b0, int nb, int N, int H, int W, int nSX, int nSY,
                   const float4* __restrict__ part, float* __restrict__ grad) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)nb * N) return;
    const int bl = (int)(t / N), i = (int)(t % N);
    const int64_t k = (b0 + bl) * (int64_t)N + i;
    const int x0 = i4[0 * S + k], x1 = i4[1 * S + k], y0 = i4[2 * S + k], y1 = i4[3 * S + k];
    const int nStrips = nSX * nSY;
    double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int sx0 = clampi(x0 / GS_W, 0, nSX - 1), sx1 = clampi(x1 / GS_W, 0, nSX - 1);
    const int sy0 = clampi(y0 / GS_H, 0, nSY - 1), sy1 = clampi(y1 / GS_H, 0, nSY - 1);
    for (int sy = sy0; sy <= sy1; ++sy)
        for (int sx = sx0; sx <= sx1; ++sx) {
            if (!strip_hit(x0, x1, y0, y1, sx, sy)) continue;
            const float4* p = part + (((int64_t)bl * nStrips + (sy * nSX + sx)) * (int64_t)N + i) * 3;
            const float4 u = p[0], v = p[1], w = p[2];
            a[0] += (double)u.x;
            a[1] += (double)u.y;
            a[2] += (double)u.z;
            a[3] += (double)u.w;
            a[4] += (double)v.x;
            a[5] += (double)v.y;
            a[6] += (double)v.z;
            a[7] += (double)v.w;
            a[8] += (double)w.x;
        }
    // the sums -> d/d(cx, cy, P, Q, R) with (P, Q, R) the inverse covariance (f9's sxx,
    // sxy, syy): q = P qx^2 + 2 Q qx qy + R qy^2, f = a exp(-q / 2), h = dL/df f
    const double P = f9[2 * S + k], Q = f9[3 * S + k], R = f9[4 * S + k];
    const double dcx = P * a[0] + Q * a[1], dcy = Q * a[0] + R * a[1];
    const double dP = -0.5 * a[2], dQ = -a[3], dR = -0.5 * a[4];
    const double da = a[5], dr = a[6], dg = a[7], db = a[8];

    const float* g = genomes + k * (int64_t)C;
    float* o = grad + k * 9;
    // colours and alpha: clip(clip(x, 0, 255), 0, 255) / 255 (encode.py:50-56, render.py:40-43)
    const double dcol[4] = {dr, dg, db, da};
#pragma unroll
    for (int j = 0; j < 4; ++j) o[5 + j] = (g[5 + j] >= 0.0f && g[5 + j] <= 255.0f) ? (float)(dcol[j] / 255.0) : 0.0f;
    // centre: clip(x, 0, 1) (W - 1) (render.py:15-16)
    o[0] = (g[0] >= 0.0f && g[0] <= 1.0f) ? (float)(dcx * (double)(W - 1)) : 0.0f;
    o[1] = (g[1] >= 0.0f && g[1] <= 1.0f) ? (float)(dcy * (double)(H - 1)) : 0.0f;

    // forward values, encode_row's and preprocess_row's own float32 operations
    const float sxf = det_expf(g[2]), syf = det_expf(g[3]);
    float sn, cs;
    det_sincosf(g[4], &sn, &cs);
    const float sx2 = sxf * sxf, sy2 = syf * syf, c2 = cs * cs, s2 = sn * sn;
    const float vxx = sx2 * c2 + sy2 * s2;
    const float vxy = ((sx2 - sy2) * sn) * cs;
    const float vyy = sx2 * s2 + sy2 * c2;
    const float l11 = ggs_sqrt_rn(nmax(vxx, EPS12));
    const float l21 = ggs_div_rn(vxy, l11);
    const float u22 = vyy - l21 * l21;
    const float l22 = ggs_sqrt_rn(nmax(u22, EPS12));
    const float e11 = det_expf(det_logf(l11)), e22 = det_expf(det_logf(l22));
    const double i11 = (double)ggs_div_rn(1.0f, nmax(e11, EPS6)), i22 = (double)ggs_div_rn(1.0f, nmax(e22, EPS6));
    const double L21 = l21, i21 = -L21 * (i11 * i22);
    // preprocess backward: P = i11^2 + i21^2, Q = i21 i22, R = i22^2, i21 = -l21 i11 i22
    const double di21 = 2.0 * i21 * dP + i22 * dQ;
    double di11 = 2.0 * i11 * dP - L21 * i22 * di21;
    double di22 = i21 * dQ + 2.0 * i22 * dR - L21 * i11 * di21;
    double dl21 = -i11 * i22 * di21;
    // i = 1 / max(exp(ll), 1e-6), ll = log(l): the max passes iff exp(ll) > 1e-6
    const double dll11 = e11 > EPS6 ? -i11 * i11 * di11 * (double)e11 : 0.0;
    const double dll22 = e22 > EPS6 ? -i22 * i22 * di22 * (double)e22 : 0.0;
    // encode backward
    double dl11 = dll11 / (double)l11;
    const double dl22 = dll22 / (double)l22;
    const double du22 = u22 > EPS12 ? dl22 / (2.0 * (double)l22) : 0.0;     // l22 = sqrt(max(u22, 1e-12))
    const double dvyy = du22;
    dl21 += -2.0 * L21 * du22;
    const double dvxy = dl21 / (double)l11;                                // l21 = vxy / l11
    dl11 += -dl21 * L21 / (double)l11;
    const double dvxx = vxx > EPS12 ? dl11 / (2.0 * (double)l11) : 0.0;     // l11 = sqrt(max(vxx, 1e-12))
    const double sc = (double)sn * (double)cs, dsq = (double)sx2 - (double)sy2;
    const double dsx2 = dvxx * c2 + dvxy * sc + dvyy * s2;
    const double dsy2 = dvxx * s2 - dvxy * sc + dvyy * c2;
    o[2] = (float)(dsx2 * 2.0 * (double)sx2);
    o[3] = (float)(dsy2 * 2.0 * (double)sy2);
    o[4] = (float)(dsq * ((dvyy - dvxx) * 2.0 * sc + dvxy * ((double)c2 - (double)s2)));
}

// ---- the renderer's vector-Jacobian product ---------------------------
// grad_strip_kernel's body entered with a cotangent: g is cot [B][H][W][3] of the
// absolute candidate b0 + bl (0 where the image clip is active or the pixel is
// outside the image) and the background is bg0, bg1, bg2 (wave-uniform).
#define GGS_STRIP_VJP 1
__global__ void __launch_bounds__(64, 3)
vjp_strip_kernel(const float* __restrict__ f9, const int* __restrict__ i4, int64_t S, int64_t b0, int N, int H, int W,
                 const float* __restrict__ cot, float bg0, float bg1, float bg2, int nSX, int nStrips,
                 float4* __restrict__ part) {
    const int lane = (int)threadIdx.x;
    const int bl = (int)(blockIdx.x / (unsigned)nStrips);
    const int strip = (int)(blockIdx.x % (unsigned)nStrips);
#include "ggs_grad_strip.inc"
}
#undef GGS_STRIP_VJP

// grad_finish_kernel with the rows' layout as a template argument: GGS_LAYOUT_AXES is
// its arithmetic statement for statement (kept apart so that the pinned code object of
// grad_finish_kernel stays what it is); GGS_LAYOUT_RENDERER stops the chain at
// preprocess (render.py:8-47), the rows being the renderer's x, y, log l11, log l22,
// l21, r, g, b, alpha.  grad [B][N][9].
template <int LAYOUT>
__global__ void __launch_bounds__(64)
vjp_finish_kernel(const float* __restrict__ genomes, int C, const float* __restrict__ f9, const int* __restrict__ i4,
                  int64_t S, int64_t b0, int nb, int N, int H, int W, int nSX, int nSY,
                  const float4* __restrict__ part, float* __restrict__ grad) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)nb * N) return;
    const int bl = (int)(t / N), i = (int)(t % N);
    const int64_t k = (b0 + bl) * (int64_t)N + i;
    const int x0 = i4[0 * S + k], x1 = i4[1 * S + k], y0 = i4[2 * S + k], y1 = i4[3 * S + k];
    const int nStrips = nSX * nSY;
    double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int sx0 = clampi(x0 / GS_W, 0, nSX - 1), sx1 = clampi(x1 / GS_W, 0, nSX - 1);
    const int sy0 = clampi(y0 / GS_H, 0, nSY - 1), sy1 = clampi(y1 / GS_H, 0, nSY - 1);
    for (int sy = sy0; sy <= sy1; ++sy)
        for (int sx = sx0; sx <= sx1; ++sx) {
            if (!strip_hit(x0, x1, y0, y1, sx, sy)) continue;
            const float4* p = part + (((int64_t)bl * nStrips + (sy * nSX + sx)) * (int64_t)N + i) * 3;
            const float4 u = p[0], v = p[1], w = p[2];
            a[0] += (double)u.x;
            a[1] += (double)u.y;
            a[2] += (double)u.z;
            a[3] += (double)u.w;
            a[4] += (double)v.x;
            a[5] += (double)v.y;
            a[6] += (double)v.z;
            a[7] += (double)v.w;
            a[8] += (double)w.x;
        }
    const double P = f9[2 * S + k], Q = f9[3 * S + k], R = f9[4 * S + k];
    const double dcx = P * a[0] + Q * a[1], dcy = Q * a[0] + R * a[1];
    const double dP = -0.5 * a[2], dQ = -a[3], dR = -0.5 * a[4];
    const double da = a[5], dr = a[6], dg = a[7], db = a[8];

    const float* g = genomes + k * (int64_t)C;
    float* o = grad + k * 9;
    // colours and alpha: clip(x, 0, 255) / 255 (render.py:40-43; AXES: encode.py:50-56 clips the same way first)
    const double dcol[4] = {dr, dg, db, da};
#pragma unroll
    for (int j = 0; j < 4; ++j) o[5 + j] = (g[5 + j] >= 0.0f && g[5 + j] <= 255.0f) ? (float)(dcol[j] / 255.0) : 0.0f;
    // centre: clip(x, 0, 1) (W - 1) (render.py:15-16)
    o[0] = (g[0] >= 0.0f && g[0] <= 1.0f) ? (float)(dcx * (double)(W - 1)) : 0.0f;
    o[1] = (g[1] >= 0.0f && g[1] <= 1.0f) ? (float)(dcy * (double)(H - 1)) : 0.0f;

    if (LAYOUT == GGS_LAYOUT_RENDERER) {
        // forward values, preprocess_row's own float32 operations
        const float e11 = det_expf(g[2]), e22 = det_expf(g[3]);
        const double i11 = (double)ggs_div_rn(1.0f, nmax(e11, EPS6)), i22 = (double)ggs_div_rn(1.0f, nmax(e22, EPS6));
        const double L21 = g[4], i21 = -L21 * (i11 * i22);
        // preprocess backward: P = i11^2 + i21^2, Q = i21 i22, R = i22^2, i21 = -l21 i11 i22
        const double di21 = 2.0 * i21 * dP + i22 * dQ;
        const double di11 = 2.0 * i11 * dP - L21 * i22 * di21;
        const double di22 = i21 * dQ + 2.0 * i22 * dR - L21 * i11 * di21;
        // i = 1 / max(exp(ll), 1e-6): the max passes iff exp(ll) > 1e-6
        o[2] = e11 > EPS6 ? (float)(-i11 * i11 * di11 * (double)e11) : 0.0f;
        o[3] = e22 > EPS6 ? (float)(-i22 * i22 * di22 * (double)e22) : 0.0f;
        o[4] = (float)(-i11 * i22 * di21);
        return;
    }
    // forward values, encode_row's and preprocess_row's own float32 operations
    const float sxf = det_expf(g[2]), syf = det_expf(g[3]);
    float sn, cs;
    det_sincosf(g[4], &sn, &cs);
    const float sx2 = sxf * sxf, sy2 = syf * syf, c2 = cs * cs, s2 = sn * sn;
    const float vxx = sx2 * c2 + sy2 * s2;
    const float vxy = ((sx2 - sy2) * sn) * cs;
    const float vyy = sx2 * s2 + sy2 * c2;
    const float l11 = ggs_sqrt_rn(nmax(vxx, EPS12));
    const float l21 = ggs_div_rn(vxy, l11);
    const float u22 = vyy - l21 * l21;
    const float l22 = ggs_sqrt_rn(nmax(u22, EPS12));
    const float e11 = det_expf(det_logf(l11)), e22 = det_expf(det_logf(l22));
    const double i11 = (double)ggs_div_rn(1.0f, nmax(e11, EPS6)), i22 = (double)ggs_div_rn(1.0f, nmax(e22, EPS6));
    const double L21 = l21, i21 = -L21 * (i11 * i22);
    const double di21 = 2.0 * i21 * dP + i22 * dQ;
    double di11 = 2.0 * i11 * dP - L21 * i22 * di21;
    double di22 = i21 * dQ + 2.0 * i22 * dR - L21 * i11 * di21;
    double dl21 = -i11 * i22 * di21;
    const double dll11 = e11 > EPS6 ? -i11 * i11 * di11 * (double)e11 : 0.0;
    const double dll22 = e22 > EPS6 ? -i22 * i22 * di22 * (double)e22 : 0.0;
    // encode backward
    double dl11 = dll11 / (double)l11;
    const double dl22 = dll22 / (double)l22;
    const double du22 = u22 > EPS12 ? dl22 / (2.0 * (double)l22) : 0.0;     // l22 = sqrt(max(u22, 1e-12))
    const double dvyy = du22;
    dl21 += -2.0 * L21 * du22;
    const double dvxy = dl21 / (double)l11;                                // l21 = vxy / l11
    dl11 += -dl21 * L21 / (double)l11;
    const double dvxx = vxx > EPS12 ? dl11 / (2.0 * (double)l11) : 0.0;     // l11 = sqrt(max(vxx, 1e-12))
    const double sc = (double)sn * (double)cs, dsq = (double)sx2 - (double)sy2;
    const double dsx2 = dvxx * c2 + dvxy * sc + dvyy * s2;
    const double dsy2 = dvxx * s2 - dvxy * sc + dvyy * c2;
    o[2] = (float)(dsx2 * 2.0 * (double)sx2);
    o[3] = (float)(dsy2 * 2.0 * (double)sy2);
    o[4] = (float)(dsq * ((dvyy - dvxx) * 2.0 * sc + dvxy * ((double)c2 - (double)s2)));
}

// ---- refine session -------------------------------------------------------------
constexpr float PI32 = 3.14159274101257324219f;     // float32(pi)
constexpr float TWO_PI32 = 6.28318548202514648438f; // float32(2*pi)
__device__ __forceinline__ float wrap_angle(float th) {      // np.remainder(th + pi, 2pi) - pi
    const float x = th + PI32;
    float r = fmodf(x, TWO_PI32);
    if (r != 0.0f && r < 0.0f) r += TWO_PI32;
    return r - PI32;
}

// one workgroup per candidate: x (the state the fitness belongs to) becomes the
// best so far iff fit + 1e-10 < best in float64 (the GA's margin)
__global__ void __launch_bounds__(256)
refine_best_kernel(const float* __restrict__ x, const float* __restrict__ fits, int row, double* __restrict__ best_fit,
                   float* __restrict__ best_x) {
    const int b = (int)blockIdx.x;
    const double f = (double)fits[b];
    if (!(f + 1e-10 < best_fit[b])) return;
    for (int i = (int)threadIdx.x; i < row; i += (int)blockDim.x) best_x[(int64_t)b * row + i] = x[(int64_t)b * row + i];
    __syncthreads();                       // every thread has read best_fit[b]
    if (threadIdx.x == 0) best_fit[b] = f;
}

// ggs/refine.py adam_step, one thread per gene, every operation rounded once
__global__ void __launch_bounds__(256)
refine_adam_kernel(float* __restrict__ x, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g,
                   int64_t n, RefineStepDev p) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % 9);
    const float gi = g[i];
    const float mi = p.beta1 * m[i] + (1.0f - p.beta1) * gi;
    const float vi = p.beta2 * v[i] + (1.0f - p.beta2) * (gi * gi);
    m[i] = mi;
    v[i] = vi;
    const float mh = ggs_div_rn(mi, p.c1);
    const float den = ggs_sqrt_rn(ggs_div_rn(vi, p.c2)) + p.eps;
    float xi = x[i] - ggs_div_rn(p.lr[c] * mh, den);
    // clamp_genome's rule of the column; an angle inside [-pi, pi) keeps its bits
    if (c < 2) xi = fminf(fmaxf(xi, 0.0f), 1.0f);
    else if (c < 4) xi = fminf(fmaxf(xi, p.log_lo), p.log_hi);
    else if (c == 4) xi = (xi >= -PI32 && xi < PI32) ? xi : wrap_angle(xi);
    else xi = fminf(fmaxf(xi, 0.0f), 255.0f);
    x[i] = xi;
}

// ---- memetic generations of the island group -------------------------
constexpr int POLISH_PMAX = RANKMAX;    // an island's rows are ranked by the counting rank in LDS, as the GA's

// One workgroup per island: the rows of fitness rank j < R (ascending fitness, ties
// by lower row: the elite list's rank) become refine candidates k * R + j: x and
// best_x the row's genome, best_fit +inf, rows[k * R + j] the row.
__global__ void __launch_bounds__(POLISH_PMAX)
polish_stage_kernel(const float* __restrict__ pop, const float* __restrict__ fits, int P, int N, int R,
                    int* __restrict__ rows, float* __restrict__ x, float* __restrict__ best_x,
                    double* __restrict__ best_fit) {
    __shared__ float key[POLISH_PMAX];
    __shared__ int top[POLISH_PMAX];
    const int k = (int)blockIdx.x;
    const float* __restrict__ f = fits + (int64_t)k * P;
    for (int r = threadIdx.x; r < P; r += blockDim.x) {
        key[r] = f[r];
        top[r] = 0;                         // a valid row whatever the fitness values (NaN ranks collide)
    }
    __syncthreads();
    for (int r = threadIdx.x; r < P; r += blockDim.x) {
        const float v = key[r];
        int rank = 0;
        for (int q = 0; q < P; ++q) rank += (key[q] < v) | ((key[q] == v) & (q < r));
        if (rank < R) top[rank] = r;
    }
    __syncthreads();
    const int64_t row = (int64_t)N * 9;
    for (int j = 0; j < R; ++j) {
        const int64_t c = (int64_t)k * R + j;
        const float* __restrict__ from = pop + ((int64_t)k * P + top[j]) * row;
        for (int64_t i = threadIdx.x; i < row; i += blockDim.x) {
            const float v = from[i];
            x[c * row + i] = v;
            best_x[c * row + i] = v;
        }
        if (threadIdx.x == 0) {
            rows[c] = top[j];
            best_fit[c] = (double)__builtin_inff();
        }
    }
}

// One workgroup per island: candidate k * R + j's best individual and fitness
// overwrite row rows[k * R + j] iff that fitness is strictly lower than the row's;
// then the island's elite list from the new fitness vector (the migration's closing
// step) and the best so far by the GA's rule (the first lowest row, fit + 1e-10 <
// best in float64).
__global__ void __launch_bounds__(POLISH_PMAX)
polish_install_kernel(float* __restrict__ pop, float* __restrict__ fits, int P, int N, int R, int elite_k,
                      const int* __restrict__ rows, const float* __restrict__ best_x,
                      const double* __restrict__ best_fit, int* __restrict__ elite, double* __restrict__ gbest_fit,
                      float* __restrict__ gbest_ind) {
    __shared__ float key[POLISH_PMAX];
    __shared__ int from_c[POLISH_PMAX];     // the candidate installed in the row, or -1
    __shared__ int s_g;
    const int k = (int)blockIdx.x;
    float* __restrict__ f = fits + (int64_t)k * P;
    const int64_t row = (int64_t)N * 9;
    for (int r = threadIdx.x; r < P; r += blockDim.x) {
        key[r] = f[r];
        from_c[r] = -1;
    }
    __syncthreads();
    for (int j = 0; j < R; ++j) {           // the rows are distinct: no order between them
        const int c = k * R + j, r = rows[c];
        const float bf = (float)best_fit[c];    // a float32 fitness, widened: exact
        if (!(bf < key[r])) continue;       // uniform over the workgroup
        float* __restrict__ to = pop + ((int64_t)k * P + r) * row;
        const float* __restrict__ src = best_x + (int64_t)c * row;
        for (int64_t i = threadIdx.x; i < row; i += blockDim.x) to[i] = src[i];
        __syncthreads();                    // every thread has compared key[r]
        if (threadIdx.x == 0) {
            key[r] = bf;
            f[r] = bf;
            from_c[r] = c;
        }
        __syncthreads();
    }
    const int E = elite_k < 1 ? 1 : elite_k;
    int* __restrict__ el = elite + (int64_t)k * P;
    for (int r = threadIdx.x; r < P; r += blockDim.x) {
        const float v = key[r];
        int rank = 0;
        for (int q = 0; q < P; ++q) rank += (key[q] < v) | ((key[q] == v) & (q < r));
        if (rank < E) el[rank] = r;
    }
    if (threadIdx.x == 0) {
        int g = 0;
        for (int r = 1; r < P; ++r)
            if (key[r] < key[g]) g = r;
        s_g = ((double)key[g] + 1e-10 < gbest_fit[k]) ? g : -1;
    }
    __syncthreads();
    const int g = s_g;
    if (g < 0) return;
    // an installed row is read from its candidate: the row's own stores are this workgroup's
    const float* __restrict__ src =
        from_c[g] >= 0 ? best_x + (int64_t)from_c[g] * row : pop + ((int64_t)k * P + g) * row;
    for (int64_t i = threadIdx.x; i < row; i += blockDim.x) gbest_ind[(int64_t)k * row + i] = src[i];
    if (threadIdx.x == 0) gbest_fit[k] = (double)key[g];
}

}  // namespace

int grad_strips(int H, int W, int* nSX) {
    const int sx = (W + GS_W - 1) / GS_W, sy = (H + GS_H - 1) / GS_H;
    if (nSX) *nSX = sx;
    return sx * sy;
}

size_t grad_partial_bytes(int N, int H, int W) {
    return sizeof(float4) * 3 * (size_t)grad_strips(H, W, nullptr) * (size_t)N;
}

hipError_t launch_grad(hipStream_t st, const float* genomes, int C, const float* f9, const int* i4, int64_t B,
                       int64_t b0, int nb, int N, int H, int W, const float* target, const float* mask, int mode,
                       float beta, const float* wblock, void* partials, float* grad) {
    if (nb <= 0 || N <= 0) return hipSuccess;
    int nSX;
    const int nStrips = grad_strips(H, W, &nSX);
    const int64_t S = B * N;
    hipLaunchKernelGGL(grad_strip_kernel, dim3((unsigned)((int64_t)nb * nStrips)), dim3(64), 0, st, f9, i4, S, b0, N,
                       H, W, target, mask, mode, beta, reinterpret_cast<const double*>(wblock), nSX, nStrips,
                       (float4*)partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t n = (int64_t)nb * N;
    hipLaunchKernelGGL(grad_finish_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, genomes, C, f9, i4, S,
                       b0, nb, N, H, W, nSX, nStrips / nSX, (const float4*)partials, grad);
    return hipGetLastError();
}

hipError_t launch_grad_set(hipStream_t st, const float* genomes, int C, const float* f9, const int* i4, int64_t B,
                           int64_t b0, int nb, int N, int H, int W, const float* targets, const float* masks,
                           int mode, float beta, const float* wblocks, int64_t wstride, int group, void* partials,
                           float* grad) {
    if (nb <= 0 || N <= 0) return hipSuccess;
    if (group < 1) return hipErrorInvalidValue;
    int nSX;
    const int nStrips = grad_strips(H, W, &nSX);
    const int64_t S = B * N;
    hipLaunchKernelGGL(grad_set_strip_kernel, dim3((unsigned)((int64_t)nb * nStrips)), dim3(64), 0, st, f9, i4, S, b0,
                       N, H, W, targets, masks, mode, beta, wblocks, wstride, group, nSX, nStrips, (float4*)partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t n = (int64_t)nb * N;
    hipLaunchKernelGGL(grad_finish_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, genomes, C, f9, i4, S,
                       b0, nb, N, H, W, nSX, nStrips / nSX, (const float4*)partials, grad);
    return hipGetLastError();
}

hipError_t launch_render_vjp(hipStream_t st, int layout, const float* genomes, int C, const float* f9, const int* i4,
                             int64_t B, int64_t b0, int nb, int N, int H, int W, const float* cot, const float bg[3],
                             void* partials, float* grad) {
    if (nb <= 0 || N <= 0) return hipSuccess;
    if (layout != GGS_LAYOUT_RENDERER && layout != GGS_LAYOUT_AXES) return hipErrorInvalidValue;
    int nSX;
    const int nStrips = grad_strips(H, W, &nSX);
    const int64_t S = B * N;
    hipLaunchKernelGGL(vjp_strip_kernel, dim3((unsigned)((int64_t)nb * nStrips)), dim3(64), 0, st, f9, i4, S, b0, N, H,
                       W, cot, bg[0], bg[1], bg[2], nSX, nStrips, (float4*)partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t n = (int64_t)nb * N;
    const dim3 grid((unsigned)((n + 63) / 64));
    if (layout == GGS_LAYOUT_AXES)
        hipLaunchKernelGGL(vjp_finish_kernel<GGS_LAYOUT_AXES>, grid, dim3(64), 0, st, genomes, C, f9, i4, S, b0, nb, N,
                           H, W, nSX, nStrips / nSX, (const float4*)partials, grad);
    else
        hipLaunchKernelGGL(vjp_finish_kernel<GGS_LAYOUT_RENDERER>, grid, dim3(64), 0, st, genomes, C, f9, i4, S, b0,
                           nb, N, H, W, nSX, nStrips / nSX, (const float4*)partials, grad);
    return hipGetLastError();
}

int polish_max_population() { return POLISH_PMAX; }

hipError_t launch_polish_stage(hipStream_t st, int K, const float* pop, const float* fits, int P, int N, int R,
                               int* rows, float* x, float* best_x, double* best_fit) {
    if (K < 1 || P > POLISH_PMAX || R < 1 || R > P) return hipErrorInvalidValue;
    int nt = 64;
    while (nt < P && nt < POLISH_PMAX) nt <<= 1;
    hipLaunchKernelGGL(polish_stage_kernel, dim3(K), dim3(nt < 256 ? 256 : nt), 0, st, pop, fits, P, N, R, rows, x,
                       best_x, best_fit);
    return hipGetLastError();
}

hipError_t launch_polish_install(hipStream_t st, int K, float* pop, float* fits, int P, int N, int R, int elite_k,
                                 const int* rows, const float* best_x, const double* best_fit, int* elite,
                                 double* gbest_fit, float* gbest_ind) {
    if (K < 1 || P > POLISH_PMAX || R < 1 || R > P) return hipErrorInvalidValue;
    int nt = 64;
    while (nt < P && nt < POLISH_PMAX) nt <<= 1;
    hipLaunchKernelGGL(polish_install_kernel, dim3(K), dim3(nt < 256 ? 256 : nt), 0, st, pop, fits, P, N, R, elite_k,
                       rows, best_x, best_fit, elite, gbest_fit, gbest_ind);
    return hipGetLastError();
}

hipError_t launch_refine_best(hipStream_t st, const float* x, const float* fits, int B, int N, double* best_fit,
                              float* best_x) {
    hipLaunchKernelGGL(refine_best_kernel, dim3((unsigned)B), dim3(256), 0, st, x, fits, N * 9, best_fit, best_x);
    return hipGetLastError();
}

hipError_t launch_refine_adam(hipStream_t st, float* x, float* m, float* v, const float* g, int B, int N,
                              const RefineStepDev& p) {
    const int64_t n = (int64_t)B * N * 9;
    hipLaunchKernelGGL(refine_adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, m, v, g, n, p);
    return hipGetLastError();
}

}  // namespace ggs
