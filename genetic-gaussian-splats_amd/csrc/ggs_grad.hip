// Fitness gradients: d fitness / d genome for the nine axes-angle
// genes of every splat, and the Adam refiner's elementwise kernels.
//
//   grad_strip_kernel   one wave per (candidate, 16 x 32 pixel strip): the per-pixel
//                       backward of the "over" blend, reduced over the strip to nine
//                       sums per visited splat -> partials [b][strip][splat][12]
//   grad_finish_kernel  one thread per (candidate, splat): the strip partials summed
//                       in ascending strip order (float64), then the chain rule
//                       through preprocess (render.py:8-47) and encode
//                       (encode.py:4-59) -> grad [b][s][9]
//   refine_best_kernel / refine_adam_kernel   the refine session's step
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
    const int sx = strip % nSX, sy = strip / nSX;
    const int64_t base = (b0 + bl) * (int64_t)N;
    const int X = sx * GS_W + (lane & 15);
    const int Y0 = sy * GS_H + (lane >> 4);
    const float xf = (float)X;
    const int nC = (N + 63) / 64;

    // ---- sweep 1: the unclipped final colour ---------------------------------
    float cr[GPL], cg[GPL], cb[GPL];
#pragma unroll
    for (int j = 0; j < GPL; ++j) cr[j] = cg[j] = cb[j] = 1.0f;     // fitness.py:15: white background
    canvas_upto(f9, i4, S, base, N, N, lane, sx, sy, X, Y0, cr, cg, cb);

    // ---- g = dL/dCf per channel (0 where the image clip is active), S = g . Cf ----
    const double hw = (double)H * (double)W;
    double D;
    if (mode == GGS_FIT_NONE) D = 3.0 * hw;                          // fitness.py:18-19
    else if (mode == GGS_FIT_WEIGHTED) D = *wsum + 1e-12;            // fitness.py:28-31
    else D = 3.0 * hw * (*wsum / hw + 1e-12);                        // fitness.py:23-27
    const float coef = (float)(2.0 / D);
    float T[GPL], Sg[GPL], gr[GPL], gg[GPL], gb[GPL];
#pragma unroll
    for (int j = 0; j < GPL; ++j) {
        const int y = Y0 + 4 * j;
        float r = 0.0f, g = 0.0f, b = 0.0f;
        if (X < W && y < H) {
            const int64_t p = (int64_t)y * W + X;
            float om = 1.0f;
            if (mode == GGS_FIT_WEIGHTED) om = mask[p];
            else if (mode == GGS_FIT_BOOST) om = 1.0f + beta * fminf(fmaxf(mask[p], 0.0f), 1.0f);
            const float k = om * coef;
            const float tr = target[3 * p + 0], tg = target[3 * p + 1], tb = target[3 * p + 2];
            r = (cr[j] >= 0.0f && cr[j] <= 1.0f) ? (cr[j] - tr) * k : 0.0f;
            g = (cg[j] >= 0.0f && cg[j] <= 1.0f) ? (cg[j] - tg) * k : 0.0f;
            b = (cb[j] >= 0.0f && cb[j] <= 1.0f) ? (cb[j] - tb) * k : 0.0f;
        }
        gr[j] = r;
        gg[j] = g;
        gb[j] = b;
        Sg[j] = (r * cr[j] + g * cg[j]) + b * cb[j];
        T[j] = 1.0f;
    }

    // ---- sweep 2: front to back ------------------------------------------------
    float4* const out = part + ((int64_t)bl * nStrips + strip) * (int64_t)N * 3;
    for (int c = nC - 1; c >= 0; --c) {
        uint64_t m = cull_chunk(i4, S, base, N, c, lane, sx, sy);
        while (m) {
            const int bit = 63 - __builtin_clzll(m);
            m &= ~(1ull << bit);
            const int i = c * 64 + bit;
            const GSplat s = load_splat(f9, i4, S, base + i);
            const bool in_x = X >= s.x0 && X <= s.x1;
            const float qx = xf - s.cx;
            const int yb = opaque(Y0);
            // 1 - f >= 1 - a: only a nearly opaque splat can need the exact walk
            bool exact = false;
            if (s.a > 1.0f - ONE_MINUS_F_MIN) {
                bool low = false;
#pragma unroll
                for (int j = 0; j < GPL; ++j) {
                    const int y = yb + 4 * j;
                    float qy;
                    const float e = gauss(s, in_x, qx, (float)y, y, &qy);
                    low = low || (e > 0.0f && 1.0f - e * s.a < ONE_MINUS_F_MIN);
                }
                exact = __builtin_amdgcn_ballot_w64(low) != 0ull;
            }
            // exact: u = g . canvas_{i-1}, linear in the canvas, so the walk carries one
            // float per pixel: u <- (1 - f) u + f (g . c) from u = g . background
            float u[GPL];
            if (exact) {
#pragma unroll
                for (int j = 0; j < GPL; ++j) u[j] = (gr[j] + gg[j]) + opaque(gb[j]);
                gdot_canvas_upto(f9, i4, S, base, N, i, lane, sx, sy, X, Y0, gr, gg, gb, u);
            }
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, a6 = 0.f, a7 = 0.f, a8 = 0.f;
#pragma unroll
            for (int j = 0; j < GPL; ++j) {
                const int y = yb + 4 * j;
                float qy;
                const float e = gauss(s, in_x, qx, (float)y, y, &qy);
                const float f = e * s.a;
                const float gc = (gr[j] * s.r + gg[j] * s.g) + gb[j] * s.b;
                const float w = T[j] * f;
                const float wgc = w * gc;
                const float rest = Sg[j] - wgc;          // T (1 - f) g . canvas_{i-1}
                float back;                               // T g . canvas_{i-1}
                if (exact) back = T[j] * u[j];
                else back = rest * __builtin_amdgcn_rcpf(1.0f - f);
                const float dLdf = T[j] * gc - back;
                const float h = dLdf * f;
                const float hx = h * qx, hy = h * qy;
                a0 += hx;
                a1 += hy;
                a2 += hx * qx;
                a3 += hx * qy;
                a4 += hy * qy;
                a5 += dLdf * e;
                a6 += w * gr[j];
                a7 += w * gg[j];
                a8 += w * gb[j];
                Sg[j] = rest;
                T[j] = T[j] - w;
            }
            a0 = wave_add(a0);
            a1 = wave_add(a1);
            a2 = wave_add(a2);
            a3 = wave_add(a3);
            a4 = wave_add(a4);
            a5 = wave_add(a5);
            a6 = wave_add(a6);
            a7 = wave_add(a7);
            a8 = wave_add(a8);
            if (lane == 0) {
                out[(int64_t)i * 3 + 0] = make_float4(a0, a1, a2, a3);
                out[(int64_t)i * 3 + 1] = make_float4(a4, a5, a6, a7);
                out[(int64_t)i * 3 + 2] = make_float4(a8, 0.0f, 0.0f, 0.0f);
            }
        }
    }
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
