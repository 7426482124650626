// Target preparation and importance mask on the device, K images per launch.
//
// Restates ggs/mask.py (the project's restatement of the reference's
// modules/mask.py:1-83 and of the target preparation at algorithm.py:33-39) as
// gfx950 kernels over K images of one input size [K,H0,W0,3] and one work size
// (H, W); blockIdx.y is the image, as in plan_kernel.  Every float32 step is the
// host's step in the host's order (-ffp-contract=off, correctly rounded sqrt and
// division), window sums are taken in double as the host's integral image
// effectively does, and the quantiles of _norm01 are exact order statistics found
// by a radix select.  No float atomics: maxima and histograms are merged with
// integer atomics, so a result does not depend on scheduling.  The stages follow
// one another on the caller's stream with no host synchronisation; every
// data-dependent decision (the /255 range rule, the selected bins) stays in
// device memory.
#include <algorithm>

#include "ggs_detmath.h"
#include "ggs_internal.h"

namespace ggs {
using namespace detmath;

constexpr int kTPB = 256;
constexpr int kBins = 256;                       // radix 8 bits, 4 passes over a 32-bit key
constexpr int kMaxRanks = 2 * kMaxQuantiles;     // two order statistics around each q (n - 1)

// order-preserving 32-bit key of a float (-0 sorts with +0)
__device__ __forceinline__ uint32_t f2key(float v) {
    uint32_t u = __builtin_bit_cast(uint32_t, v);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    return __builtin_bit_cast(float, u);
}

// workgroup maximum of the threads' keys -> one integer atomic on *dst
__device__ __forceinline__ void block_max_key(uint32_t key, uint32_t* dst) {
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
    atomicMax(&s_max, key);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(dst, s_max);
}

// ---- range rule: per-image maximum -----------------------------------------------
// keys[k * 2 + 0]: maximum of raw image k (key; zeroed before the launch)
__global__ __launch_bounds__(kTPB) void max_kernel(const float* __restrict__ x, size_t n_per, uint32_t* keys) {
    const int k = blockIdx.y;
    const float* p = x + (size_t)k * n_per;
    uint32_t m = 0u;
    for (size_t i = (size_t)blockIdx.x * kTPB + threadIdx.x; i < n_per; i += (size_t)gridDim.x * kTPB)
        m = max(m, f2key(p[i]));
    block_max_key(m, &keys[k * 2]);
}

// torch's source index of output j (align_corners=False), clamped at 0
struct Axis {
    int i0, i1;
    float w0, w1;
};
__device__ __forceinline__ Axis axis_src(int j, int n_in, int n_out) {
    const float scale = (float)n_in / (float)n_out;
    float src = ((float)j + 0.5f) * scale - 0.5f;
    src = src < 0.0f ? 0.0f : src;
    Axis a;
    a.i0 = min((int)floorf(src), n_in - 1);
    a.i1 = min(a.i0 + 1, n_in - 1);
    a.w1 = src - (float)a.i0;
    a.w0 = 1.0f - a.w1;
    return a;
}

// prepare_target: /255 when the raw maximum is > 1.5, bilinear resize (x, then y),
// identity when the sizes match.  Also the prepared image's maximum (keys[k*2+1]).
__global__ __launch_bounds__(kTPB) void resize_kernel(const float* __restrict__ img, int H0, int W0, int H, int W,
                                                      uint32_t* keys, float* __restrict__ tgt) {
    const int k = blockIdx.y;
    const int i = blockIdx.x * kTPB + threadIdx.x;
    const bool scale = key2f(keys[k * 2]) > 1.5f;
    const float* src = img + (size_t)k * H0 * W0 * 3;
    uint32_t m = 0u;
    if (i < H * W) {
        const int y = i / W, x = i - y * W;
        float* o = tgt + ((size_t)k * H * W + i) * 3;
        if (H0 == H && W0 == W) {
            for (int c = 0; c < 3; ++c) {
                float v = src[(size_t)i * 3 + c];
                if (scale) v = v / 255.0f;
                o[c] = v;
                m = max(m, f2key(v));
            }
        } else {
            const Axis ay = axis_src(y, H0, H), ax = axis_src(x, W0, W);
            const float* r0 = src + (size_t)ay.i0 * W0 * 3;
            const float* r1 = src + (size_t)ay.i1 * W0 * 3;
            for (int c = 0; c < 3; ++c) {
                float v00 = r0[ax.i0 * 3 + c], v01 = r0[ax.i1 * 3 + c];
                float v10 = r1[ax.i0 * 3 + c], v11 = r1[ax.i1 * 3 + c];
                if (scale) {
                    v00 = v00 / 255.0f;
                    v01 = v01 / 255.0f;
                    v10 = v10 / 255.0f;
                    v11 = v11 / 255.0f;
                }
                const float c0 = v00 * ax.w0 + v01 * ax.w1;
                const float c1 = v10 * ax.w0 + v11 * ax.w1;
                const float v = c0 * ay.w0 + c1 * ay.w1;
                o[c] = v;
                m = max(m, f2key(v));
            }
        }
    }
    block_max_key(m, &keys[k * 2 + 1]);
}

// luma of the prepared target under the range rule of compute_importance_mask
// (mask.py:42) and of _rgb_to_luma (mask.py:8), each on the maximum it sees
__global__ __launch_bounds__(kTPB) void luma_kernel(const float* __restrict__ tgt, int HW, const uint32_t* keys,
                                                    float* __restrict__ y) {
    const int k = blockIdx.y;
    const int i = blockIdx.x * kTPB + threadIdx.x;
    if (i >= HW) return;
    float m = key2f(keys[k * 2 + 1]);
    const bool s1 = m > 1.5f;
    if (s1) m = m / 255.0f;
    const bool s2 = m > 1.5f;
    const float* p = tgt + ((size_t)k * HW + i) * 3;
    float c[3];
    for (int j = 0; j < 3; ++j) {
        float v = p[j];
        if (s1) v = v / 255.0f;
        if (s2) v = v / 255.0f;
        c[j] = v;
    }
    y[(size_t)k * HW + i] = 0.2126f * c[0] + 0.7152f * c[1] + 0.0722f * c[2];
}

// ---- edges -----------------------------------------------------------------------
// avg_pool(s, stride s) value at (py, px) of the pooled grid (in range)
__device__ __forceinline__ float pooled(const float* __restrict__ y, int W, int s, int py, int px) {
    if (s == 1) return y[(size_t)py * W + px];
    double acc = 0.0;
    for (int dy = 0; dy < s; ++dy)
        for (int dx = 0; dx < s; ++dx) acc += (double)y[(size_t)(py * s + dy) * W + (px * s + dx)];
    return (float)(acc / (double)(s * s));
}

// Sobel magnitude (zero padding) of the pooled luma: ed [K][Hs][Ws]
__global__ __launch_bounds__(kTPB) void edge_kernel(const float* __restrict__ y, int H, int W, int s, int Hs, int Ws,
                                                    float* __restrict__ ed) {
    const int k = blockIdx.y;
    const int i = blockIdx.x * kTPB + threadIdx.x;
    if (i >= Hs * Ws) return;
    const int py = i / Ws, px = i - py * Ws;
    const float* yk = y + (size_t)k * H * W;
    float p[3][3];
    for (int dy = 0; dy < 3; ++dy)
        for (int dx = 0; dx < 3; ++dx) {
            const int qy = py + dy - 1, qx = px + dx - 1;
            p[dy][dx] = (qy >= 0 && qy < Hs && qx >= 0 && qx < Ws) ? pooled(yk, W, s, qy, qx) : 0.0f;
        }
    // the host's accumulation order (ggs/mask.py _conv3x3: row-major over the non-zero taps)
    float gx = 0.0f + -1.0f * p[0][0];
    gx = gx + 1.0f * p[0][2];
    gx = gx + -2.0f * p[1][0];
    gx = gx + 2.0f * p[1][2];
    gx = gx + -1.0f * p[2][0];
    gx = gx + 1.0f * p[2][2];
    float gy = 0.0f + -1.0f * p[0][0];
    gy = gy + -2.0f * p[0][1];
    gy = gy + -1.0f * p[0][2];
    gy = gy + 1.0f * p[2][0];
    gy = gy + 2.0f * p[2][1];
    gy = gy + 1.0f * p[2][2];
    ed[(size_t)k * Hs * Ws + i] = ggs_sqrt_rn(gx * gx + gy * gy + EPS12);
}

// edges (+)= resize(ed [Hs][Ws] -> [H][W])
__global__ __launch_bounds__(kTPB) void edge_accum_kernel(const float* __restrict__ ed, int Hs, int Ws, int H, int W,
                                                          int first, float* __restrict__ edges) {
    const int k = blockIdx.y;
    const int i = blockIdx.x * kTPB + threadIdx.x;
    if (i >= H * W) return;
    const float* e = ed + (size_t)k * Hs * Ws;
    float v;
    if (Hs == H && Ws == W) {
        v = e[i];
    } else {
        const int y = i / W, x = i - y * W;
        const Axis ay = axis_src(y, Hs, H), ax = axis_src(x, Ws, W);
        const float* r0 = e + (size_t)ay.i0 * Ws;
        const float* r1 = e + (size_t)ay.i1 * Ws;
        const float c0 = r0[ax.i0] * ax.w0 + r0[ax.i1] * ax.w1;
        const float c1 = r1[ax.i0] * ax.w0 + r1[ax.i1] * ax.w1;
        v = c0 * ay.w0 + c1 * ay.w1;
    }
    float* o = edges + (size_t)k * H * W + i;
    *o = first ? v : *o + v;
}

// ---- k x k box windows (stride 1, zero padding k / 2, count_include_pad) ----------
// VAR: local variance max(mean2 - mean^2, 0); else the window mean.
template <bool VAR>
__global__ __launch_bounds__(kTPB) void box_kernel(const float* __restrict__ in, int H, int W, int kk,
                                                   float* __restrict__ out) {
    const int k = blockIdx.y;
    const int i = blockIdx.x * kTPB + threadIdx.x;
    if (i >= H * W) return;
    const int y = i / W, x = i - y * W, pad = kk / 2;
    const float* p = in + (size_t)k * H * W;
    const int y0 = max(y - pad, 0), y1 = min(y - pad + kk - 1, H - 1);
    const int x0 = max(x - pad, 0), x1 = min(x - pad + kk - 1, W - 1);
    double a = 0.0, b = 0.0;
    for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx) {
            const float v = p[(size_t)yy * W + xx];
            a += (double)v;
            if (VAR) b += (double)(v * v);
        }
    const double area = (double)kk * (double)kk;
    const float mean = (float)(a / area);
    float r = mean;
    if (VAR) {
        const float mean2 = (float)(b / area);
        r = mean2 - mean * mean;
        r = r < 0.0f ? 0.0f : r;
    }
    out[(size_t)k * H * W + i] = r;
}

// ---- exact quantiles by radix select ---------------------------------------------
// A arrays of n floats; per array R = 2 nq ranks (floor(q (n - 1)) and the next).
// State per (array, rank): the key prefix found so far and the rank among the
// elements that share it.  A pass histograms the next 8 key bits of the elements
// matching a rank's prefix (LDS per workgroup, merged with integer atomics) and
// pick_kernel descends into the bin that holds the rank.  Ranks whose prefixes
// coincide share the histogram of the first of them.
struct QArgs {
    double q[kMaxQuantiles];
    int nq;
};

__global__ __launch_bounds__(kBins) void select_init_kernel(uint32_t n, QArgs qa, uint32_t* prefix, uint32_t* rank,
                                                            uint32_t* hist) {
    const int a = blockIdx.x, R = 2 * qa.nq;
    for (int j = threadIdx.x; j < R * kBins; j += kBins) hist[(size_t)a * R * kBins + j] = 0u;
    if ((int)threadIdx.x < qa.nq) {
        const double idx = qa.q[threadIdx.x] * (double)(n - 1u);
        uint32_t lo = (uint32_t)floor(idx);
        lo = min(lo, n - 1u);
        const uint32_t hi = min(lo + 1u, n - 1u);
        const int r = 2 * threadIdx.x;
        prefix[a * R + r] = 0u;
        prefix[a * R + r + 1] = 0u;
        rank[a * R + r] = lo;
        rank[a * R + r + 1] = hi;
    }
}

// first rank of the array with the same prefix (its histogram is the shared one)
__device__ __forceinline__ int rank_rep(const uint32_t* sp, int r) {
    int rep = r;
    for (int j = r - 1; j >= 0; --j)
        if (sp[j] == sp[r]) rep = j;
    return rep;
}

__global__ __launch_bounds__(kTPB) void select_hist_kernel(const float* __restrict__ x, uint32_t n, int R, int shift,
                                                           const uint32_t* __restrict__ prefix, uint32_t* hist) {
    __shared__ uint32_t h[kMaxRanks * kBins];
    __shared__ uint32_t sp[kMaxRanks];
    __shared__ int own[kMaxRanks];
    const int a = blockIdx.y;
    for (int j = threadIdx.x; j < R * kBins; j += kTPB) h[j] = 0u;
    if ((int)threadIdx.x < R) sp[threadIdx.x] = prefix[a * R + threadIdx.x];
    __syncthreads();
    if ((int)threadIdx.x < R) own[threadIdx.x] = rank_rep(sp, threadIdx.x) == (int)threadIdx.x;
    __syncthreads();
    const float* p = x + (size_t)a * n;
    for (uint32_t i = blockIdx.x * kTPB + threadIdx.x; i < n; i += gridDim.x * kTPB) {
        const uint32_t key = f2key(p[i]);
        const uint32_t d = (key >> shift) & (kBins - 1);
        for (int r = 0; r < R; ++r) {
            if (!own[r]) continue;
            // pass 0 (shift 24): no prefix yet; later passes compare the bits above the digit
            if (shift == 24 || ((key ^ sp[r]) >> (shift + 8)) == 0u) atomicAdd(&h[r * kBins + d], 1u);
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < R * kBins; j += kTPB)
        if (h[j]) atomicAdd(&hist[(size_t)a * R * kBins + j], h[j]);
}

// numpy's 'linear' quantile from the two order statistics (numpy _lerp, in double)
__device__ __forceinline__ float quantile_lerp(float lo, float hi, double q, uint32_t n) {
    const double idx = q * (double)(n - 1u);
    const double t = idx - floor(idx);
    const double a = (double)lo, b = (double)hi, d = b - a;
    double v = a + d * t;
    if (t >= 0.5) v = b - d * (1.0 - t);
    return (float)v;
}

__global__ __launch_bounds__(kBins) void select_pick_kernel(uint32_t n, QArgs qa, int shift, uint32_t* prefix,
                                                            uint32_t* rank, uint32_t* hist, float* qout) {
    __shared__ uint32_t sp[kMaxRanks], np_[kMaxRanks], nr[kMaxRanks];
    const int a = blockIdx.x, R = 2 * qa.nq;
    if ((int)threadIdx.x < R) sp[threadIdx.x] = prefix[a * R + threadIdx.x];
    __syncthreads();
    if ((int)threadIdx.x < R) {
        const int r = threadIdx.x;
        const uint32_t* hh = hist + ((size_t)a * R + rank_rep(sp, r)) * kBins;
        const uint32_t want = rank[a * R + r];
        uint32_t cum = 0u;
        int b = 0;
        for (; b < kBins - 1; ++b) {
            const uint32_t c = hh[b];
            if (want < cum + c) break;
            cum += c;
        }
        np_[r] = sp[r] | ((uint32_t)b << shift);
        nr[r] = want - cum;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < R * kBins; j += kBins) hist[(size_t)a * R * kBins + j] = 0u;
    if ((int)threadIdx.x < R) {
        prefix[a * R + threadIdx.x] = np_[threadIdx.x];
        rank[a * R + threadIdx.x] = nr[threadIdx.x];
    }
    if (shift == 0 && (int)threadIdx.x < qa.nq) {
        const int iq = threadIdx.x;
        qout[a * qa.nq + iq] = quantile_lerp(key2f(np_[2 * iq]), key2f(np_[2 * iq + 1]), qa.q[iq], n);
    }
}

// ---- _norm01 and the combination ---------------------------------------------------
__device__ __forceinline__ float norm01(float t, float ql, float qh) {
    const float v = (t - ql) / (qh - ql + EPS12);
    return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
}

// m = w_edge _norm01(edges) + w_var _norm01(var); qv: [2][K][2] (edges, then var)
__global__ __launch_bounds__(kTPB) void combine_kernel(const float* __restrict__ edges, const float* __restrict__ var,
                                                       int HW, int K, const float* __restrict__ qv, float w_edge,
                                                       float w_var, float* __restrict__ m) {
    const int k = blockIdx.y;
    const int i = blockIdx.x * kTPB + threadIdx.x;
    if (i >= HW) return;
    const size_t o = (size_t)k * HW + i;
    const float E = norm01(edges[o], qv[k * 2], qv[k * 2 + 1]);
    const float V = norm01(var[o], qv[(K + k) * 2], qv[(K + k) * 2 + 1]);
    m[o] = w_edge * E + w_var * V;
}

__global__ __launch_bounds__(kTPB) void norm_kernel(const float* __restrict__ in, int HW, const float* __restrict__ qv,
                                                    float* __restrict__ out) {
    const int k = blockIdx.y;
    const int i = blockIdx.x * kTPB + threadIdx.x;
    if (i >= HW) return;
    const size_t o = (size_t)k * HW + i;
    out[o] = norm01(in[o], qv[k * 2], qv[k * 2 + 1]);
}

// _norm01, pow(gamma) (detmath exp / log, 0 -> 0), the floor and the strength blend
struct FinalPrm {
    float gamma, one_m_floor, floor, one_m_strength, strength;
    int blend;
};
__global__ __launch_bounds__(kTPB) void final_kernel(const float* __restrict__ in, int HW,
                                                     const float* __restrict__ qv, FinalPrm fp,
                                                     float* __restrict__ out) {
    const int k = blockIdx.y;
    const int i = blockIdx.x * kTPB + threadIdx.x;
    if (i >= HW) return;
    const size_t o = (size_t)k * HW + i;
    float m = norm01(in[o], qv[k * 2], qv[k * 2 + 1]);
    if (fp.gamma != 1.0f) m = m == 0.0f ? 0.0f : det_expf(fp.gamma * det_logf(m));
    m = fp.one_m_floor * m + fp.floor;
    if (fp.blend) m = fp.one_m_strength * 1.0f + fp.strength * m;
    out[o] = m;
}

static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
static inline dim3 grid_for(int n, int K) { return dim3((unsigned)((n + kTPB - 1) / kTPB), (unsigned)K); }

size_t quantile_ws_bytes(int A, int nq) {
    const size_t R = 2 * (size_t)nq;
    return align256(sizeof(uint32_t) * A * R * kBins) + 2 * align256(sizeof(uint32_t) * A * R);
}

hipError_t launch_quantiles(hipStream_t st, const float* x, int A, int64_t n, const double* q, int nq, void* ws,
                            float* d_out) {
    QArgs qa;
    qa.nq = nq;
    for (int i = 0; i < kMaxQuantiles; ++i) qa.q[i] = i < nq ? q[i] : 0.0;
    const int R = 2 * nq;
    char* w = (char*)ws;
    uint32_t* hist = (uint32_t*)w;
    w += align256(sizeof(uint32_t) * (size_t)A * R * kBins);
    uint32_t* prefix = (uint32_t*)w;
    w += align256(sizeof(uint32_t) * (size_t)A * R);
    uint32_t* rank = (uint32_t*)w;
    const uint32_t un = (uint32_t)n;
    const unsigned nb = (unsigned)std::min<int64_t>(std::max<int64_t>((n + 4095) / 4096, 1), 256);
    hipLaunchKernelGGL(select_init_kernel, dim3(A), dim3(kBins), 0, st, un, qa, prefix, rank, hist);
    for (int shift = 24; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(select_hist_kernel, dim3(nb, A), dim3(kTPB), 0, st, x, un, R, shift, prefix, hist);
        hipLaunchKernelGGL(select_pick_kernel, dim3(A), dim3(kBins), 0, st, un, qa, shift, prefix, rank, hist,
                           d_out);
    }
    return hipGetLastError();
}

// workspace: keys [K][2], quantiles [4][K][2], the select state of K arrays, four
// [K][H][W] float planes
size_t targets_prepare_ws_bytes(int K, int H, int W, bool masks) {
    size_t b = align256(sizeof(uint32_t) * 2 * (size_t)K);
    if (!masks) return b;
    b += align256(sizeof(float) * 8 * (size_t)K) + align256(quantile_ws_bytes(K, 2));
    return b + 4 * align256(sizeof(float) * (size_t)K * H * W);
}

hipError_t launch_targets_prepare(hipStream_t st, const float* imgs, int K, int H0, int W0, int H, int W,
                                  const ggs_mask_params* prm, float* targets, float* masks, void* ws) {
    char* w = (char*)ws;
    uint32_t* keys = (uint32_t*)w;
    w += align256(sizeof(uint32_t) * 2 * (size_t)K);
    hipError_t e = hipMemsetAsync(keys, 0, sizeof(uint32_t) * 2 * (size_t)K, st);
    if (e != hipSuccess) return e;
    const size_t n_in = (size_t)H0 * W0 * 3;
    const unsigned nbm = (unsigned)std::min<size_t>(std::max<size_t>((n_in + 4095) / 4096, 1), 1024);
    const int HW = H * W;
    hipLaunchKernelGGL(max_kernel, dim3(nbm, K), dim3(kTPB), 0, st, imgs, n_in, keys);
    hipLaunchKernelGGL(resize_kernel, grid_for(HW, K), dim3(kTPB), 0, st, imgs, H0, W0, H, W, keys, targets);
    if (!prm) return hipGetLastError();

    float* qv = (float*)w;                       // [4][K][2]: edges, var, combined, smoothed
    w += align256(sizeof(float) * 8 * (size_t)K);
    void* qws = w;
    w += align256(quantile_ws_bytes(K, 2));
    const size_t plane = align256(sizeof(float) * (size_t)K * HW);
    float* pa = (float*)w;                       // luma, later the normalised combination
    float* pb = (float*)(w + plane);             // edges, later the smoothed mask
    float* pc = (float*)(w + 2 * plane);         // variance
    float* pd = (float*)(w + 3 * plane);         // per-scale Sobel, later the combination
    const double q[2] = {0.02, 0.98};

    hipLaunchKernelGGL(luma_kernel, grid_for(HW, K), dim3(kTPB), 0, st, targets, HW, keys, pa);
    for (int si = 0; si < prm->n_scales; ++si) {
        const int s = prm->edge_scales[si], Hs = H / s, Ws = W / s;
        hipLaunchKernelGGL(edge_kernel, grid_for(Hs * Ws, K), dim3(kTPB), 0, st, pa, H, W, s, Hs, Ws, pd);
        hipLaunchKernelGGL(edge_accum_kernel, grid_for(HW, K), dim3(kTPB), 0, st, pd, Hs, Ws, H, W, si == 0, pb);
    }
    hipLaunchKernelGGL(box_kernel<true>, grid_for(HW, K), dim3(kTPB), 0, st, pa, H, W, 9, pc);
    if ((e = launch_quantiles(st, pb, K, HW, q, 2, qws, qv)) != hipSuccess) return e;
    if ((e = launch_quantiles(st, pc, K, HW, q, 2, qws, qv + 2 * K)) != hipSuccess) return e;
    hipLaunchKernelGGL(combine_kernel, grid_for(HW, K), dim3(kTPB), 0, st, pb, pc, HW, K, qv, prm->w_edge,
                       prm->w_var, pd);
    if ((e = launch_quantiles(st, pd, K, HW, q, 2, qws, qv + 4 * K)) != hipSuccess) return e;
    const float* last = pd;
    const float* lastq = qv + 4 * K;
    if (prm->smooth > 0) {
        hipLaunchKernelGGL(norm_kernel, grid_for(HW, K), dim3(kTPB), 0, st, pd, HW, qv + 4 * K, pa);
        hipLaunchKernelGGL(box_kernel<false>, grid_for(HW, K), dim3(kTPB), 0, st, pa, H, W, prm->smooth, pb);
        if ((e = launch_quantiles(st, pb, K, HW, q, 2, qws, qv + 6 * K)) != hipSuccess) return e;
        last = pb;
        lastq = qv + 6 * K;
    }
    FinalPrm fp;
    fp.gamma = prm->gamma;
    fp.one_m_floor = (float)(1.0 - (double)prm->floor);
    fp.floor = prm->floor;
    fp.one_m_strength = (float)(1.0 - (double)prm->strength);
    fp.strength = prm->strength;
    fp.blend = prm->strength < 1.0f;
    hipLaunchKernelGGL(final_kernel, grid_for(HW, K), dim3(kTPB), 0, st, last, HW, lastq, fp, masks);
    return hipGetLastError();
}

}  // namespace ggs
