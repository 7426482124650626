// Image losses on the device: for candidate b with image x = img[b]
// [H][W][3] and target y = targets[b / group],
//   loss[b] = w_l1 mean|x - y| + w_mse mean (x - y)^2 + w_ssim (1 - mean SSIM(x, y))
// and, on request, cot[b] = d loss[b] / d x.  SSIM per channel, the 11 x 11 separable
// Gaussian window (sigma 1.5) with zero padding, C1 = 0.01^2, C2 = 0.03^2.
//
// Arithmetic: float64 from the float32 inputs on (window moments, the SSIM algebra,
// the three derivative maps and their second convolution, every sum); only loss[b]
// and cot are rounded to float32, once.  In a flat region where x = y the derivative
// maps are ~ +-1/C2 and cancel to O(1): a float32 graph loses 5e-5 of max|cot| there.
//
// image_loss_kernel: one workgroup of 256 threads per (candidate, 16 x 16 output tile).
// The tile plus its halo (5 pixels for the loss, 10 with a cotangent: the maps are
// needed on the tile plus 5) is read from HBM once, all three interleaved channels of
// a row segment in one coalesced read, into LDS as float32; the channels are then
// processed one after another with the float64 buffers reused, and no intermediate map
// touches HBM.  Pixels outside the image are the zeros of the padding, never reads.
// The tile's sums (Sum |d|, Sum d^2, Sum m over its own pixels) are reduced by a fixed
// tree and written to partials [B][tiles][3]; image_loss_finalize_kernel adds them in
// a fixed order.  No atomics: reruns and other batches give a candidate the same bits,
// and the loss bits do not depend on whether a cotangent was asked for.
#include <hip/hip_runtime.h>
#include <math.h>

#include "ggs_internal.h"

namespace ggs {
namespace {

constexpr int kLossTile = 16;       // output tile side
constexpr int kLossTaps = 11;       // window taps (radius 5)
constexpr int kLossRad = 5;
constexpr int kLossThreads = 256;   // = kLossTile^2: one thread per output pixel

struct LossTaps {
    double w[kLossTaps];
};

struct LossWeights {
    double c_l1, c_mse, c_ssim;     // w_l1 / n, 2 w_mse / n, w_ssim / n with n = 3 H W
};

constexpr int cmax(int a, int b) { return a > b ? a : b; }

template <bool WITH_COT>
__global__ __launch_bounds__(kLossThreads) void image_loss_kernel(
    const float* __restrict__ img, const float* __restrict__ targets, int group, int H, int W, int nTX, int nTiles,
    LossTaps taps, LossWeights lw, double* __restrict__ partials, float* __restrict__ cot) {
    constexpr int T = kLossTile;
    constexpr int HALO = WITH_COT ? 2 * kLossRad : kLossRad;
    constexpr int S = T + 2 * HALO;                       // staged side: 36 / 26
    constexpr int M = WITH_COT ? T + 2 * kLossRad : T;    // side of the region m and the maps are formed on
    constexpr int MOFF = (M - T) / 2;
    constexpr int G = WITH_COT ? 4 : 2;                   // adjacent outputs of a pass per thread
    constexpr int SEGS = (M + G - 1) / G;                 // such groups per row or column of the region
    static_assert(S * SEGS <= kLossThreads && T % G == 0, "one row-pass group per thread");
    constexpr int HB = cmax(cmax(S * M, WITH_COT ? 3 * M * T : 0), 3 * kLossThreads);

    __shared__ float sx[3][S][S];
    __shared__ float sy[3][S][S];
    __shared__ double hb[HB];                             // row-pass results; the reduction at the end
    __shared__ double maps[WITH_COT ? 3 : 1][WITH_COT ? M * M : 1];
    __shared__ double mt[T * T];                          // m on the tile's own pixels
    __shared__ float ost[WITH_COT ? T * T * 3 : 1];       // the tile's cotangent, written out in whole rows

    __shared__ double swt[kLossTaps];

    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x / nTiles;
    const int t = blockIdx.x % nTiles;
    const int ty0 = (t / nTX) * T, tx0 = (t % nTX) * T;
    const size_t plane = (size_t)H * W * 3;
    const float* __restrict__ x = img + (size_t)b * plane;
    const float* __restrict__ y = targets + (size_t)(b / group) * plane;
    const bool ssim_on = lw.c_ssim != 0.0;

    // The staged region in two sweeps, every global load issued before the first LDS store:
    // a pixel outside the image (or, without an SSIM term, in the halo nothing reads) is
    // a zero, and its load is aimed at the nearest pixel inside instead of being skipped.
    constexpr int NLD = (S * S * 3 + kLossThreads - 1) / kLossThreads;
    float lx[NLD], ly[NLD];
#pragma unroll
    for (int it = 0; it < NLD; ++it) {
        const int i = min(tid + it * kLossThreads, S * S * 3 - 1);
        const int r = i / (S * 3), q = i % (S * 3);
        const int c = q / 3, ch = q % 3;
        const int gy = ty0 - HALO + r, gx = tx0 - HALO + c;
        const bool wanted = ssim_on || (r >= HALO && r < HALO + T && c >= HALO && c < HALO + T);
        const bool in = wanted && gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t o = ((size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1)) * 3 + ch;
        const float vx = x[o], vy = y[o];
        lx[it] = in ? vx : 0.f;
        ly[it] = in ? vy : 0.f;
    }
#pragma unroll
    for (int it = 0; it < NLD; ++it) {
        const int i = tid + it * kLossThreads;
        if (i < S * S * 3) {
            const int r = i / (S * 3), q = i % (S * 3);
            sx[q % 3][r][q / 3] = lx[it];
            sy[q % 3][r][q / 3] = ly[it];
        }
    }
    if (tid < kLossTaps) swt[tid] = taps.w[tid];
    __syncthreads();
    // the taps in vector registers (read back from LDS): 22 scalar registers fewer
    double wt[kLossTaps];
#pragma unroll
    for (int j = 0; j < kLossTaps; ++j) wt[j] = swt[j];

    const int oy = tid / T, ox = tid % T;                  // this thread's output pixel
    const bool own_in = ty0 + oy < H && tx0 + ox < W;
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    double s1 = 0.0, s2 = 0.0, sm = 0.0;

#pragma unroll 1
    for (int ch = 0; ch < 3; ++ch) {
        double m_own = 0.0, g = 0.0;
        if (ssim_on) {
            // The five window moments E[x], E[y], E[x^2], E[y^2], E[xy] on the M x M region,
            // one at a time: a row pass through hb, the column pass into registers.  A
            // thread takes G adjacent outputs of a pass, so a window value is read from LDS
            // once for the G outputs it feeds (and, in the row pass, for all five moments).
            const int hr = tid / SEGS, hc0 = (tid % SEGS) * G;        // row pass: row, first column
            const int vc = tid % M, vr0 = (tid / M) * G;              // column pass: column, first row
            const bool h_on = tid < S * SEGS, v_on = tid < M * SEGS;
            double xw[G + kLossTaps - 1], yw[G + kLossTaps - 1];
#pragma unroll
            for (int j = 0; j < G + kLossTaps - 1; ++j) {
                const int cc = min(hc0 + j, S - 1);                   // past the row: feeds no stored output
                xw[j] = h_on ? (double)sx[ch][hr][cc] : 0.0;
                yw[j] = h_on ? (double)sy[ch][hr][cc] : 0.0;
            }
            double acc[G][5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                if (h_on) {
#pragma unroll
                    for (int q = 0; q < G; ++q) {
                        double a = 0.0;
#pragma unroll
                        for (int j = 0; j < kLossTaps; ++j) {
                            const double vx = xw[q + j], vy = yw[q + j];
                            const double v = k == 0 ? vx : k == 1 ? vy : k == 2 ? vx * vx : k == 3 ? vy * vy : vx * vy;
                            a = fma(wt[j], v, a);
                        }
                        if (hc0 + q < M) hb[hr * M + hc0 + q] = a;
                    }
                }
                __syncthreads();
                double hw[G + kLossTaps - 1];
#pragma unroll
                for (int j = 0; j < G + kLossTaps - 1; ++j)
                    hw[j] = v_on ? hb[min(vr0 + j, S - 1) * M + vc] : 0.0;
#pragma unroll
                for (int q = 0; q < G; ++q) {
                    double a = 0.0;
#pragma unroll
                    for (int j = 0; j < kLossTaps; ++j) a = fma(wt[j], hw[q + j], a);
                    acc[q][k] = a;
                }
                __syncthreads();
            }
#pragma unroll
            for (int q = 0; q < G; ++q) {
                const int r = vr0 + q, c = vc;
                if (v_on && r < M) {
                    const int p = r * M + c;
                    const int gy = ty0 - MOFF + r, gx = tx0 - MOFF + c;
                    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
                    const double mux = acc[q][0], muy = acc[q][1];
                    const double vxx = acc[q][2] - mux * mux, vyy = acc[q][3] - muy * muy, vxy = acc[q][4] - mux * muy;
                    const double A1 = 2.0 * (mux * muy) + C1, A2 = 2.0 * vxy + C2;
                    const double B1 = (mux * mux + muy * muy) + C1, B2 = (vxx + vyy) + C2;
                    const double den = B1 * B2;
                    const double m = in ? (A1 * A2) / den : 0.0;
                    if (WITH_COT) {
                        // the partials of m at this window centre, the variances held fixed
                        const double dmu = in ? (2.0 * A2) * (muy * B1 - mux * A1) / (B1 * den) : 0.0;
                        const double dxx = in ? -(A1 * A2) / (den * B2) : 0.0;
                        const double dxy = in ? (2.0 * A1) / den : 0.0;
                        maps[0][p] = dmu - 2.0 * mux * dxx - muy * dxy;
                        maps[1][p] = dxx;
                        maps[2][p] = dxy;
                    }
                    const int ry = r - MOFF, rx = c - MOFF;
                    if (ry >= 0 && ry < T && rx >= 0 && rx < T) mt[ry * T + rx] = m;
                }
            }
            __syncthreads();
            m_own = mt[tid];
            if (WITH_COT) {
                // the maps convolved again down to the tile (the zero-padded symmetric window
                // is its own adjoint): d Sum m / d x_p = conv(a) + 2 x_p conv(dxx) + y_p conv(dxy)
                for (int i = tid; i < 3 * M * (T / G); i += kLossThreads) {
                    const int k = i / (M * (T / G)), rem = i % (M * (T / G));
                    const int r = rem / (T / G), c0 = (rem % (T / G)) * G;
                    double mw[G + kLossTaps - 1];
#pragma unroll
                    for (int j = 0; j < G + kLossTaps - 1; ++j) mw[j] = maps[k][r * M + c0 + j];
#pragma unroll
                    for (int q = 0; q < G; ++q) {
                        double a = 0.0;
#pragma unroll
                        for (int j = 0; j < kLossTaps; ++j) a = fma(wt[j], mw[q + j], a);
                        hb[k * M * T + r * T + c0 + q] = a;
                    }
                }
                __syncthreads();
                double cv[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    double a = 0.0;
#pragma unroll
                    for (int j = 0; j < kLossTaps; ++j) a = fma(wt[j], hb[k * M * T + (oy + j) * T + ox], a);
                    cv[k] = a;
                }
                const double xv = (double)sx[ch][oy + HALO][ox + HALO], yv = (double)sy[ch][oy + HALO][ox + HALO];
                g = cv[0] + 2.0 * xv * cv[1] + yv * cv[2];
            }
            __syncthreads();                                // hb and mt are rewritten by the next channel
        }
        const double d = (double)sx[ch][oy + HALO][ox + HALO] - (double)sy[ch][oy + HALO][ox + HALO];
        if (own_in) {
            s1 += fabs(d);
            s2 += d * d;
            sm += m_own;
        }
        if (WITH_COT) {
            const double sgn = d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : 0.0;
            ost[tid * 3 + ch] = (float)((lw.c_l1 * sgn + lw.c_mse * d) - lw.c_ssim * g);
        }
    }

    if (WITH_COT) {
        __syncthreads();
        float* __restrict__ out = cot + (size_t)b * plane;
        for (int i = tid; i < T * T * 3; i += kLossThreads) {
            const int r = i / (T * 3), q = i % (T * 3);
            const int gy = ty0 + r, gx = tx0 + q / 3;
            if (gy < H && gx < W) out[((size_t)gy * W + gx) * 3 + q % 3] = ost[i];
        }
    }

    // the tile's three sums: a fixed tree over the 256 threads
    hb[tid * 3 + 0] = s1;
    hb[tid * 3 + 1] = s2;
    hb[tid * 3 + 2] = sm;
    __syncthreads();
    for (int st = kLossThreads / 2; st > 0; st >>= 1) {
        if (tid < st) {
            hb[tid * 3 + 0] += hb[(tid + st) * 3 + 0];
            hb[tid * 3 + 1] += hb[(tid + st) * 3 + 1];
            hb[tid * 3 + 2] += hb[(tid + st) * 3 + 2];
        }
        __syncthreads();
    }
    if (tid < 3) partials[((size_t)b * nTiles + t) * 3 + tid] = hb[tid];
}

// One wave per candidate: lane l adds the tiles l, l + 64, ... in ascending order, lane 0
// then adds the 64 lane sums in ascending lane order; the weights and 1 / (3 H W) in
// float64, loss[b] rounded to float32 once.
__global__ __launch_bounds__(64) void image_loss_finalize_kernel(const double* __restrict__ partials, int nTiles,
                                                                 double w_l1, double w_mse, double w_ssim, double n,
                                                                 float* __restrict__ loss) {
    __shared__ double ls[64][3];
    const int lane = threadIdx.x;
    const double* __restrict__ p = partials + (size_t)blockIdx.x * nTiles * 3;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll 2
    for (int t = lane; t < nTiles; t += 64) {
        a0 += p[(size_t)t * 3 + 0];
        a1 += p[(size_t)t * 3 + 1];
        a2 += p[(size_t)t * 3 + 2];
    }
    ls[lane][0] = a0;
    ls[lane][1] = a1;
    ls[lane][2] = a2;
    __syncthreads();
    if (lane == 0) {
        double s1 = 0.0, s2 = 0.0, sm = 0.0;
#pragma unroll 1
        for (int l = 0; l < 64; ++l) {
            s1 += ls[l][0];
            s2 += ls[l][1];
            sm += ls[l][2];
        }
        // w_ssim == 0: the tiles formed no m (sm = 0) and the term is a zero either way
        const double v = (w_l1 * s1 + w_mse * s2) / n + (w_ssim != 0.0 ? w_ssim * (1.0 - sm / n) : 0.0);
        loss[blockIdx.x] = (float)v;
    }
}

const LossTaps& loss_taps() {
    static const LossTaps taps = [] {
        LossTaps t;
        double sum = 0.0;
        for (int i = 0; i < kLossTaps; ++i) {
            const double d = (double)(i - kLossRad);
            t.w[i] = exp(-(d * d) / 4.5);
            sum += t.w[i];
        }
        for (int i = 0; i < kLossTaps; ++i) t.w[i] /= sum;
        return t;
    }();
    return taps;
}

}  // namespace

int64_t image_loss_tiles(int H, int W) {
    return (int64_t)((H + kLossTile - 1) / kLossTile) * ((W + kLossTile - 1) / kLossTile);
}

size_t image_loss_partial_bytes(int64_t B, int H, int W) {
    return sizeof(double) * 3 * (size_t)B * (size_t)image_loss_tiles(H, W);
}

hipError_t launch_image_loss(hipStream_t st, const float* img, int64_t B, const float* targets, int group, int H, int W,
                             const float w[3], void* partials, float* loss, float* cot) {
    const int nTX = (W + kLossTile - 1) / kLossTile;
    const int nTiles = (int)image_loss_tiles(H, W);
    const double n = 3.0 * (double)H * (double)W;
    LossWeights lw;
    lw.c_l1 = (double)w[0] / n;
    lw.c_mse = 2.0 * (double)w[1] / n;
    lw.c_ssim = (double)w[2] / n;
    const dim3 grid((unsigned)(B * nTiles));
    if (cot)
        hipLaunchKernelGGL(image_loss_kernel<true>, grid, dim3(kLossThreads), 0, st, img, targets, group, H, W, nTX,
                           nTiles, loss_taps(), lw, (double*)partials, cot);
    else
        hipLaunchKernelGGL(image_loss_kernel<false>, grid, dim3(kLossThreads), 0, st, img, targets, group, H, W, nTX,
                           nTiles, loss_taps(), lw, (double*)partials, (float*)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(image_loss_finalize_kernel, dim3((unsigned)B), dim3(64), 0, st, (const double*)partials, nTiles,
                       (double)w[0], (double)w[1], (double)w[2], n, loss);
    return hipGetLastError();
}

}  // namespace ggs
