// Residual-driven placement: where a render misses its target, and the
// splat to put there.  ggs/seed.py cell_grid / place_sites state all of it in numpy;
// the kernels are held to them bit for bit.
//   seed_cell_kernel    a wave covers 64 pixel columns of one cell row, 64 / c cells.
//                       A lane owns one column and walks the cell's c pixel rows (the
//                       loads of a row are contiguous across lanes), keeping the
//                       column's residual, its three target sums and its largest
//                       residual with the row it was on; a lane xor-butterfly over the
//                       cell's c lanes (strides 1, 2, 4, ...: the balanced tree
//                       v[0::2] + v[1::2] of the statement) gives every lane the
//                       cell's sums and peak, and the cell's first lane writes them
//   seed_rank_kernel    one thread per (candidate, cell): ranks its cell among the
//                       eligible ones by counting smaller 64-bit keys, tiled through
//                       LDS, and writes the first max_sites cells
//   seed_apply_kernel   one thread per (candidate, site slot j < M): the row, the site
//                       log and n
// Float32, one rounding per operation (-ffp-contract=off), division correctly rounded.
// The only atomics are integer counters; every index is bounded before it is used.
#include <hip/hip_runtime.h>

#include "ggs_detmath.h"
#include "ggs_internal.h"

namespace ggs {
namespace {

using namespace detmath;

constexpr int ST = 256;            // threads per workgroup; the rank kernel's tile

struct SeedCellDev {
    int B, H, W, c, Gy, Gx, WX;    // WX = ceil(W / 64): waves per cell row
    int group;
    float bg0, bg1, bg2;           // the image when img is null
};

// Of two peaks the larger residual, ties to the smaller (y, x).  A lane with no pixel
// of the image holds (-inf, INT_MAX, x), which loses to every pixel.
__device__ __forceinline__ bool peak_before(float e, int y, int x, float oe, int oy, int ox) {
    return e > oe || (e == oe && (y < oy || (y == oy && x < ox)));
}

// grid ceil(B * Gy * WX / 4) workgroups of 4 waves.  err [B][G], sums [B][G] (r, g, b,
// the in-image pixel count's bits), peak [B][G] (y, x); G = Gy * Gx.
__global__ void __launch_bounds__(ST)
seed_cell_kernel(const float* __restrict__ img, const float* __restrict__ targets, const float* __restrict__ weights,
                 SeedCellDev p, float* __restrict__ err, float4* __restrict__ sums, int2* __restrict__ peak) {
    const int lane = (int)threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (ST / 64) + ((int)threadIdx.x >> 6);
    if (wave >= (int64_t)p.B * p.Gy * p.WX) return;          // the whole wave leaves
    const int wx = (int)(wave % p.WX);
    const int gy = (int)((wave / p.WX) % p.Gy);
    const int b = (int)(wave / ((int64_t)p.WX * p.Gy));
    const int x = wx * 64 + lane;
    const int y0 = gy * p.c;
    const bool col = x < p.W;
    const int64_t plane = (int64_t)p.H * p.W;
    const int64_t ib = (int64_t)b * plane, tb = (int64_t)(b / p.group) * plane;
    float s_e = 0.0f, s_r = 0.0f, s_g = 0.0f, s_b = 0.0f;
    float pe = -INFINITY;
    int py = 0x7fffffff, px = x;
    for (int i = 0; i < p.c; ++i) {
        const int y = y0 + i;
        float e = 0.0f, tr = 0.0f, tg = 0.0f, tbl = 0.0f;     // a pixel past the image: +0.0
        const bool in = col && y < p.H;
        if (in) {
            const int64_t o = (int64_t)y * p.W + x;
            const float* __restrict__ t = targets + (tb + o) * 3;
            tr = t[0];
            tg = t[1];
            tbl = t[2];
            float ir = p.bg0, ig = p.bg1, ibl = p.bg2;
            if (img) {
                const float* __restrict__ m = img + (ib + o) * 3;
                ir = m[0];
                ig = m[1];
                ibl = m[2];
            }
            const float dr = ir - tr, dg = ig - tg, db = ibl - tbl;
            e = (dr * dr + dg * dg) + db * db;
            if (weights) e = weights[tb + o] * e;
            if (e > pe) {                                    // rows ascend: a tie keeps the smaller y
                pe = e;
                py = y;
            }
        }
        s_e = s_e + e;
        s_r = s_r + tr;
        s_g = s_g + tg;
        s_b = s_b + tbl;
    }
    // the butterfly: after stride s every lane holds the tree's node over its aligned
    // group of 2 s lanes (a + b and b + a are the same float)
    for (int s = 1; s < p.c; s <<= 1) {
        s_e = s_e + __shfl_xor(s_e, s, 64);
        s_r = s_r + __shfl_xor(s_r, s, 64);
        s_g = s_g + __shfl_xor(s_g, s, 64);
        s_b = s_b + __shfl_xor(s_b, s, 64);
        const float oe = __shfl_xor(pe, s, 64);
        const int oy = __shfl_xor(py, s, 64), ox = __shfl_xor(px, s, 64);
        if (peak_before(oe, oy, ox, pe, py, px)) {
            pe = oe;
            py = oy;
            px = ox;
        }
    }
    const int gx = x / p.c;
    if ((lane & (p.c - 1)) != 0 || gx >= p.Gx) return;       // c is a power of two
    const int64_t cell = (int64_t)b * p.Gy * p.Gx + (int64_t)gy * p.Gx + gx;
    const int count = (min(p.H, y0 + p.c) - y0) * (min(p.W, x + p.c) - x);
    err[cell] = s_e;
    sums[cell] = make_float4(s_r, s_g, s_b, __int_as_float(count));
    peak[cell] = make_int2(py, px);
}

// order-preserving 32-bit key of a float (no NaN reaches it)
__device__ __forceinline__ uint32_t float_key(float f) {
    const uint32_t u = __builtin_bit_cast(uint32_t, f + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// A cell's 64-bit key: the complement of its residual's float key above its index, so
// that keys ascend as the site list does (descending err, ties to the lower cell).  A
// cell that is not eligible (err > err_min is false, a NaN included) has every bit set,
// which is above every eligible key: an index is below 2^31.
__device__ __forceinline__ uint64_t site_key(const float* __restrict__ err, int64_t g0, int g, float err_min) {
    const float e = err[g0 + g];
    if (!(e > err_min)) return ~0ull;
    return ((uint64_t)(~float_key(e)) << 32) | (uint32_t)g;
}

// grid (ceil(G / ST), B).  counts [B] (zero on entry): the eligible cells.
__global__ void __launch_bounds__(ST)
seed_rank_kernel(const float* __restrict__ err, int G, int M, float err_min, int* __restrict__ list,
                 int* __restrict__ counts) {
    __shared__ uint64_t t_key[ST];
    const int b = (int)blockIdx.y;
    const int64_t g0 = (int64_t)b * G;
    const int g = (int)blockIdx.x * ST + (int)threadIdx.x;
    const uint64_t key = g < G ? site_key(err, g0, g, err_min) : ~0ull;
    const bool elig = key != ~0ull;
    int rank = 0;
    for (int t0 = 0; t0 < G; t0 += ST) {
        const int o = t0 + (int)threadIdx.x;
        const uint64_t k = o < G ? site_key(err, g0, o, err_min) : ~0ull;
        __syncthreads();                       // the previous tile has been counted
        t_key[threadIdx.x] = k;
        __syncthreads();
        // the whole tile, branch-free: an entry past G has every bit set, below nobody
        if (elig) {
#pragma unroll 16
            for (int j = 0; j < ST; ++j) rank += (t_key[j] < key) ? 1 : 0;
        }
    }
    // one atomic per wave (every lane is still here)
    const uint64_t lanes = __ballot(elig);
    if ((threadIdx.x & 63) == 0 && lanes) atomicAdd(&counts[b], __popcll(lanes));
    if (elig && rank < M) list[(int64_t)b * M + rank] = g;
}

struct SeedApplyDev {
    int B, N, M, G, first_row;
    float wm, hm;                  // float(max(W - 1, 1)), float(max(H - 1, 1))
    float log_sigma, alpha;
};

__device__ __forceinline__ float clip(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// One thread per (candidate, site slot j < M).  x [B][N][9] (may be null: sites only),
// rows [B][M] (may be null: first_row + j), sites [B][M] = the cell or -1, n_out [B].
__global__ void __launch_bounds__(ST)
seed_apply_kernel(float* __restrict__ x, const int* __restrict__ rows, const int* __restrict__ list,
                  const int* __restrict__ counts, const float4* __restrict__ sums, const int2* __restrict__ peak,
                  SeedApplyDev p, int* __restrict__ sites, int* __restrict__ n_out) {
    const int64_t i = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (i >= (int64_t)p.B * p.M) return;
    const int b = (int)(i / p.M), j = (int)(i % p.M);
    const int n = min(counts[b], p.M);
    if (j == 0) n_out[b] = n;
    if (j >= n) {
        sites[i] = -1;
        return;
    }
    const int g = list[i];
    sites[i] = g;
    if (!x || (unsigned)g >= (unsigned)p.G) return;           // ranks are unique: g is a cell
    const int row = rows ? rows[i] : p.first_row + j;
    if ((unsigned)row >= (unsigned)p.N) return;
    const int64_t cell = (int64_t)b * p.G + g;
    const float4 s = sums[cell];
    const int2 pk = peak[cell];                               // (y, x)
    const float cnt = (float)__float_as_int(s.w);
    float* __restrict__ r = x + ((int64_t)b * p.N + row) * 9;
    r[0] = ggs_div_rn((float)pk.y, p.wm);
    r[1] = ggs_div_rn((float)pk.x, p.hm);
    r[2] = p.log_sigma;
    r[3] = p.log_sigma;
    r[4] = 0.0f;
    r[5] = clip(255.0f * ggs_div_rn(s.x, cnt), 0.0f, 255.0f);
    r[6] = clip(255.0f * ggs_div_rn(s.y, cnt), 0.0f, 255.0f);
    r[7] = clip(255.0f * ggs_div_rn(s.z, cnt), 0.0f, 255.0f);
    r[8] = p.alpha;
}

}  // namespace

size_t seed_scratch_bytes(int B, int H, int W, int cell, int M, bool own_err) {
    const size_t G = (size_t)seed_cells(H, W, cell), n = (size_t)B * G;
    return (own_err ? n * sizeof(float) : 0) + n * sizeof(float4) + n * sizeof(int2) +
           ((size_t)B * M + (size_t)B) * sizeof(int) + 64;
}

hipError_t launch_seed_sites(hipStream_t st, const float* img, const float bg[3], const float* targets,
                             const float* weights, int B, int group, int H, int W, const ggs_seed_params& prm,
                             const int* rows, float* x, int N, void* scratch, float* err, int* sites, int* n_out) {
    const int c = prm.cell, M = prm.max_sites;
    if (B <= 0 || M <= 0) return hipSuccess;
    const int Gy = (H + c - 1) / c, Gx = (W + c - 1) / c, G = Gy * Gx;
    const size_t n = (size_t)B * G;
    // the scratch, 16-byte pieces first: sums, peak, the error grid unless the caller's, list, counts
    char* q = (char*)scratch;
    float4* sums = (float4*)q;
    q += n * sizeof(float4);
    int2* peak = (int2*)q;
    q += n * sizeof(int2);
    if (!err) {
        err = (float*)q;
        q += n * sizeof(float);
    }
    int* list = (int*)q;
    q += (size_t)B * M * sizeof(int);
    int* counts = (int*)q;
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(int) * (size_t)B, st);
    if (e != hipSuccess) return e;
    SeedCellDev cp;
    cp.B = B;
    cp.H = H;
    cp.W = W;
    cp.c = c;
    cp.Gy = Gy;
    cp.Gx = Gx;
    cp.WX = (W + 63) / 64;
    cp.group = group;
    cp.bg0 = bg[0];
    cp.bg1 = bg[1];
    cp.bg2 = bg[2];
    const int64_t waves = (int64_t)B * Gy * cp.WX;
    hipLaunchKernelGGL(seed_cell_kernel, dim3((unsigned)((waves + ST / 64 - 1) / (ST / 64))), dim3(ST), 0, st, img,
                       targets, weights, cp, err, sums, peak);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(seed_rank_kernel, dim3((unsigned)((G + ST - 1) / ST), (unsigned)B), dim3(ST), 0, st, err, G, M,
                       prm.err_min, list, counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    SeedApplyDev ap;
    ap.B = B;
    ap.N = N;
    ap.M = M;
    ap.G = G;
    ap.first_row = prm.first_row;
    ap.wm = (float)(W > 1 ? W - 1 : 1);
    ap.hm = (float)(H > 1 ? H - 1 : 1);
    ap.log_sigma = prm.log_sigma;
    ap.alpha = prm.alpha;
    const int64_t slots = (int64_t)B * M;
    hipLaunchKernelGGL(seed_apply_kernel, dim3((unsigned)((slots + ST - 1) / ST)), dim3(ST), 0, st, x, rows, list,
                       counts, sums, peak, ap, sites, n_out);
    return hipGetLastError();
}

}  // namespace ggs
