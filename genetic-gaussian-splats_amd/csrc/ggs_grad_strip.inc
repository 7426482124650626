// The body of the gradient's two strip kernels (ggs_grad.hip), included inside each:
// one wave's (candidate, strip).  It reads the kernel's names lane, bl, strip, f9,
// i4, S, b0, N, H, W, target, mask, mode, beta, wsum, nSX, nStrips and part.  Kept as
// text, not as a __device__ function: inlined through a function the same statements
// are vectorised differently and grad_strip_kernel grows from 144 to 152 VGPRs
// (DESIGN §8d), and its code object is pinned (tests/test_kernel_resources_grad.py).
// With GGS_STRIP_VJP defined it is vjp_strip_kernel's body (DESIGN §8e): g is read
// from the cotangent cot [B][H][W][3] instead of being built from target, mask and
// mode, and the background is the kernel's bg0, bg1, bg2 instead of white.
    const int sx = strip % nSX, sy = strip / nSX;
    const int64_t base = (b0 + bl) * (int64_t)N;
    const int X = sx * GS_W + (lane & 15);
    const int Y0 = sy * GS_H + (lane >> 4);
    const float xf = (float)X;
    const int nC = (N + 63) / 64;

    // ---- sweep 1: the unclipped final colour ---------------------------------
    float cr[GPL], cg[GPL], cb[GPL];
#ifdef GGS_STRIP_VJP
#pragma unroll
    for (int j = 0; j < GPL; ++j) {                                  // the caller's background
        cr[j] = bg0;
        cg[j] = bg1;
        cb[j] = bg2;
    }
#else
#pragma unroll
    for (int j = 0; j < GPL; ++j) cr[j] = cg[j] = cb[j] = 1.0f;     // fitness.py:15: white background
#endif
    canvas_upto(f9, i4, S, base, N, N, lane, sx, sy, X, Y0, cr, cg, cb);

#ifdef GGS_STRIP_VJP
    // ---- g = the cotangent per channel (0 where the image clip is active), S = g . Cf ----
    const float* __restrict__ V = cot + (b0 + bl) * ((int64_t)H * W * 3);
    float T[GPL], Sg[GPL], gr[GPL], gg[GPL], gb[GPL];
#pragma unroll
    for (int j = 0; j < GPL; ++j) {
        const int y = Y0 + 4 * j;
        float r = 0.0f, g = 0.0f, b = 0.0f;
        if (X < W && y < H) {
            const int64_t p = (int64_t)y * W + X;
            r = (cr[j] >= 0.0f && cr[j] <= 1.0f) ? V[3 * p + 0] : 0.0f;
            g = (cg[j] >= 0.0f && cg[j] <= 1.0f) ? V[3 * p + 1] : 0.0f;
            b = (cb[j] >= 0.0f && cb[j] <= 1.0f) ? V[3 * p + 2] : 0.0f;
        }
        gr[j] = r;
        gg[j] = g;
        gb[j] = b;
        Sg[j] = (r * cr[j] + g * cg[j]) + b * cb[j];
        T[j] = 1.0f;
    }
#else
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
#endif

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
#ifdef GGS_STRIP_VJP
#pragma unroll
                for (int j = 0; j < GPL; ++j) u[j] = (gr[j] * bg0 + gg[j] * bg1) + opaque(gb[j]) * bg2;
#else
#pragma unroll
                for (int j = 0; j < GPL; ++j) u[j] = (gr[j] + gg[j]) + opaque(gb[j]);
#endif
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
