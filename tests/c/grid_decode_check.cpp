// Host check of the strip-words raster's launch descriptor (csrc/ggs_internal.h):
// the multiply-shift constants against / and %, the grid decode against the
// raster's dividing prologue restated below, and the strip table's entries against
// its (tx0, ty0, wv) formulas.  Built and run by tests/test_grid_decode.py; prints
// "ok <checks>" and exits 0, or the first mismatch and 1.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "ggs_internal.h"

using namespace ggs;

static std::atomic<unsigned long long> g_checks{0};

static bool check_div(uint32_t d, GridDiv g, uint32_t n) {
    const uint32_t q = grid_div(n, g), r = n - q * d;
    if (q == n / d && r == n % d) return true;
    std::printf("divisor %u dividend %u: quotient %u remainder %u (mul %u shift %u)\n", d, n, q, r, g.mul, g.shift);
    return false;
}

// one divisor: every dividend up to 2^20, 2^31 - 1, and multiples +- 1
static bool division(uint32_t d) {
    const uint32_t top = 0x7FFFFFFFu;
    GridDiv g;
    if (!grid_div_make(d, top, &g)) { std::printf("no constant for divisor %u\n", d); return false; }
    uint32_t q = 0, r = 0;                     // n / d and n % d, counted up
    for (uint32_t n = 0; n <= (1u << 20); ++n) {
        if (grid_div(n, g) != q) return check_div(d, g, n);
        if (++r == d) { r = 0; ++q; }
    }
    if (!check_div(d, g, top)) return false;
    // multiples k d and k d +- 1: the first 64, powers of two times d, the last 64 below 2^31
    std::vector<uint64_t> ks;
    for (uint64_t k = 1; k <= 64; ++k) ks.push_back(k);
    for (uint64_t k = 64; k * d <= top; k *= 2) ks.push_back(k);
    for (uint64_t j = 0; j < 64 && j < top / d; ++j) ks.push_back(top / d - j);
    for (uint64_t k : ks)
        for (int64_t o = -1; o <= 1; ++o) {
            const int64_t n = (int64_t)(k * d) + o;
            if (n >= 0 && n <= (int64_t)top && !check_div(d, g, (uint32_t)n)) return false;
        }
    // a constant built for a launch-sized bound is exact up to that bound
    GridDiv s;
    const uint32_t lim = 65535u + d;
    if (!grid_div_make(d, lim, &s)) { std::printf("no constant for divisor %u up to %u\n", d, lim); return false; }
    for (uint32_t n = 0; n <= lim; ++n)
        if (!check_div(d, s, n)) return false;
    g_checks += (1u << 20) + 2 + 3 * ks.size() + lim + 1;    // (the thread's count, added once)
    return true;
}

// every divisor 1 .. 4096, four threads taking them in turn
static bool divisions() {
    std::atomic<bool> ok{true};
    std::vector<std::thread> th;
    for (uint32_t w = 0; w < 4; ++w)
        th.emplace_back([&ok, w] {
            for (uint32_t d = 1 + w; d <= 4096 && ok; d += 4)
                if (!division(d)) ok = false;
        });
    for (auto& t : th) t.join();
    return ok;
}

// the raster's prologue as it divides on the device (raster_body, the instances
// without the saturation check: candidates rotate by one per group)
static void decode_by_division(int idx, int B, int nTiles, int CH, int simds, int* b, int* gi) {
    const int SPB = 4;
    int b0 = 0, Bc = B;
    if (simds > 0) {
        const int n = B * nTiles * SPB;
        if (n > 2 * simds && n <= 3 * simds && idx >= simds && idx < 2 * simds) idx = 3 * simds - 1 - idx;
    }
    if (B > CH) {
        const int per = CH * nTiles * SPB;
        const int c = idx / per;
        idx -= c * per;
        b0 = c * CH;
        Bc = CH < B - b0 ? CH : B - b0;
    }
    *gi = idx / Bc;
    *b = b0 + (idx + *gi) % Bc;
}

static bool grids() {
    const int tiles[] = {2, 3, 6, 32, 1, 7};               // the test canvases', one tile, an odd count
    const int Bs[] = {1, 2, 3, 9, 20, 127, 128, 1032};
    const int CHs[] = {8, 16, 1024, 2048, 8192};           // small chunks too: several full ones and a ragged last
    const int simdss[] = {0, 1024, 96, 37};
    for (int nTiles : tiles)
        for (int B : Bs)
            for (int CH : CHs)
                for (int simds : simdss) {
                    StripLaunch d;
                    if (!strip_launch_grid(B, nTiles, CH, simds, &d)) {
                        std::printf("no descriptor for B %d nTiles %d CH %d simds %d\n", B, nTiles, CH, simds);
                        return false;
                    }
                    const int grid = B * nTiles * 4;
                    g_checks += grid;
                    for (int i = 0; i < grid; ++i) {
                        int b, gi;
                        decode_by_division(i, B, nTiles, CH, simds, &b, &gi);
                        const StripBlock s = strip_launch_block(d, (uint32_t)i);
                        if ((int)s.b != b || (int)s.group != gi) {
                            std::printf("B %d nTiles %d CH %d simds %d block %d: (%u, %u), the divisions give (%d, %d)\n",
                                        B, nTiles, CH, simds, i, s.b, s.group, b, gi);
                            return false;
                        }
                    }
                }
    // a grid the descriptor refuses: 2^31 blocks
    StripLaunch d;
    if (strip_launch_grid((int64_t)1 << 24, 32, 1 << 24, 1024, &d)) {
        std::printf("a grid of 2^31 blocks was accepted\n");
        return false;
    }
    return true;
}

// every table entry of the test canvases: (tx0, ty0, wv) of the raster's formulas
static bool tables() {
    const int TILE = 64, TILE_H = 128, SPB = 4;
    const int canvases[][2] = {{64, 128}, {70, 130}, {200, 136}, {512, 512}, {2048, 2048}, {33, 47}};
    for (const auto& c : canvases) {
        const int H = c[0], W = c[1], nTX = (W + TILE - 1) / TILE, nTY = (H + TILE_H - 1) / TILE_H;
        for (int grp = 0; grp < nTX * nTY * SPB; ++grp) {
            const int t = grp / SPB, wv = grp % SPB;
            const int tx0 = (t % nTX) * TILE, ty0 = (t / nTX) * TILE_H;
            int e = -1;
            ++g_checks;
            if (!strip_table_entry(grp, nTX, &e)) { std::printf("%dx%d group %d: no entry\n", H, W, grp); return false; }
            const int cs = strip_entry_column(e), ty = strip_entry_row(e);
            if ((cs & 3) != wv || (cs >> 2) * TILE != tx0 || ty * TILE_H != ty0 || cs * 16 != tx0 + wv * 16 ||
                ty * (nTX * 4) + cs != t * 4 + wv) {
                std::printf("%dx%d group %d: entry %#x decodes to column strip %d, row tile %d\n", H, W, grp, e, cs, ty);
                return false;
            }
        }
    }
    int e;
    if (strip_table_entry(4 * 16384, 1 << 20, &e)) {     // column strip 65536 does not fit
        std::printf("an entry past the column field was accepted\n");
        return false;
    }
    return true;
}

int main() {
    if (!divisions() || !grids() || !tables()) return 1;
    std::printf("ok %llu\n", g_checks.load());
    return 0;
}
