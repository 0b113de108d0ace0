// The window geometry of a tile (csrc/ssf_tile_geometry.hpp) on the CPU.  Built with -fsanitize=address,undefined by
// tests/test_tile_geometry.py.  The reference is the text the header replaced: tile_window_cells_max and pass_geometry_table as
// they stood in ssf_extract.hip at commit 8c714be, each with its own cell_of (only SegParams and uint2 are stand-ins here).
// Every table entry and the maximum must agree bit for bit, for shapes that cover margins of 2, 1 and 0 cells, windows of 36, 64
// and "none" (65), pass tiles without a window, and the pixel-less last column of the OX = 1 grid when W is a multiple of 32.
// The plane filter's windows (pf_window) have the reference's graph itself as their reference, walked breadth first, and its launch
// plan (pf_plan) the limits of a workgroup: see check_plane_filter.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>
#include "../../supersurfel_fusion_amd/csrc/ssf_tile_geometry.hpp"

static_assert(TILE == 32 && WIN_MAX == 64, "the reference below was written for these");
static_assert(sizeof(ssf::PassGeomEntry) == 8 && alignof(ssf::PassGeomEntry) == 8, "one 8-byte scalar load per tile");

namespace ref {          // ---- ssf_extract.hip at 8c714be ---------------------------------------------------------------------------
struct uint2 { uint32_t x, y; };
struct SegParams { int W, H; uint32_t cell_magic; };
int tile_window_cells_max(const SegParams& p) {
    auto cell_of = [&](int x) { return p.cell_magic ? (int)(((uint64_t)(uint32_t)x * p.cell_magic) >> 32) : x; };
    int best = 0;
    for (int Y0 = 0; Y0 < p.H; Y0 += TILE)
        for (int X0 = 0; X0 < p.W; X0 += TILE) {
            int margin = 2;
            const int tcx0 = cell_of(X0), tcy0 = cell_of(Y0), tcx1 = cell_of(std::min(X0 + TILE - 1, p.W - 1)), tcy1 = cell_of(std::min(Y0 + TILE - 1, p.H - 1));
            while (margin > 0 && (tcx1 - tcx0 + 1 + 2 * margin) * (tcy1 - tcy0 + 1 + 2 * margin) > WIN_MAX) margin--;
            const int n = (tcx1 - tcx0 + 1 + 2 * margin) * (tcy1 - tcy0 + 1 + 2 * margin);
            best = std::max(best, n <= WIN_MAX ? n : WIN_MAX + 1);          // (no window at all: the large instantiation, which then takes the exact path)
        }
    return best;
}
int pass_geometry_entries(int W, int H) { return 2 * ((W + (TILE - 2) + TILE - 1) / TILE) * ((H + TILE - 1) / TILE); }
void pass_geometry_table(const SegParams& p, uint2* out) {
    const int ntx = (p.W + (TILE - 2) + TILE - 1) / TILE, nty = (p.H + TILE - 1) / TILE;
    auto cell_of = [&](int x) { return p.cell_magic ? (int)(((uint64_t)(uint32_t)x * p.cell_magic) >> 32) : x; };
    for (int ox = 0; ox < 2; ox++)
        for (int by = 0; by < nty; by++)
            for (int bx = 0; bx < ntx; bx++) {
                const int X0 = bx * TILE - (ox ? 0 : TILE - 2), Y0 = by * TILE;
                const int TWP1 = TILE + 4;
                const bool interior = X0 >= 1 && X0 - 1 + TWP1 <= p.W && Y0 >= 1 && Y0 + TILE < p.H;
                int margin = 2;
                const int tcx0 = cell_of(std::max(X0, 0)), tcy0 = cell_of(Y0);
                const int tcx1 = cell_of(std::min(X0 + TILE - 1, p.W - 1)), tcy1 = cell_of(std::min(Y0 + TILE - 1, p.H - 1));
                while (margin > 0 && (tcx1 - tcx0 + 1 + 2 * margin) * (tcy1 - tcy0 + 1 + 2 * margin) > WIN_MAX) margin--;
                const int nwx = tcx1 - tcx0 + 1 + 2 * margin, nwy = tcy1 - tcy0 + 1 + 2 * margin;
                const bool ok = nwx * nwy <= WIN_MAX && nwx < 256 && nwy < 256;
                uint2 e;
                e.x = ((uint32_t)(tcx0 - margin) & 0xFFFFu) | ((uint32_t)(tcy0 - margin) << 16);
                e.y = (ok ? (uint32_t)nwx | ((uint32_t)nwy << 8) : 0u) | (interior ? 1u << 16 : 0u);
                out[(size_t)ox * ntx * nty + (size_t)by * ntx + bx] = e;
            }
}
}  // namespace ref

static int failures = 0;
#define EXPECT(cond)                                                                                       \
    do {                                                                                                   \
        if (!(cond)) { std::printf("%dx%d cell %d: line %d: %s\n", W, H, cell, __LINE__, #cond); failures++; } \
    } while (0)

static uint32_t magic_of(int cell) { return cell > 1 ? (uint32_t)((0x100000000ull + (uint64_t)cell - 1) / (uint64_t)cell) : 0u; }   // (ssf_create)

// what the shapes are there to cover, gathered over all of them
static std::set<int> seen_max, seen_margin, seen_no_window;
static int interior_min = 1 << 30, interior_max = -1, pixelless_columns = 0;

static void check(int W, int H, int cell) {
    const uint32_t magic = magic_of(cell);
    const ref::SegParams p{W, H, magic};
    const int want_max = ref::tile_window_cells_max(p), got_max = ssf::tile_window_cells_max(W, H, magic);
    EXPECT(got_max == want_max);
    seen_max.insert(want_max);
    const int ne = ref::pass_geometry_entries(W, H);
    EXPECT(ssf::pass_geometry_entries(W, H) == ne);
    // the log regions of a frame are sized by entries / 2: the tile ids by * ntx + bx of the grid launch_update_pass launches, counted
    // here tile by tile -- a column for every tile origin bx * TILE - (TILE - 2) left of the image's right edge, a row likewise
    int ntx = 0, nty = 0;
    while (ntx * TILE - (TILE - 2) < W) ntx++;
    while (nty * TILE < H) nty++;
    EXPECT(ssf::pass_grid_columns(W) == ntx && ssf::pass_grid_rows(H) == nty);
    EXPECT(ne / 2 == ntx * nty && ne % 2 == 0);
    std::vector<ref::uint2> want((size_t)ne + 1, ref::uint2{0xDEADBEEFu, 0xDEADBEEFu});
    std::vector<ssf::PassGeomEntry> got((size_t)ne + 1, ssf::PassGeomEntry{0xDEADBEEFu, 0xDEADBEEFu});
    ref::pass_geometry_table(p, want.data());
    ssf::pass_geometry_table(W, H, magic, got.data());
    int bad = 0, no_window = 0, interior = 0;
    for (int i = 0; i <= ne; i++) {                          // (entry ne: written by neither)
        if (got[i].x != want[i].x || got[i].y != want[i].y) {
            if (bad++ < 5) std::printf("%dx%d cell %d: entry %d: %08x %08x, want %08x %08x\n", W, H, cell, i, got[i].x, got[i].y, want[i].x, want[i].y);
        }
        if (i == ne) break;
        if ((want[i].y & 0xFFFFu) == 0u) no_window++;
        interior += (int)((want[i].y >> 16) & 1u);
        // the margin the entry was built with: its width less the tile's own cells
        const int bx = (i % (ne / 2)) % ntx, ox = i / (ne / 2);
        const int X0 = bx * TILE - (ox ? 0 : TILE - 2);
        const int tcx0 = ssf::cell_of_pixel(magic, std::max(X0, 0)), tcx1 = ssf::cell_of_pixel(magic, std::min(X0 + TILE - 1, W - 1));
        if ((want[i].y & 0xFFu) != 0u) seen_margin.insert(((int)(want[i].y & 0xFFu) - (tcx1 - tcx0 + 1)) / 2);
        if (ox == 1 && std::min(X0 + TILE - 1, W - 1) < X0) pixelless_columns++;
    }
    EXPECT(bad == 0);
    seen_no_window.insert(no_window);
    interior_min = std::min(interior_min, interior); interior_max = std::max(interior_max, interior);
}

// ---- the plane filter's windows and launch plan (PfWindow, pf_window, pf_plan) -------------------------------------------------------
// The reference is the graph itself, walked breadth first without pf_window: from the core nodes of a tile follow, for F steps, the
// reads of TPS_RGBD::filter -- the four neighbours under its rule (`x < gx` where `xx < gx` was meant: the right-hand neighbour of a
// node in the last column is node (0, y + 1); the read of node S is skipped).  Everything reached must have a slot of its own in
// [0, n1 + n2), or a workgroup's core would read a node it does not hold.
static long pf_windows_walked = 0, pf_nodes_reached = 0;
#define PF_EXPECT(cond)                                                                                                           \
    do {                                                                                                                          \
        if (!(cond)) { if (failures++ < 20) std::printf("grid %dx%d F %d tile (%d, %d): line %d: %s\n", gx, gy, F, tx, ty, __LINE__, #cond); } \
    } while (0)

static void pf_walk_tile(int gx, int gy, int F, int tx, int ty, std::vector<int>& seen, int& stamp) {
    const int S = gx * gy;
    const ssf::PfWindow wd = ssf::pf_window(gx, gy, tx, ty, F);
    const int nn = wd.n1 + wd.n2;
    PF_EXPECT(wd.n1 > 0 && wd.n2 >= 0);
    std::vector<int> owner((size_t)std::max(nn, 1), -1), frontier, next;
    stamp++;
    for (int y = ty * PF_TY; y < std::min(ty * PF_TY + PF_TY, gy); y++)
        for (int x = tx * PF_TX; x < std::min(tx * PF_TX + PF_TX, gx); x++) { seen[(size_t)y * gx + x] = stamp; frontier.push_back(y * gx + x); }
    PF_EXPECT(!frontier.empty());
    for (int d = 0; d <= F; d++) {
        next.clear();
        for (int node : frontier) {
            const int x = node % gx, y = node / gx;
            const int s = wd.slot(x, y);
            PF_EXPECT(s >= 0 && s < nn);
            if (s >= 0 && s < nn) {
                PF_EXPECT(owner[s] < 0);                               // no two nodes share a slot
                owner[s] = node;
                int bx = -1, by = -1;
                wd.node(s, bx, by);
                PF_EXPECT(bx == x && by == y);                         // ... and the kernel's thread for the slot finds the node
            }
            pf_nodes_reached++;
            if (d == F) continue;
            const int v[4] = {-1, 0, 0, 1}, u[4] = {0, -1, 1, 0};
            for (int j = 0; j < 4; j++) {
                const int yy = y + v[j], xx = x + u[j];
                if (!(yy >= 0 && yy < gy && xx >= 0 && x < gx)) continue;
                const int nidx = yy * gx + xx;
                if (nidx >= S || seen[nidx] == stamp) continue;
                seen[nidx] = stamp; next.push_back(nidx);
            }
        }
        frontier.swap(next);
    }
    pf_windows_walked++;
}

// the plan of a grid: what the launcher will ask the device for
static ssf::PfPlan pf_check_grid(int gx, int gy, int F, std::vector<int>& seen, int& stamp) {
    const int S = gx * gy, tx = -1, ty = -1;
    if ((int)seen.size() < S) seen.assign((size_t)S, 0);
    const int ntx = (gx + PF_TX - 1) / PF_TX, nty = (gy + PF_TY - 1) / PF_TY;
    int worst = 0;
    for (int b = 0; b < nty; b++)
        for (int a = 0; a < ntx; a++) {
            pf_walk_tile(gx, gy, F, a, b, seen, stamp);
            const ssf::PfWindow wd = ssf::pf_window(gx, gy, a, b, F);
            worst = std::max(worst, wd.n1 + wd.n2);
        }
    for (int granted = 0; granted < 2; granted++) {
        const ssf::PfPlan pl = ssf::pf_plan(gx, gy, F, granted != 0);
        PF_EXPECT(pl.threads > 0 && pl.threads <= 1024 && pl.threads % 64 == 0);
        PF_EXPECT(pl.big_lds == (pl.lds > (size_t)64 * 1024) && (granted || !pl.big_lds) && pl.lds <= (size_t)160 * 1024);
        if (pl.form == ssf::PF_TILED) {
            PF_EXPECT(worst <= 1024 && pl.window == worst && pl.npt == 1 && pl.ntx == ntx && pl.nty == nty);
        } else {
            PF_EXPECT(worst > 1024 && pl.ntx == 1 && pl.nty == 1 && pl.threads == 1024);
            if (pl.form == ssf::PF_WHOLE) {
                PF_EXPECT(S <= 5120 && pl.window == S && (pl.npt == 2 || pl.npt == 3 || pl.npt == 5));
                PF_EXPECT(pl.npt == 2 || 1024 * (pl.npt == 3 ? 2 : 3) < S);                    // the smallest that covers the grid
            } else {
                PF_EXPECT(pl.form == ssf::PF_GLOBAL && pl.window == 0 && (S > 5120 || (!granted && S > 2048)));
            }
        }
        PF_EXPECT(pl.window <= pl.threads * std::max(pl.npt, 1) && pl.lds == (size_t)32 * pl.window);
    }
    if (S <= 5120) {                                         // the whole grid as one window: slot = node index, and back
        const ssf::PfWindow wg = ssf::pf_whole_grid(gx, gy);
        PF_EXPECT(wg.n1 == S && wg.n2 == 0);
        for (int s = 0; s < S; s += (s < 2 * gx || s > S - 2 * gx) ? 1 : 7) {
            int x = -1, y = -1;
            wg.node(s, x, y);
            PF_EXPECT(x == s % gx && y == s / gx && wg.slot(x, y) == s);
        }
        PF_EXPECT(wg.slot(gx, 0) == -1 && wg.slot(0, gy) == -1 && wg.slot(-1, 0) == -1);
    }
    return ssf::pf_plan(gx, gy, F);
}

static void check_plane_filter() {
    std::vector<int> seen;
    int stamp = 0;
    for (int gy = 1; gy <= 30; gy++)
        for (int gx = 1; gx <= 48; gx++)
            for (int F = 0; F <= 10; F++) pf_check_grid(gx, gy, F, seen, stamp);
    // the forms of the shapes the GPU suite and the benchmark run (cell-16 grids; 10 x 8 is 160 x 128)
    struct Want { int gx, gy, F; ssf::PfForm form; int npt, window; };
    // 40 x 30 at F = 9 is NOT tiled: its middle tile's window runs into the last column (33 x 27 = 891 nodes) and takes the second
    // rectangle (7 x 26 = 182): 1073 nodes.  1020 = 34 x 30 is an interior window clipped by nothing, which a grid 40 wide cannot hold.
    // The two sides of the 1024-node boundary are F = 7 (750: no window reaches the last column yet) and F = 8 (1032) in this grid, and
    // F = 9 (1020) and F = 10 (1152) in 80 x 60, which has interior tiles.
    const Want table[] = {{10, 8, 4, ssf::PF_TILED, 1, 80},      {40, 30, 3, ssf::PF_TILED, 1, 0},      {40, 30, 7, ssf::PF_TILED, 1, 750},
                          {40, 30, 8, ssf::PF_WHOLE, 2, 1200},   {40, 30, 9, ssf::PF_WHOLE, 2, 1200},   {40, 30, 10, ssf::PF_WHOLE, 2, 1200},
                          {64, 32, 12, ssf::PF_WHOLE, 2, 2048},  {54, 40, 12, ssf::PF_WHOLE, 3, 2160},  {80, 60, 12, ssf::PF_WHOLE, 5, 4800},
                          {120, 90, 12, ssf::PF_GLOBAL, 0, 0},   {80, 60, 3, ssf::PF_TILED, 1, 0},      {80, 60, 9, ssf::PF_TILED, 1, 1020},
                          {80, 60, 10, ssf::PF_WHOLE, 5, 4800}};
    for (const Want& w : table) {
        const int gx = w.gx, gy = w.gy, tx = -1, ty = -1;
        for (int F = 0; F <= 13; F++) {
            const ssf::PfPlan pl = pf_check_grid(gx, gy, F, seen, stamp);
            if (F != w.F) continue;
            PF_EXPECT(pl.form == w.form && pl.npt == w.npt);
            PF_EXPECT(w.window == 0 || pl.window == w.window);
            PF_EXPECT(w.form != ssf::PF_TILED || (pl.ntx * pl.nty == 1) == (gx <= PF_TX && gy <= PF_TY));
        }
    }
    {   // 40 x 30: the largest window by the number of sweeps, on both sides of a 1024-thread workgroup
        const int gx = 40, gy = 30, tx = -1, ty = -1, F = 0;
        int worst[4] = {0, 0, 0, 0};
        for (int f = 7; f <= 10; f++)
            for (int b = 0; b < 3; b++)
                for (int a = 0; a < 3; a++) { const ssf::PfWindow wd = ssf::pf_window(gx, gy, a, b, f); worst[f - 7] = std::max(worst[f - 7], wd.n1 + wd.n2); }
        PF_EXPECT(worst[0] == 750 && worst[1] == 1032 && worst[2] == 1073 && worst[3] == 1114);
        // an interior window that nothing clips is (16 + 2 F) x (12 + 2 F): 1020 at F = 9, 1152 at F = 10 (80 x 60, tile (2, 2))
        const ssf::PfWindow w9 = ssf::pf_window(80, 60, 2, 2, 9), w10 = ssf::pf_window(80, 60, 2, 2, 10);
        PF_EXPECT(w9.n1 == 1020 && w9.n2 == 0 && w10.n1 == 1152 && w10.n2 == 0);
        PF_EXPECT(!ssf::pf_plan(64, 32, 12).big_lds && ssf::pf_plan(64, 32, 12).lds == (size_t)64 * 1024);
        PF_EXPECT(ssf::pf_plan(54, 40, 12).big_lds && ssf::pf_plan(54, 40, 12, false).form == ssf::PF_GLOBAL);
    }
    std::printf("plane filter: %ld windows walked, %ld nodes reached\n", pf_windows_walked, pf_nodes_reached);
}

int main() {
    check_plane_filter();
    int W = 0, H = 0, cell = 0;
    // x / cell by the magic multiply, for every pixel coordinate the stage admits
    for (int c : {1, 2, 3, 4, 5, 7, 8, 12, 16, 24, 32, 48, 64}) {
        cell = c;
        int mismatches = 0;
        for (int x = 0; x < 65536; x++) mismatches += ssf::cell_of_pixel(magic_of(c), x) != x / c;
        EXPECT(mismatches == 0);
    }
    const int shapes[][3] = {{640, 480, 16}, {1280, 960, 16}, {160, 128, 16}, {170, 130, 16}, {33, 31, 16}, {160, 128, 24}, {160, 128, 8}, {160, 128, 5},
                             {160, 128, 4}, {96, 64, 1}};
    for (const auto& s : shapes) check(s[0], s[1], s[2]);
    // the shapes cover what they were chosen for
    EXPECT((seen_max == std::set<int>{36, 64, 65}));
    EXPECT((seen_margin == std::set<int>{0, 1, 2}));
    EXPECT(seen_no_window.count(0) && seen_no_window.count(12) && seen_no_window.count(16));
    EXPECT(interior_min == 0 && interior_max == 2156);
    EXPECT(pixelless_columns > 0);
    if (failures) { std::printf("tile_geometry_smoke: %d failures\n", failures); return 1; }
    std::printf("tile_geometry_smoke ok\n");
    return 0;
}
