// ssf_tile_geometry.hpp -- the window of grid cells around a tile of pixels: the ONE statement of it, for the tile kernels of
// ssf_extract.hip (CellWindow) and for the two host tables a handle is created with (SegParams::win_cells_max, ::pass_geom).
// Also the plane filter's geometry: the window of superpixel-grid nodes around a core tile (PfWindow, pf_window) and the plan that
// says which kernel form a grid takes, with how many workgroups, threads and LDS bytes (pf_plan).
// Only the arithmetic, and no HIP header: tests/cpp/tile_geometry_smoke.cpp runs it on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SSF_GEOM_HD __host__ __device__ __forceinline__
#else
#define SSF_GEOM_HD inline
#endif

#define TILE 32               // tiles are TILE x TILE pixels
#define WIN_MAX 64            // most cells a window may have (the LDS tables of the tile kernels)

namespace ssf {

// x / cell for a pixel coordinate (0 <= x < 65536) without the 20-instruction integer division: the high word of
// x * ceil(2^32 / cell) (SegParams::cell_magic; 0 stands for cell == 1)
SSF_GEOM_HD int cell_of_pixel(uint32_t cell_magic, int x) { return cell_magic ? (int)(((uint64_t)(uint32_t)x * cell_magic) >> 32) : x; }

// The window of a pixel extent [x_first, x_last] x [y_first, y_last]: its cells and a margin of two cells around them, of one, or of
// none -- the widest that keeps the window within `capacity` cells.  ok = it fits; when not even the bare cells do, there is no
// window and every label takes the exact global path.
// (Extents, not a tile origin: the callers differ in how they clamp -- the relabelling passes' shifted grid starts left of the image
// -- and a clamp in here would cost the kernels whose origin needs none a scalar instruction.)
struct TileWindow { int cx0, cy0, nwx, nwy; bool ok; };
SSF_GEOM_HD TileWindow tile_window(uint32_t cell_magic, int x_first, int x_last, int y_first, int y_last, int capacity) {
    int margin = 2;
    const int tcx0 = cell_of_pixel(cell_magic, x_first), tcy0 = cell_of_pixel(cell_magic, y_first);
    const int tcx1 = cell_of_pixel(cell_magic, x_last), tcy1 = cell_of_pixel(cell_magic, y_last);
    while (margin > 0 && (tcx1 - tcx0 + 1 + 2 * margin) * (tcy1 - tcy0 + 1 + 2 * margin) > capacity) margin--;
    TileWindow w;
    w.cx0 = tcx0 - margin; w.cy0 = tcy0 - margin;
    w.nwx = tcx1 - tcx0 + 1 + 2 * margin; w.nwy = tcy1 - tcy0 + 1 + 2 * margin;
    w.ok = w.nwx * w.nwy <= capacity;
    return w;
}

// the largest window of a tile of the plain TILE x TILE grid (the grid of k_eval_samples, k_init_disp, k_render_moments):
// SegParams::win_cells_max.  WIN_MAX + 1: some tile has no window at all (the large instantiations, which then take the exact path)
inline int tile_window_cells_max(int W, int H, uint32_t cell_magic) {
    int best = 0;
    for (int Y0 = 0; Y0 < H; Y0 += TILE)
        for (int X0 = 0; X0 < W; X0 += TILE) {
            const TileWindow w = tile_window(cell_magic, X0, std::min(X0 + TILE - 1, W - 1), Y0, std::min(Y0 + TILE - 1, H - 1), WIN_MAX);
            best = std::max(best, w.ok ? w.nwx * w.nwy : WIN_MAX + 1);
        }
    return best;
}

// The relabelling passes' grid (k_update_pass): for OX = 0 the tiles start at 2 (mod 4), the first one TILE - 2 pixels left of the
// image, and the same -- one column larger -- grid serves OX = 1, so that a tile keeps its id (and its log region) in every pass.
// One entry per tile, [OX = 0 | OX = 1], each half in row-major tile order:
//   x = (first window cell in x & 0xFFFF) | first window cell in y << 16     (may be negative)
//   y = nwx | nwy << 8 | interior << 16       (nwx = nwy = 0: no window; interior: the tile, its halo and the two padding
//                                              columns of its LDS rows lie inside the image)
struct alignas(8) PassGeomEntry { uint32_t x, y; };
inline int pass_grid_columns(int W) { return (W + (TILE - 2) + TILE - 1) / TILE; }
inline int pass_grid_rows(int H) { return (H + TILE - 1) / TILE; }
inline int pass_geometry_entries(int W, int H) { return 2 * pass_grid_columns(W) * pass_grid_rows(H); }
inline void pass_geometry_table(int W, int H, uint32_t cell_magic, PassGeomEntry* out) {
    const int ntx = pass_grid_columns(W), nty = pass_grid_rows(H);
    for (int ox = 0; ox < 2; ox++)
        for (int by = 0; by < nty; by++)
            for (int bx = 0; bx < ntx; bx++) {
                const int X0 = bx * TILE - (ox ? 0 : TILE - 2), Y0 = by * TILE;
                const bool interior = X0 >= 1 && X0 - 1 + TILE + 4 <= W && Y0 >= 1 && Y0 + TILE < H;
                const TileWindow w = tile_window(cell_magic, std::max(X0, 0), std::min(X0 + TILE - 1, W - 1), Y0, std::min(Y0 + TILE - 1, H - 1), WIN_MAX);
                const bool ok = w.ok && w.nwx < 256 && w.nwy < 256;
                PassGeomEntry e;
                e.x = ((uint32_t)w.cx0 & 0xFFFFu) | ((uint32_t)w.cy0 << 16);
                e.y = (ok ? (uint32_t)w.nwx | ((uint32_t)w.nwy << 8) : 0u) | (interior ? 1u << 16 : 0u);
                out[(size_t)ox * ntx * nty + (size_t)by * ntx + bx] = e;
            }
}

// ---- the plane filter (ssf_extract.hip: k_plane_filter_lds / _global): its windows of superpixel-grid nodes and its launch plan ----
// F Jacobi sweeps make a node's final state a function of the nodes within graph distance F of it, so a workgroup that owns a CORE
// tile of PF_TX x PF_TY nodes computes everything within F of the core redundantly and exchanges nothing.  The graph is the
// reference's, typo included (TPS_RGBD_kernels.cu:583: `x<gridSizeX` where `xx<gridSizeX` was meant): the right-hand neighbour of a
// node in the LAST column is the FIRST node of the next row.  A window that touches the last column therefore takes a second
// rectangle along the first columns (W2: columns [0, F), one row down), whose nodes are at distance >= 1 + column from the core;
// nothing in the first columns reads the last one, so the closure ends there.  tests/cpp/tile_geometry_smoke.cpp walks the graph
// breadth first from every core and checks that each node reached has a slot of its own.
#define PF_TX 16
#define PF_TY 12
struct PfWindow {
    int x0, y0, w, h;              // W1: core +- F, clipped to the grid
    int x2n, y2, h2;               // W2: columns [0, x2n) x rows [y2, y2 + h2) (x2n = 0: none)
    int n1, n2;
    SSF_GEOM_HD int slot(int x, int y) const {
        const unsigned int lx = (unsigned int)(x - x0), ly = (unsigned int)(y - y0);
        if (lx < (unsigned int)w && ly < (unsigned int)h) return (int)ly * w + (int)lx;
        const unsigned int l2 = (unsigned int)(y - y2);
        if ((unsigned int)x < (unsigned int)x2n && l2 < (unsigned int)h2) return n1 + (int)l2 * x2n + x;
        return -1;
    }
    SSF_GEOM_HD void node(int s, int& x, int& y) const {       // the node that slot s < n1 + n2 is laid out for
        if (s < n1) { const int ly = s / w; x = x0 + (s - ly * w); y = y0 + ly; }
        else { const int q = s - n1, ly = q / x2n; x = q - ly * x2n; y = y2 + ly; }
    }
};
SSF_GEOM_HD PfWindow pf_window(int gx, int gy, int tx, int ty, int F) {
#if !defined(__HIPCC__)
    using std::max; using std::min;            // (under hipcc: HIP's own, as the kernels' code was built with)
#endif
    PfWindow wd;
    const int cx0 = tx * PF_TX, cy0 = ty * PF_TY, cx1 = min(cx0 + PF_TX, gx) - 1, cy1 = min(cy0 + PF_TY, gy) - 1;
    wd.x0 = max(cx0 - F, 0); wd.y0 = max(cy0 - F, 0);
    const int x1 = min(cx1 + F, gx - 1), y1 = min(cy1 + F, gy - 1);
    wd.w = x1 - wd.x0 + 1; wd.h = y1 - wd.y0 + 1; wd.n1 = wd.w * wd.h;
    wd.x2n = 0; wd.y2 = 0; wd.h2 = 0;
    if (x1 == gx - 1 && wd.x0 > 0 && F > 0) {                // touches the last column without holding the first
        // rows: a node of the last column at distance d from the core has its wrap neighbour (0, y + 1) at distance d + 1, whose
        // column neighbours matter up to F - d - 1 rows away: rows [cy0 - F + 2, cy1 + F] whatever d (one more row on top kept);
        // NOT "the window's rows + 1": a window clipped by the top of the grid still needs row 0 (found by the test with
        // filter_threshold 1.0, where no neighbour is gated away)
        wd.x2n = min(F, wd.x0); wd.y2 = max(cy0 - F + 1, 0);
        wd.h2 = min(cy1 + F + 1, gy - 1) - wd.y2 + 1;
        if (wd.h2 <= 0) { wd.x2n = 0; wd.h2 = 0; }
    }
    wd.n2 = wd.x2n * wd.h2;
    return wd;
}
// the whole grid as ONE window that is all core: slot = node index, no second rectangle
SSF_GEOM_HD PfWindow pf_whole_grid(int gx, int gy) { return PfWindow{0, 0, gx, gy, 0, 0, 0, gx * gy, 0}; }

// Which form a gx x gy grid with F sweeps takes (launch_plane_filter only executes this):
//   tiled    the largest window of a 16 x 12 core tile holds <= 1024 nodes: a workgroup per tile, a node per thread
//            (F <~ 9; a grid of one tile included -- x0 = 0, so no second rectangle);
//   whole    up to 5120 nodes: one workgroup of 1024 threads per frame, the whole grid as its window, NPT nodes per thread, the
//            smallest of 2, 3, 5 that covers the grid.  NPT 2 is 64 KB at most and needs nothing; 3 and 5 need the device to grant
//            a workgroup 160 KB of LDS (big_lds: asked by the launcher, which plans again with false when refused);
//   global   everything else: one workgroup per frame over the scratch FrameMaps::filt.
// An LDS form holds 32 B per window node: two states of three floats and the centroid.
enum PfForm { PF_TILED, PF_WHOLE, PF_GLOBAL };
struct PfPlan {
    PfForm form;
    int ntx, nty;                 // workgroups per frame
    int threads, npt;             // threads per workgroup, nodes per thread
    int window;                   // most nodes a workgroup holds in LDS (0: global)
    size_t lds;                   // dynamic LDS bytes per workgroup
    bool big_lds;                 // lds exceeds what a launch gets without the attribute
};
#define PF_THREADS 1024           // of a whole-grid workgroup, and the most nodes a tile's window may hold
#define PF_LDS_PER_NODE 32
#define PF_LDS_PLAIN (64 * 1024)
#define PF_LDS_BIG (160 * 1024)
inline PfPlan pf_plan(int gx, int gy, int F, bool big_lds_granted = true) {
    const int S = gx * gy, ntx = (gx + PF_TX - 1) / PF_TX, nty = (gy + PF_TY - 1) / PF_TY;
    int worst = 0;
    for (int ty = 0; ty < nty; ty++)
        for (int tx = 0; tx < ntx; tx++) { const PfWindow wd = pf_window(gx, gy, tx, ty, F); worst = std::max(worst, wd.n1 + wd.n2); }
    if (worst <= PF_THREADS) return PfPlan{PF_TILED, ntx, nty, ((worst + 63) / 64) * 64, 1, worst, (size_t)worst * PF_LDS_PER_NODE, false};
    const int npt = S <= 2 * PF_THREADS ? 2 : S <= 3 * PF_THREADS ? 3 : 5;
    const size_t lds = (size_t)S * PF_LDS_PER_NODE;
    const bool big = lds > PF_LDS_PLAIN;
    if (S <= PF_THREADS * npt && (!big || big_lds_granted)) return PfPlan{PF_WHOLE, 1, 1, PF_THREADS, npt, S, lds, big};
    return PfPlan{PF_GLOBAL, 1, 1, PF_THREADS, 0, 0, 0, false};
}

}  // namespace ssf
