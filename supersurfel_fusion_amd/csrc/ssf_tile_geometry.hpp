// ssf_tile_geometry.hpp -- the window of grid cells around a tile of pixels: the ONE statement of it, for the tile kernels of
// ssf_extract.hip (CellWindow) and for the two host tables a handle is created with (SegParams::win_cells_max, ::pass_geom).
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

}  // namespace ssf
