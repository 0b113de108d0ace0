// ssf_navgrid.hpp -- what ssf_navgrid.hip (ssf_navgrid_build, in the product library) shares with ssf_navcarve.hip
// (ssf_navgrid_carve, include/ssf_navcarve.h) and the live layer (ssf_navlive.hip, ssf_navdyn.hip): the kernels' view of a grid, the
// cells kernel's body, the cell of a map-frame point and the march of a ray through the grid, and the four parts of a grid call.
// Private to the library's own files: nothing here is exported.
#pragma once
#include "ssf_slots.hpp"
#include "ssf_handle.hpp"

namespace ssf {

enum { NAV_TILE = 32, NAV_TILE_SHIFT = 5, NAV_CELLS = NAV_TILE * NAV_TILE, NAV_CHUNK = 256, NAV_HIST = 2048, NAV_MAX_SPLIT = 32 };
// the grid's accumulators: four planes of P words.  Empty: ~0 in the minimum's plane, 0 in the others (no float's image is either)
struct NavAcc { uint32_t* zmin; uint32_t* zmax; uint32_t* nfloor; uint32_t* nobst; };
// the sums the host reads: rows used, samples that exist, samples accepted, cells free / occupied / unknown, list entries
enum { NAV_ROWS = 0, NAV_SAMPLES = 1, NAV_ACCEPTED = 2, NAV_FREE = 3, NAV_OCC = 4, NAV_UNKNOWN = 5, NAV_LIST = 6, NAV_STATS = 8 };
// ... of a carve (include/ssf_navcarve.h): carving rays, their samples, entries, cells seen, cells carved | atomics issued on `seen`
enum { NC_CARVING = 0, NC_SAMPLES = 1, NC_ENTRIES = 2, NC_SEEN = 3, NC_CARVED = 4, NC_ATOMICS = 5, NC_STATS = 8 };

// R = 9 floats row-major and t (grid-to-map, ssf_get_pose's layout); ntx x nty tiles of 32 x 32 cells; fW = (float)W
struct NavGrid {
    float R[9], t[3];
    int W, H, ntx, nty;
    float res, step, fW, fH, zmin, zmax, floor_max, floor_cos, min_conf, s;
    int32_t ti0, ti1, tl0, tl1;
    int max_steps, min_hits;
};
struct NavView { NavGrid grid; ModelView model; };               // one kernel argument: the grid and the rows put into it
struct NavOut { float* zmin; float* zmax; uint32_t* hits; int8_t* state; };       // nullptr = not produced

// ---- cells: one thread per cell -------------------------------------------------------------------------------------------
// CARVE (include/ssf_navcarve.h step 7): a cell with seen >= min_seen ray entries is free unless it is occupied; the cells seen
// and the cells that this turned from unknown to free are counted, and `seen` goes out with the other arrays
struct NavSeen { const uint32_t* seen; int min_seen; uint32_t* out; unsigned long long* stats; };
// the body of k_navgrid_cells (ssf_navgrid.hip) and of its carving sibling k_navcarve_cells (ssf_navcarve.hip): workgroups of 256
template <bool CARVE>
__device__ __forceinline__ void navgrid_cells_body(const NavAcc& acc, size_t P, int min_hits, const NavOut& out, unsigned long long* __restrict__ stats,
                                                   const NavSeen& sn) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long nfree = 0, nocc = 0, nunk = 0, nseen = 0, ncarved = 0;
    if (p < P) {
        const uint32_t zlo = acc.zmin[p], zhi = acc.zmax[p], nfloor = acc.nfloor[p], nobst = acc.nobst[p];
        int8_t st = nobst >= (uint32_t)min_hits ? (int8_t)100 : (nfloor >= (uint32_t)min_hits ? (int8_t)0 : (int8_t)-1);
        if (CARVE) {
            const uint32_t s = sn.seen[p];
            const bool through = s >= (uint32_t)sn.min_seen;
            nseen = through; ncarved = through && st < 0;
            if (ncarved) st = (int8_t)0;
            if (sn.out) sn.out[p] = s;
        }
        nocc = st == 100; nfree = st == 0; nunk = st < 0;
        if (out.zmin) out.zmin[p] = __uint_as_float(zlo == ~0u ? 0x7F800000u : float_order_bits_inv(zlo));       // empty: +inf
        if (out.zmax) out.zmax[p] = __uint_as_float(zhi == 0u ? 0xFF800000u : float_order_bits_inv(zhi));        // empty: -inf
        if (out.hits) { out.hits[2 * p] = nfloor; out.hits[2 * p + 1] = nobst; }
        if (out.state) out.state[p] = st;
    }
    block_sums({nfree, nocc, nunk}, stats, NAV_FREE);
    if (CARVE) block_sums({nseen, ncarved}, sn.stats, NC_SEEN);
}

// ---- rays through the grid: the march of the carve (ssf_navcarve.hip) and of the live layer (ssf_navlive.hip) -----------------
// the map-frame point S in the grid frame (ssf_navgrid.h steps 1 and 4): true iff it lies in the grid and in the band of step 5;
// (gx, gy): its position in cells; z: its height in the grid frame.  THE one place where a point meets the grid: the forms without
// z, the cell and the memory's (cell, z) below all go through it
__device__ __forceinline__ bool nav_grid_point(const NavGrid& G, float Sx, float Sy, float Sz, float& gx, float& gy, float& z) {
    const float dx = Sx - G.t[0], dy = Sy - G.t[1], dz = Sz - G.t[2];
    const float* R = G.R;
    const float Cx = (R[0] * dx + R[3] * dy) + R[6] * dz, Cy = (R[1] * dx + R[4] * dy) + R[7] * dz, Cz = (R[2] * dx + R[5] * dy) + R[8] * dz;
    gx = Cx / G.res; gy = Cy / G.res; z = Cz;
    if (!(gx >= 0.0f && gx < G.fW && gy >= 0.0f && gy < G.fH)) return false;
    return Cz > G.floor_max && Cz <= G.zmax;
}
__device__ __forceinline__ bool nav_grid_point(const NavGrid& G, float Sx, float Sy, float Sz, float& gx, float& gy) { float z; return nav_grid_point(G, Sx, Sy, Sz, gx, gy, z); }
// the cell in whose band the map-frame point S lies, or -1; z: as above (ssf_navmem.hip's slices)
__device__ __forceinline__ int nav_cell(const NavGrid& G, float Sx, float Sy, float Sz, float& z) {
    float gx, gy;
    if (!nav_grid_point(G, Sx, Sy, Sz, gx, gy, z)) return -1;
    return (int)gy * G.W + (int)gx;
}
__device__ __forceinline__ int nav_cell(const NavGrid& G, float Sx, float Sy, float Sz) { float z; return nav_cell(G, Sx, Sy, Sz, z); }
// a ray in the map frame, and the cell in whose band its sample m is accepted, or -1 (z: as above)
struct NavMarchRay { float O[3], D[3]; };
__device__ __forceinline__ int nav_sample_cell(const NavGrid& G, const NavMarchRay& r, int m, float& z) {
    const float tm = (float)m * G.step;
    return nav_cell(G, r.O[0] + tm * r.D[0], r.O[1] + tm * r.D[1], r.O[2] + tm * r.D[2], z);
}
__device__ __forceinline__ int nav_sample_cell(const NavGrid& G, const NavMarchRay& r, int m) { float z; return nav_sample_cell(G, r, m, z); }
// The march of ONE RAY BY ONE WAVE: its samples m = 0 .. M over the lanes, m = lane, lane + 64, ...  The cell of sample m - 1 comes
// from the neighbouring lane (the same formula, so the same bits), across rounds of 64 through `carry`.  Only entries -- a sample in a
// cell's band whose predecessor was not -- reach `seen`, with an integer atomicAdd (order-free).  The rays a wave takes one after the
// other are neighbouring pixels: they start in the same cell and stay together for their first cells, and all of that would land on a
// few addresses.  So what a lane would add for a sample m < 64 of consecutive rays to one cell is merged in its registers (pend_cell,
// pend_n: they live across the wave's rays) and issued as one atomic when the cell changes; the caller issues the last one.
__device__ __forceinline__ void nav_march_ray(const NavGrid& G, const NavMarchRay& r, int M, uint32_t* seen, int& pend_cell, uint32_t& pend_n,
                                              unsigned long long& n_entries, unsigned long long& n_atomics) {
    const int ln = lane();
    int carry = -1;                                                   // the cell of the sample before this round's first
    for (int base = 0; base <= M; base += 64) {
        const int m = base + ln;
        const int c = m <= M ? nav_sample_cell(G, r, m) : -1;
        int prev = __shfl_up(c, 1, 64);
        if (ln == 0) prev = carry;
        carry = __shfl(c, 63, 64);
        if (c >= 0 && c != prev) {
            n_entries++;
            if (base == 0) {
                if (c == pend_cell) pend_n++;
                else {
                    if (pend_n) { atomicAdd(&seen[pend_cell], pend_n); n_atomics++; }
                    pend_cell = c; pend_n = 1u;
                }
            } else { atomicAdd(&seen[c], 1u); n_atomics++; }
        }
    }
}

}  // namespace ssf

#pragma GCC visibility push(hidden)
// One grid call in four parts, shared by ssf_navgrid_build and ssf_navgrid_carve (`who` words the errors): begin = the refusals, the
// frame and the kernels' view of the grid; reserve = the working buffers and the staged outputs; accumulate = prep, fill and tile
// into the accumulators; finish = the cells (carved by `sn` when given), the clearance, the outputs and the stats.
struct NavCall { const char* who; NavGrid G; float pose[12]; size_t P; unsigned long long total; };

// how finish launches the cells kernel: ssf_navgrid.hip's own, or the carve's with `seen`
typedef void (*NavCellsLaunch)(hipStream_t st, const ssf::NavGrid& G, const ssf::NavAcc& acc, const ssf::NavOut& out, unsigned long long* stats,
                               const ssf::NavSeen* sn);
// log2 of a number of heading bins (1, 2, 4, .. 32), or -1: the footprint's layers, the pose plan's states
inline int nav_log2_bins(int B) {
    for (int lg = 0; lg <= 5; lg++) if (B == (1 << lg)) return lg;
    return -1;
}
const char* navgrid_size_res(const ssf_navgrid_params* p);
int navgrid_begin(ssf_handle* h, const ssf_navgrid_params* p, NavCall& c);
int navgrid_reserve(ssf_handle* h, const ssf_navgrid_params* p, const NavCall& c, StagedIo& io);
int navgrid_accumulate(ssf_handle* h, const ssf_navgrid_params* p, NavCall& c);            // (under the caller's TimerScope)
int navgrid_finish(ssf_handle* h, const ssf_navgrid_params* p, const NavCall& c, ssf::NavOut o, int32_t* d2, const StagedIo& io,
                   NavCellsLaunch cells, const ssf::NavSeen* sn, ssf_navgrid_stats* stats, unsigned long long* carve_sums = nullptr);
// the clearance of ssf_navgrid.h step 8 on a state that is on the device (navgrid_columns, navgrid_rows): what finish runs, and what
// ssf_navlive_overlay (ssf_navlive.hip) runs on its own state.  g: W * H words of working space
namespace ssf {
void launch_navgrid_clearance(hipStream_t st, const int8_t* state, int W, int H, int R, int unknown_too, uint16_t* g, int32_t* dist2);
}
#pragma GCC visibility pop
