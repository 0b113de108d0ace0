// ssf_navgrid.hip -- the floor-plane navigation grid of the fused model (include/ssf_navgrid.h) on gfx950.
//
// What is computed is pinned, operation by operation, in include/ssf_navgrid.h (the numpy restatement: tests/navgrid_ref.py).
// Every result is an integer minimum, maximum or sum: exact, and independent of the order in which rows and samples arrive.  How
// (the shape of ssf_render.hip, with cells for pixels):
//   * prep     k_navgrid_prep: one thread per slot of [visible rows | out-of-view span] (the two stores are read in place).  The
//              gates, the grid-frame record (C, E1, E2, N.z, the half-axes and lattice sizes) and a CONSERVATIVE cell box of
//              the disc; every 32 x 32-cell tile the box touches gets one integer count.  A map sits in few tiles, so the counts
//              of a workgroup are first taken in an LDS histogram (grids of up to NAV_HIST tiles) and reach the tile's global
//              counter as one atomic per workgroup and tile.  rows_used and the number of lattice samples that exist are
//              summed here (a row can sit in several tiles' lists, but is prepared once).
//   * scan     launch_slots_scan (ssf_slots.hpp) over the tile counts (64-bit total); the host reads the total once and sizes the list.
//   * fill     k_navgrid_fill: (tile -> slot) lists; a workgroup reserves its entries of a list with one returning atomic and
//              ranks them in LDS (same histogram).  The order inside a list is arbitrary.
//   * tile     k_navgrid_tile: workgroups of 16 waves; a tile's list is dealt in chunks of 256 records to `split` workgroups
//              (the lists are as uneven as the map: without the split a few workgroups do all the work).  A workgroup's
//              accumulators for the tile (min, max, two counts: 16 B per cell, 16 KB) sit in LDS; the records are staged through
//              LDS; a row's samples are spread over the lanes of ONE wave (the lattice size varies per row), and each accepted
//              sample that falls into this tile does its LDS integer atomics.  No global atomic per sample: at its end a
//              workgroup folds the cells it touched into the grid's accumulators (four integer atomics per touched cell).  A
//              workgroup without a chunk leaves at once.
//   * cells    k_navgrid_cells: one thread per cell: the accumulators decoded, the state, the outputs with plain stores, the
//              cells counted per state.
//   * columns  k_navgrid_columns: one thread per column, sweeping up and then down: the distance along y to the nearest obstacle
//              cell, capped at R + 1 (reads and writes of a wave are consecutive).
//   * rows     k_navgrid_rows: one workgroup per row holds the row's squared column distances in LDS; each cell takes the minimum
//              over |dx| <= R of g^2 + dx^2, capped at R^2.  Integers throughout.
// Sums are reduced per workgroup and added with one 64-bit atomic each.  Nothing here writes to the handle's stores, counters or
// scratch: the working set is NavGridWs (ssf_handle.hpp).
//
// The call is made of four parts -- begin, reserve, accumulate, finish (ssf_navgrid.hpp) -- which ssf_navgrid_carve
// (ssf_navcarve.hip, include/ssf_navcarve.h) runs as well, with its rays between accumulate and finish.
#include "ssf_navgrid.hpp"

namespace ssf {

// steps per half-axis (include/ssf_navgrid.h step 3): q = ceilf(h / step)
__device__ __forceinline__ int nav_steps(float h, float step, int max_steps) {
    const float q = ceilf(h / step);
    return q >= (float)max_steps ? max_steps : (q >= 1.0f ? (int)q : 1);
}
// the lattice points (i, j) with i i n2 n2 + j j n1 n1 <= n1 n1 n2 n2: per i >= 0 the largest j, a float guess made exact
__device__ __forceinline__ int nav_lattice_count(int n1, int n2) {
    const int A = n1 * n1, B = n2 * n2, AB = A * B;
    int total = 0;
    for (int i = 0; i <= n1; i++) {
        const int rem = AB - i * i * B;
        int j = min(n2, (int)sqrtf((float)rem / (float)A));
        while (j < n2 && (j + 1) * (j + 1) * A <= rem) j++;
        while (j > 0 && j * j * A > rem) j--;
        total += (i ? 2 : 1) * (2 * j + 1);
    }
    return total;
}

// ---- prep: one thread per slot ---------------------------------------------------------------------------------------
// rec[4 s ..]: (C, h1) (E1, h2) (E2, N.z) (bits n1, bits n2, 0, 0), written for slots with a box; rbox[s]: x0 | x1 << 16,
// y0 | y1 << 16 in cells (empty: x0 = 1 > x1 = 0)
__global__ __launch_bounds__(256) void k_navgrid_prep(NavView nv, float4* __restrict__ rec, uint2* __restrict__ rbox,
                                                      uint32_t* __restrict__ tcnt, unsigned long long* __restrict__ stats) {
    __shared__ uint32_t hist[NAV_HIST];
    const NavGrid& G = nv.grid;
    const int ntiles = G.ntx * G.nty;
    const bool use_hist = ntiles <= NAV_HIST;                        // block-uniform
    if (use_hist) {
        for (int t = threadIdx.x; t < ntiles; t += 256) hist[t] = 0u;
        __syncthreads();
    }
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    SurfelSoA src; size_t row;
    const bool have = slot_row(nv.model, s, src, row);
    uint2 box = make_uint2(1u, 1u);
    unsigned long long used = 0, nsamp = 0;
    if (have) {
        const float cx = src.pos[3 * row], cy = src.pos[3 * row + 1], cz = src.pos[3 * row + 2];
        const float conf = src.conf[row], dx = src.dims[2 * row], dy = src.dims[2 * row + 1];
        const int32_t t0 = src.stamps[2 * row], t1 = src.stamps[2 * row + 1];
        if (finite3(cx, cy, cz) && conf > G.min_conf && t0 >= G.ti0 && t0 <= G.ti1 && t1 >= G.tl0 && t1 <= G.tl1 &&
            dx > 0.0f && dy > 0.0f && isfinite(dx) && isfinite(dy)) {
            used = 1;
            const float* R = G.R;
            const float px = cx - G.t[0], py = cy - G.t[1], pz = cz - G.t[2];
            // C_j = (R0j d.x + R1j d.y) + R2j d.z (contraction off: one IEEE operation each, in this order)
            const float Cx = (R[0] * px + R[3] * py) + R[6] * pz, Cy = (R[1] * px + R[4] * py) + R[7] * pz, Cz = (R[2] * px + R[5] * py) + R[8] * pz;
            const float* r0 = src.r0 + 3 * row; const float* r1 = src.r1 + 3 * row; const float* r2 = src.r2 + 3 * row;
            const float a0 = r0[0], a1 = r0[1], a2 = r0[2], b0 = r1[0], b1 = r1[1], b2 = r1[2], n0 = r2[0], n1v = r2[1], n2v = r2[2];
            const float E1x = (R[0] * a0 + R[3] * a1) + R[6] * a2, E1y = (R[1] * a0 + R[4] * a1) + R[7] * a2, E1z = (R[2] * a0 + R[5] * a1) + R[8] * a2;
            const float E2x = (R[0] * b0 + R[3] * b1) + R[6] * b2, E2y = (R[1] * b0 + R[4] * b1) + R[7] * b2, E2z = (R[2] * b0 + R[5] * b1) + R[8] * b2;
            const float Nz = (R[2] * n0 + R[5] * n1v) + R[8] * n2v;
            const float h1 = G.s * sqrtf(dx), h2 = G.s * sqrtf(dy);
            const int n1 = nav_steps(h1, G.step, G.max_steps), n2 = nav_steps(h2, G.step, G.max_steps);
            nsamp = (unsigned long long)nav_lattice_count(n1, n2);
            // Conservative box.  A sample is C + a E1 + b E2 with |a| <= h1, |b| <= h2, up to the rounding of three f32 operations
            // per component (a few 6e-8 of the terms): the extent |E1| h1 + |E2| h2 widened by 1e-3 relative + 1e-5 of the terms
            // covers it, and one cell on either side covers the rounding of the division by res (< 3e-4 cells at 4096 cells).
            // With a non-finite C, E1 or E2 every sample has a NaN or infinite component where it matters (0 * inf = NaN): S.x or
            // S.y fails step 4, S.z fails step 5 -- no box at all.
            if (finite3(Cx, Cy, Cz) && finite3(E1x, E1y, E1z) && finite3(E2x, E2y, E2z)) {
                const float slack = 1e-5f * (fabsf(Cx) + fabsf(Cy) + fabsf(Cz) + h1 + h2) + 1e-6f;
                const float ex = (fabsf(E1x) * h1 + fabsf(E2x) * h2) * 1.001f + slack;
                const float ey = (fabsf(E1y) * h1 + fabsf(E2y) * h2) * 1.001f + slack;
                const float ez = (fabsf(E1z) * h1 + fabsf(E2z) * h2) * 1.001f + slack;
                const float gxl = (Cx - ex) / G.res - 1.0f, gxh = (Cx + ex) / G.res + 1.0f;
                const float gyl = (Cy - ey) / G.res - 1.0f, gyh = (Cy + ey) / G.res + 1.0f;
                if ((Cz + ez >= G.zmin) && (Cz - ez <= G.zmax) && (gxh >= 0.0f) && (gxl <= (float)(G.W - 1)) && (gyh >= 0.0f) &&
                    (gyl <= (float)(G.H - 1))) {
                    const int x0 = (int)floorf(fmaxf(gxl, 0.0f)), x1 = (int)floorf(fminf(gxh, (float)(G.W - 1)));
                    const int y0 = (int)floorf(fmaxf(gyl, 0.0f)), y1 = (int)floorf(fminf(gyh, (float)(G.H - 1)));
                    float4* o = rec + 4 * (size_t)s;
                    o[0] = make_float4(Cx, Cy, Cz, h1);
                    o[1] = make_float4(E1x, E1y, E1z, h2);
                    o[2] = make_float4(E2x, E2y, E2z, Nz);
                    o[3] = make_float4(__int_as_float(n1), __int_as_float(n2), 0.0f, 0.0f);
                    box = make_uint2((uint32_t)x0 | ((uint32_t)x1 << 16), (uint32_t)y0 | ((uint32_t)y1 << 16));
                    for (int ty = y0 >> NAV_TILE_SHIFT; ty <= (y1 >> NAV_TILE_SHIFT); ty++)
                        for (int tx = x0 >> NAV_TILE_SHIFT; tx <= (x1 >> NAV_TILE_SHIFT); tx++) atomicAdd(use_hist ? &hist[ty * G.ntx + tx] : &tcnt[ty * G.ntx + tx], 1u);
                }
            }
        }
    }
    if ((int)s < nv.model.nslots) rbox[s] = box;
    __syncthreads();                                                  // (hist is complete)
    if (use_hist)
        for (int t = threadIdx.x; t < ntiles; t += 256) { const uint32_t c = hist[t]; if (c) atomicAdd(&tcnt[t], c); }
    block_sums({used, nsamp}, stats, NAV_ROWS);
}

// ---- fill: the (tile -> slot) lists -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navgrid_fill(int nslots, int ntx, int ntiles, const uint2* __restrict__ rbox,
                                                      uint32_t* __restrict__ cursor, uint32_t* __restrict__ list) {
    __shared__ uint32_t hist[NAV_HIST], base[NAV_HIST];
    const bool use_hist = ntiles <= NAV_HIST;                        // block-uniform
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    int x0 = 1, x1 = 0, y0 = 1, y1 = 0;
    if ((int)s < nslots) { const uint2 b = rbox[s]; x0 = b.x & 0xFFFF; x1 = b.x >> 16; y0 = b.y & 0xFFFF; y1 = b.y >> 16; }
    const bool any = x0 <= x1 && y0 <= y1;
    const int tx0 = x0 >> NAV_TILE_SHIFT, tx1 = x1 >> NAV_TILE_SHIFT, ty0 = y0 >> NAV_TILE_SHIFT, ty1 = y1 >> NAV_TILE_SHIFT;
    if (!use_hist) {
        if (any)
            for (int ty = ty0; ty <= ty1; ty++)
                for (int tx = tx0; tx <= tx1; tx++) list[atomicAdd(&cursor[ty * ntx + tx], 1u)] = s;
        return;
    }
    // the workgroup's entries per tile, one reservation per tile in the global list, then the ranks inside the reservation
    for (int t = threadIdx.x; t < ntiles; t += 256) hist[t] = 0u;
    __syncthreads();
    if (any)
        for (int ty = ty0; ty <= ty1; ty++)
            for (int tx = tx0; tx <= tx1; tx++) atomicAdd(&hist[ty * ntx + tx], 1u);
    __syncthreads();
    for (int t = threadIdx.x; t < ntiles; t += 256) {
        const uint32_t c = hist[t];
        if (c) { base[t] = atomicAdd(&cursor[t], c); hist[t] = 0u; }
    }
    __syncthreads();
    if (any)
        for (int ty = ty0; ty <= ty1; ty++)
            for (int tx = tx0; tx <= tx1; tx++) { const int t = ty * ntx + tx; list[base[t] + atomicAdd(&hist[t], 1u)] = s; }
}

// ---- tile: workgroups of 1024; workgroup (tile t, part k) takes chunks k, k + split, ... of tile t's list -----------------------
__global__ __launch_bounds__(1024) void k_navgrid_tile(NavGrid G, int split, const float4* __restrict__ rec, const uint32_t* __restrict__ list,
                                                       const uint32_t* __restrict__ toff, NavAcc acc,
                                                       unsigned long long* __restrict__ stats) {
    __shared__ uint32_t cmin[NAV_CELLS], cmax[NAV_CELLS], cfloor[NAV_CELLS], cobst[NAV_CELLS];
    __shared__ float4 sr[4 * NAV_CHUNK];
    const int t = blockIdx.x / split, part = blockIdx.x - t * split, tx = t % G.ntx, ty = t / G.ntx;
    const int wv = threadIdx.x >> 6;
    const uint32_t beg = toff[t], end = toff[t + 1];
    const uint32_t first = beg + (uint32_t)part * NAV_CHUNK;
    if (first >= end || first < beg) return;                          // block-uniform: no chunk for this part (first < beg: wrapped past 2^32)
    cmin[threadIdx.x] = ~0u; cmax[threadIdx.x] = 0u; cfloor[threadIdx.x] = 0u; cobst[threadIdx.x] = 0u;
    unsigned long long accepted = 0;
    for (unsigned long long c = first; c < end; c += (unsigned long long)split * NAV_CHUNK) {
        const uint32_t c0 = (uint32_t)c;
        const int n = (int)min((uint32_t)NAV_CHUNK, end - c0);
        __syncthreads();                                              // the accumulators are set; the last chunk's records are done with
        if ((int)(threadIdx.x >> 2) < n) sr[threadIdx.x] = rec[4 * (size_t)list[c0 + (threadIdx.x >> 2)] + (threadIdx.x & 3)];
        __syncthreads();
        for (int r = wv; r < n; r += 16) {                            // a record per wave, its samples over the lanes
            const float4 A = sr[4 * r], B = sr[4 * r + 1], Cc = sr[4 * r + 2], D = sr[4 * r + 3];
            const int n1 = __float_as_int(D.x), n2 = __float_as_int(D.y);
            const int cols = 2 * n2 + 1, total = (2 * n1 + 1) * cols;
            const int lim = n1 * n1 * n2 * n2;
            const float fn1 = (float)n1, fn2 = (float)n2;
            for (int idx = lane(); idx < total; idx += 64) {
                const int q = idx / cols;
                const int i = q - n1, j = idx - q * cols - n2;
                if (i * i * n2 * n2 + j * j * n1 * n1 > lim) continue;
                const float a = ((float)i / fn1) * A.w, b = ((float)j / fn2) * B.w;
                const float Sx = (A.x + a * B.x) + b * Cc.x, Sy = (A.y + a * B.y) + b * Cc.y, z = (A.z + a * B.z) + b * Cc.z;
                const float gx = Sx / G.res, gy = Sy / G.res;
                if (!(gx >= 0.0f && gx < G.fW && gy >= 0.0f && gy < G.fH)) continue;
                const int ix = (int)gx, iy = (int)gy;
                if ((ix >> NAV_TILE_SHIFT) != tx || (iy >> NAV_TILE_SHIFT) != ty) continue;       // another tile's sample
                if (!(z >= G.zmin && z <= G.zmax)) continue;
                accepted++;
                const int cell = ((iy & (NAV_TILE - 1)) << NAV_TILE_SHIFT) | (ix & (NAV_TILE - 1));
                const uint32_t e = float_order_bits(__float_as_uint(z + 0.0f));
                atomicMin(&cmin[cell], e);
                atomicMax(&cmax[cell], e);
                if (z > G.floor_max) atomicAdd(&cobst[cell], 1u);
                else if (fabsf(Cc.w) >= G.floor_cos) atomicAdd(&cfloor[cell], 1u);
            }
        }
    }
    __syncthreads();
    // one cell per thread: what this workgroup saw of it goes into the grid's accumulators (a touched cell is inside the grid)
    const uint32_t zlo = cmin[threadIdx.x];
    if (zlo != ~0u) {
        const int x = tx * NAV_TILE + (threadIdx.x & (NAV_TILE - 1)), y = ty * NAV_TILE + (threadIdx.x >> NAV_TILE_SHIFT);
        const size_t p = (size_t)y * G.W + x;
        const uint32_t nfloor = cfloor[threadIdx.x], nobst = cobst[threadIdx.x];
        atomicMin(&acc.zmin[p], zlo);
        atomicMax(&acc.zmax[p], cmax[threadIdx.x]);
        if (nfloor) atomicAdd(&acc.nfloor[p], nfloor);
        if (nobst) atomicAdd(&acc.nobst[p], nobst);
    }
    block_sums<1, 16>({accepted}, stats, NAV_ACCEPTED);
}

// ---- cells: one thread per cell (the body: ssf_navgrid.hpp) --------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navgrid_cells(NavAcc acc, size_t P, int min_hits, NavOut out, unsigned long long* __restrict__ stats) {
    navgrid_cells_body<false>(acc, P, min_hits, out, stats, NavSeen{nullptr, 1, nullptr, nullptr});
}

// ---- clearance: columns, then rows ------------------------------------------------------------------------------------------
// g[y][x] = min(R + 1, distance along y from (x, y) to the nearest obstacle cell of column x)
__global__ __launch_bounds__(64) void k_navgrid_columns(const int8_t* __restrict__ state, int W, int H, int R, int unknown_too,
                                                        uint16_t* __restrict__ g) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    int d = R + 1;
    for (int y = 0; y < H; y++) {
        const int8_t s = state[(size_t)y * W + x];
        d = (s == 100 || (unknown_too && s < 0)) ? 0 : min(d + 1, R + 1);
        g[(size_t)y * W + x] = (uint16_t)d;
    }
    d = R + 1;
    for (int y = H - 1; y >= 0; y--) {
        const int8_t s = state[(size_t)y * W + x];
        d = (s == 100 || (unknown_too && s < 0)) ? 0 : min(d + 1, R + 1);
        const uint16_t up = g[(size_t)y * W + x];
        if ((uint16_t)d < up) g[(size_t)y * W + x] = (uint16_t)d;
    }
}
// dist2[y][x] = min(R R, min over |dx| <= R of g[y][x + dx]^2 + dx^2); one workgroup per row (W <= 4096)
__global__ __launch_bounds__(256) void k_navgrid_rows(const uint16_t* __restrict__ g, int W, int R, int32_t* __restrict__ dist2) {
    __shared__ int g2[4096];
    const size_t base = (size_t)blockIdx.x * W;
    for (int x = threadIdx.x; x < W; x += 256) { const int v = g[base + x]; g2[x] = v * v; }
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += 256) {
        int best = R * R;
        const int lo = max(0, x - R), hi = min(W - 1, x + R);
        for (int xx = lo; xx <= hi; xx++) best = min(best, g2[xx] + (xx - x) * (xx - x));
        dist2[base + x] = best;
    }
}

// ---- launches -------------------------------------------------------------------------------------------------------
// tcnt[ntiles + 1] (zeroed by the caller) becomes the list offsets, cursor[ntiles] a copy; stats[NAV_LIST] = list entries
static void launch_navgrid_prep(hipStream_t st, const NavView& nv, float4* rec, uint2* rbox, uint32_t* tcnt, uint32_t* cursor,
                                unsigned long long* stats) {
    ScopedKernel sk("navgrid_prep", st);
    const int nb = nv.model.nbv + nv.model.nbo;
    if (nb > 0) hipLaunchKernelGGL(k_navgrid_prep, dim3(nb), dim3(256), 0, st, nv, rec, rbox, tcnt, stats);
    launch_slots_scan(st, tcnt, nv.grid.ntx * nv.grid.nty, cursor, stats + NAV_LIST);
}
static void launch_navgrid_fill(hipStream_t st, const NavView& nv, const uint2* rbox, uint32_t* cursor, uint32_t* list) {
    ScopedKernel sk("navgrid_fill", st);
    if (nv.model.nslots > 0)
        hipLaunchKernelGGL(k_navgrid_fill, dim3(nv.model.nslots / 256), dim3(256), 0, st, nv.model.nslots, nv.grid.ntx, nv.grid.ntx * nv.grid.nty, rbox, cursor, list);
}
// acc (its minimum plane set to ~0, the others to 0 by the caller) += the samples
static void launch_navgrid_tile(hipStream_t st, const NavGrid& G, int split, const float4* rec, const uint32_t* list, const uint32_t* toff,
                                const NavAcc& acc, unsigned long long* stats) {
    ScopedKernel sk("navgrid_tile", st);
    hipLaunchKernelGGL(k_navgrid_tile, dim3(G.ntx * G.nty * split), dim3(1024), 0, st, G, split, rec, list, toff, acc, stats);
}
// the cells' outputs and counts (a NavCellsLaunch: the carve has its own)
static void launch_navgrid_cells(hipStream_t st, const NavGrid& G, const NavAcc& acc, const NavOut& out, unsigned long long* stats, const NavSeen*) {
    ScopedKernel sk("navgrid_cells", st);
    const size_t P = (size_t)G.W * G.H;
    hipLaunchKernelGGL(k_navgrid_cells, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, acc, P, G.min_hits, out, stats);
}
void launch_navgrid_clearance(hipStream_t st, const int8_t* state, int W, int H, int R, int unknown_too, uint16_t* g, int32_t* dist2) {
    { ScopedKernel sk("navgrid_columns", st);
      hipLaunchKernelGGL(k_navgrid_columns, dim3((W + 63) / 64), dim3(64), 0, st, state, W, H, R, unknown_too, g); }
    { ScopedKernel sk("navgrid_rows", st);
      hipLaunchKernelGGL(k_navgrid_rows, dim3(H), dim3(256), 0, st, g, W, R, dist2); }
}

}  // namespace ssf

// ---- host: the entry points of include/ssf_navgrid.h -----------------------------------------------------------------------
// what pose NULL means (include/ssf_navgrid.h): floor-aligned, centred on the camera, snapped to the cell size
static void navgrid_default_pose(const ssf_handle* h, float res, int W, int H, float* pose) {
    const float R9[9] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, -1.0f, 0.0f, 1.0f, 0.0f};
    std::memcpy(pose, R9, sizeof(R9));
    pose[9] = (floorf(h->pose.t.x / res) - (float)(W / 2)) * res;
    pose[10] = 0.0f;
    pose[11] = (floorf(h->pose.t.z / res) - (float)(H / 2)) * res;
}
const char* navgrid_size_res(const ssf_navgrid_params* p) {
    if (p->width < 1 || p->width > 4096 || p->height < 1 || p->height > 4096) return "the grid's size must be 1..4096 x 1..4096";
    if (!std::isfinite(p->res) || !(p->res > 0.0f)) return "res must be finite and > 0";
    return nullptr;
}

int navgrid_begin(ssf_handle* h, const ssf_navgrid_params* p, NavCall& c) {
    auto refuse = [&](const char* what) { h->err = std::string(c.who) + ": " + what; return SSF_ERR_INVALID_ARG; };
    if (const char* what = navgrid_size_res(p)) return refuse(what);
    NavGrid& G = c.G;
    G.s = p->splat_scale == 0.0f ? 2.0f : p->splat_scale;
    if (!(G.s >= 0.0f) || !std::isfinite(G.s)) return refuse("splat_scale must be finite and >= 0");
    if (p->max_steps < 1 || p->max_steps > 16) return refuse("max_steps must be 1..16");
    if (p->max_dist_cells < 1 || p->max_dist_cells > 1024) return refuse("max_dist_cells must be 1..1024");
    if (p->min_hits < 1) return refuse("min_hits must be >= 1");
    if (!(p->z_max >= p->z_min)) return refuse("the height range needs z_min <= z_max");
    if (p->t_init_min > p->t_init_max || p->t_last_min > p->t_last_max) return refuse("a stamp range has min > max");
    if (!(p->floor_cos >= 0.0f) || !(p->floor_cos <= 1.0f)) return refuse("floor_cos must be in [0, 1]");
    { int rc = model_at_rest(h, c.who, "has no navigation grid"); if (rc) return rc; }
    float* pose = c.pose;
    if (p->pose) std::memcpy(pose, p->pose, sizeof(c.pose));
    else navgrid_default_pose(h, p->res, p->width, p->height, pose);
    std::memcpy(G.R, pose, 9 * sizeof(float)); G.t[0] = pose[9]; G.t[1] = pose[10]; G.t[2] = pose[11];
    G.W = p->width; G.H = p->height; G.ntx = (G.W + NAV_TILE - 1) / NAV_TILE; G.nty = (G.H + NAV_TILE - 1) / NAV_TILE;
    G.res = p->res; G.step = p->res * 0.5f; G.fW = (float)G.W; G.fH = (float)G.H;
    G.zmin = p->z_min; G.zmax = p->z_max; G.floor_max = p->floor_max; G.floor_cos = p->floor_cos; G.min_conf = p->min_conf;
    G.ti0 = p->t_init_min; G.ti1 = p->t_init_max; G.tl0 = p->t_last_min; G.tl1 = p->t_last_max;
    G.max_steps = p->max_steps; G.min_hits = p->min_hits;
    c.P = (size_t)G.W * G.H; c.total = 0;
    return SSF_OK;
}

int navgrid_reserve(ssf_handle* h, const ssf_navgrid_params* p, const NavCall& c, StagedIo& io) {
    NavGridWs& w = h->navgrid;
    const size_t P = c.P;
    const size_t slots = std::max<size_t>(model_view(h, p->visible_only != 0).nslots, 256);
    bool ok = true;
    if (slots > w.slots) {
        ok = w.bufs.grow({{(void**)&w.rec, 64 * slots}, {(void**)&w.rbox, 8 * slots}});
        if (ok) w.slots = slots;
    }
    if (ok) ok = w.tl.reserve_bins(w.bufs, (size_t)c.G.ntx * c.G.nty);
    if (ok && P > w.cells) {
        ok = w.bufs.grow({{(void**)&w.acc, 16 * P}, {(void**)&w.colg, 2 * P}, {(void**)&w.state, P}});
        if (ok) w.cells = P;
    }
    if (ok && !w.stats) ok = w.bufs.grow({{(void**)&w.stats, NAV_STATS * sizeof(unsigned long long)}});
    if (ok) ok = io.reserve(w.bufs, &w.img, &w.img_bytes, io.need());
    if (!ok) { h->err = std::string(c.who) + ": allocation of the working buffers failed"; return SSF_ERR_DEVICE; }
    return SSF_OK;
}

// (under the caller's TimerScope) the accumulators of the grid from the model's rows; c.total = the list entries
int navgrid_accumulate(ssf_handle* h, const ssf_navgrid_params* p, NavCall& c) {
    NavGridWs& w = h->navgrid;
    const NavGrid& G = c.G;
    const size_t P = c.P;
    const int ntiles = G.ntx * G.nty;
    const NavView nv{G, model_view(h, p->visible_only != 0)};
    hipStream_t st = h->stream;
    HCK(hipMemsetAsync(w.tl.off, 0, 4 * ((size_t)ntiles + 1), st));
    HCK(hipMemsetAsync(w.stats, 0, NAV_STATS * sizeof(unsigned long long), st));
    launch_navgrid_prep(st, nv, w.rec, w.rbox, w.tl.off, w.tl.cursor, w.stats);
    HCK(hipGetLastError());
    unsigned long long total = 0;
    HCK(hipMemcpyAsync(&total, w.stats + NAV_LIST, sizeof(total), hipMemcpyDeviceToHost, st));
    HCK(hipStreamSynchronize(st));
    const std::string who(c.who);
    { int rc = w.tl.reserve_list(w.bufs, total, h->err, (who + ": more than 2^32 - 1 (tile, row) list entries").c_str(),
                                 (who + ": allocation of ").c_str(), " bytes for the tile lists failed"); if (rc) return rc; }
    if (total > 0) { launch_navgrid_fill(st, nv, w.rbox, w.tl.cursor, w.tl.list); HCK(hipGetLastError()); }
    const NavAcc acc{w.acc, w.acc + P, w.acc + 2 * P, w.acc + 3 * P};
    HCK(hipMemsetAsync(acc.zmin, 0xFF, 4 * P, st));
    HCK(hipMemsetAsync(acc.zmax, 0, 12 * P, st));
    // parts per tile: enough workgroups for the chip when the lists are long, one when they are short
    const int split = (int)std::min<unsigned long long>(NAV_MAX_SPLIT, std::max<unsigned long long>(1, total / (16 * NAV_CHUNK)));
    launch_navgrid_tile(st, G, split, w.rec, w.tl.list, w.tl.off, acc, w.stats);
    HCK(hipGetLastError());
    c.total = total;
    return SSF_OK;
}

// (under the caller's TimerScope) sn: nullptr, or the carve's ray entries, whose NC_STATS sums come back in carve_sums
int navgrid_finish(ssf_handle* h, const ssf_navgrid_params* p, const NavCall& c, NavOut o, int32_t* d2, const StagedIo& io, NavCellsLaunch cells,
                   const NavSeen* sn, ssf_navgrid_stats* stats, unsigned long long* carve_sums) {
    NavGridWs& w = h->navgrid;
    const NavGrid& G = c.G;
    const size_t P = c.P;
    hipStream_t st = h->stream;
    const NavAcc acc{w.acc, w.acc + P, w.acc + 2 * P, w.acc + 3 * P};
    const bool want_dist = d2 != nullptr;
    if (want_dist && !o.state) o.state = w.state;                    // dist2 alone: the state is still computed, internally
    cells(st, G, acc, o, w.stats, sn);
    HCK(hipGetLastError());
    if (want_dist) {
        launch_navgrid_clearance(st, o.state, G.W, G.H, p->max_dist_cells, p->unknown_is_obstacle != 0, w.colg, d2);
        HCK(hipGetLastError());
    }
    unsigned long long s7[NAV_LIST] = {0, 0, 0, 0, 0, 0};
    HCK(hipMemcpyAsync(s7, w.stats, sizeof(s7), hipMemcpyDeviceToHost, st));
    if (sn && carve_sums) HCK(hipMemcpyAsync(carve_sums, sn->stats, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HCK(io.copy_out(st));
    { int rc = sync_collect(h); if (rc) return rc; }
    if (stats) {
        stats->rows_used = (int64_t)s7[NAV_ROWS]; stats->samples = (int64_t)s7[NAV_SAMPLES]; stats->samples_in_grid = (int64_t)s7[NAV_ACCEPTED];
        stats->cells_free = (int64_t)s7[NAV_FREE]; stats->cells_occupied = (int64_t)s7[NAV_OCC]; stats->cells_unknown = (int64_t)s7[NAV_UNKNOWN];
        stats->list_entries = (int64_t)c.total;
        std::memcpy(stats->pose, c.pose, sizeof(c.pose));
    }
    return SSF_OK;
}

extern "C" {
int ssf_navgrid_default_params(const ssf_handle* h, ssf_navgrid_params* p) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    std::memset(p, 0, sizeof(*p));
    p->width = 512; p->height = 512; p->res = 0.05f;
    p->z_min = -1.5f; p->z_max = 0.5f; p->floor_max = -0.8f; p->floor_cos = 0.8f;
    p->t_init_min = INT32_MIN; p->t_init_max = INT32_MAX; p->t_last_min = INT32_MIN; p->t_last_max = INT32_MAX;
    p->splat_scale = 2.0f; p->max_steps = 8; p->min_hits = 1; p->max_dist_cells = 40;
    return SSF_OK;
}

int ssf_navgrid_default_pose(const ssf_handle* h, const ssf_navgrid_params* p, float* pose12) {
    if (!h || !p || !pose12) return SSF_ERR_INVALID_ARG;
    if (navgrid_size_res(p)) return SSF_ERR_INVALID_ARG;
    navgrid_default_pose(h, p->res, p->width, p->height, pose12);
    return SSF_OK;
}

int ssf_navgrid_build(ssf_handle* h, const ssf_navgrid_params* p, const ssf_navgrid_out* out, ssf_navgrid_stats* stats) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    auto refuse = [&](const char* what) { h->err = std::string("ssf_navgrid_build: ") + what; return SSF_ERR_INVALID_ARG; };
    if (!out || (!out->zmin && !out->zmax && !out->hits && !out->state && !out->dist2)) return refuse("every output is NULL");
    NavCall c;
    c.who = "ssf_navgrid_build";
    { int rc = navgrid_begin(h, p, c); if (rc) return rc; }
    const size_t P = c.P;
    NavOut o{out->zmin, out->zmax, out->hits, out->state};
    int32_t* d2 = out->dist2;
    StagedIo io;                                                     // host outputs are staged on the device
    if (!p->on_device) {
        io.out(out->zmin, 4 * P, &o.zmin); io.out(out->zmax, 4 * P, &o.zmax); io.out(out->hits, 8 * P, &o.hits);
        io.out(out->state, P, &o.state); io.out(out->dist2, 4 * P, &d2);
    }
    { int rc = navgrid_reserve(h, p, c, io); if (rc) return rc; }
    TimerScope ts(h);
    { int rc = navgrid_accumulate(h, p, c); if (rc) return rc; }
    return navgrid_finish(h, p, c, o, d2, io, launch_navgrid_cells, nullptr, stats);
}

}  // extern "C"
