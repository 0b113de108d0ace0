// ssf_navfrontier.hip -- the frontier of the navigation grid as regions (include/ssf_navfrontier.h) on gfx950: labelled, filtered,
// summed per region, with the gain of a look from each region's representative.
//
// What is computed is pinned in include/ssf_navfrontier.h (the restatement: tests/navfrontier_ref.py).  ssf_navfrontier_regions runs
//   * label, merge, flatten (k_navfrontier_roots, k_navfrontier_flatten): the members (step 1) and their connected components, with
//               connectivity 4 or 8 and membership as the only link rule, by the labeller of ssf_ccl.hpp: its scheme, its marks in
//               parent and label between the phases and the argument why it ends and loses no link are stated there.  What is the
//               frontier's own: members and merged pairs are counted; k_navfrontier_roots counts the roots of every 256 cells, the
//               slot code's scan turns the counts into offsets, and in k_navfrontier_flatten a root, whose parent word nobody needs
//               any more, keeps the running index of its region there as -2 - index (ascending grid index = ascending label);
//   * sums      the host reads the number of regions and grows the accumulators (NavFrontierAcc, one per region FOUND).
//               k_navfrontier_sums: one workgroup per tile again.  A member adds itself in LDS to the slot of the cell its parent
//               word names when that cell lies in the same tile (its local root, or for a local root the root it was hung under),
//               otherwise to its own; then every slot that holds something adds to its region's accumulator: 64-bit atomic adds
//               for the sums, atomicMin / atomicMax for the box, one 64-bit atomicMin on (cost << 32) | p for the representative.
//               So the global atomics are a few per (tile, local component), not per cell;
//   * table     k_navfrontier_keep: one thread per region: kept or not (step 4), counted per 256 regions; the scan again;
//               k_navfrontier_table: the kept regions' records at their offsets, up to max_regions;
//   * map       k_navfrontier_map: one thread per cell: the table index through label and accumulator;
//   * gain      k_navfrontier_gain: one workgroup per record of the table.  The (2 R + 1)^2 window around the representative is a
//               bitmap in LDS (at most 66049 bits); the 8 R rays go over the threads, an unknown cell is marked with an LDS atomicOr,
//               the count is a popcount reduction, and one word per region goes to global memory.
// The root of a set is its smallest index by construction (links go from the larger root to the smaller), integer sums, minima and
// maxima do not depend on arrival order, and the table is in label order: nothing here depends on scheduling.  The phases are
// separate launches: no workgroup ever waits for another.
//
// This file is NOT one of the product library's objects.  It is linked, with all of them, the carve and the plan, into
// libssf_hip_explore.so.
#include "ssf_navgrid.hpp"
#include "ssf_ccl.hpp"
#include "../../include/ssf_navfrontier.h"
#include <algorithm>

namespace ssf {

static_assert(NAV_TILE == CCL_TILE, "the label tile is ssf_ccl.hpp's");
enum : uint32_t { NF_INF = 0xFFFFFFFFu };
enum { NF_GAIN_WORDS = (257 * 257 + 31) / 32 };                   // the window's bitmap at R = 128
// the sums: members, pairs the merge looked at, regions found / too small / unreached / kept, the largest region
enum { NF_MEMBERS = 0, NF_PAIRS = 1, NF_FOUND = 2, NF_SMALL = 3, NF_UNREACHED = 4, NF_KEPT = 5, NF_LARGEST = 6, NF_STATS = 8 };

struct NavFrontierGrid { int W, H, ntx, nty; };
struct NavFrontierRule { int conn8, trav_only, min_dist2, min_cells, reachable_only, max_regions; };
// per region found, in label order.  rep = the least (cost << 32) | p over the members with a cost, ~0 = none; tix = the table index or -2
struct NavFrontierAcc {
    unsigned long long sum_x, sum_y, rep;
    uint32_t cells;
    int32_t x0, y0, x1, y1, label, tix, pad_;
};
static_assert(sizeof(NavFrontierAcc) == 56, "NavFrontierAcc");
static_assert(sizeof(ssf_navfrontier_region) == 56, "ssf_navfrontier_region");

// step 1 for a cell inside the grid
__device__ __forceinline__ bool nf_member(const NavFrontierGrid& G, const NavFrontierRule& r, const int8_t* __restrict__ state,
                                          const int32_t* __restrict__ dist2, int x, int y) {
    const size_t p = (size_t)y * G.W + x;
    if (state[p] != 0) return false;
    if (r.trav_only && dist2[p] < r.min_dist2) return false;
    return (x > 0 && state[p - 1] == -1) || (x + 1 < G.W && state[p + 1] == -1) || (y > 0 && state[p - G.W] == -1) ||
           (y + 1 < G.H && state[p + G.W] == -1);
}

// ---- label: one workgroup per tile ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navfrontier_label(NavFrontierGrid G, NavFrontierRule r, const int8_t* __restrict__ state,
                                                           const int32_t* __restrict__ dist2, int32_t* __restrict__ parent,
                                                           int32_t* __restrict__ label, unsigned long long* __restrict__ stats) {
    __shared__ int sp[NAV_CELLS];
    __shared__ uint8_t sm[NAV_CELLS];
    const int tx = blockIdx.x % G.ntx, ty = blockIdx.x / G.ntx, x0 = tx * NAV_TILE, y0 = ty * NAV_TILE;
    unsigned long long members = 0;
#pragma unroll
    for (int k = 0; k < NAV_CELLS / 256; k++) {
        const int i = k * 256 + threadIdx.x, x = x0 + (i % NAV_TILE), y = y0 + (i / NAV_TILE);
        const bool m = x < G.W && y < G.H && nf_member(G, r, state, dist2, x, y);
        sm[i] = m; members += m;
    }
    int root[NAV_CELLS / 256];
    ccl_tile_label(sp, r.conn8 != 0, [&](int i) { return sm[i] != 0; }, [](int, int) { return true; }, root);
    ccl_tile_store(G.W, G.H, x0, y0, root, parent, label);
    block_sums({members}, stats, NF_MEMBERS);
}

// ---- merge: one thread per cell on the high side of a tile border; the pairs whose two cells are members are counted -------------------
__global__ __launch_bounds__(256) void k_navfrontier_merge(NavFrontierGrid G, int conn8, int32_t* parent, unsigned long long* __restrict__ stats) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long pairs = 0;
    if (t < ccl_border_threads(G.W, G.H, G.ntx, G.nty)) pairs = ccl_merge(parent, G.W, G.H, G.ntx, t, conn8 != 0, [](int, int) { return true; });
    pairs = wave_sum(pairs);
    if (lane() == 0 && pairs) atomicAdd(&stats[NF_PAIRS], pairs);
}

// ---- flatten: the local roots walk to their root; then every other member takes its local root's label ---------------------------
__global__ __launch_bounds__(256) void k_navfrontier_roots(size_t P, const int32_t* __restrict__ parent, int32_t* __restrict__ label,
                                                           uint32_t* __restrict__ blocks) {
    __shared__ int part[4];
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool root = false;
    if (p < P && ccl_is_local_root(label, p)) {
        const int i = ccl_walk(parent, (int)p);
        label[p] = i;
        root = i == (int)p;
    }
    const int n = block_count256(root, part);
    if (threadIdx.x == 0) blocks[blockIdx.x] = (uint32_t)n;
}
// A root's parent word is read by nobody here (a cell that is no local root reads its own), so the root may keep its region's index there
__global__ __launch_bounds__(256) void k_navfrontier_flatten(size_t P, int32_t* __restrict__ parent, int32_t* __restrict__ label,
                                                             const uint32_t* __restrict__ blocks) {
    __shared__ int part[4];
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool root = false;
    if (p < P) {
        const int32_t l = label[p];
        ccl_flatten(parent, label, p, l);
        root = l == (int32_t)p;
    }
    const int rank = block_rank256(root, part);
    if (root) parent[p] = -2 - (int32_t)(blocks[blockIdx.x] + (uint32_t)rank);
}

// ---- sums: one workgroup per tile; LDS per (tile, slot), then a few global atomics per slot ------------------------------------------
__global__ __launch_bounds__(256) void k_navfrontier_clear(int n, NavFrontierAcc* __restrict__ acc) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= n) return;
    NavFrontierAcc a;
    a.sum_x = 0; a.sum_y = 0; a.rep = ~0ull; a.cells = 0; a.x0 = 0x7FFFFFFF; a.y0 = 0x7FFFFFFF; a.x1 = -1; a.y1 = -1; a.label = 0; a.tix = -2; a.pad_ = 0;
    acc[id] = a;
}
__global__ __launch_bounds__(256) void k_navfrontier_sums(NavFrontierGrid G, const int32_t* __restrict__ parent, const int32_t* __restrict__ label,
                                                          const uint32_t* __restrict__ cost, NavFrontierAcc* __restrict__ acc) {
    __shared__ uint32_t sn[NAV_CELLS], sx[NAV_CELLS], sy[NAV_CELLS], bx0[NAV_CELLS], by0[NAV_CELLS], bx1[NAV_CELLS], by1[NAV_CELLS];
    __shared__ unsigned long long skey[NAV_CELLS];
    const int tx = blockIdx.x % G.ntx, ty = blockIdx.x / G.ntx, x0 = tx * NAV_TILE, y0 = ty * NAV_TILE;
#pragma unroll
    for (int k = 0; k < NAV_CELLS / 256; k++) {
        const int i = k * 256 + threadIdx.x;
        sn[i] = 0u; sx[i] = 0u; sy[i] = 0u; bx0[i] = ~0u; by0[i] = ~0u; bx1[i] = 0u; by1[i] = 0u; skey[i] = ~0ull;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NAV_CELLS / 256; k++) {
        const int i = k * 256 + threadIdx.x, lx = i % NAV_TILE, ly = i / NAV_TILE, x = x0 + lx, y = y0 + ly;
        if (x >= G.W || y >= G.H) continue;
        const size_t p = (size_t)y * G.W + x;
        const int32_t v = parent[p];
        if (v == -1) continue;                                        // no member
        int slot = i;
        if (v >= 0) {                                                 // (a root holds -2 - index: its own slot)
            const int vx = v % G.W, vy = v / G.W;
            if ((vx >> NAV_TILE_SHIFT) == tx && (vy >> NAV_TILE_SHIFT) == ty) slot = (vy - y0) * NAV_TILE + (vx - x0);
        }
        atomicAdd(&sn[slot], 1u); atomicAdd(&sx[slot], (uint32_t)lx); atomicAdd(&sy[slot], (uint32_t)ly);
        atomicMin(&bx0[slot], (uint32_t)lx); atomicMin(&by0[slot], (uint32_t)ly); atomicMax(&bx1[slot], (uint32_t)lx); atomicMax(&by1[slot], (uint32_t)ly);
        if (cost) { const uint32_t c = cost[p]; if (c != NF_INF) atomicMin(&skey[slot], ((unsigned long long)c << 32) | (unsigned long long)p); }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NAV_CELLS / 256; k++) {
        const int i = k * 256 + threadIdx.x;
        const uint32_t n = sn[i];
        if (n == 0u) continue;                                        // (a slot that holds something is a member inside the grid)
        const size_t p = (size_t)(y0 + i / NAV_TILE) * G.W + (x0 + i % NAV_TILE);
        const int32_t root = label[p];
        NavFrontierAcc* a = &acc[-2 - parent[root]];
        atomicAdd(&a->cells, n);
        atomicAdd(&a->sum_x, (unsigned long long)sx[i] + (unsigned long long)n * (unsigned long long)x0);
        atomicAdd(&a->sum_y, (unsigned long long)sy[i] + (unsigned long long)n * (unsigned long long)y0);
        atomicMin(&a->x0, x0 + (int)bx0[i]); atomicMin(&a->y0, y0 + (int)by0[i]);
        atomicMax(&a->x1, x0 + (int)bx1[i]); atomicMax(&a->y1, y0 + (int)by1[i]);
        if (skey[i] != ~0ull) atomicMin(&a->rep, skey[i]);
        if (root == (int32_t)p) a->label = root;                      // (one cell per region: nobody else writes the word)
    }
}

// ---- table: kept or not, the scan, the records ---------------------------------------------------------------------------------------
__device__ __forceinline__ bool nf_small(const NavFrontierRule& r, const NavFrontierAcc& a) { return a.cells < (uint32_t)r.min_cells; }
__device__ __forceinline__ bool nf_kept(const NavFrontierRule& r, const NavFrontierAcc& a) {
    return !nf_small(r, a) && !(r.reachable_only && a.rep == ~0ull);
}
__global__ __launch_bounds__(256) void k_navfrontier_keep(NavFrontierRule r, int n, const NavFrontierAcc* __restrict__ acc, uint32_t* __restrict__ blocks,
                                                          unsigned long long* __restrict__ stats) {
    __shared__ int part[4];
    __shared__ unsigned long long red[4];
    const int id = blockIdx.x * 256 + threadIdx.x;
    bool kept = false;
    unsigned long long small = 0, unreached = 0, cells = 0;
    if (id < n) {
        const NavFrontierAcc a = acc[id];
        kept = nf_kept(r, a); small = nf_small(r, a); unreached = !kept && !small; cells = a.cells;
    }
    const int nk = block_count256(kept, part);
    if (threadIdx.x == 0) blocks[blockIdx.x] = (uint32_t)nk;
    block_sums({small, unreached}, stats, NF_SMALL);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long u = __shfl_xor(cells, o, 64); cells = u > cells ? u : cells; }
    if (lane() == 0) red[threadIdx.x >> 6] = cells;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
        atomicMax(&stats[NF_LARGEST], a > b ? a : b);
    }
}
__global__ __launch_bounds__(256) void k_navfrontier_table(NavFrontierGrid G, NavFrontierRule r, int n, NavFrontierAcc* __restrict__ acc,
                                                           const uint32_t* __restrict__ blocks, ssf_navfrontier_region* __restrict__ table) {
    __shared__ int part[4];
    const int id = blockIdx.x * 256 + threadIdx.x;
    NavFrontierAcc a;
    bool kept = false;
    if (id < n) { a = acc[id]; kept = nf_kept(r, a); }
    const int rank = block_rank256(kept, part);
    if (id >= n) return;
    const long long at = (long long)blocks[blockIdx.x] + rank;
    const int tix = kept && at < (long long)r.max_regions ? (int)at : -2;
    acc[id].tix = tix;
    if (tix < 0) return;
    const bool reached = a.rep != ~0ull;
    const int rp = reached ? (int)(uint32_t)(a.rep & 0xFFFFFFFFull) : a.label;
    ssf_navfrontier_region t;
    t.sum_x = (int64_t)a.sum_x; t.sum_y = (int64_t)a.sum_y; t.label = a.label; t.cells = (int32_t)a.cells;
    t.x0 = a.x0; t.y0 = a.y0; t.x1 = a.x1; t.y1 = a.y1; t.rep_x = rp % G.W; t.rep_y = rp / G.W;
    t.rep_cost = reached ? (uint32_t)(a.rep >> 32) : (uint32_t)NF_INF; t.gain = 0;
    table[tix] = t;
}

// ---- map: one thread per cell ------------------------------------------------------------------------------------------------------------
// (label and region may be the same array: a thread reads its own word before it writes it, and nobody else reads that word)
__global__ __launch_bounds__(256) void k_navfrontier_map(size_t P, const int32_t* __restrict__ parent, const int32_t* label, const NavFrontierAcc* __restrict__ acc,
                                                         int32_t* region) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int32_t l = label[p];
    region[p] = l < 0 ? -1 : acc[-2 - parent[l]].tix;
}

// ---- gain: one workgroup per record of the table (step 6) -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navfrontier_gain(NavFrontierGrid G, int R, int max_regions, const int8_t* __restrict__ state,
                                                          const unsigned long long* __restrict__ stats, ssf_navfrontier_region* __restrict__ table) {
    __shared__ uint32_t bits[NF_GAIN_WORDS];
    __shared__ int part[4];
    const unsigned long long kept = stats[NF_KEPT];
    if ((unsigned long long)blockIdx.x >= kept || (int)blockIdx.x >= max_regions) return;      // (the same for every thread)
    const int side = 2 * R + 1, words = (side * side + 31) / 32;
    for (int i = threadIdx.x; i < words; i += 256) bits[i] = 0u;
    const int ox = table[blockIdx.x].rep_x, oy = table[blockIdx.x].rep_y;
    __syncthreads();
    for (int j = threadIdx.x; j < 8 * R; j += 256) {
        // ray j ends on the window's rim: the top row left to right, the right column downwards, the bottom row right to left, the left column upwards
        const int q = j / (2 * R), o = j % (2 * R);
        const int dx = q == 0 ? -R + o : (q == 1 ? R : (q == 2 ? R - o : -R));
        const int dy = q == 0 ? -R : (q == 1 ? -R + o : (q == 2 ? R : R - o));
        const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, sgx = dx < 0 ? -1 : 1, sgy = dy < 0 ? -1 : 1;
        for (int s = 1; s <= R; s++) {
            const int ux = sgx * ((2 * ax * s + R) / (2 * R)), uy = sgy * ((2 * ay * s + R) / (2 * R));
            const int cx = ox + ux, cy = oy + uy;
            if (cx < 0 || cx >= G.W || cy < 0 || cy >= G.H) break;
            const int8_t v = state[(size_t)cy * G.W + cx];
            if (v == 100) break;
            if (v == -1) { const int b = (uy + R) * side + (ux + R); atomicOr(&bits[b >> 5], 1u << (b & 31)); }
        }
    }
    __syncthreads();
    int n = 0;
    for (int i = threadIdx.x; i < words; i += 256) n += __popc(bits[i]);
    n = wave_sum(n);
    if (lane() == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) table[blockIdx.x].gain = (part[0] + part[1]) + (part[2] + part[3]);
}

// ---- launches ---------------------------------------------------------------------------------------------------------------------------
static unsigned nf_blocks(size_t n) { return (unsigned)((n + 255) / 256); }
static void launch_navfrontier_label(hipStream_t st, const NavFrontierGrid& G, const NavFrontierRule& r, const int8_t* state, const int32_t* dist2,
                                     int32_t* parent, int32_t* label, unsigned long long* stats) {
    ScopedKernel sk("navfrontier_label", st);
    hipLaunchKernelGGL(k_navfrontier_label, dim3((unsigned)(G.ntx * G.nty)), dim3(256), 0, st, G, r, state, dist2, parent, label, stats);
}
static void launch_navfrontier_merge(hipStream_t st, const NavFrontierGrid& G, int conn8, int32_t* parent, unsigned long long* stats) {
    ScopedKernel sk("navfrontier_merge", st);
    const long long n = ccl_border_threads(G.W, G.H, G.ntx, G.nty);
    if (n > 0) hipLaunchKernelGGL(k_navfrontier_merge, dim3(nf_blocks((size_t)n)), dim3(256), 0, st, G, conn8, parent, stats);
}
static void launch_navfrontier_flatten(hipStream_t st, size_t P, int32_t* parent, int32_t* label, uint32_t* blocks, unsigned long long* stats) {
    ScopedKernel sk("navfrontier_flatten", st);
    const unsigned nb = nf_blocks(P);
    hipLaunchKernelGGL(k_navfrontier_roots, dim3(nb), dim3(256), 0, st, P, parent, label, blocks);
    launch_slots_scan(st, blocks, (int)nb, nullptr, &stats[NF_FOUND]);
    hipLaunchKernelGGL(k_navfrontier_flatten, dim3(nb), dim3(256), 0, st, P, parent, label, blocks);
}
static void launch_navfrontier_sums(hipStream_t st, const NavFrontierGrid& G, int n, const int32_t* parent, const int32_t* label, const uint32_t* cost,
                                    NavFrontierAcc* acc) {
    ScopedKernel sk("navfrontier_sums", st);
    hipLaunchKernelGGL(k_navfrontier_clear, dim3(nf_blocks((size_t)n)), dim3(256), 0, st, n, acc);
    hipLaunchKernelGGL(k_navfrontier_sums, dim3((unsigned)(G.ntx * G.nty)), dim3(256), 0, st, G, parent, label, cost, acc);
}
static void launch_navfrontier_table(hipStream_t st, const NavFrontierGrid& G, const NavFrontierRule& r, int n, NavFrontierAcc* acc, uint32_t* blocks,
                                     ssf_navfrontier_region* table, unsigned long long* stats) {
    ScopedKernel sk("navfrontier_table", st);
    const unsigned nb = nf_blocks((size_t)n);
    hipLaunchKernelGGL(k_navfrontier_keep, dim3(nb), dim3(256), 0, st, r, n, acc, blocks, stats);
    launch_slots_scan(st, blocks, (int)nb, nullptr, &stats[NF_KEPT]);
    hipLaunchKernelGGL(k_navfrontier_table, dim3(nb), dim3(256), 0, st, G, r, n, acc, blocks, table);
}
static void launch_navfrontier_map(hipStream_t st, size_t P, const int32_t* parent, const int32_t* label, const NavFrontierAcc* acc, int32_t* region) {
    ScopedKernel sk("navfrontier_map", st);
    hipLaunchKernelGGL(k_navfrontier_map, dim3(nf_blocks(P)), dim3(256), 0, st, P, parent, label, acc, region);
}
static void launch_navfrontier_gain(hipStream_t st, const NavFrontierGrid& G, int R, int max_regions, int blocks, const int8_t* state,
                                    const unsigned long long* stats, ssf_navfrontier_region* table) {
    ScopedKernel sk("navfrontier_gain", st);
    hipLaunchKernelGGL(k_navfrontier_gain, dim3((unsigned)blocks), dim3(256), 0, st, G, R, max_regions, state, stats, table);
}

}  // namespace ssf

extern "C" {
int ssf_navfrontier_default_params(const ssf_handle* h, ssf_navfrontier_params* p) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    std::memset(p, 0, sizeof(*p));
    p->width = 512; p->height = 512;
    p->connectivity = 8; p->min_cells = 1; p->max_regions = 4096; p->cost_weight = 1;
    return SSF_OK;
}

int ssf_navfrontier_regions(ssf_handle* h, const ssf_navfrontier_params* p, const int8_t* state, const int32_t* dist2, const uint32_t* cost,
                            const ssf_navfrontier_out* out, ssf_navfrontier_stats* stats) {
    using namespace ssf;
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    auto refuse = [&](const char* what) { h->err = std::string("ssf_navfrontier_regions: ") + what; return SSF_ERR_INVALID_ARG; };
    if (!state) return refuse("state is NULL");
    if (!out || (!out->region && !out->regions && !out->order)) return refuse("every output is NULL");
    if (p->width < 1 || p->width > 4096 || p->height < 1 || p->height > 4096) return refuse("the grid's size must be 1..4096 x 1..4096");
    if (p->connectivity != 4 && p->connectivity != 8) return refuse("connectivity must be 4 or 8");
    if (p->min_dist2 < 0) return refuse("min_dist2 must be >= 0");
    if (p->min_cells < 1) return refuse("min_cells must be >= 1");
    if (p->max_regions < 1 || p->max_regions > 65536) return refuse("max_regions must be 1..65536");
    if (p->gain_radius < 0 || p->gain_radius > 128) return refuse("gain_radius must be 0..128");
    if (p->cost_weight < 0 || p->cost_weight > (1 << 20) || p->gain_weight < 0 || p->gain_weight > (1 << 20) || p->size_weight < 0 ||
        p->size_weight > (1 << 20))
        return refuse("the weights must be 0..1 << 20");
    if (p->traversable_only && !dist2) return refuse("traversable_only needs dist2");
    if (p->reachable_only && !cost) return refuse("reachable_only needs cost");
    { int rc = model_at_rest(h, "ssf_navfrontier_regions", "groups no frontier"); if (rc) return rc; }

    const NavFrontierGrid G{p->width, p->height, (p->width + NAV_TILE - 1) / NAV_TILE, (p->height + NAV_TILE - 1) / NAV_TILE};
    const NavFrontierRule rule{p->connectivity == 8, p->traversable_only != 0, p->min_dist2, p->min_cells, p->reachable_only != 0, p->max_regions};
    const size_t P = (size_t)G.W * G.H, nb = (P + 255) / 256;
    const bool dev = p->on_device != 0, use_dist2 = rule.trav_only != 0;
    // the working buffers; host arrays are staged on the device
    NavFrontierWs& w = h->navfrontier;
    const int8_t* d_state = state; const int32_t* d_dist2 = use_dist2 ? dist2 : nullptr; const uint32_t* d_cost = cost;
    StagedIo io;
    if (!dev) { io.in(state, P, &d_state); io.in(d_dist2, 4 * P, &d_dist2); io.in(cost, 4 * P, &d_cost); }
    bool ok = true;
    if (!w.stats) ok = w.bufs.grow({{(void**)&w.stats, NF_STATS * sizeof(unsigned long long)}, {&w.table, 65536 * sizeof(ssf_navfrontier_region)}});
    if (ok && P > w.cells) {
        ok = w.bufs.grow({{(void**)&w.parent, 4 * P}, {(void**)&w.label, 4 * P}, {(void**)&w.cell_blocks, (nb + 1) * sizeof(uint32_t)}});
        if (ok) w.cells = P;
    }
    if (ok) ok = io.reserve(w.bufs, &w.io, &w.io_bytes, io.need());
    if (!ok) { h->err = "ssf_navfrontier_regions: allocation of the working buffers failed"; return SSF_ERR_DEVICE; }

    hipStream_t st = h->stream;
    TimerScope ts(h);
    HCK(io.copy_in(st));
    HCK(hipMemsetAsync(w.stats, 0, NF_STATS * sizeof(unsigned long long), st));
    launch_navfrontier_label(st, G, rule, d_state, d_dist2, w.parent, w.label, w.stats);
    HCK(hipGetLastError());
    launch_navfrontier_merge(st, G, rule.conn8, w.parent, w.stats);
    HCK(hipGetLastError());
    launch_navfrontier_flatten(st, P, w.parent, w.label, w.cell_blocks, w.stats);
    HCK(hipGetLastError());
    // the number of regions sizes the accumulators: the one look at the device before the end
    unsigned long long found = 0;
    HCK(hipMemcpyAsync(&found, w.stats + NF_FOUND, sizeof(found), hipMemcpyDeviceToHost, st));
    { int rc = sync_collect(h); if (rc) return rc; }
    const int nreg = (int)found;                                      // (at most P / 2 <= 2^23)
    if ((size_t)nreg > w.regions) {
        const size_t cap = std::max<size_t>((size_t)nreg, 4096);
        if (!w.bufs.grow({{&w.acc, cap * sizeof(NavFrontierAcc)}, {(void**)&w.region_blocks, ((cap + 255) / 256 + 1) * sizeof(uint32_t)}})) {
            h->err = "ssf_navfrontier_regions: allocation of the working buffers failed"; return SSF_ERR_DEVICE;
        }
        w.regions = cap;
    }
    NavFrontierAcc* acc = (NavFrontierAcc*)w.acc;
    ssf_navfrontier_region* table = (ssf_navfrontier_region*)w.table;
    const int in_table = std::min(nreg, p->max_regions);              // (an upper bound of the records written)
    if (nreg > 0) {
        launch_navfrontier_sums(st, G, nreg, w.parent, w.label, d_cost, acc);
        HCK(hipGetLastError());
        launch_navfrontier_table(st, G, rule, nreg, acc, w.region_blocks, table, w.stats);
        HCK(hipGetLastError());
        if (p->gain_radius > 0) {
            launch_navfrontier_gain(st, G, p->gain_radius, p->max_regions, in_table, d_state, w.stats, table);
            HCK(hipGetLastError());
        }
    }
    if (out->region) {                                                // (without a region, no cell is a member: acc is not read)
        int32_t* d_region = dev ? out->region : w.label;
        launch_navfrontier_map(st, P, w.parent, w.label, acc, d_region);
        HCK(hipGetLastError());
        if (!dev) HCK(hipMemcpyAsync(out->region, w.label, 4 * P, hipMemcpyDeviceToHost, st));
    }
    unsigned long long s[NF_STATS];
    // (the records are staged as 8-byte words in a container that nav's objects instantiate already: one of the record type would add
    // its instantiations to what the library exports, which is pinned to the entry points and the kernels)
    std::vector<double> staged((size_t)in_table * (sizeof(ssf_navfrontier_region) / 8));
    const ssf_navfrontier_region* recs = reinterpret_cast<const ssf_navfrontier_region*>(staged.data());
    HCK(hipMemcpyAsync(s, w.stats, sizeof(s), hipMemcpyDeviceToHost, st));
    if (in_table > 0) HCK(hipMemcpyAsync(staged.data(), table, (size_t)in_table * sizeof(ssf_navfrontier_region), hipMemcpyDeviceToHost, st));
    { int rc = sync_collect(h); if (rc) return rc; }
    const int written = (int)std::min<unsigned long long>(s[NF_KEPT], (unsigned long long)p->max_regions);
    if (out->regions && written > 0) std::memcpy(out->regions, recs, (size_t)written * sizeof(ssf_navfrontier_region));
    if (out->order) {                                                 // step 7: a total order, so std::sort has one answer
        auto key = [&](const ssf_navfrontier_region& r) {
            return (int64_t)r.rep_cost * p->cost_weight - (int64_t)r.gain * p->gain_weight - (int64_t)r.cells * p->size_weight;
        };
        for (int i = 0; i < written; i++) out->order[i] = i;
        std::sort(out->order, out->order + written, [&](int32_t a, int32_t b) {
            const ssf_navfrontier_region &ra = recs[(size_t)a], &rb = recs[(size_t)b];
            const bool ua = ra.rep_cost == NF_INF, ub = rb.rep_cost == NF_INF;
            if (ua != ub) return ub;
            const int64_t ka = key(ra), kb = key(rb);
            if (ka != kb) return ka < kb;
            return ra.label < rb.label;
        });
    }
    if (stats) {
        stats->frontier_cells = (int64_t)s[NF_MEMBERS]; stats->regions_found = (int64_t)s[NF_FOUND]; stats->regions_small = (int64_t)s[NF_SMALL];
        stats->regions_unreached = (int64_t)s[NF_UNREACHED]; stats->regions_kept = (int64_t)s[NF_KEPT]; stats->regions_written = written;
        stats->largest_cells = (int64_t)s[NF_LARGEST]; stats->gain_rays = (int64_t)8 * p->gain_radius * written; stats->merge_pairs = (int64_t)s[NF_PAIRS];
    }
    return SSF_OK;
}
}  // extern "C"
