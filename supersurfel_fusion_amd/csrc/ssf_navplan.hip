// ssf_navplan.hip -- plan on the navigation grid (include/ssf_navplan.h) on gfx950: the cost-to-goal field and the paths down it.
//
// What is computed is pinned in include/ssf_navplan.h (the restatement: tests/navplan_ref.py).  ssf_navplan_field runs
//   * init     k_navplan_init: one thread per cell: traversable and penalty packed into one word, the frontier, cost = INF (0 on a
//              frontier goal); k_navplan_goals: one thread per goal entry: the goals at 0.  Both flag the 32 x 32 tiles that see a goal;
//   * relax    k_navplan_relax, one launch per ROUND, one workgroup per flagged 32 x 32 tile on its 34 x 34 window of cost and packed
//              word: the tile-round scheme of ssf_navfield.hpp, which also says why its racy reads are benign;
//   * stats    k_navplan_stats: reached cells and the largest cost;
//   * trace    k_navplan_trace: one wave per start, lanes 0..7 the eight moves, a wave minimum over (value, k).
//
// This file is NOT one of the product library's objects.  It is linked, with all of them and the carve, into libssf_hip_nav.so.
#include "ssf_navfield.hpp"
#include "../../include/ssf_navplan.h"
#include "../../include/ssf_navplan_testing.h"

namespace ssf {

enum { NP_WIN = NAV_TILE + 2, NP_WIN_CELLS = NP_WIN * NP_WIN };
enum : uint32_t { NP_INF = NAVF_INF, NP_TRAV = 0x80000000u };
// the sums: traversable cells, frontier cells, frontier goals, goal entries used / blocked / outside, reached cells, largest cost,
// (round, tile) visits, the last round that worked + 1, the set words of the two flag arrays
enum { NP_NTRAV = 0, NP_NFRONT = 1, NP_FGOALS = 2, NP_GUSED = 3, NP_GBLOCKED = 4, NP_GOUTSIDE = 5, NP_REACHED = 6, NP_MAXCOST = 7,
       NP_VISITS = 8, NP_ROUNDS = 9, NP_FLAGGED = 10, NP_STATS = 12 };
constexpr NavFieldSums NP_SUMS{NP_VISITS, NP_ROUNDS, NP_FLAGGED};
// the rounds launched between two looks at the flagged-tile count: 16 was the best or within 2 % of the best of 1, 4, 16, 64 on all
// three grids of tools/navplan_probe.py (profiles/navplan.txt).  One workgroup per tile, idle ones included, stays the launch form:
// with 256 tiles a round costs what its busiest tile costs (about 60 us), so a compacted list of flagged tiles was not built.
enum { NP_DEFAULT_BATCH = 16, NP_MAX_BATCH = 1024 };

struct NavPlanGrid { int W, H, ntx, nty; };
struct NavPlanRule { int min_dist2, soft_dist2, near_penalty, allow_unknown, frontier_goals; };

// ---- init: one thread per cell (steps 1, 2, 4 and the frontier's part of 5) ------------------------------------------------------
__global__ __launch_bounds__(256) void k_navplan_init(NavPlanGrid G, NavPlanRule r, const int8_t* __restrict__ state, const int32_t* __restrict__ dist2,
                                                      uint32_t* __restrict__ pk, uint32_t* __restrict__ cost, uint8_t* __restrict__ frontier,
                                                      uint32_t* __restrict__ flags, unsigned long long* __restrict__ stats) {
    const size_t P = (size_t)G.W * G.H, p = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long ntrav = 0, nfront = 0, ngoal = 0;
    if (p < P) {
        const int x = (int)(p % (size_t)G.W), y = (int)(p / (size_t)G.W);
        const int s = state[p], d = dist2[p];
        const bool trav = (s == 0 || (r.allow_unknown && s == -1)) && d >= r.min_dist2;
        const uint32_t pen = navfield_penalty(d, r.soft_dist2, r.near_penalty);
        const bool fr = s == 0 && ((x > 0 && state[p - 1] == -1) || (x + 1 < G.W && state[p + 1] == -1) ||
                                   (y > 0 && state[p - G.W] == -1) || (y + 1 < G.H && state[p + G.W] == -1));
        const bool goal = r.frontier_goals && fr && trav;
        pk[p] = (trav ? (uint32_t)NP_TRAV : 0u) | pen;
        cost[p] = goal ? 0u : (uint32_t)NP_INF;
        frontier[p] = fr ? 1 : 0;
        if (goal) navfield_flag_seers<NAV_TILE>(G.ntx, G.nty, x, y, flags, &stats[NP_FLAGGED]);
        ntrav = trav; nfront = fr; ngoal = goal;
    }
    block_sums({ntrav, nfront, ngoal}, stats, NP_NTRAV);
}

// goals: one thread per entry of the caller's list (step 5); runs behind k_navplan_init, so its zeros stay
__global__ __launch_bounds__(256) void k_navplan_goals(NavPlanGrid G, const int32_t* __restrict__ goals, int n, const uint32_t* __restrict__ pk,
                                                       uint32_t* __restrict__ cost, uint32_t* __restrict__ flags, unsigned long long* __restrict__ stats) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    unsigned long long used = 0, blocked = 0, outside = 0;
    if (g < n) {
        const int x = goals[2 * g], y = goals[2 * g + 1];
        if (x < 0 || x >= G.W || y < 0 || y >= G.H) outside = 1;
        else {
            const size_t p = (size_t)y * G.W + x;
            if (!(pk[p] & NP_TRAV)) blocked = 1;
            else {
                used = 1;
                cost[p] = 0u;
                navfield_flag_seers<NAV_TILE>(G.ntx, G.nty, x, y, flags, &stats[NP_FLAGGED]);
            }
        }
    }
    block_sums({used, blocked, outside}, stats, NP_GUSED);
}

// ---- relax: one round; one workgroup per tile, gone at once when the tile is not flagged ------------------------------------------
// Thread t owns the cells (t & 31, (t >> 5) + 8 j), j = 0..3, of its tile.  Inside LDS the sweep is racy on purpose: a thread may
// read a neighbour before or after its owner lowered it; the loop ends only after a sweep in which NO thread stored, and in that
// sweep every read saw the final values.  Window cells outside the grid hold (INF, not traversable).
__global__ __launch_bounds__(256) void k_navplan_relax(NavPlanGrid G, const uint32_t* __restrict__ pk, uint32_t* cost, uint32_t* fcur, uint32_t* fnxt,
                                                       unsigned long long* __restrict__ stats, int cur, unsigned long long round) {
    __shared__ uint32_t sc[NP_WIN_CELLS], sp[NP_WIN_CELLS];
    __shared__ uint32_t seers;
    if (!navfield_flagged(fcur)) return;
    const int t = blockIdx.x, tx = t % G.ntx, ty = t / G.ntx;
    const int x0 = tx * NAV_TILE - 1, y0 = ty * NAV_TILE - 1;
    for (int i = threadIdx.x; i < NP_WIN_CELLS; i += 256) {
        const int gx = x0 + i % NP_WIN, gy = y0 + i / NP_WIN;
        const bool in = gx >= 0 && gx < G.W && gy >= 0 && gy < G.H;
        const size_t p = in ? (size_t)gy * G.W + gx : 0;
        sc[i] = in ? cost[p] : (uint32_t)NP_INF;
        sp[i] = in ? pk[p] : 0u;
    }
    if (threadIdx.x == 0) seers = 0u;
    __syncthreads();
    const int lx = threadIdx.x & 31, ly0 = threadIdx.x >> 5;
    uint32_t old[4];
#pragma unroll
    for (int j = 0; j < 4; j++) old[j] = sc[(ly0 + 8 * j + 1) * NP_WIN + lx + 1];
    for (;;) {
        int changed = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int c = (ly0 + 8 * j + 1) * NP_WIN + lx + 1;
            if (!(sp[c] & NP_TRAV)) continue;
            const uint32_t have = sc[c];
            uint32_t best = have;
            const bool right = sp[c + 1] & NP_TRAV, down = sp[c + NP_WIN] & NP_TRAV, left = sp[c - 1] & NP_TRAV, up = sp[c - NP_WIN] & NP_TRAV;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int dx = navfield_dx(k), dy = navfield_dy(k), q = c + dy * NP_WIN + dx;
                const uint32_t pq = sp[q];
                bool ok = pq & NP_TRAV;
                if (k >= 4) ok = ok && (dx > 0 ? right : left) && (dy > 0 ? down : up);
                const uint32_t cq = sc[q];
                if (ok && cq != NP_INF) { const uint32_t v = cq + navfield_w(k) + (pq & ~(uint32_t)NP_TRAV); best = v < best ? v : best; }
            }
            if (best < have) { sc[c] = best; changed = 1; }
        }
        if (!__syncthreads_or(changed)) break;
    }
    uint32_t mine = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int ly = ly0 + 8 * j;
        const uint32_t now = sc[(ly + 1) * NP_WIN + lx + 1];
        if (now < old[j]) {                                           // (a lowered cell is traversable, so inside the grid)
            cost[(size_t)(y0 + 1 + ly) * G.W + (x0 + 1 + lx)] = now;
            mine |= navfield_seers<NAV_TILE>(lx, ly);
        }
    }
    navfield_publish(G.ntx, G.nty, mine, &seers, fcur, fnxt, stats, NP_SUMS, cur, round);
}

// ---- stats: reached cells and the largest cost ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navplan_stats(size_t P, const uint32_t* __restrict__ cost, unsigned long long* __restrict__ stats) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t c = p < P ? cost[p] : (uint32_t)NP_INF;
    block_sums({c != NP_INF}, stats, NP_REACHED);
    navfield_block_max(c != NP_INF ? c : 0u, &stats[NP_MAXCOST]);
}

// ---- trace: one wave per start (step 7) ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navplan_trace(NavPlanGrid G, const uint32_t* __restrict__ pk, const uint32_t* __restrict__ cost,
                                                       const int32_t* __restrict__ starts, int n, int max_path, uint32_t* __restrict__ start_cost,
                                                       int32_t* __restrict__ start_status, int32_t* __restrict__ path_len, int32_t* __restrict__ path) {
    const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (w >= n) return;
    const int ln = lane();
    int x = starts[2 * w], y = starts[2 * w + 1];
    int status = 0, len = 0;
    uint32_t c = NP_INF;
    if (x < 0 || x >= G.W || y < 0 || y >= G.H) status = 1;
    else if (!(pk[(size_t)y * G.W + x] & NP_TRAV)) status = 2;
    else { c = cost[(size_t)y * G.W + x]; if (c == NP_INF) status = 3; }
    const uint32_t c0 = c;
    if (status == 0 && max_path > 0) {
        int32_t* out = path + (size_t)w * (size_t)max_path * 2;
        for (;;) {                                                    // (wave-uniform: x, y, c, len are the same in every lane)
            if (len == max_path) { status = 4; break; }
            if (ln == 0 && path) { out[2 * (size_t)len] = x; out[2 * (size_t)len + 1] = y; }
            len++;
            if (c == 0u) break;
            unsigned long long key = ~0ull;
            uint32_t cq = NP_INF;
            if (ln < 8) {
                const int dx = navfield_dx(ln), dy = navfield_dy(ln), qx = x + dx, qy = y + dy;
                if (qx >= 0 && qx < G.W && qy >= 0 && qy < G.H) {
                    const uint32_t pq = pk[(size_t)qy * G.W + qx];
                    bool ok = pq & NP_TRAV;
                    if (ok && ln >= 4) ok = (pk[(size_t)y * G.W + qx] & NP_TRAV) && (pk[(size_t)qy * G.W + x] & NP_TRAV);
                    if (ok) {
                        cq = cost[(size_t)qy * G.W + qx];
                        if (cq != NP_INF) key = ((unsigned long long)(cq + navfield_w(ln) + (pq & ~(uint32_t)NP_TRAV)) << 3) | (unsigned long long)ln;
                    }
                }
            }
            key = wave_min64(key);
            if (key == ~0ull) { status = 3; break; }                  // (not on a settled field: a cell of finite cost > 0 has such a neighbour)
            const int k = (int)(key & 7ull);
            c = __shfl(cq, k, 64);
            x += navfield_dx(k); y += navfield_dy(k);
        }
    }
    if (ln == 0) { start_cost[w] = c0; start_status[w] = status; path_len[w] = len; }
}

static void launch_navplan_init(hipStream_t st, const NavPlanGrid& G, const NavPlanRule& r, const int8_t* state, const int32_t* dist2, uint32_t* pk,
                                uint32_t* cost, uint8_t* frontier, uint32_t* flags, unsigned long long* stats) {
    ScopedKernel sk("navplan_init", st);
    const size_t P = (size_t)G.W * G.H;
    hipLaunchKernelGGL(k_navplan_init, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, G, r, state, dist2, pk, cost, frontier, flags, stats);
}
static void launch_navplan_goals(hipStream_t st, const NavPlanGrid& G, const int32_t* goals, int n, const uint32_t* pk, uint32_t* cost, uint32_t* flags,
                                 unsigned long long* stats) {
    ScopedKernel sk("navplan_goals", st);
    hipLaunchKernelGGL(k_navplan_goals, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, G, goals, n, pk, cost, flags, stats);
}
static void launch_navplan_relax(hipStream_t st, const NavPlanGrid& G, const uint32_t* pk, uint32_t* cost, uint32_t* flags, unsigned long long* stats,
                                 long long round) {
    ScopedKernel sk("navplan_relax", st);
    const int tiles = G.ntx * G.nty, cur = (int)(round & 1);
    hipLaunchKernelGGL(k_navplan_relax, dim3((unsigned)tiles), dim3(256), 0, st, G, pk, cost, flags + (size_t)cur * tiles, flags + (size_t)(cur ^ 1) * tiles,
                       stats, cur, (unsigned long long)round);
}
static void launch_navplan_stats(hipStream_t st, size_t P, const uint32_t* cost, unsigned long long* stats) {
    ScopedKernel sk("navplan_stats", st);
    hipLaunchKernelGGL(k_navplan_stats, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, P, cost, stats);
}
static void launch_navplan_trace(hipStream_t st, const NavPlanGrid& G, const uint32_t* pk, const uint32_t* cost, const int32_t* starts, int n, int max_path,
                                 uint32_t* start_cost, int32_t* start_status, int32_t* path_len, int32_t* path) {
    ScopedKernel sk("navplan_trace", st);
    hipLaunchKernelGGL(k_navplan_trace, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, G, pk, cost, starts, n, max_path, start_cost, start_status,
                       path_len, path);
}

}  // namespace ssf

extern "C" {
int ssf_navplan_default_params(const ssf_handle* h, ssf_navplan_params* p) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    std::memset(p, 0, sizeof(*p));
    p->width = 512; p->height = 512;
    return SSF_OK;
}

int ssf_navplan_field(ssf_handle* h, const ssf_navplan_params* p, const int8_t* state, const int32_t* dist2, const ssf_navplan_out* out,
                      ssf_navplan_stats* stats) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    auto refuse = [&](const char* what) { h->err = std::string("ssf_navplan_field: ") + what; return SSF_ERR_INVALID_ARG; };
    if (!state || !dist2) return refuse("state or dist2 is NULL");
    if (!out || (!out->cost && !out->frontier && !out->start_cost && !out->start_status && !out->path_len && !out->path))
        return refuse("every output is NULL");
    if (p->width < 1 || p->width > 4096 || p->height < 1 || p->height > 4096) return refuse("the grid's size must be 1..4096 x 1..4096");
    if (p->min_dist2 < 0) return refuse("min_dist2 must be >= 0");
    if (p->soft_dist2 < 0 || p->soft_dist2 > 1024 * 1024) return refuse("soft_dist2 must be 0..1024 * 1024");
    if (p->near_penalty < 0 || p->near_penalty > 1000) return refuse("near_penalty must be 0..1000");
    if (p->n_goals < 0 || p->n_goals > 65536) return refuse("n_goals must be 0..65536");
    if (p->n_starts < 0 || p->n_starts > 4096) return refuse("n_starts must be 0..4096");
    if (p->max_path < 0 || p->max_path > (1 << 20)) return refuse("max_path must be 0..1 << 20");
    if (p->n_goals > 0 && !p->goals) return refuse("goals is NULL");
    if (p->n_starts > 0 && !p->starts) return refuse("starts is NULL");
    if (p->n_goals == 0 && !p->goals_from_frontier) return refuse("no goals: n_goals is 0 and goals_from_frontier is off");
    const size_t P = (size_t)p->width * p->height;
    if ((unsigned long long)(14 + p->near_penalty) * (unsigned long long)P >= 0xFFFFFFFFull)
        return refuse("(14 + near_penalty) * width * height must be < 2^32 - 1, so that no cost can wrap");
    { int rc = model_at_rest(h, "ssf_navplan_field", "plans on no navigation grid"); if (rc) return rc; }

    const NavPlanGrid G{p->width, p->height, (p->width + NAV_TILE - 1) / NAV_TILE, (p->height + NAV_TILE - 1) / NAV_TILE};
    const NavPlanRule rule{p->min_dist2, p->soft_dist2, p->near_penalty, p->allow_unknown != 0, p->goals_from_frontier != 0};
    const size_t tiles = (size_t)G.ntx * G.nty;
    const int ns = p->n_starts;
    const bool dev = p->on_device != 0, want_path = out->path && ns > 0 && p->max_path > 0;
    const size_t path_words = want_path ? (size_t)ns * (size_t)p->max_path * 2 : 0;
    // the working buffers; a host grid is staged on the device
    NavPlanWs& w = h->navplan;
    const int8_t* d_state = state; const int32_t* d_dist2 = dist2;
    StagedIo io;
    if (!dev) { io.in(state, P, &d_state); io.in(dist2, 4 * P, &d_dist2); }
    bool ok = navfield_reserve(w, NP_STATS, 2, tiles, dev ? 0 : path_words);
    if (ok && P > w.cells) {
        ok = w.bufs.grow({{(void**)&w.pk, 4 * P}, {(void**)&w.cost, 4 * P}, {(void**)&w.frontier, P}});
        if (ok) w.cells = P;
    }
    if (ok) ok = io.reserve(w.bufs, &w.io, &w.io_bytes, io.need());
    if (!ok) { h->err = "ssf_navplan_field: allocation of the working buffers failed"; return SSF_ERR_DEVICE; }

    hipStream_t st = h->stream;
    TimerScope ts(h);
    HCK(io.copy_in(st));
    if (p->n_goals > 0) HCK(hipMemcpyAsync(w.goals, p->goals, 2 * sizeof(int32_t) * (size_t)p->n_goals, hipMemcpyHostToDevice, st));
    if (ns > 0) HCK(hipMemcpyAsync(w.starts, p->starts, 2 * sizeof(int32_t) * (size_t)ns, hipMemcpyHostToDevice, st));
    HCK(hipMemsetAsync(w.stats, 0, NP_STATS * sizeof(unsigned long long), st));
    HCK(hipMemsetAsync(w.flags, 0, 2 * tiles * sizeof(uint32_t), st));
    launch_navplan_init(st, G, rule, d_state, d_dist2, w.pk, w.cost, w.frontier, w.flags, w.stats);
    HCK(hipGetLastError());
    if (p->n_goals > 0) { launch_navplan_goals(st, G, w.goals, p->n_goals, w.pk, w.cost, w.flags, w.stats); HCK(hipGetLastError()); }
    {                                                                 // the rounds, with the hook's batch
        int rc = navfield_rounds(h, "ssf_navplan_field", w.stats, NP_FLAGGED, (long long)P + 2, w.round_batch > 0 ? w.round_batch : NP_DEFAULT_BATCH,
                                 [&](long long round, int) { launch_navplan_relax(st, G, w.pk, w.cost, w.flags, w.stats, round); });
        if (rc) return rc;
    }
    launch_navplan_stats(st, P, w.cost, w.stats);
    HCK(hipGetLastError());
    int32_t* d_path = want_path ? (dev ? out->path : w.path) : nullptr;      // (no path array: the trace still tells length and status)
    if (ns > 0) {
        launch_navplan_trace(st, G, w.pk, w.cost, w.starts, ns, p->max_path, w.start_cost, w.start_status, w.path_len, d_path);
        HCK(hipGetLastError());
    }
    // the outputs
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    unsigned long long s[NP_STATS];
    HCK(hipMemcpyAsync(s, w.stats, sizeof(s), hipMemcpyDeviceToHost, st));
    if (out->cost) HCK(hipMemcpyAsync(out->cost, w.cost, 4 * P, kind, st));
    if (out->frontier) HCK(hipMemcpyAsync(out->frontier, w.frontier, P, kind, st));
    {
        int rc = navfield_copy_out(h, w, ns, p->max_path, 2, kind, out->start_cost, out->start_status, out->path_len, want_path && !dev ? out->path : nullptr);
        if (rc) return rc;
    }
    w.last_rounds = (long long)s[NP_ROUNDS]; w.last_visits = (long long)s[NP_VISITS];
    if (stats) {
        stats->cells_traversable = (int64_t)s[NP_NTRAV]; stats->cells_reached = (int64_t)s[NP_REACHED];
        stats->frontier_cells = (int64_t)s[NP_NFRONT]; stats->frontier_goals = (int64_t)s[NP_FGOALS];
        stats->goals_used = (int64_t)s[NP_GUSED]; stats->goals_blocked = (int64_t)s[NP_GBLOCKED]; stats->goals_outside = (int64_t)s[NP_GOUTSIDE];
        stats->max_cost = (int64_t)s[NP_MAXCOST]; stats->rounds = (int64_t)s[NP_ROUNDS]; stats->tile_visits = (int64_t)s[NP_VISITS];
    }
    return SSF_OK;
}

// test and measurement hooks of the plan (include/ssf_navplan_testing.h): the rounds per batch (0 = the default), and what the last call
// did: the rounds that worked and the tiles they visited
int ssf_debug_navplan_set_round_batch(ssf_handle* h, int rounds) {
    if (!h || rounds < 0 || rounds > NP_MAX_BATCH) return SSF_ERR_INVALID_ARG;
    h->navplan.round_batch = rounds;
    return SSF_OK;
}
int ssf_debug_navplan_last(const ssf_handle* h, int64_t* rounds, int64_t* tile_visits) {
    if (!h) return SSF_ERR_INVALID_ARG;
    if (rounds) *rounds = h->navplan.last_rounds;
    if (tile_visits) *tile_visits = h->navplan.last_visits;
    return SSF_OK;
}
}  // extern "C"
