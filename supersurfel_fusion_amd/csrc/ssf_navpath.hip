// ssf_navpath.hip -- any-angle waypoints from the cell paths of a plan (include/ssf_navpath.h) on gfx950.
//
// What is computed is pinned in include/ssf_navpath.h (the restatement: tests/navpath_ref.py).  ssf_navpath_waypoints runs
//   * pack     k_navpath_pack: one thread per cell: traversable and d = max(dist2, 0) in one word (the plan's idea, restated here:
//              ssf_navplan.hip is untouched);
//   * check    k_navpath_check: one workgroup per path, lanes stride over its cells: inside the grid, traversable, a distinct
//              8-neighbour of the cell before; a workgroup minimum gives the smallest status;
//   * pull     k_navpath_pull: one workgroup of 256 per path of status 0.  The anchor loop is serial and uniform over the workgroup.
//              Per anchor the window's cells (x, y, d) are staged in LDS (4096 x 12 bytes at most: the cap on lookahead), the running
//              minimum of d from the anchor is a scan over the window (with keep_clearance only), and the candidates are tested one
//              per lane from the far end of the window towards the anchor in chunks of 256: each lane walks its own segment and
//              leaves it at the first cell that fails; the first chunk in which any lane sees its candidate ends the search, and the
//              winner is the largest such candidate (an LDS maximum).  The lane that owns the winner has the segment's minimum
//              already and writes the waypoint.  When no candidate is visible the lane of a + 1, which walks its (at most four)
//              cells to the end whatever it finds, writes the forced step.
// No global atomics except the sums, no device-wide barrier, no inline assembly; nothing depends on the order the hardware works in.
//
// Bounds: the pull runs only on a path whose every cell the check found inside the grid, and every cell a walk visits lies in the
// bounding box of its two ends, so every read of the packed grid is inside it.  Path reads stop at path_len <= max_path.
//
// This file is NOT one of the product library's objects.  It is linked, with all of libssf_hip_explore.so's, into libssf_hip_drive.so.
#include "ssf_navgrid.hpp"
#include "../../include/ssf_navpath.h"

namespace ssf {

enum : uint32_t { NW_TRAV = 0x80000000u, NW_D = 0x7FFFFFFFu };
enum { NW_WIN = 4096, NW_NONE = 0x7FFFFFFF };
// the sums: paths of status 0 or 4, of status 1..3, of status 4; waypoints written; forced steps among them; cells of the checked
// paths; walks begun
enum { NW_OK = 0, NW_BAD = 1, NW_TRUNC = 2, NW_WP = 3, NW_FORCED = 4, NW_CELLS = 5, NW_SEGS = 6, NW_STATS = 8 };

struct NavPathGrid { int W, H; };
struct NavPathRule { int min_dist2, allow_unknown, base, keep, cap, lookahead; };

// ---- pack: one thread per cell (step 1) ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navpath_pack(size_t P, NavPathRule r, const int8_t* __restrict__ state, const int32_t* __restrict__ dist2,
                                                      uint32_t* __restrict__ pk) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int s = state[p], d = dist2[p];
    const bool trav = (s == 0 || (r.allow_unknown && s == -1)) && d >= r.min_dist2;
    pk[p] = (trav ? (uint32_t)NW_TRAV : 0u) | (uint32_t)(d < 0 ? 0 : d);
}

// ---- check: one workgroup per path (step 2) -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navpath_check(NavPathGrid G, const uint32_t* __restrict__ pk, const int32_t* __restrict__ path,
                                                       const int32_t* __restrict__ path_len, int max_path, int32_t* __restrict__ status,
                                                       unsigned long long* __restrict__ stats) {
    __shared__ int worst;
    const int i = blockIdx.x, L = path_len[i];
    if (L < 0 || L > max_path) {                                      // (the same for every thread)
        if (threadIdx.x == 0) { status[i] = 1; atomicAdd(&stats[NW_BAD], 1ull); }
        return;
    }
    if (threadIdx.x == 0) worst = NW_NONE;
    __syncthreads();
    const int32_t* c = path + (size_t)i * (size_t)max_path * 2;
    int mine = NW_NONE;
    for (int k = threadIdx.x; k < L; k += 256) {
        const int x = c[2 * (size_t)k], y = c[2 * (size_t)k + 1];
        if (x < 0 || x >= G.W || y < 0 || y >= G.H || !(pk[(size_t)y * G.W + x] & NW_TRAV)) mine = 2;
        else if (k > 0 && mine > 3) {
            const long long ddx = (long long)x - c[2 * (size_t)k - 2], ddy = (long long)y - c[2 * (size_t)k - 1];
            const long long ax = ddx < 0 ? -ddx : ddx, ay = ddy < 0 ? -ddy : ddy;
            if ((ax > ay ? ax : ay) != 1) mine = 3;
        }
    }
    if (mine != NW_NONE) atomicMin(&worst, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int s = worst == NW_NONE ? 0 : worst;
        status[i] = s;
        if (s) atomicAdd(&stats[NW_BAD], 1ull);
        else if (L) atomicAdd(&stats[NW_CELLS], (unsigned long long)L);
    }
}

// ---- the walk of step 3 from (ax, ay) to (bx, by): true iff every visited cell is traversable with d >= thr; m = the minimum d over
// the cells visited.  Without `full` the walk ends at the first cell that fails, and m is then of no use. -------------------------------
__device__ __forceinline__ bool nw_walk(const uint32_t* __restrict__ pk, int W, int ax, int ay, int bx, int by, int thr, bool full, int& m) {
    const int dx = bx > ax ? bx - ax : ax - bx, dy = by > ay ? by - ay : ay - by;
    const int sx = bx > ax ? 1 : (bx < ax ? -1 : 0), sy = by > ay ? 1 : (by < ay ? -1 : 0);
    int x = ax, y = ay, e = dx - dy, n = dx + dy;
    bool ok = true;
    m = NW_NONE;
    auto visit = [&](int vx, int vy) {
        const uint32_t v = pk[(size_t)vy * W + vx];
        const int d = (int)(v & NW_D);
        m = d < m ? d : m;
        ok = ok && (v & NW_TRAV) && d >= thr;
    };
    visit(x, y);
    while (n > 0 && (ok || full)) {
        if (e > 0) { x += sx; e -= 2 * dy; n -= 1; }
        else if (e < 0) { y += sy; e += 2 * dx; n -= 1; }
        else { visit(x + sx, y); visit(x, y + sy); x += sx; y += sy; e += 2 * dx - 2 * dy; n -= 2; }
        visit(x, y);
    }
    return ok;
}

// ---- pull: one workgroup per path (steps 4 to 6) ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navpath_pull(NavPathGrid G, NavPathRule r, const uint32_t* __restrict__ pk, const int32_t* __restrict__ path,
                                                      const int32_t* __restrict__ path_len, int max_path, int max_wp, int32_t* __restrict__ status,
                                                      int32_t* __restrict__ n_wp, int32_t* __restrict__ path_min, int32_t* __restrict__ wp,
                                                      unsigned long long* __restrict__ stats) {
    __shared__ int wx[NW_WIN], wy[NW_WIN], wd[NW_WIN];                // the window: cells a + 1 + k; wd becomes the running minimum from a
    __shared__ int part[256];
    __shared__ int s_best, s_seg, s_forced;
    const int i = blockIdx.x, t = threadIdx.x;
    const int st0 = status[i], L = path_len[i];                       // (the check's; the same for every thread)
    if (st0 != 0 || L == 0) {
        if (t == 0) { n_wp[i] = 0; path_min[i] = -1; if (st0 == 0) atomicAdd(&stats[NW_OK], 1ull); }
        return;
    }
    const int32_t* c = path + (size_t)i * (size_t)max_path * 2;
    int32_t* out = wp ? wp + (size_t)i * (size_t)max_wp * 4 : nullptr;
    int a = 0, count = 1, forced = 0, st = 0;
    unsigned long long segs = 0;
    int ax = c[0], ay = c[1];
    int ad = (int)(pk[(size_t)ay * G.W + ax] & NW_D);
    int pmin = ad;
    if (t == 0 && out) { out[0] = ax; out[1] = ay; out[2] = 0; out[3] = ad; }
    while (a < L - 1) {                                               // (uniform: a, count, ax, ay, ad are the same in every thread)
        if (count == max_wp) { st = 4; break; }
        const int n = (L - 1 - a < r.lookahead ? L - 1 - a : r.lookahead);        // candidates j = a + 1 + k, k = 0..n-1; 1 <= n <= NW_WIN
        __syncthreads();                                              // (the window of the anchor before is no longer read)
        for (int k = t; k < n; k += 256) {
            const int x = c[2 * (size_t)(a + 1 + k)], y = c[2 * (size_t)(a + 1 + k) + 1];
            wx[k] = x; wy[k] = y; wd[k] = (int)(pk[(size_t)y * G.W + x] & NW_D);
        }
        if (t == 0) s_best = -1;
        __syncthreads();
        if (r.keep) {                                                 // wd[k] = min(d(a), d(a + 1), .., d(a + 1 + k)): thread t owns S cells in a row
            const int S = (n + 255) >> 8, k0 = t * S, k1 = k0 + S < n ? k0 + S : n;
            int mine = NW_NONE;
            for (int k = k0; k < k1; k++) mine = wd[k] < mine ? wd[k] : mine;
            part[t] = mine;
            __syncthreads();
            for (int o = 1; o < 256; o <<= 1) {
                const int v = t >= o ? part[t - o] : NW_NONE;
                __syncthreads();
                if (v < part[t]) part[t] = v;
                __syncthreads();
            }
            int run = t > 0 ? part[t - 1] : NW_NONE;
            run = ad < run ? ad : run;
            for (int k = k0; k < k1; k++) { run = wd[k] < run ? wd[k] : run; wd[k] = run; }
            __syncthreads();
        }
        int win = 0;
        for (int hi = n - 1;; hi -= 256) {                            // a chunk: candidates hi, hi - 1, .., hi - 255, one per lane
            const int k = hi - t;
            bool vis = false;
            int smin = 0;
            if (k >= 0) {
                int thr = r.base;
                if (r.keep) { const int q = wd[k] < r.cap ? wd[k] : r.cap; thr = q > thr ? q : thr; }
                vis = nw_walk(pk, G.W, ax, ay, wx[k], wy[k], thr, k == 0, smin);
                segs++;
                if (vis) atomicMax(&s_best, k);
            }
            __syncthreads();
            const int best = s_best;
            __syncthreads();                                          // (everyone has read it before a later chunk may raise it)
            if (best >= 0 || hi < 256) {                              // seen, or the last chunk: then a + 1 it is, visible or not
                win = best >= 0 ? best : 0;
                if (k == win) {
                    s_seg = smin; s_forced = vis ? 0 : 1;
                    if (out) {
                        int32_t* o = out + 4 * (size_t)count;
                        o[0] = wx[k]; o[1] = wy[k]; o[2] = (a + 1 + k) | (vis ? 0 : SSF_NAVPATH_FORCED); o[3] = smin;
                    }
                }
                __syncthreads();
                break;
            }
        }
        pmin = s_seg < pmin ? s_seg : pmin;
        forced += s_forced;
        ax = wx[win]; ay = wy[win];
        a += 1 + win; count++;
        ad = (int)(pk[(size_t)ay * G.W + ax] & NW_D);
    }
    segs = wave_sum(segs);
    if (lane() == 0 && segs) atomicAdd(&stats[NW_SEGS], segs);
    if (t == 0) {
        n_wp[i] = count; path_min[i] = pmin; status[i] = st;
        atomicAdd(&stats[NW_OK], 1ull);
        if (st == 4) atomicAdd(&stats[NW_TRUNC], 1ull);
        atomicAdd(&stats[NW_WP], (unsigned long long)count);
        if (forced) atomicAdd(&stats[NW_FORCED], (unsigned long long)forced);
    }
}

static void launch_navpath_pack(hipStream_t st, size_t P, const NavPathRule& r, const int8_t* state, const int32_t* dist2, uint32_t* pk) {
    ScopedKernel sk("navpath_pack", st);
    hipLaunchKernelGGL(k_navpath_pack, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, P, r, state, dist2, pk);
}
static void launch_navpath_check(hipStream_t st, const NavPathGrid& G, const uint32_t* pk, const int32_t* path, const int32_t* path_len, int n, int max_path,
                                 int32_t* status, unsigned long long* stats) {
    ScopedKernel sk("navpath_check", st);
    hipLaunchKernelGGL(k_navpath_check, dim3((unsigned)n), dim3(256), 0, st, G, pk, path, path_len, max_path, status, stats);
}
static void launch_navpath_pull(hipStream_t st, const NavPathGrid& G, const NavPathRule& r, const uint32_t* pk, const int32_t* path, const int32_t* path_len,
                                int n, int max_path, int max_wp, int32_t* status, int32_t* n_wp, int32_t* path_min, int32_t* wp, unsigned long long* stats) {
    ScopedKernel sk("navpath_pull", st);
    hipLaunchKernelGGL(k_navpath_pull, dim3((unsigned)n), dim3(256), 0, st, G, r, pk, path, path_len, max_path, max_wp, status, n_wp, path_min, wp, stats);
}

}  // namespace ssf

extern "C" {
int ssf_navpath_default_params(const ssf_handle* h, ssf_navpath_params* p) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    std::memset(p, 0, sizeof(*p));
    p->width = 512; p->height = 512; p->lookahead = 256;
    return SSF_OK;
}

int ssf_navpath_waypoints(ssf_handle* h, const ssf_navpath_params* p, const int8_t* state, const int32_t* dist2, const int32_t* path,
                          const int32_t* path_len, const ssf_navpath_out* out, ssf_navpath_stats* stats) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    auto refuse = [&](const char* what) { h->err = std::string("ssf_navpath_waypoints: ") + what; return SSF_ERR_INVALID_ARG; };
    if (!state || !dist2) return refuse("state or dist2 is NULL");
    if (!path || !path_len) return refuse("path or path_len is NULL");
    if (!out || (!out->n_waypoints && !out->status && !out->waypoints && !out->path_min)) return refuse("every output is NULL");
    if (p->width < 1 || p->width > 4096 || p->height < 1 || p->height > 4096) return refuse("the grid's size must be 1..4096 x 1..4096");
    if (p->min_dist2 < 0) return refuse("min_dist2 must be >= 0");
    if (p->los_dist2 < 0) return refuse("los_dist2 must be >= 0");
    if (p->keep_clearance != 0 && p->keep_clearance != 1) return refuse("keep_clearance must be 0 or 1");
    if (p->clearance_cap < 0 || p->clearance_cap > 1024 * 1024) return refuse("clearance_cap must be 0..1024 * 1024");
    if (p->lookahead < 1 || p->lookahead > NW_WIN) return refuse("lookahead must be 1..4096");
    if (p->n_paths < 1 || p->n_paths > 4096) return refuse("n_paths must be 1..4096");
    if (p->max_path < 1 || p->max_path > (1 << 20)) return refuse("max_path must be 1..1 << 20");
    if (p->max_waypoints < 1 || p->max_waypoints > (1 << 20)) return refuse("max_waypoints must be 1..1 << 20");
    { int rc = model_at_rest(h, "ssf_navpath_waypoints", "refines no path"); if (rc) return rc; }

    const NavPathGrid G{p->width, p->height};
    const NavPathRule rule{p->min_dist2, p->allow_unknown != 0, p->min_dist2 > p->los_dist2 ? p->min_dist2 : p->los_dist2, p->keep_clearance,
                           p->clearance_cap, p->lookahead};
    const size_t P = (size_t)p->width * p->height;
    const int np = p->n_paths;
    const bool dev = p->on_device != 0;
    const size_t path_words = (size_t)np * (size_t)p->max_path * 2, wp_words = out->waypoints ? (size_t)np * (size_t)p->max_waypoints * 4 : 0;
    // the working buffers; the whole-array inputs of a host caller are staged on the device
    NavPathWs& w = h->navpath;
    const int8_t* d_state = state; const int32_t* d_dist2 = dist2; const int32_t* d_path = path; const int32_t* d_len = path_len;
    StagedIo io;
    if (!dev) { io.in(state, P, &d_state); io.in(dist2, 4 * P, &d_dist2); io.in(path_len, 4 * (size_t)np, &d_len); }
    bool ok = true;
    if (!w.stats) ok = w.bufs.grow({{(void**)&w.stats, NW_STATS * sizeof(unsigned long long)}, {(void**)&w.status, 4096 * sizeof(int32_t)},
                                    {(void**)&w.n_wp, 4096 * sizeof(int32_t)}, {(void**)&w.path_min, 4096 * sizeof(int32_t)}});
    if (ok && P > w.cells) { ok = w.bufs.grow({{(void**)&w.pk, 4 * P}}); if (ok) w.cells = P; }
    if (ok) ok = io.reserve(w.bufs, &w.io, &w.io_bytes, io.need());
    if (ok && !dev && path_words > w.path_words) { ok = w.bufs.grow({{(void**)&w.path, path_words * sizeof(int32_t)}}); if (ok) w.path_words = path_words; }
    if (ok && !dev && wp_words > w.wp_words) { ok = w.bufs.grow({{(void**)&w.wp, wp_words * sizeof(int32_t)}}); if (ok) w.wp_words = wp_words; }
    if (!ok) { h->err = "ssf_navpath_waypoints: allocation of the working buffers failed"; return SSF_ERR_DEVICE; }

    hipStream_t st = h->stream;
    TimerScope ts(h);
    HCK(io.copy_in(st));
    if (!dev) {
        for (int i = 0; i < np; i++) {                                // entries past path_len are not read: each path's cells, no more
            const int L = path_len[i];
            if (L > 0 && L <= p->max_path)
                HCK(hipMemcpyAsync(w.path + (size_t)i * p->max_path * 2, path + (size_t)i * p->max_path * 2, 8 * (size_t)L, hipMemcpyHostToDevice, st));
        }
        d_path = w.path;
    }
    HCK(hipMemsetAsync(w.stats, 0, NW_STATS * sizeof(unsigned long long), st));
    launch_navpath_pack(st, P, rule, d_state, d_dist2, w.pk);
    HCK(hipGetLastError());
    launch_navpath_check(st, G, w.pk, d_path, d_len, np, p->max_path, w.status, w.stats);
    HCK(hipGetLastError());
    int32_t* d_wp = out->waypoints ? (dev ? out->waypoints : w.wp) : nullptr;      // (no array: counts, statuses and minima all the same)
    launch_navpath_pull(st, G, rule, w.pk, d_path, d_len, np, p->max_path, p->max_waypoints, w.status, w.n_wp, w.path_min, d_wp, w.stats);
    HCK(hipGetLastError());
    // the outputs
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    unsigned long long s[NW_STATS];
    int32_t counts[4096];                                             // (n_paths <= 4096)
    HCK(hipMemcpyAsync(s, w.stats, sizeof(s), hipMemcpyDeviceToHost, st));
    if (out->n_waypoints) HCK(hipMemcpyAsync(out->n_waypoints, w.n_wp, 4 * (size_t)np, kind, st));
    if (out->status) HCK(hipMemcpyAsync(out->status, w.status, 4 * (size_t)np, kind, st));
    if (out->path_min) HCK(hipMemcpyAsync(out->path_min, w.path_min, 4 * (size_t)np, kind, st));
    if (out->waypoints && !dev) HCK(hipMemcpyAsync(counts, w.n_wp, 4 * (size_t)np, hipMemcpyDeviceToHost, st));
    { int rc = sync_collect(h); if (rc) return rc; }
    if (out->waypoints && !dev) {                                     // entries past n_waypoints are not written
        for (int i = 0; i < np; i++)
            if (counts[i] > 0)
                HCK(hipMemcpyAsync(out->waypoints + (size_t)i * p->max_waypoints * 4, w.wp + (size_t)i * p->max_waypoints * 4, 16 * (size_t)counts[i],
                                   hipMemcpyDeviceToHost, st));
        HCK(hipStreamSynchronize(st));
    }
    if (stats) {
        stats->paths_ok = (int64_t)s[NW_OK]; stats->paths_bad = (int64_t)s[NW_BAD]; stats->paths_truncated = (int64_t)s[NW_TRUNC];
        stats->waypoints = (int64_t)s[NW_WP]; stats->forced_steps = (int64_t)s[NW_FORCED]; stats->cells_in = (int64_t)s[NW_CELLS];
        stats->segments_tested = (int64_t)s[NW_SEGS];
    }
    return SSF_OK;
}
}  // extern "C"
