// ssf_navsteer_walk.hpp -- the rollouts of include/ssf_navsteer.h, once: the step, the arc's walk, the admissible test, the score, the
// chunk's winner, the winner's replay, and the host side of a call (refusals, rule, staging of host arrays, working buffers, stats).
// Generic over the CELL TEST: ssf_navsteer.hip walks the packed (traversable, d) word, staged in LDS or in the grid;
// ssf_navfoot.hip (include/ssf_navfoot.h) walks the (heading mask, d) word under the set of bins a step sweeps.
//
// A cell test is a small struct by value with
//     Need need(int h, int w) const                             what a step from heading h with turn w asks of a cell
//     bool free(int ix, int iy, Need need, int& d) const        (ix, iy) is in the grid: is it traversable under `need`; d(p) when it is
// and over the STEP HOOK: ssf_navdyn.hip (include/ssf_navdyn.h) tests every step that passed the cell test against the predicted
// movers and keeps the smallest gap; the two older files pass NsNoHook, which is empty and compiles to nothing.
//
// A step hook is a small struct by value, one per lane, with
//     bool step(int s, int nx, int ny)                          step s (1-based) to (nx, ny) passed the cell test: false ends the rollout
//     long long term() const                                    what the rollout adds to its score
//     void store(size_t q, bool start_ok) const                 the candidate's own outputs, at q = pose * K + c
//     void pick(int pose, bool won) const                       the pose's own outputs, after the winner's replay
//     bool ended() const; static constexpr bool counts          the rollout was ended by the hook; whether the launch sums that
// The two cell tests (the disc's packed word, the footprint's (mask, d) word) and the disc's roll frame live here as well, so that
// ssf_navdyn.hip instantiates the very code the older kernels do.
// Everything is __forceinline__ or static: a file that includes this gains no symbol but its own kernels.
// Private to the library's own files: nothing here is exported.
#pragma once
#include "ssf_navgrid.hpp"
#include "../../include/ssf_navsteer.h"
#include "../../include/ssf_navdyn.h"
#include <cmath>

namespace ssf {

enum : uint32_t { NS_TRAV = 0x80000000u, NS_D = 0x7FFFFFFFu, NS_NO_COST = 0xFFFFFFFFu };
enum { NS_DIRS = 1024 };
// the sums: admissible, collided, steps taken, workgroups that walked LDS / the grid, poses of status 0 / 1 or 2 / 3
// and, with a step hook that counts, the rollouts it ended
enum { NS_ADM = 0, NS_COLL = 1, NS_STEPS = 2, NS_STAGED = 3, NS_GLOBAL = 4, NS_OK = 5, NS_BLOCKED = 6, NS_STUCK = 7, NS_HOOKED = 8, NS_STATS = 9 };

struct NavSteerRule {
    int W, H, min_dist2, allow_unknown, cap;
    int n_poses, n_v, n_w, K, v_min, v_step, w_min, w_step, T, min_free, brake_div, v_abs_max;
    int wc, wt, wl, ws, wr;
    int R, walk, stage_cells;         // stage_cells: the largest window that is staged, 0 with walk = 1
};
struct NavSteerCand {                 // nullptr = not produced
    int32_t* free_steps; int32_t* min_d; int32_t* end; uint32_t* end_cost; long long* score;
};
struct NavSteerPose {
    int32_t* best; int32_t* cmd; long long* score; int32_t* n_adm; int32_t* status; int32_t* len; int32_t* traj;
};

__device__ __forceinline__ int ns_cos(uint32_t w) { return (int)(int16_t)(w & 0xFFFFu); }
__device__ __forceinline__ int ns_sin(uint32_t w) { return (int)(int16_t)(w >> 16); }
// one step of step 4 from (x, y, h): the state it would commit
__device__ __forceinline__ void ns_step(uint32_t dir, int v, int x, int y, int& nx, int& ny) {
    nx = x + ((v * ns_cos(dir) + 8192) >> 14);
    ny = y + ((v * ns_sin(dir) + 8192) >> 14);
}
__device__ __forceinline__ int ns_dir_index(int h, int w) { return ((2 * h + w + 64) >> 7) & (NS_DIRS - 1); }

// the step hook of a rollout that nothing but the grid ends
struct NsNoHook {
    static constexpr bool counts = false;
    __device__ __forceinline__ bool step(int, int, int) { return true; }
    __device__ __forceinline__ long long term() const { return 0; }
    __device__ __forceinline__ void store(size_t, bool) const {}
    __device__ __forceinline__ void pick(int, bool) const {}
    __device__ __forceinline__ bool ended() const { return false; }
};

// the arc of step 4 from a traversable start: (x, y, h) in the cell (ccx, ccy) becomes the END; commit(x, y, h, d) sees every committed
// step with d of its cell.  Returns free_steps.  dirs: the packed direction table, wherever it lies.  The hook sees a step after the
// cell test has passed it
template <class Cells, class Hook, class Commit>
__device__ __forceinline__ int ns_walk(const NavSteerRule& r, const Cells& cells, const uint32_t* dirs, int v, int w, int& x, int& y, int& h, int& ccx,
                                       int& ccy, Hook& hook, Commit commit) {
    int nfree = 0;
    for (int s = 0; s < r.T; s++) {
        int nx, ny;
        ns_step(dirs[ns_dir_index(h, w)], v, x, y, nx, ny);
        const int ncx = nx >> 10, ncy = ny >> 10;
        if (ncx < 0 || ncx >= r.W || ncy < 0 || ncy >= r.H) break;
        const auto need = cells.need(h, w);
        int d, e;
        if (!cells.free(ncx, ncy, need, d)) break;
        if (ncx != ccx && ncy != ccy && (!cells.free(ncx, ccy, need, e) || !cells.free(ccx, ncy, need, e))) break;
        if (!hook.step(s + 1, nx, ny)) break;
        x = nx; y = ny; h = (h + w) & 0xFFFF; ccx = ncx; ccy = ncy; nfree++;
        commit(x, y, h, d);
    }
    return nfree;
}

// steps 4 to 7 of one workgroup of 256: candidate c = blockIdx.x * 256 + threadIdx.x of pose blockIdx.y, from (px, py, ph) in the cell
// (cx0, cy0); start_ok and start_d: the start cell's test and d (the same for every thread); s_dir: the direction table in LDS;
// staged: what the workgroup counts itself as; hook: the lane's step hook, fresh.  The caller has synchronised the workgroup after
// filling s_dir
template <class Cells, class Hook>
__device__ __forceinline__ void ns_roll_body(const NavSteerRule& r, const Cells& cells, Hook hook, bool start_ok, int start_d, bool staged, int px, int py,
                                             int ph, int cx0, int cy0, const uint32_t* s_dir, const uint32_t* __restrict__ cost,
                                             const int32_t* __restrict__ targets, unsigned long long* __restrict__ keys, int32_t* __restrict__ n_adm,
                                             const NavSteerCand& out, unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long s_key[4];
    const int t = threadIdx.x, pose = blockIdx.y;
    const int c = (int)blockIdx.x * 256 + t;
    unsigned long long key = ~0ull, n_ok = 0, n_coll = 0, n_steps = 0, n_hooked = 0;
    if (c < r.K) {
        const int i = c / r.n_w, j = c - i * r.n_w;
        const int v = r.v_min + i * r.v_step, w = r.w_min + j * r.w_step;
        const int av = v < 0 ? -v : v, aw = w < 0 ? -w : w;
        int x = px, y = py, h = ph, nfree = 0, min_d = -1;
        uint32_t ec = NS_NO_COST;
        long long score = -1;
        if (start_ok) {
            min_d = start_d;
            int ccx = cx0, ccy = cy0;
            nfree = ns_walk(r, cells, s_dir, v, w, x, y, h, ccx, ccy, hook, [&](int, int, int, int d) { min_d = d < min_d ? d : min_d; });
            if (r.wc > 0) ec = cost[(size_t)ccy * r.W + ccx];
            int need = r.min_free + (r.brake_div > 0 ? (av + r.brake_div - 1) / r.brake_div : 0);
            need = need < r.T ? need : r.T;
            if (nfree >= need && !(r.wc > 0 && ec == NS_NO_COST)) {
                score = (long long)r.wl * (r.cap - min_d) + (long long)r.ws * (r.v_abs_max - av) + (long long)r.wr * aw + hook.term();
                if (r.wc > 0) score += (long long)r.wc * (long long)ec;
                if (r.wt > 0) {
                    long long dx = (long long)x - targets[2 * (size_t)pose], dy = (long long)y - targets[2 * (size_t)pose + 1];
                    dx = dx < 0 ? -dx : dx; dy = dy < 0 ? -dy : dy;
                    const long long hi = dx > dy ? dx : dy, lo = dx > dy ? dy : dx;
                    score += (long long)r.wt * ((10 * hi + 4 * lo) >> 10);
                }
                key = ((unsigned long long)score << 16) | (unsigned long long)c;     // score < 2^44 (ssf_navdyn.h: with the hook's term too), c < 2^16
                n_ok = 1;
            }
        }
        n_coll = nfree < r.T; n_steps = (unsigned long long)nfree;
        const size_t q = (size_t)pose * r.K + c;
        if (out.free_steps) out.free_steps[q] = nfree;
        if (out.min_d) out.min_d[q] = min_d;
        if (out.end) { out.end[3 * q] = x; out.end[3 * q + 1] = y; out.end[3 * q + 2] = h; }
        if (out.end_cost) out.end_cost[q] = ec;
        if (out.score) out.score[q] = score;
        hook.store(q, start_ok);
        n_hooked = hook.ended();
    }
    // the chunk's winner and sums
    key = wave_min64(key);
    if (lane() == 0) s_key[t >> 6] = key;
    __syncthreads();
    if (t == 0) {
        const unsigned long long a = s_key[0] < s_key[1] ? s_key[0] : s_key[1], b = s_key[2] < s_key[3] ? s_key[2] : s_key[3];
        const unsigned long long m = a < b ? a : b;
        if (m != ~0ull) atomicMin(&keys[pose], m);
        if (start_ok) atomicAdd(&stats[staged ? NS_STAGED : NS_GLOBAL], 1ull);
    }
    const unsigned long long sum = block_sums({n_ok, n_coll, n_steps}, stats, NS_ADM);
    if (t == 0 && sum) atomicAdd(&n_adm[pose], (int32_t)sum);         // (thread 0 holds the first sum)
    if constexpr (Hook::counts) block_sums({n_hooked}, stats, NS_HOOKED);
}

// steps 7 and 8 of one workgroup of 256, one lane per pose.  start(cx, cy, heading): the start cell's test (the cell is in the grid);
// hook: the lane's step hook, fresh: the replay ends where the rollout did
template <class Cells, class Hook, class Start>
__device__ __forceinline__ void ns_pick_body(const NavSteerRule& r, const Cells& cells, Hook hook, Start start, const int32_t* __restrict__ poses,
                                             const uint32_t* __restrict__ dirs, const unsigned long long* __restrict__ keys,
                                             const int32_t* __restrict__ n_adm, const NavSteerPose& out, unsigned long long* __restrict__ stats) {
    const int pose = (int)blockIdx.x * 256 + threadIdx.x;
    unsigned long long n_ok = 0, n_blocked = 0, n_stuck = 0;
    if (pose < r.n_poses) {
        const int px = poses[3 * (size_t)pose], py = poses[3 * (size_t)pose + 1], ph = poses[3 * (size_t)pose + 2] & 0xFFFF;
        const int cx0 = px >> 10, cy0 = py >> 10;
        const bool inside = cx0 >= 0 && cx0 < r.W && cy0 >= 0 && cy0 < r.H;
        const bool start_ok = inside && start(cx0, cy0, ph);
        const unsigned long long key = keys[pose];
        const int status = !inside ? 1 : (!start_ok ? 2 : (key == ~0ull ? 3 : 0));
        int best = -1, v = 0, w = 0, len = 0;
        long long score = -1;
        if (status == 0) {
            best = (int)(key & 0xFFFFull); score = (long long)(key >> 16);
            const int i = best / r.n_w, j = best - i * r.n_w;
            v = r.v_min + i * r.v_step; w = r.w_min + j * r.w_step;
            // the winner's arc again (it was admissible: its start is traversable)
            int32_t* tr = out.traj ? out.traj + (size_t)pose * (size_t)(r.T + 1) * 3 : nullptr;
            int x = px, y = py, h = ph, ccx = cx0, ccy = cy0;
            if (tr) { tr[0] = x; tr[1] = y; tr[2] = h; }
            len = 1;
            ns_walk(r, cells, dirs, v, w, x, y, h, ccx, ccy, hook, [&](int sx, int sy, int sh, int) {
                if (tr) { tr[3 * len] = sx; tr[3 * len + 1] = sy; tr[3 * len + 2] = sh; }
                len++;
            });
        }
        if (out.best) out.best[pose] = best;
        if (out.cmd) { out.cmd[2 * (size_t)pose] = v; out.cmd[2 * (size_t)pose + 1] = w; }
        if (out.score) out.score[pose] = score;
        if (out.n_adm) out.n_adm[pose] = n_adm[pose];
        if (out.status) out.status[pose] = status;
        if (out.len) out.len[pose] = len;
        hook.pick(pose, status == 0);
        n_ok = status == 0; n_blocked = status == 1 || status == 2; n_stuck = status == 3;
    }
    block_sums({n_ok, n_blocked, n_stuck}, stats, NS_OK);
}

// ---- the disc (ssf_navsteer.h step 3) ------------------------------------------------------------------------------------------------
// the packed word of a cell: traversable, and d = min(max(dist2, 0), cap)
__device__ __forceinline__ uint32_t ns_disc_word(int s, int d, int min_dist2, int allow_unknown, int cap) {
    const bool trav = (s == 0 || (allow_unknown && s == -1)) && d >= min_dist2;
    const int dd = d < 0 ? 0 : (d > cap ? cap : d);
    return (trav ? (uint32_t)NS_TRAV : 0u) | (uint32_t)dd;
}

// the disc's cell test: the packed word, from the staged window when the cell lies in it, else from the grid
struct NavSteerCells {
    const uint32_t* pk; const uint32_t* win; int W, x0, y0, ww, wh; bool staged;
    __device__ __forceinline__ int need(int, int) const { return 0; }
    __device__ __forceinline__ uint32_t word(int ix, int iy) const {
        if (staged) {
            const int lx = ix - x0, ly = iy - y0;
            if ((unsigned)lx < (unsigned)ww && (unsigned)ly < (unsigned)wh) return win[ly * ww + lx];
        }
        return pk[(size_t)iy * W + ix];
    }
    __device__ __forceinline__ bool free(int ix, int iy, int, int& d) const {
        const uint32_t u = word(ix, iy);
        d = (int)(u & NS_D);
        return (u & NS_TRAV) != 0;
    }
};

// the disc's roll kernel, whole: the pose, its window of the grid staged in the launch's dynamic LDS where r.stage_cells allows, the
// direction table, then ns_roll_body.  s_dir: NS_DIRS words of the kernel's LDS
template <class Hook>
__device__ __forceinline__ void ns_disc_roll(const NavSteerRule& r, Hook hook, uint32_t* s_dir, const uint32_t* __restrict__ pk,
                                             const uint32_t* __restrict__ cost, const int32_t* __restrict__ poses, const int32_t* __restrict__ targets,
                                             const uint32_t* __restrict__ dirs, unsigned long long* __restrict__ keys, int32_t* __restrict__ n_adm,
                                             const NavSteerCand& out, unsigned long long* __restrict__ stats) {
    extern __shared__ uint32_t s_win[];                               // the staged window, row-major, ww cells a row
    const int t = threadIdx.x, pose = blockIdx.y;
    const int px = poses[3 * (size_t)pose], py = poses[3 * (size_t)pose + 1], ph = poses[3 * (size_t)pose + 2] & 0xFFFF;
    const int cx0 = px >> 10, cy0 = py >> 10;
    const bool inside = cx0 >= 0 && cx0 < r.W && cy0 >= 0 && cy0 < r.H;
    const uint32_t start = inside ? pk[(size_t)cy0 * r.W + cx0] : 0u;
    const bool start_ok = (start & NS_TRAV) != 0;                     // (the same for every thread)
    // the window of the pose, clipped to the grid
    const int x0 = cx0 - r.R > 0 ? cx0 - r.R : 0, y0 = cy0 - r.R > 0 ? cy0 - r.R : 0;
    const int x1 = cx0 + r.R < r.W - 1 ? cx0 + r.R : r.W - 1, y1 = cy0 + r.R < r.H - 1 ? cy0 + r.R : r.H - 1;
    const int ww = x1 - x0 + 1, wh = y1 - y0 + 1;
    const bool staged = start_ok && (long long)ww * wh <= r.stage_cells;
    if (start_ok) {
        for (int k = t; k < NS_DIRS; k += 256) s_dir[k] = dirs[k];
        if (staged) {
            const int n = ww * wh;
            for (int i = t; i < n; i += 256) { const int ly = i / ww, lx = i - ly * ww; s_win[i] = pk[(size_t)(y0 + ly) * r.W + (x0 + lx)]; }
        }
    }
    __syncthreads();
    const NavSteerCells cells{pk, s_win, r.W, x0, y0, ww, wh, staged};
    ns_roll_body(r, cells, hook, start_ok, (int)(start & NS_D), staged, px, py, ph, cx0, cy0, s_dir, cost, targets, keys, n_adm, out, stats);
}

// ---- the oriented footprint (ssf_navfoot.h step 3) -----------------------------------------------------------------------------------
// the packed word of cell p: (dist2 >= min_dist2 ? free_mask : 0, d); the mask is read only where dist2 lets it count
__device__ __forceinline__ uint2 ns_foot_word(const uint32_t* __restrict__ mask, const int32_t* __restrict__ dist2, size_t p, int min_dist2, int cap) {
    const int d = dist2[p];
    const int dd = d < 0 ? 0 : (d > cap ? cap : d);
    return make_uint2(d >= min_dist2 ? mask[p] : 0u, (uint32_t)dd);
}

// the footprint's cell test: the packed (mask, d) word in the grid under the bins a step sweeps
struct NavFootCells {
    const uint2* pk; int W, B, shift;
    __device__ __forceinline__ uint32_t bin_bit(int h) const { return 1u << (((h + (1 << (shift - 1))) >> shift) & (B - 1)); }
    __device__ __forceinline__ uint32_t need(int h, int w) const {
        const int a = h + (1 << (shift - 1)), b = a + w;
        const int lo = (a < b ? a : b) >> shift, hi = (a < b ? b : a) >> shift, n = hi - lo + 1;
        const uint32_t all = B == 32 ? 0xFFFFFFFFu : (1u << B) - 1u;
        if (n >= B) return all;
        const unsigned long long run = ((1ull << n) - 1ull) << (lo & (B - 1));       // n < B <= 32 bits from a bin below B: below 2^63
        return (uint32_t)(run | (run >> B)) & all;
    }
    __device__ __forceinline__ bool free(int ix, int iy, uint32_t need, int& d) const {
        const uint2 u = pk[(size_t)iy * W + ix];
        d = (int)u.y;
        return (u.x & need) == need;
    }
};

// the footprint's roll kernel, whole: nothing is staged
template <class Hook>
__device__ __forceinline__ void ns_foot_roll(const NavSteerRule& r, Hook hook, uint32_t* s_dir, int B, int shift, const uint2* __restrict__ pk,
                                             const uint32_t* __restrict__ cost, const int32_t* __restrict__ poses, const int32_t* __restrict__ targets,
                                             const uint32_t* __restrict__ dirs, unsigned long long* __restrict__ keys, int32_t* __restrict__ n_adm,
                                             const NavSteerCand& out, unsigned long long* __restrict__ stats) {
    const int t = threadIdx.x, pose = blockIdx.y;
    const int px = poses[3 * (size_t)pose], py = poses[3 * (size_t)pose + 1], ph = poses[3 * (size_t)pose + 2] & 0xFFFF;
    const int cx0 = px >> 10, cy0 = py >> 10;
    const NavFootCells cells{pk, r.W, B, shift};
    const bool inside = cx0 >= 0 && cx0 < r.W && cy0 >= 0 && cy0 < r.H;
    const uint2 start = inside ? pk[(size_t)cy0 * r.W + cx0] : make_uint2(0u, 0u);
    const bool start_ok = (start.x & cells.bin_bit(ph)) != 0;          // (the same for every thread)
    if (start_ok)
        for (int k = t; k < NS_DIRS; k += 256) s_dir[k] = dirs[k];
    __syncthreads();
    ns_roll_body(r, cells, hook, start_ok, (int)start.y, false, px, py, ph, cx0, cy0, s_dir, cost, targets, keys, n_adm, out, stats);
}

}  // namespace ssf

// ---- the host side of a call ----------------------------------------------------------------------------------------------------
#pragma GCC visibility push(hidden)
// what a launch of the disc's roll kernel stages: ssf_navsteer.hip's measured choice, defined there with its constants (the library's
// own: no part of what it exports); no output depends on it
int navsteer_stage_cells(const ssf::NavSteerRule& r);
#pragma GCC visibility pop
namespace {

// the direction table of step 1, made once: C and S, and the device's packed word (S << 16) | (C & 0xFFFF)
struct NavSteerDirs {
    int32_t c[ssf::NS_DIRS], s[ssf::NS_DIRS];
    uint32_t packed[ssf::NS_DIRS];
    NavSteerDirs() {
        const double two_pi = 6.283185307179586476925286766559;
        for (int k = 0; k < ssf::NS_DIRS; k++) {
            const double a = two_pi * (double)k / 1024.0;
            c[k] = (int32_t)std::floor(16384.0 * std::cos(a) + 0.5);
            s[k] = (int32_t)std::floor(16384.0 * std::sin(a) + 0.5);
            packed[k] = ((uint32_t)(uint16_t)(int16_t)s[k] << 16) | (uint32_t)(uint16_t)(int16_t)c[k];
        }
    }
};
inline const NavSteerDirs& navsteer_dirs() { static const NavSteerDirs d; return d; }

// the disc: the dynamic LDS of its roll kernel (the largest clipped window of any pose, capped at what is staged: a pose whose window
// is larger walks the grid), and the packed grid of h->navsteer.  What a launch stages is navsteer_stage_cells (below)
inline size_t navsteer_window_lds(const ssf::NavSteerRule& r) {
    const long long side = 2LL * r.R + 1;
    const long long bound = std::min<long long>(side, r.W) * std::min<long long>(side, r.H);
    return 4 * (size_t)std::min<long long>(bound, r.stage_cells);
}
inline bool navsteer_reserve_pk(ssf_handle* h, size_t P) {
    NavSteerWs& w = h->navsteer;
    if (P <= w.cells) return true;
    if (!w.bufs.grow({{(void**)&w.pk, 4 * P}})) return false;
    w.cells = P;
    return true;
}
// the footprint: the 8-byte packed grid of h->navfoot (log2 of a legal n_headings: nav_log2_bins, ssf_navgrid.hpp)
inline bool navfoot_reserve_pk(ssf_handle* h, size_t P) {
    NavFootWs& w = h->navfoot;
    if (P <= w.pk_cells) return true;
    if (!w.bufs.grow({{(void**)&w.pk, 8 * P}})) return false;
    w.pk_cells = P;
    return true;
}

// what include/ssf_navdyn.h adds to a rollouts call.  navsteer_call refuses what that header refuses, stages the list and the three
// outputs with the rest, and fills in where they lie on the device before run.launch, which reads them from here
struct NavSteerMovers {
    const ssf_navdyn_params* p; const int32_t* movers; const ssf_navdyn_out* out; ssf_navdyn_stats* stats;
    const int32_t* d_movers; ssf_navdyn_out o;
};

// One rollouts call: the refusals of ssf_navsteer.h, the rule, the staging of host arrays, the working buffers of h->navsteer (keys,
// counts, direction table, sums, staging), the three launches and the stats.  `who` words the errors; `grid` is the first per-cell
// input (grid_bytes a cell: state, or the footprint's mask) and `grid_name` its name.  run.stage_cells(r): the largest window that is
// staged in LDS; run.reserve(P) grows the caller's own packed grid (false: allocation failed); run.launch(st, r, d_grid, d_dist2, d_cost, d_poses,
// d_targets, w, cand, pick) enqueues pack, roll and pick.  mv: the movers of ssf_navdyn.h, nullptr without them.
template <class Run>
int navsteer_call(ssf_handle* h, const char* who, const ssf_navsteer_params* p, const void* grid, size_t grid_bytes, const char* grid_name,
                  const int32_t* dist2, const uint32_t* cost, const int32_t* poses, const int32_t* targets, const ssf_navsteer_out* out,
                  ssf_navsteer_stats* stats, Run& run, NavSteerMovers* mv = nullptr) {
    using namespace ssf;
    if (!h || !p || (mv && !mv->p)) return SSF_ERR_INVALID_ARG;
    auto refuse = [&](const std::string& what) { h->err = std::string(who) + ": " + what; return SSF_ERR_INVALID_ARG; };
    if (!grid || !dist2) return refuse(std::string(grid_name) + " or dist2 is NULL");
    if (!poses) return refuse("poses is NULL");
    const bool no_out = !out || (!out->best && !out->best_cmd && !out->best_score && !out->n_admissible && !out->pose_status && !out->best_len &&
                                 !out->best_traj && !out->cand_free && !out->cand_min_d && !out->cand_end && !out->cand_end_cost && !out->cand_score);
    const bool no_mv_out = !mv || !mv->out || (!mv->out->cand_hit && !mv->out->cand_min_gap && !mv->out->best_min_gap);
    if (no_out && no_mv_out) return refuse("every output is NULL");
    if (p->width < 1 || p->width > 4096 || p->height < 1 || p->height > 4096) return refuse("the grid's size must be 1..4096 x 1..4096");
    if (p->min_dist2 < 0) return refuse("min_dist2 must be >= 0");
    if (p->allow_unknown != 0 && p->allow_unknown != 1) return refuse("allow_unknown must be 0 or 1");
    if (p->clearance_cap < 0 || p->clearance_cap > 1024 * 1024) return refuse("clearance_cap must be 0..1024 * 1024");
    if (p->n_v < 1 || p->n_v > 256) return refuse("n_v must be 1..256");
    if (p->n_w < 1 || p->n_w > 1024) return refuse("n_w must be 1..1024");
    if (p->n_v * p->n_w > 65536) return refuse("n_v * n_w must be <= 65536");
    const long long v_a = p->v_min, v_b = (long long)p->v_min + (long long)(p->n_v - 1) * p->v_step;
    const long long w_a = p->w_min, w_b = (long long)p->w_min + (long long)(p->n_w - 1) * p->w_step;
    const long long v_abs_max = std::max(v_a < 0 ? -v_a : v_a, v_b < 0 ? -v_b : v_b), w_abs_max = std::max(w_a < 0 ? -w_a : w_a, w_b < 0 ? -w_b : w_b);
    if (v_abs_max > 1024) return refuse("every |v| of the lattice must be <= 1024");
    if (w_abs_max > 16384) return refuse("every |w| of the lattice must be <= 16384");
    if (p->n_steps < 1 || p->n_steps > 256) return refuse("n_steps must be 1..256");
    if (p->n_poses < 1 || p->n_poses > 4096) return refuse("n_poses must be 1..4096");
    if ((long long)p->n_poses * p->n_v * p->n_w > (1LL << 24)) return refuse("n_poses * n_v * n_w must be <= 1 << 24");
    if (p->min_free_steps < 0 || p->min_free_steps > 256) return refuse("min_free_steps must be 0..256");
    if (p->brake_div < 0 || p->brake_div > 1024) return refuse("brake_div must be 0..1024");
    const int wts[6] = {p->cost_weight, p->target_weight, p->clear_weight, p->speed_weight, p->turn_weight, mv ? mv->p->mover_weight : 0};
    for (int k = 0; k < 6; k++)
        if (wts[k] < 0 || wts[k] > 1000) return refuse("every weight must be 0..1000");
    if (!(wts[0] | wts[1] | wts[2] | wts[3] | wts[4] | wts[5])) return refuse("the weights must not all be 0");
    if (p->cost_weight > 0 && !cost) return refuse("cost is NULL with cost_weight > 0");
    if (p->target_weight > 0 && !targets) return refuse("targets is NULL with target_weight > 0");
    if (p->walk != 0 && p->walk != 1) return refuse("walk must be 0 or 1");
    if (mv) {
        const ssf_navdyn_params& q = *mv->p;
        if (q.n_movers < 0 || q.n_movers > SSF_NAVDYN_MAX_MOVERS) return refuse("n_movers must be 0..64");
        if (q.mover_cap < 0 || q.mover_cap > 65536) return refuse("mover_cap must be 0..65536");
        if ((q.n_movers > 0) != (mv->movers != nullptr)) return refuse("movers must be NULL iff n_movers is 0");
        for (int m = 0; m < (p->on_device ? 0 : q.n_movers); m++) {           // (a device list is the caller's responsibility)
            const int32_t* e = mv->movers + 6 * m;
            if (e[0] < -(1 << 24) || e[0] > (1 << 24) || e[1] < -(1 << 24) || e[1] > (1 << 24)) return refuse("every mover's |x| and |y| must be <= 1 << 24");
            if (e[2] < -4096 || e[2] > 4096 || e[3] < -4096 || e[3] > 4096) return refuse("every mover's |vx| and |vy| must be <= 4096");
            if (e[4] < 0 || e[4] > (1 << 20)) return refuse("every mover's r must be 0..1 << 20");
            if (e[5] < 0 || e[5] > 4096) return refuse("every mover's grow must be 0..4096");
        }
    }
    { int rc = model_at_rest(h, who, "steers nothing"); if (rc) return rc; }

    NavSteerRule r{};
    r.W = p->width; r.H = p->height; r.min_dist2 = p->min_dist2; r.allow_unknown = p->allow_unknown; r.cap = p->clearance_cap;
    r.n_poses = p->n_poses; r.n_v = p->n_v; r.n_w = p->n_w; r.K = p->n_v * p->n_w; r.v_min = p->v_min; r.v_step = p->v_step; r.w_min = p->w_min;
    r.w_step = p->w_step; r.T = p->n_steps; r.min_free = p->min_free_steps; r.brake_div = p->brake_div; r.v_abs_max = (int)v_abs_max;
    r.wc = p->cost_weight; r.wt = p->target_weight; r.wl = p->clear_weight; r.ws = p->speed_weight; r.wr = p->turn_weight;
    r.R = (int)(((long long)r.T * v_abs_max + 1023) / 1024) + 1; r.walk = p->walk;
    r.stage_cells = run.stage_cells(r);           // the largest window staged in LDS (0: none); no output depends on it
    const size_t P = (size_t)r.W * r.H, np = (size_t)r.n_poses, NK = np * (size_t)r.K, traj = np * (size_t)(r.T + 1) * 3;
    const bool dev = p->on_device != 0;
    const uint32_t* use_cost = r.wc > 0 ? cost : nullptr;
    const int32_t* use_targets = r.wt > 0 ? targets : nullptr;

    // the arrays of a call with host pointers are staged on the device.  best_traj goes in as well as out: entries past best_len
    // keep what the caller had there
    const void* d_grid = grid; const int32_t* d_dist2 = dist2; const uint32_t* d_cost = use_cost; const int32_t* d_poses = poses;
    const int32_t* d_targets = use_targets;
    ssf_navsteer_out o{};
    if (out) o = *out;
    if (mv) { mv->d_movers = mv->movers; mv->o = ssf_navdyn_out{}; if (mv->out) mv->o = *mv->out; }
    StagedIo io;
    if (!dev) {
        io.in(grid, grid_bytes * P, &d_grid); io.in(dist2, 4 * P, &d_dist2); io.in(use_cost, 4 * P, &d_cost);
        io.in(poses, 12 * np, &d_poses); io.in(use_targets, 8 * np, &d_targets);
        io.out(o.best, 4 * np, &o.best); io.out(o.best_cmd, 8 * np, &o.best_cmd); io.out(o.best_score, 8 * np, &o.best_score);
        io.out(o.n_admissible, 4 * np, &o.n_admissible); io.out(o.pose_status, 4 * np, &o.pose_status); io.out(o.best_len, 4 * np, &o.best_len);
        io.inout(o.best_traj, 4 * traj, &o.best_traj);
        io.out(o.cand_free, 4 * NK, &o.cand_free); io.out(o.cand_min_d, 4 * NK, &o.cand_min_d); io.out(o.cand_end, 12 * NK, &o.cand_end);
        io.out(o.cand_end_cost, 4 * NK, &o.cand_end_cost); io.out(o.cand_score, 8 * NK, &o.cand_score);
        if (mv) {
            io.in(mv->movers, 24 * (size_t)mv->p->n_movers, &mv->d_movers);
            io.out(mv->o.cand_hit, 4 * NK, &mv->o.cand_hit); io.out(mv->o.cand_min_gap, 4 * NK, &mv->o.cand_min_gap);
            io.out(mv->o.best_min_gap, 4 * np, &mv->o.best_min_gap);
        }
    }
    // the working buffers
    NavSteerWs& w = h->navsteer;
    bool ok = true;
    if (!w.stats) {
        ok = w.bufs.grow({{(void**)&w.stats, NS_STATS * sizeof(unsigned long long)}, {(void**)&w.keys, 4096 * sizeof(unsigned long long)},
                          {(void**)&w.n_adm, 4096 * sizeof(int32_t)}, {(void**)&w.dirs, NS_DIRS * sizeof(uint32_t)}});
    }
    if (ok) ok = run.reserve(P);
    if (ok) ok = io.reserve(w.bufs, &w.io, &w.io_bytes, io.need());
    if (!ok) { h->err = std::string(who) + ": allocation of the working buffers failed"; return SSF_ERR_DEVICE; }

    hipStream_t st = h->stream;
    TimerScope ts(h);
    if (!w.dirs_sent) {
        HCK(hipMemcpyAsync(w.dirs, navsteer_dirs().packed, NS_DIRS * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        w.dirs_sent = true;
    }
    HCK(io.copy_in(st));
    // (the sums of a call without movers are the eight words they were: its fill and its copy are the ones the older libraries issue)
    const size_t n_sums = mv ? NS_STATS : NS_HOOKED;
    HCK(hipMemsetAsync(w.stats, 0, n_sums * sizeof(unsigned long long), st));
    HCK(hipMemsetAsync(w.keys, 0xFF, np * sizeof(unsigned long long), st));
    HCK(hipMemsetAsync(w.n_adm, 0, np * sizeof(int32_t), st));
    const NavSteerCand cand{o.cand_free, o.cand_min_d, o.cand_end, o.cand_end_cost, (long long*)o.cand_score};
    const NavSteerPose pick{o.best, o.best_cmd, (long long*)o.best_score, o.n_admissible, o.pose_status, o.best_len, o.best_traj};
    { int rc = run.launch(st, r, d_grid, d_dist2, d_cost, d_poses, d_targets, w, cand, pick); if (rc) return rc; }
    unsigned long long s[NS_STATS] = {};
    HCK(hipMemcpyAsync(s, w.stats, n_sums * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HCK(io.copy_out(st));
    { int rc = sync_collect(h); if (rc) return rc; }
    if (stats) {
        stats->poses_ok = (int64_t)s[NS_OK]; stats->poses_blocked = (int64_t)s[NS_BLOCKED]; stats->poses_stuck = (int64_t)s[NS_STUCK];
        stats->candidates = (int64_t)NK; stats->admissible = (int64_t)s[NS_ADM]; stats->collided = (int64_t)s[NS_COLL];
        stats->steps_taken = (int64_t)s[NS_STEPS];
        stats->windows_staged = (int64_t)s[NS_STAGED]; stats->windows_global = (int64_t)s[NS_GLOBAL];
    }
    if (mv && mv->stats) mv->stats->hit_movers = (int64_t)s[NS_HOOKED];
    return SSF_OK;
}

}  // namespace
