// ssf_navsteer.hip -- velocity commands on the navigation grid (include/ssf_navsteer.h) on gfx950: a lattice of (v, w) candidates
// rolled out from every pose, tested, scored, and the best one picked.
//
// What is computed is pinned in include/ssf_navsteer.h (the restatement: tests/navsteer_ref.py).  ssf_navsteer_rollouts runs
//   * pack   k_navsteer_pack: one thread per cell: traversable and d = min(max(dist2, 0), clearance_cap) in one word (the waypoints'
//            idea, restated here with the cap: ssf_navpath.hip is untouched);
//   * roll   k_navsteer_roll: one workgroup of 256 per (pose, chunk of 256 candidates), one candidate per lane.  Candidate
//            c = i * n_w + j: neighbouring lanes share v and differ in w, so the arcs of a wave fan out from one speed and their
//            early steps read the same few cells.  The reach of a pose is R = ceil(n_steps * v_abs_max / 1024) + 1 cells: a step
//            moves at most |v| sub-units along each axis (|C|, |S| <= 16384 and the rounding is to nearest), so every cell a rollout
//            tests lies in the (2 R + 1)^2 window around the start cell.  A window that, clipped to the grid, has at most
//            NS_LDS_CELLS cells may be staged in LDS and walked there; otherwise the lanes walk the packed grid in global memory
//            (1 MiB at 512 x 512: it sits in L2).  Both are the same rule.  Which one runs is a measured choice
//            (profiles/navsteer.txt): the staged walk is about a tenth faster while the machine is not full (1 and 16 poses, windows
//            of 1.2 k and of 10 k cells), ties at 8192 workgroups with 1.2 k cells, and LOSES at 4096 workgroups with 10 k cells
//            (0.65 against 0.41 ms) and at 65536 with up to 14 k (5.0 against 1.9 ms): the walk is a chain of dependent reads, what
//            hides it is waves per CU, and 40 to 60 KiB of LDS per workgroup leave two or three workgroups on a CU where the
//            global walk has eight.  So a launch stages every window that fits (a) when a workgroup's LDS leaves the CU its eight
//            workgroups (NS_LDS_FREE: 20 KiB, windows up to 4056 cells), or (b) when all of its workgroups are resident at once at
//            the occupancy their LDS leaves; otherwise it stages only the windows of (a).  The record is the packed 32-bit word as
//            it is: with 4 KiB for the direction table a workgroup holds 60 KiB at most.  At the default lattice (R = 17, 1225
//            cells, 4.8 KiB) LDS is not what bounds occupancy (32 VGPRs: eight waves per SIMD).  A narrower record would double
//            the side of (a)'s windows at the price of a second format for caps above 15 bits; nothing measured asks for it.
//            cost is read once per candidate, at its end cell, from global memory.  The chunk's smallest (score << 16) | c goes
//            through a wave minimum, LDS, and ONE 64-bit atomicMin per workgroup into the pose's slot; the admissible count likewise
//            with one atomicAdd;
//   * pick   k_navsteer_pick: one lane per pose: the status, the winner's command and score, and the winner's arc replayed into
//            best_traj from the packed grid.
// No device-wide barrier, no inline assembly; nothing depends on the order the hardware works in.
//
// Bounds: a cell is read only after the test that it lies in the grid; a read of the staged window tests the window's box as well
// and goes to the grid when outside (by the reach argument it never is).  Per-candidate arrays are written at pose * K + c with
// c < K; per-pose arrays at pose < n_poses; best_traj at most at entry n_steps of its pose.
//
// This file is NOT one of the product library's objects.  It is linked, with all of libssf_hip_live.so's, into libssf_hip_steer.so.
#include "ssf_navgrid.hpp"
#include "../../include/ssf_navsteer.h"
#include <cmath>

namespace ssf {

enum : uint32_t { NS_TRAV = 0x80000000u, NS_D = 0x7FFFFFFFu, NS_NO_COST = 0xFFFFFFFFu };
enum { NS_LDS_CELLS = 14336, NS_DIRS = 1024 };
// the roll kernel's static LDS (direction table, four keys, the sums); a CU's LDS, an eighth of it, and the CUs of the part
enum { NS_STATIC_LDS = 4 * NS_DIRS + 160, NS_CU_LDS = 160 * 1024, NS_LDS_FREE = NS_CU_LDS / 8, NS_CUS = 256 };
// the sums: admissible, collided, steps taken, workgroups that walked LDS / the grid, poses of status 0 / 1 or 2 / 3
enum { NS_ADM = 0, NS_COLL = 1, NS_STEPS = 2, NS_STAGED = 3, NS_GLOBAL = 4, NS_OK = 5, NS_BLOCKED = 6, NS_STUCK = 7, NS_STATS = 8 };

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

// ---- pack: one thread per cell (step 3) ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navsteer_pack(size_t P, int min_dist2, int allow_unknown, int cap, const int8_t* __restrict__ state,
                                                       const int32_t* __restrict__ dist2, uint32_t* __restrict__ pk) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int s = state[p], d = dist2[p];
    const bool trav = (s == 0 || (allow_unknown && s == -1)) && d >= min_dist2;
    const int dd = d < 0 ? 0 : (d > cap ? cap : d);
    pk[p] = (trav ? (uint32_t)NS_TRAV : 0u) | (uint32_t)dd;
}

__device__ __forceinline__ int ns_cos(uint32_t w) { return (int)(int16_t)(w & 0xFFFFu); }
__device__ __forceinline__ int ns_sin(uint32_t w) { return (int)(int16_t)(w >> 16); }
// one step of step 4 from (x, y, h): the state it would commit
__device__ __forceinline__ void ns_step(uint32_t dir, int v, int x, int y, int& nx, int& ny) {
    nx = x + ((v * ns_cos(dir) + 8192) >> 14);
    ny = y + ((v * ns_sin(dir) + 8192) >> 14);
}
__device__ __forceinline__ int ns_dir_index(int h, int w) { return ((2 * h + w + 64) >> 7) & (NS_DIRS - 1); }

// ---- roll: one workgroup per (pose, 256 candidates) (steps 4 to 7) ------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navsteer_roll(NavSteerRule r, const uint32_t* __restrict__ pk, const uint32_t* __restrict__ cost,
                                                       const int32_t* __restrict__ poses, const int32_t* __restrict__ targets,
                                                       const uint32_t* __restrict__ dirs, unsigned long long* __restrict__ keys,
                                                       int32_t* __restrict__ n_adm, NavSteerCand out, unsigned long long* __restrict__ stats) {
    extern __shared__ uint32_t s_win[];                               // the staged window, row-major, ww cells a row
    __shared__ uint32_t s_dir[NS_DIRS];                               // (S << 16) | (C & 0xFFFF)
    __shared__ unsigned long long s_key[4];
    __shared__ unsigned long long red[4][4];
    const int t = threadIdx.x, pose = blockIdx.y;
    const int c = (int)blockIdx.x * 256 + t;
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
    auto cell = [&](int ix, int iy) -> uint32_t {                     // (ix, iy) is in the grid
        if (staged) {
            const int lx = ix - x0, ly = iy - y0;
            if ((unsigned)lx < (unsigned)ww && (unsigned)ly < (unsigned)wh) return s_win[ly * ww + lx];
        }
        return pk[(size_t)iy * r.W + ix];
    };
    auto in_grid = [&](int ix, int iy) { return ix >= 0 && ix < r.W && iy >= 0 && iy < r.H; };

    unsigned long long key = ~0ull, n_ok = 0, n_coll = 0, n_steps = 0;
    if (c < r.K) {
        const int i = c / r.n_w, j = c - i * r.n_w;
        const int v = r.v_min + i * r.v_step, w = r.w_min + j * r.w_step;
        const int av = v < 0 ? -v : v, aw = w < 0 ? -w : w;
        int x = px, y = py, h = ph, nfree = 0, min_d = -1;
        uint32_t ec = NS_NO_COST;
        long long score = -1;
        if (start_ok) {
            min_d = (int)(start & NS_D);
            int ccx = cx0, ccy = cy0;
            for (int s = 0; s < r.T; s++) {
                int nx, ny;
                ns_step(s_dir[ns_dir_index(h, w)], v, x, y, nx, ny);
                const int ncx = nx >> 10, ncy = ny >> 10;
                if (!in_grid(ncx, ncy)) break;
                const uint32_t u = cell(ncx, ncy);
                if (!(u & NS_TRAV)) break;
                if (ncx != ccx && ncy != ccy && (!(cell(ncx, ccy) & NS_TRAV) || !(cell(ccx, ncy) & NS_TRAV))) break;
                x = nx; y = ny; h = (h + w) & 0xFFFF; ccx = ncx; ccy = ncy; nfree++;
                const int d = (int)(u & NS_D);
                min_d = d < min_d ? d : min_d;
            }
            if (r.wc > 0) ec = cost[(size_t)ccy * r.W + ccx];
            int need = r.min_free + (r.brake_div > 0 ? (av + r.brake_div - 1) / r.brake_div : 0);
            need = need < r.T ? need : r.T;
            if (nfree >= need && !(r.wc > 0 && ec == NS_NO_COST)) {
                score = (long long)r.wl * (r.cap - min_d) + (long long)r.ws * (r.v_abs_max - av) + (long long)r.wr * aw;
                if (r.wc > 0) score += (long long)r.wc * (long long)ec;
                if (r.wt > 0) {
                    long long dx = (long long)x - targets[2 * (size_t)pose], dy = (long long)y - targets[2 * (size_t)pose + 1];
                    dx = dx < 0 ? -dx : dx; dy = dy < 0 ? -dy : dy;
                    const long long hi = dx > dy ? dx : dy, lo = dx > dy ? dy : dx;
                    score += (long long)r.wt * ((10 * hi + 4 * lo) >> 10);
                }
                key = ((unsigned long long)score << 16) | (unsigned long long)c;     // score < 2^44, c < 2^16
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
    }
    // the chunk's winner and sums
    key = wave_min64(key);
    n_ok = wave_sum(n_ok); n_coll = wave_sum(n_coll); n_steps = wave_sum(n_steps);
    const int wv = t >> 6;
    if (lane() == 0) { s_key[wv] = key; red[0][wv] = n_ok; red[1][wv] = n_coll; red[2][wv] = n_steps; }
    __syncthreads();
    if (t == 0) {
        const unsigned long long a = s_key[0] < s_key[1] ? s_key[0] : s_key[1], b = s_key[2] < s_key[3] ? s_key[2] : s_key[3];
        const unsigned long long m = a < b ? a : b;
        if (m != ~0ull) atomicMin(&keys[pose], m);
        if (start_ok) atomicAdd(&stats[staged ? NS_STAGED : NS_GLOBAL], 1ull);
    }
    if (t >= 1 && t < 4) {
        const unsigned long long sum = (red[t - 1][0] + red[t - 1][1]) + (red[t - 1][2] + red[t - 1][3]);
        if (sum) atomicAdd(&stats[NS_ADM + (t - 1)], sum);
        if (t == 1 && sum) atomicAdd(&n_adm[pose], (int32_t)sum);
    }
}

// ---- pick: one lane per pose (steps 7 and 8) -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navsteer_pick(NavSteerRule r, const uint32_t* __restrict__ pk, const int32_t* __restrict__ poses,
                                                       const uint32_t* __restrict__ dirs, const unsigned long long* __restrict__ keys,
                                                       const int32_t* __restrict__ n_adm, NavSteerPose out, unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long red[4][4];
    const int pose = (int)blockIdx.x * 256 + threadIdx.x;
    unsigned long long n_ok = 0, n_blocked = 0, n_stuck = 0;
    if (pose < r.n_poses) {
        const int px = poses[3 * (size_t)pose], py = poses[3 * (size_t)pose + 1], ph = poses[3 * (size_t)pose + 2] & 0xFFFF;
        const int cx0 = px >> 10, cy0 = py >> 10;
        const bool inside = cx0 >= 0 && cx0 < r.W && cy0 >= 0 && cy0 < r.H;
        const bool start_ok = inside && (pk[(size_t)cy0 * r.W + cx0] & NS_TRAV);
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
            for (int s = 0; s < r.T; s++) {
                int nx, ny;
                ns_step(dirs[ns_dir_index(h, w)], v, x, y, nx, ny);
                const int ncx = nx >> 10, ncy = ny >> 10;
                if (ncx < 0 || ncx >= r.W || ncy < 0 || ncy >= r.H) break;
                if (!(pk[(size_t)ncy * r.W + ncx] & NS_TRAV)) break;
                if (ncx != ccx && ncy != ccy && (!(pk[(size_t)ccy * r.W + ncx] & NS_TRAV) || !(pk[(size_t)ncy * r.W + ccx] & NS_TRAV))) break;
                x = nx; y = ny; h = (h + w) & 0xFFFF; ccx = ncx; ccy = ncy;
                if (tr) { tr[3 * len] = x; tr[3 * len + 1] = y; tr[3 * len + 2] = h; }
                len++;
            }
        }
        if (out.best) out.best[pose] = best;
        if (out.cmd) { out.cmd[2 * (size_t)pose] = v; out.cmd[2 * (size_t)pose + 1] = w; }
        if (out.score) out.score[pose] = score;
        if (out.n_adm) out.n_adm[pose] = n_adm[pose];
        if (out.status) out.status[pose] = status;
        if (out.len) out.len[pose] = len;
        n_ok = status == 0; n_blocked = status == 1 || status == 2; n_stuck = status == 3;
    }
    n_ok = wave_sum(n_ok); n_blocked = wave_sum(n_blocked); n_stuck = wave_sum(n_stuck);
    const int wv = threadIdx.x >> 6;
    if (lane() == 0) { red[0][wv] = n_ok; red[1][wv] = n_blocked; red[2][wv] = n_stuck; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned long long sum = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
        if (sum) atomicAdd(&stats[NS_OK + threadIdx.x], sum);
    }
}

static void launch_navsteer_pack(hipStream_t st, size_t P, const NavSteerRule& r, const int8_t* state, const int32_t* dist2, uint32_t* pk) {
    ScopedKernel sk("navsteer_pack", st);
    hipLaunchKernelGGL(k_navsteer_pack, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, P, r.min_dist2, r.allow_unknown, r.cap, state, dist2, pk);
}
static void launch_navsteer_roll(hipStream_t st, const NavSteerRule& r, const uint32_t* pk, const uint32_t* cost, const int32_t* poses, const int32_t* targets,
                                 const uint32_t* dirs, unsigned long long* keys, int32_t* n_adm, const NavSteerCand& out, unsigned long long* stats) {
    ScopedKernel sk("navsteer_roll", st);
    // the largest clipped window of any pose, capped at what is staged (r.stage_cells): a pose whose window is larger walks the grid
    const long long side = 2LL * r.R + 1;
    const long long bound = std::min<long long>(side, r.W) * std::min<long long>(side, r.H);
    const size_t lds = 4 * (size_t)std::min<long long>(bound, r.stage_cells);
    hipLaunchKernelGGL(k_navsteer_roll, dim3((unsigned)((r.K + 255) / 256), (unsigned)r.n_poses), dim3(256), lds, st, r, pk, cost, poses, targets, dirs, keys,
                       n_adm, out, stats);
}
static void launch_navsteer_pick(hipStream_t st, const NavSteerRule& r, const uint32_t* pk, const int32_t* poses, const uint32_t* dirs,
                                 const unsigned long long* keys, const int32_t* n_adm, const NavSteerPose& out, unsigned long long* stats) {
    ScopedKernel sk("navsteer_pick", st);
    hipLaunchKernelGGL(k_navsteer_pick, dim3((unsigned)((r.n_poses + 255) / 256)), dim3(256), 0, st, r, pk, poses, dirs, keys, n_adm, out, stats);
}

}  // namespace ssf

// the direction table of step 1, made once: C and S, and the device's packed word (S << 16) | (C & 0xFFFF)
namespace {
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
const NavSteerDirs& navsteer_dirs() { static const NavSteerDirs d; return d; }
}  // namespace

extern "C" {
int ssf_navsteer_direction_table(int32_t* cos_out, int32_t* sin_out) {
    const NavSteerDirs& d = navsteer_dirs();
    if (cos_out) std::memcpy(cos_out, d.c, sizeof(d.c));
    if (sin_out) std::memcpy(sin_out, d.s, sizeof(d.s));
    return SSF_OK;
}

int ssf_navsteer_default_params(const ssf_handle* h, ssf_navsteer_params* p) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    std::memset(p, 0, sizeof(*p));
    p->width = 512; p->height = 512;
    p->n_v = 9; p->n_w = 33; p->n_steps = 32;
    p->v_min = 0; p->v_step = 64; p->w_min = -2048; p->w_step = 128;
    p->min_free_steps = 2; p->brake_div = 128; p->clearance_cap = 64;
    p->cost_weight = 1; p->clear_weight = 1; p->speed_weight = 1;
    return SSF_OK;
}

int ssf_navsteer_rollouts(ssf_handle* h, const ssf_navsteer_params* p, const int8_t* state, const int32_t* dist2, const uint32_t* cost,
                          const int32_t* poses, const int32_t* targets, const ssf_navsteer_out* out, ssf_navsteer_stats* stats) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    auto refuse = [&](const char* what) { h->err = std::string("ssf_navsteer_rollouts: ") + what; return SSF_ERR_INVALID_ARG; };
    if (!state || !dist2) return refuse("state or dist2 is NULL");
    if (!poses) return refuse("poses is NULL");
    if (!out || (!out->best && !out->best_cmd && !out->best_score && !out->n_admissible && !out->pose_status && !out->best_len && !out->best_traj &&
                 !out->cand_free && !out->cand_min_d && !out->cand_end && !out->cand_end_cost && !out->cand_score))
        return refuse("every output is NULL");
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
    const int wts[5] = {p->cost_weight, p->target_weight, p->clear_weight, p->speed_weight, p->turn_weight};
    for (int k = 0; k < 5; k++)
        if (wts[k] < 0 || wts[k] > 1000) return refuse("every weight must be 0..1000");
    if (!(wts[0] | wts[1] | wts[2] | wts[3] | wts[4])) return refuse("the weights must not all be 0");
    if (p->cost_weight > 0 && !cost) return refuse("cost is NULL with cost_weight > 0");
    if (p->target_weight > 0 && !targets) return refuse("targets is NULL with target_weight > 0");
    if (p->walk != 0 && p->walk != 1) return refuse("walk must be 0 or 1");
    { int rc = model_at_rest(h, "ssf_navsteer_rollouts", "steers nothing"); if (rc) return rc; }

    NavSteerRule r{};
    r.W = p->width; r.H = p->height; r.min_dist2 = p->min_dist2; r.allow_unknown = p->allow_unknown; r.cap = p->clearance_cap;
    r.n_poses = p->n_poses; r.n_v = p->n_v; r.n_w = p->n_w; r.K = p->n_v * p->n_w; r.v_min = p->v_min; r.v_step = p->v_step; r.w_min = p->w_min;
    r.w_step = p->w_step; r.T = p->n_steps; r.min_free = p->min_free_steps; r.brake_div = p->brake_div; r.v_abs_max = (int)v_abs_max;
    r.wc = p->cost_weight; r.wt = p->target_weight; r.wl = p->clear_weight; r.ws = p->speed_weight; r.wr = p->turn_weight;
    r.R = (int)(((long long)r.T * v_abs_max + 1023) / 1024) + 1; r.walk = p->walk;
    {   // what is staged (the file's head: a measured choice); no output depends on it
        const long long side = 2LL * r.R + 1, bound = std::min<long long>(side, r.W) * std::min<long long>(side, r.H);
        const long long bytes = 4 * std::min<long long>(bound, NS_LDS_CELLS) + NS_STATIC_LDS, wgs = (long long)((r.K + 255) / 256) * r.n_poses;
        const bool roomy = bytes <= NS_LDS_FREE || wgs <= (long long)NS_CUS * (NS_CU_LDS / bytes);
        r.stage_cells = p->walk ? 0 : (roomy ? (int)NS_LDS_CELLS : (int)((NS_LDS_FREE - NS_STATIC_LDS) / 4));
    }
    const size_t P = (size_t)r.W * r.H, np = (size_t)r.n_poses, NK = np * (size_t)r.K, traj = np * (size_t)(r.T + 1) * 3;
    const bool dev = p->on_device != 0;
    const uint32_t* use_cost = r.wc > 0 ? cost : nullptr;
    const int32_t* use_targets = r.wt > 0 ? targets : nullptr;

    // the arrays of a call with host pointers, each at a 256-byte boundary of one staging buffer.  best_traj goes in as well as out:
    // entries past best_len keep what the caller had there
    struct Item { const void* host; size_t bytes; void** arg; bool in, outp; size_t off; };
    const int8_t* d_state = state; const int32_t* d_dist2 = dist2; const uint32_t* d_cost = use_cost; const int32_t* d_poses = poses;
    const int32_t* d_targets = use_targets;
    ssf_navsteer_out o = *out;
    Item items[17];
    int n_items = 0;
    size_t need = 0;
    if (!dev) {
        auto add = [&](const void* host, size_t bytes, void** arg, bool in, bool outp) {
            if (!host) return;
            items[n_items++] = Item{host, bytes, arg, in, outp, need};
            need += (bytes + 255) & ~(size_t)255;
        };
        add(state, P, (void**)&d_state, true, false); add(dist2, 4 * P, (void**)&d_dist2, true, false); add(use_cost, 4 * P, (void**)&d_cost, true, false);
        add(poses, 12 * np, (void**)&d_poses, true, false); add(use_targets, 8 * np, (void**)&d_targets, true, false);
        add(o.best, 4 * np, (void**)&o.best, false, true); add(o.best_cmd, 8 * np, (void**)&o.best_cmd, false, true);
        add(o.best_score, 8 * np, (void**)&o.best_score, false, true); add(o.n_admissible, 4 * np, (void**)&o.n_admissible, false, true);
        add(o.pose_status, 4 * np, (void**)&o.pose_status, false, true); add(o.best_len, 4 * np, (void**)&o.best_len, false, true);
        add(o.best_traj, 4 * traj, (void**)&o.best_traj, true, true);
        add(o.cand_free, 4 * NK, (void**)&o.cand_free, false, true); add(o.cand_min_d, 4 * NK, (void**)&o.cand_min_d, false, true);
        add(o.cand_end, 12 * NK, (void**)&o.cand_end, false, true); add(o.cand_end_cost, 4 * NK, (void**)&o.cand_end_cost, false, true);
        add(o.cand_score, 8 * NK, (void**)&o.cand_score, false, true);
    }
    // the working buffers
    NavSteerWs& w = h->navsteer;
    bool ok = true;
    if (!w.stats) {
        ok = w.bufs.grow({{(void**)&w.stats, NS_STATS * sizeof(unsigned long long)}, {(void**)&w.keys, 4096 * sizeof(unsigned long long)},
                          {(void**)&w.n_adm, 4096 * sizeof(int32_t)}, {(void**)&w.dirs, NS_DIRS * sizeof(uint32_t)}});
    }
    if (ok && P > w.cells) { ok = w.bufs.grow({{(void**)&w.pk, 4 * P}}); if (ok) w.cells = P; }
    if (ok && need > w.io_bytes) { ok = w.bufs.grow({{(void**)&w.io, need}}); if (ok) w.io_bytes = need; }
    if (!ok) { h->err = "ssf_navsteer_rollouts: allocation of the working buffers failed"; return SSF_ERR_DEVICE; }
    for (int k = 0; k < n_items; k++) *items[k].arg = w.io + items[k].off;

    hipStream_t st = h->stream;
    TimerScope ts(h);
    if (!w.dirs_sent) {
        HCK(hipMemcpyAsync(w.dirs, navsteer_dirs().packed, NS_DIRS * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        w.dirs_sent = true;
    }
    for (int k = 0; k < n_items; k++)
        if (const Item& it = items[k]; it.in) HCK(hipMemcpyAsync(*it.arg, it.host, it.bytes, hipMemcpyHostToDevice, st));
    HCK(hipMemsetAsync(w.stats, 0, NS_STATS * sizeof(unsigned long long), st));
    HCK(hipMemsetAsync(w.keys, 0xFF, np * sizeof(unsigned long long), st));
    HCK(hipMemsetAsync(w.n_adm, 0, np * sizeof(int32_t), st));
    launch_navsteer_pack(st, P, r, d_state, d_dist2, w.pk);
    HCK(hipGetLastError());
    const NavSteerCand cand{o.cand_free, o.cand_min_d, o.cand_end, o.cand_end_cost, (long long*)o.cand_score};
    launch_navsteer_roll(st, r, w.pk, d_cost, d_poses, d_targets, w.dirs, w.keys, w.n_adm, cand, w.stats);
    HCK(hipGetLastError());
    const NavSteerPose pick{o.best, o.best_cmd, (long long*)o.best_score, o.n_admissible, o.pose_status, o.best_len, o.best_traj};
    launch_navsteer_pick(st, r, w.pk, d_poses, w.dirs, w.keys, w.n_adm, pick, w.stats);
    HCK(hipGetLastError());
    unsigned long long s[NS_STATS];
    HCK(hipMemcpyAsync(s, w.stats, sizeof(s), hipMemcpyDeviceToHost, st));
    for (int k = 0; k < n_items; k++)
        if (const Item& it = items[k]; it.outp) HCK(hipMemcpyAsync(const_cast<void*>(it.host), *it.arg, it.bytes, hipMemcpyDeviceToHost, st));
    { int rc = sync_collect(h); if (rc) return rc; }
    if (stats) {
        stats->poses_ok = (int64_t)s[NS_OK]; stats->poses_blocked = (int64_t)s[NS_BLOCKED]; stats->poses_stuck = (int64_t)s[NS_STUCK];
        stats->candidates = (int64_t)NK; stats->admissible = (int64_t)s[NS_ADM]; stats->collided = (int64_t)s[NS_COLL];
        stats->steps_taken = (int64_t)s[NS_STEPS];
        stats->windows_staged = (int64_t)s[NS_STAGED]; stats->windows_global = (int64_t)s[NS_GLOBAL];
    }
    return SSF_OK;
}
}  // extern "C"
