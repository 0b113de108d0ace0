// ssf_navdyn.hip -- steering among moving obstacles (include/ssf_navdyn.h) on gfx950: the rollouts of ssf_navsteer.h and ssf_navfoot.h
// with every step tested against the predicted movers, and the blobs of a frame's moving pixels in the grid frame.
//
// What is computed is pinned in include/ssf_navdyn.h (the restatement: tests/navdyn_ref.py).
//   * pack, roll, pick   The kernels of ssf_navsteer.hip and ssf_navfoot.hip again -- the same packed words, the same roll frames,
//            ssf_navsteer_walk.hpp's walk, score, winner and replay -- with NavDynHook in the place of the empty step hook: one
//            workgroup per (pose, 256 candidates), a candidate per lane, the direction table in LDS, one 64-bit atomicMin per
//            workgroup, the winner's arc replayed in the pick.  The mover list (at most 1.5 KiB) is copied into LDS once per
//            workgroup; the loop over it is the same for every lane of a wave, so its reads are broadcasts.  A step costs, per mover,
//            three multiply-adds for (X_s, Y_s, R_s) = (x, y, r) + s * (vx, vy, grow), two 32 x 32 -> 64-bit multiply-adds for D2, and
//            two more for the comparisons with R_s^2 and (min_gap + R_s)^2.  The positions are NOT advanced by addition: a running sum
//            would be per-lane state (a lane leaves the loop when its rollout ends) of three registers a mover, where the
//            multiply-add from the list in LDS needs none.  The square root is taken only where it lowers the running minimum:
//            isqrt(D2) - R_s < g  <=>  D2 < (g + R_s)^2; then the f64 root, put right by one integer comparison each way.
//            Movers are not culled per workgroup: see README (the probe's figures).
//   * blobs  k_navdyn_blob_seen: a workgroup per 16 x 16 pixel tile, a thread per pixel (the live layer's tile pixel, depth test and
//            point, ssf_navlive.hpp, behind this kernel's own membership test): member, valid, point, (bx, by) into a per-pixel buffer, and a mark at the pixel's label.
//            k_navdyn_blob_slots: a thread per label value: a marked label takes the next compact slot and clears its record.
//            k_navdyn_blob_sum: a workgroup per tile again: the tile's contributing pixels are merged per slot in an LDS hash table of
//            512 entries (a tile has at most 256 labels, so a probe always ends) with LDS atomics, and every occupied entry goes to
//            the record with seven global atomics; with direct = 1 every pixel issues the seven itself.  All are integer sums, minima
//            and maxima.  The slot numbers depend on arrival order; nothing that leaves the call does: the records are sorted by
//            (-n, label) on the host.
// No device-wide barrier, no inline assembly.
//
// Bounds: the rollouts' are ssf_navsteer.hip's; the mover list is read at 6 * m + k with m < n_movers <= 64, which the host has
// checked whatever on_device says; its VALUES enter 32- and 64-bit unsigned arithmetic only.  cand_hit and cand_min_gap are written
// at pose * K + c with c < K, best_min_gap at pose < n_poses.  The blobs: a pixel is touched only with u < W and v < H; a label
// indexes the slot array only after 0 <= label < W * H; a slot is below the number of marked labels <= W * H, the records' size; the
// LDS table is indexed & 511.
//
// This file is NOT one of the product library's objects.  It is linked, with all of libssf_hip_pose.so's, into libssf_hip_dyn.so.
#include "ssf_navsteer_walk.hpp"
#include "ssf_navlive.hpp"
#include "../../include/ssf_navfoot.h"
#include <algorithm>
#include <climits>
#include <memory>
#include <new>

namespace ssf {

// ---- the rollouts with movers ------------------------------------------------------------------------------------------------------
enum { ND_MOVER_WORDS = SSF_NAVDYN_MOVER_WORDS, ND_MAX_MOVERS = SSF_NAVDYN_MAX_MOVERS };

// what the kernels get of ssf_navdyn.h: the list, the cap, the weight and the three outputs (nullptr = not produced)
struct NavDynArgs { const int32_t* movers; int n, cap, wm; int32_t* hit; int32_t* gap; int32_t* best; };

// the floor square root of a < 2^53 (ssf_navdyn.h step A.7)
__device__ __forceinline__ unsigned long long navdyn_isqrt(unsigned long long a) {
    unsigned long long r = (unsigned long long)sqrt((double)a);
    if (r * r > a) r--;
    if ((r + 1) * (r + 1) <= a) r++;
    return r;
}
__device__ __forceinline__ unsigned long long navdyn_sq(uint32_t a) { return (unsigned long long)a * (unsigned long long)a; }
__device__ __forceinline__ uint32_t navdyn_absdiff(uint32_t a, uint32_t b) {
    const int32_t d = (int32_t)(a - b);
    return d < 0 ? 0u - (uint32_t)d : (uint32_t)d;
}

// the step hook (ssf_navsteer_walk.hpp) of steps A.2 to A.5: mov, the list wherever it lies (LDS in the roll, the grid's memory in
// the pick); hit and gap, the lane's cand_hit and min_gap so far
struct NavDynHook {
    static constexpr bool counts = true;
    const int32_t* mov; int n, cap, wm;
    int32_t* o_hit; int32_t* o_gap; int32_t* o_best;
    int hit, gap;
    __device__ __forceinline__ bool step(int s, int nx, int ny) {
        int g = gap;
        for (int m = 0; m < n; m++) {                                 // (the same for every lane)
            const int32_t* e = mov + ND_MOVER_WORDS * m;
            const uint32_t X = (uint32_t)e[0] + (uint32_t)s * (uint32_t)e[2], Y = (uint32_t)e[1] + (uint32_t)s * (uint32_t)e[3];
            const uint32_t R = (uint32_t)e[4] + (uint32_t)s * (uint32_t)e[5];
            const unsigned long long D2 = navdyn_sq(navdyn_absdiff((uint32_t)nx, X)) + navdyn_sq(navdyn_absdiff((uint32_t)ny, Y));
            if (D2 < navdyn_sq(R)) { hit = m; return false; }
            if (D2 < navdyn_sq((uint32_t)g + R)) g = (int)((uint32_t)navdyn_isqrt(D2) - R);
        }
        gap = g;
        return true;
    }
    __device__ __forceinline__ long long term() const { return (long long)wm * ((10LL * (long long)(cap - gap)) >> 10); }
    __device__ __forceinline__ void store(size_t q, bool start_ok) const {
        if (o_hit) o_hit[q] = start_ok ? hit : -1;
        if (o_gap) o_gap[q] = start_ok ? gap : -1;
    }
    __device__ __forceinline__ void pick(int pose, bool won) const {
        if (o_best) o_best[pose] = won ? gap : -1;
    }
    __device__ __forceinline__ bool ended() const { return hit >= 0; }
};

__global__ __launch_bounds__(256) void k_navdyn_pack(size_t P, int min_dist2, int allow_unknown, int cap, const int8_t* __restrict__ state,
                                                     const int32_t* __restrict__ dist2, uint32_t* __restrict__ pk) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    pk[p] = ns_disc_word(state[p], dist2[p], min_dist2, allow_unknown, cap);
}
__global__ __launch_bounds__(256) void k_navdyn_foot_pack(size_t P, int min_dist2, int cap, const uint32_t* __restrict__ mask,
                                                          const int32_t* __restrict__ dist2, uint2* __restrict__ pk) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    pk[p] = ns_foot_word(mask, dist2, p, min_dist2, cap);
}

// the mover list into LDS: ALL threads call it; the roll frames synchronise the workgroup before anything reads it
__device__ __forceinline__ void navdyn_stage_movers(const NavDynArgs& a, int32_t* s_mov) {
    for (int k = threadIdx.x; k < ND_MOVER_WORDS * a.n; k += 256) s_mov[k] = a.movers[k];
}

__global__ __launch_bounds__(256) void k_navdyn_roll(NavSteerRule r, NavDynArgs a, const uint32_t* __restrict__ pk, const uint32_t* __restrict__ cost,
                                                     const int32_t* __restrict__ poses, const int32_t* __restrict__ targets,
                                                     const uint32_t* __restrict__ dirs, unsigned long long* __restrict__ keys,
                                                     int32_t* __restrict__ n_adm, NavSteerCand out, unsigned long long* __restrict__ stats) {
    __shared__ uint32_t s_dir[NS_DIRS];
    __shared__ int32_t s_mov[ND_MOVER_WORDS * ND_MAX_MOVERS];
    navdyn_stage_movers(a, s_mov);
    ns_disc_roll(r, NavDynHook{s_mov, a.n, a.cap, a.wm, a.hit, a.gap, nullptr, -1, a.cap}, s_dir, pk, cost, poses, targets, dirs, keys, n_adm, out, stats);
}
__global__ __launch_bounds__(256) void k_navdyn_foot_roll(NavSteerRule r, NavDynArgs a, int B, int shift, const uint2* __restrict__ pk,
                                                          const uint32_t* __restrict__ cost, const int32_t* __restrict__ poses,
                                                          const int32_t* __restrict__ targets, const uint32_t* __restrict__ dirs,
                                                          unsigned long long* __restrict__ keys, int32_t* __restrict__ n_adm, NavSteerCand out,
                                                          unsigned long long* __restrict__ stats) {
    __shared__ uint32_t s_dir[NS_DIRS];
    __shared__ int32_t s_mov[ND_MOVER_WORDS * ND_MAX_MOVERS];
    navdyn_stage_movers(a, s_mov);
    ns_foot_roll(r, NavDynHook{s_mov, a.n, a.cap, a.wm, a.hit, a.gap, nullptr, -1, a.cap}, s_dir, B, shift, pk, cost, poses, targets, dirs, keys, n_adm, out,
                 stats);
}

__global__ __launch_bounds__(256) void k_navdyn_pick(NavSteerRule r, NavDynArgs a, const uint32_t* __restrict__ pk, const int32_t* __restrict__ poses,
                                                     const uint32_t* __restrict__ dirs, const unsigned long long* __restrict__ keys,
                                                     const int32_t* __restrict__ n_adm, NavSteerPose out, unsigned long long* __restrict__ stats) {
    const NavSteerCells cells{pk, nullptr, r.W, 0, 0, 0, 0, false};
    ns_pick_body(r, cells, NavDynHook{a.movers, a.n, a.cap, a.wm, nullptr, nullptr, a.best, -1, a.cap},
                 [&](int cx, int cy, int) { return (pk[(size_t)cy * r.W + cx] & NS_TRAV) != 0; }, poses, dirs, keys, n_adm, out, stats);
}
__global__ __launch_bounds__(256) void k_navdyn_foot_pick(NavSteerRule r, NavDynArgs a, int B, int shift, const uint2* __restrict__ pk,
                                                          const int32_t* __restrict__ poses, const uint32_t* __restrict__ dirs,
                                                          const unsigned long long* __restrict__ keys, const int32_t* __restrict__ n_adm, NavSteerPose out,
                                                          unsigned long long* __restrict__ stats) {
    const NavFootCells cells{pk, r.W, B, shift};
    ns_pick_body(r, cells, NavDynHook{a.movers, a.n, a.cap, a.wm, nullptr, nullptr, a.best, -1, a.cap},
                 [&](int cx, int cy, int h) { return (pk[(size_t)cy * r.W + cx].x & cells.bin_bit(h)) != 0; }, poses, dirs, keys, n_adm, out, stats);
}

// ---- the blobs -------------------------------------------------------------------------------------------------------------------------
enum { NB_MEMBER = 0, NB_VALID = 1, NB_BAND = 2, NB_LABELS = 3, NB_STATS = 4 };
enum { NB_HASH = 512 };                                               // (the tile: NL_TW x NL_TH, navlive_tile_pixel, ssf_navlive.hpp)
// the record of a label (step B.3)
struct NavDynBlobRec { unsigned long long sum_x, sum_y; int32_t label; uint32_t n; int32_t min_x, max_x, min_y, max_y; };
static_assert(sizeof(NavDynBlobRec) == 40, "NavDynWs counts 40 bytes a record");

// steps B.1 and B.2: one thread per pixel.  pt[p] = (bx, by) of a contributing pixel, (-1, -1) of any other; slot[label] = 1 for the
// label of a contributing pixel (every writer writes the same word)
template <int DF>
__global__ __launch_bounds__(256) void k_navdyn_blob_seen(NavGrid G, NavLiveCam cam, const void* __restrict__ depth, double scale,
                                                          const uint8_t* __restrict__ mask, const int32_t* __restrict__ label, int2* __restrict__ pt,
                                                          int32_t* __restrict__ slot, unsigned long long* __restrict__ stats) {
    const NavTilePixel px = navlive_tile_pixel(cam.W, cam.H);
    unsigned long long member = 0, valid = 0, band = 0;
    if (px.in) {
        const int L = label[px.p];
        int2 q = make_int2(-1, -1);
        member = mask[px.p] != 0 && L >= 0 && L < cam.W * cam.H;
        if (member) {
            float d;
            valid = navlive_pixel_depth<DF>(cam, depth, px.p, scale, d);
            if (valid) {
                float Sx, Sy, Sz, gx, gy;
                navlive_pixel_point(cam, px.u, px.v, d, Sx, Sy, Sz);
                band = nav_grid_point(G, Sx, Sy, Sz, gx, gy);
                if (band) { q = make_int2((int)(gx * 1024.0f), (int)(gy * 1024.0f)); slot[L] = 1; }
            }
        }
        pt[px.p] = q;
    }
    block_sums({member, valid, band}, stats, NB_MEMBER);
}

// one thread per label value: a marked label takes the next slot (slot[L] = slot + 1) and clears its record
__global__ __launch_bounds__(256) void k_navdyn_blob_slots(int n_labels, int32_t* __restrict__ slot, NavDynBlobRec* __restrict__ rec,
                                                           unsigned long long* __restrict__ stats) {
    const int L = (int)blockIdx.x * 256 + threadIdx.x;
    if (L >= n_labels || slot[L] != 1) return;
    const unsigned long long s = atomicAdd(&stats[NB_LABELS], 1ull);  // (below n_labels: every label takes one)
    rec[s] = NavDynBlobRec{0ull, 0ull, L, 0u, INT_MAX, INT_MIN, INT_MAX, INT_MIN};
    slot[L] = (int32_t)s + 1;
}

__device__ __forceinline__ void navdyn_blob_add(NavDynBlobRec* r, uint32_t n, unsigned long long sx, unsigned long long sy, int x0, int x1, int y0, int y1) {
    atomicAdd(&r->n, n); atomicAdd(&r->sum_x, sx); atomicAdd(&r->sum_y, sy);
    atomicMin(&r->min_x, x0); atomicMax(&r->max_x, x1); atomicMin(&r->min_y, y0); atomicMax(&r->max_y, y1);
}

// step B.3: one thread per pixel, a workgroup per tile
template <bool MERGE>
__global__ __launch_bounds__(256) void k_navdyn_blob_sum(int W, int H, const int2* __restrict__ pt, const int32_t* __restrict__ label,
                                                         const int32_t* __restrict__ slot, NavDynBlobRec* __restrict__ rec) {
    __shared__ int s_key[MERGE ? NB_HASH : 1];
    __shared__ NavDynBlobRec s_rec[MERGE ? NB_HASH : 1];
    const NavTilePixel px = navlive_tile_pixel(W, H);
    const int t = threadIdx.x;
    int s = -1;
    int2 q = make_int2(-1, -1);
    if (px.in) {
        q = pt[px.p];
        if (q.x >= 0) s = slot[label[px.p]] - 1;                      // (a contributing pixel: its label was checked and took a slot)
    }
    if (!MERGE) {
        if (s >= 0) navdyn_blob_add(rec + s, 1u, (unsigned long long)q.x, (unsigned long long)q.y, q.x, q.x, q.y, q.y);
        return;
    }
    for (int e = t; e < NB_HASH; e += 256) { s_key[e] = -1; s_rec[e] = NavDynBlobRec{0ull, 0ull, 0, 0u, INT_MAX, INT_MIN, INT_MAX, INT_MIN}; }
    __syncthreads();
    if (s >= 0) {
        uint32_t e = ((uint32_t)s * 2654435761u) >> 23;               // 9 bits
        for (;;) {                                                    // (at most 256 keys in 512 entries: an empty one is always met)
            const int old = atomicCAS(&s_key[e], -1, s);
            if (old == -1 || old == s) break;
            e = (e + 1) & (NB_HASH - 1);
        }
        navdyn_blob_add(&s_rec[e], 1u, (unsigned long long)q.x, (unsigned long long)q.y, q.x, q.x, q.y, q.y);
    }
    __syncthreads();
    for (int e = t; e < NB_HASH; e += 256) {
        const int k = s_key[e];
        if (k >= 0) { const NavDynBlobRec& b = s_rec[e]; navdyn_blob_add(rec + k, b.n, b.sum_x, b.sum_y, b.min_x, b.max_x, b.min_y, b.max_y); }
    }
}

}  // namespace ssf

namespace {
using namespace ssf;

NavDynArgs navdyn_args(const NavSteerMovers& mv) {
    return NavDynArgs{mv.d_movers, mv.p->n_movers, mv.p->mover_cap, mv.p->mover_weight, mv.o.cand_hit, mv.o.cand_min_gap, mv.o.best_min_gap};
}

// the disc's part of a call with movers (navsteer_call, ssf_navsteer_walk.hpp): ssf_navsteer.hip's staging choice and packed grid
struct NavDynRun {
    ssf_handle* h; NavSteerMovers* mv;
    int stage_cells(const NavSteerRule& r) const { return navsteer_stage_cells(r); }
    bool reserve(size_t P) { return navsteer_reserve_pk(h, P); }
    int launch(hipStream_t st, const NavSteerRule& r, const void* state, const int32_t* dist2, const uint32_t* cost, const int32_t* poses,
               const int32_t* targets, NavSteerWs& w, const NavSteerCand& cand, const NavSteerPose& pick) {
        const size_t P = (size_t)r.W * r.H;
        const NavDynArgs a = navdyn_args(*mv);
        {
            ScopedKernel sk("navdyn_pack", st);
            hipLaunchKernelGGL(k_navdyn_pack, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, P, r.min_dist2, r.allow_unknown, r.cap, (const int8_t*)state,
                               dist2, w.pk);
        }
        HCK(hipGetLastError());
        {
            ScopedKernel sk("navdyn_roll", st);
            hipLaunchKernelGGL(k_navdyn_roll, dim3((unsigned)((r.K + 255) / 256), (unsigned)r.n_poses), dim3(256), navsteer_window_lds(r), st, r, a,
                               (const uint32_t*)w.pk, cost, poses, targets, (const uint32_t*)w.dirs, w.keys, w.n_adm, cand, w.stats);
        }
        HCK(hipGetLastError());
        {
            ScopedKernel sk("navdyn_pick", st);
            hipLaunchKernelGGL(k_navdyn_pick, dim3((unsigned)((r.n_poses + 255) / 256)), dim3(256), 0, st, r, a, (const uint32_t*)w.pk, poses,
                               (const uint32_t*)w.dirs, (const unsigned long long*)w.keys, (const int32_t*)w.n_adm, pick, w.stats);
        }
        HCK(hipGetLastError());
        return SSF_OK;
    }
};

// the footprint's: ssf_navfoot.hip's 8-byte packed grid, nothing staged
struct NavDynFootRun {
    ssf_handle* h; NavSteerMovers* mv; int B, shift;
    int stage_cells(const NavSteerRule&) const { return 0; }
    bool reserve(size_t P) { return navfoot_reserve_pk(h, P); }
    int launch(hipStream_t st, const NavSteerRule& r, const void* mask, const int32_t* dist2, const uint32_t* cost, const int32_t* poses,
               const int32_t* targets, NavSteerWs& w, const NavSteerCand& cand, const NavSteerPose& pick) {
        const size_t P = (size_t)r.W * r.H;
        const NavDynArgs a = navdyn_args(*mv);
        uint2* pk = (uint2*)h->navfoot.pk;
        {
            ScopedKernel sk("navdyn_pack", st);
            hipLaunchKernelGGL(k_navdyn_foot_pack, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, P, r.min_dist2, r.cap, (const uint32_t*)mask, dist2, pk);
        }
        HCK(hipGetLastError());
        {
            ScopedKernel sk("navdyn_roll", st);
            hipLaunchKernelGGL(k_navdyn_foot_roll, dim3((unsigned)((r.K + 255) / 256), (unsigned)r.n_poses), dim3(256), 0, st, r, a, B, shift, (const uint2*)pk,
                               cost, poses, targets, (const uint32_t*)w.dirs, w.keys, w.n_adm, cand, w.stats);
        }
        HCK(hipGetLastError());
        {
            ScopedKernel sk("navdyn_pick", st);
            hipLaunchKernelGGL(k_navdyn_foot_pick, dim3((unsigned)((r.n_poses + 255) / 256)), dim3(256), 0, st, r, a, B, shift, (const uint2*)pk, poses,
                               (const uint32_t*)w.dirs, (const unsigned long long*)w.keys, (const int32_t*)w.n_adm, pick, w.stats);
        }
        HCK(hipGetLastError());
        return SSF_OK;
    }
};

// the smallest r with r * r >= a
long long navdyn_ceil_sqrt(long long a) {
    long long r = (long long)std::sqrt((double)a);
    while (r * r > a) r--;
    while (r * r < a) r++;
    return r;
}
}  // namespace

extern "C" {
int ssf_navdyn_default_params(const ssf_handle* h, ssf_navdyn_params* dp) {
    if (!h || !dp) return SSF_ERR_INVALID_ARG;
    std::memset(dp, 0, sizeof(*dp));
    dp->mover_cap = 4096; dp->mover_weight = 1;
    return SSF_OK;
}

int ssf_navdyn_rollouts(ssf_handle* h, const ssf_navsteer_params* p, const ssf_navdyn_params* dp, const int8_t* state, const int32_t* dist2,
                        const uint32_t* cost, const int32_t* poses, const int32_t* targets, const int32_t* movers, const ssf_navsteer_out* out,
                        const ssf_navdyn_out* dout, ssf_navsteer_stats* stats, ssf_navdyn_stats* dstats) {
    NavSteerMovers mv{dp, movers, dout, dstats, nullptr, ssf_navdyn_out{}};
    NavDynRun run{h, &mv};
    return navsteer_call(h, "ssf_navdyn_rollouts", p, state, 1, "state", dist2, cost, poses, targets, out, stats, run, &mv);
}

int ssf_navdyn_foot_rollouts(ssf_handle* h, const ssf_navsteer_params* p, const ssf_navdyn_params* dp, int n_headings, const uint32_t* free_mask,
                             const int32_t* dist2, const uint32_t* cost, const int32_t* poses, const int32_t* targets, const int32_t* movers,
                             const ssf_navsteer_out* out, const ssf_navdyn_out* dout, ssf_navsteer_stats* stats, ssf_navdyn_stats* dstats) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    const int lg = nav_log2_bins(n_headings);
    if (lg < 0) { h->err = "ssf_navdyn_foot_rollouts: n_headings must be 1, 2, 4, 8, 16 or 32"; return SSF_ERR_INVALID_ARG; }
    NavSteerMovers mv{dp, movers, dout, dstats, nullptr, ssf_navdyn_out{}};
    NavDynFootRun run{h, &mv, n_headings, 16 - lg};
    return navsteer_call(h, "ssf_navdyn_foot_rollouts", p, free_mask, 4, "free_mask", dist2, cost, poses, targets, out, stats, run, &mv);
}

int ssf_navdyn_default_blob_params(const ssf_handle* h, ssf_navdyn_blob_params* p) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    ssf_navgrid_params g;
    { int rc = ssf_navgrid_default_params(h, &g); if (rc) return rc; }
    std::memset(p, 0, sizeof(*p));
    p->width = g.width; p->height = g.height; p->res = g.res; p->floor_max = g.floor_max; p->z_max = g.z_max;
    p->min_points = 16; p->max_blobs = SSF_NAVDYN_MAX_BLOBS;
    return SSF_OK;
}

int ssf_navdyn_blobs(ssf_handle* h, const ssf_navdyn_blob_params* p, const void* depth, const uint8_t* mask, const int32_t* label, int32_t* blobs,
                     ssf_navdyn_blob_stats* stats) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    auto refuse = [&](const char* what) { h->err = std::string("ssf_navdyn_blobs: ") + what; return SSF_ERR_INVALID_ARG; };
    if (!depth || !mask || !label) return refuse("depth, mask or label is NULL");
    if (!blobs) return refuse("blobs is NULL");
    ssf_navgrid_params g;
    (void)ssf_navgrid_default_params(h, &g);
    g.width = p->width; g.height = p->height; g.res = p->res;
    if (const char* what = navgrid_size_res(&g)) return refuse(what);
    if (std::isnan(p->floor_max) || std::isnan(p->z_max)) return refuse("floor_max or z_max is a NaN");
    NavLiveCam cam{};
    if (const char* what = navlive_pinhole(h, p->fx, p->fy, p->cx, p->cy, p->cam_width, p->cam_height, cam)) return refuse(what);
    if (const char* what = navlive_range(h, p->t_min, p->t_max, cam)) return refuse(what);
    if (p->min_points < 1) return refuse("min_points must be >= 1");
    if (p->max_blobs < 1 || p->max_blobs > SSF_NAVDYN_MAX_BLOBS) return refuse("max_blobs must be 1..64");
    if (p->direct != 0 && p->direct != 1) return refuse("direct must be 0 or 1");
    const int df = h->in_depth;
    const size_t bpp = df == SSF_DEPTH_U16_SCALED ? 2 : 4;
    if (p->frame_on_device && (uintptr_t)depth % bpp) return refuse("the device depth pointer is not aligned for the input format");
    { int rc = model_at_rest(h, "ssf_navdyn_blobs", "sees no movers"); if (rc) return rc; }

    float gpose[12];
    NavGrid G{};
    { int rc = navlive_frames(h, &g, p, 0.0f, G, cam, gpose); if (rc) return rc; }

    const size_t npix = (size_t)cam.W * cam.H;
    const void* d_depth = depth; const uint8_t* d_mask = mask; const int32_t* d_label = label;
    StagedIo io;
    if (!p->frame_on_device) { io.in(depth, bpp * npix, &d_depth); io.in(mask, npix, &d_mask); io.in(label, 4 * npix, &d_label); }
    NavDynWs& w = h->navdyn;
    bool ok = true;
    if (!w.stats) ok = w.bufs.grow({{(void**)&w.stats, NB_STATS * sizeof(unsigned long long)}});
    if (ok && npix > w.pixels) {
        ok = w.bufs.grow({{(void**)&w.pt, 8 * npix}, {(void**)&w.slot, 4 * npix}, {(void**)&w.rec, sizeof(NavDynBlobRec) * npix}});
        if (ok) w.pixels = npix;
    }
    if (ok) ok = io.reserve(w.bufs, &w.img, &w.img_bytes, io.need());
    if (!ok) { h->err = "ssf_navdyn_blobs: allocation of the working buffers failed"; return SSF_ERR_DEVICE; }

    hipStream_t st = h->stream;
    TimerScope ts(h);
    HCK(io.copy_in(st));
    HCK(hipMemsetAsync(w.stats, 0, NB_STATS * sizeof(unsigned long long), st));
    HCK(hipMemsetAsync(w.slot, 0, 4 * npix, st));
    const unsigned tiles = navlive_tiles(cam.W, cam.H);
    NavDynBlobRec* rec = (NavDynBlobRec*)w.rec;
    {
        ScopedKernel sk("navdyn_blob_seen", st);
        navlive_by_depth_format(df, [&](auto DF) {
            hipLaunchKernelGGL(k_navdyn_blob_seen<decltype(DF)::value>, dim3(tiles), dim3(256), 0, st, G, cam, d_depth, h->in_scale, d_mask, d_label, w.pt, w.slot,
                               w.stats);
        });
    }
    HCK(hipGetLastError());
    {
        ScopedKernel sk("navdyn_blob_slots", st);
        hipLaunchKernelGGL(k_navdyn_blob_slots, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, (int)npix, w.slot, rec, w.stats);
    }
    HCK(hipGetLastError());
    {
        ScopedKernel sk("navdyn_blob_sum", st);
        if (p->direct)
            hipLaunchKernelGGL(k_navdyn_blob_sum<false>, dim3(tiles), dim3(256), 0, st, cam.W, cam.H, (const int2*)w.pt, d_label, (const int32_t*)w.slot, rec);
        else
            hipLaunchKernelGGL(k_navdyn_blob_sum<true>, dim3(tiles), dim3(256), 0, st, cam.W, cam.H, (const int2*)w.pt, d_label, (const int32_t*)w.slot, rec);
    }
    HCK(hipGetLastError());
    unsigned long long s[NB_STATS];
    HCK(hipMemcpyAsync(s, w.stats, sizeof(s), hipMemcpyDeviceToHost, st));
    HCK(hipStreamSynchronize(st));
    // the compact table (one record per label seen) comes to the host: steps B.4 and B.5
    const size_t n_recs = (size_t)s[NB_LABELS];
    // (arrays, not vectors: a vector's members would be instantiated here and exported by the library)
    std::unique_ptr<NavDynBlobRec[]> recs(new (std::nothrow) NavDynBlobRec[n_recs + 1]);
    std::unique_ptr<uint32_t[]> kept(new (std::nothrow) uint32_t[n_recs + 1]);
    if (!recs || !kept) { h->err = "ssf_navdyn_blobs: allocation of the label table failed"; return SSF_ERR_DEVICE; }
    if (n_recs) HCK(hipMemcpyAsync(recs.get(), rec, n_recs * sizeof(NavDynBlobRec), hipMemcpyDeviceToHost, st));
    { int rc = sync_collect(h); if (rc) return rc; }
    size_t n_kept = 0;
    for (size_t k = 0; k < n_recs; k++)
        if (recs[k].n >= (uint32_t)p->min_points) kept[n_kept++] = (uint32_t)k;
    const NavDynBlobRec* rv = recs.get();
    std::sort(kept.get(), kept.get() + n_kept, [rv](uint32_t a, uint32_t b) { return rv[a].n != rv[b].n ? rv[a].n > rv[b].n : rv[a].label < rv[b].label; });
    const size_t n_out = std::min(n_kept, (size_t)p->max_blobs);
    int32_t rows[SSF_NAVDYN_MAX_BLOBS * SSF_NAVDYN_BLOB_WORDS];
    for (size_t k = 0; k < n_out; k++) {
        const NavDynBlobRec& b = recs[kept[k]];
        const long long cx = (long long)(b.sum_x / b.n), cy = (long long)(b.sum_y / b.n);
        const long long ex = std::max(cx - b.min_x, (long long)b.max_x - cx), ey = std::max(cy - b.min_y, (long long)b.max_y - cy);
        const int32_t row[SSF_NAVDYN_BLOB_WORDS] = {b.label, (int32_t)b.n, (int32_t)cx, (int32_t)cy, (int32_t)navdyn_ceil_sqrt(ex * ex + ey * ey), (int32_t)ex,
                                                    (int32_t)ey, 0};
        std::memcpy(rows + SSF_NAVDYN_BLOB_WORDS * k, row, sizeof(row));
    }
    if (n_out) {
        if (p->on_device) HCK(hipMemcpy(blobs, rows, n_out * sizeof(int32_t) * SSF_NAVDYN_BLOB_WORDS, hipMemcpyHostToDevice));
        else std::memcpy(blobs, rows, n_out * sizeof(int32_t) * SSF_NAVDYN_BLOB_WORDS);
    }
    if (stats) {
        stats->pixels_member = (int64_t)s[NB_MEMBER]; stats->pixels_valid = (int64_t)s[NB_VALID]; stats->points_in_band = (int64_t)s[NB_BAND];
        stats->labels_seen = (int64_t)s[NB_LABELS]; stats->blobs_kept = (int64_t)n_kept; stats->blobs_written = (int64_t)n_out;
    }
    return SSF_OK;
}
}  // extern "C"
