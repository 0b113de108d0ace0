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
// The step, the arc's walk, the score, the winner, the replay and the host side of the call live in ssf_navsteer_walk.hpp, generic
// over the cell test, and are shared with ssf_navfoot.hip (include/ssf_navfoot.h); and with
// ssf_navdyn.hip (include/ssf_navdyn.h), and so do the disc's cell test (the packed word, staged or not) and its roll frame; this
// file holds the staging choice, the three kernels and their launches.
//
// Bounds: a cell is read only after the test that it lies in the grid; a read of the staged window tests the window's box as well
// and goes to the grid when outside (by the reach argument it never is).  Per-candidate arrays are written at pose * K + c with
// c < K; per-pose arrays at pose < n_poses; best_traj at most at entry n_steps of its pose.
//
// This file is NOT one of the product library's objects.  It is linked, with all of libssf_hip_live.so's, into libssf_hip_steer.so.
#include "ssf_navsteer_walk.hpp"

namespace ssf {

// the largest window staged; the roll kernel's static LDS (direction table, four keys, the sums); a CU's LDS, an eighth of it, and the
// CUs of the part
enum { NS_LDS_CELLS = 14336, NS_STATIC_LDS = 4 * NS_DIRS + 160, NS_CU_LDS = 160 * 1024, NS_LDS_FREE = NS_CU_LDS / 8, NS_CUS = 256 };

// ---- pack: one thread per cell (step 3) ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navsteer_pack(size_t P, int min_dist2, int allow_unknown, int cap, const int8_t* __restrict__ state,
                                                       const int32_t* __restrict__ dist2, uint32_t* __restrict__ pk) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    pk[p] = ns_disc_word(state[p], dist2[p], min_dist2, allow_unknown, cap);
}

// ---- roll: one workgroup per (pose, 256 candidates) (steps 4 to 7) ------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navsteer_roll(NavSteerRule r, const uint32_t* __restrict__ pk, const uint32_t* __restrict__ cost,
                                                       const int32_t* __restrict__ poses, const int32_t* __restrict__ targets,
                                                       const uint32_t* __restrict__ dirs, unsigned long long* __restrict__ keys,
                                                       int32_t* __restrict__ n_adm, NavSteerCand out, unsigned long long* __restrict__ stats) {
    __shared__ uint32_t s_dir[NS_DIRS];                               // (S << 16) | (C & 0xFFFF)
    ns_disc_roll(r, NsNoHook{}, s_dir, pk, cost, poses, targets, dirs, keys, n_adm, out, stats);
}

// ---- pick: one lane per pose (steps 7 and 8) -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navsteer_pick(NavSteerRule r, const uint32_t* __restrict__ pk, const int32_t* __restrict__ poses,
                                                       const uint32_t* __restrict__ dirs, const unsigned long long* __restrict__ keys,
                                                       const int32_t* __restrict__ n_adm, NavSteerPose out, unsigned long long* __restrict__ stats) {
    const NavSteerCells cells{pk, nullptr, r.W, 0, 0, 0, 0, false};
    ns_pick_body(r, cells, NsNoHook{}, [&](int cx, int cy, int) { return (pk[(size_t)cy * r.W + cx] & NS_TRAV) != 0; }, poses, dirs, keys, n_adm, out, stats);
}

static void launch_navsteer_pack(hipStream_t st, size_t P, const NavSteerRule& r, const int8_t* state, const int32_t* dist2, uint32_t* pk) {
    ScopedKernel sk("navsteer_pack", st);
    hipLaunchKernelGGL(k_navsteer_pack, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, P, r.min_dist2, r.allow_unknown, r.cap, state, dist2, pk);
}
static void launch_navsteer_roll(hipStream_t st, const NavSteerRule& r, const uint32_t* pk, const uint32_t* cost, const int32_t* poses, const int32_t* targets,
                                 const uint32_t* dirs, unsigned long long* keys, int32_t* n_adm, const NavSteerCand& out, unsigned long long* stats) {
    ScopedKernel sk("navsteer_roll", st);
    hipLaunchKernelGGL(k_navsteer_roll, dim3((unsigned)((r.K + 255) / 256), (unsigned)r.n_poses), dim3(256), navsteer_window_lds(r), st, r, pk, cost, poses,
                       targets, dirs, keys, n_adm, out, stats);
}
static void launch_navsteer_pick(hipStream_t st, const NavSteerRule& r, const uint32_t* pk, const int32_t* poses, const uint32_t* dirs,
                                 const unsigned long long* keys, const int32_t* n_adm, const NavSteerPose& out, unsigned long long* stats) {
    ScopedKernel sk("navsteer_pick", st);
    hipLaunchKernelGGL(k_navsteer_pick, dim3((unsigned)((r.n_poses + 255) / 256)), dim3(256), 0, st, r, pk, poses, dirs, keys, n_adm, out, stats);
}

}  // namespace ssf

// what is staged (the file's head: a measured choice); no output depends on it.  ssf_navdyn.hip's launch asks it as well: its roll
// kernel holds the mover list (1.5 KiB) in static LDS on top of NS_STATIC_LDS, which makes `roomy` slightly optimistic for it (a choice
// of speed, never of results) and must keep the largest staged window inside the 64 KiB a workgroup gets without opting in
static_assert(4 * ssf::NS_LDS_CELLS + ssf::NS_STATIC_LDS + 4 * SSF_NAVDYN_MAX_MOVERS * SSF_NAVDYN_MOVER_WORDS <= 64 * 1024,
              "the staged window, the roll kernel's static LDS and ssf_navdyn.hip's mover list no longer fit a workgroup's LDS");
int navsteer_stage_cells(const ssf::NavSteerRule& r) {
    using namespace ssf;
    const long long side = 2LL * r.R + 1, bound = std::min<long long>(side, r.W) * std::min<long long>(side, r.H);
    const long long bytes = 4 * std::min<long long>(bound, NS_LDS_CELLS) + NS_STATIC_LDS, wgs = (long long)((r.K + 255) / 256) * r.n_poses;
    const bool roomy = bytes <= NS_LDS_FREE || wgs <= (long long)NS_CUS * (NS_CU_LDS / bytes);
    return r.walk ? 0 : (roomy ? (int)NS_LDS_CELLS : (int)((NS_LDS_FREE - NS_STATIC_LDS) / 4));
}

namespace {
// the disc's part of a call (navsteer_call, ssf_navsteer_walk.hpp): the staging choice, the packed grid, the three launches
struct NavSteerRun {
    ssf_handle* h;
    int stage_cells(const ssf::NavSteerRule& r) const { return navsteer_stage_cells(r); }
    bool reserve(size_t P) { return navsteer_reserve_pk(h, P); }
    int launch(hipStream_t st, const ssf::NavSteerRule& r, const void* state, const int32_t* dist2, const uint32_t* cost, const int32_t* poses,
               const int32_t* targets, NavSteerWs& w, const ssf::NavSteerCand& cand, const ssf::NavSteerPose& pick) {
        ssf::launch_navsteer_pack(st, (size_t)r.W * r.H, r, (const int8_t*)state, dist2, w.pk);
        HCK(hipGetLastError());
        ssf::launch_navsteer_roll(st, r, w.pk, cost, poses, targets, w.dirs, w.keys, w.n_adm, cand, w.stats);
        HCK(hipGetLastError());
        ssf::launch_navsteer_pick(st, r, w.pk, poses, w.dirs, w.keys, w.n_adm, pick, w.stats);
        HCK(hipGetLastError());
        return SSF_OK;
    }
};
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
    NavSteerRun run{h};
    return navsteer_call(h, "ssf_navsteer_rollouts", p, state, 1, "state", dist2, cost, poses, targets, out, stats, run);
}
}  // extern "C"
