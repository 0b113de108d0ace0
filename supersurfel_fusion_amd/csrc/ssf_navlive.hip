// ssf_navlive.hip -- the live obstacle layer (include/ssf_navlive.h) on gfx950: the depth frame stamped onto a navigation grid.
//
// What is computed is pinned, operation by operation, in include/ssf_navlive.h (the numpy restatement: tests/navlive_ref.py).
//   * stamp   k_navlive_stamp: a workgroup per 16 x 16 pixel tile, a thread per pixel: depth, point, cell.  The cells go through LDS
//             and come back column-major, so that a wave holds four runs of 16 vertically adjacent pixels: with an upright camera a
//             pixel column of a wall lands in one cell, and a run of lanes with one cell issues ONE atomicAdd of the run's length.
//             The result never depends on the merge: a rolled camera merges less and counts the same.
//   * march   k_navlive_march: the carve's march (nav_march_ray, ssf_navgrid.hpp) for a single-origin bundle: one ray per wave, its samples over
//             the lanes, NL_RUN consecutive lattice pixels per wave; the ray is made from the depth image in place (no ray buffer, no
//             ray cast: the hit is the pixel's own depth).  Every ray starts in the camera's own cell: what a lane would add for a
//             sample m < 64 of consecutive rays to one cell is merged in its registers, as in the carve.
//   * cells   k_navlive_cells: one thread per cell: the state of step 5 and the cell stats;
// then the clearance of ssf_navgrid.hip (navgrid_columns, navgrid_rows) on that state.  Its working set is NavLiveWs (ssf_handle.hpp).
// The depth-frame front end -- the tile pixel and its point, the transpose, the run heads, the pixel's ray and the wave's loop over its
// rays, the shared refusals, the overlap check -- is ssf_navlive.hpp's, one copy for this file, ssf_navmem.hip and ssf_navdyn.hip: what
// is here is the overlay's own (the entry count of the march, the rule of the cells, min_seen and the NaN test of the band).
//
// This file is NOT one of the product library's objects, nor of the four older navigation libraries: it is linked with
// libssf_hip_drive.so's objects into libssf_hip_live.so (csrc/Makefile), which is what a caller of the overlay loads.
#include "ssf_navlive.hpp"
#include "../../include/ssf_navlive.h"

namespace ssf {

// the sums the host reads (the unknown cells are the rest of the grid).  Every workgroup adds to them, so each sum has a 128-byte line
// of its own: sum k is word k * NL_PAD, and the additions to different sums do not queue behind one another
// (a kernel's sums are consecutive, as block_sums wants them: the stamp and the march count their atomics apart)
enum { NL_VALID = 0, NL_STAMPING, NL_POINTS, NL_STAMP_ATOMICS, NL_CARVING, NL_SAMPLES, NL_ENTRIES, NL_MARCH_ATOMICS, NL_RAYS, NL_STAMPED, NL_OPENED,
       NL_FREE, NL_OCC, NL_STATS = 13, NL_PAD = 16 };
// (the cell of a point and the march of a ray: ssf_navgrid.hpp, shared with the carve; the sums: block_sums, ssf_slots.hpp, with NL_PAD as its stride)

// ---- stamp: steps 1 to 3 ---------------------------------------------------------------------------------------------------
template <int DF>
__global__ __launch_bounds__(256) void k_navlive_stamp(NavGrid G, NavLiveCam cam, const void* __restrict__ depth, double scale,
                                                       const uint8_t* __restrict__ mask, int mask_mode, uint32_t* __restrict__ hits,
                                                       unsigned long long* __restrict__ stats) {
    __shared__ int s_cell[NL_TILE_LDS];
    int c = -1;
    bool valid, stamping;
    float Sx, Sy, Sz;
    if (navlive_tile_point<DF>(cam, depth, scale, mask, mask_mode, valid, stamping, Sx, Sy, Sz)) c = nav_cell(G, Sx, Sy, Sz);
    s_cell[navlive_tile_put()] = c;
    __syncthreads();
    const int cc = s_cell[navlive_tile_get()];
    unsigned long long heads, n_atomics = 0;
    if (nav_run_head(cc, heads) && cc >= 0) {
        atomicAdd(&hits[cc], (uint32_t)nav_run_len(heads));           // the run's lanes: all of this cell
        n_atomics = 1;
    }
    block_sums({valid, stamping, c >= 0, n_atomics}, stats, NL_VALID, NL_PAD);
}

// ---- march: step 4 ---------------------------------------------------------------------------------------------------------
template <int DF>
__global__ __launch_bounds__(256) void k_navlive_march(NavGrid G, NavLiveCam cam, const void* __restrict__ depth, double scale, float margin,
                                                       uint32_t* __restrict__ seen, unsigned long long* __restrict__ stats) {
    unsigned long long n_entries = 0, n_atomics = 0;
    int pend_cell = -1; uint32_t pend_n = 0u;
    const NavRayCounts n = navlive_wave_rays<DF>(G.step, cam, depth, scale, margin, [&](const NavMarchRay& r, int M) {
        nav_march_ray(G, r, M, seen, pend_cell, pend_n, n_entries, n_atomics);
    });
    if (pend_n) { atomicAdd(&seen[pend_cell], pend_n); n_atomics++; }
    // the sums of the workgroup's four waves (rays and samples: one lane speaks for its wave)
    const bool one = lane() == 0;
    block_sums({one ? n.carving : 0ull, one ? n.samples : 0ull, n_entries, n_atomics}, stats, NL_CARVING, NL_PAD);
    block_sums({one ? n.rays : 0ull}, stats, NL_RAYS, NL_PAD);
}

// ---- cells: step 5 and the cell stats; one thread per cell -------------------------------------------------------------------
// state_in and out_state may be one array (a thread reads its cell before it writes it); seen: nullptr when the march was skipped
struct NavLiveRule { int min_hits, min_seen, open_unknown; };
__global__ __launch_bounds__(256) void k_navlive_cells(size_t P, NavLiveRule rule, const int8_t* state_in, const uint32_t* __restrict__ hits,
                                                       const uint32_t* __restrict__ seen, uint32_t* __restrict__ out_hits,
                                                       uint32_t* __restrict__ out_seen, int8_t* out_state, unsigned long long* __restrict__ stats) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long nstamped = 0, nopened = 0, nfree = 0, nocc = 0;
    if (p < P) {
        const int8_t in = state_in[p];
        const uint32_t nh = hits[p], ns = seen ? seen[p] : 0u;
        int8_t st = (int8_t)-1;
        if (in == 100 || nh >= (uint32_t)rule.min_hits) st = (int8_t)100;
        else if (in == 0 || (rule.open_unknown && ns >= (uint32_t)rule.min_seen)) st = (int8_t)0;
        nstamped = in != 100 && st == 100; nopened = in != 100 && in != 0 && st == 0;
        nocc = st == 100; nfree = st == 0;
        if (out_hits) out_hits[p] = nh;
        if (out_seen) out_seen[p] = ns;
        if (out_state) out_state[p] = st;
    }
    block_sums({nstamped, nopened, nfree, nocc}, stats, NL_STAMPED, NL_PAD);
}

static void launch_navlive_stamp(hipStream_t st, int df, const NavGrid& G, const NavLiveCam& cam, const void* depth, double scale, const uint8_t* mask,
                                 int mask_mode, uint32_t* hits, unsigned long long* stats) {
    ScopedKernel sk("navlive_stamp", st);
    navlive_by_depth_format(df, [&](auto DF) {
        hipLaunchKernelGGL(k_navlive_stamp<decltype(DF)::value>, dim3(navlive_tiles(cam.W, cam.H)), dim3(256), 0, st, G, cam, depth, scale, mask, mask_mode, hits,
                           stats);
    });
}
static void launch_navlive_march(hipStream_t st, int df, const NavGrid& G, const NavLiveCam& cam, const void* depth, double scale, float margin,
                                 uint32_t* seen, unsigned long long* stats) {
    ScopedKernel sk("navlive_march", st);
    navlive_by_depth_format(df, [&](auto DF) {
        hipLaunchKernelGGL(k_navlive_march<decltype(DF)::value>, dim3(navlive_march_groups(cam)), dim3(256), 0, st, G, cam, depth, scale, margin, seen, stats);
    });
}
static void launch_navlive_cells(hipStream_t st, size_t P, const NavLiveRule& rule, const int8_t* state_in, const uint32_t* hits, const uint32_t* seen,
                                 uint32_t* out_hits, uint32_t* out_seen, int8_t* out_state, unsigned long long* stats) {
    ScopedKernel sk("navlive_cells", st);
    hipLaunchKernelGGL(k_navlive_cells, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, P, rule, state_in, hits, seen, out_hits, out_seen, out_state,
                       stats);
}

}  // namespace ssf

extern "C" {
int ssf_navlive_default_params(const ssf_handle* h, ssf_navlive_params* p) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    { int rc = navlive_default_fields(h, p); if (rc) return rc; }
    p->min_seen = 1;
    return SSF_OK;
}

int ssf_navlive_overlay(ssf_handle* h, const ssf_navlive_params* p, const void* depth, const uint8_t* mask, const int8_t* state_in,
                        const ssf_navlive_out* out, ssf_navlive_stats* stats) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    auto refuse = [&](const char* what) { h->err = std::string("ssf_navlive_overlay: ") + what; return SSF_ERR_INVALID_ARG; };
    if (!depth) return refuse("depth is NULL");
    if (!state_in) return refuse("state_in is NULL");
    if (!out || (!out->live_hits && !out->live_seen && !out->state && !out->dist2)) return refuse("every output is NULL");
    // the grid, the overlay's own band, the camera and its lattice (ssf_navlive.hpp: shared with ssf_navmem_update)
    ssf_navgrid_params g;
    if (const char* what = navlive_refuse_grid(h, p, g)) return refuse(what);
    if (std::isnan(p->floor_max) || std::isnan(p->z_max)) return refuse("floor_max or z_max is a NaN");
    NavLiveCam cam{};
    size_t bpp = 0;
    if (const char* what = navlive_refuse_camera(h, p, depth, mask, p->min_seen < 1 ? "min_seen must be >= 1" : nullptr, cam, bpp)) return refuse(what);
    const int df = h->in_depth;
    const size_t P = (size_t)p->width * p->height, npix = (size_t)cam.W * cam.H;
    const bool dev = p->on_device != 0, fdev = p->frame_on_device != 0;
    // overlaps: the outputs among themselves and with the inputs that live in the same memory; state == state_in is the update in place
    {
        const void* a[7] = {out->live_hits, out->live_seen, out->state, out->dist2, state_in, depth, p->mask_mode ? mask : nullptr};
        const size_t n[7] = {4 * P, 4 * P, P, 4 * P, P, bpp * npix, npix};
        const int may[1][2] = {{2, 4}};
        if (navlive_arrays_overlap(a, n, 7, 4, 5, dev != fdev, may, 1)) return refuse("arrays overlap (only state == state_in may)");
    }
    { int rc = model_at_rest(h, "ssf_navlive_overlay", "overlays no frame"); if (rc) return rc; }

    float gpose[12];
    NavGrid G{};
    { int rc = navlive_frames(h, &g, p, p->res * 0.5f, G, cam, gpose); if (rc) return rc; }

    // the arrays: host ones are staged on the device
    const void* d_depth = depth; const uint8_t* d_mask = p->mask_mode ? mask : nullptr; const int8_t* d_in = state_in;
    uint32_t* o_hits = out->live_hits; uint32_t* o_seen = out->live_seen; int8_t* o_state = out->state; int32_t* o_dist2 = out->dist2;
    StagedIo io;
    if (!fdev) { io.in(depth, bpp * npix, &d_depth); io.in(d_mask, npix, &d_mask); }
    if (!dev) {
        io.in(state_in, P, &d_in);
        io.out(out->live_hits, 4 * P, &o_hits); io.out(out->live_seen, 4 * P, &o_seen); io.out(out->state, P, &o_state); io.out(out->dist2, 4 * P, &o_dist2);
    }
    NavLiveWs& w = h->navlive;
    bool ok = true;
    if (!w.stats) ok = w.bufs.grow({{(void**)&w.stats, NL_STATS * NL_PAD * sizeof(unsigned long long)}});
    if (ok && P > w.cells) {
        ok = w.bufs.grow({{(void**)&w.hits, 4 * P}, {(void**)&w.seen, 4 * P}, {(void**)&w.colg, 2 * P}, {(void**)&w.state, P}});
        if (ok) w.cells = P;
    }
    if (ok) ok = io.reserve(w.bufs, &w.img, &w.img_bytes, io.need());
    if (!ok) { h->err = "ssf_navlive_overlay: allocation of the working buffers failed"; return SSF_ERR_DEVICE; }

    hipStream_t st = h->stream;
    TimerScope ts(h);
    const bool march = out->live_seen != nullptr || p->open_unknown != 0;
    HCK(io.copy_in(st));
    HCK(hipMemsetAsync(w.stats, 0, NL_STATS * NL_PAD * sizeof(unsigned long long), st));
    HCK(hipMemsetAsync(w.hits, 0, 4 * P, st));
    if (march) HCK(hipMemsetAsync(w.seen, 0, 4 * P, st));
    launch_navlive_stamp(st, df, G, cam, d_depth, h->in_scale, d_mask, p->mask_mode, w.hits, w.stats);
    HCK(hipGetLastError());
    if (march) {
        launch_navlive_march(st, df, G, cam, d_depth, h->in_scale, p->hit_margin_cells * p->res, w.seen, w.stats);
        HCK(hipGetLastError());
    }
    if (o_dist2 && !o_state) o_state = w.state;                       // dist2 alone: the state is still computed, internally
    const NavLiveRule rule{p->min_hits, p->min_seen, p->open_unknown != 0};
    launch_navlive_cells(st, P, rule, d_in, w.hits, march ? w.seen : nullptr, o_hits, o_seen, o_state, w.stats);
    HCK(hipGetLastError());
    if (o_dist2) {
        launch_navgrid_clearance(st, o_state, G.W, G.H, p->max_dist_cells, p->unknown_is_obstacle != 0, w.colg, o_dist2);
        HCK(hipGetLastError());
    }
    NavPaddedSums<NL_STATS, NL_PAD> s;
    HCK(s.fetch(w.stats, st));
    HCK(io.copy_out(st));
    { int rc = sync_collect(h); if (rc) return rc; }
    if (stats) {
        stats->pixels_valid = (int64_t)s[NL_VALID]; stats->pixels_stamping = (int64_t)s[NL_STAMPING]; stats->points_in_band = (int64_t)s[NL_POINTS];
        stats->rays = (int64_t)s[NL_RAYS]; stats->rays_carving = (int64_t)s[NL_CARVING]; stats->ray_samples = (int64_t)s[NL_SAMPLES];
        stats->ray_entries = (int64_t)s[NL_ENTRIES]; stats->cells_stamped = (int64_t)s[NL_STAMPED]; stats->cells_opened = (int64_t)s[NL_OPENED];
        stats->cells_free = (int64_t)s[NL_FREE]; stats->cells_occupied = (int64_t)s[NL_OCC]; stats->cells_unknown = (int64_t)P - (int64_t)s[NL_FREE] - (int64_t)s[NL_OCC];
        stats->atomics = (int64_t)(s[NL_STAMP_ATOMICS] + s[NL_MARCH_ATOMICS]);
        std::memcpy(stats->pose, gpose, sizeof(gpose));
    }
    return SSF_OK;
}
}  // extern "C"
