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
enum { NL_TW = 16, NL_TH = 16, NL_RUN = 16 };

// (the camera of the frame and the depth of a pixel: ssf_navlive.hpp, shared with ssf_navdyn.hip; the cell of a point and the march of
// a ray: ssf_navgrid.hpp, shared with the carve; the sums: block_sums, ssf_slots.hpp, with NL_PAD as its stride)

// ---- stamp: steps 1 to 3 ---------------------------------------------------------------------------------------------------
template <int DF>
__global__ __launch_bounds__(256) void k_navlive_stamp(NavGrid G, NavLiveCam cam, const void* __restrict__ depth, double scale,
                                                       const uint8_t* __restrict__ mask, int mask_mode, uint32_t* __restrict__ hits,
                                                       unsigned long long* __restrict__ stats) {
    __shared__ int s_cell[NL_TW * (NL_TH + 1)];                       // column x at x * (NL_TH + 1): the transposing write spreads over the banks
    const int ntx = (cam.W + NL_TW - 1) / NL_TW;
    const int t = threadIdx.x;
    const int u = (int)(blockIdx.x % ntx) * NL_TW + (t & (NL_TW - 1)), v = (int)(blockIdx.x / ntx) * NL_TH + (t >> 4);
    int c = -1;
    bool valid = false, stamping = false;
    if (u < cam.W && v < cam.H) {
        const size_t p = (size_t)v * cam.W + u;
        const float d = navlive_load_depth<DF>(depth, p, scale);
        valid = isfinite(d) && d >= cam.tmin && d <= cam.tmax;
        stamping = valid && (mask_mode == 0 || (mask[p] != 0) == (mask_mode == 1));
        if (stamping) {
            float Sx, Sy, Sz;
            navlive_pixel_point(cam, u, v, d, Sx, Sy, Sz);
            c = nav_cell(G, Sx, Sy, Sz);
        }
    }
    s_cell[(t & (NL_TW - 1)) * (NL_TH + 1) + (t >> 4)] = c;
    __syncthreads();
    // thread t now holds pixel (x = t / 16, y = t % 16) of the tile: a lane's predecessor is the pixel above it
    const int cc = s_cell[(t >> 4) * (NL_TH + 1) + (t & (NL_TH - 1))];
    const int ln = lane();
    const int above = __shfl_up(cc, 1, 64);
    const bool head = ln == 0 || cc != above;
    const unsigned long long heads = __ballot(head);
    unsigned long long n_atomics = 0;
    if (head && cc >= 0) {
        const unsigned long long next = ln == 63 ? 0ull : heads >> (ln + 1);
        const int len = next ? __builtin_ctzll(next) + 1 : 64 - ln;   // lanes up to the next head: all of this cell
        atomicAdd(&hits[cc], (uint32_t)len);
        n_atomics = 1;
    }
    block_sums({valid, stamping, c >= 0, n_atomics}, stats, NL_VALID, NL_PAD);
}

// ---- march: step 4 ---------------------------------------------------------------------------------------------------------
template <int DF>
__global__ __launch_bounds__(256) void k_navlive_march(NavGrid G, NavLiveCam cam, const void* __restrict__ depth, double scale, float margin,
                                                       uint32_t* __restrict__ seen, unsigned long long* __restrict__ stats) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int ln = lane();
    const int n = cam.nu * cam.nv;
    const long long first = (long long)wave * NL_RUN;
    const int r0 = (int)min(first, (long long)n), r1 = (int)min(first + NL_RUN, (long long)n);
    unsigned long long n_rays = 0, n_carving = 0, n_samples = 0, n_entries = 0, n_atomics = 0;      // the first three: the same in every lane
    int pend_cell = -1; uint32_t pend_n = 0u;
    for (int ray = r0; ray < r1; ray++) {
        const int i = ray % cam.nu, j = ray / cam.nu;
        const int u = i * cam.stride + cam.stride / 2, v = j * cam.stride + cam.stride / 2;      // u < W, v < H: nu = W / stride
        const float d = navlive_load_depth<DF>(depth, (size_t)v * cam.W + u, scale);
        if (!(isfinite(d) && d >= cam.tmin && d <= cam.tmax)) continue;                          // (wave-uniform)
        n_rays++;
        const float x = ((float)u - cam.cx) / cam.fx, y = ((float)v - cam.cy) / cam.fy;
        const float l = sqrtf((x * x + y * y) + 1.0f);
        const float dx = x / l, dy = y / l, dz = 1.0f / l;
        const float o = 0.0f;                                         // the camera-frame origin, through ssf_raycast.h step 1 as written
        NavMarchRay r;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float a = cam.R[3 * k], b = cam.R[3 * k + 1], c = cam.R[3 * k + 2];
            r.O[k] = ((a * o + b * o) + c * o) + cam.t[k];
            r.D[k] = (a * dx + b * dy) + c * dz;
        }
        const bool rvalid = finite3(r.O[0], r.O[1], r.O[2]) && finite3(r.D[0], r.D[1], r.D[2]) && !(r.D[0] == 0.0f && r.D[1] == 0.0f && r.D[2] == 0.0f);
        const float t_end = (d * l) - margin;
        const int M = rvalid && t_end >= 0.0f ? (int)floorf(t_end / G.step) : -1;                  // <= 65535: the refusal of the corners
        if (M < 0) continue;
        n_carving++; n_samples += (unsigned long long)(M + 1);
        nav_march_ray(G, r, M, seen, pend_cell, pend_n, n_entries, n_atomics);
    }
    if (pend_n) { atomicAdd(&seen[pend_cell], pend_n); n_atomics++; }
    // the sums of the workgroup's four waves (rays and samples: one lane speaks for its wave)
    block_sums({ln == 0 ? n_carving : 0ull, ln == 0 ? n_samples : 0ull, n_entries, n_atomics}, stats, NL_CARVING, NL_PAD);
    block_sums({ln == 0 ? n_rays : 0ull}, stats, NL_RAYS, NL_PAD);
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
    const unsigned tiles = (unsigned)(((cam.W + NL_TW - 1) / NL_TW) * ((cam.H + NL_TH - 1) / NL_TH));
    if (df == SSF_DEPTH_U16_SCALED)
        hipLaunchKernelGGL(k_navlive_stamp<SSF_DEPTH_U16_SCALED>, dim3(tiles), dim3(256), 0, st, G, cam, depth, scale, mask, mask_mode, hits, stats);
    else
        hipLaunchKernelGGL(k_navlive_stamp<SSF_DEPTH_F32_METRES>, dim3(tiles), dim3(256), 0, st, G, cam, depth, scale, mask, mask_mode, hits, stats);
}
static void launch_navlive_march(hipStream_t st, int df, const NavGrid& G, const NavLiveCam& cam, const void* depth, double scale, float margin,
                                 uint32_t* seen, unsigned long long* stats) {
    ScopedKernel sk("navlive_march", st);
    const unsigned waves = (unsigned)((cam.nu * cam.nv + NL_RUN - 1) / NL_RUN);
    if (df == SSF_DEPTH_U16_SCALED)
        hipLaunchKernelGGL(k_navlive_march<SSF_DEPTH_U16_SCALED>, dim3((waves + 3) / 4), dim3(256), 0, st, G, cam, depth, scale, margin, seen, stats);
    else
        hipLaunchKernelGGL(k_navlive_march<SSF_DEPTH_F32_METRES>, dim3((waves + 3) / 4), dim3(256), 0, st, G, cam, depth, scale, margin, seen, stats);
}
static void launch_navlive_cells(hipStream_t st, size_t P, const NavLiveRule& rule, const int8_t* state_in, const uint32_t* hits, const uint32_t* seen,
                                 uint32_t* out_hits, uint32_t* out_seen, int8_t* out_state, unsigned long long* stats) {
    ScopedKernel sk("navlive_cells", st);
    hipLaunchKernelGGL(k_navlive_cells, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, P, rule, state_in, hits, seen, out_hits, out_seen, out_state,
                       stats);
}

}  // namespace ssf

// [a, a + na) and [b, b + nb) share a byte (a NULL array shares nothing)
static bool navlive_overlap(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

extern "C" {
int ssf_navlive_default_params(const ssf_handle* h, ssf_navlive_params* p) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    ssf_navgrid_params g;
    { int rc = ssf_navgrid_default_params(h, &g); if (rc) return rc; }
    std::memset(p, 0, sizeof(*p));
    p->width = g.width; p->height = g.height; p->res = g.res; p->floor_max = g.floor_max; p->z_max = g.z_max;
    p->max_dist_cells = g.max_dist_cells; p->unknown_is_obstacle = g.unknown_is_obstacle;
    p->min_hits = 4; p->stride = 4; p->hit_margin_cells = 1.0f; p->min_seen = 1; p->open_unknown = 1;
    return SSF_OK;
}

int ssf_navlive_overlay(ssf_handle* h, const ssf_navlive_params* p, const void* depth, const uint8_t* mask, const int8_t* state_in,
                        const ssf_navlive_out* out, ssf_navlive_stats* stats) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    auto refuse = [&](const char* what) { h->err = std::string("ssf_navlive_overlay: ") + what; return SSF_ERR_INVALID_ARG; };
    if (!depth) return refuse("depth is NULL");
    if (!state_in) return refuse("state_in is NULL");
    if (!out || (!out->live_hits && !out->live_seen && !out->state && !out->dist2)) return refuse("every output is NULL");
    // the grid
    ssf_navgrid_params g;
    (void)ssf_navgrid_default_params(h, &g);
    g.width = p->width; g.height = p->height; g.res = p->res;
    if (const char* what = navgrid_size_res(&g)) return refuse(what);
    if (p->max_dist_cells < 1 || p->max_dist_cells > 1024) return refuse("max_dist_cells must be 1..1024");
    if (p->min_hits < 1) return refuse("min_hits must be >= 1");
    if (std::isnan(p->floor_max) || std::isnan(p->z_max)) return refuse("floor_max or z_max is a NaN");
    // the camera and its lattice
    NavLiveCam cam{};
    if (const char* what = navlive_pinhole(h, p->fx, p->fy, p->cx, p->cy, p->cam_width, p->cam_height, cam)) return refuse(what);
    if (p->stride < 1 || p->stride > 64) return refuse("stride must be 1..64");
    cam.stride = p->stride; cam.nu = cam.W / p->stride; cam.nv = cam.H / p->stride;
    if (cam.nu < 1 || cam.nv < 1) return refuse("the stride leaves no pixel lattice");
    if (!(p->hit_margin_cells >= 0.0f) || !std::isfinite(p->hit_margin_cells)) return refuse("hit_margin_cells must be finite and >= 0");
    if (p->min_seen < 1) return refuse("min_seen must be >= 1");
    if (const char* what = navlive_range(h, p->t_min, p->t_max, cam)) return refuse(what);
    if (p->mask_mode < 0 || p->mask_mode > 2) return refuse("mask_mode must be 0..2");
    if (p->mask_mode != 0 && !mask) return refuse("mask is NULL with mask_mode != 0");
    const int df = h->in_depth;
    const size_t bpp = df == SSF_DEPTH_U16_SCALED ? 2 : 4;
    if (p->frame_on_device && (uintptr_t)depth % bpp) return refuse("the device depth pointer is not aligned for the input format");
    // the sample index is bounded: l is largest at a corner of the image
    const float step = p->res * 0.5f;
    for (int k = 0; k < 4; k++) {
        const int u = (k & 1) ? cam.W - 1 : 0, v = (k & 2) ? cam.H - 1 : 0;
        const float x = ((float)u - cam.cx) / cam.fx, y = ((float)v - cam.cy) / cam.fy;
        const float l = sqrtf((x * x + y * y) + 1.0f);
        if (!((cam.tmax * l) / step <= 65535.0f)) return refuse("(t_max * l) / (res / 2) must be <= 65535 at the image's corners");
    }
    const size_t P = (size_t)p->width * p->height, npix = (size_t)cam.W * cam.H;
    const bool dev = p->on_device != 0, fdev = p->frame_on_device != 0;
    // overlaps: the outputs among themselves and with the inputs that live in the same memory; state == state_in is the update in place
    {
        const void* a[7] = {out->live_hits, out->live_seen, out->state, out->dist2, state_in, depth, p->mask_mode ? mask : nullptr};
        const size_t n[7] = {4 * P, 4 * P, P, 4 * P, P, bpp * npix, npix};
        for (int i = 0; i < 4; i++)
            for (int j = i + 1; j < 7; j++) {
                if (j >= 5 && dev != fdev) continue;                  // (a host range and a device range are no overlap)
                if (i == 2 && j == 4 && out->state == state_in) continue;
                if (navlive_overlap(a[i], n[i], a[j], n[j])) return refuse("arrays overlap (only state == state_in may)");
            }
    }
    { int rc = model_at_rest(h, "ssf_navlive_overlay", "overlays no frame"); if (rc) return rc; }

    float gpose[12];
    NavGrid G{};
    { int rc = navlive_frames(h, &g, p->grid_pose, p->cam_pose, G, cam, gpose); if (rc) return rc; }
    G.W = p->width; G.H = p->height; G.res = p->res; G.step = step; G.fW = (float)G.W; G.fH = (float)G.H;
    G.zmax = p->z_max; G.floor_max = p->floor_max;

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
    unsigned long long padded[NL_STATS * NL_PAD], s[NL_STATS];
    HCK(hipMemcpyAsync(padded, w.stats, sizeof(padded), hipMemcpyDeviceToHost, st));
    HCK(io.copy_out(st));
    { int rc = sync_collect(h); if (rc) return rc; }
    for (int k = 0; k < NL_STATS; k++) s[k] = padded[k * NL_PAD];
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
