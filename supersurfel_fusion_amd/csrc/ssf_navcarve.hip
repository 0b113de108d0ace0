// ssf_navcarve.hip -- the navigation grid with free space carved along camera rays (include/ssf_navcarve.h) on gfx950.
//
// What is computed is pinned, operation by operation, in include/ssf_navcarve.h (the numpy restatement: tests/navcarve_ref.py).
// ssf_navgrid_carve runs ssf_navgrid_build's own prep, fill and tile (ssf_navgrid.hpp), then per chunk of at most 2^20 rays
//   * rays     k_navcarve_rays: one thread per ray: the pixel's direction through the view's pose, (O, D) in the map frame;
//   * the hit  ssf_raycast itself, on the device buffers, with the identity pose (raycast_* kernels; its resident index is reused);
//   * march    k_navcarve_march: one ray per wave, its samples over the lanes (nav_march_ray, ssf_navgrid.hpp, shared with the live
//              layer); the entries of a cell's band are counted into `seen` with integer atomics (order-free), merged in registers
//              where neighbouring rays share their first cells;
// and the cells kernel's carving sibling, with `seen` as one more input of the state.  Its working set is NavCarveWs (ssf_handle.hpp).
//
// This file is NOT one of the product library's objects: libssf_hip.so's exported symbols stay what they were.  It is linked,
// with all of the product's objects, into libssf_hip_navcarve.so (csrc/Makefile), which is what a caller of the carve loads.
#include "ssf_navgrid.hpp"
#include "ssf_raycast.hpp"
#include "../../include/ssf_navcarve.h"
#include "../../include/ssf_navcarve_testing.h"

namespace ssf {

__global__ __launch_bounds__(256) void k_navcarve_cells(NavAcc acc, size_t P, int min_hits, NavOut out, unsigned long long* __restrict__ stats, NavSeen sn) {
    navgrid_cells_body<true>(acc, P, min_hits, out, stats, sn);
}

// ---- carving: rays of the views' pixel lattices, and their walk through the grid (include/ssf_navcarve.h) ---------------------
// rays: one thread per ray of a chunk [first, first + n) of all rays; ray r = (view * nv + j) * nu + i -> (O, D) in the map frame (step 2)
struct NavCam { float fx, fy, cx, cy; int nu, nv, stride; };
__global__ __launch_bounds__(256) void k_navcarve_rays(NavCam cam, const float* __restrict__ views, int first, int n, float* __restrict__ rays) {
    const int k0 = blockIdx.x * 256 + threadIdx.x;
    if (k0 >= n) return;
    const int r = first + k0;
    const int i = r % cam.nu, q = r / cam.nu, j = q % cam.nv, view = q / cam.nv;
    const int u = i * cam.stride + cam.stride / 2, v = j * cam.stride + cam.stride / 2;
    const float x = ((float)u - cam.cx) / cam.fx, y = ((float)v - cam.cy) / cam.fy;
    const float l = sqrtf((x * x + y * y) + 1.0f);
    const float dx = x / l, dy = y / l, dz = 1.0f / l;
    const float* T = views + 12 * (size_t)view;
    const float o = 0.0f;                                             // the camera-frame origin, through ssf_raycast.h step 1 as written
    float* out = rays + 6 * (size_t)k0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float a = T[3 * k], b = T[3 * k + 1], c = T[3 * k + 2];
        out[k] = ((a * o + b * o) + c * o) + T[9 + k];
        out[3 + k] = (a * dx + b * dy) + c * dz;
    }
}

// march: ONE RAY PER WAVE, like k_raycast_march; a wave takes NC_RUN consecutive rays (neighbouring pixels of one view) through
// nav_march_ray (ssf_navgrid.hpp: steps 5 and 6).  The counters go out with per-wave atomics from lane 0.
enum { NC_RUN = 16 };
__global__ __launch_bounds__(256) void k_navcarve_march(NavGrid G, int n, const float* __restrict__ rays, const float* __restrict__ tt,
                                                        const int32_t* __restrict__ index, float margin, float tmax, int carve_misses,
                                                        uint32_t* __restrict__ seen, unsigned long long* __restrict__ stats) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const long long first = (long long)wave * NC_RUN;
    const int r0 = (int)min(first, (long long)n), r1 = (int)min(first + NC_RUN, (long long)n);
    unsigned long long n_carving = 0, n_samples = 0, n_entries = 0, n_atomics = 0;       // the first two: the same in every lane
    int pend_cell = -1; uint32_t pend_n = 0u;
    for (int ray = r0; ray < r1; ray++) {
        const float* in = rays + 6 * (size_t)ray;
        NavMarchRay r;
#pragma unroll
        for (int k = 0; k < 3; k++) { r.O[k] = in[k]; r.D[k] = in[3 + k]; }
        const bool valid = finite3(r.O[0], r.O[1], r.O[2]) && finite3(r.D[0], r.D[1], r.D[2]) && !(r.D[0] == 0.0f && r.D[1] == 0.0f && r.D[2] == 0.0f);
        float t_end = -1.0f;
        if (index[ray] >= 0) t_end = tt[ray] - margin;
        else if (valid && carve_misses) t_end = tmax;
        const int M = t_end >= 0.0f ? (int)floorf(t_end / G.step) : -1;
        if (M < 0) continue;                                          // (wave-uniform)
        n_carving++; n_samples += (unsigned long long)(M + 1);
        nav_march_ray(G, r, M, seen, pend_cell, pend_n, n_entries, n_atomics);
    }
    if (pend_n) { atomicAdd(&seen[pend_cell], pend_n); n_atomics++; }
    n_entries = wave_sum(n_entries); n_atomics = wave_sum(n_atomics);
    if (lane() == 0) {
        if (n_carving) atomicAdd(&stats[NC_CARVING], n_carving);
        if (n_samples) atomicAdd(&stats[NC_SAMPLES], n_samples);
        if (n_entries) atomicAdd(&stats[NC_ENTRIES], n_entries);
        if (n_atomics) atomicAdd(&stats[NC_ATOMICS], n_atomics);
    }
}

static void launch_navcarve_cells(hipStream_t st, const NavGrid& G, const NavAcc& acc, const NavOut& out, unsigned long long* stats, const NavSeen* sn) {
    ScopedKernel sk("navgrid_cells", st);
    const size_t P = (size_t)G.W * G.H;
    hipLaunchKernelGGL(k_navcarve_cells, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, acc, P, G.min_hits, out, stats, *sn);
}
static void launch_navcarve_rays(hipStream_t st, const NavCam& cam, const float* views, int first, int n, float* rays) {
    ScopedKernel sk("navcarve_rays", st);
    hipLaunchKernelGGL(k_navcarve_rays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cam, views, first, n, rays);
}
static void launch_navcarve_march(hipStream_t st, const NavGrid& G, int n, const float* rays, const float* tt, const int32_t* index, float margin,
                                  float tmax, int carve_misses, uint32_t* seen, unsigned long long* stats) {
    ScopedKernel sk("navcarve_march", st);
    const unsigned waves = (unsigned)((n + NC_RUN - 1) / NC_RUN);
    hipLaunchKernelGGL(k_navcarve_march, dim3((waves + 3) / 4), dim3(256), 0, st, G, n, rays, tt, index, margin, tmax, carve_misses, seen, stats);
}

}  // namespace ssf

extern "C" {
int ssf_navcarve_default_params(const ssf_handle* h, ssf_navcarve_params* c) {
    if (!h || !c) return SSF_ERR_INVALID_ARG;
    std::memset(c, 0, sizeof(*c));
    c->stride = 8; c->hit_margin_cells = 1.0f; c->min_seen = 1;
    return SSF_OK;
}

int ssf_navgrid_carve(ssf_handle* h, const ssf_navgrid_params* g, const ssf_navcarve_params* cp, const ssf_navcarve_out* out,
                      ssf_navcarve_stats* stats) {
    if (!h || !g || !cp) return SSF_ERR_INVALID_ARG;
    auto refuse = [&](const char* what) { h->err = std::string("ssf_navgrid_carve: ") + what; return SSF_ERR_INVALID_ARG; };
    if (!out || (!out->grid.zmin && !out->grid.zmax && !out->grid.hits && !out->grid.state && !out->grid.dist2 && !out->seen))
        return refuse("every output is NULL");
    if (const char* what = navgrid_size_res(g)) return refuse(what);
    // the views and their camera
    if (cp->n_views < 0 || cp->n_views > 4096) return refuse("n_views must be 0..4096");
    if (cp->n_views > 0 && !cp->views) return refuse("views is NULL");
    NavCam cam{cp->fx, cp->fy, cp->cx, cp->cy, 0, 0, cp->stride};
    int cw = cp->cam_width, ch = cp->cam_height;
    if (cw == 0) { cam.fx = h->cfg.fx; cam.fy = h->cfg.fy; cam.cx = h->cfg.cx; cam.cy = h->cfg.cy; cw = h->cfg.width; ch = h->cfg.height; }
    if (cw < 1 || cw > 8192 || ch < 1 || ch > 8192) return refuse("cam_width and cam_height must be 1..8192");
    if (!std::isfinite(cam.fx) || !std::isfinite(cam.fy) || !(cam.fx > 0.0f) || !(cam.fy > 0.0f) || !std::isfinite(cam.cx) || !std::isfinite(cam.cy))
        return refuse("fx and fy must be finite and > 0, cx and cy finite");
    if (cp->stride < 1 || cp->stride > 64) return refuse("stride must be 1..64");
    cam.nu = cw / cp->stride; cam.nv = ch / cp->stride;
    if (cam.nu < 1 || cam.nv < 1) return refuse("the stride leaves no pixel lattice");
    if (!(cp->hit_margin_cells >= 0.0f) || !std::isfinite(cp->hit_margin_cells)) return refuse("hit_margin_cells must be finite and >= 0");
    if (cp->min_seen < 1) return refuse("min_seen must be >= 1");
    // the ray cast's part, by the ray cast's own check (ssf_raycast would refuse the same, but only once rays are cast)
    ssf_raycast_params rp;
    (void)ssf_raycast_default_params(h, &rp);
    const float identity[12] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f};
    rp.pose = identity; rp.t_min = cp->t_min; rp.t_max = cp->t_max; rp.min_conf = cp->ray_min_conf; rp.splat_scale = cp->ray_splat_scale;
    rp.visible_only = 0; rp.on_device = 1;
    RaycastResolved rr;
    if (const char* what = raycast_params_refusal(h, &rp, rr)) return refuse((std::string("the ray cast: ") + what).c_str());
    const float tmax = rr.tmax;
    const float step = g->res * 0.5f;
    if (!(tmax / step <= 65535.0f)) return refuse("t_max / (res / 2) must be <= 65535");
    const long long per_view = (long long)cam.nu * cam.nv, n_rays = per_view * cp->n_views;
    if (n_rays > 0x7FFFFFFFll) return refuse("more than 2^31 - 1 rays");
    NavCall c;
    c.who = "ssf_navgrid_carve";
    { int rc = navgrid_begin(h, g, c); if (rc) return rc; }
    const size_t P = c.P;
    NavOut o{out->grid.zmin, out->grid.zmax, out->grid.hits, out->grid.state};
    int32_t* d2 = out->grid.dist2;
    uint32_t* seen_out = out->seen;
    StagedIo io;
    if (!g->on_device) {
        io.out(out->grid.zmin, 4 * P, &o.zmin); io.out(out->grid.zmax, 4 * P, &o.zmax); io.out(out->grid.hits, 8 * P, &o.hits);
        io.out(out->grid.state, P, &o.state); io.out(out->grid.dist2, 4 * P, &d2); io.out(out->seen, 4 * P, &seen_out);
    }
    { int rc = navgrid_reserve(h, g, c, io); if (rc) return rc; }
    // the carve's own buffers: the views, a chunk of rays with their hits, the entries per cell, the sums
    NavCarveWs& w = h->navcarve;
    const long long chunk_rays = w.chunk_rays > 0 ? w.chunk_rays : (1ll << 20);          // 24 MB of rays + 8 MB of hits
    const size_t cap = (size_t)std::min<long long>(n_rays, chunk_rays);
    bool ok = true;
    if (!w.stats) ok = w.bufs.grow({{(void**)&w.stats, NC_STATS * sizeof(unsigned long long)}, {(void**)&w.views, 4096 * 12 * sizeof(float)}});
    if (ok && P > w.cells) { ok = w.bufs.grow({{(void**)&w.seen, 4 * P}}); if (ok) w.cells = P; }
    if (ok && cap > w.ray_cap) {
        ok = w.bufs.grow({{(void**)&w.rays, 24 * cap}, {(void**)&w.t, 4 * cap}, {(void**)&w.index, 4 * cap}});
        if (ok) w.ray_cap = cap;
    }
    if (!ok) { h->err = "ssf_navgrid_carve: allocation of the working buffers failed"; return SSF_ERR_DEVICE; }
    hipStream_t st = h->stream;
    {
        TimerScope ts(h);
        int rc = navgrid_accumulate(h, g, c);
        if (rc) return rc;
        HCK(hipMemsetAsync(w.stats, 0, NC_STATS * sizeof(unsigned long long), st));
        HCK(hipMemsetAsync(w.seen, 0, 4 * P, st));
        if (cp->n_views > 0) HCK(hipMemcpyAsync(w.views, cp->views, 12 * sizeof(float) * (size_t)cp->n_views, hipMemcpyHostToDevice, st));
    }
    long long hit = 0, invalid = 0, chunks = 0;
    for (long long r0 = 0; r0 < n_rays; r0 += chunk_rays, chunks++) {
        const int n = (int)std::min<long long>(chunk_rays, n_rays - r0);
        { TimerScope ts(h); launch_navcarve_rays(st, cam, w.views, (int)r0, n, w.rays); HCK(hipGetLastError()); }
        ssf_raycast_stats rs;
        { int rc = ssf_raycast(h, &rp, w.rays, n, w.t, w.index, nullptr, nullptr, nullptr, &rs); if (rc) return rc; }    // (synchronises)
        hit += rs.rays_hit; invalid += rs.rays_invalid;
        TimerScope ts(h);
        launch_navcarve_march(st, c.G, n, w.rays, w.t, w.index, cp->hit_margin_cells * g->res, tmax, cp->carve_misses != 0, w.seen, w.stats);
        HCK(hipGetLastError());
    }
    TimerScope ts(h);
    const NavSeen sn{w.seen, cp->min_seen, seen_out, w.stats};
    unsigned long long s6[6] = {0, 0, 0, 0, 0, 0};
    { int rc = navgrid_finish(h, g, c, o, d2, io, launch_navcarve_cells, &sn, stats ? &stats->grid : nullptr, s6); if (rc) return rc; }
    w.last_chunks = chunks; w.last_atomics = (long long)s6[NC_ATOMICS];
    if (stats) {
        stats->rays = n_rays; stats->rays_hit = hit; stats->rays_invalid = invalid;
        stats->rays_carving = (int64_t)s6[NC_CARVING]; stats->ray_samples = (int64_t)s6[NC_SAMPLES]; stats->ray_entries = (int64_t)s6[NC_ENTRIES];
        stats->cells_seen = (int64_t)s6[NC_SEEN]; stats->cells_carved = (int64_t)s6[NC_CARVED];
    }
    return SSF_OK;
}

// test and measurement hooks of the carve (include/ssf_navcarve_testing.h): the rays per chunk (0 = the default 2^20), and what the last
// call did: its chunks and the atomics it issued on `seen`
int ssf_debug_navcarve_set_chunk_rays(ssf_handle* h, int max_rays) {
    if (!h || max_rays < 0 || max_rays > (1 << 24)) return SSF_ERR_INVALID_ARG;
    h->navcarve.chunk_rays = max_rays;
    return SSF_OK;
}
int ssf_debug_navcarve_last(const ssf_handle* h, int64_t* chunks, int64_t* atomics) {
    if (!h) return SSF_ERR_INVALID_ARG;
    if (chunks) *chunks = h->navcarve.last_chunks;
    if (atomics) *atomics = h->navcarve.last_atomics;
    return SSF_OK;
}
}  // extern "C"
