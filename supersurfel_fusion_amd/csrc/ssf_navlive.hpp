// ssf_navlive.hpp -- the ONE front end of the calls that put a depth frame onto a navigation grid: ssf_navlive.hip (ssf_navlive_overlay),
// ssf_navmem.hip (ssf_navmem_update) and the blobs of ssf_navdyn.hip (ssf_navdyn_blobs).  Device: the camera, a pixel's depth, the tile
// pixel and its map-frame point (include/ssf_navlive.h steps 1 and 2; its grid point and cell: ssf_navgrid.hpp), the tile's transpose, the
// runs of lanes, the ray of a lattice pixel and a wave's loop over its rays (step 4).  Host: the launch by depth format, the shared
// refusals, the overlap check, the frames and the sums.  Private to the library's own files: nothing here is exported.
#pragma once
#include "ssf_navgrid.hpp"
#include "../../include/ssf_input.h"
#include <type_traits>

namespace ssf {

// the camera of the frame: pose (R row-major, t: camera-to-map), pinhole, image size, valid depths; the lattice of the rays
struct NavLiveCam { float R[9], t[3]; float fx, fy, cx, cy; int W, H; float tmin, tmax; int stride, nu, nv; };

// the tile of a stamping workgroup (256 threads, rows of 16 consecutive pixels: the loads coalesce) and the lattice pixels a marching wave takes
enum { NL_TW = 16, NL_TH = 16, NL_RUN = 16, NL_TILE_LDS = NL_TW * (NL_TH + 1) };

// the depth d of pixel q in the input format DF; true iff it is a valid one (ssf_navlive.h step 1)
template <int DF> __device__ __forceinline__ bool navlive_pixel_depth(const NavLiveCam& cam, const void* __restrict__ depth, size_t q, double scale, float& d) {
    if (DF == SSF_DEPTH_U16_SCALED) d = (float)((double)reinterpret_cast<const uint16_t*>(depth)[q] * scale);
    else d = reinterpret_cast<const float*>(depth)[q];
    return isfinite(d) && d >= cam.tmin && d <= cam.tmax;
}
// pixel (u, v) on the plane z = 1 of the camera, (x, y); returns the length l of (x, y, 1).  The kernels' and the host's (the corners)
__host__ __device__ __forceinline__ float navlive_pixel_dir(const NavLiveCam& cam, int u, int v, float& x, float& y) {
    x = ((float)u - cam.cx) / cam.fx; y = ((float)v - cam.cy) / cam.fy;
    return sqrtf((x * x + y * y) + 1.0f);
}
// the map-frame point of pixel (u, v) at depth d (ssf_navlive.h step 2)
__device__ __forceinline__ void navlive_pixel_point(const NavLiveCam& cam, int u, int v, float d, float& Sx, float& Sy, float& Sz) {
    float x, y;
    navlive_pixel_dir(cam, u, v, x, y);                               // (the length is not needed here)
    const float px = x * d, py = y * d;
    const float* R = cam.R;
    Sx = ((R[0] * px + R[1] * py) + R[2] * d) + cam.t[0];
    Sy = ((R[3] * px + R[4] * py) + R[5] * d) + cam.t[1];
    Sz = ((R[6] * px + R[7] * py) + R[8] * d) + cam.t[2];
}

// ---- a workgroup per 16 x 16 pixel tile, a thread per pixel ----------------------------------------------------------------------
// this thread's pixel (u, v) of the tile of workgroup blockIdx.x in a W x H image; p: its index; in: it is in the image
struct NavTilePixel { int u, v; size_t p; bool in; };
__device__ __forceinline__ NavTilePixel navlive_tile_pixel(int W, int H) {
    const int ntx = (W + NL_TW - 1) / NL_TW;
    const int t = threadIdx.x;
    NavTilePixel q;
    q.u = (int)(blockIdx.x % ntx) * NL_TW + (t & (NL_TW - 1)); q.v = (int)(blockIdx.x / ntx) * NL_TH + (t >> 4);
    q.in = q.u < W && q.v < H;
    q.p = (size_t)q.v * W + q.u;
    return q;
}
// steps 1 and 2 for this thread's pixel: valid, stamping under the mask mode, and -- returned: iff stamping -- its map-frame point S
template <int DF>
__device__ __forceinline__ bool navlive_tile_point(const NavLiveCam& cam, const void* __restrict__ depth, double scale, const uint8_t* __restrict__ mask,
                                                   int mask_mode, bool& valid, bool& stamping, float& Sx, float& Sy, float& Sz) {
    valid = false; stamping = false;
    const NavTilePixel q = navlive_tile_pixel(cam.W, cam.H);
    if (q.in) {
        float d;
        valid = navlive_pixel_depth<DF>(cam, depth, q.p, scale, d);
        stamping = valid && (mask_mode == 0 || (mask[q.p] != 0) == (mask_mode == 1));
        if (stamping) navlive_pixel_point(cam, q.u, q.v, d, Sx, Sy, Sz);
    }
    return stamping;
}
// the tile through LDS (NL_TILE_LDS words a plane, column x at x * (NL_TH + 1): the transposing write spreads over the banks): thread t
// puts its pixel and, after the barrier, gets pixel (x = t / 16, y = t % 16): a lane's predecessor is the pixel above it
__device__ __forceinline__ int navlive_tile_put() { const int t = threadIdx.x; return (t & (NL_TW - 1)) * (NL_TH + 1) + (t >> 4); }
__device__ __forceinline__ int navlive_tile_get() { const int t = threadIdx.x; return (t >> 4) * (NL_TH + 1) + (t & (NL_TH - 1)); }

// ---- runs of consecutive lanes with one cell: a run's head speaks for it ----------------------------------------------------------
// true in the first lane of a run (lane 0 is one); heads: their ballot
__device__ __forceinline__ bool nav_run_head(int c, unsigned long long& heads) {
    const int prev = __shfl_up(c, 1, 64);
    const bool head = lane() == 0 || c != prev;
    heads = __ballot(head);
    return head;
}
// the lanes of this lane's run from this one on: up to the next head
__device__ __forceinline__ int nav_run_len(unsigned long long heads) {
    const int ln = lane();
    const unsigned long long next = ln == 63 ? 0ull : heads >> (ln + 1);
    return next ? __builtin_ctzll(next) + 1 : 64 - ln;
}

// ---- one ray per wave, the rays made from the depth image in place (step 4) --------------------------------------------------------
// the ray of lattice pixel `ray` and its last sample M (<= 65535: the refusal of the corners).  All wave-uniform.
enum NavPixelRay { NAV_RAY_NO_DEPTH, NAV_RAY_IDLE, NAV_RAY_CARVES };       // no valid depth | a ray that does not carve | r and M are set
template <int DF>
__device__ __forceinline__ NavPixelRay navlive_pixel_ray(const NavLiveCam& cam, float step, const void* __restrict__ depth, double scale, float margin,
                                                         int ray, NavMarchRay& r, int& M) {
    const int i = ray % cam.nu, j = ray / cam.nu;
    const int u = i * cam.stride + cam.stride / 2, v = j * cam.stride + cam.stride / 2;      // u < W, v < H: nu = W / stride
    float d;
    if (!navlive_pixel_depth<DF>(cam, depth, (size_t)v * cam.W + u, scale, d)) return NAV_RAY_NO_DEPTH;
    float x, y;
    const float l = navlive_pixel_dir(cam, u, v, x, y);
    const float dx = x / l, dy = y / l, dz = 1.0f / l;
    const float o = 0.0f;                                             // the camera-frame origin, through ssf_raycast.h step 1 as written
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float a = cam.R[3 * k], b = cam.R[3 * k + 1], c = cam.R[3 * k + 2];
        r.O[k] = ((a * o + b * o) + c * o) + cam.t[k];
        r.D[k] = (a * dx + b * dy) + c * dz;
    }
    const bool rvalid = finite3(r.O[0], r.O[1], r.O[2]) && finite3(r.D[0], r.D[1], r.D[2]) && !(r.D[0] == 0.0f && r.D[1] == 0.0f && r.D[2] == 0.0f);
    const float t_end = (d * l) - margin;
    M = rvalid && t_end >= 0.0f ? (int)floorf(t_end / step) : -1;
    return M < 0 ? NAV_RAY_IDLE : NAV_RAY_CARVES;
}
// the wave's loop over its NL_RUN consecutive lattice pixels (four waves a workgroup): march(r, M) for every carving ray, one after
// the other, so that what the march keeps pending lives across them.  The counts are the same in every lane.
struct NavRayCounts { unsigned long long rays, carving, samples; };
template <int DF, class March>
__device__ __forceinline__ NavRayCounts navlive_wave_rays(float step, const NavLiveCam& cam, const void* __restrict__ depth, double scale, float margin,
                                                          March march) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int n = cam.nu * cam.nv;
    const long long first = (long long)wave * NL_RUN;
    const int r0 = (int)min(first, (long long)n), r1 = (int)min(first + NL_RUN, (long long)n);
    NavRayCounts k{0, 0, 0};
    for (int ray = r0; ray < r1; ray++) {
        NavMarchRay r; int M;
        const NavPixelRay what = navlive_pixel_ray<DF>(cam, step, depth, scale, margin, ray, r, M);
        if (what == NAV_RAY_NO_DEPTH) continue;
        k.rays++;
        if (what == NAV_RAY_IDLE) continue;
        k.carving++; k.samples += (unsigned long long)(M + 1);
        march(r, M);
    }
    return k;
}

}  // namespace ssf

#pragma GCC visibility push(hidden)       // (shared by the library's own files, no part of what it exports)
// the launches: the tiles of a W x H image, the workgroups of four waves for a lattice's rays, and the kernel by the handle's depth
// format (f gets DF as a std::integral_constant, the kernels' template argument)
inline unsigned navlive_tiles(int W, int H) { return (unsigned)(((W + ssf::NL_TW - 1) / ssf::NL_TW) * ((H + ssf::NL_TH - 1) / ssf::NL_TH)); }
inline unsigned navlive_march_groups(const ssf::NavLiveCam& cam) { return ((unsigned)((cam.nu * cam.nv + ssf::NL_RUN - 1) / ssf::NL_RUN) + 3) / 4; }
template <class F> inline void navlive_by_depth_format(int df, F&& f) {
    if (df == SSF_DEPTH_U16_SCALED) f(std::integral_constant<int, SSF_DEPTH_U16_SCALED>());
    else f(std::integral_constant<int, SSF_DEPTH_F32_METRES>());
}
// the pinhole and image size of a call (cam_width == 0: the handle's), and its depth range (both 0: the handle's): nullptr, or what
// is refused
inline const char* navlive_pinhole(const ssf_handle* h, float fx, float fy, float cx, float cy, int cam_width, int cam_height, ssf::NavLiveCam& cam) {
    cam.fx = fx; cam.fy = fy; cam.cx = cx; cam.cy = cy; cam.W = cam_width; cam.H = cam_height;
    if (cam.W == 0) { cam.fx = h->cfg.fx; cam.fy = h->cfg.fy; cam.cx = h->cfg.cx; cam.cy = h->cfg.cy; cam.W = h->cfg.width; cam.H = h->cfg.height; }
    if (cam.W < 1 || cam.W > 8192 || cam.H < 1 || cam.H > 8192) return "cam_width and cam_height must be 1..8192";
    if (!std::isfinite(cam.fx) || !std::isfinite(cam.fy) || !(cam.fx > 0.0f) || !(cam.fy > 0.0f) || !std::isfinite(cam.cx) || !std::isfinite(cam.cy))
        return "fx and fy must be finite and > 0, cx and cy finite";
    return nullptr;
}
inline const char* navlive_range(const ssf_handle* h, float t_min, float t_max, ssf::NavLiveCam& cam) {
    cam.tmin = t_min; cam.tmax = t_max;
    if (cam.tmin == 0.0f && cam.tmax == 0.0f) { cam.tmin = h->cfg.range_min; cam.tmax = h->cfg.range_max; }
    if (!std::isfinite(cam.tmin) || !std::isfinite(cam.tmax) || !(cam.tmin > 0.0f) || !(cam.tmax > cam.tmin))
        return "the range needs 0 < t_min < t_max, both finite";
    return nullptr;
}
// what ssf_navlive_default_params and ssf_navmem_default_params share: all zero, the grid's defaults and the frame layer's
template <class P> inline int navlive_default_fields(const ssf_handle* h, P* p) {
    ssf_navgrid_params g;
    { int rc = ssf_navgrid_default_params(h, &g); if (rc) return rc; }
    std::memset(p, 0, sizeof(*p));
    p->width = g.width; p->height = g.height; p->res = g.res; p->floor_max = g.floor_max; p->z_max = g.z_max;
    p->max_dist_cells = g.max_dist_cells; p->unknown_is_obstacle = g.unknown_is_obstacle;
    p->min_hits = 4; p->stride = 4; p->hit_margin_cells = 1.0f; p->open_unknown = 1;
    return SSF_OK;
}
// The refusals that ssf_navlive_overlay and ssf_navmem_update share (P: either params struct), in two parts with each call's own
// checks in between; nullptr, or what is refused.  The grid: its size and res into g, max_dist_cells, min_hits.
template <class P> inline const char* navlive_refuse_grid(const ssf_handle* h, const P* p, ssf_navgrid_params& g) {
    (void)ssf_navgrid_default_params(h, &g);
    g.width = p->width; g.height = p->height; g.res = p->res;
    if (const char* what = navgrid_size_res(&g)) return what;
    if (p->max_dist_cells < 1 || p->max_dist_cells > 1024) return "max_dist_cells must be 1..1024";
    if (p->min_hits < 1) return "min_hits must be >= 1";
    return nullptr;
}
// The camera (into cam), its lattice, the range, the mask mode, the depth pointer and the image's corners.  own: what the caller's
// own check between the margin and the range refuses (the overlay's min_seen), or nullptr.  bpp: bytes a depth pixel
template <class P>
inline const char* navlive_refuse_camera(const ssf_handle* h, const P* p, const void* depth, const uint8_t* mask, const char* own, ssf::NavLiveCam& cam,
                                         size_t& bpp) {
    if (const char* what = navlive_pinhole(h, p->fx, p->fy, p->cx, p->cy, p->cam_width, p->cam_height, cam)) return what;
    if (p->stride < 1 || p->stride > 64) return "stride must be 1..64";
    cam.stride = p->stride; cam.nu = cam.W / p->stride; cam.nv = cam.H / p->stride;
    if (cam.nu < 1 || cam.nv < 1) return "the stride leaves no pixel lattice";
    if (!(p->hit_margin_cells >= 0.0f) || !std::isfinite(p->hit_margin_cells)) return "hit_margin_cells must be finite and >= 0";
    if (own) return own;
    if (const char* what = navlive_range(h, p->t_min, p->t_max, cam)) return what;
    if (p->mask_mode < 0 || p->mask_mode > 2) return "mask_mode must be 0..2";
    if (p->mask_mode != 0 && !mask) return "mask is NULL with mask_mode != 0";
    bpp = h->in_depth == SSF_DEPTH_U16_SCALED ? 2 : 4;
    if (p->frame_on_device && (uintptr_t)depth % bpp) return "the device depth pointer is not aligned for the input format";
    // the sample index is bounded: l is largest at a corner of the image
    for (int k = 0; k < 4; k++) {
        float x, y;
        const float l = navlive_pixel_dir(cam, (k & 1) ? cam.W - 1 : 0, (k & 2) ? cam.H - 1 : 0, x, y);
        if (!((cam.tmax * l) / (p->res * 0.5f) <= 65535.0f)) return "(t_max * l) / (res / 2) must be <= 65535 at the image's corners";
    }
    return nullptr;
}
// [a, a + na) and [b, b + nb) share a byte (a NULL array shares nothing)
inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}
// The arrays of a call, a[k] of n[k] bytes: outputs below first_in, then inputs, the frame's (depth, mask) from first_frame on (frame_apart:
// they lie in the other memory, host against device, which is no overlap).  True iff an output overlaps another array, other than a
// pair may[k] = {output, input} being ONE array (the update in place)
inline bool navlive_arrays_overlap(const void* const* a, const size_t* n, int n_all, int first_in, int first_frame, bool frame_apart,
                                   const int (*may)[2], int n_may) {
    for (int i = 0; i < first_in; i++)
        for (int j = i + 1; j < n_all; j++) {
            if (j >= first_frame && frame_apart) continue;
            bool in_place = false;
            for (int k = 0; k < n_may; k++) in_place = in_place || (may[k][0] == i && may[k][1] == j && a[i] == a[j]);
            if (!in_place && ranges_overlap(a[i], n[i], a[j], n[j])) return true;
        }
    return false;
}
// the two frames of a call as the kernels read them, from its params (P: any of the three): the grid's (NULL: ssf_navgrid_default_pose
// now) into G and `gpose`, the camera's (NULL: the handle's pose) into cam; and the kernels' view of the grid.  step: of the march
// (the blobs: none)
template <class P>
inline int navlive_frames(ssf_handle* h, const ssf_navgrid_params* g, const P* p, float step, ssf::NavGrid& G, ssf::NavLiveCam& cam, float* gpose) {
    float cpose[12];
    if (p->grid_pose) std::memcpy(gpose, p->grid_pose, 12 * sizeof(float));
    else { int rc = ssf_navgrid_default_pose(h, g, gpose); if (rc) return rc; }
    if (p->cam_pose) std::memcpy(cpose, p->cam_pose, sizeof(cpose)); else ssf::pose_to12(h->pose, cpose);
    std::memcpy(cam.R, cpose, 9 * sizeof(float)); cam.t[0] = cpose[9]; cam.t[1] = cpose[10]; cam.t[2] = cpose[11];
    std::memcpy(G.R, gpose, 9 * sizeof(float)); G.t[0] = gpose[9]; G.t[1] = gpose[10]; G.t[2] = gpose[11];
    G.W = p->width; G.H = p->height; G.res = p->res; G.step = step; G.fW = (float)G.W; G.fH = (float)G.H;
    G.zmax = p->z_max; G.floor_max = p->floor_max;
    return SSF_OK;
}
// the sums of a call read back: N of them on the device, sum k at word k * PAD (a 128-byte line each: every workgroup adds to them).
// fetch queues the copy; s[k] is good after the stream's synchronise
template <int N, int PAD> struct NavPaddedSums {
    unsigned long long padded[N * PAD];
    hipError_t fetch(const unsigned long long* d, hipStream_t st) { return hipMemcpyAsync(padded, d, sizeof(padded), hipMemcpyDeviceToHost, st); }
    unsigned long long operator[](int k) const { return padded[k * PAD]; }
};
#pragma GCC visibility pop
