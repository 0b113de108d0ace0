// ssf_navlive.hpp -- what ssf_navlive.hip (ssf_navlive_overlay) shares with ssf_navdyn.hip (ssf_navdyn_blobs, include/ssf_navdyn.h):
// the camera of a depth frame, the depth of a pixel, the map-frame point of a pixel (include/ssf_navlive.h steps 1 and 2; its grid
// point and cell: nav_grid_point and nav_cell, ssf_navgrid.hpp), and the refusals for the camera and the depth range.
// Private to the library's own files: nothing here is exported.
#pragma once
#include "ssf_navgrid.hpp"
#include "../../include/ssf_input.h"

namespace ssf {

// the camera of the frame: pose (R row-major, t: camera-to-map), pinhole, image size, valid depths; the lattice of the rays
struct NavLiveCam { float R[9], t[3]; float fx, fy, cx, cy; int W, H; float tmin, tmax; int stride, nu, nv; };

template <int DF> __device__ __forceinline__ float navlive_load_depth(const void* __restrict__ p, size_t q, double scale) {
    if (DF == SSF_DEPTH_U16_SCALED) return (float)((double)reinterpret_cast<const uint16_t*>(p)[q] * scale);
    return reinterpret_cast<const float*>(p)[q];
}
// the map-frame point of pixel (u, v) at depth d (ssf_navlive.h step 2)
__device__ __forceinline__ void navlive_pixel_point(const NavLiveCam& cam, int u, int v, float d, float& Sx, float& Sy, float& Sz) {
    const float x = ((float)u - cam.cx) / cam.fx, y = ((float)v - cam.cy) / cam.fy;
    const float px = x * d, py = y * d;
    const float* R = cam.R;
    Sx = ((R[0] * px + R[1] * py) + R[2] * d) + cam.t[0];
    Sy = ((R[3] * px + R[4] * py) + R[5] * d) + cam.t[1];
    Sz = ((R[6] * px + R[7] * py) + R[8] * d) + cam.t[2];
}

}  // namespace ssf

#pragma GCC visibility push(hidden)       // (shared by the library's own files, no part of what it exports)
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
// the two frames of a call as the kernels read them: the grid's (NULL: ssf_navgrid_default_pose now) into G and `gpose`, the camera's
// (NULL: the handle's pose) into cam
inline int navlive_frames(ssf_handle* h, const ssf_navgrid_params* g, const float* grid_pose, const float* cam_pose, ssf::NavGrid& G, ssf::NavLiveCam& cam,
                          float* gpose) {
    float cpose[12];
    if (grid_pose) std::memcpy(gpose, grid_pose, 12 * sizeof(float));
    else { int rc = ssf_navgrid_default_pose(h, g, gpose); if (rc) return rc; }
    if (cam_pose) std::memcpy(cpose, cam_pose, sizeof(cpose)); else ssf::pose_to12(h->pose, cpose);
    std::memcpy(cam.R, cpose, 9 * sizeof(float)); cam.t[0] = cpose[9]; cam.t[1] = cpose[10]; cam.t[2] = cpose[11];
    std::memcpy(G.R, gpose, 9 * sizeof(float)); G.t[0] = gpose[9]; G.t[1] = gpose[10]; G.t[2] = gpose[11];
    return SSF_OK;
}
#pragma GCC visibility pop
