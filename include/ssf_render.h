/*
 * ssf_render.h -- the fused model drawn into a virtual pinhole camera on the device.
 *
 * A node that wants to SEE the map (rviz markers, "what the model predicts this camera sees", a top view) would otherwise copy
 * the whole model out (ssf_get_model: 104 B per row) and draw it on the host.  ssf_render_model draws it where it lives and
 * hands back images of the chosen camera.
 *
 * What is drawn: the model as it stands after the last completed frame (or ssf_set_model / ssf_apply_deformation).  Every
 * supersurfel is a flat, two-sided elliptical disc: centre c = position, in-plane axes e1 = orientation row 0, e2 = row 1,
 * normal n = row 2, half-axes s*sqrt(dims.x) along e1 and s*sqrt(dims.y) along e2 (s = splat_scale, default 3: the reference
 * node's marker size -- it draws a quad with these half-axes, this is the ellipse inscribed in it).  The nearest disc along a
 * pixel's ray wins; no blending.
 *
 * Every step below is one IEEE f32 operation, in the order written (the library builds with -ffp-contract=off and correctly
 * rounded division), so a numpy f32 restatement reproduces the images bit for bit.  Every parameter is cast to f32 first.
 *   1. Pose (R, t): camera-to-map, 12 floats as ssf_get_pose (R row-major, then t).  Per row d = c - t and C = R^T d with
 *      C_j = (R0j d.x + R1j d.y) + R2j d.z; E1, E2, N = R^T e1, R^T e2, R^T n in the same form without the subtraction.
 *   2. Ray of pixel (u, v): qx = ((float)u - cx) / fx, qy = ((float)v - cy) / fy, q = (qx, qy, 1) (pixel centres on integers).
 *   3. Depth: den = (N.x qx + N.y qy) + N.z, num = (N.x C.x + N.y C.y) + N.z C.z, z = num / den.  A candidate needs den != 0,
 *      z finite and z_min <= z <= z_max.
 *   4. Inside: P = (z qx, z qy, z), D = P - C, a = (D.x E1.x + D.y E1.y) + D.z E1.z, b likewise with E2, k = s s; inside iff
 *      (a a) dims.y + (b b) dims.x <= (k dims.x) dims.y.
 *   5. Rows: conf > min_conf (strict, as exportModel's conf_thresh), dims.x > 0 and dims.y > 0, both finite; all live rows
 *      (visible and out-of-view) or, with visible_only, the visible rows only.
 *   6. Winner: the minimum of (bits(z) << 32) | logical_index over the pixel's candidates; logical_index = the row's position
 *      in ssf_get_model's order [visible | out-of-view], so equal depths go to the smaller index.
 *   7. Outputs (each optional, NULL = not produced; an empty pixel gets depth 0, index -1, colour 0, normal 0):
 *        depth  H x W f32: z          index  H x W i32: the winner's logical index
 *        color  H x W x 3 f32: the winner's colour as stored (0..255)
 *        rgb8   H x W x 3 u8: (uint8_t)fminf(255, fmaxf(0, rintf(col))) (ties to even)
 *        normal H x W x 3 f32: N in the camera frame, facing the camera: den > 0 ? -N : N
 *   8. Stats (exact): fragments = (row, pixel) pairs passing 3-5; pixels_filled; rows_shown = distinct rows owning a pixel;
 *      list_entries = (tile, row) pairs the rasteriser visited (informative: depends on its conservative boxes).
 *
 * Defaults: pose NULL = the handle's pose; width 0 = the handle's camera (width, height, fx, fy, cx, cy); z_min = z_max = 0 =
 * cfg.range_min / cfg.range_max; splat_scale 0 = 3; min_conf 0.  ssf_render_default_params fills exactly these.
 * Refused with SSF_ERR_INVALID_ARG: a NULL handle or params, every output NULL, a camera size outside 1..4096, fx or fy zero or
 * not finite, z_min <= 0 or z_max <= z_min (after the defaults), splat_scale < 0 or not finite.  With SSF_ERR_STATE: frames
 * pending in the extract pipeline, a sharded handle (cfg.nranks > 1).
 *
 * The call is synchronous and runs on the handle's stream.  It changes no state of the handle: a render between two frames
 * changes no later result.  Its working buffers are allocated on first use and grown as a whole; a growth that fails returns
 * SSF_ERR_DEVICE and leaves the handle working (frames, smaller renders).  With on_device the outputs are device pointers (e.g.
 * tensors feeding a visualiser), otherwise host memory.  Kernels appear in ssf_get_kernel_times under profile = 1
 * (render_prep, render_fill, render_tile).
 *
 * Only the HIP product library (libssf_hip.so) exports these functions; the ABI version of ssf.h is unchanged.
 */
#ifndef SSF_RENDER_H
#define SSF_RENDER_H

#include "ssf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ssf_render_params {
    const float* pose;        /* 12 floats camera-to-map (ssf_get_pose layout); NULL = the handle's current pose */
    int width, height;        /* image size; width 0 = the handle's camera (and its intrinsics) */
    float fx, fy, cx, cy;     /* pinhole intrinsics (pixel centres on integers) */
    float z_min, z_max;       /* accepted depth range; both 0 = cfg.range_min / cfg.range_max */
    float min_conf;           /* rows with conf > min_conf are drawn */
    float splat_scale;        /* s: half-axes s * sqrt(dims); 0 = 3 */
    int visible_only;         /* 1: the visible rows only; 0: every live row */
    int on_device;            /* 1: the outputs are device pointers */
} ssf_render_params;

typedef struct ssf_render_stats {
    int64_t fragments;        /* (row, pixel) pairs that pass the depth range and inside test */
    int64_t pixels_filled;
    int64_t rows_shown;       /* distinct rows that own at least one pixel */
    int64_t list_entries;     /* (tile, row) pairs visited by the rasteriser (informative) */
} ssf_render_stats;

int ssf_render_default_params(const ssf_handle* h, ssf_render_params* p);
int ssf_render_model(ssf_handle* h, const ssf_render_params* p, float* depth, int32_t* index, uint8_t* rgb8, float* color,
                     float* normal, ssf_render_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* SSF_RENDER_H */
