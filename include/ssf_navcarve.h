/*
 * ssf_navcarve.h -- the navigation grid of ssf_navgrid.h with free space carved along camera rays, on the device.
 *
 * ssf_navgrid_build's "free" means "floor was observed in the cell".  A cell the camera looked straight through whose floor was
 * never fused -- floor behind the sensor's minimum range, dark or specular floor, every cell under the camera's own path --
 * stays unknown there, and a planner run with unknown_is_obstacle refuses to cross space that the map itself shows to be empty.
 * This call adds the missing evidence: from a list of camera poses the caller supplies (its trajectory, or the poses of stored
 * keyframes) a lattice of pixel rays is cast through the map (ssf_raycast.h), and every cell whose obstacle band a ray crosses
 * before its hit is counted as seen through.  The call is stateless like every other read-out: the result is a function of the
 * map as it stands and of the views; the frame path is not touched and no bit of a later pose or model changes.
 *
 * Every step below is one IEEE f32 operation in the order written, every parameter is cast to f32 first, and every result is
 * an integer count, minimum or maximum, so the order of the rays never matters and a numpy f32 restatement reproduces every
 * output bit for bit (tests/navcarve_ref.py).
 *   1. The uncarved grid.  zmin, zmax, hits and the internal uncarved state are exactly those of ssf_navgrid_build(h, g, ...):
 *      steps 1 to 7 of ssf_navgrid.h, with the same frame, the default pose included.
 *   2. Rays.  The pixel lattice is nu = cam_width / stride, nv = cam_height / stride (integer division, both >= 1).  Pixel
 *      (i, j) is u = i * stride + stride / 2, v = j * stride + stride / 2 (integers).  x = ((float)u - cx) / fx,
 *      y = ((float)v - cy) / fy, l = sqrtf((x * x + y * y) + 1.0f), d = (x / l, y / l, 1.0f / l).  Ray
 *      r = (view * nv + j) * nu + i has the camera-frame origin 0 and direction d; the view's pose (12 floats, camera-to-map, the
 *      layout of ssf_get_pose) takes it to the map frame exactly as ssf_raycast.h step 1 writes it.  A non-finite pose therefore
 *      makes invalid rays, which are counted (rays_invalid) and carve nothing.
 *   3. Hit.  Each map-frame ray (O, D) gets the result of ssf_raycast with the identity pose on it, with t_min, t_max,
 *      min_conf = ray_min_conf, splat_scale = ray_splat_scale, visible_only 0 and the default index parameters.  The resident
 *      index is built or reused by the ray cast's own rule.
 *   4. Extent.  step = res * 0.5f, margin = hit_margin_cells * res.  A hit at tt: t_end = tt - margin.  A valid ray that hits
 *      nothing, with carve_misses: t_end = t_max.  Anything else carves nothing.  M = t_end >= 0 ? (int)floorf(t_end / step) : -1;
 *      a ray with M >= 0 is "carving"; ray_samples is the sum of M + 1 over the carving rays.
 *   5. Samples.  For m = 0 .. M: tm = (float)m * step, S_k = O_k + tm * D_k (map frame); then the grid frame of ssf_navgrid.h
 *      step 1 (d = S - t, C = R^T d in its written form) and the cell test of its step 4.  A sample is ACCEPTED iff it is in the
 *      grid and z > floor_max && z <= z_max with z = C.z: the band that the robot's body occupies, the obstacle band of step 5.
 *   6. Entries.  Sample m is an ENTRY iff it is accepted and (m == 0, or sample m - 1 is not accepted, or sample m - 1 is in
 *      another cell).  seen[cell] is the number of entries: rays that pass through the cell's band, not samples, so a vertical ray
 *      counts once.  ray_entries is the sum of seen.
 *   7. Carved state, int8 in nav_msgs/OccupancyGrid's convention: 100 if obst_hits >= min_hits, else 0 if floor_hits >= min_hits
 *      or seen >= min_seen, else -1.  cells_seen = the cells with seen >= min_seen; cells_carved = the cells whose uncarved state
 *      was -1 and whose carved state is 0.  dist2 is step 8 of ssf_navgrid.h on the carved state.
 *   8. Identity.  With n_views == 0 every `grid` output and every `grid` stat equals ssf_navgrid_build's bit for bit, seen is 0
 *      and the ray stats are 0.
 *
 * What this means and what it does not:
 *   * the hit is what the CURRENT map shows from that pose, not what the sensor measured then: a view is a question to the map;
 *   * an obstacle cell is never carved: occupied wins over seen-through, whatever the rays say;
 *   * a miss carves nothing by default (carve_misses 0), because a hole in the map is not evidence of free space;
 *   * seen-through without observed floor is reported as free.  A caller that wants both conditions takes `seen` and `hits` and
 *     combines them itself.
 *
 * Defaults (ssf_navcarve_default_params) are design choices, not tuned values: views NULL, n_views 0, the camera from the
 * handle's cfg (cam_width 0), stride 8, t_min = t_max = 0 (cfg.range_min / cfg.range_max), ray_min_conf 0, ray_splat_scale 0
 * (the ray cast's 3), hit_margin_cells 1, carve_misses 0, min_seen 1.
 *
 * Refused with SSF_ERR_INVALID_ARG: everything ssf_navgrid_build and ssf_raycast refuse for their parts; h, g, c or out NULL;
 * every output NULL (seen alone is a valid request); n_views outside 0..4096, or views NULL with n_views > 0; stride outside
 * 1..64, or nu or nv < 1; fx or fy not finite or <= 0, cx or cy not finite; cam_width or cam_height outside 1..8192 (after the
 * cfg default); hit_margin_cells negative or not finite; min_seen < 1; t_max / step > 65535 (computed in f32), so that M is
 * bounded; n_views * nu * nv > 2^31 - 1, so that seen cannot wrap.  With SSF_ERR_STATE: frames pending in the extract pipeline;
 * a sharded handle (cfg.nranks > 1).  After any refusal the handle keeps working.
 *
 * views is HOST memory always; g->on_device governs the outputs, seen included.  The call is synchronous and runs on the
 * handle's stream; the rays are worked off in chunks of at most 2^20 rays (24 MB of rays, 8 MB of hits).  Working buffers are allocated
 * on first use and grown as a whole; a growth that fails returns SSF_ERR_DEVICE and leaves the handle working.  Kernels appear in
 * ssf_get_kernel_times under profile = 1 (navcarve_rays, navcarve_march, next to the navgrid_* and raycast_* names).
 *
 * Who exports these functions: libssf_hip_navcarve.so, which is the product library's objects with the carve linked in (it exports
 * everything libssf_hip.so does, and these).  libssf_hip.so itself does not: its exported symbols are what they were.  A caller of
 * the carve links or loads libssf_hip_navcarve.so INSTEAD of libssf_hip.so, never both: a handle belongs to the library that
 * created it.  The ABI version of ssf.h is unchanged.
 */
#ifndef SSF_NAVCARVE_H
#define SSF_NAVCARVE_H

#include "ssf_navgrid.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ssf_navcarve_params {
    const float* views;               /* n_views x 12 floats, camera-to-map (ssf_get_pose layout); HOST memory always */
    int   n_views;                    /* 0..4096 */
    float fx, fy, cx, cy;             /* pinhole of the views; */
    int   cam_width, cam_height;      /* cam_width == 0: all six from the handle's cfg */
    int   stride;                     /* pixel lattice, 1..64 */
    float t_min, t_max;               /* metres along the ray; both 0 = cfg.range_min / cfg.range_max */
    float ray_min_conf;               /* ssf_raycast's min_conf for the hit */
    float ray_splat_scale;            /* ssf_raycast's splat_scale (0 = 3) */
    float hit_margin_cells;           /* a ray stops this many cells short of its hit, >= 0 */
    int   carve_misses;               /* 1: a valid ray that hits nothing carves up to t_max; 0: it carves nothing */
    int   min_seen;                   /* ray entries that make a cell seen, >= 1 */
} ssf_navcarve_params;

typedef struct ssf_navcarve_out {     /* any may be NULL, not all */
    ssf_navgrid_out grid;
    uint32_t* seen;                   /* height x width */
} ssf_navcarve_out;

typedef struct ssf_navcarve_stats {
    ssf_navgrid_stats grid;           /* rows_used, samples, samples_in_grid, list_entries, pose: of the uncarved grid;
                                         cells_free / cells_occupied / cells_unknown: of the CARVED state */
    int64_t rays, rays_hit, rays_invalid, rays_carving, ray_samples, ray_entries, cells_seen, cells_carved;
} ssf_navcarve_stats;

int ssf_navcarve_default_params(const ssf_handle* h, ssf_navcarve_params* c);
int ssf_navgrid_carve(ssf_handle* h, const ssf_navgrid_params* g, const ssf_navcarve_params* c, const ssf_navcarve_out* out,
                      ssf_navcarve_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* SSF_NAVCARVE_H */
