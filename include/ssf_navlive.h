/*
 * ssf_navlive.h -- the live obstacle layer: the depth frame of this instant stamped onto a navigation grid, on the device.
 *
 * Every other navigation call reads the FUSED MAP, and the map leaves out whatever moves: superpixels under a dynamic mask are
 * never fused (ssf_dynamic.h, ssf_motion.h), so a person standing in the corridor is in no grid and a plan runs straight through
 * them; so is anything put down since the robot last looked.  Only the depth frame knows about such obstacles.  This call takes a
 * grid state as it stands (ssf_navgrid_build's or ssf_navgrid_carve's, or its own earlier output) and the current depth frame,
 * marks the cells in which the frame's points lie in the robot's body band as occupied, opens unknown cells that the sensor looked
 * through, and recomputes the clearance: what ssf_navplan_field takes, without leaving the device.
 *
 * Every step below is one IEEE f32 operation in the order written (the library builds with -ffp-contract=off and correctly rounded
 * division and square root), every parameter is cast to f32 first, and every result is an integer count, so the order of pixels and
 * rays never matters and a numpy f32 restatement reproduces every output with == (tests/navlive_ref.py).
 *   1. Depth.  d[p] = the depth of pixel p in metres, read in the handle's input format exactly as ssf_motion.h states it: f32
 *      metres, or (float)((double)v * depth_scale) for uint16.  A pixel is VALID iff d is finite and t_min <= d <= t_max.
 *   2. Point.  Pixel (u, v): x = ((float)u - cx) / fx, y = ((float)v - cy) / fy, Pc = (x * d, y * d, d).  With the camera pose
 *      (Rc, tc), camera-to-map: M_i = ((Rc_i0 Pc.x + Rc_i1 Pc.y) + Rc_i2 Pc.z) + tc_i.  Then the grid frame of ssf_navgrid.h step 1
 *      with c = M (d = M - t, C = R^T d in its written form) and the cell test of its step 4 on C.x, C.y (a NaN fails).  The point is
 *      an OBSTACLE POINT of that cell iff it is in the grid and C.z > floor_max && C.z <= z_max: the obstacle band of ssf_navgrid.h
 *      step 5, the heights the robot's body occupies.
 *   3. Stamp.  A pixel STAMPS iff it is valid and passes mask_mode: 0 every pixel; 1 pixels with mask != 0; 2 pixels with mask == 0.
 *      live_hits[cell] = the number of stamping pixels whose point is an obstacle point of the cell.
 *   4. See-through.  The pixel lattice (nu, nv, u, v), x, y, l and the direction (x / l, y / l, 1.0f / l) are those of
 *      ssf_navcarve.h step 2 with `stride`; the map-frame ray (O, D) is that of ssf_raycast.h step 1 with o = 0 and the camera pose.
 *      A lattice pixel has a ray iff it is valid; the mask is not consulted (a masked pixel still measured the space in front of
 *      it).  A ray whose O or D has a component that is not finite, or whose D is zero in all three, carves nothing.  Its hit is
 *      tt = d * l (one multiplication); from there steps 4 (a hit at tt; there are no misses), 5 and 6 of ssf_navcarve.h apply word
 *      for word: step = res * 0.5f, margin = hit_margin_cells * res, t_end = tt - margin, M = t_end >= 0 ? (int)floorf(t_end / step)
 *      : -1, samples m = 0 .. M at tm = (float)m * step, accepted in the same band, and live_seen[cell] = the number of entries.
 *   5. State, int8 in nav_msgs/OccupancyGrid's convention: 100 if state_in == 100 || live_hits >= min_hits; else 0 if state_in == 0
 *      || (open_unknown && live_seen >= min_seen); else -1.  Any other value of state_in counts as unknown.  Occupied always wins
 *      over seen-through, as in the carve.
 *   6. Clearance.  dist2 is step 8 of ssf_navgrid.h on that state, with max_dist_cells and unknown_is_obstacle.
 *   7. Stats, all exact: pixels_valid, pixels_stamping; points_in_band = the sum of live_hits; rays = lattice pixels with a ray;
 *      rays_carving = rays with M >= 0; ray_samples = the sum of M + 1 over them; ray_entries = the sum of live_seen;
 *      cells_stamped = cells with state_in != 100 and state 100; cells_opened = cells with state_in neither 100 nor 0 and state 0;
 *      cells_free / cells_occupied / cells_unknown of the output state.  Informative only: atomics, the atomic additions the stamp
 *      and the march issued on the two count arrays (it depends on how points and entries were merged).  pose = the grid frame used.
 *   8. Identity.  With no valid pixel, state is state_in with foreign values mapped to -1, dist2 equals what ssf_navgrid_build gives
 *      for that state bit for bit, and both count arrays are 0.
 *
 * Any output may be NULL, but not all.  The march of step 4 is skipped when nothing asks for it (live_seen NULL and open_unknown 0);
 * the ray stats are 0 then.  `state` may be the very pointer state_in (the update in place); any other overlap among state_in and the
 * outputs is refused.
 *
 * What this is and what it is not:
 *   * it is stateless: there is no decay and no memory of earlier frames.  A caller that wants an obstacle to persist after it left
 *     the view feeds the output state back as the next state_in; a caller that wants it gone feeds the map's grid again;
 *   * a pixel stamps a POINT, not a footprint.  Pixels are d / fx apart on a fronto-parallel surface, so a surface is dense in the
 *     grid as long as d / fx < res, which holds over the whole sensor range at the defaults (5 m / 525 < 0.05 m);
 *   * occupied cells are never cleared by live evidence: a ray crosses the band at one height only, and an obstacle may be lower.
 *
 * Defaults (ssf_navlive_default_params) are design choices, not tuned values: min_hits 4 (a speck filter: a few flying pixels at a
 * depth edge do not block a corridor), stride 4, hit_margin_cells 1, min_seen 1, open_unknown 1, mask_mode 0; grid_pose and cam_pose
 * NULL, the camera from the handle's cfg (cam_width 0), t_min = t_max = 0 (cfg.range_min / cfg.range_max), on_device and
 * frame_on_device 0.  width, height, res, floor_max, z_max and max_dist_cells are those of ssf_navgrid_default_params.
 *
 * Refused with SSF_ERR_INVALID_ARG: h, p, depth, state_in or out NULL; every output NULL; what ssf_navgrid_build refuses for width,
 * height, res and max_dist_cells; min_hits < 1; floor_max or z_max a NaN; what ssf_navgrid_carve refuses for the camera, stride,
 * hit_margin_cells and min_seen; t_min or t_max not finite, t_min <= 0 or t_max <= t_min (after the cfg default); mask_mode outside
 * 0..2, or mask NULL with mask_mode != 0; a device depth pointer not aligned for the input format; an overlap other than
 * state == state_in; (t_max * l_c) / step > 65535 for any of the four corner pixels (0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)
 * of the camera, in f32 with l as step 4 computes it: rounding is monotone and l is largest at a corner, so M <= 65535 for every
 * ray.  With SSF_ERR_STATE: frames pending in the extract pipeline; a sharded handle (cfg.nranks > 1).  After any refusal the handle
 * keeps working.
 *
 * The call is synchronous and runs on the handle's stream.  It changes no state of the handle: an overlay between two frames changes
 * no later pose or model bit.  on_device governs state_in and the outputs, frame_on_device governs depth and mask; the two poses are
 * host memory always.  Working buffers (per cell 11 bytes and the staged host arrays) are allocated on first use and grown as a
 * whole; a growth that fails returns SSF_ERR_DEVICE and leaves the handle working.  Kernels appear in ssf_get_kernel_times under
 * profile = 1: navlive_stamp, navlive_march, navlive_cells, then navgrid_columns and navgrid_rows.
 *
 * Who exports these functions: libssf_hip_live.so, which is libssf_hip_drive.so's objects with this call linked in (it exports
 * everything the drive library does, and these).  The other five libraries do not: their exported symbols are what they were.  A
 * caller links or loads libssf_hip_live.so INSTEAD of them, never beside one: a handle belongs to the library that created it.  The
 * ABI version of ssf.h is unchanged.
 */
#ifndef SSF_NAVLIVE_H
#define SSF_NAVLIVE_H

#include "ssf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ssf_navlive_params {
    const float* grid_pose;           /* 12 floats grid-to-map: what ssf_navgrid_stats.pose returned for `state`;
                                         NULL = ssf_navgrid_default_pose(width, height, res) now */
    int   width, height;              /* 1..4096 each */
    float res;                        /* metres per cell */
    float floor_max, z_max;           /* the obstacle band of ssf_navgrid.h step 5: floor_max < z <= z_max */
    int   max_dist_cells;             /* 1..1024 */
    int   unknown_is_obstacle;        /* 1: cells of state -1 count as obstacles in dist2 */
    const float* cam_pose;            /* 12 floats camera-to-map (ssf_get_pose layout); NULL = the handle's pose */
    float fx, fy, cx, cy;             /* pinhole of the depth frame; */
    int   cam_width, cam_height;      /* cam_width == 0: all six from the handle's cfg */
    float t_min, t_max;               /* valid depths, metres; both 0 = cfg.range_min / cfg.range_max */
    int   mask_mode;                  /* 0 no mask; 1 only pixels with mask != 0 stamp; 2 only pixels with mask == 0 stamp */
    int   min_hits;                   /* points that make a cell occupied, >= 1 */
    int   stride;                     /* pixel lattice of the see-through rays, 1..64 */
    float hit_margin_cells;           /* a ray stops this many cells short of its depth, >= 0 */
    int   min_seen;                   /* ray entries that make a cell seen, >= 1 */
    int   open_unknown;               /* 1: an unknown cell seen through becomes free */
    int   on_device;                  /* 1: state_in and every output are device pointers */
    int   frame_on_device;            /* 1: depth and mask are device pointers */
} ssf_navlive_params;

typedef struct ssf_navlive_out {      /* any may be NULL, not all; each height x width */
    uint32_t* live_hits;
    uint32_t* live_seen;
    int8_t*   state;                  /* may be state_in itself */
    int32_t*  dist2;
} ssf_navlive_out;

typedef struct ssf_navlive_stats {
    int64_t pixels_valid, pixels_stamping, points_in_band;
    int64_t rays, rays_carving, ray_samples, ray_entries;
    int64_t cells_stamped, cells_opened;
    int64_t cells_free, cells_occupied, cells_unknown;
    int64_t atomics;                  /* informative */
    float   pose[12];                 /* the grid frame used */
} ssf_navlive_stats;

int ssf_navlive_default_params(const ssf_handle* h, ssf_navlive_params* p);
int ssf_navlive_overlay(ssf_handle* h, const ssf_navlive_params* p, const void* depth, const uint8_t* mask, const int8_t* state_in,
                        const ssf_navlive_out* out, ssf_navlive_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* SSF_NAVLIVE_H */
