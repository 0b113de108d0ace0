/*
 * ssf_navgrid.h -- a floor-plane navigation grid of the fused model, built on the device: height, occupancy, clearance.
 *
 * A robot that drives through the map needs to know where the floor is, where obstacles are and how far the nearest one is.
 * Without this call it copies the whole model out (ssf_get_model: 104 B per row), rasterises discs and runs a distance
 * transform on the host.  A top view of ssf_render_model does not replace it: the render keeps the NEAREST disc per pixel of a
 * pinhole camera, the grid is an orthographic aggregate over ALL discs above a cell, split by height band.  "Free" means floor
 * was observed in the cell, not that space was seen through: this call carves nothing along the camera's rays (ssf_navgrid_carve,
 * ssf_navcarve.h, builds the same grid and does).
 *
 * What is aggregated: the model as it stands after the last completed frame (or ssf_set_model / ssf_apply_deformation).  Every
 * step below is one IEEE f32 operation, in the order written (the library builds with -ffp-contract=off and correctly rounded
 * division and square root), and every result is an integer minimum, maximum or sum, so a numpy f32 restatement reproduces every
 * output bit for bit whatever the order of the rows (tests/navgrid_ref.py).  Every parameter is cast to f32 first.
 *   1. Grid frame.  Pose (R, t): grid-to-map, 12 floats as ssf_get_pose (R row-major, then t).  x and y span the floor, z points
 *      up.  Cell (ix, iy) covers [ix res, (ix + 1) res) x [iy res, (iy + 1) res) of the frame; the outputs are row-major, iy the
 *      row.  Per row d = c - t and C = R^T d with C_j = (R0j d.x + R1j d.y) + R2j d.z; E1, E2, N = R^T e1, R^T e2, R^T n in the
 *      same form without the subtraction (c = position, e1 / e2 / n = orientation rows 0 / 1 / 2: ssf_render.h step 1).
 *   2. Rows.  A row is used iff it is live (with visible_only: a visible row), its position is finite in all three components,
 *      conf > min_conf (strict), t_init_min <= stamps.x <= t_init_max, t_last_min <= stamps.y <= t_last_max (ssf_query.h step 1),
 *      dims.x > 0 and dims.y > 0 and both are finite (ssf_render.h step 5).
 *   3. Footprint: a lattice of samples on the row's disc.  h1 = s * sqrtf(dims.x), h2 = s * sqrtf(dims.y) (s = splat_scale,
 *      default 2, a design choice: a uniform disc of radius r has standard deviation r / 2 along an axis, and dims are
 *      variances).  step = res * 0.5f.  q1 = ceilf(h1 / step); n1 = q1 >= (float)max_steps ? max_steps : (q1 >= 1.0f ? (int)q1
 *      : 1); n2 likewise from h2.  Sample (i, j), -n1 <= i <= n1 and -n2 <= j <= n2, exists iff
 *      i i n2 n2 + j j n1 n1 <= n1 n1 n2 n2 (integers).  a = ((float)i / (float)n1) * h1, b = ((float)j / (float)n2) * h2,
 *      S.k = (C.k + a * E1.k) + b * E2.k for k = x, y, z.
 *      With step = res / 2 a horizontal disc whose lattice is not clipped leaves no interior cell unhit.  A disc with
 *      h > max_steps * step along an axis is sampled more coarsely than that and MAY LEAVE HOLES between its samples: raise
 *      max_steps (up to 16) or res for maps with very large discs.
 *   4. Cell of a sample.  gx = S.x / res, gy = S.y / res.  The sample is in the grid iff gx >= 0 && gx < (float)width &&
 *      gy >= 0 && gy < (float)height (a NaN fails); then ix = (int)gx, iy = (int)gy.
 *   5. Bands, with z = S.z.  A sample in the grid is accepted iff z >= z_min && z <= z_max (this drops ceilings, overhangs the
 *      robot passes under, and noise below the floor).  An accepted sample is an OBSTACLE sample iff z > floor_max, a FLOOR
 *      sample iff z <= floor_max && fabsf(N.z) >= floor_cos; otherwise it only counts toward the heights.
 *   6. Per-cell accumulators over the accepted samples: zmin / zmax = the minimum / maximum of z + 0.0f (-0 counts as +0), taken
 *      on the order-preserving integer image of the float; an empty cell holds +inf / -inf.  floor_hits, obst_hits: uint32 counts.
 *   7. State, int8 in nav_msgs/OccupancyGrid's convention: 100 if obst_hits >= min_hits, else 0 if floor_hits >= min_hits, else -1.
 *   8. Clearance.  dist2[iy][ix] = min(R R, min over the obstacle cells (x', y') of (ix - x')^2 + (iy - y')^2), an int32, exact.
 *      An obstacle cell has state 100; with unknown_is_obstacle, state -1 counts as well.  R = max_dist_cells.  The clearance
 *      in metres is sqrtf((float)dist2) * res, which the caller takes itself.  Cells outside the grid are no obstacles.
 *   9. Outputs (ssf_navgrid_out; each optional, NULL = not produced and, where possible, not computed):
 *        zmin, zmax  height x width f32        hits  height x width x 2 u32: (floor_hits, obst_hits)
 *        state       height x width i8         dist2 height x width i32 (the state is computed internally if only dist2 is asked for)
 *  10. Stats (exact): rows_used = rows passing 2; samples = the samples that exist (3) of those rows; samples_in_grid = the
 *      samples accepted by 4 and 5; cells_free / cells_occupied / cells_unknown = cells per state; list_entries = (tile, row)
 *      pairs the rasteriser visited (informative: depends on its conservative boxes).  pose = the 12 floats of the grid frame that
 *      was used (the caller's, or the default below): what a publisher needs for the grid's origin.
 *
 * Defaults (ssf_navgrid_default_params) are design choices, not tuned values: res 0.05 m, width = height = 512, min_hits 1,
 * floor_cos 0.8, splat_scale 2, max_steps 8, max_dist_cells 40, min_conf 0, both stamp ranges INT32_MIN..INT32_MAX, everything
 * else 0 / NULL.  The bands are chosen for a camera carried roughly a metre above the floor, heights measured from the first
 * camera (see pose NULL): z_min -1.5 (half a metre below where the floor is expected), floor_max -0.8 (everything more than
 * about 0.2 m above that floor is an obstacle), z_max 0.5 (what is more than half a metre above the camera is passed under).
 * pose NULL: grid x = map x, grid y = map z, grid z = -map y (the map frame is the first camera's, y down), i.e.
 * R = (1 0 0 | 0 0 -1 | 0 1 0); the height origin is map y = 0; the grid is centred on the handle's current camera position p,
 * snapped to a multiple of res so that successive grids are cell-aligned:
 *      t = ((floorf(p.x / res) - (float)(width / 2)) * res,  0,  (floorf(p.z / res) - (float)(height / 2)) * res).
 * ssf_navgrid_default_pose writes that frame for the handle's current pose (it reads width, height and res of p only), for a
 * caller that wants it before the grid.  A caller that knows how its camera is mounted passes its own pose and bands
 * (INTEGRATION.md).
 *
 * Refused with SSF_ERR_INVALID_ARG: a NULL handle or params; `out` NULL or every output NULL; width or height outside 1..4096;
 * res not finite or <= 0; splat_scale < 0 or not finite (0 = the default 2); max_steps outside 1..16; max_dist_cells outside
 * 1..1024; min_hits < 1; z_max < z_min (or either a NaN); t_init_min > t_init_max or t_last_min > t_last_max; floor_cos outside
 * [0, 1].  With SSF_ERR_STATE: frames pending in the extract pipeline; a sharded handle (cfg.nranks > 1).  A tile list longer
 * than 2^32 - 1 entries is refused with SSF_ERR_DEVICE, never wrapped.
 *
 * The call is synchronous and runs on the handle's stream.  It changes no state of the handle: a grid built between two frames
 * changes no later pose or model bit.  Every call rebuilds the whole grid.  Working buffers are allocated on first use and grown
 * as a whole; a growth that fails returns SSF_ERR_DEVICE and leaves the handle working.  With on_device the outputs are device
 * pointers, otherwise host memory.  Kernels appear in ssf_get_kernel_times under profile = 1 (navgrid_prep, navgrid_fill,
 * navgrid_tile, navgrid_cells, navgrid_columns, navgrid_rows).
 *
 * Only the HIP product library (libssf_hip.so) exports these functions; the ABI version of ssf.h is unchanged.
 */
#ifndef SSF_NAVGRID_H
#define SSF_NAVGRID_H

#include "ssf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ssf_navgrid_params {
    const float* pose;                /* 12 floats grid-to-map (ssf_get_pose layout); NULL = floor-aligned about the camera (above) */
    int     width, height;            /* cells along grid x / grid y, 1..4096 each */
    float   res;                      /* metres per cell */
    float   z_min, z_max;             /* accepted heights (grid z) */
    float   floor_max;                /* z <= floor_max: floor band; above: obstacle band */
    float   floor_cos;                /* a floor sample needs |N.z| >= floor_cos */
    float   min_conf;                 /* rows with conf > min_conf (strict) */
    int32_t t_init_min, t_init_max;   /* stamps.x in [min, max] */
    int32_t t_last_min, t_last_max;   /* stamps.y in [min, max] */
    int     visible_only;             /* 1: the visible rows only */
    float   splat_scale;              /* s: half-axes s * sqrt(dims); 0 = 2 */
    int     max_steps;                /* lattice steps per half-axis, 1..16 */
    int     min_hits;                 /* samples that make a cell occupied / free, >= 1 */
    int     max_dist_cells;           /* R: dist2 is capped at R * R, 1..1024 */
    int     unknown_is_obstacle;      /* 1: cells of state -1 count as obstacles in dist2 */
    int     on_device;                /* 1: the outputs are device pointers */
} ssf_navgrid_params;

typedef struct ssf_navgrid_out {      /* any may be NULL, not all */
    float*    zmin;                   /* height x width */
    float*    zmax;                   /* height x width */
    uint32_t* hits;                   /* height x width x 2: floor_hits, obst_hits */
    int8_t*   state;                  /* height x width: 100 occupied, 0 free, -1 unknown */
    int32_t*  dist2;                  /* height x width: squared distance in cells to the nearest obstacle cell, capped */
} ssf_navgrid_out;

typedef struct ssf_navgrid_stats {
    int64_t rows_used;
    int64_t samples;                  /* lattice samples that exist */
    int64_t samples_in_grid;          /* ... accepted by steps 4 and 5 */
    int64_t cells_free, cells_occupied, cells_unknown;
    int64_t list_entries;             /* (tile, row) pairs visited by the rasteriser (informative) */
    float   pose[12];                 /* the grid frame used */
} ssf_navgrid_stats;

int ssf_navgrid_default_params(const ssf_handle* h, ssf_navgrid_params* p);
int ssf_navgrid_default_pose(const ssf_handle* h, const ssf_navgrid_params* p, float* pose12);   /* what pose NULL means now */
int ssf_navgrid_build(ssf_handle* h, const ssf_navgrid_params* p, const ssf_navgrid_out* out, ssf_navgrid_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* SSF_NAVGRID_H */
