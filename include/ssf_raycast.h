/*
 * ssf_raycast.h -- rays cast through the fused model on the device: the first disc each ray hits.
 *
 * ssf_render_model answers "what does this pinhole camera see", ssf_query_rows "which rows are in this region", ssf_navgrid_build
 * "what is above this floor cell".  This call answers "what does THIS RAY hit", for any set of rays with their own origins: a
 * simulated 2-D or 3-D lidar scan, a line-of-sight check, picking a surfel in a viewer.  Without it a caller copies the whole model
 * out (ssf_get_model: 104 B per row) and intersects discs on the host.
 *
 * What is hit: the model as it stands after the last completed frame (or ssf_set_model / ssf_apply_deformation).  Every step below is
 * one IEEE f32 operation, in the order written (the library builds with -ffp-contract=off and correctly rounded division and square
 * root), and the winner is an integer minimum, so a numpy f32 restatement that tests every ray against every row reproduces every
 * output bit for bit (tests/raycast_ref.py).  Every parameter is cast to f32 first.  The result is DEFINED without any index: the
 * spatial index the library keeps (below) only makes it cheaper.
 *   1. Pose (R, t0): ray-frame-to-map, 12 floats as ssf_get_pose (R row-major, then t0); NULL = the handle's pose.  A ray (o, d)
 *      becomes O_i = ((Ri0 o.x + Ri1 o.y) + Ri2 o.z) + t0_i and D_i = (Ri0 d.x + Ri1 d.y) + Ri2 d.z.  A ray whose o or d has a
 *      component that is not finite, or whose D is zero in all three components, is INVALID: a miss, counted in rays_invalid.
 *   2. Disc: a row is the two-sided elliptical disc of ssf_render.h: c = position, e1, e2, n = orientation rows 0, 1, 2, half-axes
 *      s * sqrt(dims) (s = splat_scale, 0 = 3).
 *   3. Candidate (map frame, no per-row transform): den = (n.x D.x + n.y D.y) + n.z D.z, w = c - O,
 *      num = (n.x w.x + n.y w.y) + n.z w.z, tt = num / den.  A candidate needs den != 0, tt finite and t_min <= tt <= t_max.
 *   4. Inside: P_i = O_i + tt * D_i (one multiply, one add), V = P - c, a = (V.x e1.x + V.y e1.y) + V.z e1.z, b likewise with e2,
 *      k = s * s; inside iff (a a) dims.y + (b b) dims.x <= (k dims.x) dims.y.
 *   5. Rows: live (with visible_only: a visible row), position finite in all three components, conf > min_conf (strict),
 *      dims.x > 0 and dims.y > 0 and both finite.
 *   6. Winner: the minimum of (bits(tt) << 32) | logical_index over the ray's candidates; logical_index = the row's position in
 *      ssf_get_model's order [visible | out-of-view], so equal tt goes to the smaller index.  tt is a multiple of D, not metres:
 *      unit directions give metres.  t_min > 0 is required, so tt is positive and its bits order like its value.
 *   7. Outputs (each optional, NULL = not produced and not gathered from the store; at least one is required):
 *        t      n f32: tt; 0 on a miss                      index  n i32: the winner's logical index; -1 on a miss
 *        point  n x 3 f32: P in the map frame; 0 on a miss   color  n x 3 f32: as stored; 0 on a miss
 *        normal n x 3 f32: in the map frame, facing the origin: den > 0 ? -n : n; 0 on a miss
 *      With on_device the rays and the outputs are device pointers, otherwise host memory.
 *   8. Stats.  Exact: rays; rays_hit; rays_invalid; rows_indexed = rows passing the position and dims part of 5 (whatever
 *      visible_only and min_conf say); rows_oversize (below).  Informative, they depend on the index: index_entries = (cell, row)
 *      pairs in the grid, cells_visited and candidates_tested = summed over the rays of this call, index_rebuilt = 0 or 1.
 *
 * The index.  A uniform grid of `cell` metres, its cells hashed into 2^hash_bits buckets (colliding cells share a bucket, which is
 * only extra candidates), built by a counting sort; min_conf and visible_only are applied when a candidate is tested, so they do
 * not invalidate it.  It stays on the handle and is reused while the model, cell, splat_scale and hash_bits are unchanged;
 * otherwise the call rebuilds it first (index_rebuilt = 1).  A row of rows_indexed is OVERSIZE -- kept in a list that every ray
 * tests in full, instead of the grid -- iff one of these holds, evaluated in f32 in this order (a NaN comparison counts as
 * "holds"):
 *      a. dims.x < 2^-40 or dims.y < 2^-40;
 *      b. with q(u, v) = (u.x v.x + u.y v.y) + u.z v.z and T = 2^-7: not all of |q(e1,e1) - 1| <= T, |q(e2,e2) - 1| <= T,
 *         |q(n,n) - 1| <= T, |q(e1,e2)| <= T, |q(e1,n)| <= T, |q(e2,n)| <= T (the axes are not orthonormal);
 *      c. with h1 = s * sqrtf(dims.x), h2 = s * sqrtf(dims.y), hs = h1 + h2 and per axis j
 *         E_j = ((|e1_j| * h1 + |e2_j| * h2) * 1.0625f + hs * 0.03125f) + (|c_j| * 2^-20 + cell * 2^-10),
 *         glo_j = (c_j - E_j) / cell, ghi_j = (c_j + E_j) / cell: not (glo_j >= -32000 and ghi_j <= 32000) for some j;
 *      d. the box of cells floorf(glo_j) .. floorf(ghi_j) holds more than 64 cells.
 * Every other row is entered in every cell of that box.  DESIGN.md section 4.12 proves that the grid walk of a ray visits, for every
 * accepted (ray, row) pair, a cell in which the row is entered, and that no ray is cut short.
 *
 * Params.  cell: 0 = 0.125 m (about 10^2 rows per occupied cell at the density of a fused room: two rounds of a 64-lane wave),
 * else 2^-10 <= cell <= 2^10.  hash_bits: 0 = the smallest b in 10..24 with 2^b >= index_entries / 32, else 4..24.  splat_scale: 0 = 3,
 * else 2^-10 <= s <= 2^10.  t_min = t_max = 0 means cfg.range_min / cfg.range_max.  ssf_raycast_default_params fills: pose NULL,
 * everything else 0.
 * Refused with SSF_ERR_INVALID_ARG: a NULL handle or params; NULL rays with n > 0; n < 0; every output NULL; t_min <= 0,
 * t_max <= t_min or either not finite (after the defaults); min_conf a NaN; splat_scale, cell or hash_bits outside the ranges above or
 * not finite.  n == 0 is fine: stats only.  With SSF_ERR_STATE: frames pending in the extract pipeline; a sharded handle
 * (cfg.nranks > 1).  More than 2^32 - 1 index entries are refused with SSF_ERR_DEVICE, never wrapped.
 *
 * The call is synchronous and runs on the handle's stream.  It changes no state that a later frame can see: rays cast between two
 * frames change no later pose or model bit.  Working buffers are allocated on first use and grown as a whole; a growth that fails
 * returns SSF_ERR_DEVICE and leaves the handle working.  Kernels appear in ssf_get_kernel_times under profile = 1 (raycast_prep,
 * raycast_scan, raycast_fill when the index is rebuilt; raycast_march).
 *
 * Only the HIP product library (libssf_hip.so) exports these functions; the ABI version of ssf.h is unchanged.
 */
#ifndef SSF_RAYCAST_H
#define SSF_RAYCAST_H

#include "ssf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ssf_raycast_params {
    const float* pose;        /* 12 floats ray-frame-to-map (ssf_get_pose layout); NULL = the handle's current pose */
    float t_min, t_max;       /* accepted range of tt; both 0 = cfg.range_min / cfg.range_max */
    float min_conf;           /* rows with conf > min_conf (strict) */
    float splat_scale;        /* s: half-axes s * sqrt(dims); 0 = 3 */
    int   visible_only;       /* 1: the visible rows only; 0: every live row */
    int   on_device;          /* 1: rays and outputs are device pointers */
    float cell;               /* metres per cell of the index; 0 = 0.125 */
    int   hash_bits;          /* the index has 2^hash_bits buckets; 0 = chosen from the entry count */
} ssf_raycast_params;

typedef struct ssf_raycast_stats {
    int64_t rays, rays_hit, rays_invalid;
    int64_t rows_indexed, rows_oversize;
    int64_t index_entries;    /* (cell, row) pairs in the grid (informative, as the three below) */
    int64_t cells_visited;    /* cells looked up by this call's rays */
    int64_t candidates_tested;/* bucket and oversize entries tested by this call's rays */
    int64_t index_rebuilt;    /* 1: this call built the index */
} ssf_raycast_stats;

int ssf_raycast_default_params(const ssf_handle* h, ssf_raycast_params* p);
/* rays: n x 6 (origin, direction) in the pose's frame */
int ssf_raycast(ssf_handle* h, const ssf_raycast_params* p, const float* rays, int n, float* t, int32_t* index, float* point,
                float* normal, float* color, ssf_raycast_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* SSF_RAYCAST_H */
