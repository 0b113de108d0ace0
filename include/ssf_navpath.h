/*
 * ssf_navpath.h -- any-angle waypoints from the cell paths of a plan, on the device: every path is reduced to a subsequence of its
 * cells such that consecutive waypoints are joined by a straight segment whose every cell is traversable with the asked clearance.
 *
 * ssf_navplan_field (ssf_navplan.h) returns a path as every cell of an 8-connected staircase: hundreds of cells with a heading
 * change of 45 or 90 degrees every few of them.  A follower needs a few straight legs that keep the robot's clearance.  Without
 * this call a caller copies state, dist2 and the paths to the host and string-pulls there, for every start, every time the map or
 * the goal changes.  This call reads the plan's outputs where they lie.
 *
 * All arithmetic is integer and the rule has exactly one answer, so the result does not depend on the order the hardware works in,
 * and a small restatement (tests/navpath_ref.py) reproduces every output bit for bit.
 *   Inputs.  state (int8, height x width, row-major, iy the row) and dist2 (int32, height x width): exactly what
 *      ssf_navgrid_build / ssf_navgrid_carve write.  p = iy * width + ix.  path (n_paths x max_path x 2 int32, (ix, iy)) and path_len
 *      (n_paths int32): exactly what ssf_navplan_field writes; entries past path_len are not read.
 *   1. Traversable.  As step 1 of ssf_navplan.h: trav[p] = (state[p] == 0 || (allow_unknown && state[p] == -1)) &&
 *      dist2[p] >= min_dist2.  d(p) = max(dist2[p], 0).  Cells outside the grid are not traversable, nor is a cell of any other
 *      state (1..99, 101..127, -2..-128) or of negative dist2, whatever allow_unknown.
 *   2. Path check.  L = path_len[i].  Status 1: L < 0 or L > max_path.  Status 2: some cell of the path is outside the grid or not
 *      traversable.  Status 3: two consecutive cells are not distinct 8-neighbours (their Chebyshev distance is not 1).  The
 *      smallest applicable status wins.  Such a path gets 0 waypoints and path_min -1; the other paths of the call are unaffected.
 *      L == 0 is status 0 with 0 waypoints.  The path need not obey the plan's no-corner-cutting rule.
 *   3. Segment walk from cell a to cell b: an integer supercover of the segment between the two cell centres.  dx = |bx - ax|,
 *      dy = |by - ay|, sx, sy the signs, (x, y) = a, e = dx - dy, n = dx + dy.  Visit (x, y).  While n > 0:
 *        if e > 0:       x += sx; e -= 2 dy; n -= 1;
 *        else if e < 0:  y += sy; e += 2 dx; n -= 1;
 *        else (the segment passes exactly through a lattice corner): visit (x + sx, y) and (x, y + sy), then x += sx; y += sy;
 *                        e += 2 dx - 2 dy; n -= 2;
 *        after each branch visit (x, y).
 *      A segment through the corner that two diagonal obstacles share is therefore blocked: the plan's no-corner-cutting rule
 *      carried over to segments.  All visited cells lie in the bounding box of a and b.
 *   4. Threshold.  base = max(min_dist2, los_dist2).  Without keep_clearance thr(a, j) = base.  With it
 *      thr(a, j) = max(base, min(clearance_cap, min over a <= i <= j of d(p_i))): a shortcut never comes closer to an obstacle
 *      than the piece of path it replaces, up to the cap.  visible(a, j): every cell that the walk from p_a to p_j visits is
 *      traversable and has d >= thr(a, j).
 *   5. Greedy farthest-visible.  Waypoint 0 is p_0.  From the anchor index a < L - 1 the next anchor is
 *      J = max({a + 1} u {j : a < j <= min(L - 1, a + lookahead), visible(a, j)}).  J = a + 1 is taken even when it is not visible:
 *      that step is FORCED, so progress is guaranteed; it happens when los_dist2 (or the cap) asks for more clearance than the path
 *      has, or when the path cuts a corner.  Visibility is not monotone in j: all candidates of the window count, not the first
 *      failure.  The last waypoint is p_(L-1).
 *   6. Outputs (any may be NULL, not all).  waypoints: n_paths x max_waypoints x 4 int32, each (ix, iy, index, seg_min): index is the
 *      cell's index into the path, with bit 30 (SSF_NAVPATH_FORCED) set on a forced step, that is one whose segment from the
 *      waypoint before was not visible; seg_min is the minimum d over the cells that the walk from the waypoint before visits (for
 *      waypoint 0: d(p_0)).  n_waypoints[i] is the number of waypoints written; entries past it are not written.  A path with more
 *      than max_waypoints waypoints keeps its first max_waypoints (status 4).  status[i]: 0 ok; 1, 2, 3 as in step 2; 4 ok but
 *      truncated.  path_min[i]: the minimum of seg_min over the waypoints written, -1 if none.
 *   7. Stats.  Exact: paths_ok (status 0 or 4), paths_bad (1, 2, 3), paths_truncated (4), waypoints (the sum of n_waypoints),
 *      forced_steps (the waypoints written that carry bit 30), cells_in (the sum of L over the paths of status 0 or 4).
 *      Informative only: segments_tested = the walks begun.
 *
 * Defaults (ssf_navpath_default_params) are design choices, not tuned values: width = height = 512 (the grid's default size),
 * min_dist2 0, allow_unknown 0, los_dist2 0, keep_clearance 0, clearance_cap 0, lookahead 256, n_paths 0, max_path 0,
 * max_waypoints 0, on_device 0: a caller sets the last four.
 *
 * Refused with SSF_ERR_INVALID_ARG: h, p, state, dist2, path or path_len NULL; `out` NULL or every output NULL; width or height
 * outside 1..4096; min_dist2 < 0; los_dist2 < 0; keep_clearance not 0 or 1; clearance_cap outside 0..1024 * 1024; lookahead outside
 * 1..4096; n_paths outside 1..4096; max_path or max_waypoints outside 1..1 << 20.  With SSF_ERR_STATE: frames pending in the extract
 * pipeline; a sharded handle (cfg.nranks > 1).  After any refusal the handle keeps working.
 *
 * on_device governs state, dist2, path, path_len and every output: a plan made with on_device is refined without leaving the
 * device.  The call is synchronous on the handle's stream and changes no state of the handle: a call between two frames changes no
 * later pose or model bit.  Working buffers are allocated on first use and grown as a whole; a growth that fails returns
 * SSF_ERR_DEVICE and leaves the handle working.  Kernels appear in ssf_get_kernel_times under profile = 1 (navpath_pack,
 * navpath_check, navpath_pull).
 *
 * Who exports these functions: libssf_hip_drive.so, which is libssf_hip_explore.so's objects (the product, the carve, the plan, the
 * frontier regions) with this call linked in, so that a robot that builds, carves, plans, explores and drives loads one library.
 * None of libssf_hip.so, libssf_hip_navcarve.so, libssf_hip_nav.so and libssf_hip_explore.so does: their exported symbols are what
 * they were.  A caller links or loads libssf_hip_drive.so INSTEAD of the others, never next to them: a handle belongs to the
 * library that created it.  The ABI version of ssf.h is unchanged.
 */
#ifndef SSF_NAVPATH_H
#define SSF_NAVPATH_H

#include "ssf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SSF_NAVPATH_FORCED     0x40000000     /* bit 30 of a waypoint's index word: the segment that leads to it was not visible */
#define SSF_NAVPATH_INDEX_MASK 0x3FFFFFFF     /* the index itself */

typedef struct ssf_navpath_params {
    int   width, height;              /* cells along grid x / grid y, 1..4096 each */
    int   min_dist2;                  /* a traversable cell has dist2 >= min_dist2 (the plan's meaning), >= 0 */
    int   allow_unknown;              /* 1: cells of state -1 are traversable as well (the plan's meaning) */
    int   los_dist2;                  /* every cell of a segment has d >= max(min_dist2, los_dist2), >= 0 */
    int   keep_clearance;             /* 1: a segment keeps the clearance of the piece of path it replaces, up to clearance_cap */
    int   clearance_cap;              /* 0..1024 * 1024 */
    int   lookahead;                  /* candidates per anchor, 1..4096 cells */
    int   n_paths;                    /* 1..4096 */
    int   max_path;                   /* cells per path of `path`, 1..1 << 20 */
    int   max_waypoints;              /* waypoints per path of `waypoints`, 1..1 << 20 */
    int   on_device;                  /* 1: state, dist2, path, path_len and the outputs are device pointers */
} ssf_navpath_params;

typedef struct ssf_navpath_out {      /* any may be NULL, not all */
    int32_t* n_waypoints;             /* n_paths */
    int32_t* status;                  /* n_paths: 0 ok, 1 bad length, 2 a cell outside or not traversable, 3 not 8-connected, 4 truncated */
    int32_t* waypoints;               /* n_paths x max_waypoints x 4: (ix, iy, index | forced bit, seg_min); entries past n_waypoints are not written */
    int32_t* path_min;                /* n_paths: the minimum seg_min; -1 if no waypoint */
} ssf_navpath_out;

typedef struct ssf_navpath_stats {
    int64_t paths_ok, paths_bad, paths_truncated;
    int64_t waypoints, forced_steps, cells_in;
    int64_t segments_tested;          /* informative */
} ssf_navpath_stats;

int ssf_navpath_default_params(const ssf_handle* h, ssf_navpath_params* p);
int ssf_navpath_waypoints(ssf_handle* h, const ssf_navpath_params* p, const int8_t* state, const int32_t* dist2, const int32_t* path,
                          const int32_t* path_len, const ssf_navpath_out* out, ssf_navpath_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* SSF_NAVPATH_H */
