/*
 * ssf_navsteer.h -- velocity commands on the navigation grid, on the device: from every pose a lattice of (v, w) candidates is rolled
 * forward as arcs over the grid, each arc is tested for "can still stop" and scored, and the best admissible candidate of every pose
 * comes back as a command with the arc it stands for.  This is the dynamic-window local planner, stated entirely in integers.
 *
 * ssf_navlive_overlay, ssf_navplan_field and ssf_navpath_waypoints turn a depth frame into a grid, a cost-to-goal field and waypoints
 * without the grid leaving the device.  A robot consumes a velocity.  Without this call a caller copies state, dist2 and cost to the
 * host at control rate and rolls the arcs there.  This call reads the three arrays where they lie.
 *
 * All arithmetic is integer and the rule has exactly one answer, so the result does not depend on the order the hardware works in,
 * and a small restatement (tests/navsteer_ref.py) reproduces every output bit for bit.
 *   Units.  A position is fixed point at 1024 sub-units per cell: the cell of (x, y) is (x >> 10, y >> 10), the shift a floor; the
 *      centre of cell ix is ix * 1024 + 512.  A heading is an integer in 1/65536 of a turn: 0 points along +ix and it grows toward
 *      +iy.  A candidate is (v, w): sub-units per step and heading units per step.  The ABI is integer only: metres, radians and
 *      seconds are a wrapper's business (res metres per cell, dt seconds per step: v = speed * dt * 1024 / res,
 *      w = rate * dt * 65536 / 2 pi).
 *   Inputs.  state (int8, height x width, row-major, iy the row) and dist2 (int32, height x width) exactly as ssf_navgrid_build,
 *      ssf_navgrid_carve or ssf_navlive_overlay write them; p = iy * width + ix.  cost (uint32, height x width) exactly as
 *      ssf_navplan_field writes it; it may be NULL iff cost_weight == 0, and is not read then.  poses: n_poses x 3 int32
 *      (x, y, heading), the heading taken & 0xFFFF.  targets: n_poses x 2 int32 (x, y) in sub-units; it may be NULL iff
 *      target_weight == 0, and is not read then.
 *   1. Direction table.  C[k] = floor(16384 * cos(2 pi k / 1024) + 0.5), S[k] likewise with sin, k = 0..1023, computed once on the
 *      host in double (ssf_navsteer_direction_table returns them; it takes no handle and touches no device).  No entry lies closer
 *      than 3.9e-4 to a rounding boundary, so no libm flips one; the table has the exact quarter-turn and mirror symmetries.
 *   2. Candidates.  K = n_v * n_w, candidate c = i * n_w + j has v = v_min + i * v_step, w = w_min + j * w_step.  v_abs_max is the
 *      largest |v| of the lattice.
 *   3. Traversable.  As step 1 of ssf_navplan.h: trav[p] = (state[p] == 0 || (allow_unknown && state[p] == -1)) &&
 *      dist2[p] >= min_dist2.  Cells outside the grid are not traversable.  d(p) = min(max(dist2[p], 0), clearance_cap).  A cell of
 *      any other state (1..99, 101..127, -2..-128) or of negative dist2 is not traversable, whatever allow_unknown.
 *   4. Rollout of one candidate from one pose (x, y, h).  If the start cell is outside the grid or not traversable: free_steps = 0,
 *      min_d = -1, the end is the start, and the candidate is inadmissible.  Otherwise min_d = d(start cell) and, for each of the
 *      n_steps steps:
 *        k  = ((2 h + w + 64) >> 7) & 1023          (the midpoint heading; the shift is a floor and the sum may be negative)
 *        nx = x + ((v * C[k] + 8192) >> 14),  ny = y + ((v * S[k] + 8192) >> 14)       (floor shifts again)
 *        the step is FREE iff the cell of (nx, ny) is traversable and, when both of its coordinates differ from the cell of (x, y),
 *        the two axial cells that share the corner, (nx >> 10, y >> 10) and (x >> 10, ny >> 10), are traversable as well: the
 *        plan's no-corner-cutting rule.  |v| <= 1024, so a step never leaves the 8-neighbourhood.
 *        A free step commits: x = nx, y = ny, h = (h + w) & 0xFFFF, free_steps += 1, min_d = min(min_d, d(new cell)).
 *        The first step that is not free ends the rollout at the last committed state, the END of the candidate.
 *   5. Admissible.  need = min(n_steps, min_free_steps + (brake_div > 0 ? (|v| + brake_div - 1) / brake_div : 0)).  A candidate is
 *      admissible iff the start cell is traversable, free_steps >= need and, with cost_weight > 0, the end cell's cost is not
 *      0xFFFFFFFF.  This is the dynamic window's "can still stop" test; a candidate that collides later than `need` is scored
 *      where it stopped.  The end cell's cost is read iff cost_weight > 0 and the start cell is traversable.
 *   6. Score (int64, lower is better), with dx = |end.x - target.x|, dy = |end.y - target.y| in sub-units:
 *        score = cost_weight * cost[end cell] + target_weight * ((10 * max(dx, dy) + 4 * min(dx, dy)) >> 10)
 *              + clear_weight * (clearance_cap - min_d) + speed_weight * (v_abs_max - |v|) + turn_weight * |w|
 *      The target term is in the field's own unit of 10 per cell.  An inadmissible candidate has score -1.
 *   7. Winner per pose: the admissible candidate with the smallest (score, c).  The pair is unique, so no arrival order shows.
 *   8. Outputs (any may be NULL, not all).  Per pose: best (the candidate, -1 if none), best_cmd (v, w; (0, 0) if none), best_score
 *      (-1 if none), n_admissible, pose_status (0 ok; 1 the start is outside the grid; 2 the start cell is not traversable; 3 no
 *      candidate is admissible), best_len (the entries written to best_traj: 1 + the winner's free_steps, 0 if none), best_traj
 *      ((n_steps + 1) x 3 per pose: (x, y, h) of the start, its heading & 0xFFFF, and of each committed step of the winner; entries
 *      past best_len are not written).  Per candidate (n_poses x K): cand_free, cand_min_d, cand_end (x, y, h), cand_end_cost
 *      (0xFFFFFFFF where unread) and cand_score.
 *   9. Stats.  Exact: poses_ok (status 0), poses_blocked (1 or 2), poses_stuck (3), candidates (n_poses * K), admissible, collided
 *      (candidates with free_steps < n_steps), steps_taken (the sum of free_steps).  Informative only: windows_staged and
 *      windows_global, the workgroups that walked a window of the grid staged on chip and those that walked the grid itself.
 *
 * Defaults (ssf_navsteer_default_params) are design choices, not tuned values: width = height = 512 (the grid's default size),
 * n_v 9, n_w 33, n_steps 32, v_min 0, v_step 64, w_min -2048, w_step 128, min_free_steps 2, brake_div 128, clearance_cap 64,
 * cost_weight 1, clear_weight 1, speed_weight 1; min_dist2, allow_unknown, target_weight, turn_weight, walk, n_poses and on_device 0:
 * a caller sets n_poses.
 *
 * Refused with SSF_ERR_INVALID_ARG: h, p, state, dist2 or poses NULL; `out` NULL or every output NULL; cost NULL with
 * cost_weight > 0; targets NULL with target_weight > 0; width or height outside 1..4096; min_dist2 < 0; allow_unknown not 0 or 1;
 * clearance_cap outside 0..1024 * 1024; n_v outside 1..256; n_w outside 1..1024; n_v * n_w > 65536; any |v| of the lattice > 1024 or
 * any |w| > 16384; n_steps outside 1..256; n_poses outside 1..4096; n_poses * n_v * n_w > 1 << 24; min_free_steps outside 0..256;
 * brake_div outside 0..1024; a weight outside 0..1000, or all five 0; walk not 0 or 1.  With SSF_ERR_STATE: frames pending in the
 * extract pipeline; a sharded handle (cfg.nranks > 1).  After any refusal the handle keeps working.
 *
 * on_device governs state, dist2, cost, poses, targets and every output: the grid of ssf_navlive_overlay and the field of
 * ssf_navplan_field are steered on without leaving the device.  The call is synchronous on the handle's stream and changes no state
 * of the handle: a call between two frames changes no later pose or model bit.  Working buffers are allocated on first use and
 * grown as a whole; a growth that fails returns SSF_ERR_DEVICE and leaves the handle working.  Kernels appear in
 * ssf_get_kernel_times under profile = 1 (navsteer_pack, navsteer_roll, navsteer_pick).
 *
 * Who exports these functions: libssf_hip_steer.so, which is libssf_hip_live.so's objects with this call linked in, so that a robot
 * that builds, carves, plans, explores, drives, overlays and steers loads one library.  None of the six older libraries does: their
 * exported symbols are what they were.  A caller links or loads libssf_hip_steer.so INSTEAD of the others, never next to them: a
 * handle belongs to the library that created it.  The ABI version of ssf.h is unchanged.
 */
#ifndef SSF_NAVSTEER_H
#define SSF_NAVSTEER_H

#include "ssf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SSF_NAVSTEER_SUBUNITS   1024          /* sub-units per cell */
#define SSF_NAVSTEER_TURN       65536         /* heading units per turn */
#define SSF_NAVSTEER_DIRECTIONS 1024          /* entries of the direction table */
#define SSF_NAVSTEER_NO_COST    0xFFFFFFFFu   /* cand_end_cost where the cost was not read; the field's unreached value */

typedef struct ssf_navsteer_params {
    int   width, height;              /* cells along grid x / grid y, 1..4096 each */
    int   min_dist2;                  /* a traversable cell has dist2 >= min_dist2 (the plan's meaning), >= 0 */
    int   allow_unknown;              /* 1: cells of state -1 are traversable as well (the plan's meaning) */
    int   clearance_cap;              /* d(p) = min(max(dist2, 0), clearance_cap), 0..1024 * 1024 */
    int   n_poses;                    /* 1..4096 */
    int   n_v, n_w;                   /* the lattice: 1..256 speeds x 1..1024 turn rates, n_v * n_w <= 65536 */
    int   v_min, v_step;              /* v = v_min + i * v_step, sub-units per step, every |v| <= 1024 */
    int   w_min, w_step;              /* w = w_min + j * w_step, heading units per step, every |w| <= 16384 */
    int   n_steps;                    /* steps of a rollout, 1..256 */
    int   min_free_steps;             /* 0..256 */
    int   brake_div;                  /* a candidate needs ceil(|v| / brake_div) more free steps; 0: none; 0..1024 */
    int   cost_weight, target_weight, clear_weight, speed_weight, turn_weight;       /* 0..1000 each, not all 0 */
    int   walk;                       /* 0: a pose's window of the grid is staged on chip where that was measured to pay; 1: every rollout
                                         walks the grid itself.  The outputs and the exact stats are the same either way: a measuring knob */
    int   on_device;                  /* 1: state, dist2, cost, poses, targets and the outputs are device pointers */
} ssf_navsteer_params;

typedef struct ssf_navsteer_out {     /* any may be NULL, not all */
    int32_t*  best;                   /* n_poses: the winning candidate, -1 if none */
    int32_t*  best_cmd;               /* n_poses x 2: (v, w), (0, 0) if none */
    int64_t*  best_score;             /* n_poses: -1 if none */
    int32_t*  n_admissible;           /* n_poses */
    int32_t*  pose_status;            /* n_poses: 0 ok, 1 start outside the grid, 2 start not traversable, 3 no admissible candidate */
    int32_t*  best_len;               /* n_poses: entries written to best_traj */
    int32_t*  best_traj;              /* n_poses x (n_steps + 1) x 3: (x, y, h); entries past best_len are not written */
    int32_t*  cand_free;              /* n_poses x K */
    int32_t*  cand_min_d;             /* n_poses x K: -1 where the start is not traversable */
    int32_t*  cand_end;               /* n_poses x K x 3: (x, y, h) */
    uint32_t* cand_end_cost;          /* n_poses x K: SSF_NAVSTEER_NO_COST where unread */
    int64_t*  cand_score;             /* n_poses x K: -1 where inadmissible */
} ssf_navsteer_out;

typedef struct ssf_navsteer_stats {
    int64_t poses_ok, poses_blocked, poses_stuck;
    int64_t candidates, admissible, collided, steps_taken;
    int64_t windows_staged, windows_global;       /* informative */
} ssf_navsteer_stats;

int ssf_navsteer_default_params(const ssf_handle* h, ssf_navsteer_params* p);
int ssf_navsteer_direction_table(int32_t* cos_out, int32_t* sin_out);      /* 1024 entries each; either may be NULL */
int ssf_navsteer_rollouts(ssf_handle* h, const ssf_navsteer_params* p, const int8_t* state, const int32_t* dist2, const uint32_t* cost,
                          const int32_t* poses, const int32_t* targets, const ssf_navsteer_out* out, ssf_navsteer_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* SSF_NAVSTEER_H */
