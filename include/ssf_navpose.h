/*
 * ssf_navpose.h -- plan over (x, y, heading) on the navigation grid, on the device: the cost-to-goal field over (cell, heading bin)
 * for the oriented footprint of ssf_navfoot.h, its projection onto the cells, and for a list of start poses the state paths down it.
 *
 * ssf_navplan_field (ssf_navplan.h) knows one radius and no heading.  With the inscribed radius of a long body it routes the body
 * round corners it cannot turn; with the circumscribed radius it refuses corridors the body drives through lengthwise.  The rollouts
 * of ssf_navfoot.h then stop in front of the bend the plan sent them to.  This call plans in the space the body moves in: a state is a
 * cell and a heading bin, traversable where the heading layers (ssf_navfoot_layers) say the body fits; the body drives along its
 * heading (or against it, at a price) and turns on the spot one bin at a time where the next bin fits as well.
 *
 * All arithmetic is integer.  Shortest-path cost over an integer-weighted graph has exactly one answer, so the result does not depend
 * on the order the hardware works in, and a small restatement (tests/navpose_ref.py: numpy prep, a heapq Dijkstra from the goals, the
 * projection and the trace) reproduces every output bit for bit.  Conventions (moves, weights, penalty, pose units, heading bins) are
 * those of ssf_navplan.h, ssf_navsteer.h and ssf_navfoot.h; where this text and those headers disagree, those headers win.
 *   Inputs.  free_mask (uint32, height x width) as ssf_navfoot_layers writes it; dist2 (int32, height x width) as the grid calls write
 *      it.  B = n_headings in {1, 2, 4, 8, 16, 32}; bin b stands for direction index k_b = b * (1024 / B).  A state is (p, b) with
 *      p = iy * width + ix; there are N = width * height * B states.
 *   1. Traversable.  trav[p, b] = bit b of free_mask[p] is set && dist2[p] >= min_dist2.  The mask already carries allow_unknown.
 *      Cells outside the grid are not traversable.
 *   2. Penalty.  pen[p] exactly as in step 2 of ssf_navplan.h, with the same soft_dist2 and near_penalty.
 *   3. Translations.  The eight moves k = 0..7 have (dx, dy) and w(k) as in ssf_navplan.h; their direction indices are
 *      A = (0, 256, 512, 768, 128, 384, 640, 896).  circ(a, b) = min((a - b) & 1023, (b - a) & 1023).  At bin b, move k is a FORWARD
 *      move iff circ(k_b, A[k]) <= move_tol; otherwise, with allow_reverse, a REVERSE move iff circ(k_b + 512, A[k]) <= move_tol;
 *      otherwise it is not a move of that bin.  move_tol lies in 0..256: 64 is "the grid direction nearest the heading, both on a
 *      tie"; 256 with reverse_cost 0 is a holonomic base.  A move (p, b) -> (q, b) is admissible iff (q, b) is traversable and, for a
 *      diagonal, the two axial cells at the corner are traversable at bin b (the plan's no-corner-cutting rule under the rollouts'
 *      mask test).  Its cost is w(k) + pen[q], plus reverse_cost for a reverse move.
 *   4. Rotations.  (p, b) -> (p, b') for b' = (b +- 1) & (B - 1) with b' != b, admissible iff (p, b') is traversable; the cost is
 *      turn_cost >= 1.  For B = 2 the two rotations are the same transition; for B = 1 there is none.
 *   5. The move table (ssf_navpose_moves; it takes no handle and touches no device).  B x 8 int8: 0 = not a move of the bin,
 *      1 = forward, 2 = reverse.  The kernels read this table.
 *   6. Goals.  goals: n_goals x (ix, iy, bin) of int32, HOST memory always.  bin = -1 names every traversable bin of the cell.  An
 *      entry is counted exactly once: in goals_outside if the cell is outside the grid or the bin outside -1..B-1; in goals_blocked
 *      if it names no traversable state; in goals_used otherwise.
 *   7. Field.  cost[b][p], uint32, layer-major (B x height x width): the minimum summed cost of an admissible sequence of transitions
 *      from (p, b) to any goal state; 0 on a goal state; 0xFFFFFFFF where there is none.  It is the unique fixed point of
 *      cost[s] = min over transitions s -> t of (c(s -> t) + cost[t]) with the goals at 0: every weight is positive, so the plan's
 *      induction carries over and the order of relaxation cannot matter.
 *   8. Projection.  cell_cost[p] (uint32) is the minimum over b of cost[b][p]; cell_bin[p] (uint8) the smallest b that attains it, or
 *      255 where no bin is reached.  cell_cost is what ssf_navfoot_rollouts takes as `cost`, unchanged.
 *   9. Starts.  starts: n_starts x (x, y, heading) of int32 in ssf_navsteer.h's pose units, HOST memory always.  The cell is
 *      (x >> 10, y >> 10), the bin (((h & 0xFFFF) + half) >> shift) & (B - 1) with ssf_navfoot.h's shift and half: the cell and bin a
 *      rollout from that pose starts in.  start_status: 0 reached; 1 outside the grid; 2 the state is not traversable; 3 no goal
 *      reachable; 4 reached, but the path was truncated at max_path.  start_cost is cost[start state], or 0xFFFFFFFF (status 1, 2,
 *      3).  The path: from each state take the admissible transition with the smallest c + cost[t], ties to the smallest transition
 *      number (0..7 the moves, 8 = bin + 1, 9 = bin - 1); it ends at a state of cost 0, which is included.  path is
 *      n_starts x max_path x 3 int32 (ix, iy, bin); path_len, truncation and max_path == 0 behave as in ssf_navplan.h.
 *  10. Stats (exact): states_traversable; states_reached; cells_reached (some bin reached); goals_used, goals_blocked, goals_outside;
 *      max_cost over the reached states (0 if none).  Informative only: rounds, tile_visits as in ssf_navplan.h.
 *
 * Defaults (ssf_navpose_default_params) are design choices, not tuned values: width = height = 512, n_headings 16, move_tol 64,
 * allow_reverse 1, reverse_cost 10, turn_cost 5; everything else 0 or NULL.
 *
 * Refused with SSF_ERR_INVALID_ARG: h, p, free_mask or dist2 NULL; `out` NULL or every output NULL; n_headings not one of the six
 * values; width or height outside 1..4096; width * height * B > 1 << 26 (at that size the field is 256 MiB); min_dist2 < 0;
 * soft_dist2 outside 0..1024 * 1024; near_penalty outside 0..1000; move_tol outside 0..256; allow_reverse not 0 or 1; reverse_cost
 * outside 0..1000; turn_cost outside 1..1000; n_goals outside 1..65536; n_starts outside 0..4096; max_path outside 0..1 << 20; a list
 * that is NULL with a positive count; max(14 + near_penalty + reverse_cost, turn_cost) * N >= 2^32 - 1 (computed in 64 bits): a
 * shortest sequence visits a state at most once, so below that bound no cost can wrap.  ssf_navpose_moves refuses a bad n_headings,
 * move_tol or allow_reverse and a NULL table.  With SSF_ERR_STATE: frames pending in the extract pipeline; a sharded handle
 * (cfg.nranks > 1).  After any refusal the handle keeps working.
 *
 * on_device governs free_mask, dist2 and every output; goals and starts are host memory always.  The call is synchronous on the
 * handle's stream and changes no state of the handle: a plan made between two frames changes no later pose or model bit.  Working
 * buffers are allocated on first use and grown as a whole; a growth that fails returns SSF_ERR_DEVICE and leaves the handle working.
 * The field is relaxed tile by tile (16 x 16 cells, all B layers) in rounds, each a launch; the host looks at the number of flagged
 * tiles once per SSF_NAVPOSE_ROUND_BATCH rounds; a field that has not settled after N + 2 rounds returns SSF_ERR_DEVICE ("did not
 * converge"): that would be a bug, not an input.  Kernels appear in ssf_get_kernel_times under profile = 1 (navpose_init,
 * navpose_goals, navpose_relax, navpose_stats, navpose_trace).
 *
 * Who exports these functions: libssf_hip_pose.so, which is libssf_hip_foot.so's objects with this file's linked in.  None of the
 * eight older libraries does: their exported symbols are what they were.  A caller links or loads libssf_hip_pose.so INSTEAD of the
 * others, never next to them: a handle belongs to the library that created it.  The ABI version of ssf.h is unchanged.
 */
#ifndef SSF_NAVPOSE_H
#define SSF_NAVPOSE_H

#include "ssf.h"
#include "ssf_navfoot.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SSF_NAVPOSE_UNREACHED   0xFFFFFFFFu
#define SSF_NAVPOSE_NO_BIN      255           /* cell_bin where no bin of the cell is reached */
#define SSF_NAVPOSE_TILE        16            /* cells a side of a relaxation tile */
#define SSF_NAVPOSE_ROUND_BATCH 16            /* rounds launched between two looks at the flagged-tile count */
#define SSF_NAVPOSE_MAX_STATES  (1 << 26)

typedef struct ssf_navpose_params {
    int   width, height;              /* cells along grid x / grid y, 1..4096 each */
    int   n_headings;                 /* B: 1, 2, 4, 8, 16 or 32; width * height * B <= 1 << 26 */
    int   min_dist2;                  /* a traversable state has dist2 >= min_dist2, >= 0 */
    int   soft_dist2;                 /* below this squared clearance a cell costs extra, 0..1024 * 1024; 0 = no penalty */
    int   near_penalty;               /* the extra cost of entering a cell of clearance 0, 0..1000 */
    int   move_tol;                   /* direction units (1024 a turn) between heading and move, 0..256 */
    int   allow_reverse;              /* 1: moves against the heading are allowed */
    int   reverse_cost;               /* the extra cost of a reverse move, 0..1000 */
    int   turn_cost;                  /* the cost of turning by one bin on the spot, 1..1000 */
    const int32_t* goals;             /* n_goals x (ix, iy, bin); bin -1 = every traversable bin; HOST memory always */
    int   n_goals;                    /* 1..65536 */
    const int32_t* starts;            /* n_starts x (x, y, heading) in pose units; HOST memory always */
    int   n_starts;                   /* 0..4096 */
    int   max_path;                   /* states per path, 0..1 << 20; 0 = no path */
    int   on_device;                  /* 1: free_mask, dist2 and the outputs are device pointers */
} ssf_navpose_params;

typedef struct ssf_navpose_out {      /* any may be NULL, not all */
    uint32_t* cost;                   /* n_headings x height x width; 0xFFFFFFFF = not reached */
    uint32_t* cell_cost;              /* height x width: the minimum over the bins */
    uint8_t*  cell_bin;               /* height x width: the smallest bin that attains it; 255 = none */
    uint32_t* start_cost;             /* n_starts */
    int32_t*  start_status;           /* n_starts: 0 reached, 1 outside, 2 not traversable, 3 no goal reachable, 4 truncated */
    int32_t*  path_len;               /* n_starts */
    int32_t*  path;                   /* n_starts x max_path x 3: (ix, iy, bin); entries past path_len are not written */
} ssf_navpose_out;

typedef struct ssf_navpose_stats {
    int64_t states_traversable, states_reached, cells_reached;
    int64_t goals_used, goals_blocked, goals_outside;
    int64_t max_cost;                 /* over the reached states; 0 if none */
    int64_t rounds, tile_visits;      /* informative */
} ssf_navpose_stats;

/* out: n_headings x 8 int8: 0 = not a move of the bin, 1 = forward, 2 = reverse */
int ssf_navpose_moves(int n_headings, int move_tol, int allow_reverse, int8_t* out);
int ssf_navpose_default_params(const ssf_handle* h, ssf_navpose_params* p);
int ssf_navpose_field(ssf_handle* h, const ssf_navpose_params* p, const uint32_t* free_mask, const int32_t* dist2, const ssf_navpose_out* out,
                      ssf_navpose_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* SSF_NAVPOSE_H */
