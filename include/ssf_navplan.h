/*
 * ssf_navplan.h -- plan on the navigation grid, on the device: the cost-to-goal field over the traversable cells and, for a list
 * of start cells, the cell paths down that field.
 *
 * ssf_navgrid_build (ssf_navgrid.h) and ssf_navgrid_carve (ssf_navcarve.h) say where a robot can be; this call says which cells it
 * can REACH, how expensive that is and along which cells.  Without it a caller copies state and dist2 to the host, thresholds the
 * clearance and runs Dijkstra there, every time the map or the goal changes.  With the grid's frontier cells as goals the same
 * call answers "where is the nearest unexplored edge I can drive to": the natural consumer of the carve.
 *
 * All arithmetic is integer.  Shortest-path cost over an integer-weighted grid has exactly one answer, so the result does not
 * depend on the order the hardware works in, and a small restatement (numpy prep, a heapq Dijkstra from the goals and the path
 * trace: tests/navplan_ref.py) reproduces every output bit for bit.
 *   Inputs.  state (int8, height x width, row-major, iy the row) and dist2 (int32, height x width): exactly what
 *      ssf_navgrid_build / ssf_navgrid_carve write.  The call reads them as given and never rebuilds the grid.  p = iy * width + ix.
 *      Note that dist2 is capped at the grid's max_dist_cells^2: min_dist2 or soft_dist2 above that cap ask for more clearance
 *      than the grid ever reports.
 *   1. Traversable.  trav[p] = (state[p] == 0 || (allow_unknown && state[p] == -1)) && dist2[p] >= min_dist2.  min_dist2 >= 0 is
 *      the robot's squared radius in cells.  Cells outside the grid are not traversable.  A cell of any other state (1..99 of a
 *      nav_msgs/OccupancyGrid, 101..127, -2..-128) is neither free nor unknown: not traversable whatever allow_unknown, and no
 *      frontier's neighbour (step 4); a negative dist2 is below every min_dist2.
 *   2. Penalty.  pen[p] = soft_dist2 > 0 ? near_penalty * (soft_dist2 - min(dist2[p], soft_dist2)) / soft_dist2 : 0 (integer
 *      division; a negative dist2, which no grid call writes, counts as 0).  0 <= near_penalty <= 1000 and
 *      0 <= soft_dist2 <= 1024 * 1024, so the product fits an int32.
 *   3. Moves.  Directions k = 0..7: (+1,0), (0,+1), (-1,0), (0,-1), (+1,+1), (-1,+1), (-1,-1), (+1,-1) as (dx, dy).  w(k) = 10 for
 *      k < 4, 14 otherwise.  A move p -> q is admissible iff q is traversable and, for a diagonal, the two axial cells that share
 *      the corner, (p.x + dx, p.y) and (p.x, p.y + dy), are both traversable (no corner cutting).  Its cost is w(k) + pen[q].
 *   4. Frontier.  frontier[p] = state[p] == 0 && some 4-neighbour inside the grid has state -1 (uint8, 0 / 1).
 *   5. Goals.  goals: n_goals pairs (ix, iy) of int32, HOST memory always.  With goals_from_frontier every frontier cell is a goal
 *      as well.  A goal entry outside the grid counts in goals_outside, one on a non-traversable cell in goals_blocked, every
 *      other entry in goals_used (duplicates count per entry).  The traversable frontier cells, which are the ones used as goals,
 *      are counted in frontier_goals (0 without goals_from_frontier).
 *   6. Field.  cost[p], uint32, is the minimum over the admissible move sequences from p to any goal of the summed move costs; a
 *      goal cell has cost 0; where there is no such sequence, or p is not traversable, the cost is 0xFFFFFFFF.  Equivalently it is
 *      the unique fixed point of cost[p] = min_k (w(k) + pen[q_k] + cost[q_k]) with the goals at 0: all weights are positive, so
 *      the order of relaxation cannot matter.
 *   7. Starts.  starts: n_starts pairs (ix, iy), HOST memory always.  start_status: 0 reached; 1 outside the grid; 2 not
 *      traversable; 3 no goal reachable; 4 reached, but the path was truncated at max_path.  start_cost is cost[start], or
 *      0xFFFFFFFF (status 1, 2, 3).  The path: p_0 is the start; p_(i+1) is the admissible neighbour q of p_i with the smallest
 *      w(k) + pen[q] + cost[q], ties to the smallest k (by step 6 that minimum equals cost[p_i]); the path ends at a cell of cost
 *      0, which is included.  path is n_starts x max_path x 2 int32 (ix, iy); path_len is the number of cells written; entries
 *      past path_len are not written.  A path of more than max_path cells keeps its first max_path (status 4).  With
 *      max_path == 0 no path is produced: path_len is 0 and the status is 0..3.
 *   8. Stats (exact): cells_traversable; cells_reached = the cells with cost != 0xFFFFFFFF; frontier_cells; frontier_goals;
 *      goals_used, goals_blocked, goals_outside; max_cost over the reached cells (0 if none).  Informative only: rounds = the
 *      relaxation rounds in which some tile was worked on, tile_visits = the (round, tile) pairs worked on.
 *
 * Defaults (ssf_navplan_default_params) are design choices, not tuned values: width = height = 512 (the grid's default size),
 * min_dist2 0, soft_dist2 0, near_penalty 0, allow_unknown 0, goals NULL, n_goals 0, goals_from_frontier 0, starts NULL,
 * n_starts 0, max_path 0, on_device 0.
 *
 * Refused with SSF_ERR_INVALID_ARG: h, p, state or dist2 NULL; `out` NULL or every output NULL (frontier alone is a valid
 * request); width or height outside 1..4096; min_dist2 < 0; soft_dist2 outside 0..1024 * 1024; near_penalty outside 0..1000;
 * n_goals outside 0..65536; n_starts outside 0..4096; max_path outside 0..1 << 20; a list that is NULL with a positive count;
 * n_goals == 0 && !goals_from_frontier; (14 + near_penalty) * width * height >= 2^32 - 1 (computed in 64 bits), so that no
 * reachable cost can wrap.  With SSF_ERR_STATE: frames pending in the extract pipeline; a sharded handle (cfg.nranks > 1).  After
 * any refusal the handle keeps working.
 *
 * on_device governs state, dist2 and every output; goals and starts are host memory always.  The call is synchronous on the
 * handle's stream and changes no state of the handle: a plan made between two frames changes no later pose or model bit.  Working
 * buffers are allocated on first use and grown as a whole; a growth that fails returns SSF_ERR_DEVICE and leaves the handle
 * working.  The field is relaxed tile by tile (32 x 32 cells) in rounds, each a launch; a field that has not settled after
 * width * height + 2 rounds returns SSF_ERR_DEVICE ("did not converge"): that would be a bug, not an input.  Kernels appear in
 * ssf_get_kernel_times under profile = 1 (navplan_init, navplan_goals, navplan_relax, navplan_stats, navplan_trace).
 *
 * Who exports these functions: libssf_hip_nav.so, which is the product library's objects with the carve and the plan linked in
 * (it exports everything libssf_hip.so and libssf_hip_navcarve.so do, and these), so that a robot loads one library.  Neither
 * libssf_hip.so nor libssf_hip_navcarve.so does: their exported symbols are what they were.  A caller of the plan links or loads
 * libssf_hip_nav.so INSTEAD of the others, never next to them: a handle belongs to the library that created it.  The ABI version
 * of ssf.h is unchanged.
 */
#ifndef SSF_NAVPLAN_H
#define SSF_NAVPLAN_H

#include "ssf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SSF_NAVPLAN_UNREACHED 0xFFFFFFFFu

typedef struct ssf_navplan_params {
    int   width, height;              /* cells along grid x / grid y, 1..4096 each */
    int   min_dist2;                  /* a traversable cell has dist2 >= min_dist2 (the robot's squared radius in cells), >= 0 */
    int   soft_dist2;                 /* below this squared clearance a cell costs extra, 0..1024 * 1024; 0 = no penalty */
    int   near_penalty;               /* the extra cost of entering a cell of clearance 0, 0..1000 */
    int   allow_unknown;              /* 1: cells of state -1 are traversable as well */
    const int32_t* goals;             /* n_goals x (ix, iy); HOST memory always */
    int   n_goals;                    /* 0..65536 */
    int   goals_from_frontier;        /* 1: every frontier cell is a goal as well */
    const int32_t* starts;            /* n_starts x (ix, iy); HOST memory always */
    int   n_starts;                   /* 0..4096 */
    int   max_path;                   /* cells per path, 0..1 << 20; 0 = no path */
    int   on_device;                  /* 1: state, dist2 and the outputs are device pointers */
} ssf_navplan_params;

typedef struct ssf_navplan_out {      /* any may be NULL, not all */
    uint32_t* cost;                   /* height x width; 0xFFFFFFFF = not reached */
    uint8_t*  frontier;               /* height x width, 0 / 1 */
    uint32_t* start_cost;             /* n_starts */
    int32_t*  start_status;           /* n_starts: 0 reached, 1 outside, 2 not traversable, 3 no goal reachable, 4 truncated */
    int32_t*  path_len;               /* n_starts */
    int32_t*  path;                   /* n_starts x max_path x 2: (ix, iy); entries past path_len are not written */
} ssf_navplan_out;

typedef struct ssf_navplan_stats {
    int64_t cells_traversable, cells_reached, frontier_cells, frontier_goals;
    int64_t goals_used, goals_blocked, goals_outside;
    int64_t max_cost;                 /* over the reached cells; 0 if none */
    int64_t rounds, tile_visits;      /* informative */
} ssf_navplan_stats;

int ssf_navplan_default_params(const ssf_handle* h, ssf_navplan_params* p);
int ssf_navplan_field(ssf_handle* h, const ssf_navplan_params* p, const int8_t* state, const int32_t* dist2, const ssf_navplan_out* out,
                      ssf_navplan_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* SSF_NAVPLAN_H */
