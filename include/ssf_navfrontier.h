/*
 * ssf_navfrontier.h -- the frontier of the navigation grid as REGIONS, on the device: the frontier cells grouped into connected
 * regions, the specks dropped, and per region what an exploring robot ranks by: its size, where it is, its cheapest cell to drive
 * to and how much unknown space a look from there would show.
 *
 * ssf_navgrid_build / ssf_navgrid_carve (ssf_navgrid.h, ssf_navcarve.h) say what is floor, obstacle and unknown; ssf_navplan_field
 * (ssf_navplan.h) says what each cell costs to reach.  With goals_from_frontier the plan drives to the nearest frontier CELL, which
 * may be a one-cell speck between two chair legs.  This call closes the loop from "grid" to "where do I go next": without it a
 * caller copies state, dist2 and the cost field to the host, labels components there and walks rays there, every time the map
 * changes.
 *
 * All arithmetic is integer and every result is defined without reference to an order of work, so a small restatement (numpy for
 * the members, a plain BFS for the regions, Python sets for the gain, sorted() for the order: tests/navfrontier_ref.py) reproduces
 * every output bit for bit.
 *   Inputs.  state (int8, height x width, row-major, iy the row) and dist2 (int32, height x width): exactly what
 *      ssf_navgrid_build / ssf_navgrid_carve write.  cost (uint32, height x width): exactly what ssf_navplan_field writes,
 *      0xFFFFFFFF = not reached.  p = iy * width + ix.  dist2 and cost may be NULL (steps 1, 3, 4).
 *   1. Member.  member[p] = state[p] == 0 && some 4-neighbour inside the grid has state -1: step 4 of ssf_navplan.h, word for
 *      word.  With traversable_only, dist2[p] >= min_dist2 is required as well.  dist2 == NULL is allowed only with
 *      traversable_only == 0.  A state other than 0, -1 and 100 (1..99, 101..127, -2..-128) is no member, makes no member of its
 *      neighbour, does not stop a ray of step 6 and is not counted by one; a negative dist2 is below every min_dist2.
 *   2. Regions.  The connected components of the members under `connectivity`: 8 (the default: the eight neighbours) or 4 (the
 *      four axial ones).  A region's label is the smallest p among its cells, so the labelling has one answer whatever order the
 *      hardware works in.
 *   3. Per region, exact: cells; sum_x, sum_y = the sums of the cells' ix and iy (int64: the caller divides for the centroid); the
 *      bounding box x0 <= ix <= x1, y0 <= iy <= y1; the representative (rep_x, rep_y, rep_cost): the member with the least
 *      (cost[p], p) among the region's members with cost[p] != 0xFFFFFFFF.  With cost == NULL, or no such member,
 *      rep_cost = 0xFFFFFFFF and the representative is the label cell.
 *   4. Kept.  A region is kept iff cells >= min_cells and, with reachable_only, rep_cost != 0xFFFFFFFF.  reachable_only requires
 *      cost.  The table (out->regions) holds the first max_regions kept regions in ascending label; a record's place in it is the
 *      region's table index.
 *   5. Map.  region[p] (int32) is the table index of p's region; -1 for a cell that is no member; -2 for a member whose region is
 *      not in the table, whether it was dropped or lies past max_regions.
 *   6. Gain (gain_radius R, 0..128; 0 = not computed: every gain is 0).  For each region of the table, rays leave the
 *      representative o toward every (dx, dy) with max(|dx|, |dy|) == R: 8 R rays.  Step s = 1..R of a ray is the cell
 *      (o.x + sgn(dx) * ((2 |dx| s + R) / (2 R)), o.y + sgn(dy) * ((2 |dy| s + R) / (2 R))), integer division.  A ray ends before
 *      the first step whose cell is outside the grid or has state 100; unknown cells do not stop a ray.  gain is the number of
 *      DISTINCT cells of state -1 visited by the region's rays.
 *   7. Order.  order[0 .. regions_written) holds the table indices sorted ascending by
 *      key = (int64)rep_cost * cost_weight - (int64)gain * gain_weight - (int64)cells * size_weight; every region with
 *      rep_cost == 0xFFFFFFFF comes after all others; ties go to the smaller label.  The weights are 0..1 << 20, so no key can
 *      wrap.  Computed on the host from the table with a total order: deterministic.
 *   8. Stats (exact): frontier_cells = the members; regions_found = the regions of step 2; regions_small = those with
 *      cells < min_cells; regions_unreached = those with cells >= min_cells that reachable_only dropped; regions_kept (found =
 *      small + unreached + kept); regions_written = min(regions_kept, max_regions); largest_cells over the regions found (0 if
 *      none); gain_rays = 8 R * regions_written.  Informative only: merge_pairs = the pairs of members that the cross-tile merge
 *      looked at.
 *
 * Defaults (ssf_navfrontier_default_params) are design choices, not tuned values: width = height = 512 (the grid's default size),
 * connectivity 8, min_cells 1, max_regions 4096, gain_radius 0, cost_weight 1, gain_weight 0, size_weight 0 (the cheapest region
 * first); traversable_only, min_dist2, reachable_only and on_device 0.
 *
 * Refused with SSF_ERR_INVALID_ARG: h, p or state NULL; `out` NULL or every output NULL; width or height outside 1..4096;
 * connectivity neither 4 nor 8; min_dist2 < 0; min_cells < 1; max_regions outside 1..65536; gain_radius outside 0..128; a weight
 * outside 0..1 << 20; traversable_only with dist2 NULL; reachable_only with cost NULL.  With SSF_ERR_STATE: frames pending in the
 * extract pipeline; a sharded handle (cfg.nranks > 1).  After any refusal the handle keeps working.
 *
 * on_device governs state, dist2, cost and the region map; the table (regions) and order are HOST memory always, max_regions
 * records each (at most 65536), as goals and starts are in the plan.  Records and entries past regions_written are not written.
 * The call is synchronous on the handle's stream and changes no state of the handle: made between two frames it changes no later
 * pose or model bit.  Working buffers are allocated on first use and grown as a whole; a growth that fails returns SSF_ERR_DEVICE
 * and leaves the handle working.  Kernels appear in ssf_get_kernel_times under profile = 1 (navfrontier_label, navfrontier_merge,
 * navfrontier_flatten, navfrontier_sums, navfrontier_table, navfrontier_map, navfrontier_gain).
 *
 * Who exports these functions: libssf_hip_explore.so, which is libssf_hip_nav.so's objects (the product, the carve, the plan) with
 * this call linked in, so that a robot that builds, carves, plans and explores loads one library.  None of libssf_hip.so,
 * libssf_hip_navcarve.so and libssf_hip_nav.so does: their exported symbols are what they were.  A caller links or loads
 * libssf_hip_explore.so INSTEAD of the others, never next to them: a handle belongs to the library that created it.  The ABI
 * version of ssf.h is unchanged.
 */
#ifndef SSF_NAVFRONTIER_H
#define SSF_NAVFRONTIER_H

#include "ssf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SSF_NAVFRONTIER_UNREACHED 0xFFFFFFFFu
#define SSF_NAVFRONTIER_NO_MEMBER (-1)    /* region[p] of a cell that is no member */
#define SSF_NAVFRONTIER_DROPPED   (-2)    /* region[p] of a member whose region is not in the table */

typedef struct ssf_navfrontier_params {
    int   width, height;              /* cells along grid x / grid y, 1..4096 each */
    int   connectivity;               /* 8 or 4 */
    int   traversable_only;           /* 1: a member has dist2 >= min_dist2 as well */
    int   min_dist2;                  /* the robot's squared radius in cells, >= 0 */
    int   min_cells;                  /* a kept region has at least this many cells, >= 1 */
    int   reachable_only;             /* 1: a kept region has a member of cost != 0xFFFFFFFF */
    int   max_regions;                /* records of the table, 1..65536 */
    int   gain_radius;                /* R of step 6, 0..128; 0 = no gain */
    int   cost_weight, gain_weight, size_weight;      /* step 7, 0..1 << 20 each */
    int   on_device;                  /* 1: state, dist2, cost and region are device pointers */
} ssf_navfrontier_params;

typedef struct ssf_navfrontier_region {
    int64_t  sum_x, sum_y;            /* the sums of the cells' ix, iy */
    int32_t  label;                   /* the smallest p of the region */
    int32_t  cells;
    int32_t  x0, y0, x1, y1;          /* the bounding box, inclusive */
    int32_t  rep_x, rep_y;            /* the representative */
    uint32_t rep_cost;                /* its cost; 0xFFFFFFFF = none reached */
    int32_t  gain;                    /* distinct unknown cells its rays visit; 0 with gain_radius 0 */
} ssf_navfrontier_region;

typedef struct ssf_navfrontier_out {  /* any may be NULL, not all */
    int32_t* region;                  /* height x width: table index, -1 no member, -2 not in the table */
    ssf_navfrontier_region* regions;  /* max_regions records; HOST memory always */
    int32_t* order;                   /* max_regions table indices; HOST memory always */
} ssf_navfrontier_out;

typedef struct ssf_navfrontier_stats {
    int64_t frontier_cells;
    int64_t regions_found, regions_small, regions_unreached, regions_kept, regions_written;
    int64_t largest_cells;
    int64_t gain_rays;
    int64_t merge_pairs;              /* informative */
} ssf_navfrontier_stats;

int ssf_navfrontier_default_params(const ssf_handle* h, ssf_navfrontier_params* p);
int ssf_navfrontier_regions(ssf_handle* h, const ssf_navfrontier_params* p, const int8_t* state, const int32_t* dist2, const uint32_t* cost,
                            const ssf_navfrontier_out* out, ssf_navfrontier_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* SSF_NAVFRONTIER_H */
