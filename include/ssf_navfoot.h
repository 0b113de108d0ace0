/*
 * ssf_navfoot.h -- an oriented robot footprint on the navigation grid, on the device: per cell a bit mask of the headings at which a
 * rectangular body centred there stands on clear cells only (the heading layers), and the rollouts of ssf_navsteer.h walked over
 * that mask instead of the disc's test, so that an arc is refused where the body, at the headings it sweeps, does not fit.
 *
 * Every call of the chain before this one models the robot as a disc: traversable means dist2 >= min_dist2.  A 0.6 m x 0.4 m base in
 * a 0.5 m corridor cannot enter by its circumscribed radius, and by its inscribed radius turns on the spot into the wall.  The
 * standard answer is a global plan by the inscribed radius (ssf_navplan_field as it is) and a local planner that tests the oriented
 * footprint: the two calls here.  Without them a caller copies state out and dilates it per heading on the host at control rate.
 * Where that global plan is wrong for a long body (a bend it cannot turn, a corridor it drives through lengthwise), ssf_navpose.h plans
 * over (x, y, heading) on the layers made here, and its cell_cost is the rollouts' `cost`.
 *
 * All arithmetic is integer and the rule has exactly one answer, so the result does not depend on the order the hardware works in,
 * and a small restatement (tests/navfoot_ref.py) reproduces every output bit for bit.
 *   Units are ssf_navsteer.h's: 1024 sub-units per cell, 65536 heading units per turn, the direction table C[k], S[k] of 1024 entries
 *      (ssf_navsteer_direction_table).  Heading grows toward +iy.  In the robot's frame x is forward and +y is left.
 *   Heading bins.  n_headings = B in {1, 2, 4, 8, 16, 32}; shift = 16 - log2 B; half = 1 << (shift - 1).  Bin b stands for heading
 *      b * 65536 / B, which is direction index k_b = b * (1024 / B).  The bin of a heading h in 0..65535 is
 *      ((h + half) >> shift) & (B - 1).
 *   1. The footprint's cells (ssf_navfoot_spans; it takes no handle and touches no device).  The footprint is a rectangle: front,
 *      back, left, right in sub-units from the robot's centre, each 0..24576; pad, 0..4096, is added to all four sides.  For bin b
 *      with (C, S) = (C[k_b], S[k_b]) the cell offset (dx, dy) is COVERED iff, in int64,
 *        u = 1024 * (dx * C + dy * S),  v = 1024 * (dy * C - dx * S)
 *        -(back + pad) * 16384 <= u <= (front + pad) * 16384   and   -(right + pad) * 16384 <= v <= (left + pad) * 16384.
 *      Offset (0, 0) is always covered.  For a fixed dy the covered dx form one interval (the four conditions are linear in dx).
 *      spans: B x 81 x 2 int16: for bin b and dy = -40..40 (row dy + 40) the pair (lo, hi) of that interval, (1, 0) where it is
 *      empty.  reach: the largest |dx| or |dy| of any covered cell.  The ranges bound it by sqrt(2) * 28 = 39.6 cells <=
 *      SSF_NAVFOOT_MAX_REACH = 40; a footprint of larger reach is refused.  kernel_cells: the covered cells summed over the bins.
 *      Why pad: the layers are sampled at the cell a pose lies in and at the bin its heading lies in.  A caller who wants them
 *      conservative for any position in the cell and any heading in the bin passes pad >= ceil(2 * 724.1 + rho * pi / B), rho the
 *      distance of the farthest corner in sub-units: half a cell's diagonal for the position, half again for "the square overlaps"
 *      against "the centre is inside", and the arc of half a bin.  The wrappers compute this; the ABI takes pad as given, and 0 is
 *      allowed.
 *   2. The layers (ssf_navfoot_layers).  state: int8, height x width, row-major, exactly as the grid calls or ssf_navlive_overlay
 *      write it.  clear[p] = state[p] == 0 || (allow_unknown && state[p] == -1); any other state is not clear; cells outside the
 *      grid are not clear.  dist2 is not read.  free_mask (uint32, height x width): bit b is set iff every cell p + (dx, dy)
 *      covered in bin b is clear; bits >= B are 0.  n_free (uint8, optional): its popcount.
 *      Stats, all exact: cells_clear; cells_all (all B bits set), cells_some (some, not all), cells_none (mask 0: cells_all +
 *      cells_some + cells_none = width * height); reach; kernel_cells.
 *   3. The rollouts (ssf_navfoot_rollouts).  ssf_navsteer.h with its step 3 and the tests of step 4 replaced, and nothing else:
 *      steps 5 to 9 (admissible, score, winner, outputs, stats) carry over word for word, and so do the params, the outputs and
 *      the stats structs.  state is not an argument; allow_unknown is validated as there and not read: the mask carries it.
 *        Traversable under a set of bins `need` (a bit mask): (free_mask[p] & need) == need && dist2[p] >= min_dist2.  Cells outside
 *        the grid are not.  d(p) = min(max(dist2[p], 0), clearance_cap) as before.
 *        Start.  need is the one bit of the start heading's bin.  pose_status 2 reads "the start cell does not hold the footprint at
 *        the start heading".
 *        A step from heading h with turn w: a = h + half; lo = min(a, a + w) >> shift, hi = max(a, a + w) >> shift (floor shifts;
 *        a + w may be negative or pass 65535); need = the OR of 1 << (u & (B - 1)) for u = lo..hi: the bins the heading sweeps in
 *        this step, at most B / 4 + 2 of them because |w| <= 16384.  The step is FREE iff the new cell is traversable under need and,
 *        when both coordinates of the cell change, the two axial cells are traversable under the same need.  With v = 0 a step
 *        re-tests the cell it stands in: turning on the spot is refused where the body does not fit.
 *      windows_staged is 0 and windows_global counts the workgroups of poses whose start holds: the rollouts walk a packed
 *      (mask, d) word of 8 bytes a cell in global memory.
 *
 * Defaults (ssf_navfoot_default_params): width = height = 512, n_headings 16, every other field 0: a caller sets the footprint.
 *
 * Refused with SSF_ERR_INVALID_ARG: by ssf_navfoot_spans, a side outside 0..24576, pad outside 0..4096, n_headings not one of
 * 1, 2, 4, 8, 16, 32, every output NULL, a reach above 40.  By ssf_navfoot_layers: h, p, state or out NULL, free_mask and n_free
 * both NULL, width or height outside 1..4096, allow_unknown not 0 or 1, and what ssf_navfoot_spans refuses.  By
 * ssf_navfoot_rollouts: free_mask NULL, n_headings as above, and everything ssf_navsteer_rollouts refuses.  With SSF_ERR_STATE:
 * frames pending in the extract pipeline; a sharded handle (cfg.nranks > 1).  After any refusal the handle keeps working.
 *
 * on_device governs state and the outputs of the layers, and free_mask, dist2, cost, poses, targets and every output of the
 * rollouts.  Both calls are synchronous on the handle's stream and change no state of the handle: a call between two frames changes
 * no later pose or model bit.  Working buffers are allocated on first use and grown as a whole; a growth that fails returns
 * SSF_ERR_DEVICE and leaves the handle working.  The footprint's table stays on the device while the footprint and n_headings are the
 * same from call to call, so a control loop pays for the spans once.  Kernels appear in ssf_get_kernel_times under profile = 1 (navfoot_layers,
 * navfoot_pack, navfoot_roll, navfoot_pick).
 *
 * Who exports these functions: libssf_hip_foot.so, which is libssf_hip_steer.so's objects with this file's linked in.  None of the
 * seven older libraries does: their exported symbols are what they were.  A caller links or loads libssf_hip_foot.so INSTEAD of the
 * others, never next to them: a handle belongs to the library that created it.  The ABI version of ssf.h is unchanged.
 */
#ifndef SSF_NAVFOOT_H
#define SSF_NAVFOOT_H

#include "ssf.h"
#include "ssf_navsteer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SSF_NAVFOOT_MAX_REACH    40           /* cells: the largest |dx| or |dy| a footprint may cover */
#define SSF_NAVFOOT_MAX_HEADINGS 32
#define SSF_NAVFOOT_ROWS         81           /* 2 * SSF_NAVFOOT_MAX_REACH + 1: the rows of a bin's spans */
#define SSF_NAVFOOT_MAX_SIDE     24576        /* sub-units: front, back, left, right */
#define SSF_NAVFOOT_MAX_PAD      4096

typedef struct ssf_navfoot_params {
    int   width, height;              /* cells along grid x / grid y, 1..4096 each */
    int   allow_unknown;              /* 1: cells of state -1 are clear as well */
    int   n_headings;                 /* B: 1, 2, 4, 8, 16 or 32 */
    int   front, back, left, right;   /* the rectangle from the robot's centre, sub-units, 0..24576 each */
    int   pad;                        /* added to all four sides, 0..4096 */
    int   on_device;                  /* 1: state and the outputs are device pointers */
} ssf_navfoot_params;

typedef struct ssf_navfoot_out {      /* either may be NULL, not both */
    uint32_t* free_mask;              /* height x width */
    uint8_t*  n_free;                 /* height x width: the mask's popcount */
} ssf_navfoot_out;

typedef struct ssf_navfoot_stats {
    int64_t cells_clear, cells_all, cells_some, cells_none;
    int64_t reach, kernel_cells;
} ssf_navfoot_stats;

/* spans: n_headings x 81 x 2 int16; any output may be NULL, not all */
int ssf_navfoot_spans(int front, int back, int left, int right, int pad, int n_headings, int16_t* spans, int32_t* reach, int64_t* kernel_cells);
int ssf_navfoot_default_params(const ssf_handle* h, ssf_navfoot_params* p);
int ssf_navfoot_layers(ssf_handle* h, const ssf_navfoot_params* p, const int8_t* state, const ssf_navfoot_out* out, ssf_navfoot_stats* stats);
int ssf_navfoot_rollouts(ssf_handle* h, const ssf_navsteer_params* p, int n_headings, const uint32_t* free_mask, const int32_t* dist2,
                         const uint32_t* cost, const int32_t* poses, const int32_t* targets, const ssf_navsteer_out* out, ssf_navsteer_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* SSF_NAVFOOT_H */
