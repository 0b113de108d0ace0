/*
 * ssf_navdyn.h -- steering among moving obstacles, on the device: the rollouts of ssf_navsteer.h and ssf_navfoot.h refused where they
 * meet a PREDICTED MOVER and scored by the gap they keep, and the moving pixels of a depth frame turned into grid-frame blobs from
 * which a small host tracker makes those movers.
 *
 * Every other call of the navigation chain treats the world as frozen at the instant of the call.  The library detects moving things
 * (ssf_motion.h, ssf_dynamic.h) only to keep them out of the map; downstream a walking person is either stamped as a wall where they
 * are now (ssf_navlive_overlay, mask_mode 0: the rollouts brush past the place they just left and drive into the place they will be
 * by step 10) or is invisible to the whole chain (mask_mode 2).  The rollouts already advance in discrete steps, and a step index is a
 * time: testing a step against where an obstacle will be THEN is a short loop that is the same for every lane.
 *
 * All arithmetic of the rollouts is integer and the rule has exactly one answer, so no result depends on the order the hardware works
 * in, and a small restatement (tests/navdyn_ref.py, Python ints and math.isqrt) reproduces every output bit for bit.
 *
 * A. The rollouts with movers (ssf_navdyn_rollouts for the disc, ssf_navdyn_foot_rollouts for the oriented footprint).
 *   Everything of ssf_navsteer.h steps 1 to 9 holds word for word -- units, direction table, lattice, traversable, corner rule,
 *   admissible, winner, outputs, stats -- and for the footprint everything of ssf_navfoot.h step 3.  The additions:
 *   1. Movers.  movers: n_movers x 6 int32 (x, y, vx, vy, r, grow): position and radius in sub-units (1024 per cell), velocity and
 *      growth in sub-units per step.  One list serves all poses of a call.  It may be NULL iff n_movers == 0.  At step s (1-based: the
 *      step being attempted) mover m is the disc with centre (X_s, Y_s) = (x + s * vx, y + s * vy) and radius R_s = r + s * grow.
 *      The caller puts the robot's own radius (for the footprint its circumscribed radius) into r; grow is the prediction's
 *      uncertainty.
 *   2. Step.  A step to (nx, ny) is FREE iff it is free by ssf_navsteer.h step 4 (for the footprint: by ssf_navfoot.h step 3) AND
 *      every mover has D2 >= R_s * R_s, D2 = (nx - X_s)^2 + (ny - Y_s)^2, all in int64.  The static test comes first.  cand_hit is
 *      the smallest m with D2 < R_s * R_s at the step that ended the rollout; it is -1 where the rollout ran all its steps, ended on
 *      the static test or left the grid, or where the start is not traversable.
 *      The start (s = 0) is NOT tested against the movers: a mover on top of the robot refuses nothing by itself, so that the robot
 *      may still drive away from it.  (Its first step is tested like any other: it must leave the mover's disc of step 1.)
 *   3. Gap.  For every committed step and every mover g = isqrt(D2) - R_s, isqrt the floor square root; g >= 0 by step 2.
 *      min_gap = min(mover_cap, every g); it equals mover_cap with no mover or no committed step.  cand_min_gap is -1 where the
 *      start is not traversable.
 *   4. Score.  score (ssf_navsteer.h step 6) gains + mover_weight * ((10 * (mover_cap - min_gap)) >> 10): the field's unit of 10 per
 *      cell, like the target term.  "Not all weights 0" counts six weights.
 *      The winner's key (score << 16) | c still fits 64 bits: cost_weight * cost < 1000 * 2^32 < 2^42; the target term is at most
 *      1000 * ((14 * 2^32) >> 10) < 2^36; the clearance term at most 1000 * 2^20 < 2^30; speed and turn at most 1000 * 1024 and
 *      1000 * 16384 < 2^24; the mover term at most 1000 * ((10 * 65536) >> 10) = 640000 < 2^20.  The sum is below 2^43 < 2^48.
 *   5. Outputs.  ssf_navdyn_out: cand_hit and cand_min_gap (n_poses x K each) and best_min_gap (n_poses: the winner's min_gap, -1 if
 *      there is no winner).  Each may be NULL; "every output NULL" is judged over ssf_navsteer_out and ssf_navdyn_out together, and
 *      `out` (the ssf_navsteer_out) may itself be NULL when a ssf_navdyn_out output is given.
 *   6. Stats.  ssf_navdyn_stats.hit_movers: exactly the candidates with cand_hit >= 0.  ssf_navsteer_stats.collided keeps its meaning
 *      (free_steps < n_steps) and so includes them.
 *   7. Bounds.  With |x|, |y| <= 2^24, |vx|, |vy| <= 4096, s <= 256: |X_s| <= 2^24 + 2^20.  A step that reaches the mover test lies in
 *      the grid, 0 <= nx < 4096 * 1024 = 2^22, so |nx - X_s| < 2^24 + 2^20 + 2^22 < 2^25 and D2 < 2 * 2^50 = 2^51 < 2^53: D2 is
 *      exact in int64 and in f64.  R_s <= 2^20 + 256 * 4096 = 2^21, so R_s^2 <= 2^42 < 2^43.  The gap's comparison uses
 *      k = min_gap + R_s <= 2^16 + 2^21 < 2^22, k^2 < 2^44.  isqrt: the f64 square root of an exact D2 < 2^53 is within 2^-26 of
 *      the true root (below 2^26.5), so its truncation is the floor or one off; one integer comparison each way makes it exact.
 *   8. Identity.  With n_movers == 0 and mover_weight == 0 every output and stat that ssf_navsteer_rollouts / ssf_navfoot_rollouts
 *      also produce equals theirs.
 *
 * B. Blobs of the moving pixels (ssf_navdyn_blobs).  depth in the handle's input format, mask (uint8) and label (int32) exactly as
 *   ssf_motion_mask / ssf_motion_segment write them, all cam_height x cam_width.  The params carry the grid frame, the camera, the
 *   band and the depth range exactly as ssf_navlive_params does, with the same defaults and the same refusals for those fields.
 *   1. A pixel is a MEMBER iff mask[p] != 0 and 0 <= label[p] < cam_width * cam_height (ssf_motion.h writes -1 or a pixel index).
 *      A member CONTRIBUTES iff its depth is VALID (ssf_navlive.h step 1) and its point is an OBSTACLE POINT of a grid cell
 *      (ssf_navlive.h step 2: the same f32 operations in the same order).
 *   2. Position.  With gx = C.x / res, gy = C.y / res (ssf_navgrid.h step 4): bx = (int)(gx * 1024.0f), by likewise; the product is
 *      a scaling by a power of two, exact, and 0 <= bx < width * 1024.
 *   3. Per label: n, sum_x, sum_y (int64) and the minimum and maximum of bx and of by over its contributing pixels.  All are integer
 *      sums, minima and maxima: no arrival order shows.
 *   4. A label is KEPT iff n >= min_points.  For a kept label cx = sum_x / n, cy = sum_y / n (the operands are >= 0: a floor);
 *      ex = max(cx - min_x, max_x - cx), ey likewise; r = the smallest integer with r * r >= ex * ex + ey * ey.
 *   5. The kept blobs in the order (-n, label); the first max_blobs are written as rows of SSF_NAVDYN_BLOB_WORDS = 8 int32:
 *      (label, n, cx, cy, r, ex, ey, 0).  Rows past blobs_written are not written.
 *   6. Stats, all exact: pixels_member; pixels_valid (members of valid depth); points_in_band (contributing pixels); labels_seen
 *      (labels with n >= 1); blobs_kept; blobs_written = min(blobs_kept, max_blobs).
 *
 * C. From two blob tables to movers: a tracker on the host, integer only (ssf.hpp's supersurfel_fusion::MoverTracker and binding.MoverTracker state
 *   the same rule; the ABI has no entry point for it).  update(blobs, steps_since >= 1) walks the new table in order; a new blob
 *   matches the not-yet-matched blob of the previous table with the smallest (squared centre distance, previous index) among those
 *   with squared centre distance <= gate * gate; vx = floor((cx - pcx) / steps_since), vy likewise; r_out = r + inflate; grow_out =
 *   grow if matched, else grow_unmatched with zero velocity.  It returns n x 6 int32 (cx, cy, vx, vy, r_out, grow_out), each clamped
 *   to the bounds below, and keeps the new table.
 *
 * Defaults are design choices, not tuned values.  ssf_navdyn_default_params: n_movers 0, mover_cap 4096 (four cells), mover_weight 1.
 * ssf_navdyn_default_blob_params: the fields shared with ssf_navlive_params as ssf_navlive_default_params sets them, min_points 16,
 * max_blobs 64, direct 0, on_device and frame_on_device 0.
 *
 * Refused with SSF_ERR_INVALID_ARG, by the rollouts: dp NULL; n_movers outside 0..64; movers NULL with n_movers > 0 or not NULL with
 * n_movers == 0; mover_cap outside 0..65536; mover_weight outside 0..1000; and, of a HOST list, |x| or |y| > 1 << 24, |vx| or |vy| >
 * 4096, r outside 0..1 << 20, grow outside 0..4096; and everything ssf_navsteer_rollouts / ssf_navfoot_rollouts refuse, with the two
 * changes of steps 4 and 5.  A DEVICE list (on_device = 1) is not read by the host: its values are the caller's responsibility.
 * Out-of-range values there change what is computed, never what is touched: they enter arithmetic only (unsigned, of 32 and 64 bits,
 * which wraps), never an address.
 * By ssf_navdyn_blobs: h, p, depth, mask, label or blobs NULL; what ssf_navlive_overlay refuses for width, height, res, floor_max,
 * z_max, the camera, t_min and t_max; min_points < 1; max_blobs outside 1..64; direct not 0 or 1; a device depth pointer not aligned
 * for the input format.  With SSF_ERR_STATE: frames pending in the extract pipeline; a sharded handle.  After any refusal the handle
 * keeps working.
 *
 * on_device governs, for the rollouts, movers and the three outputs like every other array of the call; for the blobs it governs
 * `blobs`.  frame_on_device governs depth, mask and label: ssf_motion_mask's device outputs are read where they lie, so that no
 * image leaves the device.  The order of step B.5 is made on the host from the compact per-label table (at most one record per
 * label), as the frontier regions' is.  All calls are synchronous on the handle's stream and change no state of the handle: a call
 * between two frames changes no later pose or model bit.  Working buffers are allocated on first use and grown as a whole; a growth
 * that fails returns SSF_ERR_DEVICE and leaves the handle working.  Kernels appear in ssf_get_kernel_times under profile = 1:
 * navdyn_pack, navdyn_roll, navdyn_pick; navdyn_blob_seen, navdyn_blob_slots, navdyn_blob_sum.
 *
 * Who exports these functions: libssf_hip_dyn.so, which is libssf_hip_pose.so's objects with this file's linked in.  None of the
 * nine older libraries does: their exported symbols are what they were.  A caller links or loads libssf_hip_dyn.so INSTEAD of the
 * others, never next to them: a handle belongs to the library that created it.  The ABI version of ssf.h is unchanged.
 */
#ifndef SSF_NAVDYN_H
#define SSF_NAVDYN_H

#include "ssf.h"
#include "ssf_navsteer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SSF_NAVDYN_MAX_MOVERS  64
#define SSF_NAVDYN_MOVER_WORDS 6              /* (x, y, vx, vy, r, grow) */
#define SSF_NAVDYN_MAX_BLOBS   64
#define SSF_NAVDYN_BLOB_WORDS  8              /* (label, n, cx, cy, r, ex, ey, 0) */

typedef struct ssf_navdyn_params {
    int   n_movers;                   /* 0..64 */
    int   mover_cap;                  /* min_gap = min(mover_cap, every gap), sub-units, 0..65536 */
    int   mover_weight;               /* 0..1000; the sixth weight of the score */
} ssf_navdyn_params;

typedef struct ssf_navdyn_out {       /* any may be NULL */
    int32_t* cand_hit;                /* n_poses x K: the mover that ended the rollout, -1 if none did */
    int32_t* cand_min_gap;            /* n_poses x K: -1 where the start is not traversable */
    int32_t* best_min_gap;            /* n_poses: the winner's, -1 if there is no winner */
} ssf_navdyn_out;

typedef struct ssf_navdyn_stats {
    int64_t hit_movers;               /* candidates with cand_hit >= 0 */
} ssf_navdyn_stats;

typedef struct ssf_navdyn_blob_params {
    const float* grid_pose;           /* as ssf_navlive_params: 12 floats grid-to-map, NULL = ssf_navgrid_default_pose now */
    int   width, height;              /* 1..4096 each */
    float res;                        /* metres per cell */
    float floor_max, z_max;           /* the obstacle band: floor_max < z <= z_max */
    const float* cam_pose;            /* 12 floats camera-to-map; NULL = the handle's pose */
    float fx, fy, cx, cy;             /* pinhole of the depth frame; */
    int   cam_width, cam_height;      /* cam_width == 0: all six from the handle's cfg */
    float t_min, t_max;               /* valid depths, metres; both 0 = cfg.range_min / cfg.range_max */
    int   min_points;                 /* a kept label has at least this many contributing pixels, >= 1 */
    int   max_blobs;                  /* rows of `blobs`, 1..64 */
    int   direct;                     /* 0: a tile's pixels are merged per label in LDS before the global atomics; 1: every pixel adds to
                                         the table itself.  The outputs are the same either way: a measuring knob */
    int   on_device;                  /* 1: blobs is a device pointer */
    int   frame_on_device;            /* 1: depth, mask and label are device pointers */
} ssf_navdyn_blob_params;

typedef struct ssf_navdyn_blob_stats {
    int64_t pixels_member, pixels_valid, points_in_band;
    int64_t labels_seen, blobs_kept, blobs_written;
} ssf_navdyn_blob_stats;

int ssf_navdyn_default_params(const ssf_handle* h, ssf_navdyn_params* dp);
int ssf_navdyn_rollouts(ssf_handle* h, const ssf_navsteer_params* p, const ssf_navdyn_params* dp, const int8_t* state, const int32_t* dist2,
                        const uint32_t* cost, const int32_t* poses, const int32_t* targets, const int32_t* movers, const ssf_navsteer_out* out,
                        const ssf_navdyn_out* dout, ssf_navsteer_stats* stats, ssf_navdyn_stats* dstats);
int ssf_navdyn_foot_rollouts(ssf_handle* h, const ssf_navsteer_params* p, const ssf_navdyn_params* dp, int n_headings, const uint32_t* free_mask,
                             const int32_t* dist2, const uint32_t* cost, const int32_t* poses, const int32_t* targets, const int32_t* movers,
                             const ssf_navsteer_out* out, const ssf_navdyn_out* dout, ssf_navsteer_stats* stats, ssf_navdyn_stats* dstats);
int ssf_navdyn_default_blob_params(const ssf_handle* h, ssf_navdyn_blob_params* p);
int ssf_navdyn_blobs(ssf_handle* h, const ssf_navdyn_blob_params* p, const void* depth, const uint8_t* mask, const int32_t* label, int32_t* blobs,
                     ssf_navdyn_blob_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* SSF_NAVDYN_H */
