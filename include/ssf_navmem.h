/*
 * ssf_navmem.h -- the live layer with memory: the depth frame stamped into height slices of the obstacle band, cleared by the rays
 * that see through a slice, and aged by a tick, on the device.
 *
 * ssf_navlive_overlay (ssf_navlive.h) is stateless, and the only memory its caller can give it -- the output state fed back as the
 * next state_in -- is one-way: occupied always wins, so a person who walks across the corridor leaves a wall of occupied cells behind.
 * That header refuses to clear in 2-D for the right reason: "a ray crosses the band at one height only, and an obstacle may be lower".
 * This call slices the band by height, as a voxel layer does: a point marks the slice it lies in, a ray sample clears the slice it
 * passes through and no other, and a low box survives the rays that pass over it.
 *
 * The memory belongs to the CALLER, not the handle: the layer goes in and comes out, and the call stays a pure function of its inputs
 * like every read-out here.  The layer is three height x width u32 arrays (host or device under on_device):
 *   marks      bit k set: slice k of the cell's obstacle band holds remembered evidence;
 *   mark_tick  the tick at which a stamp last refreshed the cell, or 0;
 *   seen_tick  the tick at which the cell was last seen through, or 0.
 * layer_in may be NULL, or any of its three arrays: all zero.  Each output array of the layer may be the matching input pointer (the
 * update in place), and `state` may be state_in; any other overlap is refused.
 *
 * Every step is one IEEE f32 operation in the order written, every result an integer, so the order of pixels and rays never matters
 * and a numpy restatement reproduces every output with == (tests/navmem_ref.py).
 *   1. Steps 1 to 4 of ssf_navlive.h hold word for word: the depth, the point, who stamps, the see-through lattice, the samples of a
 *      ray and the band test of a point and of a sample.
 *   2. Slice.  A point or sample in the band has the grid-frame height z, the third component as ssf_navgrid.h step 1 forms it:
 *      z = (R[2] * dx + R[5] * dy) + R[8] * dz with d = the map-frame point - t.  slice_h = (z_max - floor_max) / (float)slices;
 *      k = min(slices - 1, (int)floorf((z - floor_max) / slice_h)): one subtraction, one division, floorf, the cast, the min.  (z >
 *      floor_max in the band, so k >= 0; z == z_max may give `slices`, which the min takes back to the top slice.)
 *   3. Evidence of the frame.  live_hits[cell] as in ssf_navlive.h.  hit_bits[cell] = the OR of bit k over the stamping obstacle points
 *      of the cell.  seen_bits[cell] = the OR of bit k over the ACCEPTED SAMPLES of all rays: every accepted sample, not only entries
 *      (OR is idempotent, and a ray may climb through several slices inside one cell).
 *   4. The layer, per cell, u32 arithmetic modulo 2^32:
 *        hb = live_hits >= min_hits ? hit_bits : 0          (min_hits gates all bits of the cell)
 *        m  = (marks_in & ~seen_bits) | hb                   (a slice hit in this frame stays marked: hit wins over seen)
 *        mt = hb ? tick : mark_tick_in
 *        if m != 0 && max_mark_age > 0 && tick - mt > max_mark_age: the cell EXPIRES, m = 0
 *        if m == 0: mt = 0
 *        st = seen_bits ? tick : seen_tick_in
 *        if st != 0 && max_seen_age > 0 && tick - st > max_seen_age: st = 0
 *      marks = m, mark_tick = mt, seen_tick = st.
 *   5. State, int8: 100 if state_in == 100 || m != 0; else 0 if state_in == 0 || (open_unknown && st != 0); else -1.  Any other value
 *      of state_in counts as unknown.  state_in is the STATIC grid of every frame (the map's, or the carve's), not an earlier output:
 *      the layer holds the live evidence and nothing else, so the map can be refreshed on its own.
 *   6. Clearance.  dist2 is step 8 of ssf_navgrid.h on that state, with max_dist_cells and unknown_is_obstacle.
 *   7. Stats, all exact: pixels_valid, pixels_stamping, points_in_band, rays, rays_carving, ray_samples as in ssf_navlive.h;
 *      cells_marked = cells with m != 0; cells_newly_marked = those with marks_in == 0; cells_cleared = cells with marks_in != 0 and
 *      (marks_in & ~seen_bits) | hb == 0; cells_expired = cells that step 4 expired; bits_cleared = the sum of
 *      popcount(marks_in & seen_bits & ~hb); cells_remembered = cells of state 100 with state_in != 100 and hb == 0 (what only the
 *      memory keeps occupied); cells_opened = cells with state_in neither 100 nor 0 and state 0; cells_free / cells_occupied /
 *      cells_unknown of the output state.  Informative only: atomics, the atomic operations the stamp and the march issued (it depends on
 *      how points and samples were merged).  pose = the grid frame used.
 *
 * Two identities:
 *   (a) with a zero layer and both ages 0, for any `slices`: state, dist2 and live_hits equal ssf_navlive_overlay's with min_seen = 1
 *       on the same inputs, bit for bit, and seen_bits != 0 exactly where its live_seen >= 1 (a cell has an entry iff it has an
 *       accepted sample);
 *   (b) with no valid pixel and both ages 0 the layer comes back unchanged, and state is state_in (foreign values at -1, cells with
 *       seen_tick_in != 0 opened under open_unknown) with the marked cells at 100.
 *
 * Any output may be NULL, but not all.  The march always runs: every array of the layer and every cell stat depends on seen_bits.
 *
 * Deliberately not in this rule: counts per slice (a slice is marked by one point of a cell that has min_hits), a hysteresis on
 * clearing (one sample clears), scrolling the layer with a grid that moves (the caller keeps grid_pose fixed, or clears the layer),
 * and sharded handles.
 *
 * Defaults (ssf_navmem_default_params) are design choices, not tuned values: slices 16 (0.08 m at the default band), max_mark_age
 * and max_seen_age 0 (never expire), tick 1; the rest are ssf_navlive_default_params'.
 *
 * Refused with SSF_ERR_INVALID_ARG: everything ssf_navlive_overlay refuses for the fields the two share (h, p, depth, state_in or
 * out NULL; every output NULL; width, height, res, max_dist_cells, min_hits, the camera, stride, hit_margin_cells, the range,
 * mask_mode and mask, the alignment of a device depth pointer, the corner bound); tick == 0; slices outside 1..32; floor_max or z_max
 * not finite, z_max <= floor_max, slice_h not finite or not > 0; an overlap other than an output of the layer on its own input or
 * state == state_in.  With SSF_ERR_STATE: frames pending in the extract pipeline; a sharded handle (cfg.nranks > 1).  After any
 * refusal the handle keeps working.
 *
 * The call is synchronous and runs on the handle's stream.  It changes no state of the handle: an update between two frames changes
 * no later pose or model bit.  on_device governs state_in, the layer and the outputs, frame_on_device governs depth and mask; the
 * two poses are host memory always.  Working buffers (per cell 15 bytes and the staged host arrays) are allocated on first use and
 * grown as a whole; a growth that fails returns SSF_ERR_DEVICE and leaves the handle working.  Kernels appear in
 * ssf_get_kernel_times under profile = 1: navmem_stamp, navmem_march, navmem_cells, then navgrid_columns and navgrid_rows.
 *
 * Who exports these functions: libssf_hip_mem.so, which is libssf_hip_dyn.so's objects with this call linked in (it exports
 * everything the dyn library does, and these).  The other ten libraries do not: their exported symbols are what they were.  A caller
 * links or loads libssf_hip_mem.so INSTEAD of them, never beside one: a handle belongs to the library that created it.  The ABI
 * version of ssf.h is unchanged.
 */
#ifndef SSF_NAVMEM_H
#define SSF_NAVMEM_H

#include "ssf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ssf_navmem_params {
    const float* grid_pose;           /* 12 floats grid-to-map; NULL = ssf_navgrid_default_pose(width, height, res) now */
    int   width, height;              /* 1..4096 each */
    float res;                        /* metres per cell */
    float floor_max, z_max;           /* the obstacle band: floor_max < z <= z_max, cut into `slices` */
    int   max_dist_cells;             /* 1..1024 */
    int   unknown_is_obstacle;        /* 1: cells of state -1 count as obstacles in dist2 */
    const float* cam_pose;            /* 12 floats camera-to-map; NULL = the handle's pose */
    float fx, fy, cx, cy;             /* pinhole of the depth frame; */
    int   cam_width, cam_height;      /* cam_width == 0: all six from the handle's cfg */
    float t_min, t_max;               /* valid depths, metres; both 0 = cfg.range_min / cfg.range_max */
    int   mask_mode;                  /* 0 no mask; 1 only pixels with mask != 0 stamp; 2 only pixels with mask == 0 stamp */
    int   min_hits;                   /* points that make a cell's hit bits count, >= 1 */
    int   stride;                     /* pixel lattice of the see-through rays, 1..64 */
    float hit_margin_cells;           /* a ray stops this many cells short of its depth, >= 0 */
    int   open_unknown;               /* 1: an unknown cell with seen_tick != 0 becomes free */
    int   slices;                     /* 1..32 */
    uint32_t tick;                    /* >= 1, the caller's and monotone (modulo 2^32) */
    uint32_t max_mark_age;            /* a mark not refreshed for more ticks than this expires; 0 = never */
    uint32_t max_seen_age;            /* likewise for seen_tick; 0 = never */
    int   on_device;                  /* 1: state_in, the layer and every output are device pointers */
    int   frame_on_device;            /* 1: depth and mask are device pointers */
} ssf_navmem_params;

typedef struct ssf_navmem_layer {     /* the caller's memory, each height x width; NULL = all zero */
    const uint32_t* marks;
    const uint32_t* mark_tick;
    const uint32_t* seen_tick;
} ssf_navmem_layer;

typedef struct ssf_navmem_out {       /* any may be NULL, not all; each height x width */
    uint32_t* marks;                  /* may be layer_in->marks itself */
    uint32_t* mark_tick;              /* may be layer_in->mark_tick itself */
    uint32_t* seen_tick;              /* may be layer_in->seen_tick itself */
    uint32_t* live_hits;
    uint32_t* hit_bits;
    uint32_t* seen_bits;
    int8_t*   state;                  /* may be state_in itself */
    int32_t*  dist2;
} ssf_navmem_out;

typedef struct ssf_navmem_stats {
    int64_t pixels_valid, pixels_stamping, points_in_band;
    int64_t rays, rays_carving, ray_samples;
    int64_t cells_marked, cells_newly_marked, cells_cleared, cells_expired, bits_cleared, cells_remembered;
    int64_t cells_opened, cells_free, cells_occupied, cells_unknown;
    int64_t atomics;                  /* informative */
    float   pose[12];                 /* the grid frame used */
} ssf_navmem_stats;

int ssf_navmem_default_params(const ssf_handle* h, ssf_navmem_params* p);
int ssf_navmem_update(ssf_handle* h, const ssf_navmem_params* p, const void* depth, const uint8_t* mask, const int8_t* state_in,
                      const ssf_navmem_layer* layer_in, const ssf_navmem_out* out, ssf_navmem_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* SSF_NAVMEM_H */
