/*
 * ssf_query.h -- rows of the fused model selected on the device: by region, age and confidence.
 *
 * A consumer that wants a PART of the map (the rows around the camera for a planner, the confident rows for markers, "the rows
 * last seen before stamp t" after a loop closure) would otherwise copy the whole model out (ssf_get_model: 104 B per row) and
 * filter it on the host.  ssf_query_rows selects where the rows live and hands back the selected rows only; ssf_query_count
 * only counts them.
 *
 * What is selected: rows of the model as it stands after the last completed frame (or ssf_set_model / ssf_apply_deformation).
 * Every step below is one IEEE f32 operation, in the order written (the library builds with -ffp-contract=off and correctly
 * rounded division), so a numpy f32 restatement reproduces the selection bit for bit (tests/query_ref.py).  Every parameter is
 * cast to f32 first.
 *   1. A row qualifies iff it is live (with visible_only: a visible row), its position c is finite in all three components,
 *      conf > min_conf (strict, as exportModel's conf_thresh and ssf_render_model), t_init_min <= stamps.x <= t_init_max,
 *      t_last_min <= stamps.y <= t_last_max, and the region test passes.
 *   2. Pose (R, t): frame-to-map, 12 floats as ssf_get_pose (R row-major, then t).  d = c - t and C = R^T d with
 *      C_j = (R0j d.x + R1j d.y) + R2j d.z (ssf_render.h step 1).
 *   3. SSF_REGION_ALL: every row.
 *      SSF_REGION_SPHERE: r2 = (d.x d.x + d.y d.y) + d.z d.z; inside iff r2 <= radius * radius.  Only t of the pose is used.
 *      SSF_REGION_BOX: inside iff fabsf(C.x) <= half[0] && fabsf(C.y) <= half[1] && fabsf(C.z) <= half[2] (the pose is the
 *        box's frame).
 *      SSF_REGION_FRUSTUM: z = C.z with z_min <= z <= z_max; u = (fx * C.x) / z + cx, v = (fy * C.y) / z + cy; inside iff
 *        u >= -0.5f && u < (float)width - 0.5f && v >= -0.5f && v < (float)height - 0.5f (the pose is the camera's).  This is a
 *        POINT test of the row's centre: a disc whose centre projects outside the image is not selected even where the disc
 *        reaches into it.  It is not filterModel's classification of a row as visible (which also looks at the normal and
 *        at the row's stamps), and visible_only does not make it one.
 *   4. Output order is logical order: ssf_get_model's [visible | out-of-view].  out_index[j] = the logical index of output row
 *      j; the arrays of `out` hold bit copies of what ssf_get_model returns for those indices (orientations packed as
 *      row-major Mat33).  Any NULL array of `out` is skipped and not read from the store either; out_index may be NULL; out
 *      may be NULL if out_index is not.
 *   5. Stats (exact): n_scanned = the live rows looked at (n_model, or n_visible with visible_only); n_selected;
 *      n_selected_visible = the selected rows whose logical index is < n_visible; lo / hi = the minimum / maximum per axis of
 *      the selected positions, where -0 counts as +0 (x + 0.0f before the comparison: the result depends on no order); all 0
 *      when nothing is selected.
 *
 * Defaults (ssf_query_default_params): min_conf 0, both stamp ranges INT32_MIN..INT32_MAX, SSF_REGION_ALL, everything else 0 /
 * NULL.  pose NULL = the handle's pose; width 0 = the handle's camera (width, height, fx, fy, cx, cy); z_min = z_max = 0 =
 * cfg.range_min / cfg.range_max.
 *
 * n_selected > capacity: SSF_ERR_CAPACITY, *stats is filled (the caller can size its buffers) and nothing is written to the
 * outputs.  Refused with SSF_ERR_INVALID_ARG: a NULL handle or params; both outputs NULL (every array of `out` NULL counts as
 * NULL) in ssf_query_rows, NULL stats in ssf_query_count; a negative capacity; an unknown region; a radius or half extent that is
 * negative or not finite; a frustum size outside 1..4096, fx or fy zero or not finite, z_min <= 0 or z_max <= z_min (after the
 * defaults); t_init_min > t_init_max or t_last_min > t_last_max -- every parameter is checked, whatever the region (start from
 * ssf_query_default_params: its values pass).  With SSF_ERR_STATE: frames
 * pending in the extract pipeline; a sharded handle (cfg.nranks > 1) -- deliberately not part of this interface: a shard would
 * answer for its own rows only, in an order that means nothing to the caller.
 *
 * The calls are synchronous and run on the handle's stream.  They change no state of the handle: a query between two frames
 * changes no later pose or model bit.  Working buffers are allocated on first use and grown as a whole; a growth that fails
 * returns SSF_ERR_DEVICE and leaves the handle working.  With on_device the outputs of ssf_query_rows are device pointers,
 * otherwise host memory (the selected rows are copied, not `capacity` rows).  Kernels appear in ssf_get_kernel_times under
 * profile = 1 (query_select, query_scan, query_gather).
 *
 * Only the HIP product library (libssf_hip.so) exports these functions; the ABI version of ssf.h is unchanged.
 */
#ifndef SSF_QUERY_H
#define SSF_QUERY_H

#include "ssf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { SSF_REGION_ALL = 0, SSF_REGION_SPHERE = 1, SSF_REGION_BOX = 2, SSF_REGION_FRUSTUM = 3 } ssf_region_kind;

typedef struct ssf_query_params {
    float   min_conf;                 /* rows with conf > min_conf (strict, as exportModel / ssf_render_model) */
    int32_t t_init_min, t_init_max;   /* stamps.x in [min, max] */
    int32_t t_last_min, t_last_max;   /* stamps.y in [min, max] */
    int     visible_only;             /* 1: the visible rows only */
    int     region;                   /* ssf_region_kind */
    const float* pose;                /* 12 floats, frame-to-map (ssf_get_pose layout): the box's frame / the frustum's camera;
                                         NULL = the handle's pose.  SPHERE: only t is used (the centre) */
    float   radius;                   /* SPHERE */
    float   half[3];                  /* BOX: half extents along the frame's axes */
    int     width, height;            /* FRUSTUM; width 0 = the handle's camera and intrinsics */
    float   fx, fy, cx, cy;
    float   z_min, z_max;             /* FRUSTUM; both 0 = cfg.range_min / cfg.range_max */
    int     on_device;                /* 1: the outputs of ssf_query_rows are device pointers */
} ssf_query_params;

typedef struct ssf_query_stats {
    int64_t n_scanned;                /* live rows looked at (n_model, or n_visible with visible_only) */
    int64_t n_selected;
    int64_t n_selected_visible;       /* of those, logical index < n_visible */
    float   lo[3], hi[3];             /* bounding box of the selected positions; all 0 when n_selected == 0 */
} ssf_query_stats;

int ssf_query_default_params(const ssf_handle* h, ssf_query_params* p);
int ssf_query_count(ssf_handle* h, const ssf_query_params* p, ssf_query_stats* stats);
int ssf_query_rows(ssf_handle* h, const ssf_query_params* p, ssf_surfels* out, int32_t* out_index, int capacity,
                   ssf_query_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* SSF_QUERY_H */
