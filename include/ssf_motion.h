/*
 * ssf_motion.h -- moving objects detected on the device from the incoming depth frame and the fused map.
 *
 * ssf_dynamic.h takes a per-pixel mask "from a detector"; this is a detector of the library's own.  It is purely geometric: a
 * pixel that lies clearly IN FRONT of a surface the map knows occupies space the map has seen free, so something moved there
 * (a seed).  Seeds are grown over depth-continuous pixels the map says nothing about, which gives whole-object masks in exactly
 * the form the ssf_*_pixmask calls consume -- as a device pointer, with no host round trip.  The reference's own moving-object
 * detection (optical flow and a person detector) is NOT reproduced: its source is not on hand.  The rule below is this library's
 * specification.
 *
 * Every step is one IEEE f32 operation, in the order written (the library builds with -ffp-contract=off), so a numpy f32
 * restatement (tests/motion_ref.py) reproduces every output bit for bit.  Every parameter is cast to f32 first.
 * d[p] = the incoming depth of pixel p in metres, read in the handle's input format (ssf_input.h: f32 metres, or
 * (float)((double)v * depth_scale) for uint16) -- the depth as given, not the bilateral-filtered depth.  m[p] = the model depth
 * of the same pixel, f32; 0 means the map shows nothing there.
 *   1. Valid: d is finite and cfg.range_min <= d <= cfg.range_max.
 *   2. Class:   SSF_MOTION_INVALID  d is not valid
 *               SSF_MOTION_SEED     d valid, m > 0 and (m - d) > tau, tau = front_abs + front_quad * (d * d) (strict)
 *               SSF_MOTION_UNKNOWN  d valid and m == 0
 *               SSF_MOTION_STATIC   everything else: the pixel agrees with the map or lies behind it (a surface that has
 *                                   vanished is the business of the fuse stage's free-space test, not of this detector)
 *   3. Members are the SEED and UNKNOWN pixels.  Two 4-neighbours p, q are linked iff both are members and
 *      fabsf(d[p] - d[q]) <= link_abs + link_rel * fminf(d[p], d[q]).  Equality links.  Diagonal neighbours never link.
 *   4. Components are the connected components of that graph.  A component's label is the smallest row-major pixel index in
 *      it.  Per component, n_seed and n_unknown are exact integers.
 *   5. A component is dynamic iff n_seed >= min_seeds and (int64)n_unknown <= (int64)unknown_per_seed * n_seed.  The first
 *      condition drops speckle; the second keeps a newly seen region that happens to touch a small seed blob from being
 *      swallowed.
 *   6. Outputs (each optional, NULL = not produced; at least one must be given):
 *        mask  H x W u8: 1 for the members of dynamic components, else 0
 *        label H x W i32: the component label for members, else -1
 *        cls   H x W u8: the class
 *   7. Stats (exact): n_seed, n_unknown (pixels), n_components, n_dynamic_components, pixels_masked.
 *
 * The defaults (ssf_motion_default_params: front_abs 0.05, front_quad 0.01, link_abs 0.02, link_rel 0.01, min_seeds
 * max(1, W * H / 1024), unknown_per_seed 2, min_conf 0, splat_scale 3, pose NULL) are DESIGN CHOICES, not tuned values: no
 * sequence with ground truth has been run through this detector yet.
 *
 * ssf_motion_segment       steps 1-7 on two caller images: depth in the input format, model_depth f32.  pose, min_conf and
 *                          splat_scale are ignored.  For a caller with a prediction of its own.
 * ssf_motion_mask          m = the depth image of ssf_render_model at p->pose (NULL = the handle's pose) with the handle's
 *                          camera, z_min = z_max = 0 (the configuration's range), visible_only = 0 and the given min_conf and
 *                          splat_scale; model_depth_out (nullable) returns that image.
 * ssf_process_frame_motion computes the mask at p->pose if set, else prior_pose if set, else the handle's pose, then processes
 *                          the frame exactly as ssf_process_frame_pixmask would with that mask: bit-identical to ssf_motion_mask
 *                          followed by ssf_process_frame_pixmask.  The mask never visits the host.  p->on_device is not read
 *                          (the frame's on_device holds).  On an empty model every valid pixel is UNKNOWN, so the mask is
 *                          empty and the frame is processed as without a mask.
 * ssf_get_motion_mask      the mask (H * W bytes, host memory, nullable) and stats (nullable) of the last
 *                          ssf_process_frame_motion; SSF_ERR_STATE if there has been none.
 *
 * Refused with SSF_ERR_INVALID_ARG: a NULL handle, params or depth (ssf_motion_segment: or model_depth); every output NULL; a
 * non-finite or negative front_abs, front_quad, link_abs or link_rel; min_seeds < 1; unknown_per_seed < 0; a device depth pointer
 * not aligned for the input format.  With SSF_ERR_STATE: frames pending in the extract pipeline, a sharded handle
 * (cfg.nranks > 1), as ssf_render_model.
 *
 * The calls are synchronous and run on the handle's stream.  Apart from the frame of ssf_process_frame_motion they change no
 * state that a later frame result depends on.  The working buffers (31 bytes per pixel) are allocated on first use, all or
 * nothing: a failed allocation returns SSF_ERR_DEVICE and leaves the handle working.  With on_device the images are device
 * pointers, otherwise host memory.  Kernels appear in ssf_get_kernel_times under profile = 1 (motion_classify, motion_label,
 * motion_merge, motion_flatten, motion_decide).  A handle that never calls these entry points launches the very kernels it
 * launches without this header.
 *
 * Only the HIP product library (libssf_hip.so) exports these functions; the ABI version of ssf.h is unchanged.
 */
#ifndef SSF_MOTION_H
#define SSF_MOTION_H

#include "ssf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum ssf_motion_class {
    SSF_MOTION_INVALID = 0,
    SSF_MOTION_STATIC = 1,
    SSF_MOTION_SEED = 2,
    SSF_MOTION_UNKNOWN = 3
} ssf_motion_class;

typedef struct ssf_motion_params {
    const float* pose;        /* 12 floats camera-to-map (ssf_get_pose layout) to render at; NULL = the handle's pose */
    float min_conf;           /* rows with conf > min_conf are drawn */
    float splat_scale;        /* as in ssf_render.h; 0 = 3 */
    float front_abs;          /* tau = front_abs + front_quad * (d * d), metres */
    float front_quad;
    float link_abs;           /* linked iff |d[p] - d[q]| <= link_abs + link_rel * min(d[p], d[q]) */
    float link_rel;
    int min_seeds;            /* a dynamic component has at least this many seed pixels */
    int unknown_per_seed;     /* ... and at most this many unknown pixels per seed pixel */
    int on_device;            /* 1: the images are device pointers */
} ssf_motion_params;

typedef struct ssf_motion_stats {
    int64_t n_seed;           /* pixels of class SEED */
    int64_t n_unknown;        /* pixels of class UNKNOWN */
    int64_t n_components;
    int64_t n_dynamic_components;
    int64_t pixels_masked;
} ssf_motion_stats;

int ssf_motion_default_params(const ssf_handle* h, ssf_motion_params* p);
int ssf_motion_segment(ssf_handle* h, const ssf_motion_params* p, const void* depth, const float* model_depth, uint8_t* mask,
                       int32_t* label, uint8_t* cls, ssf_motion_stats* stats);
int ssf_motion_mask(ssf_handle* h, const ssf_motion_params* p, const void* depth, uint8_t* mask, int32_t* label, uint8_t* cls,
                    float* model_depth_out, ssf_motion_stats* stats);
int ssf_process_frame_motion(ssf_handle* h, const void* rgb, const void* depth, int on_device, const float* prior_pose,
                             const ssf_motion_params* p, ssf_frame_result* out);
int ssf_get_motion_mask(ssf_handle* h, uint8_t* mask, ssf_motion_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* SSF_MOTION_H */
