/*
 * ssf_odometry.h -- dense RGB-D odometry on the device: the pose prior of a frame, made by the library itself.
 *
 * ssf_process_frame* track by ICP from the previous pose unless the caller hands in prior_pose.  The reference gets that prior
 * from its sparse VO (ORB features, g2o), which is NOT part of this library and stays out.  This header offers a prior of the
 * library's own instead: a dense photometric frame-to-frame alignment (the RGB-D term of DVO / ElasticFusion), coarse to fine
 * over a pyramid of intensity and depth, warping by the REFERENCE frame's depth.  The normal equations are accumulated on the
 * device as exact integer sums, the 6 x 6 step is taken by the host solvers the ICP loop already uses (ssf_solvers.hpp:
 * sym6_ldlt_solve, gn_increment, pinned against Eigen by tests/test_solvers.py).  The rule below is this library's
 * specification; a numpy restatement (tests/odometry_ref.py) reproduces every output bit for bit.
 *
 * Every f32 step is one IEEE operation in the order written (the library builds with -ffp-contract=off and correctly rounded
 * division); every parameter is an f32.  "valid depth" = finite and cfg.range_min <= d <= cfg.range_max.
 *
 * INPUT.  Colour and depth are read in the handle's input format (ssf_input.h).  Depth is the depth as given -- f32 metres, or
 * (float)((double)v * depth_scale) for uint16 -- not the bilateral-filtered one.
 *
 * INTENSITY.  Y = (77 R + 150 G + 29 B) >> 8 in integers (the weights sum to 2^8, so 0 <= Y <= 255), I = (float)Y * 2^-8: exact,
 * in [0, 1).  An alpha byte is ignored.
 *
 * PYRAMID.  Level 0 is the image: I as above, D = the depth where valid, else 0.  A pixel of the reference masked by ref_mask
 * has D = 0 at level 0 (it has no depth for this purpose; its intensity stays).  Level l + 1 has floor(W_l / 2) x floor(H_l / 2)
 * pixels; with a, b = the upper and c, d = the lower pixels of the 2 x 2 block at (2x, 2y) of level l:
 *     I = 0.25f * ((a + b) + (c + d))         D = the smallest non-zero D of the four, 0 when all four are 0 (no arithmetic)
 * Intrinsics follow the pixel-centre convention: fx_{l+1} = fx_l / 2.0f, fy likewise, cx_{l+1} = (cx_l + 0.5f) / 2.0f - 0.5f, cy
 * likewise.  The number of levels used is min(p->levels, SSF_ODO_MAX_LEVELS), lowered until the coarsest level has
 * W_l >= SSF_ODO_MIN_W and H_l >= SSF_ODO_MIN_H (at least 1).  Gradients are central differences with the index clamped at the
 * border:  gx(x, y) = 0.5f * (I(min(x + 1, W_l - 1), y) - I(max(x - 1, 0), y)),  gy likewise in y.  So |gx|, |gy| <= 0.5.
 *
 * LINEARISATION of level l at T = (R, t), which maps reference-camera points to the current camera.  For every pixel (x, y) of
 * the reference's level l with d = D(x, y) != 0, with the level's fx, fy, cx, cy:
 *   1. X = ((((float)x - cx) / fx) * d, (((float)y - cy) / fy) * d, d)
 *   2. Y = (dot3(R.row0, X) + t.x, dot3(R.row1, X) + t.y, dot3(R.row2, X) + t.z),  dot3(a, b) = (a.x b.x + a.y b.y) + a.z b.z
 *   3. rejected unless range_min <= Y.z <= range_max (a NaN is rejected)
 *   4. iz = 1.0f / Y.z;  u = ((fx * Y.x) * iz) + cx;  v = ((fy * Y.y) * iz) + cy
 *   5. rejected unless u >= 0, v >= 0, u < (float)(W_l - 1), v < (float)(H_l - 1) (all four bilinear neighbours inside; a NaN is
 *      rejected).  x0 = (int)u, y0 = (int)v, ax = u - (float)x0, ay = v - (float)y0
 *   6. for each of the CURRENT frame's I, gx, gy of level l: top = p00 + ax * (p10 - p00), bot = p01 + ax * (p11 - p01),
 *      value = top + ay * (bot - top), with p10 = the pixel at (x0 + 1, y0), p01 = the pixel at (x0, y0 + 1)
 *   7. r = I_cur - I_ref(x, y)
 *   8. rejected unless fabsf(r) <= r_max.  w = 1 when fabsf(r) <= huber, else huber / fabsf(r)
 *   9. a = gx * fx, b = gy * fy, g = (a * iz, b * iz, -((((a * Y.x) + (b * Y.y)) * iz) * iz)),
 *      J = (cross3(Y, g), g): d r / d (omega, tau) for the left increment Y <- Y + omega x Y + tau, in the (omega, tau) order of
 *      gn_increment (ssf_dbg_gn_increment).
 * The RECORD is 29 int64 words: [0..20] the upper triangle of sum w J J^T row by row ((0,0), (0,1), .., (0,5), (1,1), ..), term
 * (w * J[i]) * J[j]; [21..26] sum w J r, term (w * J[i]) * r; [27] sum w r^2, term (w * r) * r; [28] the number of pixels that
 * passed step 8.
 *
 * SUMS.  Every f32 term v is quantised on its own as q = rint((double)v * 2^S) (round to nearest even), clamped to +-2^40
 * (a NaN gives 0), and added as int64: the record does not depend on thread, wave or workgroup order and equals a sequential
 * sum (the library's standing rule).  S = SSF_ODO_S_A = 10 for [0..20], SSF_ODO_S_B = 24 for [21..26],
 * SSF_ODO_S_C = 36 for [27].  Why these: with I in [0, 1) and |gx|, |gy| <= 0.5, |r| < 1 and w <= 1.  A pixel that passes step
 * 5 has |Y.x| iz <= W_l / fx, so |g.xy| <= 0.5 fx / range_min, |g.z| <= 0.5 (W_l + H_l) / range_min, and the rotational part
 * |cross3(Y, g)| <= |Y| |g| is of the order fx whatever the depth.  For fx, fy <= 2048 and range_min >= 0.1 every |J[i]| stays
 * below 2^15, so a term of [0..20] is below 2^30 * 2^10 = 2^40, of [21..26] below 2^15 * 2^24 = 2^39, of [27] below 2^36: no
 * term reaches the clamp.  Outside those assumptions a term saturates at the clamp and never wraps.  Whatever the values, a
 * sum has at most W * H terms of magnitude <= 2^40: at 1280 x 960 (< 2^21 pixels) it stays below 2^61 and cannot overflow int64.
 *
 * LOOP.  T starts as the inverse of init (below; the identity without one), kept as a 4 x 4 f64 matrix.  From the coarsest level
 * to level 0, up to p->iters[l] times per level:
 *   1. the kernel is given T rounded to f32 entry by entry, and the record is read back; result.iters[l] counts these
 *   2. if record[28] < min_pixels[l] = max(1, (int)(min_pixel_share * (float)(W_l * H_l))): the estimate ends invalid
 *      (SSF_ODO_TOO_FEW_PIXELS)
 *   3. A[i][j] = (double)record[k] / 2^10 (symmetric), b[i] = -((double)record[21 + i] / 2^24): one division per word
 *   4. delta = sym6_ldlt_solve(A, b); a non-finite delta ends the estimate invalid (SSF_ODO_DEGENERATE);
 *      T <- gn_increment(delta) * T (mat4_lmul)
 *   5. the level ends when sqrt((d0 d0 + d1 d1) + d2 d2) < tol_rot and sqrt((d3 d3 + d4 d4) + d5 d5) < tol_trans (f64)
 * result.pixels and result.mean_sq_residual = ((double)record[27] / 2^36) / (double)record[28] (0 without pixels) are those of
 * the last record read.  The end reason of a finished loop is SSF_ODO_CONVERGED when level 0 ended by step 5, else
 * SSF_ODO_MAX_ITERATIONS.  Afterwards rel = T^-1 = (R^T, -(R^T t)) in f64, -(((R0i t0) + (R1i t1)) + (R2i t2)), each entry
 * rounded to f32 once.  The estimate is invalid (SSF_ODO_MOTION_GATE) when, in f64 on T^-1, sqrt((tx tx + ty ty) + tz tz) >
 * max_translation or sqrt(max(0, 3 - ((R00 + R11) + R22))) > max_rotation.  The latter is the chord 2 sin(angle / 2) of the
 * rotation angle -- the angle itself to 1 % up to 0.5 rad -- and needs no trigonometric function.  rel and result are written
 * whatever the verdict; a caller acts on result.valid.
 *
 * DEFAULTS (ssf_odometry_default_params: levels 4, iters {4, 6, 8, 10, 10, 10} for levels 0.., r_max 0.5, huber 0.2,
 * min_pixel_share 0.05, tol_rot 1e-4, tol_trans 1e-4, max_translation 0.3, max_rotation 0.35) are DESIGN CHOICES, not tuned values.
 *
 * ssf_odometry_set_reference  builds the pyramid of a frame and keeps it resident as the reference, together with the handle's
 *                             pose at that moment.  ref_mask (nullable): H x W u8, non-zero = ignore the pixel; host memory, or
 *                             device memory with on_device.
 * ssf_odometry_linearise      one record of level `level` at T12 (ssf_get_pose's 12-float layout: R row-major, then t) of the
 *                             CURRENT pyramid (the frame of the last ssf_odometry_estimate; after ssf_odometry_track or
 *                             ssf_odometry_set_reference alone there is none: SSF_ERR_STATE) against the reference.
 * ssf_odometry_estimate       builds the current frame's pyramid and runs the loop.  init12 (nullable) and rel12 are transforms
 *                             from the current camera to the reference camera in ssf_get_pose's layout.  Does not change the
 *                             reference.
 * ssf_odometry_track          ssf_odometry_estimate with init = NULL against the resident reference; when the estimate is valid,
 *                             prior12 = pose_ref o rel: R = m3_mul(R_ref, R_rel), t = m3_mulv(R_ref, t_rel) + t_ref in f32, the
 *                             operation order of ssf_dbg_m3_mul / ssf_dbg_m3_mulv (prior12 is left alone otherwise).  Then the
 *                             current pyramid becomes the reference -- a swap of buffers, not a copy -- without a mask.  Its
 *                             pose is not known yet: it is taken from the handle (ssf_get_pose) at the start of the next
 *                             ssf_odometry_track / _estimate / _linearise, i.e. it is the result of the frame processed in between.
 * ssf_process_frame_odometry  ssf_odometry_track, then the frame exactly as ssf_process_frame / _device would process it with
 *                             prior_pose = that prior -- or, with motion != NULL, as ssf_process_frame_motion would: bit-identical
 *                             to making the two calls by hand.  Without a reference (the first frame) the frame becomes the
 *                             reference, without a mask and with the pose it results in (as after a track), and is processed
 *                             with prior_pose = NULL; an invalid estimate also passes prior_pose = NULL.
 * ssf_get_odometry            rel, prior (each nullable) and result of the last ssf_odometry_track (also the one inside
 *                             ssf_process_frame_odometry); SSF_ERR_STATE before the first.  prior is 12 zeros when the estimate
 *                             was invalid.
 * ssf_odometry_get_pyramid    level `level` of the reference (which = 0) or current (which = 1) pyramid to host memory: I, D,
 *                             gx, gy (each nullable, W_l * H_l floats), the level's size and intrinsics (fx, fy, cx, cy;
 *                             nullable).  For tests and tools.
 *
 * Refused with SSF_ERR_INVALID_ARG: a NULL handle, params, image or output; level outside [0, levels used); a non-finite T12 or
 * init12; a negative or non-finite r_max, huber, min_pixel_share, tol_*, max_*; levels < 1; a negative iters[l]; a device
 * pointer not aligned for the input format.  With SSF_ERR_STATE: frames pending in the extract pipeline; a sharded handle
 * (cfg.nranks > 1); no reference (linearise, estimate, track) or no current pyramid (linearise).
 *
 * The calls are synchronous and run on the handle's stream.  Apart from the frame that ssf_process_frame_odometry itself
 * processes they change no state that a later frame result depends on.  The working buffers (about 52 bytes per pixel) are
 * allocated on first use, all or nothing: a failed allocation returns SSF_ERR_DEVICE and leaves the handle working.  Kernels
 * appear in ssf_get_kernel_times under profile = 1 as odo_pyramid and odo_linearise.  No environment variable is read.  A handle
 * that never calls these entry points launches the very kernels it launches without this header.
 *
 * Only the HIP product library (libssf_hip.so) exports these functions; the ABI version of ssf.h is unchanged.
 */
#ifndef SSF_ODOMETRY_H
#define SSF_ODOMETRY_H

#include "ssf.h"
#include "ssf_motion.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SSF_ODO_MAX_LEVELS 6
#define SSF_ODO_MIN_W 8
#define SSF_ODO_MIN_H 8
#define SSF_ODO_RECORD 29
#define SSF_ODO_S_A 10
#define SSF_ODO_S_B 24
#define SSF_ODO_S_C 36
#define SSF_ODO_CLAMP_BITS 40

typedef enum ssf_odometry_reason {
    SSF_ODO_CONVERGED = 0,
    SSF_ODO_MAX_ITERATIONS = 1,
    SSF_ODO_TOO_FEW_PIXELS = 2,
    SSF_ODO_DEGENERATE = 3,
    SSF_ODO_MOTION_GATE = 4
} ssf_odometry_reason;

typedef struct ssf_odometry_params {
    int levels;                         /* pyramid levels asked for; clamped as described above */
    int iters[SSF_ODO_MAX_LEVELS];      /* most iterations of level l (0 = the full image) */
    float r_max;                        /* hard gate on |r| (intensity in [0, 1)) */
    float huber;                        /* Huber width */
    float min_pixel_share;              /* a level needs this share of its pixels in the record */
    float tol_rot, tol_trans;           /* a level ends when |omega| and |tau| of the step fall below these */
    float max_translation;              /* motion gates on rel: metres, and the chord 2 sin(angle / 2) */
    float max_rotation;
} ssf_odometry_params;

typedef struct ssf_odometry_result {
    int valid;                          /* 1: rel may be used as a prior */
    int reason;                         /* ssf_odometry_reason */
    int levels;                         /* levels used */
    int iters[SSF_ODO_MAX_LEVELS];      /* records read per level */
    int64_t pixels;                     /* of the last record read */
    double mean_sq_residual;            /* sum w r^2 / pixels of the last record read */
} ssf_odometry_result;

int ssf_odometry_default_params(const ssf_handle* h, ssf_odometry_params* p);
int ssf_odometry_set_reference(ssf_handle* h, const void* rgb, const void* depth, int on_device, const uint8_t* ref_mask);
int ssf_odometry_linearise(ssf_handle* h, const ssf_odometry_params* p, int level, const float* T12, int64_t* record);
int ssf_odometry_estimate(ssf_handle* h, const ssf_odometry_params* p, const void* rgb, const void* depth, int on_device,
                          const float* init12, float* rel12, ssf_odometry_result* result);
int ssf_odometry_track(ssf_handle* h, const ssf_odometry_params* p, const void* rgb, const void* depth, int on_device, float* prior12,
                       ssf_odometry_result* result);
int ssf_process_frame_odometry(ssf_handle* h, const void* rgb, const void* depth, int on_device, const ssf_odometry_params* p,
                               const ssf_motion_params* motion, ssf_frame_result* out);
int ssf_get_odometry(ssf_handle* h, float* rel12, float* prior12, ssf_odometry_result* result);
int ssf_odometry_get_pyramid(ssf_handle* h, int which, int level, float* intensity, float* depth, float* gx, float* gy, int* width,
                             int* height, float* intrinsics4);

#ifdef __cplusplus
}
#endif

#endif /* SSF_ODOMETRY_H */
