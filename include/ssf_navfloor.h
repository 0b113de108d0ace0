/*
 * ssf_navfloor.h -- the floor plane of the fused model, fitted on the device: the navigation grid's own frame and bands.
 *
 * Every navigation call works in a grid frame.  With pose == NULL, ssf_navgrid.h takes the first camera for level and a metre above
 * the floor, which is right for few robots and for no hand-held start.  A caller that passes its own pose and bands has to know the
 * floor; without this call it copies the model out (ssf_get_model: 104 B per row) and fits on the host.  The map already holds what
 * is needed: every row carries a position and a normal, and the floor is the LOWEST LARGE set of rows whose normals agree and whose
 * heights agree.  The result is the `pose` and the three bands that ssf_navgrid_build, the carve and the live calls already take.
 *
 * The limit of the rule: the result is the dominant plane whose normal lies within tilt_cos of the up hint.  If the true floor tilts
 * further than that from the hint (50 degrees, say), the call finds whatever else is near the hint -- a wall, for instance.  A caller
 * whose camera is mounted that steeply passes its own `up`.
 *
 * Every device step below is one IEEE f32 operation in the order written (the library builds with -ffp-contract=off and correctly
 * rounded division and square root); everything the device accumulates is an integer count or an exact integer sum, so no result
 * depends on the order of the rows; the host steps are f64 operations in the order written.  A numpy restatement reproduces every
 * integer, histogram and float of the result with == (tests/navfloor_ref.py).  dot(v, w) below is ALWAYS the three-term form
 * (v.x w.x + v.y w.y) + v.z w.z in the precision of its arguments.
 *
 *   0. Up hint, origin, hint frame (host).
 *      u: U = (double)up; u.k = (float)(U.k / sqrt(dot(U, U))).
 *      o: `origin` (3 floats), or with NULL the handle's current camera position.  Positions are taken relative to it, so that
 *      the fixed point of step 4 stays small on long trajectories.
 *      frame(n, v) for f32 vectors n (unit) and v: N = (double)n, V = (double)v, t = dot(V, N), W.k = V.k - t * N.k,
 *      L = sqrt(dot(W, W)), X.k = W.k / L, Y = N x X = (N.y X.z - N.z X.y, N.z X.x - N.x X.z, N.x X.y - N.y X.x); the frame is
 *      ((float)X, (float)Y, n).  It does not exist when !(L > 0).
 *      Hint frame (a, b, u) = frame(u, e), e = the map axis k with the smallest fabsf(u.k), ties to the lowest k.  With the default
 *      hint (0, -1, 0) -- the map's y points down -- this is (map x, map z, -map y), the frame pose == NULL uses.
 *   1. Rows.  A row is USED iff it passes ssf_navgrid.h step 2 word for word -- live (with visible_only: a visible row), finite
 *      position c, conf > min_conf (strict), t_init_min <= stamps.x <= t_init_max, t_last_min <= stamps.y <= t_last_max, dims.x > 0
 *      and dims.y > 0 and both finite -- and its normal n (orientation row 2) is finite with every fabsf(n.k) <= 2 (a unit vector's
 *      components pass with room to spare; the bound keeps the fixed point of step 2 in range).
 *      p = c - o (per component).  s = dot(n, u).  The row is a CANDIDATE iff fabsf(s) >= tilt_cos and every fabsf(p.k) < 512.0f.
 *      m = s < 0 ? -n : n (the map's normals carry no consistent sign).
 *   2. Direction vote: a 31 x 31 histogram (u32 counts, index ib * 31 + ia) of m projected onto the hint plane.
 *      pa = dot(m, a), pb = dot(m, b).  range = sqrtf(1.0f - tilt_cos * tilt_cos), scale = 15.0f / range (host, f32).
 *      t = floorf(pa * scale + 0.5f); ia = !(t > -15.0f) ? 0 : (t >= 15.0f ? 30 : (int)t + 15) -- that is
 *      clamp((int)t + 15, 0, 30), with the clamp made before the cast; ib likewise from pb.
 *      The winner is the bin with the largest 3 x 3 window sum (the window clipped at the border), ties to the smallest
 *      ib * 31 + ia.  Without a candidate the status is SSF_NAVFLOOR_NO_FLOOR and nothing below runs.
 *      n0: over the candidates whose bin lies in the winner's window, each component of m is quantised on its own,
 *      q.k = rint((double)m.k * 1048576.0) (2^20), and summed as int64: S, with the count direction_rows.  Host:
 *      D = (double)S, n0.k = (float)(D.k / sqrt(dot(D, D))).
 *   3. Height vote: a histogram of 2048 u32 bins.  A candidate is ALIGNED iff dot(m, n0) >= align_cos.  hgt = dot(p, n0),
 *      t = floorf(hgt / height_res).  With t >= -1024.0f && t < 1024.0f the row counts in bin j = (int)t + 1024; another aligned
 *      row is counted in height_out_of_range and otherwise ignored.  W(j) = H[j - 1] + H[j] + H[j + 1] (clipped at the ends).
 *      The floor is the LOWEST large plane, so that a table top with more rows than the visible floor does not win:
 *      j0 = the smallest j with W(j) >= min_rows and W(j) * 256 >= floor_share256 * max W; j* = the bin of [j0, min(j0 + 4, 2047)]
 *      with the largest W, ties to the lowest; d0 = ((float)(j* - 1024) + 0.5f) * height_res; height_rows = W(j*).  Without such a
 *      j the status is SSF_NAVFLOOR_NO_FLOOR and no round runs.
 *   4. Refinement: refine_iters rounds.  Round k has the plane (n_k, d_k) -- n.p = d -- and its frame (a_k, b_k, n_k) =
 *      frame(n_k, a); round 0 starts from (n0, d0).  dist_0 = first_dist, dist_k = inlier_dist afterwards.
 *      A candidate is an INLIER iff dot(m, n_k) >= align_cos and fabsf(z) <= dist_k with z = dot(p, n_k) - d_k.
 *      Per inlier x = dot(p, a_k), y = dot(p, b_k) and z are quantised each on its own, q = (int64)rint((double)v * 1024.0) (2^10),
 *      and the device accumulates ten int64 words, the products taken in integers:
 *          N, Sx, Sy, Sz, Sxx, Sxy, Syy, Sxz, Syz, Szz.
 *      (|p.k| < 512 gives |q| < 2^20 and products < 2^40; a model of fewer than 2^22 rows keeps every sum below 2^62.)
 *      Host: with N < min_rows the status is NO_FLOOR; otherwise the centred moments in exact 128-bit integers,
 *          Cxx = N Sxx - Sx Sx, Cxy = N Sxy - Sx Sy, Cyy = N Syy - Sy Sy, Cxz = N Sxz - Sx Sz, Cyz = N Syz - Sy Sz, Czz = N Szz - Sz Sz,
 *      each converted to f64 once (round to nearest even), and then in f64
 *          det = Cxx * Cyy - Cxy * Cxy;                with !(det > 0) the status is SSF_NAVFLOOR_DEGENERATE;
 *          alpha = (Cxz * Cyy - Cyz * Cxy) / det;      beta = (Cyz * Cxx - Cxz * Cxy) / det;
 *          gamma = (((double)Sz - alpha * (double)Sx) - beta * (double)Sy) / (double)N;
 *          V.k = ((double)n_k.k - alpha * (double)a_k.k) - beta * (double)b_k.k;   L = sqrt(dot(V, V));
 *          n_{k+1}.k = (float)(V.k / L);               d_{k+1} = (float)(((double)d_k + gamma * 0.0009765625) / L);
 *          r = (Czz - alpha * Cxz) - beta * Cyz;  with !(r > 0): r = 0;  rms_k = (float)(sqrt(r / ((double)N * (double)N)) * 0.0009765625).
 *      A round that ends in NO_FLOOR or DEGENERATE (also: frame(n_k, a) does not exist) leaves the plane of the round before in the
 *      result and ends the refinement; its inliers and sums are still reported.  `rounds` counts the rounds that gave a new plane.
 *      A flat, exactly level set of rows gives Cxz = Cyz = 0 in integers, hence alpha = beta = 0 exactly.
 *   5. Result.  The plane (normal, d) is the last one reached: (u, 0) without a candidate, (n0, 0) without a height, (n0, d0)
 *      with refine_iters = 0 or a first round that fails, else (n_k, d_k).  origin = o.  With c = the handle's camera position,
 *      pc = c - o (f32): camera_height = (float)(dot((double)pc, (double)normal) - (double)d), the signed distance of the camera
 *      above the plane.  The grid frame, (x, y, normal) = frame(normal, a) (when it does not exist: frame(normal, b)):
 *          gx = dot(pc, x), gy = dot(pc, y) (f32);  sx = (floorf(gx / res) - (float)(width / 2)) * res, sy likewise with height --
 *          the camera's foot point in the middle of the grid, snapped to multiples of res as the default pose snaps it;
 *          pose[3 i + 0] = x.i + 0.0f, pose[3 i + 1] = y.i + 0.0f, pose[3 i + 2] = normal.i + 0.0f (no -0 in the rotation);
 *          pose[9 + i] = (float)((((double)o.i + (double)sx * (double)x.i) + (double)sy * (double)y.i) + (double)d * (double)normal.i):
 *      grid z = the fitted normal, the height origin on the plane.  The multiples of res are counted from o: a caller that wants
 *      successive grids cell-aligned passes the same `origin` every time.  The bands with the floor at height 0:
 *      z_min = -below, floor_max = step, z_max = body_height; width, height and res are handed through.
 *      The counts are exact: rows_used, candidates, direction_rows, aligned (in and out of the histogram), height_out_of_range,
 *      height_rows; dir_bin = (ia, ib) of the winner, height_bin = j*; per round inliers[k] = N, rms[k] and sums[k] = the ten words.
 *      ssf_navfloor_out (both optional, host memory): dir_hist 31 x 31 u32, height_hist 2048 u32.  The call returns 0 and writes
 *      the counts and histograms whatever the status.
 *
 * Defaults (ssf_navfloor_default_params) are design choices, not tuned values: up (0, -1, 0), origin NULL, tilt_cos 0.8, align_cos
 * 0.95, height_res 0.02 m, min_rows 32, floor_share256 64 (a quarter), refine_iters 3, first_dist 0.15 m, inlier_dist 0.05 m,
 * min_conf 0, both stamp ranges INT32_MIN..INT32_MAX, visible_only 0, width = height = 512, res 0.05 (ssf_navgrid.h's), below 0.5,
 * step 0.2, body_height 1.5 -- the default bands' meaning (ssf_navgrid.h) with the floor at 0.
 *
 * Refused with SSF_ERR_INVALID_ARG, each with a text of its own in ssf_last_error: a NULL handle, params or result; up not finite or
 * zero; origin not finite; tilt_cos outside (0, 1); align_cos outside (0, 1]; height_res, inlier_dist, first_dist, res, below, step
 * or body_height not finite or <= 0; refine_iters outside 0..8; min_rows < 3; floor_share256 outside 1..256; width or height outside
 * 1..4096; t_init_min > t_init_max or t_last_min > t_last_max.  With SSF_ERR_STATE: frames pending in the extract pipeline; a sharded
 * handle (cfg.nranks > 1).
 *
 * The call is synchronous and runs on the handle's stream.  It changes no state of the handle: a fit made between two frames changes
 * no later pose or model bit.  The host reads a small record after each stage (3 + refine_iters waits for the stream): the fit is
 * made at start-up, after a loop closure or every few seconds, not per frame.  Working buffers are allocated on first use and grown
 * as a whole; a growth that fails returns SSF_ERR_DEVICE and leaves the handle working.  Kernels appear in ssf_get_kernel_times under
 * profile = 1 (navfloor_prep, navfloor_direction, navfloor_height, navfloor_refine).
 *
 * Only libssf_hip_floor.so exports these functions; the ABI version of ssf.h is unchanged.
 */
#ifndef SSF_NAVFLOOR_H
#define SSF_NAVFLOOR_H

#include "ssf.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SSF_NAVFLOOR_OK = 0, SSF_NAVFLOOR_NO_FLOOR = 1, SSF_NAVFLOOR_DEGENERATE = 2 };
enum { SSF_NAVFLOOR_DIR_BINS = 31, SSF_NAVFLOOR_HEIGHT_BINS = 2048, SSF_NAVFLOOR_MAX_ROUNDS = 8 };

typedef struct ssf_navfloor_params {
    const float* origin;              /* 3 floats, map frame; NULL = the handle's current camera position */
    float   up[3];                    /* up hint in the map frame */
    float   tilt_cos;                 /* a candidate's normal has |n.u| >= tilt_cos */
    float   align_cos;                /* aligned / inlier: m.n0 (m.n_k) >= align_cos */
    float   height_res;               /* metres per bin of the height histogram */
    int     min_rows;                 /* the floor's window and every round need this many rows, >= 3 */
    int     floor_share256;           /* ... and W * 256 >= floor_share256 * max W, 1..256 */
    int     refine_iters;             /* rounds, 0..8 */
    float   first_dist, inlier_dist;  /* inlier distance of round 0 / of the later rounds, metres */
    float   min_conf;                 /* rows with conf > min_conf (strict) */
    int32_t t_init_min, t_init_max;   /* stamps.x in [min, max] */
    int32_t t_last_min, t_last_max;   /* stamps.y in [min, max] */
    int     visible_only;             /* 1: the visible rows only */
    int     width, height;            /* the grid the pose is centred and snapped for, 1..4096 each */
    float   res;                      /* its metres per cell */
    float   below, step, body_height; /* the bands: z_min = -below, floor_max = step, z_max = body_height */
} ssf_navfloor_params;

typedef struct ssf_navfloor_out {     /* host memory; either may be NULL */
    uint32_t* dir_hist;               /* 31 x 31, index ib * 31 + ia */
    uint32_t* height_hist;            /* 2048 */
} ssf_navfloor_out;

typedef struct ssf_navfloor_fit_result {
    int     status;                   /* SSF_NAVFLOOR_OK / NO_FLOOR / DEGENERATE */
    int     rounds;                   /* rounds that gave a new plane */
    float   normal[3], d;             /* the plane normal . (c - origin) = d */
    float   origin[3];
    float   camera_height;            /* signed distance of the handle's camera above the plane */
    int64_t rows_used, candidates, direction_rows, aligned, height_out_of_range, height_rows;
    int     dir_bin[2];               /* (ia, ib) of the winning direction bin */
    int     height_bin;               /* j* */
    int     reserved;
    int64_t inliers[8];               /* per round: N */
    float   rms[8];                   /* per round: residual of the fit, metres */
    int64_t sums[8][10];              /* per round: N, Sx, Sy, Sz, Sxx, Sxy, Syy, Sxz, Syz, Szz */
    float   pose[12];                 /* grid-to-map, what ssf_navgrid_params.pose takes */
    float   z_min, floor_max, z_max;  /* the bands for that pose */
    int     width, height;            /* as given */
    float   res;
} ssf_navfloor_fit_result;

int ssf_navfloor_default_params(const ssf_handle* h, ssf_navfloor_params* p);
int ssf_navfloor_fit(ssf_handle* h, const ssf_navfloor_params* p, const ssf_navfloor_out* out, ssf_navfloor_fit_result* res);

#ifdef __cplusplus
}
#endif

#endif /* SSF_NAVFLOOR_H */
