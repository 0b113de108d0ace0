/*
 * ssf_keyframes.h -- a fern-coded keyframe database kept on the device: encode the current frame, search the stored keyframes,
 * store the frame's supersurfels when the view is new, register a stored keyframe against the current frame.
 *
 * This is the step that decides WHETHER a loop exists and AGAINST WHICH keyframe; with it the chain
 *   ssf_keyframes_consider -> ssf_keyframes_align -> ssf_graph_build -> (the caller optimises) -> ssf_graph_apply
 * runs without a row-sized transfer: a keyframe's rows were produced on the device by the frame that became the keyframe, and
 * they stay there.  Per frame one small record (152 bytes) comes back to the host.
 *
 * The rule is this library's own, in the shape of randomised ferns (ElasticFusion's / the reference's Ferns); it claims no bit
 * parity with another implementation.  Every result is an exact integer and independent of any arrival order; the numpy
 * restatement tests/keyframe_ref.py reproduces every output bit for bit.
 *
 * "Current frame" = the last processed or extracted frame of the handle: its colour map (R, G, B as ingested, after any
 * ssf_set_input_format conversion), its plane depth (what ssf_get_plane_depth returns), its supersurfels (ssf_get_frame), and the
 * handle's pose (ssf_get_pose) and stamp (ssf_get_counts) at the moment of the call.  W x H = the handle's image size.
 *
 * 1. Coarse image.  Cells of B x B pixels, B in {4, 8, 16}; grid GW = W / B, GH = H / B (floor; the pixels beyond are ignored;
 *    W, H >= B).  Per cell and colour channel c: mean_c = (sum of c + B B / 2) / (B B) in integers.  A pixel's depth d counts iff
 *    d is finite and range_min <= d <= range_max (the handle's configuration); then q = (uint32) lrintf(d * 1000.0f) (one f32
 *    multiplication, then round to nearest even).  Per cell cnt = the pixels that count and
 *    depth_mm = cnt ? (sum of q + cnt / 2) / cnt : 0.  Integer sums only.
 * 2. Fern table, n ferns, 1 <= n <= SSF_KEYFRAMES_MAX_FERNS: per fern a cell (x, y), thresholds r, g, b (u8) and depth_mm (u32):
 *    ssf_fern.  Either the caller's (ssf_keyframes_set_ferns) or generated on the host from the 64-bit seed: the state s starts at
 *    the seed; one draw is  s += 0x9E3779B97F4A7C15;  z = s;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *    z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31  (splitmix64, all modulo 2^64).  Fern i takes six draws in the order
 *    x = z % GW, y = z % GH, r = z % 256, g = z % 256, b = z % 256, depth_mm = dlo + z % (dhi - dlo) with
 *    dlo = lrintf(range_min * 1000.0f), dhi = lrintf(range_max * 1000.0f) (dhi > dlo is required).
 * 3. Code of fern i against the coarse image: bit 0 mean_r > r, bit 1 mean_g > g, bit 2 mean_b > b, bit 3 cnt > 0 and
 *    depth_mm(cell) > depth_mm_i  (the bit order of ssf_fern_codes).  Codes are kept packed: eight 4-bit codes per u32, fern i in
 *    bits 4 (i % 8) .. 4 (i % 8) + 3 of word i / 8, padded with zero nibbles to a multiple of 64 words.  The interface carries
 *    them unpacked: n bytes, one code (0 .. 15) each.
 * 4. Dissimilarity of two code vectors: diff = the number of ferns whose codes differ, an integer in [0, n].
 * 5. Query of a code vector with a stamp t against the K stored keyframes: min_diff_all = the smallest diff over all of them
 *    (n + 1 when K = 0); the candidates are the keyframes with stamp <= t - min_gap (evaluated in 64 bits), ordered by the pair
 *    (diff, id) ascending; the first k <= SSF_KEYFRAMES_MAX_CANDIDATES of them are returned as (id, diff, stamp, loop) with
 *    loop = 1 iff (float) diff / (float) n <= loop_ratio (one IEEE f32 division).
 * 6. Consider (the per-frame call): encode the current frame, query it with the handle's stamp, the configured min_gap and
 *    k = SSF_KEYFRAMES_MAX_CANDIDATES, and add the frame as a new keyframe iff K == 0 or
 *    (float) min_diff_all / (float) n >= new_ratio.  When the store is full -- K == max_keyframes, or the rows in use plus the
 *    frame's rows with conf > 0 exceed max_rows -- nothing is added and the record says full = 1.
 * 7. A keyframe keeps: its id (dense, in insertion order, from 0), its packed codes, the handle's pose (12 f32, ssf_get_pose's
 *    layout) and stamp at that frame, and the frame's supersurfels with conf > 0 in frame order (a stable compaction) as full rows
 *    (26 words: position 3, colour 3, stamps 2, orientation 9, shape 6, dims 2, confidence 1) in the keyframe's camera frame.
 *    Capacity: max_keyframes keyframes and a pool of max_rows rows (0 = max_keyframes x S, S = the handle's superpixels), allocated
 *    by ssf_keyframes_configure, all or nothing.
 * 8. ssf_keyframes_align has ssf_align's outputs and ssf_align's arithmetic, its sources derived on the device from the stored
 *    rows: positions as stored, Lab of the stored colours (the same function the kernels use), normals = the third row of the
 *    stored orientation, confidences as stored (use_conf != 0) or all 1 (use_conf == 0: ssf_align without a confidence array).
 *
 * Defaults (ssf_keyframes_default_params): B 8, 500 ferns, seed 1234, 256 keyframes, max_rows 0, min_gap 30, new_ratio 0.3,
 * loop_ratio 0.2 -- defaults, not claims.
 *
 * Refusals.  SSF_ERR_INVALID_ARG: a NULL handle / parameter block / required output, a parameter out of range, an id that is not
 * stored, a code > 15.  SSF_ERR_STATE: before ssf_keyframes_configure (or after ssf_keyframes_clear); a second configure while a
 * database is live; ssf_keyframes_set_ferns while keyframes are stored; for the calls that read the current frame: no frame yet,
 * or one that came in through ssf_submit_frame_tables (it has no colour map); frames pending in the extract pipeline or a fuse
 * in progress; a sharded handle (cfg.nranks > 1: with a dealt extract a rank need not hold the colour map -- deliberately not
 * part of this interface).  SSF_ERR_CAPACITY: a full store (ssf_keyframes_add, ssf_keyframes_put) or a too-small output.
 * SSF_ERR_DEVICE: a failed allocation, which leaves the handle working and no half-built database.
 *
 * Every call is synchronous, runs on the handle's stream and changes no other state of the handle: a call between two frames
 * changes no later pose or model bit.  Nothing here reads an environment variable.  Kernel times appear in ssf_get_kernel_times
 * under profile = 1 (kf_encode, kf_search, kf_select, kf_align_prep, align).
 *
 * Only the HIP product library (libssf_hip.so) exports these functions; the ABI version of ssf.h is unchanged.
 */
#ifndef SSF_KEYFRAMES_H
#define SSF_KEYFRAMES_H

#include "ssf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SSF_KEYFRAMES_MAX_FERNS 4096
#define SSF_KEYFRAMES_MAX_CANDIDATES 8

typedef struct ssf_keyframes_params {
    int cell;                 /* B: 4, 8 or 16 */
    int n_ferns;              /* 1 .. SSF_KEYFRAMES_MAX_FERNS */
    uint64_t seed;            /* of the generated fern table */
    int max_keyframes;        /* >= 1 */
    int min_gap;              /* a candidate's stamp is <= the query's stamp - min_gap; >= 0 */
    int64_t max_rows;         /* rows of the pool; 0 = max_keyframes x S */
    float new_ratio;          /* consider adds iff min_diff_all / n >= new_ratio; finite */
    float loop_ratio;         /* a candidate is a loop candidate iff diff / n <= loop_ratio; finite */
} ssf_keyframes_params;

typedef struct ssf_fern {
    uint16_t x, y;            /* the cell: x < GW, y < GH */
    uint8_t r, g, b, pad;     /* pad = 0 */
    uint32_t depth_mm;
} ssf_fern;

typedef struct ssf_keyframe_candidate { int32_t id, diff, stamp, loop; } ssf_keyframe_candidate;

typedef struct ssf_keyframe_result {
    int32_t added;            /* 1: the frame became a keyframe */
    int32_t id;               /* its id, or -1 */
    int32_t full;             /* 1: it would have been added but the store is full */
    int32_t min_diff_all;     /* n + 1 when nothing was stored */
    int32_t n_keyframes;      /* stored after the call */
    int32_t n_candidates;
    ssf_keyframe_candidate candidates[SSF_KEYFRAMES_MAX_CANDIDATES];
} ssf_keyframe_result;

int ssf_keyframes_default_params(ssf_keyframes_params* p);
/* allocate the database (all or nothing) and generate the fern table from p->seed */
int ssf_keyframes_configure(ssf_handle* h, const ssf_keyframes_params* p);
/* replace the fern table (n = the configured n_ferns; only while no keyframe is stored) / read it back */
int ssf_keyframes_set_ferns(ssf_handle* h, const ssf_fern* ferns, int n);
int ssf_keyframes_get_ferns(ssf_handle* h, ssf_fern* ferns, int capacity);
/* the codes of the current frame, unpacked: n bytes */
int ssf_keyframes_encode(ssf_handle* h, uint8_t* codes, int capacity);
/* rule 5.  codes == NULL: the current frame's, with the handle's stamp (`stamp` is ignored); else n caller bytes with `stamp`.
 * min_gap < 0: the configured one.  0 <= k <= SSF_KEYFRAMES_MAX_CANDIDATES.  added = 0, id = -1, full = 0 in the record */
int ssf_keyframes_query(ssf_handle* h, const uint8_t* codes, int stamp, int min_gap, int k, ssf_keyframe_result* out);
/* the current frame becomes a keyframe whatever its codes; *id (optional) = its id */
int ssf_keyframes_add(ssf_handle* h, int* id);
/* rule 6 */
int ssf_keyframes_consider(ssf_handle* h, ssf_keyframe_result* out);
/* a keyframe from host data: codes n bytes, n_rows rows (every array of `rows` required when n_rows > 0), pose 12 f32, stamp */
int ssf_keyframes_put(ssf_handle* h, const uint8_t* codes, const ssf_surfels* rows, int n_rows, const float* pose, int stamp, int* id);
/* one keyframe back, each output optional: rows (arrays of `capacity` rows; SSF_ERR_CAPACITY when it has more), *n_rows,
 * pose 12 f32, *stamp, codes n bytes */
int ssf_keyframes_get(ssf_handle* h, int id, ssf_surfels* rows, int capacity, int* n_rows, float* pose, int* stamp, uint8_t* codes);
/* the caller moves a keyframe's pose (after a closure) */
int ssf_keyframes_set_pose(ssf_handle* h, int id, const float* pose);
/* rule 8: ssf_align with the stored rows of keyframe id as sources */
int ssf_keyframes_align(ssf_handle* h, int id, const float* init_pose, int use_conf, float* rel_pose, int* valid, int* iters,
                        int* pairs_last);
/* each optional: configured = 1 while a database is live, the stored keyframes, the pool rows in use, the parameters in force
 * (max_rows resolved) */
int ssf_keyframes_info(ssf_handle* h, int* configured, int* n_keyframes, int64_t* rows_used, ssf_keyframes_params* p);
/* free the database; ssf_keyframes_configure may be called again */
int ssf_keyframes_clear(ssf_handle* h);

#ifdef __cplusplus
}
#endif

#endif /* SSF_KEYFRAMES_H */
