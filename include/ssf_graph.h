/*
 * ssf_graph.h -- the deformation graph's nodes and the per-row weights, built and kept on the device.
 *
 * After a loop closure the caller bends the whole map: ssf_apply_deformation wants four node indices and four weights per model
 * row.  Everything that is O(model rows) is done here, where the model lives: sampling the nodes from the model, binding every
 * row to its nodes, keeping that binding resident, and applying the optimised node transforms through it.  Only the node table
 * (16 B per node out, 48 B per node in) crosses to the host.  The graph OPTIMISATION between ssf_graph_bind_points and
 * ssf_graph_apply is ssf_graph_solve.h's (on the device, over the same resident nodes); a caller may still run its own.
 *
 * The rule is this library's own, deterministic, in the ElasticFusion shape (nodes in time order, a row looks at the nodes born
 * around its own birth, the k + 1-th nearest sets the support radius); it claims no bit parity with any other implementation.
 * Every arithmetic step is one IEEE f32 operation in the order written (the library builds with -ffp-contract=off and correctly
 * rounded divide / sqrt), so the numpy restatement tests/graph_ref.py reproduces every output bit for bit.
 *
 * Rows and order.  Logical row index = position in ssf_get_model's order [visible | out-of-view], n = n_model.
 *   t_init(i) = stamps[2 i].
 * Sampling (stride, min_conf).  Eligible rows: conf > min_conf (strict) and a finite position.  Order the eligible rows by the
 *   pair (t_init, logical index) ascending; the row of rank r in that order is a node iff r % stride == 0.  Nodes keep that
 *   order: node k is the eligible row of rank k * stride, m = ceil(eligible / stride).  Per node: position (3 f32, the row's
 *   bits), t_init (i32), the source row (i32).
 * Binding (look = L), for every row i in [0, n), eligible or not:
 *   1. c = the first node index whose t_init >= t_init(i) (c in [0, m]: a lower bound over the time-ordered nodes).
 *   2. Window [lo, lo + W) with W = min(m, 2 L) and lo = clamp(c - L, 0, max(0, m - 2 L)).
 *   3. For every node k of the window, d = p_i - g_k componentwise and d2 = (d.x d.x + d.y d.y) + d.z d.z.
 *   4. The five smallest of (bits(d2) << 32) | k (u64) in ascending order: k_0 ... k_4.  idx4 = (k_0, k_1, k_2, k_3).
 *   5. dist_j = sqrtf(d2_j), dmax = dist_4, r_j = 1 - dist_j / dmax, w_j = r_j r_j, s = ((w_0 + w_1) + w_2) + w_3,
 *      weights4_j = w_j / s.
 *   6. Fallback: if dmax == 0, or s is not > 0, or the row's position is not finite: weights4 = (0.25, 0.25, 0.25, 0.25); for a
 *      non-finite position additionally idx4 = (lo, lo + 1, lo + 2, lo + 3).
 * Parameters: stride >= 1, look >= 3, min_conf finite, and m >= 5 after sampling (otherwise SSF_ERR_STATE, nothing is kept).
 * Defaults (ssf_graph_default_params): stride 50, look 20, min_conf 0.
 * Birth stamps may be any int32 (ssf_set_model), negative ones included; the time order is a counting sort over the span
 * [min, max] of the eligible rows' stamps, and a span max - min >= SSF_GRAPH_MAX_STAMP_SPAN (2^20) is refused with SSF_ERR_STATE.
 *
 * Validity.  A graph describes the logical rows at the moment of ssf_graph_build.  Anything that rewrites rows or their order --
 * a processed frame, ssf_set_model, ssf_apply_deformation, ssf_graph_apply itself, ssf_rehome_begin / _end -- makes it stale:
 * ssf_graph_apply, ssf_graph_get_binding and ssf_graph_bind_points then return SSF_ERR_STATE ("graph is stale: build it
 * again"); ssf_graph_get_nodes still returns the node table of the last build (a snapshot).  ssf_graph_build changes no other
 * state of the handle: a build between two frames changes no later pose or model bit.
 *
 * Refusals.  SSF_ERR_INVALID_ARG: a NULL handle / params / output, stride < 1, look < 3, min_conf not finite.  SSF_ERR_STATE:
 * frames pending in the extract pipeline or a fuse in progress, an empty model, m < 5, a stamp span too wide, a stale or missing
 * graph, and a sharded handle (cfg.nranks > 1): a time-ordered node set over the shards of a map needs an exchange between the
 * ranks, which is deliberately not part of this interface.  SSF_ERR_DEVICE: a working buffer could not be allocated; buffers
 * are allocated on first use and grown as a whole, a failed growth keeps no half-built graph and leaves the handle working.
 *
 * All calls are synchronous and run on the handle's stream.  The node table is bit-identical from run to run (integer counts
 * only, no result depends on the arrival order of an atomic).  Kernel times appear in ssf_get_kernel_times under profile = 1
 * (graph_rank, graph_sample, graph_bind, apply_deformation).
 *
 * Only the HIP product library (libssf_hip.so) exports these functions; the ABI version of ssf.h is unchanged.
 */
#ifndef SSF_GRAPH_H
#define SSF_GRAPH_H

#include "ssf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SSF_GRAPH_MAX_STAMP_SPAN (1 << 20)

typedef struct ssf_graph_params {
    int stride;               /* every stride-th eligible row in (t_init, logical index) order is a node; >= 1 */
    int look;                 /* L: a row looks at the 2 L nodes born around its own birth; >= 3 */
    float min_conf;           /* rows with conf > min_conf (and a finite position) are eligible as nodes */
} ssf_graph_params;

int ssf_graph_default_params(ssf_graph_params* p);
/* sample the nodes and bind all n_model rows; *n_nodes (optional) = m.  Nodes and binding stay resident on the device */
int ssf_graph_build(ssf_handle* h, const ssf_graph_params* p, int* n_nodes);
/* the node table: positions 3 m f32, t_init m i32, rows m i32 (each optional); SSF_ERR_CAPACITY when capacity < m */
int ssf_graph_get_nodes(ssf_handle* h, float* positions, int32_t* t_init, int32_t* rows, int capacity);
/* the resident binding: weights4 4 n f32, idx4 4 n i32 (n = the rows of the build); on_device: the outputs are device pointers */
int ssf_graph_get_binding(ssf_handle* h, float* weights4, int32_t* idx4, int on_device);
/* steps 1-6 for n caller points (host arrays: points 3 n f32, t_init n i32) against the resident nodes, with the build's look */
int ssf_graph_bind_points(ssf_handle* h, const float* points, const int32_t* t_init, int n, float* weights4, int32_t* idx4);
/* deform the model through the resident nodes and binding: node_rotations 9 m f32 (row-major), node_translations 3 m f32, as
 * ssf_apply_deformation's; the same kernels, no row-sized upload.  The graph is stale afterwards */
int ssf_graph_apply(ssf_handle* h, const float* node_rotations, const float* node_translations);
/* each optional: the nodes and rows of the last build (0 before one), valid = 1 while the graph describes the model */
int ssf_graph_info(ssf_handle* h, int* n_nodes, int* n_rows, int* valid);

#ifdef __cplusplus
}
#endif

#endif /* SSF_GRAPH_H */
