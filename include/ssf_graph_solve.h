/*
 * ssf_graph_solve.h -- the deformation graph's optimisation on the device: node transforms from point constraints.
 *
 * ssf_graph_build (ssf_graph.h) leaves the node table resident; ssf_graph_apply bends the map by solved node transforms.  This is
 * the step between them: the embedded deformation of Sumner et al. in the ElasticFusion shape, minimised by Gauss-Newton with a
 * diagonally preconditioned conjugate-gradient inner loop, on the node table where it lives.  Only the constraints come in and (on
 * request) 48 B per node go out.
 *
 * The rule is this library's own and deterministic; it claims no bit parity with any other implementation.  All solver state and
 * arithmetic is IEEE f64, one operation per step in the order written (-ffp-contract=off; f64 divide and sqrt are correctly
 * rounded); inputs and outputs are f32, converted exactly on the way in and rounded once on the way out.  The numpy restatement
 * tests/graph_solve_ref.py reproduces every output bit for bit.  Notation: dot3(a, b) = (a0 b0 + a1 b1) + a2 b2; a sum written
 * a + b + c is evaluated left to right.
 *
 * Unknowns.  Per node j of the resident graph (m nodes, positions g_j, time order): A_j (3 x 3, row-major, A[i][c]) and t_j; the
 *   vector x is node-major, 12 per node (A's nine, then t's three); start A = I, t = 0.  c_k(j) is column k of A_j.
 * Edges.  For node j run steps 1-4 of ssf_graph.h's binding on (g_j, t_init_j) against the node table with the build's look;
 *   N(j) = the first four of k_0 ... k_4 that are != j (m >= 5 guarantees four).  Edge id e = 4 j + n, e_jn = g_k - g_j (k = N(j)_n).
 * Constraints.  n_con triples (src s 3 f32, t_init i32, dst d 3 f32), each bound by steps 1-6 (ssf_graph_bind_points) to
 *   (idx4, weights4); u_n = s - g_k (k = idx4_n).  A pin is simply d == s.
 * Residuals, with sr = sqrt(w_rot), sg = sqrt(w_reg), sc = sqrt(w_con):
 *   rot, 6 per node:   sr dot3(c_0, c_1), sr dot3(c_0, c_2), sr dot3(c_1, c_2), sr (dot3(c_k, c_k) - 1) for k = 0, 1, 2.
 *   reg, 3 per edge:   row i = sg ((((dot3(A_j[i], e) + g_j[i]) + t_j[i]) - g_k[i]) - t_k[i]).
 *   con, 3 per constraint: row i = sc (((w_0 v_0 + w_1 v_1) + w_2 v_2) + w_3 v_3), v_n = ((dot3(A_k[i], u_n) + g_k[i]) + t_k[i]) - d[i].
 *     This is the position formula of the deformation kernel with d taken inside the weighted sum: weights4 add up to 1 only to
 *     f32 rounding, and inside the sum a pin's residual is exactly zero at the identity (the two forms differ by (sum w - 1) d).
 *   E = (E_rot + E_reg) + E_con, each the sum of its squared rows (no factor 1/2).
 * Jacobian entries (J v and J^T y use exactly these products):
 *   rot: s_k = sr c_k;  rows 0-2 pair the columns: y_0 = dot3(s_1, V_0) + dot3(s_0, V_1), y_1 = dot3(s_2, V_0) + dot3(s_0, V_2),
 *        y_2 = dot3(s_2, V_1) + dot3(s_1, V_2), y_{3+k} = dot3(2 s_k, V_k) (V_k: column k of v's A part).  Transposed, entry [i] of
 *        column 0: (y_0 s_1[i] + y_1 s_2[i]) + y_3 (2 s_0[i]); column 1: (y_0 s_0[i] + y_2 s_2[i]) + y_4 (2 s_1[i]); column 2:
 *        (y_1 s_0[i] + y_2 s_1[i]) + y_5 (2 s_2[i]).  Diagonal: (s_1[i]^2 + s_2[i]^2) + (2 s_0[i])^2 and cyclically as above.
 *   reg: se = sg e (componentwise).  y_i = (dot3(se, V_j[i]) + sg vt_j[i]) - sg vt_k[i].  Transposed: A_j[i][c] += y_i se_c,
 *        t_j[i] += y_i sg, t_k[i] -= y_i sg.  Diagonal: se_c^2 on A_j[i][c], sg sg on t_j[i] and on t_k[i].
 *   con: sw_n = sc w_n, su_n = sw_n u_n.  y_i = ((q_0 + q_1) + q_2) + q_3, q_n = dot3(su_n, V_k[i]) + sw_n vt_k[i].  Transposed:
 *        A_k[i][c] += y_i su_n,c, t_k[i] += y_i sw_n.  Diagonal: su_n,c^2 and sw_n^2.
 * Gather form.  J^T y, J^T J v and the diagonal are computed per node, never scattered: each of the node's 12 sums starts at +0.0
 *   and takes, in this order: the rot rows' term above; its own four edges n = 0 ... 3; the edges that point AT it, in ascending
 *   edge id; its constraint incidences in ascending 4 c + n.  (The two transposed lists are stable counting sorts by target node.)
 *   Last, damping v_c (for J^T J v) or damping (for the diagonal D) is added.
 * Dot products and energies.  Per node the 12 products are added left to right; the per-node values are reduced in blocks of 256
 *   by the halving tree s[i] += s[i + h], h = 128 ... 1 (the tail padded with +0.0), and the block sums are added in ascending
 *   block order starting from +0.0.  E_rot: per node the 6 squares left to right; E_reg: per node the 12 squares of its own edges
 *   (n major, i minor); E_con: per constraint its 3 squares, blocks of 256 constraints.  No float atomics; no result depends on
 *   an arrival order.
 * Outer loop (Gauss-Newton).  r = residuals(x), E = energy.  Up to max_outer times: b = -(J^T r), D = diag(J^T J) + damping,
 *   delta = the inner loop's result, x = x + delta, E_new = energy(residuals(x)); stop after this step when
 *   |E - E_new| <= outer_tol E; else E = E_new.  Every step is taken (no line search).
 * Inner loop (conjugate gradients on (J^T J + damping I) delta = b, preconditioned by 1 / D).  delta = 0, r = b,
 *   z_c = D_c > 0 ? r_c / D_c : 0, rho_0 = rho = r.z.  If not rho_0 > 0: zero iterations (ended "zero").  Iteration it = 0, 1, ...:
 *   p = z (it = 0) or z + (rho / rho_prev) p;  q = J^T (J p) + damping p;  pq = p.q;  if pq is not > 0 or not finite the loop ends
 *   ("breakdown": this iteration does not count, delta is kept);  alpha = rho / pq;  delta += alpha p;  r -= alpha q;  z as above;
 *   rho_prev = rho, rho = r.z;  it += 1.  Then, only when it is a multiple of inner_check: end ("tolerance") if
 *   rho <= (inner_tol inner_tol) rho_0.  Then end ("max_inner") if it >= max_inner.  The stop rule being tested every inner_check
 *   iterations only (one small host read each), the iteration counts are part of the specification.
 * Output.  node_rotations 9 m f32 (A rounded once) and node_translations 3 m f32, in ssf_graph_apply's layout, resident on the
 *   device with the graph, and the result record below.
 *
 * Parameters (ssf_graph_solve_default_params): w_rot 1, w_reg 10, w_con 100, max_outer 8, max_inner 512, inner_check 16,
 * inner_tol 1e-6, outer_tol 1e-6, damping 0.
 *
 * Validity.  As ssf_graph.h: a solve needs a graph that still describes the model.  ssf_graph_solve changes no other state of
 * the handle (a build + solve between two frames changes no later pose or model bit) and touches no buffer of the frame path.
 * Solved transforms belong to the graph they were solved on: a new ssf_graph_build discards them, and once the graph is stale
 * ssf_graph_get_transforms and ssf_graph_apply_solved return SSF_ERR_STATE.  ssf_graph_apply_solved deforms the model through
 * the resident nodes, binding and transforms (ssf_graph_apply with nothing uploaded); the graph is stale afterwards.
 *
 * Refusals.  SSF_ERR_INVALID_ARG: a NULL handle / params / src / t_init / dst / output, n_con < 1 (or > 2^20: the counting sorts' one-workgroup scan), a non-finite src or
 * dst, a weight, tolerance or damping that is not finite or < 0, max_outer < 1 or > SSF_GRAPH_SOLVE_MAX_OUTER, max_inner < 1,
 * inner_check < 1.  SSF_ERR_STATE: frames pending, a sharded handle, a missing or stale graph, m >= 2^20 (the counting sorts' key
 * range), no solve yet (get_transforms / apply_solved).  SSF_ERR_CAPACITY: capacity < m.  SSF_ERR_DEVICE: a working buffer could
 * not be allocated (buffers are allocated on first use and grown as a whole or not at all; the handle keeps working).
 * A call refused with SSF_ERR_INVALID_ARG or SSF_ERR_STATE touches nothing: the transforms of the last solve stay as they were.
 *
 * All calls are synchronous and run on the handle's stream.  Kernel time appears in ssf_get_kernel_times under profile = 1 as
 * graph_solve.  Only the HIP product library exports these functions; the ABI version of ssf.h is unchanged.
 */
#ifndef SSF_GRAPH_SOLVE_H
#define SSF_GRAPH_SOLVE_H

#include "ssf_graph.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SSF_GRAPH_SOLVE_MAX_OUTER 64
#define SSF_GRAPH_SOLVE_MAX_NODES (1 << 20)
#define SSF_GRAPH_SOLVE_MAX_CONSTRAINTS (1 << 20)

/* how the last inner loop ended */
#define SSF_GRAPH_SOLVE_END_TOLERANCE 0
#define SSF_GRAPH_SOLVE_END_MAX_INNER 1
#define SSF_GRAPH_SOLVE_END_BREAKDOWN 2
#define SSF_GRAPH_SOLVE_END_ZERO 3

typedef struct ssf_graph_solve_params {
    double w_rot, w_reg, w_con;       /* weights of the three residual groups; finite, >= 0 */
    double inner_tol, outer_tol;      /* relative: on rho = r.z, on the energy change; finite, >= 0 */
    double damping;                   /* added to the diagonal of J^T J; finite, >= 0 */
    int max_outer, max_inner, inner_check;
} ssf_graph_solve_params;

typedef struct ssf_graph_solve_result {
    double e_before, e_after;         /* E at the identity and after the last step */
    double e_rot, e_reg, e_con;       /* the split of e_after */
    int outer;                        /* Gauss-Newton steps taken */
    int inner_end;                    /* SSF_GRAPH_SOLVE_END_* of the last step's inner loop */
    int inner[SSF_GRAPH_SOLVE_MAX_OUTER];      /* inner iterations of every step taken (0 beyond) */
} ssf_graph_solve_result;

int ssf_graph_solve_default_params(ssf_graph_solve_params* p);
/* N(j) of every node: 4 m i32 (edge 4 j + n); SSF_ERR_CAPACITY when capacity < m */
int ssf_graph_get_edges(ssf_handle* h, int32_t* edges, int capacity);
/* host arrays src 3 n_con f32, t_init n_con i32, dst 3 n_con f32; result is optional */
int ssf_graph_solve(ssf_handle* h, const ssf_graph_solve_params* p, const float* src, const int32_t* t_init, const float* dst,
                    int n_con, ssf_graph_solve_result* result);
/* the transforms of the last solve: rotations 9 m f32, translations 3 m f32 (each optional) */
int ssf_graph_get_transforms(ssf_handle* h, float* rotations, float* translations, int capacity);
int ssf_graph_apply_solved(ssf_handle* h);

#ifdef __cplusplus
}
#endif

#endif /* SSF_GRAPH_SOLVE_H */
