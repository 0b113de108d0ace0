// ssf_graph_solve.hip -- the deformation graph's optimisation (include/ssf_graph_solve.h) on gfx950.
//
// What is computed is pinned, operation by operation, in include/ssf_graph_solve.h (the numpy restatement: tests/graph_solve_ref.py).
// How:
//   * setup  the edges are ssf_graph.hip's five-nearest kernel run for the nodes themselves, the constraints are bound by its
//            bind-points kernel, and the two transposed lists (edges that point AT a node, constraint incidences of a node) are its
//            stable counting sort with the target node as the key (lo = 0, 1..3 digit passes for m < 2^20), booked under graph_solve;
//            k_solve_offsets turns the sorted keys into per-node offsets by a lower bound.
//   * layout every vector is node-major f64, 12 per node, one thread per node (or per constraint) in workgroups of 256: at 20 000
//            nodes a vector is 1.9 MB and everything sits in L2; the design problem is launches, not bytes.
//   * an inner iteration is three launches, with no host trip and no single-workgroup launch between them:
//            k_solve_jp      p = z + beta p (beta from the block partials of rho, summed in ascending order by every workgroup) and
//                            y = J p.  A thread is node i and constraint i; a constraint forms the p of its four nodes from z and
//                            the previous p, the same operation on the same operands as the node's own thread, hence the same bits;
//                            p is kept in two buffers that take turns.
//            k_solve_jt      q = J^T y + damping p as a gather per node, the block partials of p.q.
//            k_solve_update  alpha from the partials; delta, r, z; the block partials of the next rho.
//            (Two launches would need every node to recompute the rows of all its constraints -- hundreds for the few nodes that a
//            frame's supersurfels bind to; the residual-space vector is written once instead.)
//   * the host reads the partials of rho once per inner_check iterations.  A breakdown (p.q not positive) freezes the iteration on
//            the device: the update is skipped and rho becomes NaN, which every later launch of the chunk inherits; the host finds
//            the iteration in the p.q history.
//   * reductions: the halving tree over 256 in LDS (2 KB, the only LDS), block sums added in ascending block order.  No float
//            atomics, no cooperative launch: kernel boundaries are the barrier.
#include "ssf_handle.hpp"

namespace ssf {

struct SolveArgs {
    const float4* nodes; const int4* edges; int m, nc, nbn, nbc;
    const uint32_t *in_off, *in_list, *con_off, *con_list;
    const float *src, *dst; const float4* w4; const int4* idx4;
    double *x, *b, *D, *delta, *r, *z, *q, *y_rot, *y_reg, *y_con;
    double *e_rot, *e_reg, *e_con, *pq, *hist;
    float *rot, *trans;
    double sr, sg, sc, damping;
};

// the halving tree over the workgroup's 256 values; every thread gets the sum (the closing barrier frees s for the next use)
__device__ __forceinline__ double block_tree256(double v, double* s) {
    s[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int h = 128; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + h];
        __syncthreads();
    }
    const double out = s[0];
    __syncthreads();
    return out;
}
__device__ __forceinline__ double ordered_sum(const double* __restrict__ part, int nb) {
    double s = 0.0;
    for (int b = 0; b < nb; b++) s = s + part[b];
    return s;
}
__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }
__device__ __forceinline__ void ld12(const double* __restrict__ v, int j, double* o) {
#pragma unroll
    for (int c = 0; c < 12; c++) o[c] = v[12 * (size_t)j + c];
}
__device__ __forceinline__ int lane4(const int4& v, int n) { return n == 0 ? v.x : n == 1 ? v.y : n == 2 ? v.z : v.w; }
__device__ __forceinline__ float lane4(const float4& v, int n) { return n == 0 ? v.x : n == 1 ? v.y : n == 2 ? v.z : v.w; }

// off[k] = the first position of the sorted keys that holds a key >= k, k in [0, m]
__global__ __launch_bounds__(256) void k_solve_offsets(const int32_t* __restrict__ key, int n, int m, uint32_t* __restrict__ off) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k > m) return;
    int a = 0, b = n;
    while (a < b) { const int mid = (a + b) >> 1; if (key[mid] < k) a = mid + 1; else b = mid; }
    off[k] = (uint32_t)a;
}
__global__ __launch_bounds__(256) void k_solve_init(double* __restrict__ x, int m) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
#pragma unroll
    for (int c = 0; c < 12; c++) x[12 * (size_t)j + c] = (c == 0 || c == 4 || c == 8) ? 1.0 : 0.0;
}

// ---- residuals at x (into y_rot / y_reg / y_con) and the block partials of the three energies ------------------------------
__global__ __launch_bounds__(256) void k_solve_residual(SolveArgs a) {
    __shared__ double red[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double erot = 0.0, ereg = 0.0, econ = 0.0;
    if (i < a.m) {
        double X[12]; ld12(a.x, i, X);
        const float4 gf = a.nodes[i];
        const double g[3] = {(double)gf.x, (double)gf.y, (double)gf.z};
        const double c0[3] = {X[0], X[3], X[6]}, c1[3] = {X[1], X[4], X[7]}, c2[3] = {X[2], X[5], X[8]};
        double rr[6];
        rr[0] = a.sr * dot3(c0[0], c0[1], c0[2], c1[0], c1[1], c1[2]);
        rr[1] = a.sr * dot3(c0[0], c0[1], c0[2], c2[0], c2[1], c2[2]);
        rr[2] = a.sr * dot3(c1[0], c1[1], c1[2], c2[0], c2[1], c2[2]);
        rr[3] = a.sr * (dot3(c0[0], c0[1], c0[2], c0[0], c0[1], c0[2]) - 1.0);
        rr[4] = a.sr * (dot3(c1[0], c1[1], c1[2], c1[0], c1[1], c1[2]) - 1.0);
        rr[5] = a.sr * (dot3(c2[0], c2[1], c2[2], c2[0], c2[1], c2[2]) - 1.0);
        erot = rr[0] * rr[0];
#pragma unroll
        for (int k = 1; k < 6; k++) erot = erot + rr[k] * rr[k];
#pragma unroll
        for (int k = 0; k < 6; k++) a.y_rot[6 * (size_t)i + k] = rr[k];
        const int4 ed = a.edges[i];
#pragma unroll
        for (int n = 0; n < 4; n++) {
            const int k = lane4(ed, n);
            const float4 kf = a.nodes[k];
            const double gk[3] = {(double)kf.x, (double)kf.y, (double)kf.z};
            const double e0 = gk[0] - g[0], e1 = gk[1] - g[1], e2 = gk[2] - g[2];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double Ae = dot3(X[3 * r], X[3 * r + 1], X[3 * r + 2], e0, e1, e2);
                const double v = a.sg * ((((Ae + g[r]) + X[9 + r]) - gk[r]) - a.x[12 * (size_t)k + 9 + r]);
                a.y_reg[12 * (size_t)i + 3 * n + r] = v;
                ereg = (n == 0 && r == 0) ? v * v : ereg + v * v;
            }
        }
    }
    if (i < a.nc) {
        const int4 id = a.idx4[i]; const float4 wf = a.w4[i];
        double wv[4][3];
#pragma unroll
        for (int n = 0; n < 4; n++) {
            const int k = lane4(id, n);
            const double w = (double)lane4(wf, n);
            const float4 kf = a.nodes[k];
            const double gk[3] = {(double)kf.x, (double)kf.y, (double)kf.z};
            const double u0 = (double)a.src[3 * (size_t)i] - gk[0], u1 = (double)a.src[3 * (size_t)i + 1] - gk[1], u2 = (double)a.src[3 * (size_t)i + 2] - gk[2];
            double Xk[12]; ld12(a.x, k, Xk);
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double Au = dot3(Xk[3 * r], Xk[3 * r + 1], Xk[3 * r + 2], u0, u1, u2);
                wv[n][r] = w * (((Au + gk[r]) + Xk[9 + r]) - (double)a.dst[3 * (size_t)i + r]);
            }
        }
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const double v = a.sc * (((wv[0][r] + wv[1][r]) + wv[2][r]) + wv[3][r]);
            a.y_con[3 * (size_t)i + r] = v;
            econ = r == 0 ? v * v : econ + v * v;
        }
    }
    const double s0 = block_tree256(erot, red), s1 = block_tree256(ereg, red), s2 = block_tree256(econ, red);
    if (threadIdx.x == 0) {
        if ((int)blockIdx.x < a.nbn) { a.e_rot[blockIdx.x] = s0; a.e_reg[blockIdx.x] = s1; }
        if ((int)blockIdx.x < a.nbc) a.e_con[blockIdx.x] = s2;
    }
}

// ---- J^T y per node, in the header's gather order ------------------------------------------------------------------------------
// GRAD: y = the residuals: b = -(J^T y), D = diag(J^T J) + damping, delta = 0, r = b, z = r / D, the partials of rho_0 into `dots`
// else: y = J p: q = J^T y + damping p, the partials of p.q into `dots`
template <bool GRAD>
__global__ __launch_bounds__(256) void k_solve_jt(SolveArgs a, const double* __restrict__ p, double* __restrict__ dots) {
    __shared__ double red[256];
    const int j = blockIdx.x * 256 + threadIdx.x;
    double part = 0.0;
    if (j < a.m) {
        double X[12]; ld12(a.x, j, X);
        double acc[12], dg[12];
        double y[6];
#pragma unroll
        for (int k = 0; k < 6; k++) y[k] = a.y_rot[6 * (size_t)j + k];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double s0 = a.sr * X[3 * i], s1 = a.sr * X[3 * i + 1], s2 = a.sr * X[3 * i + 2];
            acc[3 * i] = 0.0 + ((y[0] * s1 + y[1] * s2) + y[3] * (2.0 * s0));
            acc[3 * i + 1] = 0.0 + ((y[0] * s0 + y[2] * s2) + y[4] * (2.0 * s1));
            acc[3 * i + 2] = 0.0 + ((y[1] * s0 + y[2] * s1) + y[5] * (2.0 * s2));
            acc[9 + i] = 0.0;
            if (GRAD) {
                dg[3 * i] = 0.0 + ((s1 * s1 + s2 * s2) + (2.0 * s0) * (2.0 * s0));
                dg[3 * i + 1] = 0.0 + ((s0 * s0 + s2 * s2) + (2.0 * s1) * (2.0 * s1));
                dg[3 * i + 2] = 0.0 + ((s0 * s0 + s1 * s1) + (2.0 * s2) * (2.0 * s2));
                dg[9 + i] = 0.0;
            }
        }
        const float4 gf = a.nodes[j];
        const double g[3] = {(double)gf.x, (double)gf.y, (double)gf.z};
        const double sg2 = a.sg * a.sg;
        const int4 ed = a.edges[j];
#pragma unroll
        for (int n = 0; n < 4; n++) {                                 // its own four edges
            const float4 kf = a.nodes[lane4(ed, n)];
            const double se[3] = {a.sg * ((double)kf.x - g[0]), a.sg * ((double)kf.y - g[1]), a.sg * ((double)kf.z - g[2])};
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double yv = a.y_reg[12 * (size_t)j + 3 * n + r];
#pragma unroll
                for (int c = 0; c < 3; c++) { acc[3 * r + c] = acc[3 * r + c] + yv * se[c]; if (GRAD) dg[3 * r + c] = dg[3 * r + c] + se[c] * se[c]; }
                acc[9 + r] = acc[9 + r] + yv * a.sg;
                if (GRAD) dg[9 + r] = dg[9 + r] + sg2;
            }
        }
        for (uint32_t q = a.in_off[j]; q < a.in_off[j + 1]; q++) {     // the edges that point at it, ascending edge id
            const size_t e = a.in_list[q];
#pragma unroll
            for (int r = 0; r < 3; r++) { acc[9 + r] = acc[9 + r] - a.y_reg[3 * e + r] * a.sg; if (GRAD) dg[9 + r] = dg[9 + r] + sg2; }
        }
        for (uint32_t q = a.con_off[j]; q < a.con_off[j + 1]; q++) {   // its constraint incidences, ascending 4 c + n
            const uint32_t inc = a.con_list[q];
            const size_t c = inc >> 2;
            const double sw = a.sc * (double)reinterpret_cast<const float*>(a.w4)[inc];
            const double su[3] = {sw * ((double)a.src[3 * c] - g[0]), sw * ((double)a.src[3 * c + 1] - g[1]), sw * ((double)a.src[3 * c + 2] - g[2])};
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double yv = a.y_con[3 * c + r];
#pragma unroll
                for (int cc = 0; cc < 3; cc++) { acc[3 * r + cc] = acc[3 * r + cc] + yv * su[cc]; if (GRAD) dg[3 * r + cc] = dg[3 * r + cc] + su[cc] * su[cc]; }
                acc[9 + r] = acc[9 + r] + yv * sw;
                if (GRAD) dg[9 + r] = dg[9 + r] + sw * sw;
            }
        }
        if (GRAD) {
#pragma unroll
            for (int c = 0; c < 12; c++) {
                const double bv = -acc[c], dv = dg[c] + a.damping;
                const double zv = dv > 0.0 ? bv / dv : 0.0;
                a.b[12 * (size_t)j + c] = bv; a.D[12 * (size_t)j + c] = dv; a.r[12 * (size_t)j + c] = bv; a.z[12 * (size_t)j + c] = zv;
                a.delta[12 * (size_t)j + c] = 0.0;
                part = c == 0 ? bv * zv : part + bv * zv;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 12; c++) {
                const double pv = p[12 * (size_t)j + c];
                const double qv = acc[c] + a.damping * pv;
                a.q[12 * (size_t)j + c] = qv;
                part = c == 0 ? pv * qv : part + pv * qv;
            }
        }
    }
    const double s = block_tree256(part, red);
    if (threadIdx.x == 0) dots[blockIdx.x] = s;
}

// ---- p = z + beta p (into p_new) and y = J p -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_solve_jp(SolveArgs a, int first, const double* __restrict__ rho_cur, const double* __restrict__ rho_prev,
                                                  const double* __restrict__ p_old, double* __restrict__ p_new) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    double beta = 0.0;
    if (!first) beta = ordered_sum(rho_cur, a.nbn) / ordered_sum(rho_prev, a.nbn);
    auto pv = [&](int k, int c) -> double {
        const double zv = a.z[12 * (size_t)k + c];
        return first ? zv : zv + beta * p_old[12 * (size_t)k + c];
    };
    if (i < a.m) {
        double X[12], P[12]; ld12(a.x, i, X);
#pragma unroll
        for (int c = 0; c < 12; c++) { P[c] = pv(i, c); p_new[12 * (size_t)i + c] = P[c]; }
        double s0[3], s1[3], s2[3];
#pragma unroll
        for (int r = 0; r < 3; r++) { s0[r] = a.sr * X[3 * r]; s1[r] = a.sr * X[3 * r + 1]; s2[r] = a.sr * X[3 * r + 2]; }
        double* yo = a.y_rot + 6 * (size_t)i;
        yo[0] = dot3(s1[0], s1[1], s1[2], P[0], P[3], P[6]) + dot3(s0[0], s0[1], s0[2], P[1], P[4], P[7]);
        yo[1] = dot3(s2[0], s2[1], s2[2], P[0], P[3], P[6]) + dot3(s0[0], s0[1], s0[2], P[2], P[5], P[8]);
        yo[2] = dot3(s2[0], s2[1], s2[2], P[1], P[4], P[7]) + dot3(s1[0], s1[1], s1[2], P[2], P[5], P[8]);
        yo[3] = dot3(2.0 * s0[0], 2.0 * s0[1], 2.0 * s0[2], P[0], P[3], P[6]);
        yo[4] = dot3(2.0 * s1[0], 2.0 * s1[1], 2.0 * s1[2], P[1], P[4], P[7]);
        yo[5] = dot3(2.0 * s2[0], 2.0 * s2[1], 2.0 * s2[2], P[2], P[5], P[8]);
        const float4 gf = a.nodes[i];
        const int4 ed = a.edges[i];
#pragma unroll
        for (int n = 0; n < 4; n++) {
            const int k = lane4(ed, n);
            const float4 kf = a.nodes[k];
            const double se0 = a.sg * ((double)kf.x - (double)gf.x), se1 = a.sg * ((double)kf.y - (double)gf.y), se2 = a.sg * ((double)kf.z - (double)gf.z);
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double Pe = dot3(se0, se1, se2, P[3 * r], P[3 * r + 1], P[3 * r + 2]);
                a.y_reg[12 * (size_t)i + 3 * n + r] = (Pe + a.sg * P[9 + r]) - a.sg * pv(k, 9 + r);
            }
        }
    }
    if (i < a.nc) {
        const int4 id = a.idx4[i]; const float4 wf = a.w4[i];
        double qn[4][3];
#pragma unroll
        for (int n = 0; n < 4; n++) {
            const int k = lane4(id, n);
            const double sw = a.sc * (double)lane4(wf, n);
            const float4 kf = a.nodes[k];
            const double su0 = sw * ((double)a.src[3 * (size_t)i] - (double)kf.x), su1 = sw * ((double)a.src[3 * (size_t)i + 1] - (double)kf.y),
                         su2 = sw * ((double)a.src[3 * (size_t)i + 2] - (double)kf.z);
#pragma unroll
            for (int r = 0; r < 3; r++)
                qn[n][r] = dot3(su0, su1, su2, pv(k, 3 * r), pv(k, 3 * r + 1), pv(k, 3 * r + 2)) + sw * pv(k, 9 + r);
        }
#pragma unroll
        for (int r = 0; r < 3; r++) a.y_con[3 * (size_t)i + r] = ((qn[0][r] + qn[1][r]) + qn[2][r]) + qn[3][r];
    }
}

// ---- alpha = rho / p.q; delta, r, z; the partials of the next rho; hist[slot] = p.q ---------------------------------------------
__global__ __launch_bounds__(256) void k_solve_update(SolveArgs a, const double* __restrict__ p, const double* __restrict__ rho_cur,
                                                      double* __restrict__ rho_next, int slot) {
    __shared__ double red[256];
    const int j = blockIdx.x * 256 + threadIdx.x;
    const double rho = ordered_sum(rho_cur, a.nbn), pq = ordered_sum(a.pq, a.nbn);
    if (blockIdx.x == 0 && threadIdx.x == 0) a.hist[slot] = pq;
    if (!(pq > 0.0 && pq <= 1.7976931348623157e308)) {                // breakdown: nothing moves, and rho = NaN freezes what follows
        if (threadIdx.x == 0) rho_next[blockIdx.x] = __longlong_as_double(0x7FF8000000000000ll);
        return;
    }
    const double alpha = rho / pq;
    double part = 0.0;
    if (j < a.m) {
#pragma unroll
        for (int c = 0; c < 12; c++) {
            const size_t o = 12 * (size_t)j + c;
            const double pv = p[o];
            a.delta[o] = a.delta[o] + alpha * pv;
            const double rv = a.r[o] - alpha * a.q[o];
            const double dv = a.D[o];
            const double zv = dv > 0.0 ? rv / dv : 0.0;
            a.r[o] = rv; a.z[o] = zv;
            part = c == 0 ? rv * zv : part + rv * zv;
        }
    }
    const double s = block_tree256(part, red);
    if (threadIdx.x == 0) rho_next[blockIdx.x] = s;
}

// x += delta, and the transforms rounded to f32
__global__ __launch_bounds__(256) void k_solve_step(SolveArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.m) return;
#pragma unroll
    for (int c = 0; c < 12; c++) {
        const size_t o = 12 * (size_t)j + c;
        const double v = a.x[o] + a.delta[o];
        a.x[o] = v;
        if (c < 9) a.rot[9 * (size_t)j + c] = (float)v; else a.trans[3 * (size_t)j + c - 9] = (float)v;
    }
}

}  // namespace ssf

// ---- host: the entry points of include/ssf_graph_solve.h ---------------------------------------------------------------------
static double host_ordered_sum(const double* part, int nb) {
    double s = 0.0;
    for (int b = 0; b < nb; b++) s = s + part[b];
    return s;
}
#define SOLVE_HIST 256                            // iterations between two host reads at most (the p.q history's length)

extern "C" {
int ssf_graph_solve_default_params(ssf_graph_solve_params* p) {
    if (!p) return SSF_ERR_INVALID_ARG;
    p->w_rot = 1.0; p->w_reg = 10.0; p->w_con = 100.0; p->inner_tol = 1e-6; p->outer_tol = 1e-6; p->damping = 0.0;
    p->max_outer = 8; p->max_inner = 512; p->inner_check = 16;
    return SSF_OK;
}
static int solve_usable(ssf_handle* h, const char* who) {
    { int rc = graph_usable(h, who); if (rc) return rc; }
    if (h->graph.m >= SSF_GRAPH_SOLVE_MAX_NODES) { h->err = std::string(who) + ": " + std::to_string(h->graph.m) + " nodes; fewer than 2^20 are solved"; return SSF_ERR_STATE; }
    return SSF_OK;
}
// the per-node group (edges included): grown as a whole
static int solve_grow_nodes(ssf_handle* h, const char* who) {
    SolveWs& s = h->solve;
    const size_t m = (size_t)h->graph.m;
    if (m <= s.node_cap) return SSF_OK;
    const size_t cap = m + m / 4, v = 96 * cap, nb = (cap + 255) / 256;
    s.solved = false;
    if (!s.bufs.grow({{(void**)&s.edges, 16 * cap}, {(void**)&s.in_off, 4 * (cap + 1)}, {(void**)&s.con_off, 4 * (cap + 1)}, {(void**)&s.x, v},
                      {(void**)&s.b, v}, {(void**)&s.D, v}, {(void**)&s.delta, v}, {(void**)&s.r, v}, {(void**)&s.z, v}, {(void**)&s.p0, v},
                      {(void**)&s.p1, v}, {(void**)&s.q, v}, {(void**)&s.y_rot, 48 * cap}, {(void**)&s.y_reg, v},
                      {(void**)&s.part, 8 * (5 * nb + SOLVE_HIST)}, {(void**)&s.rot, 36 * cap}, {(void**)&s.trans, 12 * cap}})) {
        h->err = std::string(who) + ": allocation of the working buffers failed"; return SSF_ERR_DEVICE;
    }
    s.node_cap = cap;
    return SSF_OK;
}
int ssf_graph_get_edges(ssf_handle* h, int32_t* edges, int capacity) {
    if (!h || !edges) return SSF_ERR_INVALID_ARG;
    { int rc = solve_usable(h, "ssf_graph_get_edges"); if (rc) return rc; }
    const GraphWs& g = h->graph;
    if (capacity < g.m) { h->err = "ssf_graph_get_edges: " + std::to_string(g.m) + " nodes, room for " + std::to_string(capacity); return SSF_ERR_CAPACITY; }
    { int rc = solve_grow_nodes(h, "ssf_graph_get_edges"); if (rc) return rc; }
    { TimerScope ts(h); launch_graph_edges(h->stream, g.nodes, g.m, g.look, h->solve.edges, "graph_solve"); }
    HCK(hipGetLastError());
    HCK(hipMemcpyAsync(edges, h->solve.edges, 16 * (size_t)g.m, hipMemcpyDeviceToHost, h->stream));
    return sync_collect(h);
}
int ssf_graph_solve(ssf_handle* h, const ssf_graph_solve_params* p, const float* src, const int32_t* t_init, const float* dst, int n_con,
                    ssf_graph_solve_result* result) {
    if (!h || !p || !src || !t_init || !dst) return SSF_ERR_INVALID_ARG;
    const double reals[6] = {p->w_rot, p->w_reg, p->w_con, p->inner_tol, p->outer_tol, p->damping};
    for (double v : reals)
        if (!std::isfinite(v) || v < 0.0) { h->err = "ssf_graph_solve: weights, tolerances and damping must be finite and >= 0"; return SSF_ERR_INVALID_ARG; }
    if (p->max_outer < 1 || p->max_outer > SSF_GRAPH_SOLVE_MAX_OUTER || p->max_inner < 1 || p->inner_check < 1) {
        h->err = "ssf_graph_solve: needs 1 <= max_outer <= " + std::to_string(SSF_GRAPH_SOLVE_MAX_OUTER) + ", max_inner >= 1 and inner_check >= 1";
        return SSF_ERR_INVALID_ARG;
    }
    if (n_con < 1 || n_con > SSF_GRAPH_SOLVE_MAX_CONSTRAINTS) { h->err = "ssf_graph_solve: needs between 1 and 2^20 constraints"; return SSF_ERR_INVALID_ARG; }
    for (size_t i = 0; i < 3 * (size_t)n_con; i++)
        if (!std::isfinite(src[i]) || !std::isfinite(dst[i])) { h->err = "ssf_graph_solve: constraint " + std::to_string(i / 3) + " is not finite"; return SSF_ERR_INVALID_ARG; }
    { int rc = solve_usable(h, "ssf_graph_solve"); if (rc) return rc; }
    const GraphWs& g = h->graph;
    SolveWs& s = h->solve;
    const int m = g.m, nc = n_con, nbn = (m + 255) / 256, nbc = (nc + 255) / 256;
    s.solved = false;
    { int rc = solve_grow_nodes(h, "ssf_graph_solve"); if (rc) return rc; }
    if ((size_t)nc > s.con_cap) {
        const size_t cap = (size_t)nc + (size_t)nc / 4;
        if (!s.bufs.grow({{(void**)&s.src, 12 * cap}, {(void**)&s.dst, 12 * cap}, {(void**)&s.t0, 4 * cap}, {(void**)&s.w4, 16 * cap},
                          {(void**)&s.idx4, 16 * cap}, {(void**)&s.y_con, 24 * cap}, {(void**)&s.e_con, 8 * ((cap + 255) / 256)}})) {
            h->err = "ssf_graph_solve: allocation of the constraint buffers failed"; return SSF_ERR_DEVICE;
        }
        s.con_cap = cap;
    }
    const size_t items = 4 * (size_t)std::max(m, nc);
    if (items > s.item_cap) {
        const size_t cap = items + items / 4, nb = (cap + 2047) / 2048;
        if (!s.bufs.grow({{(void**)&s.key_a, 4 * cap}, {(void**)&s.key_b, 4 * cap}, {(void**)&s.slot_a, 4 * cap}, {(void**)&s.slot_b, 4 * cap},
                          {(void**)&s.cnt, 4 * (256 * nb + 1)}, {(void**)&s.in_list, 4 * cap}, {(void**)&s.con_list, 4 * cap}})) {
            h->err = "ssf_graph_solve: allocation of the sort buffers failed"; return SSF_ERR_DEVICE;
        }
        s.item_cap = cap;
    }
    hipStream_t st = h->stream;
    TimerScope ts(h);
    HCK(hipMemcpyAsync(s.src, src, 12 * (size_t)nc, hipMemcpyHostToDevice, st));
    HCK(hipMemcpyAsync(s.dst, dst, 12 * (size_t)nc, hipMemcpyHostToDevice, st));
    HCK(hipMemcpyAsync(s.t0, t_init, 4 * (size_t)nc, hipMemcpyHostToDevice, st));
    // setup: edges, the constraints' binding, the two transposed lists
    launch_graph_edges(st, g.nodes, m, g.look, s.edges, "graph_solve");
    launch_graph_bind_points(st, s.src, s.t0, nc, g.nodes, m, g.look, s.w4, s.idx4, "graph_solve");
    HCK(hipGetLastError());
    const int passes = m <= 256 ? 1 : m <= 65536 ? 2 : 3;
    // each sort ping-pongs between a list buffer of its own and one of the shared slot buffers, so both sorted lists stay where
    // the sort left them (the sorted keys are consumed by k_solve_offsets before the next sort reuses key_a / key_b)
    const uint32_t* lists[2] = {nullptr, nullptr};
    for (int which = 0; which < 2; which++) {
        const int n = which == 0 ? 4 * m : 4 * nc;
        const int32_t* keys = which == 0 ? s.edges : s.idx4;
        uint32_t* sa = which == 0 ? s.in_list : s.con_list; uint32_t* sb = which == 0 ? s.slot_b : s.slot_a;
        const int out = launch_graph_sort(st, n, n, 0, passes, keys, nullptr, s.cnt, s.key_a, sa, s.key_b, sb, "graph_solve");
        HCK(hipGetLastError());
        ScopedKernel sk("graph_solve", st);
        hipLaunchKernelGGL(k_solve_offsets, dim3((m + 256) / 256), dim3(256), 0, st, out == 0 ? s.key_a : s.key_b, n, m, which == 0 ? s.in_off : s.con_off);
        lists[which] = out == 0 ? sa : sb;
    }
    HCK(hipGetLastError());

    SolveArgs a{};
    a.nodes = g.nodes; a.edges = reinterpret_cast<const int4*>(s.edges); a.m = m; a.nc = nc; a.nbn = nbn; a.nbc = nbc;
    a.in_off = s.in_off; a.in_list = lists[0]; a.con_off = s.con_off; a.con_list = lists[1];
    a.src = s.src; a.dst = s.dst; a.w4 = reinterpret_cast<const float4*>(s.w4); a.idx4 = reinterpret_cast<const int4*>(s.idx4);
    a.x = s.x; a.b = s.b; a.D = s.D; a.delta = s.delta; a.r = s.r; a.z = s.z; a.q = s.q; a.y_rot = s.y_rot; a.y_reg = s.y_reg; a.y_con = s.y_con;
    const size_t nbcap = (s.node_cap + 255) / 256;
    double* rho[2] = {s.part + 2 * nbcap, s.part + 3 * nbcap};
    a.e_rot = s.part; a.e_reg = s.part + nbcap; a.e_con = s.e_con; a.pq = s.part + 4 * nbcap; a.hist = s.part + 5 * nbcap;
    a.rot = s.rot; a.trans = s.trans;
    a.sr = std::sqrt(p->w_rot); a.sg = std::sqrt(p->w_reg); a.sc = std::sqrt(p->w_con); a.damping = p->damping;
    double* pbuf[2] = {s.p0, s.p1};
    const int nbmax = std::max(nbn, nbc);
    std::vector<double> hp(2 * (size_t)nbn + (size_t)nbc + SOLVE_HIST);

    // residuals at x and E = (E_rot + E_reg) + E_con, its parts in e[1..3]
    auto energy = [&](double e[4]) -> int {
        { ScopedKernel sk("graph_solve", st); hipLaunchKernelGGL(k_solve_residual, dim3(nbmax), dim3(256), 0, st, a); }
        HCK(hipGetLastError());
        HCK(hipMemcpyAsync(hp.data(), a.e_rot, 8 * (size_t)nbn, hipMemcpyDeviceToHost, st));
        HCK(hipMemcpyAsync(hp.data() + nbn, a.e_reg, 8 * (size_t)nbn, hipMemcpyDeviceToHost, st));
        HCK(hipMemcpyAsync(hp.data() + 2 * nbn, a.e_con, 8 * (size_t)nbc, hipMemcpyDeviceToHost, st));
        HCK(hipStreamSynchronize(st));
        e[1] = host_ordered_sum(hp.data(), nbn); e[2] = host_ordered_sum(hp.data() + nbn, nbn); e[3] = host_ordered_sum(hp.data() + 2 * nbn, nbc);
        e[0] = (e[1] + e[2]) + e[3];
        return SSF_OK;
    };
    ssf_graph_solve_result res{};
    { ScopedKernel sk("graph_solve", st); hipLaunchKernelGGL(k_solve_init, dim3(nbn), dim3(256), 0, st, s.x, m); }
    double E[4], En[4];
    { int rc = energy(E); if (rc) return rc; }
    res.e_before = E[0]; res.inner_end = SSF_GRAPH_SOLVE_END_ZERO;
    const double tol2 = p->inner_tol * p->inner_tol;
    for (int outer = 0; outer < p->max_outer; outer++) {
        { ScopedKernel sk("graph_solve", st); hipLaunchKernelGGL(k_solve_jt<true>, dim3(nbn), dim3(256), 0, st, a, (const double*)nullptr, rho[0]); }
        HCK(hipGetLastError());
        HCK(hipMemcpyAsync(hp.data(), rho[0], 8 * (size_t)nbn, hipMemcpyDeviceToHost, st));
        HCK(hipStreamSynchronize(st));
        const double rho0 = host_ordered_sum(hp.data(), nbn);
        int it = 0, end = SSF_GRAPH_SOLVE_END_ZERO;
        bool running = rho0 > 0.0;
        while (running) {
            // up to the next multiple of inner_check, max_inner, or the history's length
            const int chunk = std::min(std::min(p->inner_check - it % p->inner_check, p->max_inner - it), SOLVE_HIST);
            {
                ScopedKernel sk("graph_solve", st);
                for (int k = 0; k < chunk; k++, it++) {
                    const int cur = it & 1;
                    hipLaunchKernelGGL(k_solve_jp, dim3(nbmax), dim3(256), 0, st, a, it == 0 ? 1 : 0, rho[cur], rho[cur ^ 1], pbuf[cur ^ 1], pbuf[cur]);
                    hipLaunchKernelGGL(k_solve_jt<false>, dim3(nbn), dim3(256), 0, st, a, (const double*)pbuf[cur], a.pq);
                    hipLaunchKernelGGL(k_solve_update, dim3(nbn), dim3(256), 0, st, a, (const double*)pbuf[cur], (const double*)rho[cur], rho[cur ^ 1], k);
                }
            }
            HCK(hipGetLastError());
            HCK(hipMemcpyAsync(hp.data(), rho[it & 1], 8 * (size_t)nbn, hipMemcpyDeviceToHost, st));
            HCK(hipMemcpyAsync(hp.data() + nbn, a.hist, 8 * (size_t)chunk, hipMemcpyDeviceToHost, st));
            HCK(hipStreamSynchronize(st));
            for (int k = 0; k < chunk; k++) {
                const double pq = hp[nbn + k];
                if (!(pq > 0.0 && std::isfinite(pq))) { it = it - chunk + k; end = SSF_GRAPH_SOLVE_END_BREAKDOWN; running = false; break; }
            }
            if (!running) break;
            const double rho_now = host_ordered_sum(hp.data(), nbn);
            if (it % p->inner_check == 0 && rho_now <= tol2 * rho0) { end = SSF_GRAPH_SOLVE_END_TOLERANCE; break; }
            if (it >= p->max_inner) { end = SSF_GRAPH_SOLVE_END_MAX_INNER; break; }
        }
        { ScopedKernel sk("graph_solve", st); hipLaunchKernelGGL(k_solve_step, dim3(nbn), dim3(256), 0, st, a); }
        { int rc = energy(En); if (rc) return rc; }
        res.inner[outer] = it; res.inner_end = end; res.outer = outer + 1;
        const bool done = std::fabs(E[0] - En[0]) <= p->outer_tol * E[0];
        std::memcpy(E, En, sizeof(E));
        if (done) break;
    }
    res.e_after = E[0]; res.e_rot = E[1]; res.e_reg = E[2]; res.e_con = E[3];
    { int rc = sync_collect(h); if (rc) return rc; }
    s.solved = true; s.gen = g.gen;
    if (result) *result = res;
    return SSF_OK;
}
static int solved_usable(ssf_handle* h, const char* who) {
    { int rc = graph_usable(h, who); if (rc) return rc; }
    if (!h->solve.solved || h->solve.gen != h->graph.gen) { h->err = std::string(who) + ": no transforms have been solved on this graph (ssf_graph_solve)"; return SSF_ERR_STATE; }
    return SSF_OK;
}
int ssf_graph_get_transforms(ssf_handle* h, float* rotations, float* translations, int capacity) {
    if (!h || (!rotations && !translations)) return SSF_ERR_INVALID_ARG;
    { int rc = solved_usable(h, "ssf_graph_get_transforms"); if (rc) return rc; }
    const size_t m = h->graph.m;
    if (capacity < h->graph.m) { h->err = "ssf_graph_get_transforms: " + std::to_string(m) + " nodes, room for " + std::to_string(capacity); return SSF_ERR_CAPACITY; }
    if (rotations) HCK(hipMemcpyAsync(rotations, h->solve.rot, 36 * m, hipMemcpyDeviceToHost, h->stream));
    if (translations) HCK(hipMemcpyAsync(translations, h->solve.trans, 12 * m, hipMemcpyDeviceToHost, h->stream));
    HCK(hipStreamSynchronize(h->stream));
    return SSF_OK;
}
int ssf_graph_apply_solved(ssf_handle* h) {
    if (!h) return SSF_ERR_INVALID_ARG;
    { int rc = solved_usable(h, "ssf_graph_apply_solved"); if (rc) return rc; }
    drop_shard_sizes(h);
    h->ahead.valid = false;
    const GraphWs& g = h->graph;
    float* d_nodes;
    DevTemps tmp;
    HCK(tmp.take(&d_nodes, 64 * (size_t)g.m));
    return deform_dense(h, g.m, g.npos3, h->solve.rot, h->solve.trans, d_nodes, g.w4, g.idx4);
}
}  // extern "C"
