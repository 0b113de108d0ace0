// ssf_upkeep.hip -- the kernels that run BETWEEN frames: loop-closure registration (DenseRegistration::align, one single-workgroup
// launch per iteration with exact sums) and fern codes (a gather), applyDeformation (core/src/deformation_graph_kernels.cu:27-73),
// the getters' orientation pack and Lab refresh, re-homing of a sharded map, compaction of the out-of-view store.
#include "ssf_rows.hpp"

namespace ssf {

// ---- loop-closure registration (DenseRegistration::align) -----------------------------------------------------
// makeCorrespondences, dense_registration_kernels.cu:27-100, for one source supersurfel
__device__ __forceinline__ bool align_pair(const Cam& cam, const float* __restrict__ spos, const float* __restrict__ slab,
                                           const float* __restrict__ snrm, const float* __restrict__ sconf, int id,
                                           const SurfelSoA& frame, const int32_t* __restrict__ label,
                                           const float* __restrict__ plane_depth, const M3& R, const V3& t,
                                           V3& pv, V3& sn, V3& tp, V3& tn) {
    if (sconf && !(sconf[id] > 0.0f)) return false;
    pv = add(m3_mulv(R, ld3(spos, id)), t);
    const int u = pixel_round(pv.x * cam.fx / pv.z + cam.cx), v = pixel_round(pv.y * cam.fy / pv.z + cam.cy);
    if (!(u >= 0 && u < cam.W && v >= 0 && v < cam.H)) return false;
    const size_t q = (size_t)v * cam.W + u;
    const int tid = label[q];
    if (!(frame.conf[tid] > 0.0f)) return false;
    const float dist_color = len3(sub(ld3(slab, id), ld3(frame.lab, tid)));
    const float td = plane_depth[q];
    if (!isfinite(td)) return false;
    sn = unit3(ld3(snrm, id));
    sn = unit3(m3_mulv(R, sn));
    tn = unit3(ld3(frame.r2, tid));
    tp = v3(td * ((float)u - cam.cx) / cam.fx, td * ((float)v - cam.cy) / cam.fy, td);
    return dist_color < 20.0f && len3(sub(pv, tp)) < 0.1f && fabsf(dot3(sn, tn)) > 0.8f;
}
// One iteration of align in ONE single-workgroup launch: pair count + centroids, scale, normalised symmetric
// point-to-plane system (buildSymmetricPoint2PlaneSystem, dense_registration_kernels.cuh:87-173).  The reference
// compacts the valid pairs (thrust::remove_if) to feed three reductions; all sums here are exact integers, so the
// pairs are simply re-derived in each phase (a keyframe has ~S sources: the whole problem is LDS-sized).
// out: [0..28] record as k_icp, [29] pairs, [30..32] source centroid bits, [33..35] target centroid bits, [36] scale bits
__global__ __launch_bounds__(1024) void k_align(Cam cam, const float* __restrict__ spos, const float* __restrict__ slab,
                                                const float* __restrict__ snrm, const float* __restrict__ sconf, int n,
                                                SurfelSoA frame, const int32_t* __restrict__ label,
                                                const float* __restrict__ plane_depth, Rt T, long long* __restrict__ out) {
    __shared__ unsigned long long acc[8];
    __shared__ unsigned long long red[29 * 16];
    __shared__ float s_c[7];
    __shared__ int s_pairs;
    for (int i = threadIdx.x; i < 29 * 16; i += blockDim.x) red[i] = 0ull;
    if (threadIdx.x < 8) acc[threadIdx.x] = 0ull;
    __syncthreads();
    const M3 R = T.R; const V3 t = T.t;
    V3 pv, sn, tp, tn;
    for (int id = threadIdx.x; id < n; id += blockDim.x) {
        if (!align_pair(cam, spos, slab, snrm, sconf, id, frame, label, plane_depth, R, t, pv, sn, tp, tn)) continue;
        atomicAdd(&acc[0], (unsigned long long)fx64((double)pv.x, SSF_ALIGN_SCALE_POS, SSF_ALIGN_LIM));
        atomicAdd(&acc[1], (unsigned long long)fx64((double)pv.y, SSF_ALIGN_SCALE_POS, SSF_ALIGN_LIM));
        atomicAdd(&acc[2], (unsigned long long)fx64((double)pv.z, SSF_ALIGN_SCALE_POS, SSF_ALIGN_LIM));
        atomicAdd(&acc[3], (unsigned long long)fx64((double)tp.x, SSF_ALIGN_SCALE_POS, SSF_ALIGN_LIM));
        atomicAdd(&acc[4], (unsigned long long)fx64((double)tp.y, SSF_ALIGN_SCALE_POS, SSF_ALIGN_LIM));
        atomicAdd(&acc[5], (unsigned long long)fx64((double)tp.z, SSF_ALIGN_SCALE_POS, SSF_ALIGN_LIM));
        atomicAdd(&acc[6], 1ull);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int pairs = (int)acc[6];
        s_pairs = pairs;
        for (int i = 0; i < 6; i++) s_c[i] = (float)((double)(long long)acc[i] / SSF_ALIGN_SCALE_POS) / (float)pairs;
        out[29] = pairs;
    }
    __syncthreads();
    const int pairs = s_pairs;
    if (pairs < 100) {                                       // the host stops here (dense_registration.cu:133-138)
        if (threadIdx.x < 29) out[threadIdx.x] = 0;
        if (threadIdx.x >= 30 && threadIdx.x < 37) out[threadIdx.x] = 0;
        return;
    }
    const V3 cs = v3(s_c[0], s_c[1], s_c[2]), ct = v3(s_c[3], s_c[4], s_c[5]);
    for (int id = threadIdx.x; id < n; id += blockDim.x) {
        if (!align_pair(cam, spos, slab, snrm, sconf, id, frame, label, plane_depth, R, t, pv, sn, tp, tn)) continue;
        const V3 a = v3(tp.x - ct.x, tp.y - ct.y, tp.z - ct.z), b = v3(pv.x - cs.x, pv.y - cs.y, pv.z - cs.z);
        atomicAdd(&acc[7], (unsigned long long)fx64((double)((a.x * a.x + a.y * a.y) + a.z * a.z), SSF_ALIGN_SCALE_D2, SSF_ALIGN_LIM));
        atomicAdd(&acc[7], (unsigned long long)fx64((double)((b.x * b.x + b.y * b.y) + b.z * b.z), SSF_ALIGN_SCALE_D2, SSF_ALIGN_LIM));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float sv = (float)((double)(long long)acc[7] / SSF_ALIGN_SCALE_D2);
        sv = sqrtf(sv / (2.0f * (float)pairs));
        s_c[6] = 1.0f / sv;
    }
    __syncthreads();
    const float sc = s_c[6];
    const int slot = lane() & 15;
    for (int id = threadIdx.x; id < n; id += blockDim.x) {
        if (!align_pair(cam, spos, slab, snrm, sconf, id, frame, label, plane_depth, R, t, pv, sn, tp, tn)) continue;
        const V3 ps = scale(sc, sub(pv, cs)), pt = scale(sc, sub(tp, ct));
        const V3 ns = unit3(sn), nt = unit3(tn);
        const V3 d = sub(pt, ps), c1 = cross3(pt, ns), c2 = cross3(ps, nt);
        const float dn1 = dot3(d, ns), dn2 = dot3(d, nt);
        const float x1[6] = {c1.x, c1.y, c1.z, ns.x, ns.y, ns.z};
        const float x2[6] = {c2.x, c2.y, c2.z, nt.x, nt.y, nt.z};
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = i; j < 6; j++, k++)
                atomicAdd(&red[k * 16 + slot], (unsigned long long)(long long)fx32(x1[i] * x1[j] + x2[i] * x2[j], 1048576.0f));
#pragma unroll
        for (int i = 0; i < 6; i++)
            atomicAdd(&red[(21 + i) * 16 + slot], (unsigned long long)(long long)fx32(dn1 * x1[i] + dn2 * x2[i], 16777216.0f));
        atomicAdd(&red[27 * 16 + slot], (unsigned long long)fx64((double)(dn2 * dn2), 17592186044416.0, 4611686018427387904.0));
        atomicAdd(&red[28 * 16 + slot], 1ull);
    }
    __syncthreads();
    if (threadIdx.x < 29) {
        unsigned long long tot = 0;
        for (int sidx = 0; sidx < 16; sidx++) tot += red[threadIdx.x * 16 + sidx];
        out[threadIdx.x] = (long long)tot;
    }
    if (threadIdx.x < 7) out[30 + threadIdx.x] = (long long)__float_as_uint(s_c[threadIdx.x]);
}

// computeCodes_kernel, ferns_kernels.cu:48-70 (point sampling, clamp: texture_impl.hpp:43-46)
__global__ void k_fern_codes(const uint8_t* __restrict__ rgb, const float* __restrict__ depth, int W, int H,
                             const uint32_t* __restrict__ fpos, const uint8_t* __restrict__ frgb,
                             const float* __restrict__ fdepth, int n, uint8_t* __restrict__ codes) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int x = (int)min(fpos[2 * k], (uint32_t)W - 1u), y = (int)min(fpos[2 * k + 1], (uint32_t)H - 1u);
    const size_t q = (size_t)y * W + x;
    uint8_t r = 0;
    r |= rgb[3 * q] > frgb[3 * k] ? 1 : 0;
    r |= rgb[3 * q + 1] > frgb[3 * k + 1] ? 2 : 0;
    r |= rgb[3 * q + 2] > frgb[3 * k + 2] ? 4 : 0;
    r |= depth[q] > fdepth[k] ? 8 : 0;
    codes[k] = r;
}
// ---- re-homing of a sharded map after positions changed outside a frame (ssf_rehome_begin / _end in ssf.h) ---------------
// over the dense logical view [visible | out of view]: a row leaves when it is valid and its position belongs to another
// rank's tile.  Three launches: per-block counts (staying rows, leaving rows, staying rows of the visible block), their
// exclusive scan by one workgroup (totals -> tot3), and the ordered scatter: staying rows close ranks in `stay`, leaving
// rows become migrant-table records (word 1 = 1: the row sat in the visible block) in logical order.
__device__ __forceinline__ int rehome_class(const SurfelSoA& D, int i, int n, int rank, int nranks, float tile) {
    if (i >= n) return 2;                                          // 0 stays, 1 leaves
    return (D.conf[i] > 0.0f && tile_owner(ld3(D.pos, i), nranks, tile) != rank) ? 1 : 0;
}
__global__ __launch_bounds__(256) void k_rehome_count(SurfelSoA D, int n, int n_visible, int rank, int nranks, float tile, uint32_t* __restrict__ bc) {
    __shared__ int part[4][3];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = rehome_class(D, i, n, rank, nranks, tile);
    const int k0 = __popcll(__ballot(c == 0)), k1 = __popcll(__ballot(c == 1)), k2 = __popcll(__ballot(c == 0 && i < n_visible));
    if (lane() == 0) { part[threadIdx.x >> 6][0] = k0; part[threadIdx.x >> 6][1] = k1; part[threadIdx.x >> 6][2] = k2; }
    __syncthreads();
    if (threadIdx.x < 3) bc[3 * blockIdx.x + threadIdx.x] = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}
__global__ __launch_bounds__(1024) void k_rehome_scan(uint32_t* __restrict__ bc, int nblocks, int* __restrict__ tot3) {
    __shared__ uint32_t tot[3];
    workgroup_scan<3, uint32_t>(bc, nblocks, nullptr, tot);
    if (threadIdx.x < 3) tot3[threadIdx.x] = (int)tot[threadIdx.x];
}
__global__ __launch_bounds__(256) void k_rehome_scatter(SurfelSoA D, int n, int n_visible, int rank, int nranks, float tile,
                                                        const uint32_t* __restrict__ bc, SurfelSoA stay, int32_t* __restrict__ table, int table_rows) {
    __shared__ int part[2][4];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = rehome_class(D, i, n, rank, nranks, tile);
    const int r0 = block_rank256(c == 0, part[0]), r1 = block_rank256(c == 1, part[1]);      // (before any thread leaves)
    if (c > 1) return;
    const size_t j = (size_t)bc[3 * blockIdx.x + c] + (c == 0 ? r0 : r1);
    if (c == 0) { copy_row(D, (size_t)i, stay, j); return; }
    if (j >= (size_t)table_rows) return;                               // (the host sees the total and reports SSF_ERR_CAPACITY)
    const RowRegs r = load_row(D, (size_t)i);
    int32_t* o = table + (size_t)SSF_MIGRANT_WORDS * j;
    o[0] = tile_owner(r.pos, nranks, tile) + 1; o[1] = i < n_visible ? 1 : 0;
    migrant_pack(r, o);
}
// records [0, n) of a packed table -> rows [base, base + n) of D (the Lab cache is rebuilt from the colour)
__global__ __launch_bounds__(256) void k_rehome_unpack(const int32_t* __restrict__ table, int n, SurfelSoA D, int base) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    RowRegs row;
    migrant_unpack(table + (size_t)SSF_MIGRANT_WORDS * j, row);
    store_row(D, (size_t)base + j, row);
}
void launch_rehome_split(hipStream_t st, SurfelSoA dense, int n, int n_visible, int rank, int nranks, float tile, uint32_t* bc, int* tot3,
                         SurfelSoA stay, int32_t* table, int table_rows) {
    const int nb = (n + 255) / 256;
    if (nb <= 0) return;
    hipLaunchKernelGGL(k_rehome_count, dim3(nb), dim3(256), 0, st, dense, n, n_visible, rank, nranks, tile, bc);
    hipLaunchKernelGGL(k_rehome_scan, dim3(1), dim3(1024), 0, st, bc, nb, tot3);
    hipLaunchKernelGGL(k_rehome_scatter, dim3(nb), dim3(256), 0, st, dense, n, n_visible, rank, nranks, tile, bc, stay, table, table_rows);
}
void launch_rehome_unpack(hipStream_t st, const int32_t* table, int n, SurfelSoA dst, int base) {
    if (n > 0) hipLaunchKernelGGL(k_rehome_unpack, dim3((n + 255) / 256), dim3(256), 0, st, table, n, dst, base);
}

// ---- out-of-view store maintenance: stable compaction of the live rows into the other store -------------------
// (head and tail come from the device counters: the launches are enqueued before the host knows them)
__global__ __launch_bounds__(256) void k_oov_count(OovStore O, uint32_t* __restrict__ bc, const Counters* __restrict__ cnt) {
    __shared__ int part[4];
    size_t phys;
    const int k = block_count256(span_live(O.live, cnt->oov_head, cnt->oov_tail, blockIdx.x * 256u + threadIdx.x, phys), part);
    if (threadIdx.x == 0) bc[blockIdx.x] = k;
}
__global__ __launch_bounds__(1024) void k_oov_scan(uint32_t* __restrict__ bc, int nb_upper, const Counters* __restrict__ cnt) {
    __shared__ uint32_t tot[1];
    workgroup_scan<1, uint32_t>(bc, min(nb_upper, (cnt->oov_tail - cnt->oov_head + 255) / 256), nullptr, tot);
}
__global__ __launch_bounds__(256) void k_oov_compact(OovStore A, OovStore B, const uint32_t* __restrict__ bc, int new_head,
                                                     const Counters* __restrict__ cnt) {
    __shared__ int part[4];
    size_t phys;
    const bool lv = span_live(A.live, cnt->oov_head, cnt->oov_tail, blockIdx.x * 256u + threadIdx.x, phys);
    const int before = block_rank256(lv, part);
    if (lv) {
        const size_t j = (size_t)new_head + bc[blockIdx.x] + before;
        copy_row(A.rows, phys, B.rows, j);
        B.live[j] = 1;
    }
}
__global__ void k_oov_set_span(Counters* cnt, int new_head) { cnt->oov_head = new_head; cnt->oov_tail = new_head + cnt->oov_live; }

// the three row streams of the orientations -> packed row-major Mat33 (the reference's layout, supersurfels.hpp:37)
__global__ void k_pack_orient(SurfelSoA s, int n, float* __restrict__ out9) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 a = ld3(s.r0, i), b = ld3(s.r1, i), c = ld3(s.r2, i);
    float* o = out9 + 9 * (size_t)i;
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = b.x; o[4] = b.y; o[5] = b.z; o[6] = c.x; o[7] = c.y; o[8] = c.z;
}
void launch_pack_orient(hipStream_t st, SurfelSoA s, int n, float* out9) {
    if (n > 0) hipLaunchKernelGGL(k_pack_orient, dim3((n + 255) / 256), dim3(256), 0, st, s, n, out9);
}
__global__ void k_lab_refresh(SurfelSoA s, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) st3(s.lab, i, rgb_to_lab(ld3(s.col, i)));
}

// ---- deformation apply ("next" row) -----------------------------------------------------------------
// rotMatToQuat matrix_math.cuh:529-618; quatToRotMat :512-527 (its wy = q.w*q.z is reproduced)
// The nodes of the deformation graph as ONE 64-BYTE RECORD each (round 6): (g.xyz, R00) (t.xyz, R01) (R02, R10, R11, R12) (R20, R21,
// R22, 0) -- a supersurfel's four nodes are 4 x 4 whole 16-byte loads, each record one aligned 64-byte piece of a line, the table
// 1.28 MB at 20 k nodes.  The node's quaternion (rotMatToQuat: four branches, an IEEE sqrt and a divide) is worked out per row and
// node, as the reference does (deformation_graph_kernels.cu:44-52) -- the same operations on the same operands, so the same bits.
// Measured (tools/deform_probe.py, profiles/deformation_r06.txt, 1 M rows, N / 50 nodes): rounds 2-5 kept a 96-byte record with the
// quaternion precomputed (five gathers per node): 75 us with uniformly random node indices, of which 35 us were the gathers (nodes
// 0 / 1 only: 40 us) -- this form: 60 us; records padded to 128 bytes: 85 (the table's footprint in L2 matters, not lines per
// record); non-temporal row accesses: no change; one or two nodes per round at 8 / 5 waves per SIMD: 68-88.  With node indices that
// follow the row order (what a time-ordered graph gives rows in arrival order) every form runs at 40-42 us = 0.52-0.55 of HBM peak.
__global__ __launch_bounds__(256) void k_pack_nodes(int m, const float* __restrict__ npos, const float* __restrict__ nrot,
                                                    const float* __restrict__ ntrans, float4* __restrict__ nodes) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const V3 g = ld3(npos, k), t = ld3(ntrans, k);
    float4* o = nodes + 4 * (size_t)k;
    o[0] = make_float4(g.x, g.y, g.z, nrot[9 * k]); o[1] = make_float4(t.x, t.y, t.z, nrot[9 * k + 1]);
    o[2] = make_float4(nrot[9 * k + 2], nrot[9 * k + 3], nrot[9 * k + 4], nrot[9 * k + 5]);
    o[3] = make_float4(nrot[9 * k + 6], nrot[9 * k + 7], nrot[9 * k + 8], 0.f);
}
__global__ __launch_bounds__(256) void k_deformation(SurfelSoA M, int n, const float4* __restrict__ nodes,
                                                     const float* __restrict__ w4, const int32_t* __restrict__ idx4) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 pi = ld3(M.pos, i);
    const int4 id = reinterpret_cast<const int4*>(idx4)[i];
    const float4 w = reinterpret_cast<const float4*>(w4)[i];
    const int node[4] = {id.x, id.y, id.z, id.w};
    const float wv[4] = {w.x, w.y, w.z, w.w};
    float4 rec[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int j = 0; j < 4; j++) rec[k][j] = nodes[4 * (size_t)node[k] + j];       // all sixteen gathers in one round
    V3 po = v3(0, 0, 0);
    float bq[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float wk = wv[k];
        const V3 gk = v3(rec[k][0].x, rec[k][0].y, rec[k][0].z), tk = v3(rec[k][1].x, rec[k][1].y, rec[k][1].z);
        const M3 Rk = m3(v3(rec[k][0].w, rec[k][1].w, rec[k][2].x), v3(rec[k][2].y, rec[k][2].z, rec[k][2].w),
                         v3(rec[k][3].x, rec[k][3].y, rec[k][3].z));
        // rot_to_quat (ssf_math.hpp) with its result in named scalars: through the array the compiler kept it in scratch
        float s_, qx, qy, qz, qw; const float tr = (Rk.r0.x + Rk.r1.y) + Rk.r2.z;
        if (tr > 0) { s_ = sqrtf(tr + 1); qw = 0.5f * s_; s_ = 0.5f / s_; qx = (Rk.r2.y - Rk.r1.z) * s_; qy = (Rk.r0.z - Rk.r2.x) * s_; qz = (Rk.r1.x - Rk.r0.y) * s_; }
        else {
            int ii = 0;
            if (Rk.r1.y > Rk.r0.x) ii = 1;
            if (Rk.r2.z > Rk.r0.x || Rk.r2.z > Rk.r1.y) ii = 2;
            if (ii == 0) { s_ = sqrtf(((1.0f + Rk.r0.x) - Rk.r1.y) - Rk.r2.z); qx = 0.5f * s_; s_ = 0.5f / s_; qw = (Rk.r2.y - Rk.r1.z) * s_; qy = (Rk.r0.y + Rk.r1.x) * s_; qz = (Rk.r0.z + Rk.r2.x) * s_; }
            else if (ii == 1) { s_ = sqrtf(((1.0f + Rk.r1.y) - Rk.r0.x) - Rk.r2.z); qy = 0.5f * s_; s_ = 0.5f / s_; qw = (Rk.r0.z - Rk.r2.x) * s_; qx = (Rk.r0.y + Rk.r1.x) * s_; qz = (Rk.r1.z + Rk.r2.y) * s_; }
            else { s_ = sqrtf(((1.0f + Rk.r2.z) - Rk.r0.x) - Rk.r1.y); qz = 0.5f * s_; s_ = 0.5f / s_; qw = (Rk.r1.x - Rk.r0.y) * s_; qx = (Rk.r0.z + Rk.r2.x) * s_; qy = (Rk.r1.z + Rk.r2.y) * s_; }
        }
        po = add(po, scale(wk, add(add(m3_mulv(Rk, sub(pi, gk)), gk), tk)));
        bq[0] += wk * qx; bq[1] += wk * qy; bq[2] += wk * qz; bq[3] += wk * qw;
    }
    const float len = sqrtf(((bq[0] * bq[0] + bq[1] * bq[1]) + bq[2] * bq[2]) + bq[3] * bq[3]);
    const float inv = 1.0f / len;
#pragma unroll
    for (int a = 0; a < 4; a++) bq[a] *= inv;
    const M3 av = quat_to_rot_quirk(bq);
    const M3 avT = m3_transpose(av);
    st3(M.r0, i, row_mul(ld3(M.r0, i), avT));
    st3(M.r1, i, row_mul(ld3(M.r1, i), avT));
    st3(M.r2, i, row_mul(ld3(M.r2, i), avT));
    st6(M.shape, i, rot_sym(av, ld6(M.shape, i)));
    st3(M.pos, i, po);
}

// ---- launchers -----------------------------------------------------------------------------------
void launch_oov_compact(hipStream_t st, OovStore src, OovStore dst, int span_upper, int new_head, uint32_t* bc_oov, Counters* cnt,
                        int set_span) {
    const int nb = (span_upper + 255) / 256;
    ScopedKernel sk("oov_compact", st);
    if (nb > 0) {
        hipLaunchKernelGGL(k_oov_count, dim3(nb), dim3(256), 0, st, src, bc_oov, cnt);
        hipLaunchKernelGGL(k_oov_scan, dim3(1), dim3(1024), 0, st, bc_oov, nb, cnt);
        hipLaunchKernelGGL(k_oov_compact, dim3(nb), dim3(256), 0, st, src, dst, bc_oov, new_head, cnt);
    }
    if (set_span) hipLaunchKernelGGL(k_oov_set_span, dim3(1), dim3(1), 0, st, cnt, new_head);
}
void launch_align(hipStream_t st, const Cam& cam, const float* spos, const float* slab, const float* snrm, const float* sconf,
                  int n, SurfelSoA frame, const int32_t* label, const float* plane_depth, Rt T, long long* out40) {
    ScopedKernel sk("align_iteration", st);
    hipLaunchKernelGGL(k_align, dim3(1), dim3(1024), 0, st, cam, spos, slab, snrm, sconf, n, frame, label, plane_depth, T, out40);
}
void launch_fern_codes(hipStream_t st, const uint8_t* rgb, const float* depth, int W, int H, const uint32_t* fpos,
                       const uint8_t* frgb, const float* fdepth, int n, uint8_t* codes) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_fern_codes, dim3((n + 63) / 64), dim3(64), 0, st, rgb, depth, W, H, fpos, frgb, fdepth, n, codes);
}
void launch_lab_refresh(hipStream_t st, SurfelSoA s, int n) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_lab_refresh, dim3((n + 255) / 256), dim3(256), 0, st, s, n);
}
void launch_deformation(hipStream_t st, SurfelSoA model, int n, int m, const float* npos, const float* nrot,
                        const float* ntrans, float* nodes16, const float* w4, const int32_t* idx4) {
    if (n <= 0) return;
    ScopedKernel sk("apply_deformation", st);
    hipLaunchKernelGGL(k_pack_nodes, dim3((m + 255) / 256), dim3(256), 0, st, m, npos, nrot, ntrans, reinterpret_cast<float4*>(nodes16));
    hipLaunchKernelGGL(k_deformation, dim3((n + 255) / 256), dim3(256), 0, st, model, n, reinterpret_cast<const float4*>(nodes16), w4, idx4);
}

}  // namespace ssf
