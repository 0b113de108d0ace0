// ssf_query.hip -- rows of the model selected on the device by region, age and confidence (include/ssf_query.h) on gfx950.
//
// What is selected is pinned, operation by operation, in include/ssf_query.h (the numpy restatement: tests/query_ref.py).  How:
//   * select  k_query_select: one thread per slot of [visible rows | out-of-view span] (the two stores are read in place, never
//             materialised).  The predicate reads the live flag, position, confidence and stamps of a slot (25 B).  Every wave
//             stores its 64-bit ballot as one word of the MASK (nslots / 64 words); every workgroup stores two counts for its
//             256-slot block -- selected rows and, in the out-of-view span, live rows (the count of k_slots_oov_count) -- and
//             reduces its selected positions to a per-block box (wave shuffles, then four LDS words per bound), which at most
//             six integer atomicMin / atomicMax per block fold into the call's box: the order-preserving integer image of
//             the floats makes the result exact and independent of any order.
//   * scan    k_query_scan: one workgroup, workgroup_scan<2> over the interleaved counts: block offsets of the output, and the
//             out-of-view blocks' live offsets (copied to bc[] for slot_logical256).  The totals and n_selected_visible go
//             into the record the host reads in one copy: the only wait before the gather, and where ssf_query_count ends.
//   * gather  k_query_gather: one thread per slot again.  A block without a selected row leaves at once (two words read); in the
//             others a wave whose mask word is 0 leaves right behind the block-uniform part (slot_logical256).  A selected
//             thread's output row = its block's offset + the popcounts of the mask words of the block's waves in front of it +
//             its rank in its own word: the mask IS the ballot, the predicate is not evaluated again.  Only the streams the
//             caller asked for are read and written (null = skipped, uniform for the launch); the three orientation row
//             streams are packed into the 9-float Mat33 on the way.
// Nothing here writes to the handle's stores, counters or scratch: the working set is QueryWs (ssf_handle.hpp).
#include "ssf_slots.hpp"
#include "ssf_handle.hpp"
#include "../../include/ssf_query.h"

namespace ssf {

// R = 9 floats row-major and t (frame-to-map, ssf_get_pose's layout); r2max = radius * radius; ulim = (float)width - 0.5f
struct QueryArgs {
    float R[9], t[3];
    int region;
    float r2max, half[3], fx, fy, cx, cy, ulim, vlim, zmin, zmax, min_conf;
    int32_t ti0, ti1, tl0, tl1;
};
struct QueryView { QueryArgs q; ModelView model; };              // one kernel argument: the predicate and the rows it looks at
struct QueryOut { float *pos, *col; int32_t* stamps; float *ori, *shape, *dims, *conf; int32_t* index; };   // nullptr = not produced
// the record the host reads: [0] n_selected, [1] live out-of-view rows, [2] n_selected_visible, [3..5] lo, [6..8] hi (encoded)
enum { QREC_WORDS = 9, QREC_LO = 3, QREC_HI = 6 };

// the region test of include/ssf_query.h, steps 2 and 3 (contraction off: one IEEE operation each, in this order)
__device__ __forceinline__ bool query_inside(const QueryArgs& q, float px, float py, float pz) {
    if (q.region == SSF_REGION_ALL) return true;
    const float dx = px - q.t[0], dy = py - q.t[1], dz = pz - q.t[2];
    if (q.region == SSF_REGION_SPHERE) {
        const float r2 = (dx * dx + dy * dy) + dz * dz;
        return r2 <= q.r2max;
    }
    const float* R = q.R;
    const float Cx = (R[0] * dx + R[3] * dy) + R[6] * dz, Cy = (R[1] * dx + R[4] * dy) + R[7] * dz, Cz = (R[2] * dx + R[5] * dy) + R[8] * dz;
    if (q.region == SSF_REGION_BOX) return fabsf(Cx) <= q.half[0] && fabsf(Cy) <= q.half[1] && fabsf(Cz) <= q.half[2];
    if (!(Cz >= q.zmin) || !(Cz <= q.zmax)) return false;
    const float u = (q.fx * Cx) / Cz + q.cx, v = (q.fy * Cy) / Cz + q.cy;
    return u >= -0.5f && u < q.ulim && v >= -0.5f && v < q.vlim;
}

// ---- select: one thread per slot ---------------------------------------------------------------------------------------
// mask[nslots / 64]: the waves' ballots; cnt[2 b], cnt[2 b + 1]: selected rows of block b, live rows of an out-of-view block (0
// for a block of the visible array); rec[QREC_LO..], rec[QREC_HI..]: the box (set to ~0 / 0 by the caller)
__global__ __launch_bounds__(256) void k_query_select(QueryView qv, unsigned long long* __restrict__ mask, uint32_t* __restrict__ cnt,
                                                      uint32_t* __restrict__ rec) {
    __shared__ int part_sel[4], part_live[4];
    __shared__ float red[6][4];
    const QueryArgs& q = qv.q;
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    SurfelSoA src; size_t row;
    const bool have = slot_row(qv.model, s, src, row);
    bool sel = false;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (have) {
        px = src.pos[3 * row]; py = src.pos[3 * row + 1]; pz = src.pos[3 * row + 2];
        const float conf = src.conf[row];
        const int32_t t0 = src.stamps[2 * row], t1 = src.stamps[2 * row + 1];
        sel = finite3(px, py, pz) && conf > q.min_conf && t0 >= q.ti0 && t0 <= q.ti1 && t1 >= q.tl0 && t1 <= q.tl1 &&
              query_inside(q, px, py, pz);
    }
    const unsigned long long m = __ballot(sel);
    if (lane() == 0) mask[s >> 6] = m;
    // the block's box: -0 counts as +0 (x + 0.0f), a lane without a row is neutral
    const float inf = __uint_as_float(0x7F800000u);
    float b[6] = {sel ? px + 0.0f : inf, sel ? py + 0.0f : inf, sel ? pz + 0.0f : inf,
                  sel ? px + 0.0f : -inf, sel ? py + 0.0f : -inf, sel ? pz + 0.0f : -inf};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; a++) { b[a] = fminf(b[a], __shfl_xor(b[a], o, 64)); b[3 + a] = fmaxf(b[3 + a], __shfl_xor(b[3 + a], o, 64)); }
    }
    if (lane() == 0) {
#pragma unroll
        for (int a = 0; a < 6; a++) red[a][threadIdx.x >> 6] = b[a];
    }
    const int nsel = block_count256(sel, part_sel);                   // (its barrier also publishes red)
    int nlive = 0;
    if ((int)blockIdx.x >= qv.model.nbv) nlive = block_count256(have, part_live);      // block-uniform
    if (threadIdx.x == 0) { cnt[2 * blockIdx.x] = (uint32_t)nsel; cnt[2 * blockIdx.x + 1] = (uint32_t)nlive; }
    if (threadIdx.x < 6 && nsel > 0) {
        const float* r = red[threadIdx.x];
        if (threadIdx.x < 3) atomicMin(&rec[QREC_LO + threadIdx.x], float_order_bits(__float_as_uint(fminf(fminf(r[0], r[1]), fminf(r[2], r[3])))));
        else atomicMax(&rec[QREC_HI + threadIdx.x - 3], float_order_bits(__float_as_uint(fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3])))));
    }
}

// ---- scan: block counts -> block offsets (one workgroup of 1024) ------------------------------------------------------------
// cnt[2 nb + 2]: in place; cnt[2 nb], cnt[2 nb + 1] = the totals.  bc[i] = live rows in front of out-of-view block i.
__global__ __launch_bounds__(1024) void k_query_scan(uint32_t* __restrict__ cnt, int nb, int nbv, uint32_t* __restrict__ bc,
                                                     uint32_t* __restrict__ rec) {
    __shared__ uint32_t tot[2];
    workgroup_scan<2, uint32_t>(cnt, nb, nullptr, tot);
    if (threadIdx.x == 0) {
        cnt[2 * nb] = tot[0]; cnt[2 * nb + 1] = tot[1];
        rec[0] = tot[0]; rec[1] = tot[1];
        rec[2] = nbv < nb ? cnt[2 * nbv] : tot[0];                 // selected rows in front of the first out-of-view block
    }
    for (int i = threadIdx.x; i < nb - nbv; i += 1024) bc[i] = cnt[2 * (nbv + i) + 1];
}

// ---- gather: one thread per slot ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_query_gather(ModelView mv, const unsigned long long* __restrict__ mask,
                                                      const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ bc, QueryOut o) {
    __shared__ int part[4];
    const uint32_t off = cnt[2 * blockIdx.x];
    if (cnt[2 * blockIdx.x + 2] == off) return;                     // block-uniform: no row of this block is selected
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    SurfelSoA src; size_t row;
    const bool have = slot_row(mv, s, src, row);
    const int lg = slot_logical256(mv, have, bc, part);
    const int wv = threadIdx.x >> 6;
    const unsigned long long* bm = mask + 4 * (size_t)blockIdx.x;
    const unsigned long long m = bm[wv];
    if (m == 0ull || !((m >> lane()) & 1ull)) return;
    size_t j = off + (uint32_t)__popcll(m & ((1ull << lane()) - 1ull));
    for (int w = 0; w < wv; w++) j += (uint32_t)__popcll(bm[w]);
    if (o.pos) { o.pos[3 * j] = src.pos[3 * row]; o.pos[3 * j + 1] = src.pos[3 * row + 1]; o.pos[3 * j + 2] = src.pos[3 * row + 2]; }
    if (o.col) { o.col[3 * j] = src.col[3 * row]; o.col[3 * j + 1] = src.col[3 * row + 1]; o.col[3 * j + 2] = src.col[3 * row + 2]; }
    if (o.stamps) { o.stamps[2 * j] = src.stamps[2 * row]; o.stamps[2 * j + 1] = src.stamps[2 * row + 1]; }
    if (o.ori) {
        float* q = o.ori + 9 * j;
        const float* r0 = src.r0 + 3 * row; const float* r1 = src.r1 + 3 * row; const float* r2 = src.r2 + 3 * row;
        q[0] = r0[0]; q[1] = r0[1]; q[2] = r0[2]; q[3] = r1[0]; q[4] = r1[1]; q[5] = r1[2]; q[6] = r2[0]; q[7] = r2[1]; q[8] = r2[2];
    }
    if (o.shape) {
#pragma unroll
        for (int k = 0; k < 6; k++) o.shape[6 * j + k] = src.shape[6 * row + k];
    }
    if (o.dims) { o.dims[2 * j] = src.dims[2 * row]; o.dims[2 * j + 1] = src.dims[2 * row + 1]; }
    if (o.conf) o.conf[j] = src.conf[row];
    if (o.index) o.index[j] = lg;
}

// ---- launches -------------------------------------------------------------------------------------------------------
static hipError_t launch_query_select(hipStream_t st, const QueryView& qv, unsigned long long* mask, uint32_t* cnt, uint32_t* rec) {
    ScopedKernel sk("query_select", st);
    hipError_t e = hipMemsetAsync(rec + QREC_LO, 0xFF, 3 * sizeof(uint32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(rec + QREC_HI, 0, 3 * sizeof(uint32_t), st);
    const int nb = qv.model.nbv + qv.model.nbo;
    if (e == hipSuccess && nb > 0) hipLaunchKernelGGL(k_query_select, dim3(nb), dim3(256), 0, st, qv, mask, cnt, rec);
    return e;
}
static void launch_query_scan(hipStream_t st, const ModelView& mv, uint32_t* cnt, uint32_t* bc, uint32_t* rec) {
    ScopedKernel sk("query_scan", st);
    hipLaunchKernelGGL(k_query_scan, dim3(1), dim3(1024), 0, st, cnt, mv.nbv + mv.nbo, mv.nbv, bc, rec);
}
static void launch_query_gather(hipStream_t st, const ModelView& mv, const unsigned long long* mask, const uint32_t* cnt,
                                const uint32_t* bc, const QueryOut& o) {
    ScopedKernel sk("query_gather", st);
    hipLaunchKernelGGL(k_query_gather, dim3(mv.nbv + mv.nbo), dim3(256), 0, st, mv, mask, cnt, bc, o);
}

}  // namespace ssf

// ---- host: the entry points of include/ssf_query.h -------------------------------------------------------------------------
static bool query_extent_ok(float v) { return std::isfinite(v) && v >= 0.0f; }

// the checks of include/ssf_query.h (every parameter, whatever the region) and the kernels' argument
static int query_args(ssf_handle* h, const ssf_query_params* p, const char* who, QueryArgs& q) {
    auto refuse = [&](const char* what) { h->err = std::string(who) + ": " + what; return SSF_ERR_INVALID_ARG; };
    if (p->region != SSF_REGION_ALL && p->region != SSF_REGION_SPHERE && p->region != SSF_REGION_BOX && p->region != SSF_REGION_FRUSTUM)
        return refuse("unknown region");
    if (!query_extent_ok(p->radius)) return refuse("the radius must be finite and >= 0");
    if (!query_extent_ok(p->half[0]) || !query_extent_ok(p->half[1]) || !query_extent_ok(p->half[2])) return refuse("the half extents must be finite and >= 0");
    if (p->t_init_min > p->t_init_max || p->t_last_min > p->t_last_max) return refuse("a stamp range has min > max");
    int W = p->width, H = p->height;
    q.fx = p->fx; q.fy = p->fy; q.cx = p->cx; q.cy = p->cy;
    if (p->width == 0) { W = h->cam.W; H = h->cam.H; q.fx = h->cam.fx; q.fy = h->cam.fy; q.cx = h->cam.cx; q.cy = h->cam.cy; }
    if (W < 1 || W > 4096 || H < 1 || H > 4096) return refuse("the frustum's size must be 1..4096 x 1..4096");
    if (!std::isfinite(q.fx) || !std::isfinite(q.fy) || q.fx == 0.0f || q.fy == 0.0f) return refuse("fx and fy must be finite and non-zero");
    q.zmin = p->z_min; q.zmax = p->z_max;
    if (q.zmin == 0.0f && q.zmax == 0.0f) { q.zmin = h->cfg.range_min; q.zmax = h->cfg.range_max; }
    if (!(q.zmin > 0.0f) || !(q.zmax > q.zmin)) return refuse("the depth range needs 0 < z_min < z_max");
    q.ulim = (float)W - 0.5f; q.vlim = (float)H - 0.5f;
    const Rt T = p->pose ? pose_from12(p->pose) : h->pose;
    const float R9[9] = {T.R.r0.x, T.R.r0.y, T.R.r0.z, T.R.r1.x, T.R.r1.y, T.R.r1.z, T.R.r2.x, T.R.r2.y, T.R.r2.z};
    std::memcpy(q.R, R9, sizeof(R9)); q.t[0] = T.t.x; q.t[1] = T.t.y; q.t[2] = T.t.z;
    q.region = p->region; q.r2max = p->radius * p->radius;
    q.half[0] = p->half[0]; q.half[1] = p->half[1]; q.half[2] = p->half[2];
    q.min_conf = p->min_conf; q.ti0 = p->t_init_min; q.ti1 = p->t_init_max; q.tl0 = p->t_last_min; q.tl1 = p->t_last_max;
    return SSF_OK;
}

// select + scan, the record read back into *stats; the mask and offsets stay in h->query for the gather
static int query_select(ssf_handle* h, const QueryView& qv, ssf_query_stats* stats) {
    QueryWs& w = h->query;
    const ModelView& mv = qv.model;
    const size_t slots = std::max<size_t>(mv.nslots, 256);
    bool ok = true;
    if (slots > w.slots) {
        ok = w.bufs.grow({{(void**)&w.mask, 8 * (slots / 64)}, {(void**)&w.cnt, 8 * (slots / 256 + 1)}, {(void**)&w.bc, 4 * (slots / 256 + 1)}});
        if (ok) w.slots = slots;
    }
    if (ok && !w.rec) ok = w.bufs.grow({{(void**)&w.rec, QREC_WORDS * sizeof(uint32_t)}});
    if (!ok) { h->err = "ssf_query: allocation of the working buffers failed"; return SSF_ERR_DEVICE; }
    hipStream_t st = h->stream;
    HCK(launch_query_select(st, qv, w.mask, w.cnt, w.rec));
    launch_query_scan(st, mv, w.cnt, w.bc, w.rec);
    HCK(hipGetLastError());
    uint32_t rec[QREC_WORDS];
    HCK(hipMemcpyAsync(rec, w.rec, sizeof(rec), hipMemcpyDeviceToHost, st));
    HCK(hipStreamSynchronize(st));
    std::memset(stats, 0, sizeof(*stats));
    stats->n_scanned = (int64_t)mv.n_visible + (int64_t)rec[1];      // (rec[1]: the live rows of the out-of-view blocks looked at)
    stats->n_selected = rec[0]; stats->n_selected_visible = rec[2];
    if (rec[0] > 0)
        for (int a = 0; a < 3; a++) {
            const uint32_t lo = float_order_bits_inv(rec[QREC_LO + a]), hi = float_order_bits_inv(rec[QREC_HI + a]);
            std::memcpy(&stats->lo[a], &lo, 4); std::memcpy(&stats->hi[a], &hi, 4);
        }
    return SSF_OK;
}

extern "C" {
int ssf_query_default_params(const ssf_handle* h, ssf_query_params* p) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    std::memset(p, 0, sizeof(*p));
    p->t_init_min = INT32_MIN; p->t_init_max = INT32_MAX; p->t_last_min = INT32_MIN; p->t_last_max = INT32_MAX;
    p->region = SSF_REGION_ALL;
    return SSF_OK;
}

int ssf_query_count(ssf_handle* h, const ssf_query_params* p, ssf_query_stats* stats) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    if (!stats) { h->err = "ssf_query_count: stats is NULL"; return SSF_ERR_INVALID_ARG; }
    QueryView qv;
    { int rc = query_args(h, p, "ssf_query_count", qv.q); if (rc) return rc; }
    { int rc = model_at_rest(h, "ssf_query_count", "is not queried"); if (rc) return rc; }
    qv.model = model_view(h, p->visible_only != 0);
    TimerScope ts(h);
    { int rc = query_select(h, qv, stats); if (rc) return rc; }
    return sync_collect(h);
}

int ssf_query_rows(ssf_handle* h, const ssf_query_params* p, ssf_surfels* out, int32_t* out_index, int capacity, ssf_query_stats* stats) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    const ssf_surfels none = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const ssf_surfels u = out ? *out : none;                          // the caller's arrays
    if (!u.positions && !u.colors && !u.stamps && !u.orientations && !u.shapes && !u.dims && !u.confidences && !out_index) {
        h->err = "ssf_query_rows: every output is NULL"; return SSF_ERR_INVALID_ARG;
    }
    if (capacity < 0) { h->err = "ssf_query_rows: the capacity is negative"; return SSF_ERR_INVALID_ARG; }
    QueryView qv;
    { int rc = query_args(h, p, "ssf_query_rows", qv.q); if (rc) return rc; }
    { int rc = model_at_rest(h, "ssf_query_rows", "is not queried"); if (rc) return rc; }
    qv.model = model_view(h, p->visible_only != 0);
    QueryWs& w = h->query;
    TimerScope ts(h);
    ssf_query_stats s;
    { int rc = query_select(h, qv, &s); if (rc) return rc; }
    if (stats) *stats = s;
    if (s.n_selected > (int64_t)capacity) {
        { int rc = sync_collect(h); if (rc) return rc; }
        h->err = "ssf_query_rows: " + std::to_string((long long)s.n_selected) + " rows are selected, the capacity is " + std::to_string(capacity);
        return SSF_ERR_CAPACITY;
    }
    if (s.n_selected == 0) return sync_collect(h);
    const size_t n = (size_t)s.n_selected;
    hipStream_t st = h->stream;
    QueryOut o{u.positions, u.colors, u.stamps, u.orientations, u.shapes, u.dims, u.confidences, out_index};
    StagedIo io;
    if (!p->on_device) {
        // host outputs: gathered into the staging buffer, then the n selected rows are copied out
        io.out(u.positions, 12 * n, &o.pos); io.out(u.colors, 12 * n, &o.col); io.out(u.stamps, 8 * n, &o.stamps);
        io.out(u.orientations, 36 * n, &o.ori); io.out(u.shapes, 24 * n, &o.shape); io.out(u.dims, 8 * n, &o.dims);
        io.out(u.confidences, 4 * n, &o.conf); io.out(out_index, 4 * n, &o.index);
        const size_t cap = io.need() + io.need() / 4;
        if (!io.reserve(w.bufs, &w.rows, &w.rows_bytes, cap)) {
            h->err = "ssf_query_rows: allocation of " + std::to_string(cap) + " bytes for the selected rows failed";
            return SSF_ERR_DEVICE;
        }
    }
    launch_query_gather(st, qv.model, w.mask, w.cnt, w.bc, o);
    HCK(hipGetLastError());
    HCK(io.copy_out(st));
    return sync_collect(h);
}
}  // extern "C"
