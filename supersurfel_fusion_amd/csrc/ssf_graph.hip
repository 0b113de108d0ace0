// ssf_graph.hip -- the deformation graph's nodes and the per-row binding (include/ssf_graph.h) on gfx950.
//
// What is computed is pinned, operation by operation, in include/ssf_graph.h (the numpy restatement: tests/graph_ref.py).  How:
//   * rows   both model stores are read in place (never materialised), one thread per SLOT of [visible rows | out-of-view
//            span], as the render kernels do.  Slot order = logical order, so a sort that is stable over slots is stable over
//            logical indices; an out-of-view slot's logical index = n_visible + (live rows before it): a per-256-block count
//            (k_graph_keys), an exclusive scan (launch_slots_scan32 into own scratch: the handle's Counters and d_bc_oov are not
//            touched) and a rank inside the block -- the view and these helpers are ssf_slots.hpp's, shared with the render.
//   * rank   k_graph_keys: per slot the birth stamp and an eligibility byte, the out-of-view live counts, and min / max /
//            count of the eligible stamps with exact integer atomics (the result does not depend on their order).  Then a
//            stable least-significant-digit counting sort of (stamp - min) over 8-bit digits, 1..3 passes for a span of up to
//            2^24 (the header admits 2^20): per pass a per-workgroup digit histogram (k_graph_hist), one launch_slots_scan32 over
//            (digit, workgroup) and a scatter (k_graph_scatter) whose position inside a workgroup comes from wave ballots,
//            never from the arrival order of an atomic.  Pass 0 drops the ineligible slots, so the sorted list is dense:
//            rank -> slot.
//   * sample k_graph_sample: node k = the slot of rank k * stride: its position bits, stamp and logical index, as one 16-byte
//            record (x, y, z, bits(t_init)) per node in time order plus a packed position (what k_pack_nodes reads) and the row.
//   * bind   k_graph_bind / k_graph_bind_points: one thread per slot (or per caller point): lower bound over the records'
//            stamps (from L2: 16 steps at 64 k nodes), then the window's records, the five smallest (bits(d2) << 32 | k) kept sorted in ten registers by a min / max
//            chain, the weights, one 16-byte store each for weights4 and idx4 at the logical index.
//   * edges  k_graph_edges: the same five nearest for every node itself, for the solve (ssf_graph_solve.hip).
// No float atomics anywhere; every count is an integer.
#include <climits>
#include "ssf_slots.hpp"
#include "ssf_handle.hpp"

namespace ssf {

#define GRAPH_SORT_ITEMS 2048                     // items of one workgroup of the counting sort

// ---- keys: stamp + eligibility per slot, live counts of the out-of-view blocks, min / max / count of the eligible stamps ----
// mm[0] = min (starts INT_MAX), mm[1] = max (starts INT_MIN), mm[2] = eligible rows, mm[3] = live rows
__global__ __launch_bounds__(256) void k_graph_keys(ModelView mv, float min_conf, int32_t* __restrict__ stamp, uint8_t* __restrict__ elig,
                                                    uint32_t* __restrict__ bc, int* __restrict__ mm) {
    __shared__ int mmw[4][2], ce[4], cl[4];
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    SurfelSoA src; size_t row;
    const bool lv = slot_row(mv, s, src, row);
    int t = 0; bool el = false;
    if (lv) {
        t = src.stamps[2 * row];
        el = src.conf[row] > min_conf && finite3(src.pos[3 * row], src.pos[3 * row + 1], src.pos[3 * row + 2]);
    }
    stamp[s] = t; elig[s] = el ? 1 : 0;
    int lo = el ? t : INT_MAX, hi = el ? t : INT_MIN;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o, 64)); hi = max(hi, __shfl_xor(hi, o, 64)); }
    if (lane() == 0) { mmw[threadIdx.x >> 6][0] = lo; mmw[threadIdx.x >> 6][1] = hi; }
    const int e = block_count256(el, ce), l = block_count256(lv, cl);      // (their barrier also publishes mmw)
    if (threadIdx.x == 0) {
        if ((int)blockIdx.x >= mv.nbv) bc[blockIdx.x - mv.nbv] = (uint32_t)l;
        if (e > 0) {
            atomicMin(&mm[0], min(min(mmw[0][0], mmw[1][0]), min(mmw[2][0], mmw[3][0])));
            atomicMax(&mm[1], max(max(mmw[0][1], mmw[1][1]), max(mmw[2][1], mmw[3][1])));
            atomicAdd(&mm[2], e);
        }
        if (l > 0) atomicAdd(&mm[3], l);
    }
}

// ---- one pass of the stable counting sort: GRAPH_SORT_ITEMS items per workgroup, digit = ((key - lo) >> shift) & 255 ----------
// elig (pass 0 only): items with elig == 0 take no part; slot_in == nullptr (pass 0): the item's own index
__global__ __launch_bounds__(256) void k_graph_hist(const int32_t* __restrict__ key, const uint8_t* __restrict__ elig, int n, int lo, int shift,
                                                    uint32_t* __restrict__ cnt, int nb) {
    __shared__ uint32_t hist[256];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int base = blockIdx.x * GRAPH_SORT_ITEMS;
    for (int r = 0; r < GRAPH_SORT_ITEMS / 256; r++) {
        const int i = base + r * 256 + threadIdx.x;
        if (i < n && (!elig || elig[i])) atomicAdd(&hist[(((uint32_t)key[i] - (uint32_t)lo) >> shift) & 255u], 1u);
    }
    __syncthreads();
    cnt[(size_t)threadIdx.x * nb + blockIdx.x] = hist[threadIdx.x];
}

__global__ __launch_bounds__(256) void k_graph_scatter(const int32_t* __restrict__ key, const uint8_t* __restrict__ elig,
                                                       const uint32_t* __restrict__ slot_in, int n, int lo, int shift,
                                                       const uint32_t* __restrict__ cnt, int nb, int32_t* __restrict__ key_out,
                                                       uint32_t* __restrict__ slot_out) {
    __shared__ uint32_t run[256];
    __shared__ uint32_t wc[4][256];
    run[threadIdx.x] = cnt[(size_t)threadIdx.x * nb + blockIdx.x];
#pragma unroll
    for (int w = 0; w < 4; w++) wc[w][threadIdx.x] = 0;
    __syncthreads();
    const int base = blockIdx.x * GRAPH_SORT_ITEMS, wave = threadIdx.x >> 6;
    for (int r = 0; r < GRAPH_SORT_ITEMS / 256; r++) {
        const int i = base + r * 256 + threadIdx.x;
        const bool on = i < n && (!elig || elig[i]);
        const int32_t k = on ? key[i] : 0;
        const uint32_t d = (((uint32_t)k - (uint32_t)lo) >> shift) & 255u;
        // the lanes of this wave that hold the same digit: eight ballots; the rank inside the wave is the lanes before this one
        unsigned long long same = __ballot(on);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long v = __ballot(bit);
            same &= bit ? v : ~v;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane()) - 1ull));
        if (on && rank == 0) wc[wave][d] = (uint32_t)__popcll(same);
        __syncthreads();
        if (on) {
            uint32_t off = run[d] + rank;
            for (int w = 0; w < wave; w++) off += wc[w][d];
            key_out[off] = k;
            slot_out[off] = slot_in ? slot_in[i] : (uint32_t)i;
        }
        __syncthreads();
        run[threadIdx.x] += (wc[0][threadIdx.x] + wc[1][threadIdx.x]) + (wc[2][threadIdx.x] + wc[3][threadIdx.x]);
#pragma unroll
        for (int w = 0; w < 4; w++) wc[w][threadIdx.x] = 0;
        __syncthreads();
    }
}

// ---- sample: node k = the slot of rank k * stride ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_graph_sample(ModelView mv, const uint32_t* __restrict__ bc, const uint32_t* __restrict__ order,
                                                      int m, int stride, float4* __restrict__ nodes, float* __restrict__ npos3,
                                                      int32_t* __restrict__ nrow) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    const uint32_t s = order[(size_t)k * stride];
    SurfelSoA src; size_t row;
    (void)slot_row(mv, s, src, row);
    int logical = (int)s;
    if (s >= (uint32_t)mv.nvs) {                  // live rows of the span in front of this one: bc[its block] + a walk over the block
        const uint32_t b = (s - (uint32_t)mv.nvs) >> 8;
        int before = 0;
        for (size_t q = (size_t)mv.oov_head + ((size_t)b << 8); q < row; q++) before += mv.oov.live[q] ? 1 : 0;
        logical = mv.n_visible + (int)bc[b] + before;
    }
    const float x = src.pos[3 * row], y = src.pos[3 * row + 1], z = src.pos[3 * row + 2];
    nodes[k] = make_float4(x, y, z, __int_as_float(src.stamps[2 * row]));
    npos3[3 * k] = x; npos3[3 * k + 1] = y; npos3[3 * k + 2] = z;
    nrow[k] = logical;
}

// ---- bind: steps 1-6 of ssf_graph.h for one point ------------------------------------------------------------------------
// steps 1-4: the five smallest keys (bits(d2) << 32 | k) in ascending order, and the window's first node
__device__ __forceinline__ void graph_nearest5(const float4* __restrict__ nodes, int m, int L, float px, float py, float pz, int t,
                                               unsigned long long& k0, unsigned long long& k1, unsigned long long& k2,
                                               unsigned long long& k3, unsigned long long& k4, int& lo) {
    int a = 0, b = m;                             // the first node whose stamp >= t
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (__float_as_int(nodes[mid].w) < t) a = mid + 1; else b = mid;
    }
    const int W = min(m, 2 * L);
    lo = max(0, min(a - L, max(0, m - 2 * L)));
    k0 = k1 = k2 = k3 = k4 = ~0ull;
    for (int j = 0; j < W; j++) {
        const float4 g = nodes[lo + j];
        const float dx = px - g.x, dy = py - g.y, dz = pz - g.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        unsigned long long x = ((unsigned long long)__float_as_uint(d2) << 32) | (uint32_t)(lo + j), lo_k;
        lo_k = min(k0, x); x = max(k0, x); k0 = lo_k;
        lo_k = min(k1, x); x = max(k1, x); k1 = lo_k;
        lo_k = min(k2, x); x = max(k2, x); k2 = lo_k;
        lo_k = min(k3, x); x = max(k3, x); k3 = lo_k;
        k4 = min(k4, x);
    }
}
__device__ __forceinline__ void graph_bind_one(const float4* __restrict__ nodes, int m, int L, float px, float py, float pz, int t,
                                               float4& w4, int4& i4) {
    unsigned long long k0, k1, k2, k3, k4; int lo;
    graph_nearest5(nodes, m, L, px, py, pz, t, k0, k1, k2, k3, k4, lo);
    i4 = make_int4((int)(uint32_t)k0, (int)(uint32_t)k1, (int)(uint32_t)k2, (int)(uint32_t)k3);
    const float e0 = sqrtf(__uint_as_float((uint32_t)(k0 >> 32))), e1 = sqrtf(__uint_as_float((uint32_t)(k1 >> 32)));
    const float e2 = sqrtf(__uint_as_float((uint32_t)(k2 >> 32))), e3 = sqrtf(__uint_as_float((uint32_t)(k3 >> 32)));
    const float dmax = sqrtf(__uint_as_float((uint32_t)(k4 >> 32)));
    const float r0 = 1.0f - e0 / dmax, r1 = 1.0f - e1 / dmax, r2 = 1.0f - e2 / dmax, r3 = 1.0f - e3 / dmax;
    const float w0 = r0 * r0, w1 = r1 * r1, w2 = r2 * r2, w3 = r3 * r3;
    const float s = ((w0 + w1) + w2) + w3;
    const bool fin = finite3(px, py, pz);
    if (dmax == 0.0f || !(s > 0.0f) || !fin) {
        w4 = make_float4(0.25f, 0.25f, 0.25f, 0.25f);
        if (!fin) i4 = make_int4(lo, lo + 1, lo + 2, lo + 3);
    } else {
        w4 = make_float4(w0 / s, w1 / s, w2 / s, w3 / s);
    }
}

// every logical row of the model: one thread per slot; bc = the exclusive scan of the out-of-view blocks' live counts
__global__ __launch_bounds__(256) void k_graph_bind(ModelView mv, const uint32_t* __restrict__ bc, const float4* __restrict__ nodes, int m,
                                                    int L, float4* __restrict__ w4, int4* __restrict__ i4) {
    __shared__ int part[4];
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    SurfelSoA src; size_t row;
    const bool lv = slot_row(mv, s, src, row);
    const int logical = slot_logical256(mv, lv, bc, part);
    if (!lv) return;
    float4 w; int4 i;
    graph_bind_one(nodes, m, L, src.pos[3 * row], src.pos[3 * row + 1], src.pos[3 * row + 2], src.stamps[2 * row], w, i);
    w4[logical] = w; i4[logical] = i;
}

// n caller points against the same nodes
__global__ __launch_bounds__(256) void k_graph_bind_points(const float* __restrict__ pts, const int32_t* __restrict__ t0, int n,
                                                           const float4* __restrict__ nodes, int m, int L, float4* __restrict__ w4,
                                                           int4* __restrict__ i4) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    float4 w; int4 i;
    graph_bind_one(nodes, m, L, pts[3 * (size_t)p], pts[3 * (size_t)p + 1], pts[3 * (size_t)p + 2], t0[p], w, i);
    w4[p] = w; i4[p] = i;
}

// the solve's edges (ssf_graph_solve.h): node j's own steps 1-4, then the first four of k_0 ... k_4 that are not j
__global__ __launch_bounds__(256) void k_graph_edges(const float4* __restrict__ nodes, int m, int L, int4* __restrict__ edges) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const float4 g = nodes[j];
    unsigned long long k0, k1, k2, k3, k4; int lo;
    graph_nearest5(nodes, m, L, g.x, g.y, g.z, __float_as_int(g.w), k0, k1, k2, k3, k4, lo);
    const int a = (int)(uint32_t)k0, b = (int)(uint32_t)k1, c = (int)(uint32_t)k2, d = (int)(uint32_t)k3, e = (int)(uint32_t)k4;
    // (the five are distinct: at most one is j, and everything after it moves up by one)
    edges[j] = make_int4(a == j ? b : a, (a == j || b == j) ? c : b, (a == j || b == j || c == j) ? d : c,
                         (a == j || b == j || c == j || d == j) ? e : d);
}

// ---- launches ----------------------------------------------------------------------------------------------------------
// stamp[nslots], elig[nslots]; bc[nbo + 1] = exclusive scan of the out-of-view blocks' live counts; mm[4] (preset INT_MAX, INT_MIN,
// 0, 0) = min / max stamp of the eligible rows, their number, the live rows
static void launch_graph_keys(hipStream_t st, const ModelView& mv, float min_conf, int32_t* stamp, uint8_t* elig, uint32_t* bc, int* mm) {
    ScopedKernel sk("graph_rank", st);
    hipLaunchKernelGGL(k_graph_keys, dim3(mv.nbv + mv.nbo), dim3(256), 0, st, mv, min_conf, stamp, elig, bc, mm);
    if (mv.nbo > 0) launch_slots_scan32(st, bc, mv.nbo);
}
// stable sort of the eligible slots by (stamp - lo), `passes` 8-bit digits; cnt[256 ceil(nslots / GRAPH_SORT_ITEMS) + 1]; returns
// which of the pairs (key_a, slot_a) = 0 / (key_b, slot_b) = 1 holds the n_elig sorted (stamp, slot) entries
// (any int32 key with key - lo below 2^(8 passes); elig == nullptr: every item takes part and n_elig == nslots.  The solve's two
// transposed lists use it with lo = 0 and keys below 2^20, booked under their own name)
int launch_graph_sort(hipStream_t st, int nslots, int n_elig, int lo, int passes, const int32_t* stamp, const uint8_t* elig,
                      uint32_t* cnt, int32_t* key_a, uint32_t* slot_a, int32_t* key_b, uint32_t* slot_b, const char* name) {
    ScopedKernel sk(name, st);
    const int32_t* kin = stamp; const uint32_t* sin = nullptr; const uint8_t* el = elig;
    int n = nslots, out = 0;
    for (int p = 0; p < passes; p++) {
        const int nb = (n + GRAPH_SORT_ITEMS - 1) / GRAPH_SORT_ITEMS;
        int32_t* kout = out == 0 ? key_a : key_b; uint32_t* sout = out == 0 ? slot_a : slot_b;
        hipLaunchKernelGGL(k_graph_hist, dim3(nb), dim3(256), 0, st, kin, el, n, lo, 8 * p, cnt, nb);
        launch_slots_scan32(st, cnt, 256 * nb);
        hipLaunchKernelGGL(k_graph_scatter, dim3(nb), dim3(256), 0, st, kin, el, sin, n, lo, 8 * p, cnt, nb, kout, sout);
        kin = kout; sin = sout; el = nullptr; n = n_elig; out ^= 1;
    }
    return out ^ 1;                               // which pair holds the sorted list: 0 = a, 1 = b
}
// node k = the slot order[k stride]: nodes[k] = (x, y, z, bits(t_init)), npos3 = the packed positions, nrow = the logical row
static void launch_graph_sample(hipStream_t st, const ModelView& mv, const uint32_t* bc, const uint32_t* order, int m, int stride,
                                float4* nodes, float* npos3, int32_t* nrow) {
    ScopedKernel sk("graph_sample", st);
    hipLaunchKernelGGL(k_graph_sample, dim3((m + 255) / 256), dim3(256), 0, st, mv, bc, order, m, stride, nodes, npos3, nrow);
}
static void launch_graph_bind(hipStream_t st, const ModelView& mv, const uint32_t* bc, const float4* nodes, int m, int look, float* w4, int32_t* i4) {
    ScopedKernel sk("graph_bind", st);
    hipLaunchKernelGGL(k_graph_bind, dim3(mv.nbv + mv.nbo), dim3(256), 0, st, mv, bc, nodes, m, look, reinterpret_cast<float4*>(w4),
                       reinterpret_cast<int4*>(i4));
}
void launch_graph_edges(hipStream_t st, const float4* nodes, int m, int look, int32_t* edges, const char* name) {
    ScopedKernel sk(name, st);
    hipLaunchKernelGGL(k_graph_edges, dim3((m + 255) / 256), dim3(256), 0, st, nodes, m, look, reinterpret_cast<int4*>(edges));
}
void launch_graph_bind_points(hipStream_t st, const float* pts, const int32_t* t0, int n, const float4* nodes, int m, int look,
                              float* w4, int32_t* i4, const char* name) {
    ScopedKernel sk(name, st);
    hipLaunchKernelGGL(k_graph_bind_points, dim3((n + 255) / 256), dim3(256), 0, st, pts, t0, n, nodes, m, look,
                       reinterpret_cast<float4*>(w4), reinterpret_cast<int4*>(i4));
}

}  // namespace ssf

// ---- host: the entry points of include/ssf_graph.h -------------------------------------------------------------------------
extern "C" {
int ssf_graph_default_params(ssf_graph_params* p) {
    if (!p) return SSF_ERR_INVALID_ARG;
    p->stride = 50; p->look = 20; p->min_conf = 0.0f;
    return SSF_OK;
}
static bool graph_valid(const ssf_handle* h) { return h->graph.built && h->graph.gen == h->model_gen; }
}  // extern "C"
// the refusals every call that uses the resident graph shares (ssf_graph_solve.hip's too)
int ssf::graph_usable(ssf_handle* h, const char* who) {
    { int rc = model_at_rest(h, who, "has no deformation graph"); if (rc) return rc; }
    if (!h->graph.built) { h->err = std::string(who) + ": no graph has been built (ssf_graph_build)"; return SSF_ERR_STATE; }
    if (!graph_valid(h)) { h->err = std::string(who) + ": graph is stale: build it again"; return SSF_ERR_STATE; }
    return SSF_OK;
}
extern "C" {
int ssf_graph_build(ssf_handle* h, const ssf_graph_params* p, int* n_nodes) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    if (p->stride < 1 || p->look < 3 || !std::isfinite(p->min_conf)) {
        h->err = "ssf_graph_build: needs stride >= 1, look >= 3 and a finite min_conf"; return SSF_ERR_INVALID_ARG;
    }
    { int rc = model_at_rest(h, "ssf_graph_build", "has no deformation graph"); if (rc) return rc; }
    GraphWs& g = h->graph;
    g.built = false;                              // whatever happens below, no half-built graph is kept
    h->solve.solved = false;                      // (solved transforms die with the graph they belong to)
    if (h->n_model <= 0) { h->err = "ssf_graph_build: the model is empty"; return SSF_ERR_STATE; }

    const ModelView mv = model_view(h, false);
    const size_t slots = (size_t)mv.nslots;       // (>= n_model > 0: every row has a slot)
    if (slots > g.slots) {
        const size_t nb = (slots + GRAPH_SORT_ITEMS - 1) / GRAPH_SORT_ITEMS;
        if (!g.bufs.grow({{(void**)&g.stamp, 4 * slots}, {(void**)&g.elig, slots}, {(void**)&g.key_a, 4 * slots}, {(void**)&g.key_b, 4 * slots},
                          {(void**)&g.slot_a, 4 * slots}, {(void**)&g.slot_b, 4 * slots}, {(void**)&g.cnt, 4 * (256 * nb + 1)},
                          {(void**)&g.bc, 4 * (slots / 256 + 1)}, {(void**)&g.w4, 16 * slots}, {(void**)&g.idx4, 16 * slots},
                          {(void**)&g.mm, 4 * sizeof(int)}})) {
            h->err = "ssf_graph_build: allocation of the working buffers failed"; return SSF_ERR_DEVICE;
        }
        g.slots = slots;
    }
    TimerScope ts(h);
    hipStream_t st = h->stream;
    const int mm0[4] = {INT_MAX, INT_MIN, 0, 0};
    int mm[4] = {0, 0, 0, 0};
    HCK(hipMemcpyAsync(g.mm, mm0, sizeof(mm0), hipMemcpyHostToDevice, st));
    launch_graph_keys(st, mv, p->min_conf, g.stamp, g.elig, g.bc, g.mm);
    HCK(hipGetLastError());
    HCK(hipMemcpyAsync(mm, g.mm, sizeof(mm), hipMemcpyDeviceToHost, st));
    { int rc = sync_collect(h); if (rc) return rc; }          // (here, so that the refusals below have nothing left to book)
    if (mm[3] != h->n_model) { h->err = "ssf_graph_build: the stores hold " + std::to_string(mm[3]) + " rows, the handle counts " + std::to_string(h->n_model); return SSF_ERR_DEVICE; }
    const int n_elig = mm[2];
    const long long m64 = ((long long)n_elig + p->stride - 1) / p->stride;
    if (m64 < 5) {
        h->err = "ssf_graph_build: " + std::to_string(m64) + " nodes (" + std::to_string(n_elig) + " eligible rows, stride " +
                 std::to_string(p->stride) + "); a graph needs at least 5";
        return SSF_ERR_STATE;
    }
    const long long span = (long long)mm[1] - (long long)mm[0];
    if (span >= SSF_GRAPH_MAX_STAMP_SPAN) {
        h->err = "ssf_graph_build: the eligible rows' birth stamps span " + std::to_string(span) + " frames; at most " +
                 std::to_string(SSF_GRAPH_MAX_STAMP_SPAN - 1) + " are sorted";
        return SSF_ERR_STATE;
    }
    const int m = (int)m64;
    if ((size_t)m > g.node_cap) {
        const size_t cap = (size_t)m + (size_t)m / 4;
        if (!g.bufs.grow({{(void**)&g.nodes, 16 * cap}, {(void**)&g.npos3, 12 * cap}, {(void**)&g.nrow, 4 * cap}})) {
            h->err = "ssf_graph_build: allocation of the node table failed"; return SSF_ERR_DEVICE;
        }
        g.node_cap = cap;
    }
    const int passes = span < 256 ? 1 : span < 65536 ? 2 : 3;
    const int which = launch_graph_sort(st, mv.nslots, n_elig, mm[0], passes, g.stamp, g.elig, g.cnt, g.key_a, g.slot_a, g.key_b, g.slot_b, "graph_rank");
    HCK(hipGetLastError());
    launch_graph_sample(st, mv, g.bc, which == 0 ? g.slot_a : g.slot_b, m, p->stride, g.nodes, g.npos3, g.nrow);
    HCK(hipGetLastError());
    launch_graph_bind(st, mv, g.bc, g.nodes, m, p->look, g.w4, g.idx4);
    HCK(hipGetLastError());
    { int rc = sync_collect(h); if (rc) return rc; }
    g.m = m; g.rows = h->n_model; g.look = p->look; g.gen = h->model_gen; g.built = true;
    if (n_nodes) *n_nodes = m;
    return SSF_OK;
}
int ssf_graph_info(ssf_handle* h, int* n_nodes, int* n_rows, int* valid) {
    if (!h) return SSF_ERR_INVALID_ARG;
    if (n_nodes) *n_nodes = h->graph.built ? h->graph.m : 0;
    if (n_rows) *n_rows = h->graph.built ? h->graph.rows : 0;
    if (valid) *valid = graph_valid(h) ? 1 : 0;
    return SSF_OK;
}
int ssf_graph_get_nodes(ssf_handle* h, float* positions, int32_t* t_init, int32_t* rows, int capacity) {
    if (!h || (!positions && !t_init && !rows)) return SSF_ERR_INVALID_ARG;
    const GraphWs& g = h->graph;
    if (!g.built) { h->err = "ssf_graph_get_nodes: no graph has been built (ssf_graph_build)"; return SSF_ERR_STATE; }
    if (capacity < g.m) { h->err = "ssf_graph_get_nodes: " + std::to_string(g.m) + " nodes, room for " + std::to_string(capacity); return SSF_ERR_CAPACITY; }
    hipStream_t st = h->stream;
    const size_t m = g.m;
    std::vector<float> rec;
    if (positions) HCK(hipMemcpyAsync(positions, g.npos3, 12 * m, hipMemcpyDeviceToHost, st));
    if (rows) HCK(hipMemcpyAsync(rows, g.nrow, 4 * m, hipMemcpyDeviceToHost, st));
    if (t_init) { rec.resize(4 * m); HCK(hipMemcpyAsync(rec.data(), g.nodes, 16 * m, hipMemcpyDeviceToHost, st)); }
    HCK(hipStreamSynchronize(st));
    if (t_init) for (size_t k = 0; k < m; k++) std::memcpy(&t_init[k], &rec[4 * k + 3], 4);
    return SSF_OK;
}
int ssf_graph_get_binding(ssf_handle* h, float* weights4, int32_t* idx4, int on_device) {
    if (!h || (!weights4 && !idx4)) return SSF_ERR_INVALID_ARG;
    { int rc = graph_usable(h, "ssf_graph_get_binding"); if (rc) return rc; }
    const GraphWs& g = h->graph;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (weights4) HCK(hipMemcpyAsync(weights4, g.w4, 16 * (size_t)g.rows, kind, h->stream));
    if (idx4) HCK(hipMemcpyAsync(idx4, g.idx4, 16 * (size_t)g.rows, kind, h->stream));
    HCK(hipStreamSynchronize(h->stream));
    return SSF_OK;
}
int ssf_graph_bind_points(ssf_handle* h, const float* points, const int32_t* t_init, int n, float* weights4, int32_t* idx4) {
    if (!h || !points || !t_init || !weights4 || !idx4 || n < 0) return SSF_ERR_INVALID_ARG;
    { int rc = graph_usable(h, "ssf_graph_bind_points"); if (rc) return rc; }
    if (n == 0) return SSF_OK;
    const GraphWs& g = h->graph;
    float *d_p, *d_w; int32_t *d_t, *d_i;
    DevTemps tmp;
    HCK(tmp.take(&d_p, 12 * (size_t)n)); HCK(tmp.take(&d_t, 4 * (size_t)n)); HCK(tmp.take(&d_w, 16 * (size_t)n)); HCK(tmp.take(&d_i, 16 * (size_t)n));
    hipStream_t st = h->stream;
    HCK(hipMemcpyAsync(d_p, points, 12 * (size_t)n, hipMemcpyHostToDevice, st));
    HCK(hipMemcpyAsync(d_t, t_init, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    { TimerScope ts(h); launch_graph_bind_points(st, d_p, d_t, n, g.nodes, g.m, g.look, d_w, d_i, "graph_bind"); }
    HCK(hipGetLastError());
    HCK(hipMemcpyAsync(weights4, d_w, 16 * (size_t)n, hipMemcpyDeviceToHost, st));
    HCK(hipMemcpyAsync(idx4, d_i, 16 * (size_t)n, hipMemcpyDeviceToHost, st));
    { int rc = sync_collect(h); if (rc) return rc; }
    return SSF_OK;
}
int ssf_graph_apply(ssf_handle* h, const float* nr, const float* nt) {
    if (!h || !nr || !nt) return SSF_ERR_INVALID_ARG;
    { int rc = graph_usable(h, "ssf_graph_apply"); if (rc) return rc; }
    drop_shard_sizes(h);
    h->ahead.valid = false;
    const GraphWs& g = h->graph;
    const size_t m = g.m;
    float *d_nr, *d_nt, *d_nodes;
    DevTemps tmp;
    HCK(tmp.take(&d_nr, 36 * m)); HCK(tmp.take(&d_nt, 12 * m)); HCK(tmp.take(&d_nodes, 64 * m));
    HCK(hipMemcpyAsync(d_nr, nr, 36 * m, hipMemcpyHostToDevice, h->stream));
    HCK(hipMemcpyAsync(d_nt, nt, 12 * m, hipMemcpyHostToDevice, h->stream));
    return deform_dense(h, g.m, g.npos3, d_nr, d_nt, d_nodes, g.w4, g.idx4);
}
}  // extern "C"
