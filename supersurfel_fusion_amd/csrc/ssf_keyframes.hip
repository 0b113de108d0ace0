// ssf_keyframes.hip -- the fern-coded keyframe database (include/ssf_keyframes.h) on gfx950.
//
// What is computed is pinned, step by step, in include/ssf_keyframes.h (the numpy restatement: tests/keyframe_ref.py).  How:
//   * encode  k_kf_encode: only the cells the ferns name are reduced.  One wave per fern, eight ferns per workgroup = one packed
//             u32 of codes.  A lane takes the cell's pixels lane, lane + 64, ... (B = 8: one pixel each, B = 16: four, B = 4: the
//             first sixteen lanes one each), the five integer sums (r, g, b, depth in mm, counted pixels) are reduced across the
//             wave by xor shuffles -- no LDS in the sums, no atomics --, lane 0 compares against the fern's thresholds.
//   * search  k_kf_search: one wave per stored keyframe, a dword (eight codes) per lane and round: x = a ^ b, fold the four bits
//             of a nibble into its lowest, popcount, wave sum -> diff[k].
//   * select  k_kf_select: ONE workgroup.  min_diff_all and the first k candidates in (diff, id) order come out of k + 1
//             workgroup-wide MIN reductions over (diff << 32) | id (round j: the smallest key above round j - 1's), so nothing
//             depends on an arrival order.  The same workgroup then takes the "add" decision of ssf_keyframes_consider, counts
//             the frame's rows with conf > 0, and -- when the keyframe is added -- appends the packed codes and the stamp to the
//             tables and compacts the rows into the pool, stable, 1024 rows a round: a row's place = the rows of the waves in front
//             (ballot counts through LDS) + the lanes below it, as block_rank256 of ssf_slots.hpp does for 256.
//             One 152-byte record (ssf_keyframe_result + the stored rows) is all the host fetches.
//   * align   k_kf_align_prep: stored rows -> Lab and normals for k_align (positions and confidences are read in place).
// Every count is an integer; there is no atomic in this file.
#include "ssf_slots.hpp"

namespace ssf {

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- encode: grid = words of the packed code vector, 512 threads = eight waves = eight ferns ---------------------------------
// ferns[i] = (x | y << 16, r | g << 8 | b << 16, depth_mm, 0); the words past ceil(n / 8) are the zero padding
__global__ __launch_bounds__(512) void k_kf_encode(const uint32_t* __restrict__ rgba, const float* __restrict__ plane_depth, int W, int B,
                                                   float zmin, float zmax, const uint4* __restrict__ ferns, int n,
                                                   uint32_t* __restrict__ codes) {
    __shared__ uint32_t nib[8];
    const int wv = threadIdx.x >> 6, i = blockIdx.x * 8 + wv;
    uint32_t code = 0;
    if (i < n) {                                                     // (uniform per wave)
        const uint4 f = ferns[i];
        const int x0 = (int)(f.x & 0xFFFFu) * B, y0 = (int)(f.x >> 16) * B;
        int sr = 0, sg = 0, sb = 0, sd = 0, cnt = 0;
        for (int p = lane(); p < B * B; p += 64) {
            const size_t q = (size_t)(y0 + p / B) * W + (x0 + p % B);
            const uint32_t c = rgba[q];
            const float d = plane_depth[q];
            sr += (int)(c & 0xFFu); sg += (int)((c >> 8) & 0xFFu); sb += (int)((c >> 16) & 0xFFu);
            if (isfinite(d) && d >= zmin && d <= zmax) { sd += __float2int_rn(d * 1000.0f); cnt += 1; }
        }
        sr = wave_sum(sr); sg = wave_sum(sg); sb = wave_sum(sb); sd = wave_sum(sd); cnt = wave_sum(cnt);
        const uint32_t bb = (uint32_t)(B * B), h = bb / 2u;
        const uint32_t mr = ((uint32_t)sr + h) / bb, mg = ((uint32_t)sg + h) / bb, mb = ((uint32_t)sb + h) / bb;
        const uint32_t dm = cnt ? ((uint32_t)sd + (uint32_t)cnt / 2u) / (uint32_t)cnt : 0u;
        code = (mr > (f.y & 0xFFu) ? 1u : 0u) | (mg > ((f.y >> 8) & 0xFFu) ? 2u : 0u) | (mb > ((f.y >> 16) & 0xFFu) ? 4u : 0u) |
               ((cnt > 0 && dm > f.z) ? 8u : 0u);
    }
    if (lane() == 0) nib[wv] = code << (4 * wv);
    __syncthreads();
    if (threadIdx.x == 0) codes[blockIdx.x] = ((nib[0] | nib[1]) | (nib[2] | nib[3])) | ((nib[4] | nib[5]) | (nib[6] | nib[7]));
}

// packed words -> one byte per fern (ssf_keyframes_encode / _get)
__global__ __launch_bounds__(256) void k_kf_unpack(const uint32_t* __restrict__ codes, int n, uint8_t* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (uint8_t)((codes[i >> 3] >> (4 * (i & 7))) & 15u);
}

// ---- search: diff[k] of the query against keyframe k; 256 threads = four keyframes -------------------------------------------
__global__ __launch_bounds__(256) void k_kf_search(const uint32_t* __restrict__ q, const uint32_t* __restrict__ table, int words, int K,
                                                   uint32_t* __restrict__ diff) {
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;                                              // (uniform per wave; no barrier below)
    const uint32_t* __restrict__ row = table + (size_t)k * words;
    int d = 0;
    for (int w = lane(); w < words; w += 64) {
        uint32_t x = q[w] ^ row[w];
        x |= x >> 1; x |= x >> 2;
        d += __popc(x & 0x11111111u);
    }
    d = wave_sum(d);
    if (lane() == 0) diff[k] = (uint32_t)d;
}

// ---- select (+ the add): one workgroup of 1024 -----------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long workgroup_min64(unsigned long long v, unsigned long long* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    __syncthreads();                                                 // (red may still be read from the previous round)
    if (lane() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long m = red[0];
#pragma unroll
    for (int w = 1; w < 16; w++) m = red[w] < m ? red[w] : m;
    return m;
}

// mode 0: query only; 1: consider (add iff K == 0 or min_diff_all / n >= new_ratio); 2: add whatever the codes.
// rec (SSF_KF_REC_WORDS words): ssf_keyframe_result (38 words), then [38] = the rows stored.  The add appends to table / stamps at K and to the pool
// at rows_used; the host mirrors both from the record.
struct KfSelect {
    const uint32_t* q; uint32_t* table; int32_t* stamps; const uint32_t* diff;
    int words, n, K, max_keyframes, mode, kmax, stamp, min_gap;
    long long rows_used, max_rows;
    float new_ratio, loop_ratio;
    SurfelSoA frame; int S;
    KfPool pool;
    int32_t* rec;
};
__global__ __launch_bounds__(1024) void k_kf_select(KfSelect a) {
    __shared__ unsigned long long red[16];
    __shared__ int part[16];
    const unsigned long long NONE = ~0ull;
    // min over all
    unsigned long long m = NONE;
    for (int k = threadIdx.x; k < a.K; k += 1024) {
        const unsigned long long key = ((unsigned long long)a.diff[k] << 32) | (uint32_t)k;
        m = key < m ? key : m;
    }
    m = workgroup_min64(m, red);
    const int min_all = a.K > 0 ? (int)(m >> 32) : a.n + 1;
    // candidates: round j picks the smallest eligible key above round j - 1's
    const long long latest = (long long)a.stamp - (long long)a.min_gap;
    unsigned long long last = 0; bool first = true; int ncand = 0;
    for (int j = 0; j < a.kmax; j++) {
        unsigned long long c = NONE;
        for (int k = threadIdx.x; k < a.K; k += 1024) {
            if ((long long)a.stamps[k] > latest) continue;
            const unsigned long long key = ((unsigned long long)a.diff[k] << 32) | (uint32_t)k;
            if ((first || key > last) && key < c) c = key;
        }
        c = workgroup_min64(c, red);
        if (c == NONE) break;                                        // (uniform: every thread holds the same c)
        if (threadIdx.x == 0) {
            const int id = (int)(uint32_t)c, df = (int)(c >> 32);
            a.rec[6 + 4 * j] = id; a.rec[7 + 4 * j] = df; a.rec[8 + 4 * j] = a.stamps[id];
            a.rec[9 + 4 * j] = ((float)df / (float)a.n <= a.loop_ratio) ? 1 : 0;
        }
        last = c; first = false; ncand = j + 1;
    }
    if (threadIdx.x == 0) for (int j = ncand; j < SSF_KEYFRAMES_MAX_CANDIDATES; j++) { a.rec[6 + 4 * j] = -1; a.rec[7 + 4 * j] = 0; a.rec[8 + 4 * j] = 0; a.rec[9 + 4 * j] = 0; }
    // the decision
    const bool want = a.mode == 2 || (a.mode == 1 && (a.K == 0 || (float)min_all / (float)a.n >= a.new_ratio));
    int nrows = 0;
    if (want) {                                                      // (uniform) the frame's rows with conf > 0
        int c = 0;
        for (int i = threadIdx.x; i < a.S; i += 1024) c += a.frame.conf[i] > 0.0f ? 1 : 0;
        c = wave_sum(c);
        __syncthreads();
        if (lane() == 0) part[threadIdx.x >> 6] = c;
        __syncthreads();
        for (int w = 0; w < 16; w++) nrows += part[w];
    }
    const bool full = want && (a.K >= a.max_keyframes || a.rows_used + (long long)nrows > a.max_rows);
    const bool add = want && !full;
    if (threadIdx.x == 0) {
        a.rec[0] = add ? 1 : 0; a.rec[1] = add ? a.K : -1; a.rec[2] = full ? 1 : 0; a.rec[3] = min_all;
        a.rec[4] = a.K + (add ? 1 : 0); a.rec[5] = ncand; a.rec[38] = add ? nrows : 0;
    }
    if (!add) return;
    for (int w = threadIdx.x; w < a.words; w += 1024) a.table[(size_t)a.K * a.words + w] = a.q[w];
    if (threadIdx.x == 0) a.stamps[a.K] = a.stamp;
    // stable compaction, 1024 rows a round: rank inside the round = the waves in front + the lanes below
    long long base = a.rows_used;
    for (int i0 = 0; i0 < a.S; i0 += 1024) {
        const int i = i0 + threadIdx.x;
        const bool mine = i < a.S && a.frame.conf[i] > 0.0f;
        const unsigned long long bal = __ballot(mine);
        __syncthreads();
        if (lane() == 0) part[threadIdx.x >> 6] = __popcll(bal);
        __syncthreads();
        int before = __popcll(bal & ((1ull << lane()) - 1ull)), all = 0;
        for (int w = 0; w < 16; w++) { const int t = part[w]; if (w < (int)(threadIdx.x >> 6)) before += t; all += t; }
        if (mine) {
            const size_t o = (size_t)(base + before), r = (size_t)i;
            const SurfelSoA& f = a.frame;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                a.pool.pos[3 * o + c] = f.pos[3 * r + c]; a.pool.col[3 * o + c] = f.col[3 * r + c];
                a.pool.orient[9 * o + c] = f.r0[3 * r + c]; a.pool.orient[9 * o + 3 + c] = f.r1[3 * r + c];
                a.pool.orient[9 * o + 6 + c] = f.r2[3 * r + c];
            }
#pragma unroll
            for (int c = 0; c < 6; c++) a.pool.shape[6 * o + c] = f.shape[6 * r + c];
            a.pool.stamps[2 * o] = f.stamps[2 * r]; a.pool.stamps[2 * o + 1] = f.stamps[2 * r + 1];
            a.pool.dims[2 * o] = f.dims[2 * r]; a.pool.dims[2 * o + 1] = f.dims[2 * r + 1];
            a.pool.conf[o] = f.conf[r];
        }
        base += all;
    }
}

// ---- align prep: Lab of the stored colours, the stored normals ---------------------------------------------------------------
__global__ __launch_bounds__(256) void k_kf_align_prep(const float* __restrict__ col, const float* __restrict__ orient, int n,
                                                       float* __restrict__ lab, float* __restrict__ nrm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const V3 l = rgb_to_lab(v3(col[3 * (size_t)i], col[3 * (size_t)i + 1], col[3 * (size_t)i + 2]));
    lab[3 * (size_t)i] = l.x; lab[3 * (size_t)i + 1] = l.y; lab[3 * (size_t)i + 2] = l.z;
#pragma unroll
    for (int c = 0; c < 3; c++) nrm[3 * (size_t)i + c] = orient[9 * (size_t)i + 6 + c];
}

// ---- launches ----------------------------------------------------------------------------------------------------------
void launch_kf_encode(hipStream_t st, const uint32_t* rgba, const float* plane_depth, int W, int B, float zmin, float zmax,
                      const uint4* ferns, int n, int words, uint32_t* codes) {
    ScopedKernel sk("kf_encode", st);
    hipLaunchKernelGGL(k_kf_encode, dim3(words), dim3(512), 0, st, rgba, plane_depth, W, B, zmin, zmax, ferns, n, codes);
}
void launch_kf_unpack(hipStream_t st, const uint32_t* codes, int n, uint8_t* out) {
    hipLaunchKernelGGL(k_kf_unpack, dim3((n + 255) / 256), dim3(256), 0, st, codes, n, out);
}
void launch_kf_search(hipStream_t st, const uint32_t* q, const uint32_t* table, int words, int K, uint32_t* diff) {
    if (K <= 0) return;
    ScopedKernel sk("kf_search", st);
    hipLaunchKernelGGL(k_kf_search, dim3((K + 3) / 4), dim3(256), 0, st, q, table, words, K, diff);
}
void launch_kf_select(hipStream_t st, const KfQuery& qy, const uint32_t* q, uint32_t* table, int32_t* stamps, const uint32_t* diff,
                      const SurfelSoA& frame, int S, const KfPool& pool, int32_t* rec) {
    ScopedKernel sk("kf_select", st);
    KfSelect a;
    a.q = q; a.table = table; a.stamps = stamps; a.diff = diff;
    a.words = qy.words; a.n = qy.n; a.K = qy.K; a.max_keyframes = qy.max_keyframes; a.mode = qy.mode; a.kmax = qy.kmax;
    a.stamp = qy.stamp; a.min_gap = qy.min_gap; a.rows_used = qy.rows_used; a.max_rows = qy.max_rows;
    a.new_ratio = qy.new_ratio; a.loop_ratio = qy.loop_ratio; a.frame = frame; a.S = S; a.pool = pool; a.rec = rec;
    hipLaunchKernelGGL(k_kf_select, dim3(1), dim3(1024), 0, st, a);
}
void launch_kf_align_prep(hipStream_t st, const float* col, const float* orient, int n, float* lab, float* nrm) {
    if (n <= 0) return;
    ScopedKernel sk("kf_align_prep", st);
    hipLaunchKernelGGL(k_kf_align_prep, dim3((n + 255) / 256), dim3(256), 0, st, col, orient, n, lab, nrm);
}

}  // namespace ssf
