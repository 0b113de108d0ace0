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
#include "ssf_handle.hpp"

namespace ssf {

#define SSF_KF_REC_WORDS 40                       // ssf_keyframe_result (38 words), the rows stored, one spare
// one query: n ferns in `words` packed words, K stored keyframes; mode 0 query, 1 consider, 2 add (see k_kf_select)
struct KfQuery { int words, n, K, max_keyframes, mode, kmax, stamp, min_gap; long long rows_used, max_rows; float new_ratio, loop_ratio; };

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
    v = wave_min64(v);
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
    ssf_surfels pool;                             // device arrays: a keyframe's rows are consecutive, in ssf_surfels' layout
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
                a.pool.positions[3 * o + c] = f.pos[3 * r + c]; a.pool.colors[3 * o + c] = f.col[3 * r + c];
                a.pool.orientations[9 * o + c] = f.r0[3 * r + c]; a.pool.orientations[9 * o + 3 + c] = f.r1[3 * r + c];
                a.pool.orientations[9 * o + 6 + c] = f.r2[3 * r + c];
            }
#pragma unroll
            for (int c = 0; c < 6; c++) a.pool.shapes[6 * o + c] = f.shape[6 * r + c];
            a.pool.stamps[2 * o] = f.stamps[2 * r]; a.pool.stamps[2 * o + 1] = f.stamps[2 * r + 1];
            a.pool.dims[2 * o] = f.dims[2 * r]; a.pool.dims[2 * o + 1] = f.dims[2 * r + 1];
            a.pool.confidences[o] = f.conf[r];
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
// ferns[i] = (x | y << 16, r | g << 8 | b << 16, depth_mm, 0); codes: `words` packed words of the frame (rgba, plane_depth)
static void launch_kf_encode(hipStream_t st, const uint32_t* rgba, const float* plane_depth, int W, int B, float zmin, float zmax,
                             const uint4* ferns, int n, int words, uint32_t* codes) {
    ScopedKernel sk("kf_encode", st);
    hipLaunchKernelGGL(k_kf_encode, dim3(words), dim3(512), 0, st, rgba, plane_depth, W, B, zmin, zmax, ferns, n, codes);
}
static void launch_kf_unpack(hipStream_t st, const uint32_t* codes, int n, uint8_t* out) {
    hipLaunchKernelGGL(k_kf_unpack, dim3((n + 255) / 256), dim3(256), 0, st, codes, n, out);
}
static void launch_kf_search(hipStream_t st, const uint32_t* q, const uint32_t* table, int words, int K, uint32_t* diff) {
    if (K <= 0) return;
    ScopedKernel sk("kf_search", st);
    hipLaunchKernelGGL(k_kf_search, dim3((K + 3) / 4), dim3(256), 0, st, q, table, words, K, diff);
}
static void launch_kf_select(hipStream_t st, const KfQuery& qy, const uint32_t* q, uint32_t* table, int32_t* stamps, const uint32_t* diff,
                             const SurfelSoA& frame, int S, const ssf_surfels& pool, int32_t* rec) {
    ScopedKernel sk("kf_select", st);
    KfSelect a;
    a.q = q; a.table = table; a.stamps = stamps; a.diff = diff;
    a.words = qy.words; a.n = qy.n; a.K = qy.K; a.max_keyframes = qy.max_keyframes; a.mode = qy.mode; a.kmax = qy.kmax;
    a.stamp = qy.stamp; a.min_gap = qy.min_gap; a.rows_used = qy.rows_used; a.max_rows = qy.max_rows;
    a.new_ratio = qy.new_ratio; a.loop_ratio = qy.loop_ratio; a.frame = frame; a.S = S; a.pool = pool; a.rec = rec;
    hipLaunchKernelGGL(k_kf_select, dim3(1), dim3(1024), 0, st, a);
}
static void launch_kf_align_prep(hipStream_t st, const float* col, const float* orient, int n, float* lab, float* nrm) {
    if (n <= 0) return;
    ScopedKernel sk("kf_align_prep", st);
    hipLaunchKernelGGL(k_kf_align_prep, dim3((n + 255) / 256), dim3(256), 0, st, col, orient, n, lab, nrm);
}

}  // namespace ssf

// ---- host: the entry points of include/ssf_keyframes.h ---------------------------------------------------------------------
extern "C" {
int ssf_keyframes_default_params(ssf_keyframes_params* p) {
    if (!p) return SSF_ERR_INVALID_ARG;
    std::memset(p, 0, sizeof(*p));
    p->cell = 8; p->n_ferns = 500; p->seed = 1234; p->max_keyframes = 256; p->min_gap = 30; p->max_rows = 0;
    p->new_ratio = 0.3f; p->loop_ratio = 0.2f;
    return SSF_OK;
}
static uint64_t kf_splitmix64(uint64_t& s) {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the refusals the calls share: a sharded handle, no database, a model that is not at rest and (needs_frame: 1 = a current
// frame, 2 = one with a colour map) no frame to read
static int kf_usable(ssf_handle* h, const char* who, int needs_frame) {
    if (h->cfg.nranks > 1) { h->err = std::string(who) + ": a sharded handle (cfg.nranks > 1) keeps no keyframe database"; return SSF_ERR_STATE; }
    if (!h->kf.on) { h->err = std::string(who) + ": no keyframe database (ssf_keyframes_configure)"; return SSF_ERR_STATE; }
    if (!h->pending.empty() || h->fusing) { h->err = std::string(who) + ": frames are pending in the extract pipeline"; return SSF_ERR_STATE; }
    if (needs_frame && !(h->active.ctx && h->active.activated)) { h->err = std::string(who) + ": no frame has been processed yet"; return SSF_ERR_STATE; }
    if (needs_frame == 2 && !h->active.has_rgba) {
        h->err = std::string(who) + ": the current frame came in as tables (ssf_submit_frame_tables): it has no colour map"; return SSF_ERR_STATE;
    }
    return SSF_OK;
}
static void kf_pack_ferns(const std::vector<ssf_fern>& f, std::vector<uint32_t>& out) {
    out.resize(4 * f.size());
    for (size_t i = 0; i < f.size(); i++) {
        out[4 * i] = (uint32_t)f[i].x | ((uint32_t)f[i].y << 16);
        out[4 * i + 1] = (uint32_t)f[i].r | ((uint32_t)f[i].g << 8) | ((uint32_t)f[i].b << 16);
        out[4 * i + 2] = f[i].depth_mm; out[4 * i + 3] = 0;
    }
}
static int kf_upload_ferns(ssf_handle* h) {
    std::vector<uint32_t> w;
    kf_pack_ferns(h->kf.host_ferns, w);
    HCK(hipMemcpyAsync(h->kf.ferns, w.data(), 4 * w.size(), hipMemcpyHostToDevice, h->stream));
    HCK(hipStreamSynchronize(h->stream));
    return SSF_OK;
}
int ssf_keyframes_configure(ssf_handle* h, const ssf_keyframes_params* p) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    const int W = h->cfg.width, H = h->cfg.height;
    if ((p->cell != 4 && p->cell != 8 && p->cell != 16) || W < p->cell || H < p->cell || p->n_ferns < 1 || p->n_ferns > SSF_KEYFRAMES_MAX_FERNS ||
        p->max_keyframes < 1 || p->min_gap < 0 || p->max_rows < 0 || !std::isfinite(p->new_ratio) || !std::isfinite(p->loop_ratio)) {
        h->err = "ssf_keyframes_configure: needs cell 4 / 8 / 16 (<= the image), 1 .. 4096 ferns, max_keyframes >= 1, min_gap >= 0, max_rows >= 0 and finite ratios";
        return SSF_ERR_INVALID_ARG;
    }
    // the depth range in mm: the sum of a cell's 256 depths must fit 31 bits
    if (!(h->cfg.range_min >= 0.0f) || !(h->cfg.range_max <= 8000.0f) || !(lrintf(h->cfg.range_max * 1000.0f) > lrintf(h->cfg.range_min * 1000.0f))) {
        h->err = "ssf_keyframes_configure: needs 0 <= range_min < range_max <= 8000 m (whole millimetres apart)"; return SSF_ERR_INVALID_ARG;
    }
    if (h->cfg.nranks > 1) { h->err = "ssf_keyframes_configure: a sharded handle (cfg.nranks > 1) keeps no keyframe database"; return SSF_ERR_STATE; }
    KeyframeWs& k = h->kf;
    if (k.on) { h->err = "ssf_keyframes_configure: a database is live (ssf_keyframes_clear first)"; return SSF_ERR_STATE; }
    const size_t words = (((size_t)p->n_ferns + 7) / 8 + 63) / 64 * 64, K = (size_t)p->max_keyframes;
    const size_t rows = p->max_rows > 0 ? (size_t)p->max_rows : K * (size_t)h->S;
    if (!k.bufs.grow({{(void**)&k.ferns, 16 * (size_t)p->n_ferns}, {(void**)&k.q, 4 * words}, {(void**)&k.table, 4 * words * K},
                      {(void**)&k.stamps, 4 * K}, {(void**)&k.diff, 4 * K}, {(void**)&k.rec, 4 * SSF_KF_REC_WORDS},
                      {(void**)&k.bytes, (size_t)SSF_KEYFRAMES_MAX_FERNS},
                      {(void**)&k.pool.positions, 12 * rows}, {(void**)&k.pool.colors, 12 * rows}, {(void**)&k.pool.stamps, 8 * rows},
                      {(void**)&k.pool.orientations, 36 * rows}, {(void**)&k.pool.shapes, 24 * rows}, {(void**)&k.pool.dims, 8 * rows},
                      {(void**)&k.pool.confidences, 4 * rows}})) {
        k.bufs.release();
        h->err = "ssf_keyframes_configure: allocation of the database failed"; return SSF_ERR_DEVICE;
    }
    k.p = *p; k.p.max_rows = (int64_t)rows;
    k.words = (int)words; k.gw = W / p->cell; k.gh = H / p->cell;
    k.kfs.clear(); k.rows_used = 0;
    const uint32_t dlo = (uint32_t)lrintf(h->cfg.range_min * 1000.0f), dhi = (uint32_t)lrintf(h->cfg.range_max * 1000.0f);
    k.host_ferns.assign((size_t)p->n_ferns, ssf_fern());
    uint64_t s = p->seed;
    for (auto& f : k.host_ferns) {
        f.x = (uint16_t)(kf_splitmix64(s) % (uint64_t)k.gw); f.y = (uint16_t)(kf_splitmix64(s) % (uint64_t)k.gh);
        f.r = (uint8_t)(kf_splitmix64(s) % 256u); f.g = (uint8_t)(kf_splitmix64(s) % 256u); f.b = (uint8_t)(kf_splitmix64(s) % 256u);
        f.pad = 0; f.depth_mm = dlo + (uint32_t)(kf_splitmix64(s) % (uint64_t)(dhi - dlo));
    }
    { int rc = kf_upload_ferns(h); if (rc) { k.bufs.release(); return rc; } }
    k.on = true;
    return SSF_OK;
}
int ssf_keyframes_clear(ssf_handle* h) {
    if (!h) return SSF_ERR_INVALID_ARG;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    KeyframeWs& k = h->kf;
    k.bufs.release();
    k.on = false; k.kfs.clear(); k.host_ferns.clear(); k.rows_used = 0; k.words = 0;
    return SSF_OK;
}
int ssf_keyframes_info(ssf_handle* h, int* configured, int* n_keyframes, int64_t* rows_used, ssf_keyframes_params* p) {
    if (!h) return SSF_ERR_INVALID_ARG;
    const KeyframeWs& k = h->kf;
    if (configured) *configured = k.on ? 1 : 0;
    if (n_keyframes) *n_keyframes = k.on ? (int)k.kfs.size() : 0;
    if (rows_used) *rows_used = k.on ? (int64_t)k.rows_used : 0;
    if (p) { if (k.on) *p = k.p; else std::memset(p, 0, sizeof(*p)); }
    return SSF_OK;
}
int ssf_keyframes_set_ferns(ssf_handle* h, const ssf_fern* ferns, int n) {
    if (!h || !ferns) return SSF_ERR_INVALID_ARG;
    { int rc = kf_usable(h, "ssf_keyframes_set_ferns", 0); if (rc) return rc; }
    KeyframeWs& k = h->kf;
    if (n != k.p.n_ferns) { h->err = "ssf_keyframes_set_ferns: the database is configured for " + std::to_string(k.p.n_ferns) + " ferns"; return SSF_ERR_INVALID_ARG; }
    if (!k.kfs.empty()) { h->err = "ssf_keyframes_set_ferns: keyframes are stored under the present table"; return SSF_ERR_STATE; }
    for (int i = 0; i < n; i++)
        if ((int)ferns[i].x >= k.gw || (int)ferns[i].y >= k.gh) {
            h->err = "ssf_keyframes_set_ferns: fern " + std::to_string(i) + " names a cell outside the " + std::to_string(k.gw) + " x " + std::to_string(k.gh) + " grid";
            return SSF_ERR_INVALID_ARG;
        }
    k.host_ferns.assign(ferns, ferns + n);
    for (auto& f : k.host_ferns) f.pad = 0;
    return kf_upload_ferns(h);
}
int ssf_keyframes_get_ferns(ssf_handle* h, ssf_fern* ferns, int capacity) {
    if (!h || !ferns) return SSF_ERR_INVALID_ARG;
    { int rc = kf_usable(h, "ssf_keyframes_get_ferns", 0); if (rc) return rc; }
    const KeyframeWs& k = h->kf;
    if (capacity < k.p.n_ferns) { h->err = "ssf_keyframes_get_ferns: " + std::to_string(k.p.n_ferns) + " ferns, room for " + std::to_string(capacity); return SSF_ERR_CAPACITY; }
    std::memcpy(ferns, k.host_ferns.data(), sizeof(ssf_fern) * k.host_ferns.size());
    return SSF_OK;
}
// the current frame's packed codes into kf.q (enqueued only)
static void kf_encode_current(ssf_handle* h) {
    const KeyframeWs& k = h->kf;
    launch_kf_encode(h->stream, h->cc->maps.rgba, h->cc->maps.plane_depth, h->cfg.width, k.p.cell, h->cfg.range_min, h->cfg.range_max,
                     k.ferns, k.p.n_ferns, k.words, k.q);
}
// n code bytes -> the packed words; false: a code > 15
static bool kf_pack_codes(const uint8_t* codes, int n, int words, std::vector<uint32_t>& out) {
    out.assign((size_t)words, 0u);
    for (int i = 0; i < n; i++) {
        if (codes[i] > 15) return false;
        out[i >> 3] |= (uint32_t)codes[i] << (4 * (i & 7));
    }
    return true;
}
// search + select (+ the add) of kf.q; rec: SSF_KF_REC_WORDS words.  The host takes the keyframe the device added into its mirror
static int kf_run(ssf_handle* h, const char* who, int mode, int kmax, int stamp, int min_gap, bool with_frame, int32_t* rec) {
    KeyframeWs& k = h->kf;
    hipStream_t st = h->stream;
    KfQuery q;
    q.words = k.words; q.n = k.p.n_ferns; q.K = (int)k.kfs.size(); q.max_keyframes = k.p.max_keyframes; q.mode = mode; q.kmax = kmax;
    q.stamp = stamp; q.min_gap = min_gap; q.rows_used = k.rows_used; q.max_rows = (long long)k.p.max_rows;
    q.new_ratio = k.p.new_ratio; q.loop_ratio = k.p.loop_ratio;
    launch_kf_search(st, k.q, k.table, k.words, q.K, k.diff);
    HCK(hipGetLastError());
    SurfelSoA none; std::memset(&none, 0, sizeof(none));
    launch_kf_select(st, q, k.q, k.table, k.stamps, k.diff, with_frame ? h->cc->frame : none, with_frame ? h->S : 0, k.pool, k.rec);
    HCK(hipGetLastError());
    HCK(hipMemcpyAsync(rec, k.rec, 4 * SSF_KF_REC_WORDS, hipMemcpyDeviceToHost, st));
    { int rc = sync_collect(h); if (rc) return rc; }
    const bool added = rec[0] != 0;
    // the decision was taken on the device; the host checks what it can from the record
    if (rec[4] != q.K + (added ? 1 : 0) || (added && (rec[1] != q.K || mode == 0 || rec[38] < 0 || k.rows_used + rec[38] > (long long)k.p.max_rows)) ||
        rec[5] < 0 || rec[5] > kmax) {
        h->err = std::string(who) + ": the device's record contradicts the host's view of the database"; return SSF_ERR_DEVICE;
    }
    if (added) {
        KeyframeMeta m; m.first = k.rows_used; m.rows = rec[38]; m.stamp = stamp; pose_to12(h->pose, m.pose);
        k.kfs.push_back(m); k.rows_used += m.rows;
    }
    return SSF_OK;
}
int ssf_keyframes_encode(ssf_handle* h, uint8_t* codes, int capacity) {
    if (!h || !codes) return SSF_ERR_INVALID_ARG;
    { int rc = kf_usable(h, "ssf_keyframes_encode", 2); if (rc) return rc; }
    KeyframeWs& k = h->kf;
    if (capacity < k.p.n_ferns) { h->err = "ssf_keyframes_encode: " + std::to_string(k.p.n_ferns) + " codes, room for " + std::to_string(capacity); return SSF_ERR_CAPACITY; }
    { TimerScope ts(h); kf_encode_current(h); }
    HCK(hipGetLastError());
    launch_kf_unpack(h->stream, k.q, k.p.n_ferns, k.bytes);
    HCK(hipGetLastError());
    HCK(hipMemcpyAsync(codes, k.bytes, (size_t)k.p.n_ferns, hipMemcpyDeviceToHost, h->stream));
    { int rc = sync_collect(h); if (rc) return rc; }
    return SSF_OK;
}
int ssf_keyframes_query(ssf_handle* h, const uint8_t* codes, int stamp, int min_gap, int kmax, ssf_keyframe_result* out) {
    if (!h || !out || kmax < 0 || kmax > SSF_KEYFRAMES_MAX_CANDIDATES) return SSF_ERR_INVALID_ARG;
    { int rc = kf_usable(h, "ssf_keyframes_query", codes ? 0 : 2); if (rc) return rc; }
    KeyframeWs& k = h->kf;
    std::vector<uint32_t> packed;
    TimerScope ts(h);
    if (codes) {
        if (!kf_pack_codes(codes, k.p.n_ferns, k.words, packed)) { h->err = "ssf_keyframes_query: a code is a value 0 .. 15"; return SSF_ERR_INVALID_ARG; }
        HCK(hipMemcpyAsync(k.q, packed.data(), 4 * packed.size(), hipMemcpyHostToDevice, h->stream));
    } else {
        kf_encode_current(h);
        HCK(hipGetLastError());
        stamp = h->stamp;
    }
    int32_t rec[SSF_KF_REC_WORDS];
    { int rc = kf_run(h, "ssf_keyframes_query", 0, kmax, stamp, min_gap < 0 ? k.p.min_gap : min_gap, false, rec); if (rc) return rc; }
    std::memcpy(out, rec, sizeof(*out));
    return SSF_OK;
}
int ssf_keyframes_consider(ssf_handle* h, ssf_keyframe_result* out) {
    if (!h || !out) return SSF_ERR_INVALID_ARG;
    { int rc = kf_usable(h, "ssf_keyframes_consider", 2); if (rc) return rc; }
    TimerScope ts(h);
    kf_encode_current(h);
    HCK(hipGetLastError());
    int32_t rec[SSF_KF_REC_WORDS];
    { int rc = kf_run(h, "ssf_keyframes_consider", 1, SSF_KEYFRAMES_MAX_CANDIDATES, h->stamp, h->kf.p.min_gap, true, rec); if (rc) return rc; }
    std::memcpy(out, rec, sizeof(*out));
    return SSF_OK;
}
int ssf_keyframes_add(ssf_handle* h, int* id) {
    if (!h) return SSF_ERR_INVALID_ARG;
    { int rc = kf_usable(h, "ssf_keyframes_add", 2); if (rc) return rc; }
    TimerScope ts(h);
    kf_encode_current(h);
    HCK(hipGetLastError());
    int32_t rec[SSF_KF_REC_WORDS];
    { int rc = kf_run(h, "ssf_keyframes_add", 2, 0, h->stamp, h->kf.p.min_gap, true, rec); if (rc) return rc; }
    if (!rec[0]) { h->err = "ssf_keyframes_add: the store is full"; return SSF_ERR_CAPACITY; }
    if (id) *id = rec[1];
    return SSF_OK;
}
int ssf_keyframes_put(ssf_handle* h, const uint8_t* codes, const ssf_surfels* rows, int n_rows, const float* pose, int stamp, int* id) {
    if (!h || !codes || !pose || n_rows < 0 || (n_rows > 0 && (!rows || !rows->positions || !rows->colors || !rows->stamps || !rows->orientations ||
                                                              !rows->shapes || !rows->dims || !rows->confidences))) return SSF_ERR_INVALID_ARG;
    { int rc = kf_usable(h, "ssf_keyframes_put", 0); if (rc) return rc; }
    KeyframeWs& k = h->kf;
    const size_t K = k.kfs.size(), n = (size_t)n_rows, o = (size_t)k.rows_used;
    if ((int)K >= k.p.max_keyframes || k.rows_used + n_rows > (long long)k.p.max_rows) { h->err = "ssf_keyframes_put: the store is full"; return SSF_ERR_CAPACITY; }
    std::vector<uint32_t> packed;
    if (!kf_pack_codes(codes, k.p.n_ferns, k.words, packed)) { h->err = "ssf_keyframes_put: a code is a value 0 .. 15"; return SSF_ERR_INVALID_ARG; }
    hipStream_t st = h->stream;
    const int32_t stamp32 = stamp;
    HCK(hipMemcpyAsync(k.table + K * (size_t)k.words, packed.data(), 4 * packed.size(), hipMemcpyHostToDevice, st));
    HCK(hipMemcpyAsync(k.stamps + K, &stamp32, 4, hipMemcpyHostToDevice, st));
    if (n > 0) { int rc = copy_rows(h, k.pool, o, *rows, 0, n, hipMemcpyHostToDevice); if (rc) return rc; }
    HCK(hipStreamSynchronize(st));
    KeyframeMeta m; m.first = k.rows_used; m.rows = n_rows; m.stamp = stamp; std::memcpy(m.pose, pose, sizeof(m.pose));
    k.kfs.push_back(m); k.rows_used += n_rows;
    if (id) *id = (int)K;
    return SSF_OK;
}
static int kf_lookup(ssf_handle* h, const char* who, int id) {
    if (id < 0 || (size_t)id >= h->kf.kfs.size()) {
        h->err = std::string(who) + ": no keyframe " + std::to_string(id) + " (" + std::to_string(h->kf.kfs.size()) + " stored)"; return SSF_ERR_INVALID_ARG;
    }
    return SSF_OK;
}
int ssf_keyframes_get(ssf_handle* h, int id, ssf_surfels* rows, int capacity, int* n_rows, float* pose, int* stamp, uint8_t* codes) {
    if (!h) return SSF_ERR_INVALID_ARG;
    { int rc = kf_usable(h, "ssf_keyframes_get", 0); if (rc) return rc; }
    { int rc = kf_lookup(h, "ssf_keyframes_get", id); if (rc) return rc; }
    KeyframeWs& k = h->kf;
    const KeyframeMeta& m = k.kfs[(size_t)id];
    if (rows && capacity < m.rows) { h->err = "ssf_keyframes_get: " + std::to_string(m.rows) + " rows, room for " + std::to_string(capacity); return SSF_ERR_CAPACITY; }
    hipStream_t st = h->stream;
    const size_t n = (size_t)m.rows, o = (size_t)m.first;
    if (rows) { int rc = copy_rows(h, *rows, 0, k.pool, o, n, hipMemcpyDeviceToHost); if (rc) return rc; }
    if (codes) {
        launch_kf_unpack(st, k.table + (size_t)id * k.words, k.p.n_ferns, k.bytes);
        HCK(hipGetLastError());
        HCK(hipMemcpyAsync(codes, k.bytes, (size_t)k.p.n_ferns, hipMemcpyDeviceToHost, st));
    }
    HCK(hipStreamSynchronize(st));
    if (n_rows) *n_rows = m.rows;
    if (pose) std::memcpy(pose, m.pose, sizeof(m.pose));
    if (stamp) *stamp = m.stamp;
    return SSF_OK;
}
int ssf_keyframes_set_pose(ssf_handle* h, int id, const float* pose) {
    if (!h || !pose) return SSF_ERR_INVALID_ARG;
    { int rc = kf_usable(h, "ssf_keyframes_set_pose", 0); if (rc) return rc; }
    { int rc = kf_lookup(h, "ssf_keyframes_set_pose", id); if (rc) return rc; }
    std::memcpy(h->kf.kfs[(size_t)id].pose, pose, 12 * sizeof(float));
    return SSF_OK;
}
int ssf_keyframes_align(ssf_handle* h, int id, const float* init_pose, int use_conf, float* rel_pose, int* valid, int* iters, int* pairs_last) {
    if (!h || !rel_pose || !valid) return SSF_ERR_INVALID_ARG;
    { int rc = kf_usable(h, "ssf_keyframes_align", 1); if (rc) return rc; }
    { int rc = kf_lookup(h, "ssf_keyframes_align", id); if (rc) return rc; }
    const KeyframeWs& k = h->kf;
    const KeyframeMeta& m = k.kfs[(size_t)id];
    const size_t N = (size_t)std::max(m.rows, 1), o = (size_t)m.first;
    float *d_lab = nullptr, *d_nrm = nullptr; long long* d_out = nullptr;
    DevTemps tmp;
    HCK(tmp.take(&d_lab, 12 * N)); HCK(tmp.take(&d_nrm, 12 * N)); HCK(tmp.take(&d_out, 40 * sizeof(long long)));
    TimerScope ts(h);
    launch_kf_align_prep(h->stream, k.pool.colors + 3 * o, k.pool.orientations + 9 * o, m.rows, d_lab, d_nrm);
    HCK(hipGetLastError());
    return align_loop(h, k.pool.positions + 3 * o, d_lab, d_nrm, use_conf ? k.pool.confidences + o : nullptr, m.rows, d_out, init_pose, rel_pose, valid, iters,
                      pairs_last);
}
}  // extern "C"
