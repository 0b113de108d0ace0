// ssf_navfoot.hip -- an oriented robot footprint on the navigation grid (include/ssf_navfoot.h) on gfx950: the heading layers of a
// state, and the rollouts of ssf_navsteer.h walked over them.
//
// What is computed is pinned in include/ssf_navfoot.h (the restatement: tests/navfoot_ref.py).
//   * spans  ssf_navfoot_spans: host only.  Per bin and row dy the interval of covered dx, by the header's inequalities over the
//            square of offsets -41..41 (one more than the largest reach, so that a reach above 40 is seen and refused).
//   * layers k_navfoot_layers: one workgroup of 256 per 32 x 32-cell tile.  The tile's window of 32 + 2 reach cells a side (at most
//            112) is held in LDS as BIT ROWS: two 64-bit words a row, bit i = "window column i is clear", made by a wave's ballot over
//            64 cells, so the window costs 1.8 KiB whatever the reach.  A lane takes four cells of the tile.  For a cell at tile column
//            lx and a row dy it shifts the window row's 128 bits right by lx ONCE: bit i of the result is the cell at dx = i - reach.
//            The host has turned every span (bin, dy) into a mask of those bits (two 64-bit words), the same for every lane, so the
//            loops over rows and bins are uniform, the masks come through the scalar cache, and a span test is two ANDs and a compare
//            that clears the bin's bit: no loop over cells, no shift per span.  A row whose 2 reach + 1 cells are all clear skips its
//            bins (in open space a cell costs 2 reach + 1 row tests and nothing else); a row no bin has a span in is skipped for the
//            whole launch; a cell that is itself not clear, or has lost every bin, stops.  No atomics on the mask (every cell is
//            written by its one lane), four atomicAdds per workgroup for the sums, no device-wide barrier.
//   * pack   k_navfoot_pack: one thread per cell: (dist2 >= min_dist2 ? free_mask : 0, d) as one 8-byte word, so the walk's test is
//            one load and (mask & need) == need.
//   * roll, pick  k_navfoot_roll, k_navfoot_pick: ssf_navsteer_walk.hpp's bodies (the walk, the score, the winner, the replay: the
//            same code ssf_navsteer.hip instantiates) with this file's cell test: the packed word in global memory (2 MiB at
//            512 x 512: it sits in L2) under the bins the step sweeps.  Nothing is staged in LDS.
//
// Bounds: a window row index is ly + r with r <= 2 reach and ly < 32, below the window's side; the shift is lx in 0..31 and the bits
// looked at are 0..2 reach <= 80 of 128; the masks' index is below B * (2 reach + 1) * 2, the size uploaded.  The mask and n_free are
// written at cells inside the grid only; the walk reads a cell only after the test that it lies in the grid.
//
// This file is NOT one of the product library's objects.  It is linked, with all of libssf_hip_steer.so's, into libssf_hip_foot.so.
#include "ssf_navsteer_walk.hpp"
#include "../../include/ssf_navfoot.h"

namespace ssf {

enum { NF_RMAX = SSF_NAVFOOT_MAX_REACH, NF_ROWS = SSF_NAVFOOT_ROWS, NF_BINS = SSF_NAVFOOT_MAX_HEADINGS, NF_SIDE = 32 + 2 * NF_RMAX };
// the table a call uploads: per bin b and row r = dy + reach (2 reach + 1 rows) the span as a mask of two 64-bit words, bit i = the
// offset dx = i - reach is covered, at word (b * (2 reach + 1) + r) * 2; after NF_MASK_WORDS words, per row the bins with a span in it
enum { NF_MASK_WORDS = NF_BINS * NF_ROWS * 2, NF_TABLE_BYTES = NF_MASK_WORDS * 8 + NF_ROWS * 4 };
// the sums: cells clear, cells with all / some / none of the bins
enum { NF_CLEAR = 0, NF_ALL = 1, NF_SOME = 2, NF_NONE = 3, NF_STATS = 4 };

// ---- layers: one workgroup per 32 x 32 tile (step 2) ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navfoot_layers(int W, int H, int allow_unknown, int B, int reach, const int8_t* __restrict__ state,
                                                        const unsigned long long* __restrict__ masks, const uint32_t* __restrict__ row_bins,
                                                        uint32_t* __restrict__ mask, uint8_t* __restrict__ n_free, unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long s_row[NF_SIDE][2];                  // the window's bit rows
    const int t = threadIdx.x, wv = t >> 6, ln = t & 63;
    const int side = 32 + 2 * reach, nrow = 2 * reach + 1;
    const int gx0 = (int)blockIdx.x * 32 - reach, gy0 = (int)blockIdx.y * 32 - reach;
    for (int wy = wv; wy < side; wy += 4) {                           // (uniform in a wave: the ballot sees all 64 lanes)
        const int gy = gy0 + wy;
        for (int half = 0; half < 2; half++) {
            const int col = half * 64 + ln, gx = gx0 + col;
            bool c = false;
            if (col < side && gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const int s = state[(size_t)gy * W + gx];
                c = s == 0 || (allow_unknown && s == -1);
            }
            const unsigned long long bits = __ballot(c);
            if (ln == 0) s_row[wy][half] = bits;
        }
    }
    __syncthreads();
    const uint32_t all = B == 32 ? 0xFFFFFFFFu : (1u << B) - 1u;
    // the bits of a shifted row that lie within reach: 0 .. 2 reach
    const unsigned long long full_lo = nrow >= 64 ? ~0ull : (1ull << nrow) - 1ull, full_hi = nrow > 64 ? (1ull << (nrow - 64)) - 1ull : 0ull;
    const int lx = t & 31, gx = (int)blockIdx.x * 32 + lx;
    unsigned long long n_clear = 0, n_all = 0, n_some = 0, n_none = 0;
    for (int k = 0; k < 4; k++) {
        const int ly = (t >> 5) + 8 * k, gy = (int)blockIdx.y * 32 + ly;
        if (gx >= W || gy >= H) continue;
        const int cx = lx + reach, cy = ly + reach;
        const bool own = (s_row[cy][cx >> 6] >> (cx & 63)) & 1ull;
        uint32_t m = own ? all : 0u;
        for (int r = 0; r < nrow && m; r++) {
            const uint32_t bins = row_bins[r];                        // (uniform)
            if (!bins) continue;
            const unsigned long long a = s_row[ly + r][0], c = s_row[ly + r][1];
            // blocked cells of this row at dx = i - reach, i = 0 .. 2 reach: the row shifted right by lx
            const unsigned long long bl = ~(lx ? (a >> lx) | (c << (64 - lx)) : a) & full_lo, bh = ~(c >> lx) & full_hi;
            if (!(bl | bh)) continue;
            for (int b = 0; b < B; b++) {
                if (!(bins >> b & 1u)) continue;                      // (uniform)
                const unsigned long long* mk = masks + ((size_t)b * nrow + r) * 2;
                if ((bl & mk[0]) | (bh & mk[1])) m &= ~(1u << b);
            }
        }
        const size_t p = (size_t)gy * W + gx;
        if (mask) mask[p] = m;
        if (n_free) n_free[p] = (uint8_t)__popc(m);
        n_clear += own; n_all += m == all; n_some += m != 0u && m != all; n_none += m == 0u;
    }
    block_sums({n_clear, n_all, n_some, n_none}, stats, NF_CLEAR);
}

// ---- pack: one thread per cell (step 3's traversable, folded) --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navfoot_pack(size_t P, int min_dist2, int cap, const uint32_t* __restrict__ mask, const int32_t* __restrict__ dist2,
                                                      uint2* __restrict__ pk) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    pk[p] = ns_foot_word(mask, dist2, p, min_dist2, cap);
}

// ---- roll: one workgroup per (pose, 256 candidates) ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navfoot_roll(NavSteerRule r, int B, int shift, const uint2* __restrict__ pk, const uint32_t* __restrict__ cost,
                                                      const int32_t* __restrict__ poses, const int32_t* __restrict__ targets,
                                                      const uint32_t* __restrict__ dirs, unsigned long long* __restrict__ keys,
                                                      int32_t* __restrict__ n_adm, NavSteerCand out, unsigned long long* __restrict__ stats) {
    __shared__ uint32_t s_dir[NS_DIRS];                               // (S << 16) | (C & 0xFFFF)
    ns_foot_roll(r, NsNoHook{}, s_dir, B, shift, pk, cost, poses, targets, dirs, keys, n_adm, out, stats);
}

// ---- pick: one lane per pose ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navfoot_pick(NavSteerRule r, int B, int shift, const uint2* __restrict__ pk, const int32_t* __restrict__ poses,
                                                      const uint32_t* __restrict__ dirs, const unsigned long long* __restrict__ keys,
                                                      const int32_t* __restrict__ n_adm, NavSteerPose out, unsigned long long* __restrict__ stats) {
    const NavFootCells cells{pk, r.W, B, shift};
    ns_pick_body(r, cells, NsNoHook{}, [&](int cx, int cy, int h) { return (pk[(size_t)cy * r.W + cx].x & cells.bin_bit(h)) != 0; }, poses, dirs, keys, n_adm, out,
                 stats);
}

}  // namespace ssf

namespace {
using namespace ssf;

// step 1: what the header's inequalities cover; lo[b][dy + 40], hi likewise, (1, 0) where empty.  nullptr: fine; else what is wrong
struct NavFootSpans { int16_t lo[NF_BINS][NF_ROWS], hi[NF_BINS][NF_ROWS]; int reach; long long cells; };
const char* navfoot_spans(int front, int back, int left, int right, int pad, int B, NavFootSpans& sp) {
    const int sides[4] = {front, back, left, right};
    for (int k = 0; k < 4; k++)
        if (sides[k] < 0 || sides[k] > SSF_NAVFOOT_MAX_SIDE) return "front, back, left and right must be 0..24576";
    if (pad < 0 || pad > SSF_NAVFOOT_MAX_PAD) return "pad must be 0..4096";
    if (nav_log2_bins(B) < 0) return "n_headings must be 1, 2, 4, 8, 16 or 32";
    const NavSteerDirs& dirs = navsteer_dirs();
    const long long u_lo = -(long long)(back + pad) * 16384, u_hi = (long long)(front + pad) * 16384;
    const long long v_lo = -(long long)(right + pad) * 16384, v_hi = (long long)(left + pad) * 16384;
    sp.reach = 0; sp.cells = 0;
    for (int b = 0; b < B; b++) {
        const long long C = dirs.c[b * (NS_DIRS / B)], S = dirs.s[b * (NS_DIRS / B)];
        for (int dy = -NF_RMAX - 1; dy <= NF_RMAX + 1; dy++) {
            int lo = 1, hi = 0;
            for (int dx = -NF_RMAX - 1; dx <= NF_RMAX + 1; dx++) {
                const long long u = 1024 * (dx * C + dy * S), v = 1024 * (dy * C - dx * S);
                if (u < u_lo || u > u_hi || v < v_lo || v > v_hi) continue;
                if (lo > hi) lo = dx;
                hi = dx;
            }
            if (lo <= hi) {
                if (dy < -NF_RMAX || dy > NF_RMAX || lo < -NF_RMAX || hi > NF_RMAX) return "the footprint reaches farther than 40 cells";
                sp.reach = std::max(sp.reach, std::max(std::abs(dy), std::max(std::abs(lo), std::abs(hi))));
                sp.cells += hi - lo + 1;
            }
            if (dy >= -NF_RMAX && dy <= NF_RMAX) { sp.lo[b][dy + NF_RMAX] = (int16_t)lo; sp.hi[b][dy + NF_RMAX] = (int16_t)hi; }
        }
    }
    return nullptr;
}

// the footprint's part of a rollouts call (navsteer_call, ssf_navsteer_walk.hpp): nothing staged, the 8-byte packed grid, the launches
struct NavFootRun {
    ssf_handle* h; int B, shift;
    int stage_cells(const NavSteerRule&) const { return 0; }
    bool reserve(size_t P) { return navfoot_reserve_pk(h, P); }
    int launch(hipStream_t st, const NavSteerRule& r, const void* mask, const int32_t* dist2, const uint32_t* cost, const int32_t* poses,
               const int32_t* targets, NavSteerWs& w, const NavSteerCand& cand, const NavSteerPose& pick) {
        const size_t P = (size_t)r.W * r.H;
        uint2* pk = (uint2*)h->navfoot.pk;
        {
            ScopedKernel sk("navfoot_pack", st);
            hipLaunchKernelGGL(k_navfoot_pack, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, P, r.min_dist2, r.cap, (const uint32_t*)mask, dist2, pk);
        }
        HCK(hipGetLastError());
        {
            ScopedKernel sk("navfoot_roll", st);
            hipLaunchKernelGGL(k_navfoot_roll, dim3((unsigned)((r.K + 255) / 256), (unsigned)r.n_poses), dim3(256), 0, st, r, B, shift, (const uint2*)pk, cost,
                               poses, targets, (const uint32_t*)w.dirs, w.keys, w.n_adm, cand, w.stats);
        }
        HCK(hipGetLastError());
        {
            ScopedKernel sk("navfoot_pick", st);
            hipLaunchKernelGGL(k_navfoot_pick, dim3((unsigned)((r.n_poses + 255) / 256)), dim3(256), 0, st, r, B, shift, (const uint2*)pk, poses,
                               (const uint32_t*)w.dirs, (const unsigned long long*)w.keys, (const int32_t*)w.n_adm, pick, w.stats);
        }
        HCK(hipGetLastError());
        return SSF_OK;
    }
};
}  // namespace

extern "C" {
int ssf_navfoot_spans(int front, int back, int left, int right, int pad, int n_headings, int16_t* spans, int32_t* reach, int64_t* kernel_cells) {
    if (!spans && !reach && !kernel_cells) return SSF_ERR_INVALID_ARG;
    NavFootSpans sp;
    if (navfoot_spans(front, back, left, right, pad, n_headings, sp)) return SSF_ERR_INVALID_ARG;
    if (spans)
        for (int b = 0; b < n_headings; b++)
            for (int k = 0; k < NF_ROWS; k++) { spans[2 * (b * NF_ROWS + k)] = sp.lo[b][k]; spans[2 * (b * NF_ROWS + k) + 1] = sp.hi[b][k]; }
    if (reach) *reach = sp.reach;
    if (kernel_cells) *kernel_cells = sp.cells;
    return SSF_OK;
}

int ssf_navfoot_default_params(const ssf_handle* h, ssf_navfoot_params* p) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    std::memset(p, 0, sizeof(*p));
    p->width = 512; p->height = 512; p->n_headings = 16;
    return SSF_OK;
}

int ssf_navfoot_layers(ssf_handle* h, const ssf_navfoot_params* p, const int8_t* state, const ssf_navfoot_out* out, ssf_navfoot_stats* stats) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    auto refuse = [&](const char* what) { h->err = std::string("ssf_navfoot_layers: ") + what; return SSF_ERR_INVALID_ARG; };
    if (!state) return refuse("state is NULL");
    if (!out || (!out->free_mask && !out->n_free)) return refuse("every output is NULL");
    if (p->width < 1 || p->width > 4096 || p->height < 1 || p->height > 4096) return refuse("the grid's size must be 1..4096 x 1..4096");
    if (p->allow_unknown != 0 && p->allow_unknown != 1) return refuse("allow_unknown must be 0 or 1");
    // the footprint's table is kept on the device from call to call: a robot asks for the same body at control rate, and the spans
    // (220 k inequalities on the host) and their upload would cost more than the kernel
    NavFootWs& w = h->navfoot;
    const int key[6] = {p->front, p->back, p->left, p->right, p->pad, p->n_headings};
    const bool kept = w.table_valid && std::memcmp(key, w.key, sizeof(key)) == 0;
    NavFootSpans sp;
    if (!kept) {
        if (const char* what = navfoot_spans(p->front, p->back, p->left, p->right, p->pad, p->n_headings, sp)) return refuse(what);
    } else {
        sp.reach = w.reach; sp.cells = w.cells;
    }
    { int rc = model_at_rest(h, "ssf_navfoot_layers", "holds no footprint"); if (rc) return rc; }

    const int W = p->width, H = p->height, B = p->n_headings;
    const size_t P = (size_t)W * H;
    const bool dev = p->on_device != 0;
    // the spans as the kernel reads them: a mask of the covered dx per (bin, row), and per row the bins with a span in it
    const int reach = sp.reach, nrow = 2 * reach + 1;
    // (made in the workspace's host buffer, not on this frame's stack: it is the source of two asynchronous copies, and a call that
    // returns early after enqueueing them must not leave them reading a dead frame.  Before it is overwritten the stream is drained,
    // for the same reason: an earlier call may have failed between its enqueue and its synchronisation)
    hipStream_t st = h->stream;
    if (!kept) {
        w.table_valid = false;
        HCK(hipStreamSynchronize(st));
        if (!w.host_table) w.host_table = (unsigned long long*)std::malloc(NF_TABLE_BYTES + 8);
        if (!w.host_table) { h->err = "ssf_navfoot_layers: allocation of the working buffers failed"; return SSF_ERR_DEVICE; }
        std::memset(w.host_table, 0, NF_TABLE_BYTES + 8);
    }
    unsigned long long* table = w.host_table;
    uint32_t* row_bins = (uint32_t*)(table + NF_MASK_WORDS);
    for (int b = 0; b < (kept ? 0 : B); b++)
        for (int r = 0; r < nrow; r++) {
            const int k = r - reach + NF_RMAX;
            for (int dx = sp.lo[b][k]; dx <= sp.hi[b][k]; dx++) table[((size_t)b * nrow + r) * 2 + ((dx + reach) >> 6)] |= 1ull << ((dx + reach) & 63);
            if (sp.lo[b][k] <= sp.hi[b][k]) row_bins[r] |= 1u << b;
        }
    // the arrays of a call with host pointers are staged on the device
    const int8_t* d_state = state; uint32_t* d_mask = out->free_mask; uint8_t* d_n = out->n_free;
    StagedIo io;
    if (!dev) { io.in(state, P, &d_state); io.out(out->free_mask, 4 * P, &d_mask); io.out(out->n_free, P, &d_n); }
    bool ok = true;
    if (!w.stats) ok = w.bufs.grow({{(void**)&w.stats, NF_STATS * sizeof(unsigned long long)}, {(void**)&w.table, NF_TABLE_BYTES}});
    if (ok) ok = io.reserve(w.bufs, &w.io, &w.io_bytes, io.need());
    if (!ok) { h->err = "ssf_navfoot_layers: allocation of the working buffers failed"; return SSF_ERR_DEVICE; }

    TimerScope ts(h);
    if (!kept) {
        w.table_valid = false;                                           // (until both copies are enqueued: a call may fail in between)
        HCK(hipMemcpyAsync(w.table, table, (size_t)B * nrow * 16, hipMemcpyHostToDevice, st));
        HCK(hipMemcpyAsync((unsigned char*)w.table + NF_MASK_WORDS * 8, row_bins, (size_t)nrow * 4, hipMemcpyHostToDevice, st));
        std::memcpy(w.key, key, sizeof(key)); w.reach = sp.reach; w.cells = sp.cells; w.table_valid = true;
    }
    HCK(io.copy_in(st));
    HCK(hipMemsetAsync(w.stats, 0, NF_STATS * sizeof(unsigned long long), st));
    {
        ScopedKernel sk("navfoot_layers", st);
        hipLaunchKernelGGL(k_navfoot_layers, dim3((unsigned)((W + 31) / 32), (unsigned)((H + 31) / 32)), dim3(256), 0, st, W, H, p->allow_unknown, B, sp.reach,
                           d_state, (const unsigned long long*)w.table, (const uint32_t*)((const unsigned char*)w.table + NF_MASK_WORDS * 8), d_mask, d_n,
                           w.stats);
    }
    HCK(hipGetLastError());
    unsigned long long s[NF_STATS];
    HCK(hipMemcpyAsync(s, w.stats, sizeof(s), hipMemcpyDeviceToHost, st));
    HCK(io.copy_out(st));
    { int rc = sync_collect(h); if (rc) return rc; }
    if (stats) {
        stats->cells_clear = (int64_t)s[NF_CLEAR]; stats->cells_all = (int64_t)s[NF_ALL]; stats->cells_some = (int64_t)s[NF_SOME];
        stats->cells_none = (int64_t)s[NF_NONE]; stats->reach = sp.reach; stats->kernel_cells = sp.cells;
    }
    return SSF_OK;
}

int ssf_navfoot_rollouts(ssf_handle* h, const ssf_navsteer_params* p, int n_headings, const uint32_t* free_mask, const int32_t* dist2,
                         const uint32_t* cost, const int32_t* poses, const int32_t* targets, const ssf_navsteer_out* out, ssf_navsteer_stats* stats) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    const int lg = nav_log2_bins(n_headings);
    if (lg < 0) { h->err = "ssf_navfoot_rollouts: n_headings must be 1, 2, 4, 8, 16 or 32"; return SSF_ERR_INVALID_ARG; }
    NavFootRun run{h, n_headings, 16 - lg};
    return navsteer_call(h, "ssf_navfoot_rollouts", p, free_mask, 4, "free_mask", dist2, cost, poses, targets, out, stats, run);
}
}  // extern "C"
