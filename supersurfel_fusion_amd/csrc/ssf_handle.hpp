// ssf_handle.hpp -- the handle (ssf_handle, the types it holds by value, HCK) and the few host helpers that the entry points
// outside ssf_host.hip call.  Private to the library's host code: included by ssf_host.hip (the core ABI, where the helpers are
// defined), by ssf_render.hip, ssf_query.hip, ssf_navgrid.hip, ssf_motion.hip, ssf_odometry.hip, ssf_graph.hip, ssf_graph_solve.hip and ssf_keyframes.hip, whose entry points sit next to their kernels,
// and through ssf_exchange.hpp by ssf_exchange.hip.  Nothing here is part of the frame path's device interface (ssf_device.hpp).
#pragma once
#include <algorithm>
#include <cassert>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <initializer_list>
#include <map>
#include <string>
#include <utility>
#include <vector>
#include "ssf_device.hpp"
#include "ssf_stage_layout.hpp"
#include "../../include/ssf_render.h"
#include "../../include/ssf_graph.h"
#include "../../include/ssf_graph_solve.h"
#include "../../include/ssf_keyframes.h"
#include "../../include/ssf_motion.h"
#include "../../include/ssf_odometry.h"
#include "../../include/ssf_navgrid.h"
#include "../../include/ssf_track.h"

struct ncclComm; typedef struct ncclComm* ncclComm_t;      // (as <rccl/rccl.h> declares it: the handle only holds communicators)
struct Uploader;                                            // the handle only points to it (ssf_host.hip)
namespace ssf {
struct KernelTimer {
    struct Rec { const char* name; hipEvent_t e0, e1; };
    std::vector<Rec> open, pool_free;
    std::vector<Rec> pending;
    std::map<std::string, std::pair<double, long long>> acc;
    const char* cur_name = nullptr; hipEvent_t cur_e0 = nullptr, cur_e1 = nullptr;
    // what an EMPTY (e0, e1) bracket measures on this device: the two event packets themselves (~5 us).  Part of it
    // overlaps with the dispatch when a kernel sits in between: 0.7 x the empty bracket is what makes back-to-back
    // launches agree with rocprofv3's kernel durations (relabelling pass: 14.3 us live vs 14.4 us rocprofv3).
    double bracket_bias_ms = -1.0;
};
}  // namespace ssf
using namespace ssf;          // (as every file that includes this header does: the handle's members are ssf:: types)

// ---- the first ICP iteration of the next frame: inside the row-move kernel, or as a launch of its own? ------------------------
// Both forms give the same record bit for bit (exact integer sums).  Which one is FASTER depends on what else the part is doing,
// and flipped sign between measurements of round 5 (profiles/track_chain_r05.txt): alone on the part the fused form saves a launch
// and a trip (first record 11 us after the frame's entry against 15); next to the extract launches of a filling pipeline its
// 3900-workgroup launch finishes late (36 us against 27) -- the driver's 20-frame form ran 4-7 % faster WITHOUT the fusion, a
// 1200-frame steady state 3-5 % faster WITH it.  So the handle measures: the period between consecutive frame completions of a
// pipelined sequence is attributed to the form that was in effect, the two forms take turns of PROBE frames, and the better mean
// holds for HOLD frames before the next probe.  A handle starts WITHOUT the fusion (short sequences are fill-bound and never leave
// that phase).  Results do not depend on any of it.
struct AheadTuner {
    static const int START = 48, PROBE = 16, ROUNDS = 3, HOLD = 1024, SKIP = 2;
    int forced = -1;                 // lab: SSF_ICP_AHEAD = 0 / 1 / 2 pins the form (2: fused and the track stream waits for the next batch)
    int mode = 0, frames = 0, left = START, round = 0, since_switch = 0;
    bool probing = false;
    double sum[2] = {0, 0}; int n[2] = {0, 0};
    double last_done_us = -1.0; int last_mode = 0;
    int current() const { return forced >= 0 ? (forced ? 1 : 0) : mode; }
    void sequence_break() { last_done_us = -1.0; }                       // (the period across a drained pipeline says nothing)
    void frame_done(double t_us, int iters) {
        if (forced >= 0) return;
        if (last_done_us >= 0.0 && since_switch >= SKIP && probing && iters > 0) { sum[last_mode] += (t_us - last_done_us) / (double)(iters + 4); n[last_mode]++; }   // (per unit of chain work: iterations + the fixed part)
        last_done_us = t_us; last_mode = mode; frames++; since_switch++;
        if (--left > 0) return;
        if (!probing) { probing = true; round = 0; sum[0] = sum[1] = 0; n[0] = n[1] = 0; mode ^= 1; left = PROBE; since_switch = 0; return; }
        if (++round < 2 * ROUNDS) { mode ^= 1; left = PROBE; since_switch = 0; return; }
        probing = false;
        if (n[0] > 0 && n[1] > 0) mode = (sum[1] / n[1] < sum[0] / n[0]) ? 1 : 0;
        left = HOLD; since_switch = 0;
    }
};

// ---- handle -----------------------------------------------------------------------------------------
struct IcpLoop {
    bool active = false, valid = true, done = true;
    int iter = 0;
    unsigned long long ahead_seq = 0;         // != 0: the first iteration's record was accumulated ahead (ssf_handle::ahead)
    double tf_inc[16], prev_error, JtJ[36];
    M3 R_init; V3 t_init, t_inc_stale;
};

// Everything the extract stage of one BATCH of frames owns (cfg.extract_batch frames, slot b of every
// buffer at + b * slab bytes).  With pipeline_depth > 0 there are pipeline_depth + 1 of these, each on
// its own stream: the extract of later batches runs while the track/fuse chain (h->stream) consumes the
// frames of an earlier one.  Extract has no cross-frame state (the RANSAC draws are keyed by the frame
// number), so batches are independent of one another.
struct ExtractCtx {
    FrameMaps maps;                               // slot 0; maps.slab = bytes to the next slot
    SurfelSoA frame;
    unsigned long long* d_best = nullptr; uint8_t* d_matched = nullptr;
    uint8_t* d_rgb_in = nullptr; float* d_depth_in = nullptr; float* d_depth_filt = nullptr; uint8_t* d_mask = nullptr;
    float* d_wire = nullptr;                      // 26 S words: the frame supersurfels of a frame extracted elsewhere (ssf_submit_frame_tables)
    ncclComm_t deal_comm = nullptr;               // dealt extract stage: this context's own communicator (a collective per batch on ITS stream)
    bool mine = true; long long deal_batch = 0;   // ... whether the open batch is this rank's to extract, and its number in the frame stream
    hipStream_t stream = nullptr; bool own_stream = false; int stream_prio = 0;
    hipEvent_t ev_done = nullptr, ev_consumed = nullptr, ev_t0 = nullptr, ev_t1 = nullptr;
    bool consumed_valid = false, timed = false;
    hipGraph_t graph[SSF_MAX_BATCH + 1] = {}; hipGraphExec_t exec[SSF_MAX_BATCH + 1] = {};
    // batch state: open (count > 0, !launched) -> in flight (launched, inflight > 0) -> free
    int count = 0, inflight = 0, stamp0 = 0, nb_launched = 1; bool launched = false, waited = false;
    uint32_t epoch0 = 0;
    BatchIn in = {}; unsigned mask_bits = 0;
    // pixel masks (ssf_dynamic.h): P mask bytes and 2 S pixel counts (total, masked) per slot; bit b of pixmask_bits: slot b has
    // a mask.  A batch with any bit set runs the counting instantiations (k_render_moments<., true>, k_finalize_surfels<true>),
    // whose segmentation chain is captured in a graph of its own.
    uint8_t* d_pixmask = nullptr; uint32_t* d_pixcnt = nullptr; unsigned pixmask_bits = 0;
    bool from_tables = false;                     // the batch came in through ssf_submit_frame_tables: its slot has no colour map
    hipGraph_t graph_pm[SSF_MAX_BATCH + 1] = {}; hipGraphExec_t exec_pm[SSF_MAX_BATCH + 1] = {};
};
// the frame the track/fuse chain works on: slot views into its context
struct ActiveFrame {
    FrameMaps maps; SurfelSoA frame;
    unsigned long long* d_best = nullptr; uint8_t* d_matched = nullptr;
    ExtractCtx* ctx = nullptr; int slot = 0;
    bool pixmask = false;                         // the frame was submitted with a pixel mask: ssf_get_dynamic_superpixels reads its counts
    bool has_rgba = false;                        // the frame was extracted here: maps.rgba is its colour map (ssf_keyframes.h reads it)
    bool activated = false;                       // a submitted frame has been made the current one (ssf_create only points at slot 0)
};

// Round 6: the tile-sorted copy (ssf_tile_rows.inc) in the product, for LARGE visible sets.  At BASELINE config 3 (940 k visible
// rows, ten iterations) it takes k_icp from 23.0 to 19.1 us per iteration and k_match from 55.3 to 31.7 us for a 35 us sort
// (profiles/config3_sorted_rows_r06.txt); at the metric's 120 k visible rows and four iterations the sort costs more than it saves,
// hence the threshold.  -DSSF_BIN_MIN_ROWS_DEFAULT=-1 builds a product without it (the A/B).
#ifndef SSF_BIN_MIN_ROWS_DEFAULT
#define SSF_BIN_MIN_ROWS_DEFAULT 400000
#endif
// The copy has ONE rule.  It is valid from the launch_bin_rows that made it (make_if_large, at the start of a frame's tracking) until the first
// of icp_begin (another frame, or another pose to sort by), fuse_begin (which EVERY frame passes before its rows are rewritten and
// n_visible changes -- also the frame whose association ran inside the waiting k_icp launch and never entered do_match) and
// store_from_dense (the visible array replaced outside a frame: ssf_set_model, deformation, re-homing).  Each of the three calls
// drop; nothing else writes `valid`.  While it is valid the ICP and association launches stream `rows` (icp_rows).
struct TileCopy {
    SurfelSoA rows{};                             // rows.pos: one 48-byte record per row (k_bin_scatter); the other streams stay null
    int32_t* d_idx = nullptr; uint32_t* d_count = nullptr; uint32_t* d_cursor = nullptr;       // launch_match's flag "sorted records" | bin_buffer_words each
    bool valid = false; int min_rows = SSF_BIN_MIN_ROWS_DEFAULT;      // min_rows: visible rows from which a frame's tracking makes the copy (< 0: never)
    long long frames = 0;                         // frames whose tracking made the copy (ssf_tile_copy_frames)
    int make_if_large(ssf_handle* h);             // (ssf_host.hip) the frame's copy, if it wants one: on first use the buffers, then launch_bin_rows
    void drop() { valid = false; }
};
// The device buffers a workspace owns.  grow is all or nothing: allocate every (pointer, bytes) of `want`; only when all succeeded
// free the old buffers and install the new ones.  A failed hipMalloc leaves its error behind in the runtime: it is cleared, so
// that the next frame's launch checks do not report it.  release frees whatever grow installed, and so does the destructor (a
// workspace is a member of the handle: ssf_destroy's `delete h` frees it): a pointer that a workspace gains is named in its grow
// call and nowhere else.
struct DevBufs {
    std::vector<void**> owned;                                    // the workspace's members that hold a buffer
    bool grow(std::initializer_list<std::pair<void**, size_t>> want) {
        std::vector<void*> got;
        for (const auto& w : want) {
            void* q = nullptr;
            if (hipMalloc(&q, std::max<size_t>(w.second, 1)) != hipSuccess) {
                for (void* g : got) (void)hipFree(g);
                (void)hipGetLastError();
                return false;
            }
            got.push_back(q);
        }
        size_t i = 0;
        for (const auto& w : want) { if (*w.first) (void)hipFree(*w.first); else owned.push_back(w.first); *w.first = got[i++]; }
        return true;
    }
    void release() { for (void** q : owned) { (void)hipFree(*q); *q = nullptr; } owned.clear(); }
    DevBufs() = default; DevBufs(const DevBufs&) = delete; ~DevBufs() { release(); }       // (owned points into the workspace that holds this)
};
#pragma GCC visibility push(hidden)       // (StagedIo, BinnedList: the library's own, no part of what it exports)
// The host arrays of one call, carried through a staging buffer on the device: every array is declared ONCE, with its bytes and
// the kernel argument that points at it (on declaration: the caller's own pointer).  reserve grows the buffer when the call needs
// more and points every argument at its item's place (nullptr for a NULL array: not produced); copy_in / copy_out enqueue the
// copies of the inputs / outputs, in the order of declaration; an inout item is in both.  The offsets are StageLayout's
// (ssf_stage_layout.hpp).
struct StagedIo {
    StageLayout lay;
    void** arg[StageLayout::MAX_ITEMS];
    static_assert(StageLayout::MAX_ITEMS <= 32, "inputs and outputs hold a bit per item");
    unsigned inputs = 0, outputs = 0;                             // bit i: item i is read (host -> device) / written (device -> host) by the device
    void add(const void* host, size_t bytes, void** dev, bool in, bool out) {
        const int i = lay.add(host, bytes);
        assert(i >= 0);                                           // (more items than StageLayout::MAX_ITEMS: raise it)
        arg[i] = dev; if (in) inputs |= 1u << i; if (out) outputs |= 1u << i;
    }
    template <typename T> void out(T* host, size_t bytes, T** dev) { add(host, bytes, (void**)dev, false, true); }
    template <typename T> void in(const T* host, size_t bytes, const T** dev) { add(host, bytes, (void**)dev, true, false); }
    template <typename T> void inout(T* host, size_t bytes, T** dev) { add(host, bytes, (void**)dev, true, true); }
    size_t need() const { return lay.total; }
    // *buf holds *have bytes: grown to cap (>= need(), the caller's growth rule) when need() does not fit
    bool reserve(DevBufs& bufs, unsigned char** buf, size_t* have, size_t cap) {
        if (need() > *have) { if (!bufs.grow({{(void**)buf, cap}})) return false; *have = cap; }
        for (int i = 0; i < lay.n; i++) *arg[i] = lay.at(*buf, i);
        return true;
    }
    hipError_t copy(hipStream_t st, bool in) const {
        for (int i = 0; i < lay.n; i++) {
            const StageLayout::Item& it = lay.item[i];
            if (!it.host || !(((in ? inputs : outputs) >> i) & 1u)) continue;
            const hipError_t e = in ? hipMemcpyAsync(*arg[i], it.host, it.bytes, hipMemcpyHostToDevice, st)
                                    : hipMemcpyAsync(const_cast<void*>(it.host), *arg[i], it.bytes, hipMemcpyDeviceToHost, st);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    hipError_t copy_in(hipStream_t st) const { return copy(st, true); }
    hipError_t copy_out(hipStream_t st) const { return copy(st, false); }
};
// (bin -> slot) lists: per bin (+ 1) the counts that launch_slots_scan turns into offsets and a copy of them, the fill's cursors,
// and the list.  The caller zeroes off[0 .. bins], counts, scans and reads the 64-bit total; then reserve_list; then fills.
struct BinnedList {
    uint32_t* off = nullptr; uint32_t* cursor = nullptr; size_t bin_cap = 0;          // bin_cap words each (bins + 1)
    uint32_t* list = nullptr; size_t list_cap = 0;
    bool reserve_bins(DevBufs& bufs, size_t bins) {
        if (bins + 1 <= bin_cap) return true;
        if (!bufs.grow({{(void**)&off, 4 * (bins + 1)}, {(void**)&cursor, 4 * (bins + 1)}})) return false;
        bin_cap = bins + 1;
        return true;
    }
    // room for `total` entries: more than 2^32 - 1 are refused, a list that grows takes a quarter more (capped there).  On a
    // failure (SSF_ERR_DEVICE) err is the caller's wording: too_many, or alloc_a [+ the bytes asked for + alloc_b]
    int reserve_list(DevBufs& bufs, unsigned long long total, std::string& err, const char* too_many, const char* alloc_a, const char* alloc_b = nullptr) {
        if (total > 0xFFFFFFFFull) { err = too_many; return SSF_ERR_DEVICE; }
        if (total <= list_cap) return SSF_OK;
        const size_t cap = std::min<unsigned long long>(total + total / 4, 0xFFFFFFFFull);
        if (!bufs.grow({{(void**)&list, 4 * cap}})) {
            err = alloc_b ? alloc_a + std::to_string(4 * cap) + alloc_b : std::string(alloc_a);
            return SSF_ERR_DEVICE;
        }
        list_cap = cap;
        return SSF_OK;
    }
};
#pragma GCC visibility pop
// working buffers of ssf_render_model (ssf_render.h): allocated on first use; each group (per slot / per tile / list / staged images)
// is grown as a whole or not at all (DevBufs::grow)
struct RenderWs {
    DevBufs bufs;
    float4* rec = nullptr; uint2* rbox = nullptr; int32_t* logical = nullptr; uint32_t* seen = nullptr; uint32_t* bc = nullptr;
    size_t slots = 0;                                              // per slot: record, pixel box, logical index, `seen` epoch
    BinnedList tl;                                                // (tile -> slot) lists, a bin per 16 x 16 tile
    unsigned long long* stats = nullptr;                          // fragments, filled pixels, rows shown, list entries
    unsigned char* img = nullptr; size_t img_bytes = 0;           // host outputs, staged on the device
    uint32_t epoch = 0;                                           // of the last render: seen[slot] == epoch <=> shown by it
};
// working buffers of ssf_motion_* (ssf_motion.h), P = W * H of the handle's camera: allocated on first use as a whole or not at
// all (DevBufs::grow), 31 bytes per pixel.  `last` and last_stats keep the mask of the last ssf_process_frame_motion: the frame's
// extract context copies from it, and later ssf_motion_mask calls do not touch it.
struct MotionWs {
    DevBufs bufs;
    unsigned char* din = nullptr;                                 // a host depth image, uploaded in the input format (4 P)
    float* m = nullptr; float* d32 = nullptr;                     // model depth (rendered or uploaded); the frame's depth in metres
    uint8_t* cls = nullptr; int32_t* parent = nullptr; int32_t* label = nullptr;
    // (seed, unknown) pixels: of a tile's component at its local root, then of the component at its root.  A word that is no local
    // root's is never written and must never be read: k_motion_roots reads cnt[p] only where label[p] >= 0, k_motion_decide only cnt[label[p]]
    uint2* cnt = nullptr;
    uint8_t* mask = nullptr; uint8_t* last = nullptr;
    unsigned long long* stats = nullptr;                          // ssf_motion_stats' five counts
    size_t pixels = 0;
    bool have_last = false; ssf_motion_stats last_stats{};
};
// ssf_odometry_* (ssf_odometry.h): two pyramids (I, D, gx, gy; every level in one buffer each, level l at off[l]) that swap the
// roles of reference and current, the staged host images, the record.  Allocated on first use as a whole or not at all
// (DevBufs::grow).  Nothing here is read or written by the frame path.
struct OdoPyramid { float* I = nullptr; float* D = nullptr; float* gx = nullptr; float* gy = nullptr; };
struct OdoWs {
    DevBufs bufs;
    OdoPyramid pyr[2]; int ref = 0;                               // pyr[ref] is the reference, pyr[1 - ref] the current frame
    unsigned char* rgb_in = nullptr; unsigned char* depth_in = nullptr; uint8_t* mask_in = nullptr;     // host images, uploaded (4 P, 4 P, P)
    unsigned long long* rec = nullptr;                            // the 29-word record
    size_t pixels = 0;
    int levels = 0, lw[SSF_ODO_MAX_LEVELS] = {}, lh[SSF_ODO_MAX_LEVELS] = {}; size_t off[SSF_ODO_MAX_LEVELS + 1] = {};
    float lfx[SSF_ODO_MAX_LEVELS] = {}, lfy[SSF_ODO_MAX_LEVELS] = {}, lcx[SSF_ODO_MAX_LEVELS] = {}, lcy[SSF_ODO_MAX_LEVELS] = {};
    bool have_ref = false, have_cur = false, ref_pose_pending = false, have_last = false;
    Rt ref_pose;
    float last_rel[12] = {}, last_prior[12] = {}; ssf_odometry_result last_result{};
};
// ssf_graph_build (ssf_graph.h): the resident node table and binding, and the working buffers of the time-order sort.  Allocated
// on first use; each group (per slot / per node) is grown as a whole or not at all (DevBufs::grow)
struct GraphWs {
    DevBufs bufs;
    int32_t* stamp = nullptr; uint8_t* elig = nullptr; int32_t* key_a = nullptr; int32_t* key_b = nullptr;
    uint32_t* slot_a = nullptr; uint32_t* slot_b = nullptr; uint32_t* cnt = nullptr; uint32_t* bc = nullptr;
    float* w4 = nullptr; int32_t* idx4 = nullptr; int* mm = nullptr; size_t slots = 0;       // per slot; w4 / idx4 per logical row
    float4* nodes = nullptr; float* npos3 = nullptr; int32_t* nrow = nullptr; size_t node_cap = 0;   // per node, in time order
    int m = 0, rows = 0, look = 0; bool built = false; unsigned long long gen = 0;          // valid <=> built && gen == h->model_gen
};
// ssf_graph_solve (ssf_graph_solve.h): the solver's vectors (f64, 12 per node), the residual-space vectors, the two transposed
// lists and the solved transforms.  Allocated on first use; each group (per node / per constraint) is grown as a whole or not at
// all (DevBufs::grow).  Nothing here is read or written by the frame path.
struct SolveWs {
    DevBufs bufs;
    // per node
    int32_t* edges = nullptr; uint32_t* in_off = nullptr; uint32_t* con_off = nullptr;
    double *x = nullptr, *b = nullptr, *D = nullptr, *delta = nullptr, *r = nullptr, *z = nullptr, *p0 = nullptr, *p1 = nullptr, *q = nullptr;
    double *y_rot = nullptr, *y_reg = nullptr;                       // 6 / 12 per node: residuals, then J p
    double* part = nullptr;                                          // block partials: see ssf_graph_solve.hip
    float *rot = nullptr, *trans = nullptr; size_t node_cap = 0;
    // per constraint
    float *src = nullptr, *dst = nullptr, *w4 = nullptr; int32_t *t0 = nullptr, *idx4 = nullptr; double *y_con = nullptr, *e_con = nullptr; size_t con_cap = 0;
    // the counting sorts' working set, for max(4 m, 4 n_con) items
    int32_t *key_a = nullptr, *key_b = nullptr; uint32_t *slot_a = nullptr, *slot_b = nullptr, *cnt = nullptr, *in_list = nullptr, *con_list = nullptr;
    size_t item_cap = 0;
    bool solved = false; unsigned long long gen = 0;                 // the transforms belong to the graph of that generation
};
// the keyframe database of ssf_keyframes.h: everything is allocated by ssf_keyframes_configure, as a whole or not at all
// (DevBufs::grow), and freed by ssf_keyframes_clear / ssf_destroy.  The host mirrors what it needs to address a keyframe (its
// first pool row, row count, stamp, pose); codes, stamps and rows live on the device.
struct KeyframeMeta { long long first; int rows; int stamp; float pose[12]; };
struct KeyframeWs {
    DevBufs bufs;
    ssf_keyframes_params p{}; bool on = false;
    int words = 0, gw = 0, gh = 0;
    uint4* ferns = nullptr; uint32_t* q = nullptr; uint32_t* table = nullptr; int32_t* stamps = nullptr; uint32_t* diff = nullptr;
    int32_t* rec = nullptr; uint8_t* bytes = nullptr;
    ssf_surfels pool{};                           // the row pool: device arrays, a keyframe's rows consecutive (what _get / _put copy as they are)
    std::vector<ssf_fern> host_ferns; std::vector<KeyframeMeta> kfs; long long rows_used = 0;
};
// ssf_query_count / ssf_query_rows (ssf_query.h): the ballot mask (one word per 64 slots), the interleaved block counts (selected,
// live out-of-view) that the scan turns into offsets, the out-of-view blocks' live offsets, the record the host reads, and the
// staging buffer of host outputs.  Allocated on first use; each group is grown as a whole or not at all (DevBufs::grow)
struct QueryWs {
    DevBufs bufs;
    unsigned long long* mask = nullptr; uint32_t* cnt = nullptr; uint32_t* bc = nullptr; size_t slots = 0;
    uint32_t* rec = nullptr;
    unsigned char* rows = nullptr; size_t rows_bytes = 0;
};
// ssf_navgrid_build (ssf_navgrid.h): per slot the grid-frame record and the cell box, per 32 x 32-cell tile (+ 1) the counts that
// the scan turns into list offsets and the fill's cursors, the (tile -> slot) lists, per cell the four accumulator words, the column distances and
// the state when the caller did not ask for it, the seven 64-bit sums, and the staging buffer of host outputs.  Allocated on first use;
// each group is grown as a whole or not at all (DevBufs::grow).  Nothing here is read or written by the frame path.
struct NavGridWs {
    DevBufs bufs;
    float4* rec = nullptr; uint2* rbox = nullptr; size_t slots = 0;
    BinnedList tl;                                                // (tile -> slot) lists, a bin per 32 x 32-cell tile
    uint32_t* acc = nullptr; uint16_t* colg = nullptr; int8_t* state = nullptr; size_t cells = 0;
    unsigned long long* stats = nullptr;
    unsigned char* img = nullptr; size_t img_bytes = 0;
};
// ssf_navgrid_carve (ssf_navcarve.h, ssf_navcarve.hip: linked into libssf_hip_navcarve.so only), next to NavGridWs, which it shares with ssf_navgrid_build: the views (4096 x 12 floats), a
// chunk of rays with their hits (t, index), per cell the ray entries, the sums.  Allocated on first use; each group is grown as a
// whole or not at all (DevBufs::grow).  chunk_rays: the test hook (0 = 2^20 rays per chunk); last_*: what the last call did.
struct NavCarveWs {
    DevBufs bufs;
    float* views = nullptr; unsigned long long* stats = nullptr;
    float* rays = nullptr; float* t = nullptr; int32_t* index = nullptr; size_t ray_cap = 0;
    uint32_t* seen = nullptr; size_t cells = 0;
    int chunk_rays = 0; long long last_chunks = 0, last_atomics = 0;
};
// ssf_navplan_field (ssf_navplan.h, ssf_navplan.hip: linked into libssf_hip_nav.so only): per cell the packed (traversable, penalty)
// word, the cost and the frontier; per 32 x 32-cell tile the two ping-pong flag words; the goals (65536 pairs) and starts (4096 pairs)
// with the starts' results; the paths of a call with host outputs and the staging buffer of its host grid (state, dist2); the sums.
// Allocated on first use; each group is grown as a whole or not at all (DevBufs::grow).  round_batch: the test hook (0 = the
// default); last_*: what the last call did.  Nothing here is read or written by the frame path.
struct NavPlanWs {
    DevBufs bufs;
    uint32_t* pk = nullptr; uint32_t* cost = nullptr; uint8_t* frontier = nullptr; size_t cells = 0;
    unsigned char* io = nullptr; size_t io_bytes = 0;
    uint32_t* flags = nullptr; size_t tiles = 0;
    int32_t* goals = nullptr; int32_t* starts = nullptr; uint32_t* start_cost = nullptr; int32_t* start_status = nullptr; int32_t* path_len = nullptr;
    unsigned long long* stats = nullptr;
    int32_t* path = nullptr; size_t path_words = 0;
    int round_batch = 0; long long last_rounds = 0, last_visits = 0;
};
// ssf_navfrontier_regions (ssf_navfrontier.h, ssf_navfrontier.hip: linked into libssf_hip_explore.so only): per cell the union-find's
// parent word and the label; per 256 cells and per 256 regions (+ 1) the counts that are scanned into offsets; per region found the
// accumulators (acc: NavFrontierAcc, ssf_navfrontier.hip); the table (65536 records) and the sums; the staging buffer of a call with
// host arrays (state, dist2, cost).  Allocated on first use; each group is grown as a whole or not at all (DevBufs::grow).
// Nothing here is read or written by the frame path.
struct NavFrontierWs {
    DevBufs bufs;
    int32_t* parent = nullptr; int32_t* label = nullptr;
    uint32_t* cell_blocks = nullptr; size_t cells = 0;
    unsigned char* io = nullptr; size_t io_bytes = 0;
    void* acc = nullptr; uint32_t* region_blocks = nullptr; size_t regions = 0;
    void* table = nullptr; unsigned long long* stats = nullptr;
};
// ssf_navpath_waypoints (ssf_navpath.h, ssf_navpath.hip: linked into libssf_hip_drive.so only): per cell the packed (traversable, d)
// word; per path (4096) the status, waypoint count and minimum; the paths and the waypoints of a call with host arrays and the
// staging buffer of its whole-array inputs (state, dist2, path_len); the sums.  Allocated on first use; each group is grown as a
// whole or not at all (DevBufs::grow).  Nothing here is read or written by the frame path.
struct NavPathWs {
    DevBufs bufs;
    uint32_t* pk = nullptr; size_t cells = 0;
    int32_t* status = nullptr; int32_t* n_wp = nullptr; int32_t* path_min = nullptr; unsigned long long* stats = nullptr;
    int32_t* path = nullptr; size_t path_words = 0;
    int32_t* wp = nullptr; size_t wp_words = 0;
    unsigned char* io = nullptr; size_t io_bytes = 0;
};
// ssf_navlive_overlay (ssf_navlive.h, ssf_navlive.hip: linked into libssf_hip_live.so only): per cell the points and the ray entries of
// the frame, the column distances of the clearance and the state when the caller did not ask for it (11 bytes); the sums; the staging
// buffer of host arrays (depth, mask, state_in and the outputs).  Allocated on first use; each group is grown as a whole or not at
// all (DevBufs::grow).  Nothing here is read or written by the frame path.
struct NavLiveWs {
    DevBufs bufs;
    uint32_t* hits = nullptr; uint32_t* seen = nullptr; uint16_t* colg = nullptr; int8_t* state = nullptr; size_t cells = 0;
    unsigned long long* stats = nullptr;
    unsigned char* img = nullptr; size_t img_bytes = 0;
};
// ssf_navsteer_rollouts (ssf_navsteer.h, ssf_navsteer.hip: linked into libssf_hip_steer.so only): per cell the packed (traversable, d)
// word; per pose (4096) the smallest (score, candidate) key and the admissible count; the packed direction table (uploaded once);
// the sums; the staging buffer of a call with host arrays.  Allocated on first use; each group is grown as a whole or not at all
// (DevBufs::grow).  Nothing here is read or written by the frame path.
struct NavSteerWs {
    DevBufs bufs;
    uint32_t* pk = nullptr; size_t cells = 0;
    unsigned long long* keys = nullptr; int32_t* n_adm = nullptr; uint32_t* dirs = nullptr; unsigned long long* stats = nullptr;
    bool dirs_sent = false;                       // the table's upload has been enqueued (a call may fail between allocation and upload)
    unsigned char* io = nullptr; size_t io_bytes = 0;
};
// ssf_navdyn_blobs (ssf_navdyn.h, ssf_navdyn.hip: linked into libssf_hip_dyn.so only): per pixel the point (bx, by) of a contributing
// pixel and, per label value, its compact slot (12 bytes a pixel); the per-label records (40 bytes, one per pixel at the most); the
// sums; the staging buffer of host images.  The rollouts with movers use NavSteerWs and NavFootWs.  Allocated on first use; each
// group is grown as a whole or not at all (DevBufs::grow).  Nothing here is read or written by the frame path.
struct NavDynWs {
    DevBufs bufs;
    int2* pt = nullptr; int32_t* slot = nullptr; unsigned char* rec = nullptr; size_t pixels = 0;
    unsigned long long* stats = nullptr;
    unsigned char* img = nullptr; size_t img_bytes = 0;
};
// ssf_navmem_update (ssf_navmem.h, ssf_navmem.hip: linked into libssf_hip_mem.so only): per cell the points, the hit bits and the seen
// bits of the frame (one more u32 plane than NavLiveWs: the hit bits beside the points), the column distances of the clearance and
// the state when the caller did not ask for it (15 bytes); the sums; the staging buffer of host arrays.  The layer itself is the
// caller's, never the handle's.  Allocated on first use; each group is grown as a whole or not at all (DevBufs::grow).  Nothing here
// is read or written by the frame path.
struct NavMemWs {
    DevBufs bufs;
    uint32_t* hits = nullptr; uint32_t* hit_bits = nullptr; uint32_t* seen_bits = nullptr; uint16_t* colg = nullptr; int8_t* state = nullptr;
    size_t cells = 0;
    unsigned long long* stats = nullptr;
    unsigned char* img = nullptr; size_t img_bytes = 0;            // staged host arrays: depth, mask, state_in, the layer, the outputs
};
// ssf_navfloor_fit (ssf_navfloor.h, ssf_navfloor.hip: linked into libssf_hip_floor.so only): per slot the 32-byte candidate record; the
// sums (rows, candidates, the record cursor, the direction's four words, the height's two, ten per round); the two histograms.
// Allocated on first use; each group is grown as a whole or not at all (DevBufs::grow).  Nothing here is read or written by the
// frame path.
struct NavFloorWs {
    DevBufs bufs;
    float4* rec = nullptr; size_t slots = 0;
    unsigned long long* stats = nullptr; uint32_t* hist = nullptr;
};
// ssf_navfoot_layers and ssf_navfoot_rollouts (ssf_navfoot.h, ssf_navfoot.hip: linked into libssf_hip_foot.so only): the footprint's
// table of spans as the layers kernel reads it (kept from call to call while the footprint is the same), the layers' sums and the staging buffer of a layers call with host arrays; per cell
// the rollouts' packed (heading mask, d) word of 8 bytes.  The rollouts' keys, counts, direction table, sums and staging are
// NavSteerWs's.  Allocated on first use; each group is grown as a whole or not at all (DevBufs::grow).  Nothing here is read or
// written by the frame path.
struct NavFootWs {
    DevBufs bufs;
    unsigned long long* table = nullptr; unsigned long long* stats = nullptr;
    int key[6] = {0, 0, 0, 0, 0, 0}; int reach = 0; long long cells = 0; bool table_valid = false;      // the footprint the table on the device is of
    // the table as it is uploaded (malloc, freed with the handle): it outlives the call, whose copies may still read it after an early return
    unsigned long long* host_table = nullptr;
    NavFootWs() = default; NavFootWs(const NavFootWs&) = delete; ~NavFootWs() { std::free(host_table); }
    unsigned char* io = nullptr; size_t io_bytes = 0;
    unsigned long long* pk = nullptr; size_t pk_cells = 0;
};
// ssf_navpose_field (ssf_navpose.h, ssf_navpose.hip: linked into libssf_hip_pose.so only): per cell the packed (traversable bins,
// penalty) word of 8 bytes and the projection (cell_cost, cell_bin); per state the cost; per 16 x 16-cell tile the two ping-pong flag
// words; the goals (65536 triples) and starts (4096 triples) with the starts' results; the paths of a call with host outputs and the
// staging buffer of its host grid (free_mask, dist2); the sums.  Allocated on first use; each group is grown as a whole or not at
// all (DevBufs::grow).  Nothing here is read or written by the frame path.
struct NavPoseWs {
    DevBufs bufs;
    unsigned long long* pk = nullptr; uint32_t* cell_cost = nullptr; uint8_t* cell_bin = nullptr;
    size_t cells = 0;
    unsigned char* io = nullptr; size_t io_bytes = 0;
    uint32_t* cost = nullptr; size_t states = 0;
    uint32_t* flags = nullptr; size_t tiles = 0;
    int32_t* goals = nullptr; int32_t* starts = nullptr; uint32_t* start_cost = nullptr; int32_t* start_status = nullptr; int32_t* path_len = nullptr;
    unsigned long long* stats = nullptr;
    int32_t* path = nullptr; size_t path_words = 0;
};
// ssf_raycast (ssf_raycast.h): the resident index -- per slot the 64-byte record and the box of cells with the row's class, the
// out-of-view blocks' live offsets, the oversize list; per bucket (+ 1) the list offsets and the fill's cursors; the (bucket -> slot)
// lists; the sums and the box of indexed cells -- and the staging buffer of a call's host rays and outputs.  The index is valid
// <=> built && gen == h->model_gen && recentres == h->n_recentres (a compaction moves rows to other slots) && (cell, s, hash_bits)
// are the call's.  Allocated on first use; each group is grown as a whole or not at all (DevBufs::grow).  Nothing here is read or
// written by the frame path.
struct RayIndex {                                   // what the march needs of the index
    float cell, s, k;
    uint32_t mask;
    int cmin[3], cmax[3];                           // the box of indexed cells (cmin > cmax: the grid is empty)
    int n_over, nvs;                                // oversize list length; slots below nvs are visible rows
    float cabs;                                     // the largest |coordinate| of the indexed cells' box, metres
};
struct RaycastWs {
    DevBufs bufs;
    float4* rec = nullptr; uint4* rbox = nullptr; uint32_t* bc = nullptr; uint32_t* over = nullptr; size_t slots = 0;
    BinnedList bl;                                  // (bucket -> slot) lists, a bin per bucket of the table
    unsigned long long* stats = nullptr; int* cbox = nullptr;
    unsigned char* io = nullptr; size_t io_bytes = 0;
    RayIndex ix{};
    bool built = false; unsigned long long gen = 0; long long recentres = 0; float cell = 0, s = 0; int hash_bits = 0;
    long long rows_indexed = 0, rows_oversize = 0, entries = 0;
};
struct ssf_handle {
    ssf_config cfg;
    int S = 0, gx = 0, gy = 0;
    std::string err;
    hipStream_t stream = nullptr; bool own_stream = false; int stream_prio = 0;
    SegParams seg; Cam cam;
    std::vector<ExtractCtx> ctx; int open_ctx = 0, batch = 1;
    std::deque<std::pair<int, int>> pending;      // (context, slot) submitted, not yet processed (oldest first)
    ActiveFrame active; ActiveFrame* cc = &active; // the frame the track/fuse chain is working on (or last worked on)
    uint32_t extract_ordinal = 0;                 // frames submitted so far = RNG epoch of the next frame
    // ssf_process_sequence: frames still to be submitted; do_fuse submits them between its launches and its wait for
    // the counters (the ~40 us of host work of a batch launch hide behind the ~55 us fuse chain on the GPU)
    const void* const* seq_rgb = nullptr; const void* const* seq_depth = nullptr; const uint8_t* const* seq_pixmask = nullptr; int seq_next = 0, seq_n = 0, seq_on_device = 0, stamp_bias = 0;
    long long n_waiter_matches = 0;           // frames whose association ran in a waiting ICP launch (debug)
    int seq_k = 0;                            // frame of the sequence the track loop is working on (debug marks)
    int seq_batches = 0;                      // batches launched by the running ssf_process_sequence (see seq_batch_size)
    double us_wait_upload = 0.0;                          // the submitting thread's wait for uploads (ssf_upload_stats)
    Uploader* up = nullptr; bool seq_upload = false;   // host frames of a sequence are copied ahead by a worker thread
    // the format every frame entry point reads its images in (ssf_set_input_format, ssf_input.h); the buffers that hold frames
    // on the device (batch input slabs, upload ring, pre-filter input) are sized for the largest one, so a change allocates nothing
    int in_color = SSF_COLOR_RGB8, in_depth = SSF_DEPTH_F32_METRES; double in_scale = 1.0;
    // multi-GPU: RCCL communicator over the ranks of cfg.nranks (ssf_comm_attach); the shard sizes of all ranks
    // are all-gathered at the end of every frame and read lazily at the start of the next one
    ncclComm_t comm = nullptr; int* d_all5 = nullptr;
    int deal = 0; long long deal_batches = 0;     // ssf_comm_deal_extract: 0 replicated, 1 dealt, 2 dealt + the extracting rank re-imports its own tables (self-check)
    // ... or the peer-to-peer exchange region of ssf_p2p_* (one node; no collective launches): own region, the peers'
    // regions as mapped into this process, and one sequence number per exchange kind (identical on every rank)
    struct P2P {
        unsigned char* region = nullptr; size_t bytes = 0; bool fine = false;
        bool same_device = false; double timeout_s = 30.0;       // ssf_p2p_configure
        P2PView view{}; bool on = false; std::vector<void*> opened;
        unsigned long long seq_icp = 0, seq_cnt = 0, seq_assoc = 0, seq_migr = 0;
    } p2p;
    unsigned long long all_seq = 0; bool all_pending = false, all_valid = false;
    long long all_cnt[5 * SSF_MAX_RANKS];
    SurfelSoA model[2]; int mcur = 0;
    std::vector<void*> allocs;
    struct Guarded { void* base; size_t bytes, guard; };
    std::vector<Guarded> guarded;         // SSF_ALLOC_GUARD (debug): see dalloc
    float* d_bf_in = nullptr; float* d_bf_out = nullptr; float* d_orient9 = nullptr; float* d_frame_orient9 = nullptr;
    long long* d_icp = nullptr;
    uint8_t* d_state = nullptr; int32_t* d_cand = nullptr; Counters* d_cnt = nullptr;
    // multi-GPU migration: this shard's migrant table (SSF_MIGRANT_WORDS x S int32), state between the two fuse halves
    int32_t* d_migrants = nullptr; PartitionWs fuse_ws{}; bool fuse_first = false, fuse_migrate = false, fusing = false;
    MoveTotals fuse_totals{0, 0, 0, 0}; bool move_totals_on = true;      // (lab: SSF_MOVE_TOTALS=0 keeps the fuse launch's tail)
    // model store: model[mcur] = dense array of the visible rows (ping-pong), oov[ocur] = out-of-view rows (deque
    // with live flags, host mirror of the span below), dense = materialised [visible | out-of-view] view for the
    // consumers of the whole model (get/set model, export, deformation)
    OovStore oov[2]; int ocur = 0; int oov_head = 0, oov_tail = 0, oov_live = 0; long long n_recentres = 0;
    uint8_t* d_state_oov = nullptr; uint32_t* d_bc_oov = nullptr;
    // sums of the per-frame partition (PartitionWs): two sets of part_words, used alternately; 128 arrival counters
    uint32_t* d_part = nullptr; uint32_t* d_part_ticket = nullptr; int part_words = 0, part_sup_vis = 0, part_sup_oov = 0, part_set = 0;
    SurfelSoA dense; uint8_t* d_live_scratch = nullptr;
    int32_t* d_scratch_map = nullptr;
    long long* d_icp_replicas = nullptr; unsigned int* d_tickets = nullptr; float* d_srgb_lut = nullptr;
    // host-mapped mailbox (fine-grained): results the host waits for are polled, not synchronised on
    Mailbox* mb_host = nullptr; Mailbox* mb_dev = nullptr;
    unsigned long long icp_seq = 0, cnt_seq = 0;
    // first ICP iteration of the next submitted frame, accumulated ahead by the row-move kernel of the frame just
    // fused (do_fuse): valid for exactly that frame, that pose and that model; anything else drops it
    struct { bool valid = false; unsigned long long seq = 0; ExtractCtx* ctx = nullptr; int slot = 0; int stamp = 0; Rt pose; } ahead;
    int assoc_rstride = 0;                // the frame in process_oldest bids into the replicas of its association table (0: table 0 alone)
#ifdef SSF_EXPERIMENTS
    long long n_assoc_replica_frames = 0; // frames that did (ssf_dbg_assoc_replica_frames)
#endif
    double wait_launched_us = 0.0; long long n_waiter_match_repairs = 0; long long dbg_stall_before_match_us = 0;     // see process_oldest: SSF_ICP_GO_MATCH has no acknowledgement
    bool icp_ahead = true; int icp_ahead_mode = 1;         // 1: when the next frame's extract has finished (the product); 2 (lab): always, the track stream waits for it
    AheadTuner ahead_tuner;
    // chained ICP launches: iteration i + 1 is launched while iteration i runs and waits on the device for the host's
    // word (launch_icp, IcpGo): slots in fine-grained device memory the host stores into directly
    IcpGo* go = nullptr; bool icp_chain = true; unsigned long long go_count = 0;
    // the resident ICP launch (launch_icp_resident): two sets (frame parity) of cfg.icp_iter + 1 lines behind the SSF_ICP_GO_SLOTS
    // of `go`, one per iteration index | visible rows up to which a frame takes it (a safety condition: every workgroup of the
    // launch must hold a place at once; tests lower it) | frames that took it, those of them that started behind a record made ahead,
    // launches made (picks the set of lines)
    IcpGo* go_res = nullptr; int resident_max_rows = 0; long long n_resident_frames = 0, n_resident_ahead_frames = 0, n_resident_launches = 0;
    bool graph_failed = false; hipStream_t capture_stream = nullptr;
    TileCopy bins;                                // tile-sorted copy of the visible rows' ICP / association fields, for large visible sets
    // what the fuse launches take as groups: built by ssf_create; plane_depth and migrate are the frame's (fuse_begin)
    ClassifyArgs classify{}; ShardArgs shard{};
    long long h_icp_local[SSF_ICP_RECORD];
    long long* h_icp = nullptr; Counters* h_cnt = nullptr;
    int n_model = 0, n_visible = 0, stamp = 0, max_passes = 0;
    Rt pose;
    IcpLoop icp;
    long long id_offset = 0, global_n_model = -1, global_n_visible = -1;
    bool have_frame = false;
    int last_icp_valid = 0, last_icp_iters = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    KernelTimer timer;
    std::vector<std::string> timer_names;
    double seq_mark_us[4][64] = {{0}}, seq_launch_us[32] = {0}, seq_launch_host_us[32] = {0}; int seq_launch_n[32] = {0}, seq_launches = 0;   // debug: entry / first ICP record / ICP done / counters back per frame, batch launches
    double seq_t0_us = 0, seq_done_us[64] = {0};      // debug: completion time of the first frames of the last ssf_process_sequence
    double host_us[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // debug: submit | icp loop | match+fuse | frames | extract ready at activation | first icp iteration
    RenderWs render;                              // ssf_render_model (ssf_render.h)
    GraphWs graph;                                // ssf_graph_* (ssf_graph.h)
    KeyframeWs kf;                                // ssf_keyframes_* (ssf_keyframes.h)
    SolveWs solve;                                // ssf_graph_solve (ssf_graph_solve.h)
    QueryWs query;                                // ssf_query_* (ssf_query.h)
    MotionWs motion;                              // ssf_motion_* (ssf_motion.h)
    OdoWs odo;                                    // ssf_odometry_* (ssf_odometry.h)
    NavGridWs navgrid;                            // ssf_navgrid_build (ssf_navgrid.h)
    NavCarveWs navcarve;                          // ssf_navgrid_carve (ssf_navcarve.h)
    NavPlanWs navplan;                            // ssf_navplan_field (ssf_navplan.h)
    NavFrontierWs navfrontier;                    // ssf_navfrontier_regions (ssf_navfrontier.h)
    NavPathWs navpath;                            // ssf_navpath_waypoints (ssf_navpath.h)
    NavLiveWs navlive;                            // ssf_navlive_overlay (ssf_navlive.h)
    NavSteerWs navsteer;                          // ssf_navsteer_rollouts (ssf_navsteer.h)
    NavFootWs navfoot;                            // ssf_navfoot_layers, ssf_navfoot_rollouts (ssf_navfoot.h)
    NavPoseWs navpose;                            // ssf_navpose_field (ssf_navpose.h)
    NavDynWs navdyn;                              // ssf_navdyn_blobs (ssf_navdyn.h)
    RaycastWs raycast;                            // ssf_raycast (ssf_raycast.h)
    unsigned long long model_gen = 0;             // bumped by whatever rewrites model rows or their order (a fuse, store_from_dense); the out-of-view
                                                  // compaction keeps rows and order but moves slots: who keeps slot numbers also watches n_recentres (RaycastWs)
    NavMemWs navmem;                              // ssf_navmem_update (ssf_navmem.h); behind the older members, so that none of them moves
    NavFloorWs navfloor;                          // ssf_navfloor_fit (ssf_navfloor.h); last, for the same reason
};

#define HCK(call)                                                                                    \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            h->err = std::string(#call) + ": " + hipGetErrorString(e_);                              \
            return SSF_ERR_DEVICE;                                                                   \
        }                                                                                            \
    } while (0)

// ---- helpers of ssf_host.hip that the render, graph, keyframe and exchange entry points call ----------------------------------
#pragma GCC visibility push(hidden)       // (shared by the library's own files, no part of what it exports)
namespace ssf {
// device temporaries of one call: freed on every exit path
struct DevTemps {
    std::vector<void*> p;
    template <typename T> hipError_t take(T** out, size_t bytes) {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes ? bytes : 1);
        if (e == hipSuccess) { p.push_back(q); *out = (T*)q; }
        return e;
    }
    ~DevTemps() { for (void* q : p) (void)hipFree(q); }
};
// while one lives, the calling thread's launches are timed into h->timer (cfg.profile == 1)
struct TimerScope { ssf_handle* h; explicit TimerScope(ssf_handle* hh); ~TimerScope(); };
void timer_collect(KernelTimer* t);                 // call after a stream sync
// the end of a call that launched under a TimerScope: wait for the handle's stream, then book the brackets it recorded
inline int sync_collect(ssf_handle* h) {
    HCK(hipStreamSynchronize(h->stream)); if (h->cfg.profile == 1) timer_collect(&h->timer); return SSF_OK;
}
ModelView model_view(const ssf_handle* h, bool visible_only);
int model_at_rest(ssf_handle* h, const char* who = nullptr, const char* lacks = nullptr);
int materialise(ssf_handle* h);
// for ssf_motion.hip: what every frame entry point asks of its arguments first (false: SSF_ERR_INVALID_ARG), and
// ssf_process_frame_pixmask with the pixel mask in device memory whatever on_device says of the frame
bool frame_inputs_ok(ssf_handle* h, const void* rgb, const void* depth, int on_device);
int process_frame_devmask(ssf_handle* h, const void* rgb, const void* depth, int on_device, const float* prior, const uint8_t* d_pixmask,
                          ssf_frame_result* out);
int store_from_dense(ssf_handle* h, int n, int n_visible);
void drop_shard_sizes(ssf_handle* h);
// for ssf_exchange.hip: ssf_last_error(NULL)'s text, a buffer the handle owns, the wait for a mailbox word, row views and copies.
// dalloc is defined in ssf_host.hip, which instantiates it for that file (<int>): another element type there needs its own line.
void set_create_error(const char* what);
template <typename T> bool dalloc(ssf_handle* h, T** p, size_t count);
int wait_seq(ssf_handle* h, const volatile unsigned long long* word, unsigned long long want);
SurfelSoA soa_rows(const SurfelSoA& s, size_t r);
int copy_soa(ssf_handle* h, const SurfelSoA& d, const SurfelSoA& s, size_t n);
inline P2PView p2p_view(ssf_handle* h, unsigned long long seq) { P2PView v = h->p2p.view; v.seq = seq; return v; }
inline Rt pose_from12(const float* p) {
    Rt r; r.R = m3(v3(p[0], p[1], p[2]), v3(p[3], p[4], p[5]), v3(p[6], p[7], p[8])); r.t = v3(p[9], p[10], p[11]); return r;
}
inline void pose_to12(const Rt& r, float* p) {
    p[0] = r.R.r0.x; p[1] = r.R.r0.y; p[2] = r.R.r0.z; p[3] = r.R.r1.x; p[4] = r.R.r1.y; p[5] = r.R.r1.z;
    p[6] = r.R.r2.x; p[7] = r.R.r2.y; p[8] = r.R.r2.z; p[9] = r.t.x; p[10] = r.t.y; p[11] = r.t.z;
}
int align_loop(ssf_handle* h, const float* d_pos, const float* d_lab, const float* d_nrm, const float* d_conf, int n, long long* d_out,
               const float* init_pose, float* rel_pose, int* valid, int* iters, int* pairs_last);
int deform_dense(ssf_handle* h, int m, const float* d_np, const float* d_nr, const float* d_nt, float* d_nodes, const float* d_w,
                 const int32_t* d_i);
// ssf_graph.hip's pieces that ssf_graph_solve.hip uses: the refusals of a call on the resident graph, node j's four neighbours,
// the binding of device points, and the stable counting sort (returns which pair, a = 0 / b = 1, holds the sorted list)
int graph_usable(ssf_handle* h, const char* who);
void launch_graph_edges(hipStream_t st, const float4* nodes, int m, int look, int32_t* edges, const char* name);
void launch_graph_bind_points(hipStream_t st, const float* pts, const int32_t* t0, int n, const float4* nodes, int m, int look,
                              float* w4, int32_t* i4, const char* name);
int launch_graph_sort(hipStream_t st, int nslots, int n_elig, int lo, int passes, const int32_t* stamp, const uint8_t* elig,
                      uint32_t* cnt, int32_t* key_a, uint32_t* slot_a, int32_t* key_b, uint32_t* slot_b, const char* name);
// rows [s0, s0 + n) of src -> rows [d0, d0 + n) of dst on the handle's stream (enqueued only); a NULL array of dst is skipped
int copy_rows(ssf_handle* h, const ssf_surfels& dst, size_t d0, const ssf_surfels& src, size_t s0, size_t n, hipMemcpyKind kind);
}  // namespace ssf
#pragma GCC visibility pop
