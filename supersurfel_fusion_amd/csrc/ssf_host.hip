// ssf_host.hip -- host side of the product library: handle, HBM allocation, the per-frame driver
// (the C++ counterpart of SupersurfelFusion::processFrame, core/src/supersurfel_fusion.cu:166-530,
// hot-path parts only): extract contexts (pipelined / batched extract on their own streams and graphs),
// the track chain (ICP loop with the host Gauss-Newton step of core/src/dense_registration.cu:324-421,
// association, fusion, model-store upkeep) with its exchanges in the multi-GPU mode, the loop-closure
// registration, and the core of the C ABI of include/ssf.h: the handle's life cycle, the frame entry points, the stage seams, the
// getters.  The handle and the helpers shared with the library's other host files are declared in ssf_handle.hpp: the entry points of
// ssf_render.h, ssf_graph*.h and ssf_keyframes.h sit next to their kernels, attaching an exchange and re-homing a sharded map are in
// ssf_exchange.hip, the host solvers in ssf_solvers.hpp, the hooks of ssf_testing.h in ssf_testing.hip.
//
// There is NO CPU fallback here: without a gfx950 device ssf_create fails with SSF_ERR_NO_DEVICE.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <type_traits>
#include <unistd.h>
#include "ssf_exchange.hpp"          // (RcclApi, NCK; with it ssf_handle.hpp: the handle, ssf_device.hpp, include/ssf*.h and the containers it holds)
#include "ssf_solvers.hpp"

using namespace ssf;

// ---- kernel timer (cfg.profile) -------------------------------------------------------------------
namespace ssf {
static thread_local KernelTimer* g_timer = nullptr;
KernelTimer* current_timer() { return g_timer; }
void set_current_timer(KernelTimer* t) { g_timer = t; }
void timer_begin(KernelTimer* t, const char* name, hipStream_t st) {
    KernelTimer::Rec r;
    if (!t->pool_free.empty()) { r = t->pool_free.back(); t->pool_free.pop_back(); }
    else { (void)hipEventCreate(&r.e0); (void)hipEventCreate(&r.e1); }
    r.name = name;
    (void)hipEventRecord(r.e0, st);
    t->open.push_back(r);
}
void timer_end(KernelTimer* t, hipStream_t st) {
    KernelTimer::Rec r = t->open.back(); t->open.pop_back();
    (void)hipEventRecord(r.e1, st);
    t->pending.push_back(r);
}
static void timer_calibrate(KernelTimer* t, hipStream_t st) {
    if (t->bracket_bias_ms >= 0.0) return;
    hipEvent_t e[2 * 16];
    for (auto& x : e) (void)hipEventCreate(&x);
    for (int i = 0; i < 16; i++) { (void)hipEventRecord(e[2 * i], st); (void)hipEventRecord(e[2 * i + 1], st); }
    (void)hipStreamSynchronize(st);
    double sum = 0; int n = 0;
    for (int i = 4; i < 16; i++) { float ms; if (hipEventElapsedTime(&ms, e[2 * i], e[2 * i + 1]) == hipSuccess) { sum += ms; n++; } }
    for (auto& x : e) (void)hipEventDestroy(x);
    t->bracket_bias_ms = n ? 0.7 * sum / n : 0.0;
}
void timer_collect(KernelTimer* t) {     // call after a stream sync
    const double bias = t->bracket_bias_ms > 0.0 ? t->bracket_bias_ms : 0.0;
    for (auto& r : t->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) { auto& a = t->acc[r.name]; a.first += std::max(0.0, (double)ms - bias); a.second += 1; }
        t->pool_free.push_back(r);
    }
    t->pending.clear();
}
TimerScope::TimerScope(ssf_handle* hh) : h(hh) {
    if (hh->cfg.profile == 1) timer_calibrate(&hh->timer, hh->stream);       // first use only
    set_current_timer(hh->cfg.profile == 1 ? &hh->timer : nullptr);
}
TimerScope::~TimerScope() { set_current_timer(nullptr); }
}  // namespace ssf

static inline double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// ---- upload of host frames ahead of the pipeline (ssf_process_sequence with host buffers) --------------------------
// The caller of the reference hands over host images (cv::Mat).  Copying them inside the submit call costs the thread
// that also drives the track chain 30-70 us per frame (two hipMemcpyAsync, for pageable memory incl. the staging
// copy).  In ssf_process_sequence the frames are known ahead, so a worker thread copies them into a ring of device
// buffers on a stream of its own; the submitting thread only makes the extract stream wait for the copy's event.
// A sequence starts with small batches (3/8, then 5/8 of extract_batch, then full ones): the first frame can
// only be tracked when the whole first batch has been extracted, and a full batch of 8 takes twice as long as one of 2.
// (Round 3, at the faster relabelling pass, two sweeps of three runs each over the driver's 20 frames: 3,5 7253-7378 frames/s |
// 2,4 7168-7315 | 2,5 7243-7350 | 2,6 6920-7108 | 1,3 7162-7245 | 1,2,4 6811-6858 | 4 6665-6985: tools/ramp_probe.sh.)
// (SSF_SEQ_RAMP="a,b,..": sizes of the leading batches for experiments, each clamped to [1, batch].  Measured over the
// driver's 20 timed frames, batch 8, three runs each: 2,4 (the default) 5900-5990 frames/s | 2,2 5880-5980 | 2 5760-5820 |
// 3 5680-5810 | 2,8 5700-5810 | 1 5600-5780 | 4 5530-5560)
struct SeqRamp { int n = -1; int size[8]; };
static const SeqRamp& seq_ramp() {
    static const SeqRamp ramp = [] {              // (initialised once, also when several handles are driven by several threads)
        SeqRamp r;
        r.n = 0;
        const char* e = SSF_ENV_STR("SEQ_RAMP");
        if (e) { for (const char* q = e; *q && r.n < 8;) { r.size[r.n++] = atoi(q); while (*q && *q != ',') q++; if (*q == ',') q++; } }
        else { r.n = 2; r.size[0] = -3; r.size[1] = -5; }          // (negative: |value| eighths of the batch, rounded)
        return r;
    }();
    return ramp;
}
static inline int seq_batch_size(int b, int batch) {
    const SeqRamp& r = seq_ramp();
    if (b >= r.n) return batch;
    const int v = r.size[b] < 0 ? (-r.size[b] * batch + 4) / 8 : r.size[b];
    return std::min(batch, std::max(1, v));
}
static inline int seq_batch_of(int i, int batch) {
    int b = 0;
    for (;; b++) {
        const int sz = seq_batch_size(b, batch);
        if (b >= seq_ramp().n) return b + i / batch;
        if (i < sz) return b;
        i -= sz;
    }
}
// (a longer ramp -- 2, 4, 4, 6 before the batches of 8 -- was measured in round 2: 6100-6150 against 5960-6260 frames/s over
// 20 timed frames, i.e. nothing)
#ifndef SSF_UPLOAD_RING_BYTES
#define SSF_UPLOAD_RING_BYTES (256ull << 20)          // cap of the upload ring's device buffers (and, again, of its page-locked staging)
#endif
struct Uploader {
    // several workers, frames dealt to them in turn: a pageable hipMemcpyAsync is a host memcpy into a staging buffer, and one
    // thread sustains 6-10 GB/s of it (box to box) = 3000-5000 frames/s at 2.1 MB per frame, less than the pipeline consumes.
    // Two workers were the bottleneck on the slower hosts of the pool (6200 frames/s with host frames against 11 460 with frames in
    // HBM, page-locked caller memory no better: tools/host_buffer_probe.py, round 4) and are not on the faster ones (9900 with 2,
    // 3, 4 workers, 10 600 with 6: tools/upload_ab.sh); four.
#ifndef SSF_UPLOAD_THREADS
#define SSF_UPLOAD_THREADS 4
#endif
    static const int NTH = SSF_UPLOAD_THREADS;
    std::thread th[NTH];
    std::atomic<int> done[NTH];                // worker t: frames < done[t] of its residue class are enqueued
    std::atomic<int> processed{0};            // frames the caller has finished with (their ring slots may be reused)
    std::atomic<int> failed{0}, stop{0};
    int n = 0, ring = 0, device = 0;
    const void* const* rgb = nullptr; const void* const* depth = nullptr;
    size_t rgb_bytes = 0, depth_bytes = 0;
    // frame i is copied on the stream of the extract context that will take it (contexts take batches in turn): the
    // copy precedes that batch's launch in stream order, and no further hardware queue becomes active (a 5th one
    // halves the throughput of the others)
    std::vector<hipStream_t> ctx_stream; int ctx0 = 0, batch = 1;
    std::vector<uint8_t*> d_rgb; std::vector<float*> d_depth;
    // page-locked staging slots (one per ring slot): the worker copies the caller's pageable frame here itself and hands
    // the runtime a truly asynchronous DMA; left to the runtime, pageable copies of several threads serialise inside it
    std::vector<uint8_t*> p_rgb; std::vector<float*> p_depth;
    // pixel masks of ssf_process_sequence_pixmask (ssf_dynamic.h): masks[i] == NULL or masks == NULL, no copy; P bytes per ring slot
    const uint8_t* const* masks = nullptr; size_t mask_bytes = 0;
    std::vector<uint8_t*> d_mask, p_mask;
    bool ready(int i) const { return done[i % NTH].load(std::memory_order_acquire) > i; }
    // where the workers' time went, microseconds summed over the workers since the handle was created (ssf_upload_stats):
    // waiting for a free ring slot | the staging memcpy | the two hipMemcpyAsync calls; frames
    std::atomic<long long> us_ring{0}, us_memcpy{0}, us_enqueue{0}, frames_done{0};
    void run(int t) {
        if (hipSetDevice(device) != hipSuccess) { failed.store(1); return; }
        for (int i = t; i < n && !stop.load(std::memory_order_relaxed); i += NTH) {
            const double t0 = now_us();
            while (i >= processed.load(std::memory_order_acquire) + ring) {
                if (stop.load(std::memory_order_relaxed)) return;
                std::this_thread::sleep_for(std::chrono::microseconds(20));       // (the ring is two batches ahead of the submitting thread)
            }
            const double t1 = now_us();
            const int sl = i % ring;
            hipStream_t st = ctx_stream[(size_t)(ctx0 + seq_batch_of(i, batch)) % ctx_stream.size()];
            const void* src_rgb = rgb[i]; const void* src_depth = depth[i];
            const uint8_t* src_mask = masks ? masks[i] : nullptr;
            if (!p_rgb.empty()) {           // (slot sl was last used by frame i - ring, which has been processed: its DMA is done)
                std::memcpy(p_rgb[sl], rgb[i], rgb_bytes); std::memcpy(p_depth[sl], depth[i], depth_bytes);
                src_rgb = p_rgb[sl]; src_depth = p_depth[sl];
                if (src_mask) { std::memcpy(p_mask[sl], src_mask, mask_bytes); src_mask = p_mask[sl]; }
            }
            const double t2 = now_us();
            if (hipMemcpyAsync(d_rgb[sl], src_rgb, rgb_bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
                hipMemcpyAsync(d_depth[sl], src_depth, depth_bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
                (src_mask && hipMemcpyAsync(d_mask[sl], src_mask, mask_bytes, hipMemcpyHostToDevice, st) != hipSuccess)) { failed.store(1); return; }
            done[t].store(i + 1, std::memory_order_release);
            const double t3 = now_us();
            us_ring += (long long)(t1 - t0); us_memcpy += (long long)(t2 - t1); us_enqueue += (long long)(t3 - t2); frames_done++;
        }
    }
    // The workers live as long as the handle: a thread's first HIP call initialises the runtime's per-thread state (several
    // milliseconds), which a sequence of 240 host frames used to pay anew on every call -- 200 us per frame instead of 125.
    // start() posts the sequence described by the fields above as job `gen`; join() waits until every worker has finished it.
    std::mutex mu; std::condition_variable cv;
    unsigned long long gen = 0; int finished = NTH; bool quit = false, spawned = false;
    void worker(int t) {
        unsigned long long seen = 0;
        for (;;) {
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return quit || gen != seen; }); if (quit) return; seen = gen; }
            run(t);
            { std::lock_guard<std::mutex> lk(mu); finished++; }
            cv.notify_all();
        }
    }
    void start() {
        { std::lock_guard<std::mutex> lk(mu); for (int t = 0; t < NTH; t++) done[t].store(0); finished = 0; gen++; }
        if (!spawned) { spawned = true; for (int t = 0; t < NTH; t++) th[t] = std::thread([this, t] { worker(t); }); }
        cv.notify_all();
    }
    void join() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return finished >= NTH; }); }
    void shutdown() {
        { std::lock_guard<std::mutex> lk(mu); quit = true; }
        cv.notify_all();
        for (int t = 0; t < NTH; t++) if (th[t].joinable()) th[t].join();
    }
};

// ---- streams outlive handles ---------------------------------------------------------------------------
// The runtime maps streams onto hardware queues when they are created, and how it does that depends on the process' history: the
// SECOND handle of a process (first one destroyed, its streams with it) ran the very same sequence at 6400 instead of 11 300 frames/s --
// device-resident frames, nothing else changed (tools/host_buffer_probe.py with PROBE_KINDS=device,device; round 4: what had looked
// like "slow hosts" in the node-call figures of bench.py was this: those figures are taken on later handles of the process).  A handle
// therefore returns its streams to a pool when it is destroyed, and the next handle with the same device and priorities takes them:
// every handle of a process runs on the queues the first one got.  (Handles that live side by side get streams of their own.)
struct StreamPool {
    std::mutex mu;
    std::map<std::pair<int, int>, std::vector<hipStream_t>> idle;         // (device, priority) -> streams
    static const int CAPTURE = 1 << 20;                                    // "priority" of the capture-only streams
    // (dev: the handle's device, cfg.device_id -- not the calling thread's current one: a handle may be destroyed from a thread whose
    // current device is another GPU of the node)
    // A stream is created ON the handle's device (the calling thread's current device is put back afterwards: the capture stream is
    // taken lazily, from whatever thread first runs a segmentation).  The idle list of a key is bounded: a process that has run many
    // handles SIDE BY SIDE and destroyed them keeps at most MAX_IDLE streams per (device, priority) -- what a later handle can take --
    // and destroys the surplus instead of holding every hardware queue for good.
    static const size_t MAX_IDLE = 8;
    hipStream_t take(int dev, int prio) {
        {
            std::lock_guard<std::mutex> lk(mu);
            auto& v = idle[std::make_pair(dev, prio)];
            if (!v.empty()) { hipStream_t st = v.back(); v.pop_back(); return st; }
        }
        int cur = -1;
        const bool switched = hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess;
        hipStream_t st = nullptr;
        const hipError_t e = prio == CAPTURE ? hipStreamCreateWithFlags(&st, hipStreamNonBlocking) : hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio);
        if (switched) (void)hipSetDevice(cur);
        return e == hipSuccess ? st : nullptr;
    }
    void give(hipStream_t st, int dev, int prio) {
        if (!st) return;
        {
            std::lock_guard<std::mutex> lk(mu);
            auto& v = idle[std::make_pair(dev, prio)];
            if (v.size() < MAX_IDLE) { v.push_back(st); return; }
        }
        (void)hipStreamDestroy(st);                 // (the caller has synchronised it)
    }
};
static StreamPool& stream_pool() { static StreamPool* p = new StreamPool(); return *p; }      // (never destroyed: the runtime may be gone by then)

static std::string g_create_err;
namespace ssf {
void set_create_error(const char* what) { g_create_err = what; }

// Wait until the device has published sequence number `want` into the host-mapped mailbox word.
// Bounded: falls back to a stream synchronise (and reports a device error) after ~5 s.
int wait_seq(ssf_handle* h, const volatile unsigned long long* word, unsigned long long want) {
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long long spins = 0;
    while (__atomic_load_n(word, __ATOMIC_ACQUIRE) != want) {
        if ((++spins & 0xFFFF) == 0) {
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 5.0) {
                hipError_t e = hipStreamSynchronize(h->stream);
                if (e != hipSuccess) { h->err = std::string("device error while waiting: ") + hipGetErrorString(e); return SSF_ERR_DEVICE; }
                if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == want) return SSF_OK;
                h->err = "mailbox sequence number never arrived"; return SSF_ERR_DEVICE;
            }
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    return SSF_OK;
}

template <typename T>
bool dalloc(ssf_handle* h, T** p, size_t count) {
    void* q = nullptr;
    // (SSF_ALLOC_GUARD=bytes: that much unused memory on both sides of every buffer -- a probe for out-of-bounds accesses
    // between the small buffers of handles that live side by side, tools/p2p_first_frame_stress.py)
    static const size_t guard = (size_t)SSF_ENV_INT("ALLOC_GUARD", 0) & ~(size_t)255;          // (lab: poisoned guard zones around every buffer)
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    if (hipMalloc(&q, bytes + 2 * guard) != hipSuccess) return false;
    h->allocs.push_back(q);
    if (guard) {                                   // poisoned guard zones, checked by ssf_destroy
        static const int poison_all = SSF_ENV_INT("GUARD_BYTE", 0xA5) & 255;
        static const int only = SSF_ENV_INT("GUARD_ONLY", -1);      // poison this allocation's zones, zero the others'
        const int poison = (only < 0 || (int)h->guarded.size() == only) ? poison_all : 0;
        (void)hipMemset(q, poison, guard);
        (void)hipMemset((char*)q + guard + bytes, poison, guard);
        h->guarded.push_back({q, bytes, guard});
    }
    *p = (T*)((char*)q + guard);
    return true;
}
template bool dalloc<int>(ssf_handle*, int**, size_t);          // (ssf_exchange.hip's one allocation: the shard sizes of all ranks)
}  // namespace ssf
static void check_guards(ssf_handle* h) {
    int idx = 0;
    for (auto& g : h->guarded) {
        std::vector<unsigned char> host(g.guard);
        for (int side = 0; side < 2; side++) {
            const char* zone = (const char*)g.base + (side ? g.guard + g.bytes : 0);
            if (hipMemcpy(host.data(), zone, g.guard, hipMemcpyDeviceToHost) != hipSuccess) continue;
            size_t first = g.guard, last = 0, n = 0;
            static const int poison = SSF_ENV_INT("GUARD_BYTE", 0xA5) & 255;
            for (size_t i = 0; i < g.guard; i++) if (host[i] != (unsigned char)poison) { if (first == g.guard) first = i; last = i; n++; }
            if (n) std::fprintf(stderr, "[ssf guard] allocation #%d (%zu bytes): %zu bytes modified %s it, offsets %zu..%zu relative to the %s (rank %d)\n",
                                idx, g.bytes, n, side ? "BEHIND" : "IN FRONT OF", side ? first : g.guard - 1 - last, side ? last : g.guard - 1 - first,
                                side ? "end" : "start", h->cfg.rank);
        }
        idx++;
    }
}
// the ten streams of a supersurfel row set, stated once: f(the stream's member, its 4-byte words per row)
template <typename F> static void each_stream(F&& f) {
    f(&SurfelSoA::pos, 3); f(&SurfelSoA::col, 3); f(&SurfelSoA::lab, 3); f(&SurfelSoA::stamps, 2); f(&SurfelSoA::r0, 3);
    f(&SurfelSoA::r1, 3); f(&SurfelSoA::r2, 3); f(&SurfelSoA::shape, 6); f(&SurfelSoA::dims, 2); f(&SurfelSoA::conf, 1);
}
static bool alloc_surfels(ssf_handle* h, SurfelSoA& s, size_t n) {
    bool ok = true;
    each_stream([&](auto m, size_t w) { ok = ok && dalloc(h, &(s.*m), w * n); });
    return ok;
}
static void zero_surfels(ssf_handle* h, SurfelSoA& s, size_t n) {
    each_stream([&](auto m, size_t w) { (void)hipMemsetAsync(s.*m, 0, 4 * w * n, h->stream); });
}

// ---- stages -----------------------------------------------------------------------------------------
// the segmentation chain between ingest and finalize: fixed topology and arguments per context.
// Pass k reads label/sums buffer k&1 and writes the other; no merge launch between passes (the pass
// kernel rebuilds the rows it needs from the quiescent sums buffer).  The global superpixel table is
// only materialised where a later stage wants it: before the plane filter.
static void enqueue_segmentation(ssf_handle* h, ExtractCtx& c, hipStream_t st, bool pixmask) {
    const SegParams& p = h->seg;
    const int nb = c.count;
    const int limit = h->max_passes > 0 ? h->max_passes : (1 << 30);
    const int ox[4] = {0, 1, 0, 1}, oy[4] = {0, 1, 1, 0};                 // pass order, TPS_RGBD.cu:190-268
    const int k1 = std::min(4 * (h->cfg.seg_iter / 2), limit), k2 = std::min(4 * h->cfg.seg_iter, std::max(limit, k1));
    for (int k = 0; k < k1; k++) launch_update_pass(st, p, c.maps, nb, k, ox[k & 3], oy[k & 3], false, 0);
    // sums[k1&1] holds the exact sums after k1 passes; RANSAC and the inlier initialisation read them directly
    if (h->cfg.seg_use_ransac) {
        launch_init_samples(st, p, c.maps, nb, k1 & 1);
        launch_eval_samples(st, p, c.maps, nb);
        launch_init_disp(st, p, c.maps, nb, true);
    } else launch_init_disp(st, p, c.maps, nb, false);
    int k = k1;
    for (; k < k2; k++) launch_update_pass(st, p, c.maps, nb, k, ox[k & 3], oy[k & 3], true, 0);
    launch_plane_filter(st, p, c.maps, nb, k & 1);             // final merge (table + planes) + smoothing sweeps
    if (pixmask) launch_render_moments_pixmask(st, p, h->cam, c.maps, nb, c.d_pixmask, c.d_pixcnt);
    else launch_render_moments(st, p, h->cam, c.maps, nb);
}
// ~45 short dependent kernels: replayed as one captured hipGraph (launch-bound inner loop), one graph per
// batch size; eager when kernels are individually timed or the pass count is being bisected
static int run_segmentation(ssf_handle* h, ExtractCtx& c) {
    const bool use_graph = h->cfg.profile != 1 && h->max_passes == 0 && !h->graph_failed;
    const bool pm = c.pixmask_bits != 0;
    if (use_graph) {
        hipGraphExec_t& ex = pm ? c.exec_pm[c.count] : c.exec[c.count];
        hipGraph_t& graph = pm ? c.graph_pm[c.count] : c.graph[c.count];
        if (!ex) {
            // captured on a stream of its own, not on the context's: the upload thread (Uploader) may be enqueueing
            // copies on the context's stream at this very moment
            // (one capture at a time in the process: with several handles driven by several threads -- shards of one map, or
            // several cameras on one GPU -- captures that ran side by side left, once in ~100 first frames, a graph whose
            // first replay differed from the eager chain: tools/p2p_probe.py, round 2)
            static std::mutex capture_mutex;
            static const bool unlocked = SSF_ENV_SET("CAPTURE_UNLOCKED");          // (control runs of that probe)
            std::unique_lock<std::mutex> capture_lock(capture_mutex, std::defer_lock);
            if (!unlocked) capture_lock.lock();
            bool ok = (h->capture_stream || (h->capture_stream = stream_pool().take(h->cfg.device_id, StreamPool::CAPTURE)) != nullptr) &&
                      hipStreamBeginCapture(h->capture_stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
            if (ok) {
                enqueue_segmentation(h, c, h->capture_stream, pm);
                ok = hipStreamEndCapture(h->capture_stream, &graph) == hipSuccess && graph != nullptr;
            }
            if (ok) ok = hipGraphInstantiate(&ex, graph, nullptr, nullptr, 0) == hipSuccess;
            if (!ok) { h->graph_failed = true; ex = nullptr; (void)hipGetLastError(); }
            if (ex) { HCK(hipGraphLaunch(ex, c.stream)); return SSF_OK; }       // (the first replay still under the lock)
        }
        if (ex) { HCK(hipGraphLaunch(ex, c.stream)); return SSF_OK; }
    }
    enqueue_segmentation(h, c, c.stream, pm);
    return SSF_OK;
}

// Launch the extract stage of the open batch of context c (asynchronous; nothing is waited for).
static int launch_batch(ssf_handle* h, ExtractCtx& c) {
    const double t_launch0 = now_us();
    hipStream_t st = c.stream;
    const bool multi = h->ctx.size() > 1;
    const int nb = c.count;
    // the track/fuse chain must be done with the frames this context held before they are overwritten
    if (multi && c.consumed_valid) HCK(hipStreamWaitEvent(st, c.ev_consumed, 0));
    c.timed = h->cfg.profile != 0;
    if (c.timed) HCK(hipEventRecord(c.ev_t0, st));
    // The extract stage DEALT over the ranks of a sharded map (ssf_comm_deal_extract): batch j of the frame
    // stream is extracted by rank j % nranks alone, which broadcasts every frame's label map, plane depth and supersurfels (2.5 MB
    // at 640 x 480) on THIS context's communicator and stream; the other ranks receive them into the same slots and rebuild their
    // private tables (k_import_frame).  Every rank launches the same batches in the same order (same frames, same configuration),
    // so the collectives of a context's communicator are issued in the same order everywhere.
    const bool dealt = h->deal != 0 && h->comm != nullptr;
    const bool mine = !dealt || c.mine;
    int extract_rc = SSF_OK;
    if (mine) {
        c.in.color_format = h->in_color; c.in.depth_format = h->in_depth; c.in.depth_scale = h->in_scale;
        if (h->cfg.depth_prefilter) {                                      // supersurfel_fusion.cu:180 -- the batch's frames in one launch
            launch_bilateral_batch(st, c.in, c.d_depth_filt, c.maps.slab, nb, h->cfg.width, h->cfg.height, h->cfg.prefilter_sigma_color, h->cfg.prefilter_sigma_space);
            for (int b = 0; b < nb; b++) c.in.depth[b] = slab_shift(c.d_depth_filt, (size_t)b * c.maps.slab);
            c.in.depth_format = SSF_DEPTH_F32_METRES;                      // (ingest reads the filter's float output, the raw colour)
        }
        launch_ingest(st, h->seg, c.in, c.maps, nb, c.epoch0);
        for (int b = 0; b < nb; b++)                                       // (the pixel counts of the frames that vote)
            if ((c.pixmask_bits >> b) & 1u) HCK(hipMemsetAsync(slab_shift(c.d_pixcnt, (size_t)b * c.maps.slab), 0, 2 * sizeof(uint32_t) * h->S, st));
        extract_rc = run_segmentation(h, c);
        if (extract_rc && !dealt) return extract_rc;
        if (!extract_rc && c.pixmask_bits)
            launch_finalize_surfels_pixmask(st, h->seg, c.maps, nb, c.frame, h->cfg.range_min, h->cfg.range_max, c.stamp0, c.d_mask, c.mask_bits,
                                            c.d_best, c.d_matched, c.d_pixcnt, c.pixmask_bits);
        else if (!extract_rc) launch_finalize_surfels(st, h->seg, c.maps, nb, c.frame, h->cfg.range_min, h->cfg.range_max, c.stamp0, c.d_mask, c.mask_bits,
                                                      c.d_best, c.d_matched);
    }
    if (dealt) {
        // (a local failure above must not leave the other ranks waiting in their broadcasts: the group is issued regardless -- what it
        //  ships is then meaningless, and this rank reports the error -- and GroupStart is always paired with GroupEnd)
        RcclApi* api = rccl_api();
        const int root = (int)(c.deal_batch % (long long)h->cfg.nranks);
        const size_t P = (size_t)h->cfg.width * h->cfg.height;
        if (mine && !extract_rc) launch_export_rows(st, h->seg, c.maps, nb, c.frame, c.d_wire);
        NCK(api->GroupStart());
        ncclResult_t bc_rc = ncclSuccess;
        for (int b = 0; b < nb && bc_rc == ncclSuccess; b++) {
            const size_t off = (size_t)b * c.maps.slab;
            int32_t* lab = slab_shift(c.maps.label, off); float* pd = slab_shift(c.maps.plane_depth, off); float* w = slab_shift(c.d_wire, off);
            bc_rc = api->Broadcast(lab, lab, P, ncclInt32, root, c.deal_comm, st);
            if (bc_rc == ncclSuccess) bc_rc = api->Broadcast(pd, pd, P, ncclFloat32, root, c.deal_comm, st);
            if (bc_rc == ncclSuccess) bc_rc = api->Broadcast(w, w, 26 * (size_t)h->S, ncclFloat32, root, c.deal_comm, st);
        }
        const ncclResult_t end_rc = api->GroupEnd();
        if (extract_rc) return extract_rc;
        NCK(bc_rc); NCK(end_rc);
        if (!mine || h->deal == 2) launch_import_frame(st, h->seg, c.maps, nb, c.frame, c.d_wire, c.d_best, c.d_matched);
    }
    HCK(hipGetLastError());
    if (c.timed) HCK(hipEventRecord(c.ev_t1, st));
    if (multi) HCK(hipEventRecord(c.ev_done, st));
    c.launched = true; c.waited = false; c.inflight = nb; c.nb_launched = nb;
    h->open_ctx = (int)((&c - h->ctx.data() + 1) % (ptrdiff_t)h->ctx.size());
    if (h->seq_n > 0) {
        if (h->seq_launches < 32) { h->seq_launch_us[h->seq_launches] = t_launch0 - h->seq_t0_us; h->seq_launch_host_us[h->seq_launches] = now_us() - t_launch0; h->seq_launch_n[h->seq_launches++] = nb; }
        h->seq_batches++;
    }
    return SSF_OK;
}
// bytes per pixel of the handle's input format (ssf_input.h), and whether device frames are aligned for it
static size_t color_bpp(const ssf_handle* h) { return (h->in_color == SSF_COLOR_RGBA8 || h->in_color == SSF_COLOR_BGRA8) ? 4 : 3; }
static size_t depth_bpp(const ssf_handle* h) { return h->in_depth == SSF_DEPTH_U16_SCALED ? 2 : 4; }
static bool device_input_aligned(ssf_handle* h, const void* rgb, const void* depth) {
    const size_t ca = color_bpp(h) == 4 ? 4 : 1, da = depth_bpp(h);
    if ((rgb && (uintptr_t)rgb % ca) || (depth && (uintptr_t)depth % da)) {
        h->err = "device frame pointer not aligned for the input format (4-byte colour: 4 bytes; depth: its element size)";
        return false;
    }
    return true;
}
// what every entry point that takes a frame asks of its arguments first (false: SSF_ERR_INVALID_ARG)
static bool frame_args_ok(ssf_handle* h, const void* rgb, const void* depth, int on_device) {
    return h && rgb && depth && (!on_device || device_input_aligned(h, rgb, depth));
}
// Add one frame to the open batch; the batch is launched when it is full (or when its first frame is needed).
// pixmask: the frame's pixel mask (ssf_dynamic.h), P bytes, a device pointer when pixmask_on_device, NULL = none.
static int submit_extract(ssf_handle* h, const void* rgb, const void* depth, int on_device, const uint8_t* mask,
                          const uint8_t* pixmask = nullptr, int pixmask_on_device = 0) {
    ExtractCtx& c = h->ctx[h->open_ctx];
    if (c.launched) { h->err = "extract pipeline is full: process a submitted frame first"; return SSF_ERR_STATE; }
    if (on_device && !device_input_aligned(h, rgb, depth)) return SSF_ERR_INVALID_ARG;
    const int b = c.count;
    if (b == 0) {
        c.stamp0 = h->stamp + h->stamp_bias + (int)h->pending.size(); c.mask_bits = 0; c.pixmask_bits = 0; c.epoch0 = h->extract_ordinal;
        c.from_tables = false;
        if (h->deal && h->comm) { c.deal_batch = h->deal_batches++; c.mine = (int)(c.deal_batch % (long long)h->cfg.nranks) == h->cfg.rank; }
        else c.mine = true;
    }
    h->extract_ordinal++;
    const size_t P = (size_t)h->cfg.width * h->cfg.height, off = (size_t)b * c.maps.slab;
    c.in.rgb[b] = (const uint8_t*)rgb; c.in.depth[b] = depth;
    if (!on_device && c.mine) {            // (a batch another rank extracts: its images are never looked at here)
        uint8_t* drgb = slab_shift(c.d_rgb_in, off); float* ddep = slab_shift(c.d_depth_in, off);
        HCK(hipMemcpyAsync(drgb, rgb, color_bpp(h) * P, hipMemcpyHostToDevice, c.stream));
        HCK(hipMemcpyAsync(ddep, depth, depth_bpp(h) * P, hipMemcpyHostToDevice, c.stream));
        c.in.rgb[b] = drgb; c.in.depth[b] = ddep;
    }
    if (mask && c.mine) { HCK(hipMemcpyAsync(slab_shift(c.d_mask, off), mask, h->S, hipMemcpyHostToDevice, c.stream)); c.mask_bits |= 1u << b; }
    if (pixmask && c.mine) {               // (only the extracting rank votes; the peers import the confidences)
        HCK(hipMemcpyAsync(slab_shift(c.d_pixmask, off), pixmask, P, pixmask_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c.stream));
        c.pixmask_bits |= 1u << b;
    }
    c.count = b + 1;
    h->pending.push_back(std::make_pair(h->open_ctx, b));
    // (inside ssf_process_sequence the first two batches are smaller: seq_batch_size)
    if (c.count == (h->seq_n > 0 ? seq_batch_size(h->seq_batches, h->batch) : h->batch)) return launch_batch(h, c);
    return SSF_OK;
}
// A frame extracted elsewhere takes a batch context of its own: its maps and rows are copied into slot 0 and the private tables
// rebuilt (k_import_frame) on the context's stream, where a local batch would run its extract chain.
static int submit_tables(ssf_handle* h, const int32_t* label, const float* plane_depth, const ssf_surfels* fr, int on_device) {
    if (h->ctx[h->open_ctx].count > 0 && !h->ctx[h->open_ctx].launched) {        // an open local batch: it goes first (frame order)
        int rc = launch_batch(h, h->ctx[h->open_ctx]);
        if (rc) return rc;
    }
    ExtractCtx& c = h->ctx[h->open_ctx];
    if (c.launched) { h->err = "extract pipeline is full: process a submitted frame first"; return SSF_ERR_STATE; }
    hipStream_t st = c.stream;
    const bool multi = h->ctx.size() > 1;
    if (multi && c.consumed_valid) HCK(hipStreamWaitEvent(st, c.ev_consumed, 0));
    c.stamp0 = h->stamp + h->stamp_bias + (int)h->pending.size(); c.mask_bits = 0; c.pixmask_bits = 0; c.epoch0 = h->extract_ordinal;
    h->extract_ordinal++;                          // (the RANSAC epoch advances as if the frame had been extracted here)
    c.from_tables = true;
    const size_t P = (size_t)h->cfg.width * h->cfg.height, S = (size_t)h->S;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    c.timed = false;
    HCK(hipMemcpyAsync(c.maps.label, label, 4 * P, kind, st));
    HCK(hipMemcpyAsync(c.maps.plane_depth, plane_depth, 4 * P, kind, st));
    float* w = c.d_wire;
    HCK(hipMemcpyAsync(w, fr->positions, 12 * S, kind, st)); w += 3 * S;
    HCK(hipMemcpyAsync(w, fr->colors, 12 * S, kind, st)); w += 3 * S;
    HCK(hipMemcpyAsync(w, fr->stamps, 8 * S, kind, st)); w += 2 * S;
    HCK(hipMemcpyAsync(w, fr->orientations, 36 * S, kind, st)); w += 9 * S;
    HCK(hipMemcpyAsync(w, fr->shapes, 24 * S, kind, st)); w += 6 * S;
    HCK(hipMemcpyAsync(w, fr->dims, 8 * S, kind, st)); w += 2 * S;
    HCK(hipMemcpyAsync(w, fr->confidences, 4 * S, kind, st));
    if (!on_device) HCK(hipStreamSynchronize(st));             // (pageable host buffers: the caller may reuse them on return)
    launch_import_frame(st, h->seg, c.maps, 1, c.frame, c.d_wire, c.d_best, c.d_matched);
    HCK(hipGetLastError());
    if (multi) HCK(hipEventRecord(c.ev_done, st));
    c.count = 1; c.launched = true; c.waited = false; c.inflight = 1; c.nb_launched = 1;
    h->pending.push_back(std::make_pair(h->open_ctx, 0));
    h->open_ctx = (int)((&c - h->ctx.data() + 1) % (ptrdiff_t)h->ctx.size());
    return SSF_OK;
}
// the frame held by h->active will not be fused (or has been): its slot is free again
static int retire_active(ssf_handle* h) {
    ExtractCtx* c = h->active.ctx;
    if (!c || !h->have_frame) return SSF_OK;
    h->have_frame = false;
    if (--c->inflight == 0) {
        if (h->ctx.size() > 1) { HCK(hipEventRecord(c->ev_consumed, h->stream)); c->consumed_valid = true; }
        c->launched = false; c->count = 0;
    }
    return SSF_OK;
}
// Make the oldest submitted frame the one the track/fuse chain works on.
static int activate_oldest(ssf_handle* h) {
    if (h->fusing) { h->err = "a frame is between ssf_stage_fuse_begin and ssf_stage_fuse_end"; return SSF_ERR_STATE; }
    if (h->pending.empty()) { h->err = "no submitted frame"; return SSF_ERR_STATE; }
    int rc = retire_active(h);                    // an activated frame that was never fused is dropped
    if (rc) return rc;
    const std::pair<int, int> fr = h->pending.front();
    ExtractCtx& c = h->ctx[fr.first];
    if (!c.launched) { rc = launch_batch(h, c); if (rc) return rc; }
    h->pending.pop_front();
    if (h->ctx.size() > 1 && !c.waited) { HCK(hipStreamWaitEvent(h->stream, c.ev_done, 0)); c.waited = true; }
    if (c.stamp0 + fr.second != h->stamp) { h->err = "submitted frame is out of sequence (model stamp changed while frames were pending)"; return SSF_ERR_STATE; }
    const size_t off = (size_t)fr.second * c.maps.slab;
    ActiveFrame& a = h->active;
    a.maps = batch_slot(c.maps, fr.second); a.frame = batch_slot(c.frame, off);
    a.d_best = slab_shift(c.d_best, off); a.d_matched = slab_shift(c.d_matched, off);
    a.ctx = &c; a.slot = fr.second; a.pixmask = ((c.pixmask_bits >> fr.second) & 1u) != 0;
    a.has_rgba = !c.from_tables && c.mine; a.activated = true;
    h->have_frame = true;
    return SSF_OK;
}
// submit the next frame of the sequence being processed (ssf_process_sequence)
// the last frames of a sequence form a partial batch: nothing more will join it, so it is launched at once instead of
// when the track chain gets to it (its extract would then run with nothing to hide behind: 0.7 ms at the end of a run)
static int seq_flush_tail(ssf_handle* h) {
    if (h->seq_next < h->seq_n) return SSF_OK;
    ExtractCtx& c = h->ctx[h->open_ctx];
    return (c.count > 0 && !c.launched) ? launch_batch(h, c) : SSF_OK;
}
static int seq_submit(ssf_handle* h) {
    const int i = h->seq_next;
    const uint8_t* pixmask = h->seq_pixmask ? h->seq_pixmask[i] : nullptr;
    if (h->seq_on_device || !h->seq_upload) {
        int rc = submit_extract(h, h->seq_rgb[i], h->seq_depth[i], h->seq_on_device, nullptr, pixmask, h->seq_on_device);
        if (!rc) { h->seq_next++; rc = seq_flush_tail(h); }
        return rc;
    }
    Uploader& u = *h->up;
    const auto t0 = std::chrono::steady_clock::now();
    const double w0 = now_us();
    for (unsigned long long spins = 0; !u.ready(i); spins++) {
        if (u.failed.load()) { h->err = "upload of a host frame failed"; return SSF_ERR_DEVICE; }
        if ((spins & 0xFFFF) == 0xFFFF && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 10.0) {
            h->err = "upload of a host frame never finished"; return SSF_ERR_DEVICE;
        }
        std::this_thread::yield();
    }
    h->us_wait_upload += now_us() - w0;
    const int sl = i % u.ring;                    // (its copies are already in the stream of the context it goes to)
    int rc = submit_extract(h, u.d_rgb[sl], u.d_depth[sl], 1, nullptr, pixmask ? u.d_mask[sl] : nullptr, 1);
    if (!rc) { h->seq_next++; rc = seq_flush_tail(h); }
    return rc;
}
static int do_extract(ssf_handle* h, const void* rgb, const void* depth, int on_device, const uint8_t* mask, const uint8_t* pixmask = nullptr) {
    if (!frame_args_ok(h, rgb, depth, on_device)) return SSF_ERR_INVALID_ARG;
    TimerScope ts(h);
    if (!h->pending.empty()) { h->err = "frames are pending in the extract pipeline"; return SSF_ERR_STATE; }
    int rc = retire_active(h);
    if (!rc) rc = submit_extract(h, rgb, depth, on_device, mask, pixmask, on_device);
    return rc ? rc : activate_oldest(h);
}

// a single shard with no exchange of any kind | a shard of a map that runs its exchanges natively (RCCL or peer-to-peer) | an ICP
// iteration is ONE launch (also on peer-to-peer shards: its last workgroup trades the record), as chained launches and the record made ahead need
static inline bool single_shard_alone(const ssf_handle* h) { return h->cfg.nranks == 1 && !h->comm && !h->p2p.on; }
static inline bool exchanges_natively(const ssf_handle* h) { return h->comm || h->p2p.on; }
static inline bool icp_is_one_launch(const ssf_handle* h) { return single_shard_alone(h) || (h->p2p.on && !h->comm); }
// rows of the whole map (the sum over the shards once it is known, ssf_stage_set_shard / comm_counts): the same decision on every rank
static inline long long total_model(const ssf_handle* h) { return (h->cfg.nranks > 1 && h->global_n_model >= 0) ? h->global_n_model : h->n_model; }
static inline long long total_visible(const ssf_handle* h) { return (h->cfg.nranks > 1 && h->global_n_visible >= 0) ? h->global_n_visible : h->n_visible; }
static void icp_start_from(IcpLoop& I, const Rt& pose) {
    I.R_init = m3_transpose(pose.R);
    I.t_init = negate(m3_mulv(I.R_init, pose.t));
    for (int i = 0; i < 16; i++) I.tf_inc[i] = (i % 5 == 0) ? 1.0 : 0.0;
}
static void icp_begin(ssf_handle* h, const float* prior) {
    h->bins.drop();                               // (process_oldest makes this frame's tile-sorted copy after this call)
    if (prior) h->pose = pose_from12(prior);
    IcpLoop& I = h->icp;
    // a record accumulated ahead is this frame's first iteration only if nothing it was computed from has changed
    I.ahead_seq = 0;
    if (h->ahead.valid && !prior && h->have_frame && h->active.ctx == h->ahead.ctx && h->active.slot == h->ahead.slot &&
        h->stamp == h->ahead.stamp && std::memcmp(&h->pose, &h->ahead.pose, sizeof(Rt)) == 0) I.ahead_seq = h->ahead.seq;
    h->ahead.valid = false;
    I.active = total_visible(h) > 0 && h->cfg.icp_iter > 0;
    I.valid = true; I.done = !I.active; I.iter = 0;
    icp_start_from(I, h->pose);
    for (int i = 0; i < 36; i++) I.JtJ[i] = 0.0;
    I.prev_error = DBL_MAX;
    I.t_inc_stale = v3(0, 0, 0);
    h->last_icp_valid = 0; h->last_icp_iters = 0;
}
static void inc_to_float(const double* tf, M3& R, V3& t) {
    R = m3(v3((float)tf[0], (float)tf[1], (float)tf[2]), v3((float)tf[4], (float)tf[5], (float)tf[6]),
           v3((float)tf[8], (float)tf[9], (float)tf[10]));
    t = v3((float)tf[3], (float)tf[7], (float)tf[11]);
}
// model -> camera transform of the coming iteration
static Rt icp_transform(IcpLoop& I) {
    M3 R_inc; V3 t_inc;
    inc_to_float(I.tf_inc, R_inc, t_inc);
    I.t_inc_stale = t_inc;
    Rt T; T.R = m3_mul(R_inc, I.R_init); T.t = add(m3_mulv(R_inc, I.t_init), t_inc);
    return T;
}
// drain the write-combining buffers: the stores above become visible to the device in order, now
static inline void store_fence() {
#if defined(__x86_64__)
    __builtin_ia32_sfence();
#else
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
#endif
}
// the host's word to a waiting launch: its transform and "go", or "no further iteration"
static void icp_release_waiting(IcpGo* slot, unsigned long long go_seq, const Rt* T, unsigned long long p2p_seq = 0, bool match = false) {
    volatile IcpGo* s = slot;
    const unsigned long long want = go_seq & 0xFFFFFFFFull;
    if (T) {
        const float v[12] = {T->R.r0.x, T->R.r0.y, T->R.r0.z, T->R.r1.x, T->R.r1.y, T->R.r1.z, T->R.r2.x, T->R.r2.y, T->R.r2.z,
                             T->t.x, T->t.y, T->t.z};
        uint32_t w[12]; memcpy(w, v, sizeof w);
        uint32_t sum = (uint32_t)p2p_seq * icp_go_word_weight(14) + (uint32_t)(p2p_seq >> 32) * icp_go_word_weight(15);
        for (unsigned int i = 0; i < 12; i++) sum += w[i] * icp_go_word_weight(i);
        // the whole line, then ONE fence: the write-combining buffer goes out as one 64-byte write (were it ever split, the
        // checksum in the flag word keeps the kernel polling until the rest has landed)
        for (int i = 0; i < 12; i++) s->T[i] = v[i];
        s->x = p2p_seq;
        s->flag = want | ((unsigned long long)((sum >> 2) & SSF_ICP_GO_CHECK_MASK) << 32) | (match ? SSF_ICP_GO_MATCH : 0ull);
    } else s->flag = want | ((unsigned long long)icp_go_abort_check((unsigned int)want) << 32) | SSF_ICP_GO_ABORT;
    store_fence();
}

// a launch made ahead that is waiting on the device for the host's word: the slot the word goes to, the number the word
// carries and the sequence number of the record the launch will publish
// (resident: the frame's resident launch, launch_icp_resident -- it stays `waiting` from its launch to the end of the loop, slot / go_seq are
// the line and the number of the NEXT word it will wait for)
struct IcpWaiter { bool waiting = false; IcpGo* slot = nullptr; unsigned long long go_seq = 0, seq_rec = 0; bool resident = false, resident_counted = false; };
// wait for mailbox record `seq` and copy it to h->h_icp_local (h_icp then points at that copy).  waiter: the launch made ahead, if one
// is waiting.  Before the stream is drained it is told to leave (waiter->waiting = false: the next iteration, if any, is launched
// afresh): it would otherwise hold the stream until its own bound expires.
static int icp_fetch(ssf_handle* h, unsigned long long seq, IcpWaiter* waiter = nullptr) {
    // (icp_record_read, ssf_mailbox.hpp: anything but a whole record `seq` is a record still in flight)
    const volatile unsigned long long* rec = h->mb_host->icp_rec;
    auto t0 = std::chrono::steady_clock::now();
    bool drained = false;                     // the stream has been synchronised once after a timeout
    for (unsigned long long spins = 0;; spins++) {
        if (icp_record_read(rec, seq, h->h_icp_local)) break;
        if ((spins & 0xFFFF) == 0xFFFF && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > (drained ? 1.0 : 5.0)) {
            // Nothing for 5 s.  The device may simply be slow or stalled (a cold box, a debugger, another tenant): drain the
            // stream -- however long that takes -- and look again before calling it an error; only a record that is
            // still missing once everything enqueued has run is one.
            if (drained) {
                char where[160];
                std::snprintf(where, sizeof(where), " (rank %d of %d, frame stamp %d, iteration %d, record %llu, peer exchange %llu, %d visible rows)", h->cfg.rank,
                              h->cfg.nranks, h->stamp, h->icp.iter, seq, h->p2p.seq_icp, h->n_visible);
                h->err = std::string("ICP mailbox record never arrived") + where; return SSF_ERR_DEVICE;
            }
            if (waiter) { icp_release_waiting(waiter->slot, waiter->go_seq, nullptr); waiter->waiting = false; waiter = nullptr; }
            hipError_t e = hipStreamSynchronize(h->stream);
            if (e != hipSuccess) { h->err = std::string("device error while waiting for the ICP record: ") + hipGetErrorString(e); return SSF_ERR_DEVICE; }
            drained = true; t0 = std::chrono::steady_clock::now();
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    h->h_icp = h->h_icp_local;
    return SSF_OK;
}
// the rows an ICP / association launch streams: the visible array, or its tile-sorted copy when this frame has one
static inline const SurfelSoA& icp_rows(const ssf_handle* h) { return h->bins.valid ? h->bins.rows : h->model[h->mcur]; }
// THE k_icp launch of the frame path: the current frame's tables, the rows above, the handle's reduction buffers and mailbox
// (sums_out: the record's place on the device, nullptr = h->d_icp; go, go_seq, pv, match: as launch_icp's)
static int icp_issue(ssf_handle* h, const Rt& T, unsigned long long seq, long long* sums_out = nullptr, IcpGo* go = nullptr,
                     unsigned long long go_seq = 0, const P2PView* pv = nullptr, const MatchArgs* match = nullptr) {
    launch_icp(h->stream, h->cam, icp_rows(h), h->n_visible, h->cc->maps.pix2, h->cc->maps.fpack, T, h->d_icp_replicas, h->d_tickets + 8,
               sums_out ? sums_out : h->d_icp, h->mb_dev, seq, -1, go, go_seq, pv, h->bins.valid ? 1 : 0, match);
    HCK(hipGetLastError());
    return SSF_OK;
}
// one iteration's record under the loop's current transform (pv: summed over the peers by the launch itself)
static int icp_accumulate(ssf_handle* h, bool to_host, long long* d_out = nullptr, const P2PView* pv = nullptr) {
    const Rt T = icp_transform(h->icp);
    const unsigned long long seq = ++h->icp_seq;
    const int rc = icp_issue(h, T, seq, d_out, nullptr, 0, pv);
    return (rc || !to_host) ? rc : icp_fetch(h, seq);
}
static void icp_update(ssf_handle* h, const int64_t* sums, int* again) {
    IcpLoop& I = h->icp;
    *again = 0;
    if (!I.active || I.done) return;
    I.iter++; h->last_icp_iters = I.iter;
    static const int tri[6][6] = {{0, 1, 2, 3, 4, 5}, {1, 6, 7, 8, 9, 10}, {2, 7, 11, 12, 13, 14},
                                  {3, 8, 12, 15, 16, 17}, {4, 9, 13, 16, 18, 19}, {5, 10, 14, 17, 19, 20}};
    double Jtr[6];
    for (int i = 0; i < 6; i++) {
        for (int j = 0; j < 6; j++) I.JtJ[i * 6 + j] = (double)sums[tri[i][j]] / SSF_ICP_SCALE_JTJ;
        Jtr[i] = (double)sums[21 + i] / SSF_ICP_SCALE_JTR;
    }
    const float r = (float)((double)sums[27] / SSF_ICP_SCALE_R);
    const float inliers = (float)sums[28];
    const double error = std::sqrt((double)(r / inliers));
    if (inliers < 100.0f) { I.valid = false; I.done = true; return; }
    double X[6], tf_iter[16];
    sym6_ldlt_solve(I.JtJ, Jtr, X);
    gn_increment(X, tf_iter);
    mat4_lmul(tf_iter, I.tf_inc);
    if (!h->cfg.icp_force_iters && error / I.prev_error > 0.9995) { I.done = true; return; }
    I.prev_error = error;
    if (I.iter >= h->cfg.icp_iter) { I.done = true; return; }
    *again = 1;
}
static void icp_end(ssf_handle* h, int* valid) {
    IcpLoop& I = h->icp;
    *valid = 0;
    if (!I.active) return;
    bool ok = I.valid;
    double cov[36];
    mat6_inverse_lu(I.JtJ, cov);
    for (int i = 0; i < 6; i++) if (cov[i * 6 + i] > h->cfg.icp_cov_thresh) { ok = false; break; }
    if (ok) {
        if (len3(I.t_inc_stale) > 0.2f) ok = false;
        else {
            M3 R_inc; V3 t_inc;
            inc_to_float(I.tf_inc, R_inc, t_inc);
            const M3 R_rel = m3_transpose(R_inc);
            const V3 t_rel = negate(m3_mulv(R_rel, t_inc));
            h->pose.t = add(m3_mulv(h->pose.R, t_rel), h->pose.t);
            h->pose.R = m3_mul(h->pose.R, R_rel);
            float R9[9] = {h->pose.R.r0.x, h->pose.R.r0.y, h->pose.R.r0.z, h->pose.R.r1.x, h->pose.R.r1.y, h->pose.R.r1.z,
                           h->pose.R.r2.x, h->pose.R.r2.y, h->pose.R.r2.z};
            renormalise_rotation<float>(R9);
            h->pose.R = m3(v3(R9[0], R9[1], R9[2]), v3(R9[3], R9[4], R9[5]), v3(R9[6], R9[7], R9[8]));
        }
    }
    *valid = ok ? 1 : 0;
    h->last_icp_valid = *valid;
    I.active = false;
}

// ---- model store upkeep -----------------------------------------------------------------------------------
namespace ssf {
SurfelSoA soa_rows(const SurfelSoA& s, size_t r) {       // view starting at row r
    SurfelSoA v = s;
    each_stream([&](auto m, size_t w) { v.*m += w * r; });
    return v;
}
int copy_soa(ssf_handle* h, const SurfelSoA& d, const SurfelSoA& s, size_t n) {      // device -> device, n rows
    if (n == 0) return SSF_OK;
    hipError_t copy_of_a_stream = hipSuccess;                   // (the first failure ends the copies)
    each_stream([&](auto m, size_t w) { if (!copy_of_a_stream) copy_of_a_stream = hipMemcpyAsync(d.*m, s.*m, 4 * w * n, hipMemcpyDeviceToDevice, h->stream); });
    HCK(copy_of_a_stream);
    return SSF_OK;
}
static int oov_home(const ssf_handle* h) { return h->cfg.nb_supersurfels_max + h->S + 256; }   // head after a recentre
// compact the live out-of-view rows into the other store, span starting at oov_home (no dead slots afterwards)
static int oov_recentre(ssf_handle* h) {
    OovStore& src = h->oov[h->ocur]; OovStore& dst = h->oov[h->ocur ^ 1];
    HCK(hipMemsetAsync(dst.live, 0, (size_t)dst.cap, h->stream));
    launch_oov_compact(h->stream, src, dst, h->oov_tail - h->oov_head, oov_home(h), h->d_bc_oov, h->d_cnt, 1);
    HCK(hipGetLastError());
    h->ocur ^= 1;
    h->oov_head = oov_home(h); h->oov_tail = h->oov_head + h->oov_live;
    h->n_recentres++;
    return SSF_OK;
}
// dense [visible | out-of-view] copy of the model in h->dense (stream ordered)
int materialise(ssf_handle* h) {
    int rc = copy_soa(h, h->dense, h->model[h->mcur], (size_t)h->n_visible);
    if (rc) return rc;
    if (h->oov_live > 0) {
        OovStore dst; dst.rows = h->dense; dst.live = h->d_live_scratch; dst.cap = h->cfg.nb_supersurfels_max;
        launch_oov_compact(h->stream, h->oov[h->ocur], dst, h->oov_tail - h->oov_head, h->n_visible, h->d_bc_oov, h->d_cnt, 0);
        HCK(hipGetLastError());
    }
    return SSF_OK;
}
// the stores <- h->dense (n rows, the first n_visible of them visible); also resets the device counters
int store_from_dense(ssf_handle* h, int n, int n_visible) {
    h->ahead.valid = false;                       // the model is replaced: a record accumulated ahead is stale
    h->bins.drop();                               // ... and so is a tile-sorted copy of its visible rows (TileCopy's rule)
    h->model_gen++;
    int rc = copy_soa(h, h->model[h->mcur], h->dense, (size_t)n_visible);
    if (rc) return rc;
    OovStore& o = h->oov[h->ocur];
    const int head = oov_home(h), n_oov = n - n_visible;
    rc = copy_soa(h, soa_rows(o.rows, (size_t)head), soa_rows(h->dense, (size_t)n_visible), (size_t)n_oov);
    if (rc) return rc;
    HCK(hipMemsetAsync(o.live, 0, (size_t)o.cap, h->stream));
    if (n_oov > 0) HCK(hipMemsetAsync(o.live + head, 1, (size_t)n_oov, h->stream));
    Counters c; std::memset(&c, 0, sizeof(c));
    c.n_model = n; c.n_visible = n_visible; c.oov_head = head; c.oov_tail = head + n_oov; c.oov_live = n_oov;
    c.last[0] = n; c.last[1] = n_visible;
    HCK(hipStreamSynchronize(h->stream));
    HCK(hipMemcpy(h->d_cnt, &c, sizeof(c), hipMemcpyHostToDevice));
    h->n_model = n; h->n_visible = n_visible; h->oov_head = c.oov_head; h->oov_tail = c.oov_tail; h->oov_live = n_oov;
    return SSF_OK;
}
// The shard sizes the ranks exchanged at the end of the last frame (read lazily at the start of the next) describe the map
// before a call that replaces it: dropped, the next frame exchanges them afresh.  Called at the TOP of every such entry
// point (ssf_set_model, ssf_apply_deformation, ssf_rehome_begin / _end), before any early return: whether a rank then
// actually rewrites its shard depends on the rank (an empty shard, nothing leaving, nothing arriving), but all ranks make
// the same call sequence, and every rank must enter the next frame in the same state -- a rank that kept the old record
// would skip an exchange its peers perform (their exchange numbers / the RCCL collective order would go out of step).
void drop_shard_sizes(ssf_handle* h) { h->all_valid = false; h->all_pending = false; }
}  // namespace ssf

// exchange != 0 (native multi-rank frame calls with the peer-to-peer backend): the association tables are traded with
// the peers by the match launch's last workgroup -- or, when no rank has anything to match, by a launch of its own
static int do_match(ssf_handle* h, int exchange = 0) {
    const bool any = total_model(h) > 0 && total_visible(h) > 0;               // (global quantities: the same decision on every rank)
    const int n = any ? h->n_visible : 0;
    launch_match(h->stream, h->cam, icp_rows(h), n, h->cc->maps.pix2, h->cc->maps.fpack, h->pose, h->cfg.range_min,
                 h->cfg.range_max, h->id_offset, h->cc->d_best, h->cc->d_matched, h->d_cand, h->S, h->bins.valid ? h->bins.d_idx : nullptr);
    if (exchange && h->p2p.on) launch_p2p_assoc(h->stream, p2p_view(h, ++h->p2p.seq_assoc), h->cc->d_best, h->cc->d_matched, h->mb_dev);
    HCK(hipGetLastError());
    return SSF_OK;
}

// update | insert | classify | reorder, all stream-ordered through the device-side counters; the
// final counters come back through the mailbox (no D2H copy, no stream synchronise).  In two halves: between them a
// sharded map exchanges the rows that crossed a tile edge (migrate: fuse_begin leaves this shard's migrant table in
// h->d_migrants; fuse_end takes the rank-reduced table, or nullptr when nothing can arrive).
static int fuse_begin(ssf_handle* h, int migrate) {
    const long long nmodel_g = total_model(h), nvis_g = total_visible(h);
    SurfelSoA& M = h->model[h->mcur];
    h->bins.drop();                               // (TileCopy's rule: from here on the frame rewrites the rows the copy was made from)
    h->fuse_first = !(nmodel_g > 0);
    h->fuse_migrate = migrate && h->cfg.nranks > 1 && !h->fuse_first;
    h->classify.plane_depth = h->cc->maps.plane_depth; h->shard.migrate = h->fuse_migrate ? 1 : 0;
    if (nmodel_g > 0) {
        // out-of-view store upkeep before the frame's launches: room in front for the rows that leave the view (at
        // most all visible rows), room behind for out-of-view insertions, and not too many dead slots in the span
        {
            const int span = h->oov_tail - h->oov_head;
            if (h->oov_head < h->n_visible + h->S + 256 || h->oov[h->ocur].cap - h->oov_tail < 2 * h->S + 256 ||
                span > h->oov_live + h->oov_live / 4 + 65536) { int rc2 = oov_recentre(h); if (rc2) return rc2; }
        }
        // a single shard: the fuse launch ends without its three-trip tail, the move kernel works the counters out from the class
        // totals (MoveTotals: the counts the frame starts from are mirrored here).  A sharded map keeps the tail: arrivals from
        // other ranks change the counters between the two launches (launch_migrate_in).
        h->fuse_totals.from_tot = (single_shard_alone(h) && !h->fuse_migrate && h->move_totals_on) ? 1 : 0;
        h->fuse_totals.nv = h->n_visible; h->fuse_totals.head_old = h->oov_head; h->fuse_totals.tail_old = h->oov_tail;
        PartitionWs& ws = h->fuse_ws;
        {
            uint32_t* set = h->d_part + (size_t)h->part_set * h->part_words;
            ws.sup_vis = set; ws.sup_oov = set + h->part_sup_vis; ws.tot = ws.sup_oov + h->part_sup_oov;
            ws.ticket = h->d_part_ticket; ws.other = h->d_part + (size_t)(h->part_set ^ 1) * h->part_words; ws.words = h->part_words;
            h->part_set ^= 1;
        }
        // update | insert | classification of every row | publication of the counters: one launch
        const AssocTables at{h->cc->d_best, h->cc->d_matched, h->d_cand, h->S, h->assoc_rstride};
        launch_fuse(h->stream, M, h->cc->frame, h->pose, h->stamp, h->id_offset, h->n_visible, at, nvis_g > 0 ? 1 : 0,
                    h->cfg.nb_supersurfels_max, h->shard, h->d_cnt, h->oov[h->ocur], h->oov_tail - h->oov_head, h->classify,
                    h->d_state, h->d_state_oov, h->d_bc_oov, ws, h->fuse_totals.from_tot);
        if (h->fuse_migrate)
            launch_pack_emigrants(h->stream, M, at, h->id_offset, h->n_visible, h->d_state, nvis_g > 0 ? 1 : 0, h->shard, h->d_migrants);
    }
    HCK(hipGetLastError());
    h->fusing = true;
    h->model_gen++;
    return SSF_OK;
}
// ---- the end of the fuse stage, step by step (fuse_end below) ---------------------------------------------------------------
// The rows the move kernel writes to the new visible array are the rows the next frame's first ICP iteration reads, under a
// transform that is known now (the pose just estimated, when the caller supplies no prior): if that frame's extract has
// finished, the move kernel accumulates the record on the way (k_move_rows<true>).  have_next: it does, with next / next_pv.
static int fuse_next_icp(ssf_handle* h, NextIcp& next, P2PView& next_pv, bool& have_next) {
    have_next = false;
    if (!(h->icp_ahead && (h->p2p.on || h->ahead_tuner.current() == 1) && icp_is_one_launch(h) && h->cfg.icp_iter > 0 && !h->pending.empty()))
        return SSF_OK;
    ExtractCtx& nc = h->ctx[h->pending.front().first];
    const int nslot = h->pending.front().second;
    const bool multi = h->ctx.size() > 1;         // one context: extract ran on the track stream itself
    // Only when that frame's extract HAS finished (round 5).  Frames of the batch being consumed are ready by construction;
    // at a batch boundary the next context's event is asked.  Until round 4 the track stream was made to wait for it here --
    // in a sequence's fill phase that parked the row moves behind a batch that was still 100-200 us from done, and the
    // driver's 20-frame form ran 4 % slower with the fusion than without (7680-7730 against 8030-8060 frames/s, same box,
    // alternated twice: profiles/track_chain_r05.txt); in the steady state the next batch is ready and nothing changes.
    bool ready = nc.launched && (!multi || nc.waited);
    // (peer-to-peer shards: every rank must take the SAME form for a frame -- a rank that fused would spin in the exchange until
    //  its peer's later launch publishes -- so there the decision stays host-deterministic: wait for the event, as until round 4)
    if (nc.launched && !ready && (h->icp_ahead_mode == 2 || h->p2p.on || hipEventQuery(nc.ev_done) == hipSuccess)) {
        HCK(hipStreamWaitEvent(h->stream, nc.ev_done, 0)); nc.waited = true; ready = true;
    }
    (void)hipGetLastError();                      // (hipErrorNotReady of the query is not an error)
    if (!ready) return SSF_OK;
    const FrameMaps nm = batch_slot(nc.maps, nslot);
    IcpLoop first;
    icp_start_from(first, h->pose);
    next = NextIcp{h->cam, nm.pix2, nm.fpack, icp_transform(first), h->d_icp_replicas, h->d_tickets + 8, h->d_icp, h->mb_dev, ++h->icp_seq};
    if (h->p2p.on) next_pv = p2p_view(h, ++h->p2p.seq_icp);
    h->ahead.valid = true; h->ahead.seq = next.seq; h->ahead.ctx = &nc; h->ahead.slot = nslot;
    h->ahead.stamp = h->stamp + 1; h->ahead.pose = h->pose;
    have_next = true;
    return SSF_OK;
}
// The frame's last launches: arrivals from other shards, the row moves (or the first frame's copy), and -- a sharded map -- the
// exchange of the shard sizes; counter record `seq` is published on the way.
static int fuse_launch_moves(ssf_handle* h, const int32_t* d_table, unsigned long long seq) {
    SurfelSoA& M = h->model[h->mcur];
    if (h->fuse_first) {
        launch_first_frame(h->stream, M, h->cc->frame, h->pose, h->S, h->cfg.nb_supersurfels_max, h->shard, h->d_cnt);
        launch_publish_counts(h->stream, h->d_cnt, 0, h->mb_dev, seq);
        if (exchanges_natively(h)) { int rg = comm_gather_counts(h); if (rg) return rg; }
        return SSF_OK;
    }
    const PartitionWs& ws = h->fuse_ws;
    if (h->fuse_migrate && d_table)
        launch_migrate_in(h->stream, M, d_table, h->S, h->cfg.nb_supersurfels_max, h->d_cnt, h->shard, h->classify, h->pose, h->stamp,
                          h->d_state, ws);
    NextIcp next{};
    P2PView next_pv{};
    bool have_next;
    { int rn = fuse_next_icp(h, next, next_pv, have_next); if (rn) return rn; }
    // move: the host continues once the counters arrive (published by the fuse launch), the row moves of this
    // frame overlap the host-side launch work of the next one (stream order keeps every later reader of the
    // model behind them)
    // (a sharded map: the shard sizes of all ranks are exchanged now -- the counters are final -- so that the next
    // frame does not have to wait for the row moves to learn them)
    if (exchanges_natively(h)) { int rg = comm_gather_counts(h); if (rg) return rg; }
    launch_move_rows(h->stream, M, h->model[h->mcur ^ 1], h->oov[h->ocur], h->n_visible + (h->fuse_migrate ? 2 : 1) * h->S, h->oov_tail - h->oov_head,
                     h->d_state, h->d_state_oov, h->d_bc_oov, ws, h->d_cnt, h->mb_dev, seq, have_next ? &next : nullptr,
                     have_next && h->p2p.on ? &next_pv : nullptr, h->fuse_totals.from_tot ? &h->fuse_totals : nullptr);
    h->mcur ^= 1;
    return SSF_OK;
}
// wait for counter record `seq`, read it into c and take the handle's mirrors of the model's sizes from it
static int fuse_read_counters(ssf_handle* h, unsigned long long seq, Counters& c) {
    int rc = wait_seq(h, &h->mb_host->cnt_seq, seq);
    if (rc) return rc;
    for (int attempt = 0; !int_record_read(reinterpret_cast<const int*>(&h->mb_host->cnt), MAILBOX_COUNTER_WORDS, &h->mb_host->cnt_check, seq,
                                           reinterpret_cast<int*>(&c)); attempt++)
        if (attempt > 100000) { h->err = "counter mailbox record failed its checksum"; return SSF_ERR_DEVICE; }
    h->n_model = c.n_model; h->n_visible = c.n_visible;
    h->oov_head = c.oov_head; h->oov_tail = c.oov_tail; h->oov_live = c.oov_live;
    return SSF_OK;
}
// the flag a kernel without a record of its own to withhold leaves in the mailbox: reported once
static int fuse_device_flags(ssf_handle* h) {
    if (h->p2p.on && __atomic_load_n(&h->mb_host->p2p_timeout, __ATOMIC_ACQUIRE) != 0u) {
        __atomic_store_n(&h->mb_host->p2p_timeout, 0u, __ATOMIC_RELEASE);       // reported once; a later frame starts clean
        h->err = "a peer's association / migrant tables never arrived (peer-to-peer exchange)"; return SSF_ERR_DEVICE;
    }
    return SSF_OK;
}
static void fuse_result(ssf_handle* h, const Counters& c, ssf_frame_result* out) {
    std::memset(out, 0, sizeof(*out));
    pose_to12(h->pose, out->pose);
    out->icp_valid = h->last_icp_valid; out->icp_iters = h->last_icp_iters;
    out->n_model = h->n_model; out->n_visible = h->n_visible; out->n_removed = c.n_removed;
    out->n_inserted = c.n_inserted; out->n_updated = c.n_updated; out->stamp = h->stamp;
    ExtractCtx* ec = h->active.ctx;            // extract time of the batch this frame came in, per frame
    float ms;
    if (h->cfg.profile != 0 && ec && ec->timed && hipEventElapsedTime(&ms, ec->ev_t0, ec->ev_t1) == hipSuccess)
        out->stage_ms[0] = ms / (float)ec->nb_launched;
}
static int fuse_end(ssf_handle* h, const int32_t* d_table, ssf_frame_result* out) {
    const unsigned long long seq = ++h->cnt_seq;
    h->fusing = false;                           // (also on every error path below: the frame is over either way)
    int rc = fuse_launch_moves(h, d_table, seq);
    if (rc) return rc;
    HCK(hipGetLastError());
    rc = retire_active(h);                       // last reader of this frame's buffers is enqueued
    if (rc) return rc;
    h->stamp_bias = 1;                           // the frame being fused still holds h->stamp
    while (!rc && h->seq_next < h->seq_n && !h->ctx[h->open_ctx].launched) rc = seq_submit(h);      // see seq_rgb
    h->stamp_bias = 0;
    if (rc) return rc;
    Counters c;
    rc = fuse_read_counters(h, seq, c);
    if (!rc) rc = fuse_device_flags(h);
    if (rc) return rc;
    if (out) fuse_result(h, c, out);
    h->stamp++;
    h->global_n_model = -1; h->global_n_visible = -1;
    if (h->cfg.profile == 1) { HCK(hipStreamSynchronize(h->stream)); timer_collect(&h->timer); }
    return SSF_OK;
}

static int do_fuse(ssf_handle* h, ssf_frame_result* out) {          // no exchange of rows (single shard, or ssf_stage_fuse)
    int rc = fuse_begin(h, 0);
    return rc ? rc : fuse_end(h, nullptr, out);
}

// ---- chained ICP launches --------------------------------------------------------------------------------
// launch the NEXT iteration now, to wait on the device for its transform (icp_waiter_can_match: the launch can be told to do the
// frame's association instead of an iteration -- SSF_ICP_GO_MATCH)
static bool icp_waiter_can_match(const ssf_handle* h) {
    static const bool off = SSF_ENV_SET("NO_MATCH_IN_WAITER");          // (measurement switch)
    return !off && single_shard_alone(h) && h->cfg.profile == 0 && icp_variant_mode() == 0;
}
// Which frames bid into the replicas of the association table (ssf_device.hpp): those whose association runs inside an ICP launch
// over the visible array -- a single shard alone.  The tile-sorted copy (its XCDs already bid for disjoint frame supersurfels),
// k_match as a launch of its own, sharded handles and the stage seams stay on table 0: rstride 0, and the readers read one word.
static int assoc_replica_stride(const ssf_handle* h) {
#ifdef SSF_EXPERIMENTS
    static const bool off = SSF_ENV_INT("ASSOC_REPLICAS", 1) == 0;          // (measurement switch: A/B runs of one build)
    if (off) return 0;
#endif
    return (icp_waiter_can_match(h) && !h->bins.valid) ? assoc_stride(h->S) : 0;
}
static int icp_launch_waiting(ssf_handle* h, IcpWaiter& w) {
    w.seq_rec = ++h->icp_seq;
    w.go_seq = ++h->go_count;
    w.slot = h->go + (w.go_seq % SSF_ICP_GO_SLOTS);
    h->wait_launched_us = now_us();               // (before the launch call: no workgroup of it can have started waiting earlier)
    Rt none; none.R = m3_identity(); none.t = v3(0, 0, 0);
    const P2PView pv = h->p2p.view;               // (the number of the peer exchange arrives with the go word)
    const MatchArgs ma{h->cfg.range_min, h->cfg.range_max, h->id_offset, h->cc->d_best, h->cc->d_matched, h->d_cand, h->assoc_rstride};
    const int rc = icp_issue(h, none, w.seq_rec, nullptr, w.slot, w.go_seq, h->p2p.on ? &pv : nullptr, icp_waiter_can_match(h) ? &ma : nullptr);
    w.waiting = rc == SSF_OK;
    return rc;
}
// ---- the resident launch: one per frame, an iteration is one word -----------------------------------------------------------------
// When a frame takes it: a single shard alone, rows streamed from the visible array (no tile-sorted copy), the product's kernel, and
// few enough visible rows that every workgroup of the launch holds a place at once (resident_max_rows: 256 x icp_resident_max_wgs()
// = 1024 workgroups of the 1792 places the kernel's registers leave on the part, 7 per compute unit -- a safety condition, not a
// tuning knob.  It assumes ONE handle tracking on the GPU: resident grids of several handles or processes add up, and past 1792
// places each waits for workgroups that cannot get one until the bounded waits end the launches in SSF_ERR_DEVICE.  Callers that
// share a GPU among handles with large maps lower the limit, ssf_debug_set_resident_icp_max_rows).
// Not with the depth pre-filter in the frame (cfg.depth_prefilter): that pipeline is bound by its extract stage, not by this
// chain, and the workgroups that stay slow the relabelling launches beside them (k_update_pass 12.8 -> 13.6 us per launch in
// the kernel traces) -- with the pre-filter in the frame the resident launch ran 3.3 % SLOWER, the same build with the limit at 0 as fast
// as before (profiles/icp_resident.txt).  Everything else takes the launches above.
static bool icp_resident_ok(const ssf_handle* h) {
    return h->go_res && single_shard_alone(h) && !h->bins.valid && !h->cfg.depth_prefilter && icp_variant_mode() == 0 && h->n_visible > 0 &&
           h->n_visible <= h->resident_max_rows;
}
// T0: the first iteration's transform, record seq0 (nullptr: the first record came from the row-move kernel, the launch starts at word 1)
static int icp_launch_resident(ssf_handle* h, IcpWaiter& w, const Rt* T0, unsigned long long seq0) {
    const int last = h->cfg.icp_iter;             // words 1 .. last: at most icp_iter - 1 iterations and the word that ends the launch
    IcpGo* lines = h->go_res + (size_t)(h->n_resident_launches++ & 1) * (size_t)(last + 1);
    const unsigned long long go_base = h->go_count;
    h->go_count += (unsigned long long)last;
    w.resident = true; w.slot = lines + 1; w.go_seq = go_base + 1;
    h->wait_launched_us = now_us();               // (before the launch call: no workgroup of it can have started waiting earlier)
    const MatchArgs ma{h->cfg.range_min, h->cfg.range_max, h->id_offset, h->cc->d_best, h->cc->d_matched, h->d_cand, h->assoc_rstride};
    launch_icp_resident(h->stream, h->cam, h->model[h->mcur], h->n_visible, h->cc->maps.pix2, h->cc->maps.fpack, T0, h->d_icp_replicas, h->d_icp, h->mb_dev,
                        seq0, lines, (unsigned int)go_base, last, icp_waiter_can_match(h) ? &ma : nullptr);
    HCK(hipGetLastError());
    w.waiting = true;
    if (!w.resident_counted) { w.resident_counted = true; h->n_resident_frames++; if (!T0) h->n_resident_ahead_frames++; }    // (per frame, not per launch: icp_fetch may have dismissed one)
    return SSF_OK;
}
// the next iteration of the resident launch: ONE store of the word (transform, number, record number), no launch call.  A workgroup
// can start waiting for the word behind this one only once this one is stored: the clock of the host's repair rule (icp_loop_end)
// restarts here.
static void icp_resident_iterate(ssf_handle* h, IcpWaiter& w, const Rt& T, unsigned long long seq_rec) {
    h->wait_launched_us = now_us();
    icp_release_waiting(w.slot, w.go_seq, &T, seq_rec);
    w.slot++; w.go_seq++;
}
// A chained launch that never got its word (host stalled past the kernel's bound, or the record never arrived) may
// have left the arrival counters / replica records of the ICP reduction half filled: drain the stream, put them back
// to rest and stop chaining launches on this handle.
static void icp_chain_reset(ssf_handle* h) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipMemsetAsync(h->d_icp_replicas, 0, 2 * SSF_ICP_REPLICAS * 32 * sizeof(long long), h->stream);
    (void)hipMemsetAsync(h->d_tickets, 0, 512 * sizeof(unsigned int), h->stream);
    (void)hipStreamSynchronize(h->stream);
    h->icp_chain = false; h->ahead.valid = false;
}
// ---- the track stage of one frame, step by step (process_oldest below is the list) -------------------------------------------------
// what the steps share: entry time, end of the ICP loop, the frame's number inside a sequence (debug marks) | the stage split is
// timed (costs an event synchronise: opt-in) | no record has come back yet | the launch made ahead
struct TrackFrame { double t_a = 0.0, t_b = 0.0; int kf = -1; bool timing = false, first_it = true; IcpWaiter w; };
// The tile-sorted copy's buffers, on first use (48 B per row of capacity; d_idx: only the flag "this is the sorted copy" of
// launch_match).  Shared by the frame's copy and the read-out ssf_debug_tile_copy.
static int tile_copy_buffers(ssf_handle* h, TileCopy& b) {
    if (b.d_idx) return SSF_OK;
    const size_t N = (size_t)h->cfg.nb_supersurfels_max, bw = bin_buffer_words(h->cam, N);
    const bool ok = bw && dalloc(h, &b.rows.pos, 12 * N) && dalloc(h, &b.d_idx, 1) && dalloc(h, &b.d_count, bw) && dalloc(h, &b.d_cursor, bw);
    if (!ok) { h->err = "allocation of the tile-sorted copy failed"; return SSF_ERR_DEVICE; }
    return SSF_OK;
}
// The tile-copy step of a frame (after icp_begin, which dropped the last copy).  A large visible set: its ICP / association fields
// once more, sorted by the image tile they project to under the frame's initial transform (ssf_track_fuse.hip, k_bin_*): the
// iterations and the association stream that copy.  The decision: a frame that iterates, on a single shard, min_rows visible rows or more.
int TileCopy::make_if_large(ssf_handle* h) {
    if (!(h->icp.active && min_rows >= 0 && h->n_visible >= min_rows && h->n_visible > 0 && single_shard_alone(h) && bin_buffer_words(h->cam, 1) != 0)) return SSF_OK;
    { const int rc = tile_copy_buffers(h, *this); if (rc) return rc; }
    Rt T0; T0.R = h->icp.R_init; T0.t = h->icp.t_init;
    // In front of the loop, on the track stream.  (Measured and removed, round 6: the sort on a stream of its own beside the
    // frame's first two iterations, the launch made ahead for iteration 3 the first to wait for it -- 2 003-2 026 frames/s at
    // BASELINE config 3 against 2 351-2 366 in front and 2 286-2 301 without the copy: launches made ahead hold their workgroups'
    // places while they wait for the host's word, and the sort's three launches queue behind them.  profiles/config3_sorted_rows_r06.txt)
    launch_bin_rows(h->stream, h->cam, h->model[h->mcur], h->n_visible, T0, d_count, d_cursor, rows);
    HCK(hipGetLastError());
    valid = true; frames++;
    return SSF_OK;
}
// chained launches (single GPU, kernels not individually timed): while iteration i runs, iteration i + 1 is
// already launched and waits on the device for its transform
// (with the peer-to-peer exchange too: there an iteration is one launch as well; every rank takes the same decisions)
static inline bool icp_chains(const ssf_handle* h) { return h->icp_chain && h->go && icp_is_one_launch(h) && h->cfg.profile != 1; }
static int icp_loop_chained(ssf_handle* h, TrackFrame& f) {
    IcpWaiter& w = f.w;
    int again = h->icp.active ? 1 : 0, rc;
    const bool resident = again && icp_resident_ok(h);
    while (again) {
        unsigned long long seq_rec;
        if (h->icp.ahead_seq) { seq_rec = h->icp.ahead_seq; h->icp.ahead_seq = 0; }     // iteration 1 came from the move kernel
        else {
            const Rt T = icp_transform(h->icp);
            const unsigned long long xseq = h->p2p.on ? ++h->p2p.seq_icp : 0;             // (the number of this iteration's peer exchange)
            if (resident) {                            // one launch for the frame: up already -> one store; else it starts with this iteration
                seq_rec = ++h->icp_seq;
                if (w.waiting) icp_resident_iterate(h, w, T, seq_rec);
                else { rc = icp_launch_resident(h, w, &T, seq_rec); if (rc) return rc; }
            } else if (w.waiting) { icp_release_waiting(w.slot, w.go_seq, &T, xseq); seq_rec = w.seq_rec; w.waiting = false; }   // already on the device
            else {
                const P2PView pv = p2p_view(h, xseq);
                seq_rec = ++h->icp_seq;
                rc = icp_issue(h, T, seq_rec, nullptr, nullptr, 0, h->p2p.on ? &pv : nullptr);
                if (rc) return rc;
            }
        }
        // the next iteration, should there be one (the loop may run cfg.icp_iter iterations at most) -- and behind the LAST
        // iteration the loop allows, a launch that can only be told to do the association: a loop that ends at the cap
        // (BASELINE config 3: ten forced iterations) then starts its association ~1 us after the host's last step instead of
        // a launch latency later (11-13 us between the tenth k_icp and k_match in the round-4 traces), like one that converges
        // (the resident launch is up from the first iteration on: behind a first record that came from the move kernel it starts here)
        if (resident) { if (!w.waiting) { rc = icp_launch_resident(h, w, nullptr, 0); if (rc) return rc; } }
        else if (h->icp.iter + 1 < h->cfg.icp_iter || (!f.timing && icp_waiter_can_match(h))) {
            rc = icp_launch_waiting(h, w);
            if (rc) return rc;
        }
        rc = icp_fetch(h, seq_rec, w.waiting ? &w : nullptr);
        if (rc) { if (w.waiting) icp_release_waiting(w.slot, w.go_seq, nullptr); icp_chain_reset(h); return rc; }
        if (f.first_it) { h->host_us[5] += now_us() - f.t_a; f.first_it = false; if (f.kf >= 0 && f.kf < 64) h->seq_mark_us[1][f.kf] = now_us() - h->seq_t0_us; }
        icp_update(h, (const int64_t*)h->h_icp, &again);
    }
    return SSF_OK;
}
// one launch (or launch + collective) per iteration, waited for before the next is made
static int icp_loop_plain(ssf_handle* h, TrackFrame& f) {
    int again = h->icp.active ? 1 : 0, rc;
    while (again) {
        if (h->p2p.on) {
            // one launch: its last workgroup trades the shard record with the peers through the exchange regions and
            // publishes the SUM over the ranks (exact: int64)
            const P2PView pv = p2p_view(h, ++h->p2p.seq_icp);
            rc = icp_accumulate(h, true, nullptr, &pv);
        } else if (h->comm) {
            // shard record -> SUM over the ranks in HBM (exact: int64) -> mailbox -> host solve
            rc = icp_accumulate(h, false);
            if (rc) return rc;
            { ScopedKernel sk("exchange_icp_record", h->stream);
              NCK(rccl_api()->AllReduce(h->d_icp, h->d_icp, SSF_ICP_RECORD, ncclInt64, ncclSum, h->comm, h->stream)); }
            const unsigned long long seq = ++h->icp_seq;
            launch_publish_icp(h->stream, h->d_icp, h->mb_dev, seq);
            HCK(hipGetLastError());
            rc = icp_fetch(h, seq);
        } else if (h->icp.ahead_seq) {
            // first iteration: the record was accumulated by the previous frame's move kernel
            rc = icp_fetch(h, h->icp.ahead_seq);
            h->icp.ahead_seq = 0;
        } else
            rc = icp_accumulate(h, true);
        if (rc) return rc;
        if (f.first_it) { h->host_us[5] += now_us() - f.t_a; f.first_it = false; }
        icp_update(h, (const int64_t*)h->h_icp, &again);
    }
    return SSF_OK;
}
// The end of the loop.  No further iteration: the launch made ahead leaves -- or, told the frame's final pose, does the association
// on its way out (the rows, tables and frame it was launched with are the ones the association reads); otherwise the association is
// a launch of its own.  Then its reduction over the ranks of an RCCL communicator.
static int icp_loop_end(ssf_handle* h, TrackFrame& f) {
    IcpWaiter& w = f.w;
    int valid = 0; bool matched_by_waiter = false;
    if (w.waiting && !f.timing && icp_waiter_can_match(h)) {
        icp_end(h, &valid);
#ifdef SSF_EXPERIMENTS
        if (h->dbg_stall_before_match_us > 0) usleep((useconds_t)h->dbg_stall_before_match_us);      // (test hook of the lab build: a stalled host thread)
#endif
        icp_release_waiting(w.slot, w.go_seq, &h->pose, 0, true);
        matched_by_waiter = true;
#ifdef SSF_EXPERIMENTS
        if (h->assoc_rstride) h->n_assoc_replica_frames++;          // (a frame the rule below repairs has bid into the replicas too, with whatever part of its grid was left)
#endif
        // The word has no acknowledgement.  A waiting workgroup gives up after SSF_ICP_GO_WAIT_TICKS (0.25 s) and tells the rest
        // of its launch to leave; if this thread was stalled that long (descheduled, a debugger, SIGSTOP) between the launch and
        // the store above, the word may have found only the late-dispatched part of the grid and the association would cover a
        // subset of the rows -- silently.  The host's own clock bounds the device's: no workgroup started waiting before
        // wait_launched_us, so below 0.1 s on this side nobody has given up.  Past it the association is run again as a launch
        // of its own: match_row only takes minima and sets flags, so a partial pass followed by a full one is the full one.
        if (now_us() - h->wait_launched_us > 100000.0) { matched_by_waiter = false; h->n_waiter_match_repairs++; }
    } else {
        if (w.waiting) icp_release_waiting(w.slot, w.go_seq, nullptr);
        icp_end(h, &valid);
    }
    f.t_b = now_us();
    if (f.kf >= 0 && f.kf < 64) h->seq_mark_us[2][f.kf] = f.t_b - h->seq_t0_us;
    if (f.timing) HCK(hipEventRecord(h->ev[2], h->stream));
    if (matched_by_waiter) h->n_waiter_matches++;
    else { const int rc = do_match(h, 1); if (rc) return rc; }
    if (h->comm) {
        // best key over the ranks (keys < 2^63: signed MIN == unsigned MIN), matched = OR over the ranks
        RcclApi* api = rccl_api();
        ScopedKernel sk("exchange_association", h->stream);
        NCK(api->AllReduce(h->cc->d_best, h->cc->d_best, h->S, ncclInt64, ncclMin, h->comm, h->stream));
        NCK(api->AllReduce(h->cc->d_matched, h->cc->d_matched, h->S, ncclUint8, ncclMax, h->comm, h->stream));
    }
    return SSF_OK;
}
// the two fuse halves, and between them -- a shard that exchanges natively -- the migrant tables of all ranks summed in HBM: rows whose
// fused position crossed a tile edge move to the rank that owns their new tile (one slot per frame supersurfel, at most one rank fills it)
static int exchange_and_fuse(ssf_handle* h, ssf_frame_result* r) {
    if (!exchanges_natively(h)) return do_fuse(h, r);
    static const int migrate = SSF_ENV_SET("NO_MIGRATE") ? 0 : 1;                  // (bisecting switch of tools/p2p_first_frame_stress.py)
    const int rc = fuse_begin(h, migrate);
    if (rc) { h->fusing = false; return rc; }
    if (h->fuse_migrate && h->p2p.on) launch_p2p_migrants(h->stream, p2p_view(h, ++h->p2p.seq_migr), h->d_migrants, h->d_tickets + 320, h->mb_dev);
    else if (h->fuse_migrate) {
        RcclApi* api = rccl_api();
        ScopedKernel sk("exchange_migrants", h->stream);
        const ncclResult_t nr = api->AllReduce(h->d_migrants, h->d_migrants, (size_t)SSF_MIGRANT_WORDS * h->S, ncclInt32, ncclSum, h->comm, h->stream);
        if (nr != ncclSuccess) {          // the frame cannot be completed: the handle must not stay "between the two halves"
            h->fusing = false;
            h->err = std::string("ncclAllReduce (migrant table): ") + (api->GetErrorString ? api->GetErrorString(nr) : "RCCL error");
            return SSF_ERR_DEVICE;
        }
    }
    return fuse_end(h, h->d_migrants, r);
}
// the stage split of a timed frame (ev[1] entry, ev[2] ICP done, ev[3] here): waits for the frame
static int stage_times(ssf_handle* h, ssf_frame_result* r) {
    HCK(hipEventRecord(h->ev[3], h->stream));
    HCK(hipEventSynchronize(h->ev[3]));
    float ms;
    ExtractCtx* ec = h->cc->ctx;      // extract time of the batch this frame came in, per frame
    if (hipEventElapsedTime(&ms, ec->ev_t0, ec->ev_t1) == hipSuccess) r->stage_ms[0] = ms / (float)ec->nb_launched;
    if (hipEventElapsedTime(&ms, h->ev[1], h->ev[2]) == hipSuccess) r->stage_ms[1] = ms;
    if (hipEventElapsedTime(&ms, h->ev[2], h->ev[3]) == hipSuccess) r->stage_ms[2] = ms;
    return SSF_OK;
}

// ICP + association + fusion of the oldest submitted frame, on the track stream
static int process_oldest(ssf_handle* h, const float* prior, ssf_frame_result* out) {
    TimerScope ts(h);
    int rc = activate_oldest(h);
    if (rc) return rc;
    TrackFrame f;
    f.t_a = now_us();
    f.kf = h->seq_n > 0 ? h->seq_k : -1;
    if (f.kf >= 0 && f.kf < 64) { h->seq_mark_us[0][f.kf] = f.t_a - h->seq_t0_us; h->seq_mark_us[1][f.kf] = 0; }
    if (h->ctx.size() > 1 && hipEventQuery(h->cc->ctx->ev_done) == hipSuccess) h->host_us[4] += 1;
    f.timing = h->cfg.profile != 0 && h->cc->ctx->timed;
    if (f.timing) HCK(hipEventRecord(h->ev[1], h->stream));
    if (exchanges_natively(h)) { rc = comm_counts(h); if (rc) return rc; }
    icp_begin(h, prior);
    rc = h->bins.make_if_large(h);
    h->assoc_rstride = rc ? 0 : assoc_replica_stride(h);
    if (!rc) rc = icp_chains(h) ? icp_loop_chained(h, f) : icp_loop_plain(h, f);
    if (!rc) rc = icp_loop_end(h, f);
    ssf_frame_result r;
    if (!rc) rc = exchange_and_fuse(h, &r);
    h->assoc_rstride = 0;                         // (the frame's: a stage seam that fuses next reads table 0 alone)
    if (rc) return rc;
    if (h->pending.empty()) h->ahead_tuner.sequence_break(); else h->ahead_tuner.frame_done(now_us(), r.icp_iters);
    h->host_us[1] += f.t_b - f.t_a; h->host_us[2] += now_us() - f.t_b; h->host_us[3] += 1;
    if (f.timing) { rc = stage_times(h, &r); if (rc) return rc; }
    if (out) *out = r;
    return SSF_OK;
}
static int process_frame_impl(ssf_handle* h, const void* rgb, const void* depth, int on_device, const float* prior,
                              const uint8_t* mask, ssf_frame_result* out, const uint8_t* pixmask = nullptr, int pixmask_on_device = -1) {
    if (!frame_args_ok(h, rgb, depth, on_device)) return SSF_ERR_INVALID_ARG;
    if (!h->pending.empty()) { h->err = "frames are pending in the extract pipeline: use ssf_process_submitted"; return SSF_ERR_STATE; }
    int rc;
    { TimerScope ts(h); rc = submit_extract(h, rgb, depth, on_device, mask, pixmask, pixmask_on_device < 0 ? on_device : pixmask_on_device); }
    return rc ? rc : process_oldest(h, prior, out);
}

// ---- what the entry points of ssf_render.hip, ssf_graph.hip and ssf_keyframes.hip share with the ones here (ssf_handle.hpp) ----
namespace ssf {
bool frame_inputs_ok(ssf_handle* h, const void* rgb, const void* depth, int on_device) { return frame_args_ok(h, rgb, depth, on_device); }
int process_frame_devmask(ssf_handle* h, const void* rgb, const void* depth, int on_device, const float* prior, const uint8_t* d_pixmask,
                          ssf_frame_result* out) {
    return process_frame_impl(h, rgb, depth, on_device ? 1 : 0, prior, nullptr, out, d_pixmask, 1);
}
int copy_rows(ssf_handle* h, const ssf_surfels& dst, size_t d0, const ssf_surfels& src, size_t s0, size_t n, hipMemcpyKind kind) {
    if (n == 0) return SSF_OK;
    auto one = [&](auto* d, const auto* s, size_t w) { return d ? hipMemcpyAsync(d + w * d0, s + w * s0, 4 * w * n, kind, h->stream) : hipSuccess; };
    HCK(one(dst.positions, src.positions, 3)); HCK(one(dst.colors, src.colors, 3)); HCK(one(dst.stamps, src.stamps, 2));
    HCK(one(dst.orientations, src.orientations, 9)); HCK(one(dst.shapes, src.shapes, 6)); HCK(one(dst.dims, src.dims, 2));
    HCK(one(dst.confidences, src.confidences, 1));
    return SSF_OK;
}
// the six arrays a row set in streams shares with ssf_surfels (its orientations are three streams: transposed where they cross)
static ssf_surfels soa_surfels(const SurfelSoA& s) { return ssf_surfels{s.pos, s.col, s.stamps, nullptr, s.shape, s.dims, s.conf}; }
// what ssf_render_model and ssf_graph_build read: both stores of the handle in place (visible_only: without the out-of-view span)
ModelView model_view(const ssf_handle* h, bool visible_only) {
    ModelView mv;
    mv.vis = h->model[h->mcur]; mv.oov = h->oov[h->ocur];
    mv.n_visible = h->n_visible; mv.nbv = (h->n_visible + 255) / 256; mv.nvs = 256 * mv.nbv;
    mv.oov_head = h->oov_head; mv.oov_tail = h->oov_tail;
    mv.nbo = visible_only ? 0 : (h->oov_tail - h->oov_head + 255) / 256;
    mv.nslots = 256 * (mv.nbv + mv.nbo);
    return mv;
}
// the refusals of the calls that work on the model between frames: frames in flight and, for a call that does not serve a
// sharded handle (who != nullptr), such a handle: "<who>: a sharded handle (cfg.nranks > 1) <lacks>"
int model_at_rest(ssf_handle* h, const char* who, const char* lacks) {
    if (!h->pending.empty() || h->fusing) { h->err = "frames are pending in the extract pipeline"; return SSF_ERR_STATE; }
    if (who && h->cfg.nranks > 1) { h->err = std::string(who) + ": a sharded handle (cfg.nranks > 1) " + lacks; return SSF_ERR_STATE; }
    return SSF_OK;
}
// the iterations of align on device sources (ssf_align: uploaded; ssf_keyframes_align: derived from the stored rows); d_out: 40 i64
int align_loop(ssf_handle* h, const float* d_pos, const float* d_lab, const float* d_nrm, const float* d_conf, int n, long long* d_out,
               const float* init_pose, float* rel_pose, int* valid, int* iters, int* pairs_last) {
    hipStream_t st = h->stream;
    int rc = SSF_OK;
    M3 R_init = m3_identity(); V3 t_init = v3(0, 0, 0);
    if (init_pose) { const Rt p0 = pose_from12(init_pose); R_init = p0.R; t_init = p0.t; }
    double tf_inc[16], JtJ[36];
    for (int i = 0; i < 16; i++) tf_inc[i] = (i % 5 == 0) ? 1.0 : 0.0;
    for (int i = 0; i < 36; i++) JtJ[i] = 0.0;
    M3 R_inc = m3_identity(); V3 t_inc = v3(0, 0, 0);
    bool ok = true;
    int it = 0, pairs = 0;
    static const int tri[6][6] = {{0, 1, 2, 3, 4, 5}, {1, 6, 7, 8, 9, 10}, {2, 7, 11, 12, 13, 14},
                                  {3, 8, 12, 15, 16, 17}, {4, 9, 13, 16, 18, 19}, {5, 10, 14, 17, 19, 20}};
    while (it < h->cfg.icp_iter) {
        it++;
        inc_to_float(tf_inc, R_inc, t_inc);
        Rt T; T.R = m3_mul(R_inc, R_init); T.t = add(m3_mulv(R_inc, t_init), t_inc);
        launch_align(st, h->cam, d_pos, d_lab, d_nrm, d_conf, n, h->cc->frame, h->cc->maps.label, h->cc->maps.plane_depth, T, d_out);
        long long rec[40];
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(rec, d_out, 37 * sizeof(long long), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) { rc = SSF_ERR_DEVICE; h->err = "align iteration failed on the device"; break; }
        pairs = (int)rec[29];
        if (pairs < 100) { ok = false; break; }
        float cs[3], ct[3], scale;
        for (int i = 0; i < 3; i++) {
            const uint32_t a = (uint32_t)rec[30 + i], b = (uint32_t)rec[33 + i];
            std::memcpy(&cs[i], &a, 4); std::memcpy(&ct[i], &b, 4);
        }
        { const uint32_t a = (uint32_t)rec[36]; std::memcpy(&scale, &a, 4); }
        double Jtr[6];
        for (int i = 0; i < 6; i++) {
            for (int j = 0; j < 6; j++) JtJ[i * 6 + j] = (double)rec[tri[i][j]] / SSF_ICP_SCALE_JTJ;
            Jtr[i] = (double)rec[21 + i] / SSF_ICP_SCALE_JTR;
        }
        double tf_iter[16];
        align_increment(JtJ, Jtr, scale, cs, ct, tf_iter);
        mat4_lmul(tf_iter, tf_inc);
    }
    if (rc) return rc;
    double cov[36];
    mat6_inverse_lu(JtJ, cov);
    for (int i = 0; i < 6; i++) if (cov[i * 6 + i] > h->cfg.icp_cov_thresh) { ok = false; break; }
    Rt rel; rel.R = m3_identity(); rel.t = v3(0, 0, 0);
    if (ok) {
        if (len3(t_inc) > 0.3f) ok = false;                      // stale t_inc (start of the last iteration), :226
        else { rel.R = m3_transpose(R_inc); rel.t = negate(m3_mulv(rel.R, t_inc)); }
    }
    pose_to12(rel, rel_pose);
    *valid = ok ? 1 : 0;
    if (iters) *iters = it;
    if (pairs_last) *pairs_last = pairs;
    if (h->cfg.profile == 1) timer_collect(&h->timer);
    return SSF_OK;
}
// the shared part of ssf_apply_deformation and ssf_graph_apply: k_pack_nodes + k_deformation on the dense logical view (weights are
// per logical row) with device arrays, then the split back into the two stores
int deform_dense(ssf_handle* h, int m, const float* d_np, const float* d_nr, const float* d_nt, float* d_nodes, const float* d_w,
                 const int32_t* d_i) {
    hipStream_t st = h->stream;
    { int rc = materialise(h); if (rc) return rc; }
    { TimerScope ts(h); launch_deformation(st, h->dense, h->n_model, m, d_np, d_nr, d_nt, d_nodes, d_w, d_i); }
    { int rc = store_from_dense(h, h->n_model, h->n_visible); if (rc) return rc; }
    return sync_collect(h);
}
}  // namespace ssf

// ---- C ABI ----------------------------------------------------------------------------------------------
// (kernels of ssf_stream_copy_rate, further down)
typedef float f4v __attribute__((ext_vector_type(4)));
template <int U, bool NT, bool ONE_PASS>
__global__ __launch_bounds__(256) void k_stream_copy(const f4v* __restrict__ in, f4v* __restrict__ out, size_t n) {
    // (n is a multiple of U x the grid's threads -- ssf_stream_copy_rate rounds to 256 MiB and refuses less: the first round is unguarded)
    const size_t stride = ONE_PASS ? (size_t)256 : (size_t)gridDim.x * 256;
    size_t i = ONE_PASS ? (size_t)blockIdx.x * 256 * U + threadIdx.x : (size_t)blockIdx.x * 256 + threadIdx.x;
    do {
        f4v v[U];
#pragma unroll
        for (int k = 0; k < U; k++) v[k] = NT ? __builtin_nontemporal_load(&in[i + k * stride]) : in[i + k * stride];
#pragma unroll
        for (int k = 0; k < U; k++) { if (NT) __builtin_nontemporal_store(v[k], &out[i + k * stride]); else out[i + k * stride] = v[k]; }
        i += U * stride;
    } while (!ONE_PASS && i + (U - 1) * stride < n);
}

extern "C" {

int ssf_abi_version(void) { return SSF_ABI_VERSION; }
const char* ssf_backend_name(void) { return "hip-gfx950"; }

void ssf_default_config(ssf_config* c) {       // default arguments of initialize, supersurfel_fusion.hpp:46-74
    std::memset(c, 0, sizeof(*c));
    c->width = 640; c->height = 480; c->fx = 525.f; c->fy = 525.f; c->cx = 319.5f; c->cy = 239.5f;
    c->cell_size = 16; c->lambda_pos = 50.f; c->lambda_bound = 1000.f; c->lambda_size = 10000.f;
    c->lambda_disp = 1e6f; c->thresh_disp = 1e-4f; c->seg_iter = 10; c->seg_use_ransac = 1;
    c->nb_samples = 16; c->filter_iter = 4; c->filter_alpha = 0.1f; c->filter_beta = 1.0f;
    c->filter_threshold = 0.05f; c->range_min = 0.2f; c->range_max = 5.0f; c->delta_t = 20;
    c->conf_thresh = 2500.f; c->nb_supersurfels_max = 50000; c->icp_iter = 10; c->icp_cov_thresh = 0.04;
    c->rng_seed = 1234; c->icp_force_iters = 0; c->device_id = 0; c->stream = nullptr;
    c->rank = 0; c->nranks = 1; c->shard_tile = 0.5f; c->profile = 0;
    c->depth_prefilter = 1; c->prefilter_sigma_color = 0.03f; c->prefilter_sigma_space = 4.5f;
    c->pipeline_depth = 0; c->extract_batch = 1;
}

void ssf_destroy(ssf_handle* h) {
    if (!h) return;
    if (h->up) {
        h->up->stop.store(1);
        h->up->join();
        h->up->shutdown();
        for (auto q : h->up->p_rgb) if (q) (void)hipHostFree(q);
        for (auto q : h->up->p_depth) if (q) (void)hipHostFree(q);
        for (auto q : h->up->p_mask) if (q) (void)hipHostFree(q);
        delete h->up; h->up = nullptr;
    }
    for (auto& c : h->ctx) if (c.stream) (void)hipStreamSynchronize(c.stream);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& c : h->ctx) if (c.deal_comm) { RcclApi* api = rccl_api(); if (api) (void)api->CommDestroy(c.deal_comm); c.deal_comm = nullptr; }
    if (h->comm) { RcclApi* api = rccl_api(); if (api) (void)api->CommDestroy(h->comm); h->comm = nullptr; }
    for (void* q : h->p2p.opened) (void)hipIpcCloseMemHandle(q);
    if (h->p2p.region) (void)hipFree(h->p2p.region);
    for (auto& c : h->ctx) {
        for (int n = 0; n <= SSF_MAX_BATCH; n++) { if (c.exec[n]) (void)hipGraphExecDestroy(c.exec[n]); if (c.graph[n]) (void)hipGraphDestroy(c.graph[n]); }
        for (int n = 0; n <= SSF_MAX_BATCH; n++) { if (c.exec_pm[n]) (void)hipGraphExecDestroy(c.exec_pm[n]); if (c.graph_pm[n]) (void)hipGraphDestroy(c.graph_pm[n]); }
        hipEvent_t evs[4] = {c.ev_done, c.ev_consumed, c.ev_t0, c.ev_t1};
        for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e);
        if (c.own_stream && c.stream) stream_pool().give(c.stream, h->cfg.device_id, c.stream_prio);          // (synchronised above)
    }
    if (h->capture_stream) stream_pool().give(h->capture_stream, h->cfg.device_id, StreamPool::CAPTURE);
    if (!h->guarded.empty() && !SSF_ENV_SET("GUARD_ONLY")) check_guards(h);
    for (void* p : h->allocs) (void)hipFree(p);
    // (the workspaces -- render, graph, keyframes and any later one -- free their buffers with the handle below: ~DevBufs)
    if (h->mb_host) (void)hipHostFree(h->mb_host);
    for (int i = 0; i < 4; i++) if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
    for (auto& r : h->timer.pool_free) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    if (h->own_stream && h->stream) { (void)hipStreamSynchronize(h->stream); stream_pool().give(h->stream, h->cfg.device_id, h->stream_prio); }
    delete h;
}

int ssf_create(const ssf_config* cfg, ssf_handle** out) {
    if (!cfg || !out) { g_create_err = "null argument"; return SSF_ERR_INVALID_ARG; }
    if (cfg->width <= 0 || cfg->height <= 0 || cfg->cell_size <= 0 || cfg->nb_samples <= 0 || cfg->nb_samples > 64 ||
        cfg->nb_supersurfels_max <= 0 || cfg->nranks < 1 || cfg->rank < 0 || cfg->rank >= cfg->nranks) {
        g_create_err = "invalid configuration"; return SSF_ERR_INVALID_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        g_create_err = "no HIP device: libssf_hip.so needs a gfx950 GPU (there is no CPU fallback)";
        return SSF_ERR_NO_DEVICE;
    }
    if (cfg->device_id < 0 || cfg->device_id >= ndev) { g_create_err = "device_id out of range"; return SSF_ERR_INVALID_ARG; }
    if (hipSetDevice(cfg->device_id) != hipSuccess) { g_create_err = "hipSetDevice failed"; return SSF_ERR_DEVICE; }
    ssf_handle* h = new (std::nothrow) ssf_handle();
    if (!h) return SSF_ERR_DEVICE;
    h->cfg = *cfg;
    const int W = cfg->width, H = cfg->height, c = cfg->cell_size;
    h->gx = (W + c - 1) / c; h->gy = (H + c - 1) / c; h->S = h->gx * h->gy;
    if (cfg->nb_supersurfels_max < h->S) { delete h; g_create_err = "nb_supersurfels_max < nbSuperpixels"; return SSF_ERR_INVALID_ARG; }
#ifndef SSF_MOVE_TOTALS_DEFAULT
#define SSF_MOVE_TOTALS_DEFAULT 1
#endif
    h->move_totals_on = SSF_ENV_INT("MOVE_TOTALS", SSF_MOVE_TOTALS_DEFAULT) != 0;      // (-DSSF_MOVE_TOTALS_DEFAULT=0: a product build that keeps the fuse launch's tail, for the A/B)
    h->icp_ahead_mode = SSF_ENV_INT("ICP_AHEAD", 1);      // (lab: measurement switches, tools/)
    h->icp_ahead = h->icp_ahead_mode != 0;
    h->ahead_tuner.forced = SSF_ENV_INT("ICP_AHEAD", -1);  // (lab: 0 / 1 / 2 pin the form; the product measures, see AheadTuner)
    h->icp_chain = SSF_ENV_INT("ICP_CHAIN", 1) != 0;
    if (SSF_ENV_SET("NO_GRAPH")) h->graph_failed = true;                             // extract chain launched eagerly
    if (cfg->stream) h->stream = (hipStream_t)cfg->stream;
    else {
        // own track stream: highest priority (ICP -> fuse is the serial chain of the pipeline; its short kernels
        // should not queue behind the wide extract launches of the low-priority context streams)
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        const int prio = SSF_ENV_INT("TRACK_PRIORITY", greatest);
        h->stream = stream_pool().take(cfg->device_id, prio);
        if (!h->stream) { delete h; g_create_err = "hipStreamCreate failed"; return SSF_ERR_DEVICE; }
        h->own_stream = true; h->stream_prio = prio;
    }
    SegParams& p = h->seg;
    p.W = W; p.H = H; p.cell = c; p.gx = h->gx; p.gy = h->gy; p.S = h->S; p.nb_samples = cfg->nb_samples;
    p.min_size = (int)((float)(c * c) / 4.f);                                   // TPS_RGBD.cu:198 (float -> int parameter)
    p.lambda_pos = cfg->lambda_pos; p.lambda_bound = cfg->lambda_bound; p.lambda_size = cfg->lambda_size;
    p.lambda_disp = cfg->lambda_disp; p.thresh_disp = cfg->thresh_disp;
    p.filter_alpha = cfg->filter_alpha; p.filter_beta = cfg->filter_beta; p.filter_threshold = cfg->filter_threshold;
    p.filter_iter = cfg->filter_iter; p.seed = cfg->rng_seed;
    p.inv_gx = 1.0f / (float)h->gx;
    p.cell_magic = c > 1 ? (uint32_t)((0x100000000ull + (uint64_t)c - 1) / (uint64_t)c) : 0u;
    p.win_cells_max = tile_window_cells_max(W, H, p.cell_magic);          // (selects the LDS footprint of the tile kernels: ssf_extract.hip, WCAP)
    h->cam.fx = cfg->fx; h->cam.fy = cfg->fy; h->cam.cx = cfg->cx; h->cam.cy = cfg->cy; h->cam.W = W; h->cam.H = H;
    h->classify = ClassifyArgs{h->cam, nullptr, cfg->delta_t, cfg->conf_thresh, cfg->range_min, cfg->range_max};
    h->shard = ShardArgs{cfg->rank, cfg->nranks, 0, cfg->shard_tile};
    const size_t P = (size_t)W * H, S = h->S, N = cfg->nb_supersurfels_max, NS = S * cfg->nb_samples;
    // relabelling tiles (the shifted grid has one more column), a log region of 256 entries each.  NT32 is the grid k_update_pass
    // runs (pass_geometry_entries / 2); the larger 2 * NT64 is what the 64-wide tiles deleted in round 6 needed.  It stays until the
    // smaller slab has been measured: every pointer carved behind the logs moves with it (profiles/pass_body_refactor.txt).
    const size_t NT32 = (size_t)((W + 30 + 31) / 32) * ((H + 31) / 32), NT64 = (size_t)((W + 62 + 63) / 64) * ((H + 31) / 32);
    const size_t NT = std::max(NT32, 2 * NT64);
    const int nctx = std::max(0, std::min(cfg->pipeline_depth, SSF_MAX_PIPELINE_DEPTH)) + 1;
    h->batch = std::max(1, std::min(cfg->extract_batch, SSF_MAX_BATCH));
    h->ctx.resize(nctx);
    bool ok = dalloc(h, &h->d_srgb_lut, 256) && dalloc(h, &h->d_tickets, 512);
    {   // window geometry of the relabelling tiles (SegParams::pass_geom)
        const int ne = pass_geometry_entries(W, H);
        std::vector<PassGeomEntry> tab((size_t)ne);
        p.pass_geom = nullptr; p.pass_ntile = ne / 2;
        pass_geometry_table(W, H, p.cell_magic, tab.data());
        PassGeomEntry* d_geom = nullptr;
        ok = ok && dalloc(h, &d_geom, (size_t)ne) && hipMemcpy(d_geom, tab.data(), (size_t)ne * sizeof(PassGeomEntry), hipMemcpyHostToDevice) == hipSuccess;
        if (ok) p.pass_geom = d_geom;
    }
    // working set of one frame, carved out of a slab (256 B aligned pieces); a context owns `batch` slabs
    auto carve = [&](ExtractCtx& c, char* base) -> size_t {
        size_t off = 0;
        auto take = [&](auto*& ptr, size_t count) {
            using T = typename std::remove_reference<decltype(*ptr)>::type;
            off = (off + 255) & ~(size_t)255;
            ptr = reinterpret_cast<T*>(base + off);
            off += std::max<size_t>(count, 1) * sizeof(T);
        };
        FrameMaps& m = c.maps;
        take(m.rgba, P); take(m.disp, P); take(m.label, P); take(m.inlier, P); take(m.plane_depth, P);
        take(m.sp, S); take(m.samples, NS); take(m.sample_score, NS); take(m.moments, 13 * S); take(m.filt, 11 * S); take(m.epoch, 64); take(m.pix2, P); take(m.fpack, 4 * S);
        for (int b = 0; b < 2; b++) take(m.sums[b].r, S);
        for (int b = 0; b < 3; b++) { take(m.log.ent[b], NT * 256); take(m.log.disp[b], NT * 256); take(m.log.count[b], NT); }
        SurfelSoA& f = c.frame;
        take(f.pos, 3 * S); take(f.col, 3 * S); take(f.lab, 3 * S); take(f.stamps, 2 * S); take(f.r0, 3 * S); take(f.r1, 3 * S);
        take(f.r2, 3 * S); take(f.shape, 6 * S); take(f.dims, 2 * S); take(f.conf, S);
        take(c.d_best, assoc_table_words(S)); take(c.d_matched, S); take(c.d_rgb_in, 4 * P); take(c.d_depth_in, P); take(c.d_depth_filt, P); take(c.d_mask, S);
        take(c.d_wire, 26 * S);
        take(c.d_pixmask, P); take(c.d_pixcnt, 2 * S);
        return (off + 255) & ~(size_t)255;
    };
    size_t slab_bytes = 0;
    for (int ci = 0; ci < nctx && ok; ci++) {
        ExtractCtx& c = h->ctx[ci];
        slab_bytes = carve(c, nullptr);
        char* base = nullptr;
        ok = dalloc(h, &base, slab_bytes * h->batch);
        if (!ok) break;
        (void)carve(c, base);
        FrameMaps& m = c.maps;
        m.slab = slab_bytes;
        m.srgb_lut = h->d_srgb_lut;
        (void)hipMemsetAsync(base, 0, slab_bytes * h->batch, h->stream);
        if (nctx == 1) c.stream = h->stream;                            // sequential: extract shares the track stream
        else {
            // low priority: the track chain (ICP -> fuse, on h->stream) is the critical path, and the
            // runtime keeps a separate pool of hardware queues per priority, so every context gets a
            // queue of its own instead of sharing one with the track stream (head-of-line blocking)
            // (context 0 one level above the others: a sequence that starts on an empty pipeline puts its first, small batch
            // there -- ssf_process_sequence -- and that batch is what the track chain waits for while the larger batches of the
            // other contexts, launched microseconds later, compete for the part.  SSF_CTX0_PRIORITY=0 switches it off.)
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            static const bool ctx0_up = SSF_ENV_INT("CTX0_PRIORITY", 1) != 0;
            const int prio = (ci == 0 && ctx0_up && least - greatest >= 2) ? least - 1 : least;
            c.stream = stream_pool().take(h->cfg.device_id, prio); ok = c.stream != nullptr; c.own_stream = ok; c.stream_prio = prio;
        }
        ok = ok && hipEventCreateWithFlags(&c.ev_done, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&c.ev_consumed, hipEventDisableTiming) == hipSuccess &&
             hipEventCreate(&c.ev_t0) == hipSuccess && hipEventCreate(&c.ev_t1) == hipSuccess;
    }
    const size_t OC = 3 * N + 4 * S + 1024;        // out-of-view store: home of the span = N + S + 256, room for N rows either side (+ 2 S appended per frame)
    h->part_sup_vis = 6 * (int)(((N + 255) / 256 + 2) / PART_GROUP + 1);
    h->part_sup_oov = (int)(((OC + 255) / 256 + 8) / PART_GROUP + 1);
    h->part_words = h->part_sup_vis + h->part_sup_oov + 8 * PART_REPLICAS;
    ok = ok && dalloc(h, &h->d_part, 2 * (size_t)h->part_words) && dalloc(h, &h->d_part_ticket, 128);
    if (ok) {
        // host-writable device memory for the chained ICP launches; without it (no large BAR) the launches are not chained
        void* q = nullptr;
        int large_bar = 0;
        (void)hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, cfg->device_id);
        // (behind the SSF_ICP_GO_SLOTS lines of the launches made ahead: the resident launch's, two sets of icp_iter + 1 -- ssf_handle.hpp)
        const size_t n_res = cfg->icp_iter > 0 && cfg->icp_iter < 4096 ? 2 * ((size_t)cfg->icp_iter + 1) : 0;
        if (large_bar && hipExtMallocWithFlags(&q, (SSF_ICP_GO_SLOTS + n_res) * sizeof(IcpGo), hipDeviceMallocFinegrained) == hipSuccess) {
            h->allocs.push_back(q); h->go = (IcpGo*)q;
            (void)hipMemset(q, 0, (SSF_ICP_GO_SLOTS + n_res) * sizeof(IcpGo));
            if (n_res) { h->go_res = h->go + SSF_ICP_GO_SLOTS; h->resident_max_rows = 256 * icp_resident_max_wgs(); }
        } else { (void)hipGetLastError(); h->go = nullptr; }
    }
    ok = ok && alloc_surfels(h, h->model[0], N) && alloc_surfels(h, h->model[1], N) && alloc_surfels(h, h->dense, N) &&
         alloc_surfels(h, h->oov[0].rows, OC) && alloc_surfels(h, h->oov[1].rows, OC) && dalloc(h, &h->oov[0].live, OC) &&
         dalloc(h, &h->oov[1].live, OC) && dalloc(h, &h->d_state_oov, OC) && dalloc(h, &h->d_bc_oov, (OC + 255) / 256 + 8) &&
         dalloc(h, &h->d_live_scratch, N) && dalloc(h, &h->d_bf_in, P) && dalloc(h, &h->d_bf_out, P) &&
         dalloc(h, &h->d_icp, 64) && dalloc(h, &h->d_state, N + 16) && dalloc(h, &h->d_cand, N) &&
         dalloc(h, &h->d_cnt, 2) && dalloc(h, &h->d_migrants, (size_t)SSF_MIGRANT_WORDS * S) && dalloc(h, &h->d_scratch_map, P) && dalloc(h, &h->d_icp_replicas, 2 * SSF_ICP_REPLICAS * 32)     /* second half: the counted record of k_icp */;
#ifdef SSF_EXPERIMENTS
    h->bins.min_rows = SSF_ENV_INT("BIN_MIN_ROWS", SSF_BIN_MIN_ROWS_DEFAULT);          // (lab: the threshold by environment; < 0 never.  The copy's buffers are allocated on first use)
#endif
    if (ok) {
        ok = hipHostMalloc((void**)&h->mb_host, sizeof(Mailbox), hipHostMallocCoherent) == hipSuccess ||
             hipHostMalloc((void**)&h->mb_host, sizeof(Mailbox), hipHostMallocDefault) == hipSuccess;
        if (ok) { std::memset(h->mb_host, 0, sizeof(Mailbox)); ok = hipHostGetDevicePointer((void**)&h->mb_dev, h->mb_host, 0) == hipSuccess; }
    }
    for (int i = 0; i < 4 && ok; i++) ok = hipEventCreate(&h->ev[i]) == hipSuccess;
    if (!ok) { g_create_err = std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError()); ssf_destroy(h); return SSF_ERR_DEVICE; }
    {   // gamma-expansion table for 8-bit colours, built with the same inline function the kernels use
        float lut[256];
        for (int c8 = 0; c8 < 256; c8++) lut[c8] = srgb_expand((float)c8 / 255.0f);
        (void)hipMemcpy(h->d_srgb_lut, lut, sizeof(lut), hipMemcpyHostToDevice);
    }
    (void)hipMemsetAsync(h->d_icp_replicas, 0, 2 * SSF_ICP_REPLICAS * 32 * sizeof(long long), h->stream);
    (void)hipMemsetAsync(h->d_tickets, 0, 512 * sizeof(unsigned int), h->stream);
    (void)hipMemsetAsync(h->d_part, 0, 2 * (size_t)h->part_words * sizeof(uint32_t), h->stream);
    (void)hipMemsetAsync(h->d_part_ticket, 0, 128 * sizeof(uint32_t), h->stream);
    (void)hipMemsetAsync(h->d_cand, 0xFF, N * sizeof(int32_t), h->stream);
    h->oov[0].cap = h->oov[1].cap = (int)OC;
    h->oov_head = h->oov_tail = oov_home(h); h->oov_live = 0;
    {
        Counters c0; std::memset(&c0, 0, sizeof(c0)); c0.oov_head = c0.oov_tail = h->oov_head;
        (void)hipMemcpy(h->d_cnt, &c0, sizeof(c0), hipMemcpyHostToDevice);
    }
    (void)hipMemsetAsync(h->oov[0].live, 0, OC, h->stream); (void)hipMemsetAsync(h->oov[1].live, 0, OC, h->stream);
    zero_surfels(h, h->model[0], N); zero_surfels(h, h->model[1], N); zero_surfels(h, h->dense, N);
    if (hipStreamSynchronize(h->stream) != hipSuccess) { g_create_err = "initialisation failed"; ssf_destroy(h); return SSF_ERR_DEVICE; }
    {   // getters before the first frame see slot 0 of context 0 (zeroed)
        ExtractCtx& c0 = h->ctx[0];
        h->active.maps = c0.maps; h->active.frame = c0.frame; h->active.d_best = c0.d_best; h->active.d_matched = c0.d_matched;
        h->active.ctx = &c0; h->active.slot = 0;
    }
    h->pose.R = m3_identity(); h->pose.t = v3(0, 0, 0);
    *out = h;
    return SSF_OK;
}
const char* ssf_last_error(const ssf_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int ssf_process_frame(ssf_handle* h, const uint8_t* rgb, const float* depth, const float* prior, const uint8_t* mask, ssf_frame_result* out) { return process_frame_impl(h, rgb, depth, 0, prior, mask, out); }
int ssf_process_frame_device(ssf_handle* h, const void* rgb, const void* depth, const float* prior, const uint8_t* mask, ssf_frame_result* out) { return process_frame_impl(h, rgb, depth, 1, prior, mask, out); }

// pipelined form: extract of future frames runs ahead on its own stream(s)
static int submit_frame(ssf_handle* h, const void* rgb, const void* depth, int on_device, const uint8_t* mask, const uint8_t* pixmask) {
    if (!frame_args_ok(h, rgb, depth, on_device)) return SSF_ERR_INVALID_ARG;
    TimerScope ts(h);
    const double t0 = now_us();
    int rc = submit_extract(h, rgb, depth, on_device, mask, pixmask, on_device);
    h->host_us[0] += now_us() - t0;
    return rc;
}
int ssf_submit_frame(ssf_handle* h, const void* rgb, const void* depth, int on_device, const uint8_t* mask) { return submit_frame(h, rgb, depth, on_device, mask, nullptr); }
int ssf_submit_frame_tables(ssf_handle* h, const int32_t* label, const float* plane_depth, const ssf_surfels* frame, int on_device) {
    if (!h || !label || !plane_depth || !frame) return SSF_ERR_INVALID_ARG;
    if (!frame->positions || !frame->colors || !frame->stamps || !frame->orientations || !frame->shapes || !frame->dims || !frame->confidences) return SSF_ERR_INVALID_ARG;
    // (dealt extract counts batches to choose the broadcasting rank; a frame handed in here would not be counted and the ranks'
    //  root choice would drift apart: the two ways of receiving a frame extracted elsewhere do not mix)
    if (h->deal != 0) { h->err = "ssf_submit_frame_tables: the handle deals its extract stage (ssf_comm_deal_extract); submit frames, not tables"; return SSF_ERR_STATE; }
    TimerScope ts(h);
    return submit_tables(h, label, plane_depth, frame, on_device);
}
int ssf_process_submitted(ssf_handle* h, const float* prior, ssf_frame_result* out) {
    if (!h) return SSF_ERR_INVALID_ARG;
    return process_oldest(h, prior, out);
}
static int process_sequence_impl(ssf_handle* h, const void* const* rgb, const void* const* depth, const uint8_t* const* pixmasks, int n,
                                 int on_device, ssf_frame_result* out) {
    if (!h || !rgb || !depth || n < 0) return SSF_ERR_INVALID_ARG;
    if (!h->pending.empty()) { h->err = "frames are pending in the extract pipeline"; return SSF_ERR_STATE; }
    for (int i = 0; i < n; i++) if (!rgb[i] || !depth[i]) return SSF_ERR_INVALID_ARG;
    if (on_device) for (int i = 0; i < n; i++) if (!device_input_aligned(h, rgb[i], depth[i])) return SSF_ERR_INVALID_ARG;
    int rc = SSF_OK;
    // an empty pipeline: the sequence's first (small) batch goes to context 0, whose stream outranks the other contexts'
    // (ssf_create): the batch the track chain is waiting for is not slowed down by the larger ones launched right behind it
    if (h->ctx.size() > 1 && !h->ctx[h->open_ctx].launched && h->ctx[h->open_ctx].count == 0) {
        bool idle = true;
        for (auto& c : h->ctx) idle = idle && !c.launched && c.count == 0;
        if (idle) h->open_ctx = 0;
    }
    const bool ahead = !on_device && h->ctx.size() > 1 && n > 1;       // host frames, pipelined: copy them ahead
    if (ahead) {
        const size_t P = (size_t)h->cfg.width * h->cfg.height;
        if (!h->up) {
            Uploader* u = new (std::nothrow) Uploader();
            if (!u) { h->err = "out of memory"; return SSF_ERR_DEVICE; }
            // The submitting thread runs up to (contexts + 1) batches ahead of the frame being tracked (every context full + the open
            // batch); a worker may start on frame i when frame i - ring has been processed and needs ~250 us for it (wake-up, 2.1 MB
            // staging memcpy, two enqueues).  With a ring of only two frames more than that window (round 1-4) the submitting thread --
            // the one that drives the track chain -- waited 18 us per frame for uploads and the replay ran at 6100-6300 frames/s on hosts
            // with a slower memcpy (8800-10 000 on faster ones) against 11 400 with frames in HBM: tools/host_buffer_probe.py.  Two
            // more batches of slack.
            // The ring is capped by BYTES as well (advisor, round 4: at depth 3 x 16 frames per launch the formula asks for 98 slots =
            // 0.85 GB of HBM and as much page-locked host memory at 1280x960, held until ssf_destroy): never more than
            // SSF_UPLOAD_RING_BYTES of device buffers (and the same again page-locked), never fewer than the window the submitting
            // thread can run ahead by + 2 (below that the workers could not keep up at all).  INTEGRATION.md section 2b has the footprint.
            const int window = ((int)h->ctx.size() + 1) * h->batch + 2;
            // (slots sized for the largest input format, ssf_input.h: 4 colour bytes per pixel; a format change reallocates nothing)
            const int by_bytes = (int)(SSF_UPLOAD_RING_BYTES / (8 * P));
            u->ring = std::max(window, std::min(((int)h->ctx.size() + 3) * h->batch + 2, by_bytes));
            u->device = h->cfg.device_id;
            bool ok = true;
            // (and P bytes per slot for a pixel mask, ssf_process_sequence_pixmask: allocated with the ring, never mid-sequence)
            u->d_rgb.assign(u->ring, nullptr); u->d_depth.assign(u->ring, nullptr); u->d_mask.assign(u->ring, nullptr);
            for (int i = 0; i < u->ring && ok; i++) ok = dalloc(h, &u->d_rgb[i], 4 * P) && dalloc(h, &u->d_depth[i], P) && dalloc(h, &u->d_mask[i], P);
            if (ok && !SSF_ENV_SET("UPLOAD_PAGEABLE")) {     // page-locked staging (optional: without it the copies go through the runtime's)
                u->p_rgb.assign(u->ring, nullptr); u->p_depth.assign(u->ring, nullptr); u->p_mask.assign(u->ring, nullptr);
                bool pin = true;
                for (int i = 0; i < u->ring && pin; i++)
                    pin = hipHostMalloc((void**)&u->p_rgb[i], 4 * P, hipHostMallocDefault) == hipSuccess &&
                          hipHostMalloc((void**)&u->p_depth[i], 4 * P, hipHostMallocDefault) == hipSuccess &&
                          hipHostMalloc((void**)&u->p_mask[i], P, hipHostMallocDefault) == hipSuccess;
                if (!pin) {
                    for (auto q : u->p_rgb) if (q) (void)hipHostFree(q);
                    for (auto q : u->p_depth) if (q) (void)hipHostFree(q);
                    for (auto q : u->p_mask) if (q) (void)hipHostFree(q);
                    u->p_rgb.clear(); u->p_depth.clear(); u->p_mask.clear(); (void)hipGetLastError();
                }
            }
            for (auto& c : h->ctx) u->ctx_stream.push_back(c.stream);
            u->batch = h->batch;
            if (!ok) { delete u; h->err = "allocation of the upload ring failed"; return SSF_ERR_DEVICE; }    // (buffers taken so far stay in h->allocs)
            h->up = u;
        }
        Uploader& u = *h->up;
        u.n = n; u.rgb = rgb; u.depth = depth; u.ctx0 = h->open_ctx;
        u.rgb_bytes = color_bpp(h) * P; u.depth_bytes = depth_bpp(h) * P;
        u.masks = pixmasks; u.mask_bytes = P;
        u.processed.store(0); u.failed.store(0); u.stop.store(0);
        u.start();
    }
    h->seq_rgb = rgb; h->seq_depth = depth; h->seq_pixmask = pixmasks; h->seq_next = 0; h->seq_n = n; h->seq_on_device = on_device; h->seq_upload = ahead;
    h->seq_batches = 0; h->seq_launches = 0;
    h->seq_t0_us = now_us();
    for (int k = 0; k < n && !rc; k++) {
        while (!rc && h->seq_next < n && !h->ctx[h->open_ctx].launched) {       // fill the pipeline (later refills happen inside do_fuse)
            TimerScope ts(h);
            rc = seq_submit(h);
            // (Measured and removed, round 3: a head start of 150-450 us for the first, small batch before the larger ones join it
            // on the GPU.  Its frame is through at 0.6-0.7 ms instead of 0.83, but the 20-frame sequence takes 3.2-3.5 ms
            // instead of 3.07: the fill is bound by the extract work of the first 14 frames, not by its order -- profiles/fill_r03.txt.)
        }
        h->seq_k = k;
        if (!rc) rc = process_oldest(h, nullptr, out ? &out[k] : nullptr);
        if (k < 64) h->seq_done_us[k] = h->seq_mark_us[3][k] = now_us() - h->seq_t0_us;
        if (ahead) h->up->processed.store(k + 1, std::memory_order_release);
    }
    if (ahead) {
        h->up->stop.store(1);
        h->up->join();
    }
    h->seq_rgb = nullptr; h->seq_depth = nullptr; h->seq_pixmask = nullptr; h->seq_n = 0; h->seq_next = 0; h->seq_upload = false;
    if (h->up) h->up->masks = nullptr;
    return rc;
}
int ssf_process_sequence(ssf_handle* h, const void* const* rgb, const void* const* depth, int n, int on_device, ssf_frame_result* out) {
    return process_sequence_impl(h, rgb, depth, nullptr, n, on_device, out);
}
int ssf_pending_frames(const ssf_handle* h) { return h ? (int)h->pending.size() : 0; }
int ssf_pipeline_capacity(const ssf_handle* h) { return h ? (int)h->ctx.size() * h->batch : 0; }
int ssf_can_submit(const ssf_handle* h) { return (h && !h->ctx[h->open_ctx].launched) ? 1 : 0; }

// ---- loop-closure registration + fern codes -------------------------------------
int ssf_align(ssf_handle* h, const ssf_surfels* src, int n, const float* init_pose, float* rel_pose, int* valid, int* iters,
              int* pairs_last) {
    if (!h || !src || n < 0 || !rel_pose || !valid || !src->positions || !src->colors || !src->orientations) return SSF_ERR_INVALID_ARG;
    TimerScope ts(h);
    // sources: positions, Lab of the colours (same inline function as the kernels), normals = rows[2]
    const size_t N = (size_t)std::max(n, 1);
    std::vector<float> lab(3 * N), nrm(3 * N);
    for (int i = 0; i < n; i++) {
        const V3 l = rgb_to_lab(v3(src->colors[3 * i], src->colors[3 * i + 1], src->colors[3 * i + 2]));
        lab[3 * i] = l.x; lab[3 * i + 1] = l.y; lab[3 * i + 2] = l.z;
        for (int c = 0; c < 3; c++) nrm[3 * i + c] = src->orientations[9 * i + 6 + c];
    }
    float *d_pos = nullptr, *d_lab = nullptr, *d_nrm = nullptr, *d_conf = nullptr; long long* d_out = nullptr;
    DevTemps tmp;
    HCK(tmp.take(&d_pos, 12 * N)); HCK(tmp.take(&d_lab, 12 * N)); HCK(tmp.take(&d_nrm, 12 * N));
    HCK(tmp.take(&d_out, 40 * sizeof(long long)));
    if (src->confidences) HCK(tmp.take(&d_conf, 4 * N));
    hipStream_t st = h->stream;
    if (n > 0) {
        if (hipMemcpyAsync(d_pos, src->positions, 12 * (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(d_lab, lab.data(), 12 * (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(d_nrm, nrm.data(), 12 * (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess ||
            (d_conf && hipMemcpyAsync(d_conf, src->confidences, 4 * (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess)) {
            h->err = "upload of the source supersurfels failed"; return SSF_ERR_DEVICE;
        }
    }
    return align_loop(h, d_pos, d_lab, d_nrm, d_conf, n, d_out, init_pose, rel_pose, valid, iters, pairs_last);
}
int ssf_fern_codes(ssf_handle* h, const uint8_t* rgb, const float* depth, int width, int height, const uint32_t* fern_pos,
                   const uint8_t* fern_rgb, const float* fern_depth, int n, uint8_t* codes) {
    if (!h || !rgb || !depth || !fern_pos || !fern_rgb || !fern_depth || !codes || width <= 0 || height <= 0 || n < 0) return SSF_ERR_INVALID_ARG;
    if (n == 0) return SSF_OK;
    const size_t P = (size_t)width * height;
    uint8_t *d_rgb = nullptr, *d_frgb = nullptr, *d_codes = nullptr; float *d_depth = nullptr, *d_fd = nullptr; uint32_t* d_fp = nullptr;
    DevTemps tmp;
    HCK(tmp.take(&d_rgb, 3 * P)); HCK(tmp.take(&d_depth, 4 * P)); HCK(tmp.take(&d_fp, 8 * (size_t)n));
    HCK(tmp.take(&d_frgb, 3 * (size_t)n)); HCK(tmp.take(&d_fd, 4 * (size_t)n)); HCK(tmp.take(&d_codes, (size_t)n));
    hipStream_t st = h->stream;
    bool ok = hipMemcpyAsync(d_rgb, rgb, 3 * P, hipMemcpyHostToDevice, st) == hipSuccess &&
              hipMemcpyAsync(d_depth, depth, 4 * P, hipMemcpyHostToDevice, st) == hipSuccess &&
              hipMemcpyAsync(d_fp, fern_pos, 8 * (size_t)n, hipMemcpyHostToDevice, st) == hipSuccess &&
              hipMemcpyAsync(d_frgb, fern_rgb, 3 * (size_t)n, hipMemcpyHostToDevice, st) == hipSuccess &&
              hipMemcpyAsync(d_fd, fern_depth, 4 * (size_t)n, hipMemcpyHostToDevice, st) == hipSuccess;
    if (ok) {
        launch_fern_codes(st, d_rgb, d_depth, width, height, d_fp, d_frgb, d_fd, n, d_codes);
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(codes, d_codes, (size_t)n, hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipStreamSynchronize(st) == hipSuccess;
    }
    if (!ok) { h->err = "fern encoding failed on the device"; return SSF_ERR_DEVICE; }
    return SSF_OK;
}

int ssf_set_input_format(ssf_handle* h, int color, int depth, double depth_scale) {
    if (!h) return SSF_ERR_INVALID_ARG;
    if (color < SSF_COLOR_RGB8 || color > SSF_COLOR_BGRA8 || (depth != SSF_DEPTH_F32_METRES && depth != SSF_DEPTH_U16_SCALED)) {
        h->err = "ssf_set_input_format: unknown colour or depth format"; return SSF_ERR_INVALID_ARG;
    }
    if (depth == SSF_DEPTH_U16_SCALED && !(std::isfinite(depth_scale) && depth_scale > 0.0)) {
        h->err = "ssf_set_input_format: depth_scale must be finite and > 0"; return SSF_ERR_INVALID_ARG;
    }
    if (!h->pending.empty() || h->seq_n > 0) { h->err = "ssf_set_input_format: frames are pending in the extract pipeline"; return SSF_ERR_STATE; }
    h->in_color = color; h->in_depth = depth; h->in_scale = depth == SSF_DEPTH_U16_SCALED ? depth_scale : 1.0;
    return SSF_OK;
}
int ssf_get_input_format(const ssf_handle* h, int* color, int* depth, double* depth_scale) {
    if (!h) return SSF_ERR_INVALID_ARG;
    if (color) *color = h->in_color;
    if (depth) *depth = h->in_depth;
    if (depth_scale) *depth_scale = h->in_scale;
    return SSF_OK;
}

int ssf_stage_extract(ssf_handle* h, const void* rgb, const void* depth, int on_device, const uint8_t* mask) { return do_extract(h, rgb, depth, on_device, mask); }

// ---- pixel masks (ssf_dynamic.h) ----------------------------------------------------------------------
static int copy_map(ssf_handle* h, void* dst, const void* src, size_t bytes);
int ssf_process_frame_pixmask(ssf_handle* h, const void* rgb, const void* depth, int on_device, const float* prior, const uint8_t* pixel_mask,
                              ssf_frame_result* out) {
    return process_frame_impl(h, rgb, depth, on_device ? 1 : 0, prior, nullptr, out, pixel_mask);
}
int ssf_submit_frame_pixmask(ssf_handle* h, const void* rgb, const void* depth, int on_device, const uint8_t* pixel_mask) { return submit_frame(h, rgb, depth, on_device ? 1 : 0, nullptr, pixel_mask); }
int ssf_process_sequence_pixmask(ssf_handle* h, const void* const* rgb, const void* const* depth, const uint8_t* const* pixel_masks, int n,
                                 int on_device, ssf_frame_result* out) {
    return process_sequence_impl(h, rgb, depth, pixel_masks, n, on_device ? 1 : 0, out);
}
int ssf_stage_extract_pixmask(ssf_handle* h, const void* rgb, const void* depth, int on_device, const uint8_t* pixel_mask) { return do_extract(h, rgb, depth, on_device ? 1 : 0, nullptr, pixel_mask); }
// the vote of the current frame, recomputed on the host from the counts k_finalize_surfels<true> voted on (same integer rule)
int ssf_get_dynamic_superpixels(ssf_handle* h, uint8_t* out, int* n_dynamic) {
    if (!h || !out) return SSF_ERR_INVALID_ARG;
    const ActiveFrame& a = *h->cc;
    const size_t S = (size_t)h->S;
    int n = 0;
    if (a.pixmask && a.ctx) {
        std::vector<uint32_t> cnt(2 * S);
        const int rc = copy_map(h, cnt.data(), slab_shift(a.ctx->d_pixcnt, (size_t)a.slot * a.ctx->maps.slab), 2 * S * sizeof(uint32_t));
        if (rc) return rc;
        for (size_t k = 0; k < S; k++) {
            const uint32_t total = cnt[2 * k], masked = cnt[2 * k + 1];
            out[k] = (masked > 0u && 2ull * masked >= (unsigned long long)total) ? 1 : 0;
            n += out[k];
        }
    } else std::memset(out, 0, S);
    if (n_dynamic) *n_dynamic = n;
    return SSF_OK;
}
// test hook: compact / recentre the out-of-view store now (normally done when its span runs out of room or holes pile up)
int ssf_debug_recentre(ssf_handle* h) {
    if (!h) return SSF_ERR_INVALID_ARG;
    if (!h->pending.empty()) return SSF_ERR_STATE;
    return oov_recentre(h);
}
long long ssf_debug_recentre_count(const ssf_handle* h) { return h ? h->n_recentres : -1; }
int ssf_debug_set_max_passes(ssf_handle* h, int n) { if (!h) return SSF_ERR_INVALID_ARG; h->max_passes = n; return SSF_OK; }
// visible rows from which a frame's tracking streams a tile-sorted copy of them (default: SSF_BIN_MIN_ROWS_DEFAULT, 400 000; 0: always; < 0: never)
int ssf_debug_set_bin_min_rows(ssf_handle* h, int n) {
    if (!h) return SSF_ERR_INVALID_ARG;
    h->bins.min_rows = bin_buffer_words(h->cam, 1) == 0 ? -1 : n;
    return SSF_OK;
}
// test read-out: the sort itself.  launch_bin_rows over the visible array under the transform T12 (R row-major, then t) into the
// copy's own buffers, then to the host: the 48-byte records, the bin totals (the first nbins words of `cursor`) and the stored Lab
// stream of the visible rows in array order (no other read-out returns its bits).  The copy stays invalid: no frame streams it.
int ssf_debug_tile_copy(ssf_handle* h, const float* T12, float* records, uint32_t* totals, float* lab_src) {
    if (!h || !T12 || !records || !totals) return SSF_ERR_INVALID_ARG;
    if (!h->pending.empty()) { h->err = "frames are pending in the extract pipeline"; return SSF_ERR_STATE; }
    if (!single_shard_alone(h)) { h->err = "the tile-sorted copy is made on a single shard only"; return SSF_ERR_STATE; }
    const size_t nbins = bin_buffer_words(h->cam, 0);          // (no rows: the bin totals alone)
    if (bin_buffer_words(h->cam, 1) == 0) { h->err = "the frame is too fine for the tile-sorted copy"; return SSF_ERR_STATE; }
    const size_t n = (size_t)h->n_visible;
    if (n == 0) { std::memset(totals, 0, nbins * sizeof(uint32_t)); return SSF_OK; }
    { const int rc = tile_copy_buffers(h, h->bins); if (rc) return rc; }
    h->bins.drop();
    Rt T; T.R = m3(v3(T12[0], T12[1], T12[2]), v3(T12[3], T12[4], T12[5]), v3(T12[6], T12[7], T12[8])); T.t = v3(T12[9], T12[10], T12[11]);
    const SurfelSoA& M = h->model[h->mcur];
    launch_bin_rows(h->stream, h->cam, M, (int)n, T, h->bins.d_count, h->bins.d_cursor, h->bins.rows);
    HCK(hipGetLastError());
    HCK(hipMemcpyAsync(records, h->bins.rows.pos, 48 * n, hipMemcpyDeviceToHost, h->stream));
    HCK(hipMemcpyAsync(totals, h->bins.d_cursor, nbins * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (lab_src) HCK(hipMemcpyAsync(lab_src, M.lab, 12 * n, hipMemcpyDeviceToHost, h->stream));
    HCK(hipStreamSynchronize(h->stream));
    return SSF_OK;
}
// frames whose tracking made the tile-sorted copy since the handle was created
long long ssf_tile_copy_frames(ssf_handle* h) { return h ? h->bins.frames : -1; }
// visible rows up to which a frame's ICP loop and association run in ONE resident launch (default and ceiling: 262 144, every
// workgroup of it must hold a place at once; 0: never)
int ssf_debug_set_resident_icp_max_rows(ssf_handle* h, int n) {
    if (!h) return SSF_ERR_INVALID_ARG;
    h->resident_max_rows = h->go_res ? std::max(0, std::min(n, 256 * icp_resident_max_wgs())) : 0;
    return SSF_OK;
}
int ssf_stage_set_shard(ssf_handle* h, int64_t off, int64_t gm, int64_t gv) {
    if (!h) return SSF_ERR_INVALID_ARG;
    h->id_offset = off; h->global_n_model = gm; h->global_n_visible = gv; return SSF_OK;
}
int ssf_stage_icp_begin(ssf_handle* h, const float* prior) {
    if (!h || !h->have_frame) return SSF_ERR_STATE;
    icp_begin(h, prior); return SSF_OK;
}
int ssf_stage_icp_accumulate(ssf_handle* h, int64_t* sums) {
    if (!h || !sums) return SSF_ERR_INVALID_ARG;
    TimerScope ts(h);
    int rc = icp_accumulate(h, true);
    if (rc) return rc;
    std::memcpy(sums, h->h_icp, SSF_ICP_RECORD * sizeof(int64_t));
    return SSF_OK;
}
int ssf_stage_icp_update(ssf_handle* h, const int64_t* sums, int* again) {
    if (!h || !sums || !again) return SSF_ERR_INVALID_ARG;
    icp_update(h, sums, again); return SSF_OK;
}
int ssf_stage_icp_end(ssf_handle* h, int* valid) {
    if (!h || !valid) return SSF_ERR_INVALID_ARG;
    icp_end(h, valid); return SSF_OK;
}
// the association of the current frame, run and copied out: to the host (and waited for) or to device tables (enqueued only)
static int stage_match(ssf_handle* h, uint64_t* best, uint8_t* matched, hipMemcpyKind kind) {
    if (!h || !best || !matched) return SSF_ERR_INVALID_ARG;
    if (!h->have_frame) return SSF_ERR_STATE;
    TimerScope ts(h);
    int rc = do_match(h);
    if (rc) return rc;
    HCK(hipMemcpyAsync(best, h->cc->d_best, (size_t)h->S * 8, kind, h->stream));
    HCK(hipMemcpyAsync(matched, h->cc->d_matched, (size_t)h->S, kind, h->stream));
    if (kind == hipMemcpyDeviceToHost) HCK(hipStreamSynchronize(h->stream));
    return SSF_OK;
}
int ssf_stage_match(ssf_handle* h, uint64_t* best, uint8_t* matched) { return stage_match(h, best, matched, hipMemcpyDeviceToHost); }
int ssf_stage_begin_submitted(ssf_handle* h) {
    if (!h) return SSF_ERR_INVALID_ARG;
    return activate_oldest(h);
}
int ssf_stage_icp_accumulate_device(ssf_handle* h, int64_t* d_sums) {
    if (!h || !d_sums) return SSF_ERR_INVALID_ARG;
    if (!h->have_frame) return SSF_ERR_STATE;
    TimerScope ts(h);
    return icp_accumulate(h, false, (long long*)d_sums);
}
int ssf_stage_icp_fetch(ssf_handle* h, const int64_t* d_sums, int64_t* sums) {
    if (!h || !d_sums || !sums) return SSF_ERR_INVALID_ARG;
    const unsigned long long seq = ++h->icp_seq;
    launch_publish_icp(h->stream, (const long long*)d_sums, h->mb_dev, seq);
    HCK(hipGetLastError());
    int rc = icp_fetch(h, seq);
    if (rc) return rc;
    std::memcpy(sums, h->h_icp, SSF_ICP_RECORD * sizeof(int64_t));
    return SSF_OK;
}
int ssf_stage_match_device(ssf_handle* h, uint64_t* d_best, uint8_t* d_matched) { return stage_match(h, d_best, d_matched, hipMemcpyDeviceToDevice); }
// the caller's association tables -> the current frame's (enqueued on the track stream)
static int assoc_in(ssf_handle* h, const uint64_t* best, const uint8_t* matched, hipMemcpyKind kind) {
    HCK(hipMemcpyAsync(h->cc->d_best, best, (size_t)h->S * 8, kind, h->stream));
    HCK(hipMemcpyAsync(h->cc->d_matched, matched, (size_t)h->S, kind, h->stream));
    return SSF_OK;
}
// this shard's migrant table -> the caller's (zeros when the frame migrates nothing); a host table is waited for
static int migrants_out(ssf_handle* h, int32_t* table, hipMemcpyKind kind) {
    const size_t bytes = (size_t)SSF_MIGRANT_WORDS * h->S * 4;
    const bool host = kind == hipMemcpyDeviceToHost;
    hipError_t e = hipSuccess;
    if (h->fuse_migrate) { e = hipMemcpyAsync(table, h->d_migrants, bytes, kind, h->stream); if (host && e == hipSuccess) e = hipStreamSynchronize(h->stream); }
    else if (host) std::memset(table, 0, bytes);
    else e = hipMemsetAsync(table, 0, bytes, h->stream);
    if (e != hipSuccess) { h->fusing = false; h->err = std::string("migrant table copy: ") + hipGetErrorString(e); return SSF_ERR_DEVICE; }
    return SSF_OK;
}
static int stage_fuse(ssf_handle* h, const uint64_t* best, const uint8_t* matched, ssf_frame_result* out, hipMemcpyKind in) {
    if (!h || !best || !matched) return SSF_ERR_INVALID_ARG;
    if (!h->have_frame || h->fusing) return SSF_ERR_STATE;
    TimerScope ts(h);
    int rc = assoc_in(h, best, matched, in);
    return rc ? rc : do_fuse(h, out);
}
static int stage_fuse_begin(ssf_handle* h, const uint64_t* best, const uint8_t* matched, int32_t* table, hipMemcpyKind in, hipMemcpyKind out) {
    if (!h || !best || !matched || !table) return SSF_ERR_INVALID_ARG;
    if (!h->have_frame || h->fusing) return SSF_ERR_STATE;
    TimerScope ts(h);
    int rc = assoc_in(h, best, matched, in);
    if (!rc) rc = fuse_begin(h, 1);
    return rc ? rc : migrants_out(h, table, out);
}
int ssf_stage_fuse_device(ssf_handle* h, const uint64_t* d_best, const uint8_t* d_matched, ssf_frame_result* out) { return stage_fuse(h, d_best, d_matched, out, hipMemcpyDeviceToDevice); }
int ssf_stage_fuse_begin_device(ssf_handle* h, const uint64_t* d_best, const uint8_t* d_matched, int32_t* d_table) { return stage_fuse_begin(h, d_best, d_matched, d_table, hipMemcpyDeviceToDevice, hipMemcpyDeviceToDevice); }
int ssf_stage_fuse_end_device(ssf_handle* h, const int32_t* d_table, ssf_frame_result* out) {
    if (!h) return SSF_ERR_INVALID_ARG;
    if (!h->fusing) return SSF_ERR_STATE;
    TimerScope ts(h);
    return fuse_end(h, d_table, out);
}
int ssf_stage_fuse_begin(ssf_handle* h, const uint64_t* best, const uint8_t* matched, int32_t* table) { return stage_fuse_begin(h, best, matched, table, hipMemcpyHostToDevice, hipMemcpyDeviceToHost); }
int ssf_stage_fuse_end(ssf_handle* h, const int32_t* table, ssf_frame_result* out) {
    if (!h) return SSF_ERR_INVALID_ARG;
    if (!h->fusing) return SSF_ERR_STATE;
    TimerScope ts(h);
    if (table && h->fuse_migrate) HCK(hipMemcpyAsync(h->d_migrants, table, (size_t)SSF_MIGRANT_WORDS * h->S * 4, hipMemcpyHostToDevice, h->stream));
    return fuse_end(h, (table && h->fuse_migrate) ? h->d_migrants : nullptr, out);
}
int ssf_stage_fuse(ssf_handle* h, const uint64_t* best, const uint8_t* matched, ssf_frame_result* out) { return stage_fuse(h, best, matched, out, hipMemcpyHostToDevice); }

int ssf_get_pose(const ssf_handle* h, float* p) { if (!h || !p) return SSF_ERR_INVALID_ARG; pose_to12(h->pose, p); return SSF_OK; }
int ssf_set_pose(ssf_handle* h, const float* p) { if (!h || !p) return SSF_ERR_INVALID_ARG; h->pose = pose_from12(p); return SSF_OK; }
int ssf_get_counts(const ssf_handle* h, int* nm, int* nv, int* st, int* ns) {
    if (!h) return SSF_ERR_INVALID_ARG;
    if (nm) *nm = h->n_model;
    if (nv) *nv = h->n_visible;
    if (st) *st = h->stamp;
    if (ns) *ns = h->S;
    return SSF_OK;
}

// orientations: 9 floats per row at the ABI (3 x 3, row-major), the three matrix rows as three streams of 3 n floats in the stores
static void orient_to_streams(const float* o9, float* rows, size_t n) {
    for (size_t i = 0; i < n; i++)
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) rows[(size_t)r * 3 * n + 3 * i + c] = o9[9 * i + 3 * r + c];
}
static void orient_from_streams(const float* rows, float* o9, size_t n) {
    for (size_t i = 0; i < n; i++)
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) o9[9 * i + 3 * r + c] = rows[(size_t)r * 3 * n + 3 * i + c];
}
static int copy_out(ssf_handle* h, const SurfelSoA& s, int first, int count, ssf_surfels* o) {
    if (count <= 0) return SSF_OK;
    const size_t n = count, f = first;
    hipStream_t st = h->stream;
    ssf_surfels flat = *o; flat.orientations = nullptr;
    { int rc = copy_rows(h, flat, 0, soa_surfels(s), f, n, hipMemcpyDeviceToHost); if (rc) return rc; }
    std::vector<float> rows;
    if (o->orientations) {
        rows.resize(9 * n);
        HCK(hipMemcpyAsync(rows.data(), s.r0 + 3 * f, 12 * n, hipMemcpyDeviceToHost, st));
        HCK(hipMemcpyAsync(rows.data() + 3 * n, s.r1 + 3 * f, 12 * n, hipMemcpyDeviceToHost, st));
        HCK(hipMemcpyAsync(rows.data() + 6 * n, s.r2 + 3 * f, 12 * n, hipMemcpyDeviceToHost, st));
    }
    HCK(hipStreamSynchronize(st));
    if (o->orientations) orient_from_streams(rows.data(), o->orientations, n);
    return SSF_OK;
}
int ssf_get_model(ssf_handle* h, int first, int count, ssf_surfels* o) {
    if (!h || !o || first < 0 || count < 0 || first + count > h->cfg.nb_supersurfels_max) return SSF_ERR_INVALID_ARG;
    int rc = materialise(h);
    return rc ? rc : copy_out(h, h->dense, first, count, o);
}
int ssf_get_frame(ssf_handle* h, ssf_surfels* o) { if (!h || !o) return SSF_ERR_INVALID_ARG; return copy_out(h, h->cc->frame, 0, h->S, o); }
int ssf_set_model(ssf_handle* h, const ssf_surfels* in, int n, int n_visible, int stamp) {
    if (!h || !in || n < 0 || n > h->cfg.nb_supersurfels_max || n_visible < 0 || n_visible > n) return SSF_ERR_INVALID_ARG;
    if (!in->positions || !in->colors || !in->stamps || !in->orientations || !in->shapes || !in->dims || !in->confidences) return SSF_ERR_INVALID_ARG;
    if (!h->pending.empty()) { h->err = "frames are pending in the extract pipeline"; return SSF_ERR_STATE; }
    drop_shard_sizes(h);
    SurfelSoA& s = h->dense;                       // upload the logical order, then split it into the two stores
    hipStream_t st = h->stream;
    const size_t N = n;
    if (n > 0) {
        std::vector<float> rows(9 * N);
        orient_to_streams(in->orientations, rows.data(), N);
        { int rc = copy_rows(h, soa_surfels(s), 0, *in, 0, N, hipMemcpyHostToDevice); if (rc) return rc; }
        HCK(hipMemcpyAsync(s.r0, rows.data(), 12 * N, hipMemcpyHostToDevice, st));
        HCK(hipMemcpyAsync(s.r1, rows.data() + 3 * N, 12 * N, hipMemcpyHostToDevice, st));
        HCK(hipMemcpyAsync(s.r2, rows.data() + 6 * N, 12 * N, hipMemcpyHostToDevice, st));
        launch_lab_refresh(st, s, n);
        HCK(hipStreamSynchronize(st));
    }
    h->stamp = stamp;
    return store_from_dense(h, n, n_visible);
}
static int copy_map(ssf_handle* h, void* dst, const void* src, size_t bytes) {
    HCK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HCK(hipStreamSynchronize(h->stream));
    return SSF_OK;
}
int ssf_get_index_map(ssf_handle* h, int32_t* o) { if (!h || !o) return SSF_ERR_INVALID_ARG; return copy_map(h, o, h->cc->maps.label, (size_t)h->cfg.width * h->cfg.height * 4); }
int ssf_get_boundary_map(ssf_handle* h, int32_t* o) {
    if (!h || !o) return SSF_ERR_INVALID_ARG;
    launch_boundary_map(h->stream, h->seg, h->cc->maps.label, h->d_scratch_map);
    return copy_map(h, o, h->d_scratch_map, (size_t)h->cfg.width * h->cfg.height * 4);
}
int ssf_get_inlier_map(ssf_handle* h, uint8_t* o) { if (!h || !o) return SSF_ERR_INVALID_ARG; return copy_map(h, o, h->cc->maps.inlier, (size_t)h->cfg.width * h->cfg.height); }
int ssf_get_plane_depth(ssf_handle* h, float* o) { if (!h || !o) return SSF_ERR_INVALID_ARG; return copy_map(h, o, h->cc->maps.plane_depth, (size_t)h->cfg.width * h->cfg.height * 4); }
int ssf_get_superpixels(ssf_handle* h, float* o) {
    if (!h || !o) return SSF_ERR_INVALID_ARG;
    std::vector<SpRow> rows(h->S);
    int rc = copy_map(h, rows.data(), h->cc->maps.sp, (size_t)h->S * sizeof(SpRow));
    if (rc) return rc;
    for (int k = 0; k < h->S; k++) {
        const SpRow& r = rows[k];
        const float v[9] = {r.cx, r.cy, r.r, r.g, r.b, r.ta, r.tb, r.tc, r.size};
        std::memcpy(&o[9 * k], v, sizeof(v));
    }
    return SSF_OK;
}
int ssf_get_model_device(ssf_handle* h, ssf_surfels* o, int* n) {
    if (!h || !o) return SSF_ERR_INVALID_ARG;
    if (!h->d_orient9 && !dalloc(h, &h->d_orient9, 9 * (size_t)h->cfg.nb_supersurfels_max)) { h->err = "allocation failed"; return SSF_ERR_DEVICE; }
    { int rc = materialise(h); if (rc) return rc; }
    const SurfelSoA& s = h->dense;                 // a dense copy: [visible | out-of-view], valid until the next call
    launch_pack_orient(h->stream, s, h->n_model, h->d_orient9);
    HCK(hipGetLastError());
    HCK(hipStreamSynchronize(h->stream));
    *o = soa_surfels(s); o->orientations = h->d_orient9;
    if (n) *n = h->n_model;
    return SSF_OK;
}

int ssf_get_frame_device(ssf_handle* h, ssf_surfels* o, int* n) {
    if (!h || !o) return SSF_ERR_INVALID_ARG;
    if (!h->cc || !h->cc->frame.pos) { h->err = "no frame has been processed yet"; return SSF_ERR_STATE; }
    if (!h->d_frame_orient9 && !dalloc(h, &h->d_frame_orient9, 9 * (size_t)h->S)) { h->err = "allocation failed"; return SSF_ERR_DEVICE; }
    const SurfelSoA& s = h->cc->frame;
    launch_pack_orient(h->stream, s, h->S, h->d_frame_orient9);
    HCK(hipGetLastError());
    HCK(hipStreamSynchronize(h->stream));
    *o = soa_surfels(s); o->orientations = h->d_frame_orient9;
    if (n) *n = h->S;
    return SSF_OK;
}
int ssf_get_preview_image(ssf_handle* h, uint8_t* o) {
    if (!h || !o) return SSF_ERR_INVALID_ARG;
    const size_t P = (size_t)h->cfg.width * h->cfg.height;
    uint8_t* d = reinterpret_cast<uint8_t*>(h->d_scratch_map);      // P x int32 of scratch: 3P bytes fit
    launch_preview(h->stream, h->cfg.width, h->cfg.height, h->cc->maps.label, h->cc->maps.rgba, d);
    HCK(hipGetLastError());
    return copy_map(h, o, d, 3 * P);
}

// exportModel, supersurfel_fusion.cu:595-633 (std::to_string == "%f"/"%d")
int ssf_export_model_txt(ssf_handle* h, const char* path) {
    if (!h || !path) return SSF_ERR_INVALID_ARG;
    const int n = h->n_model;
    std::vector<float> pos(3 * (size_t)n), col(3 * (size_t)n), ori(9 * (size_t)n), shp(6 * (size_t)n), dims(2 * (size_t)n), conf(n);
    std::vector<int32_t> stamps(2 * (size_t)n);
    ssf_surfels o = {pos.data(), col.data(), stamps.data(), ori.data(), shp.data(), dims.data(), conf.data()};
    int rc = materialise(h);
    if (!rc) rc = copy_out(h, h->dense, 0, n, &o);
    if (rc) return rc;
    FILE* f = std::fopen(path, "w");
    if (!f) { h->err = "cannot open file"; return SSF_ERR_IO; }
    for (int i = 0; i < n; i++) {
        if (!(conf[i] > h->cfg.conf_thresh)) continue;
        std::fprintf(f, "%d %d %f\n", stamps[2 * i], stamps[2 * i + 1], conf[i]);
        std::fprintf(f, "%f %f %f\n", pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
        std::fprintf(f, "%f %f %f\n", col[3 * i], col[3 * i + 1], col[3 * i + 2]);
        std::fprintf(f, "%f %f\n", dims[2 * i], dims[2 * i + 1]);
        const float* q = &ori[9 * (size_t)i];
        std::fprintf(f, "%f %f %f %f %f %f %f %f %f\n", q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]);
        const float* c = &shp[6 * (size_t)i];
        std::fprintf(f, "%f %f %f %f %f %f\n\n", c[0], c[1], c[2], c[3], c[4], c[5]);
    }
    std::fclose(f);
    return SSF_OK;
}

int ssf_apply_deformation(ssf_handle* h, const float* np, const float* nr, const float* nt, int m, const float* w4, const int32_t* idx4) {
    if (!h || !np || !nr || !nt || !w4 || !idx4 || m <= 0) return SSF_ERR_INVALID_ARG;
    drop_shard_sizes(h);
    h->ahead.valid = false;
    const size_t n = h->n_model;
    if (n == 0) return SSF_OK;
    float *d_np, *d_nr, *d_nt, *d_w, *d_nodes; int32_t* d_i;
    DevTemps tmp;
    HCK(tmp.take(&d_np, 12 * (size_t)m)); HCK(tmp.take(&d_nr, 36 * (size_t)m)); HCK(tmp.take(&d_nt, 12 * (size_t)m));
    HCK(tmp.take(&d_nodes, 64 * (size_t)m));
    HCK(tmp.take(&d_w, 16 * n)); HCK(tmp.take(&d_i, 16 * n));
    hipStream_t st = h->stream;
    HCK(hipMemcpyAsync(d_np, np, 12 * (size_t)m, hipMemcpyHostToDevice, st));
    HCK(hipMemcpyAsync(d_nr, nr, 36 * (size_t)m, hipMemcpyHostToDevice, st));
    HCK(hipMemcpyAsync(d_nt, nt, 12 * (size_t)m, hipMemcpyHostToDevice, st));
    HCK(hipMemcpyAsync(d_w, w4, 16 * n, hipMemcpyHostToDevice, st));
    HCK(hipMemcpyAsync(d_i, idx4, 16 * n, hipMemcpyHostToDevice, st));
    return deform_dense(h, m, d_np, d_nr, d_nt, d_nodes, d_w, d_i);
}

int ssf_bilateral_filter(ssf_handle* h, const void* in, void* out, int on_device) {
    if (!h || !in || !out) return SSF_ERR_INVALID_ARG;
    const size_t P = (size_t)h->cfg.width * h->cfg.height;
    const void* d_in = in; float* d_out = (float*)out;
    if (on_device && (!device_input_aligned(h, nullptr, in) || (uintptr_t)out % 4)) return SSF_ERR_INVALID_ARG;
    // (input in the handle's depth format, ssf_input.h: h->d_bf_in holds P floats, room for either; the output is float metres)
    if (!on_device) { HCK(hipMemcpyAsync(h->d_bf_in, in, depth_bpp(h) * P, hipMemcpyHostToDevice, h->stream)); d_in = h->d_bf_in; d_out = h->d_bf_out; }
    { TimerScope ts(h); launch_bilateral(h->stream, d_in, h->in_depth, h->in_scale, d_out, h->cfg.width, h->cfg.height, h->cfg.prefilter_sigma_color, h->cfg.prefilter_sigma_space); }
    if (!on_device) HCK(hipMemcpyAsync(out, d_out, 4 * P, hipMemcpyDeviceToHost, h->stream));
    HCK(hipStreamSynchronize(h->stream));
    if (h->cfg.profile == 1) timer_collect(&h->timer);
    return SSF_OK;
}
int ssf_get_kernel_times(ssf_handle* h, const char** names, double* ms, int64_t* calls, int max_k) {
    if (!h || !names || !ms || !calls) return 0;
    h->timer_names.clear();
    for (auto& kv : h->timer.acc) h->timer_names.push_back(kv.first);
    int k = 0;
    for (auto& nm : h->timer_names) {
        if (k >= max_k) break;
        names[k] = nm.c_str(); ms[k] = h->timer.acc[nm].first; calls[k] = h->timer.acc[nm].second; k++;
    }
    return k;
}
int ssf_reset_kernel_times(ssf_handle* h) { if (!h) return SSF_ERR_INVALID_ARG; h->timer.acc.clear(); return SSF_OK; }
int ssf_set_profile(ssf_handle* h, int enable) {
    if (!h) return SSF_ERR_INVALID_ARG;
    h->cfg.profile = enable;
    if (enable == 1) timer_calibrate(&h->timer, h->stream);
    return SSF_OK;
}

// per frame of the last sequence (first 64): entry of the track loop, first ICP record back, ICP loop done, counters
// back [us from the call's entry]; then 32 x (time, frames) of the extract batches launched
int ssf_sequence_marks(ssf_handle* h, double* out320) {
    if (!h || !out320) return SSF_ERR_INVALID_ARG;
    for (int m = 0; m < 4; m++) for (int i = 0; i < 64; i++) out320[m * 64 + i] = h->seq_mark_us[m][i];
    for (int i = 0; i < 32; i++) { out320[256 + 2 * i] = i < h->seq_launches ? h->seq_launch_us[i] : -1.0; out320[257 + 2 * i] = i < h->seq_launches ? h->seq_launch_n[i] + h->seq_launch_host_us[i] / 1e4 : 0; }
    return SSF_OK;
}
// frames whose association ran inside a waiting ICP launch (SSF_ICP_GO_MATCH) since the handle was created
long long ssf_waiter_matches(ssf_handle* h) { return h ? h->n_waiter_matches : -1; }
// frames whose ICP iterations ran in one resident launch (launch_icp_resident)
long long ssf_resident_icp_frames(ssf_handle* h) { return h ? h->n_resident_frames : -1; }
// ... and those of them whose launch started at its second word: the first record had been made by the frame before (k_move_rows<true>)
long long ssf_resident_icp_ahead_frames(ssf_handle* h) { return h ? h->n_resident_ahead_frames : -1; }
// the self-tuned choice of AheadTuner: [0] form in effect (1: first ICP iteration inside the row-move kernel), [1] pipelined frames
// seen, [2] / [3] mean chain period per unit of work measured in the last probe without / with the fusion (0: not probed yet)
int ssf_tuner_state(ssf_handle* h, double* out4) {
    if (!h || !out4) return SSF_ERR_INVALID_ARG;
    const AheadTuner& t = h->ahead_tuner;
    out4[0] = t.current(); out4[1] = t.frames; out4[2] = t.n[0] ? t.sum[0] / t.n[0] : 0.0; out4[3] = t.n[1] ? t.sum[1] / t.n[1] : 0.0;
    return SSF_OK;
}
// ... and the frames whose association was run again as a launch of its own because the host's word to the waiting launch came
// too late to be trusted
long long ssf_waiter_match_repairs(ssf_handle* h) { return h ? h->n_waiter_match_repairs : -1; }
// completion times (us since the call started) of the first 64 frames of the last ssf_process_sequence (tools/startup_probe.py)
int ssf_sequence_times(ssf_handle* h, double* out64) {
    if (!h || !out64) return SSF_ERR_INVALID_ARG;
    for (int i = 0; i < 64; i++) out64[i] = h->seq_done_us[i];
    return SSF_OK;
}

// What a stream copy reaches on THIS box (nominal AND measured-achievable peak): 16 bytes per lane, `mib` MiB
// read + the same written, best of `reps` over four forms of the same copy -- MI355X_MICROARCH.md quotes 6.29 TB/s (79 % of the
// 8 TB/s spec) for a float4 copy; round 4's single grid-stride form reached 4.7-4.8 TB/s on these boxes and torch's own copy kernel
// 5.2, neither tuned.  Forms: U independent 16-byte loads per lane in flight before the first store (4 or 8), plain or
// non-temporal (`nt`: streamed data is not kept in L2 / MALL, which a copy of 2 GiB only thrashes), grid-stride over 8192
// workgroups or one pass of exactly-sized workgroups.  The best form's rate is returned.
double ssf_stream_copy_rate(int mib, int reps) {
    // Every form moves WHOLE rounds: the grid-stride forms cover U x 2^21 threads x 16 B = 128 MiB (U = 4) or 256 MiB (U = 8) per
    // round of their loop and their first round is unguarded (k_stream_copy), so the buffers are a multiple of 256 MiB and sizes
    // below that are refused -- a smaller buffer would be overrun, a ragged one credited with bytes it did not move.
    if (mib < 256 || reps < 1) return -1.0;
    const size_t bytes = ((size_t)mib << 20) & ~(size_t)((1u << 28) - 1u), n = bytes / sizeof(f4v);
    if (bytes == 0) return -1.0;
    f4v *a = nullptr, *b = nullptr;
    if (hipMalloc(&a, bytes) != hipSuccess || hipMalloc(&b, bytes) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(a); return -1.0; }
    (void)hipMemset(a, 1, bytes); (void)hipMemset(b, 0, bytes);
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    double best = 0.0;
    for (int form = 0; form < 6; form++) {
        for (int r = 0; r < reps + 2; r++) {
            (void)hipEventRecord(e0, 0);
            const dim3 grid_stride(256 * 32), blk(256);
            switch (form) {
                case 0: hipLaunchKernelGGL((k_stream_copy<4, false, false>), grid_stride, blk, 0, 0, a, b, n); break;
                case 1: hipLaunchKernelGGL((k_stream_copy<4, true, false>), grid_stride, blk, 0, 0, a, b, n); break;
                case 2: hipLaunchKernelGGL((k_stream_copy<8, true, false>), grid_stride, blk, 0, 0, a, b, n); break;
                case 3: hipLaunchKernelGGL((k_stream_copy<4, true, true>), dim3((unsigned int)(n / (256 * 4))), blk, 0, 0, a, b, n); break;
                case 4: hipLaunchKernelGGL((k_stream_copy<8, true, true>), dim3((unsigned int)(n / (256 * 8))), blk, 0, 0, a, b, n); break;
                default: hipLaunchKernelGGL((k_stream_copy<8, false, true>), dim3((unsigned int)(n / (256 * 8))), blk, 0, 0, a, b, n); break;
            }
            (void)hipEventRecord(e1, 0);
            (void)hipEventSynchronize(e1);
            float ms = 0.f; (void)hipEventElapsedTime(&ms, e0, e1);
            if (r >= 2 && ms > 0.f) best = std::max(best, 2.0 * (double)bytes / (ms * 1e-3) / 1e9);
        }
    }
    (void)hipGetLastError();
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(a); (void)hipFree(b);
    return best;
}

// streams waiting in the process-wide pool for the next handle (StreamPool)
int ssf_pooled_streams(void) {
    StreamPool& sp = stream_pool();
    std::lock_guard<std::mutex> lk(sp.mu);
    int n = 0;
    for (auto& kv : sp.idle) n += (int)kv.second.size();
    return n;
}
// host frames of sequences: [0] workers, [1] frames uploaded, microseconds summed over the workers [2] waiting for a ring slot,
// [3] in the staging memcpy, [4] in the two hipMemcpyAsync calls, [5] the submitting thread's wait for uploads (tools/host_buffer_probe.py)
int ssf_upload_stats(ssf_handle* h, double* out6) {
    if (!h || !out6) return SSF_ERR_INVALID_ARG;
    for (int i = 0; i < 6; i++) out6[i] = 0.0;
    if (h->up) {
        out6[0] = Uploader::NTH; out6[1] = (double)h->up->frames_done.load(); out6[2] = (double)h->up->us_ring.load();
        out6[3] = (double)h->up->us_memcpy.load(); out6[4] = (double)h->up->us_enqueue.load();
    }
    out6[5] = h->us_wait_upload;
    return SSF_OK;
}
#ifdef SSF_EXPERIMENTS          // (laboratory build only: probes of tools/, not part of the product)
#include "lab/host_probes.inc"
#endif
}  // extern "C"
