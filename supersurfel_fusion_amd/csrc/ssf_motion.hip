// ssf_motion.hip -- moving objects from the incoming depth and the model depth (include/ssf_motion.h) on gfx950.
//
// What is computed is pinned, operation by operation, in include/ssf_motion.h (the numpy restatement: tests/motion_ref.py).  How:
//   * classify  k_motion_classify: one thread per pixel.  Reads the depth once, converting the input format where it loads it,
//               and the model depth; writes the class and the f32 depth the later phases read.  Seed and unknown pixels are
//               counted per workgroup (ballots), one 64-bit atomic each.
//   * label, merge, flatten (k_motion_roots, k_motion_flatten): the connected components of the members under the link rule of
//               step 3 with 4-connectivity, by the labeller of ssf_ccl.hpp: its scheme, its marks in parent and label between the
//               phases and the argument why it ends and loses no link are stated there.  What is motion's own: the link test on
//               the depths, and the counts.  k_motion_label counts the seed / unknown pixels per local component in LDS and
//               writes them to cnt at the local root, and nowhere else; in k_motion_roots a local root that is not the
//               component's root adds its counts to the root's (integer atomics: one pair per (tile, local component), never
//               one per pixel).
//   * decide    k_motion_decide: one thread per pixel: the component's counts at cnt[label[p]], the rule of step 5, the mask
//               byte; components (label[p] == p), dynamic components and masked pixels are counted per workgroup.
// The root of a set is its smallest index, so labels, counts and the mask do not depend on scheduling.  The phases are separate
// launches: no workgroup ever waits for another.  The host reads the five counts once, at the end.  Nothing here writes to the
// handle's stores, counters or scratch: the working set is MotionWs (ssf_handle.hpp); the model depth of ssf_motion_mask is drawn
// by ssf_render_model itself.
#include "ssf_ccl.hpp"
#include "ssf_handle.hpp"

namespace ssf {

enum { MT_W = 32, MT_H = 32, MT_P = MT_W * MT_H };              // the label tile; 256 threads, MT_P / 256 pixels each
static_assert(MT_W == CCL_TILE && MT_H == CCL_TILE, "the label tile is ssf_ccl.hpp's");
enum { MST_SEED = 0, MST_UNKNOWN, MST_COMP, MST_DYN, MST_MASKED, MST_WORDS };

struct MotionArgs {
    int W, H, ntx, nty;
    float rmin, rmax, front_abs, front_quad, link_abs, link_rel;
    int min_seeds, unknown_per_seed;
};

__device__ __forceinline__ bool motion_member(uint8_t c) { return c == SSF_MOTION_SEED || c == SSF_MOTION_UNKNOWN; }
// step 3 of include/ssf_motion.h (contraction off: one IEEE operation each, in this order); both depths are valid ones
__device__ __forceinline__ bool motion_linked(const MotionArgs& a, float dp, float dq) {
    return fabsf(dp - dq) <= a.link_abs + a.link_rel * fminf(dp, dq);
}
template <int DF> __device__ __forceinline__ float motion_load_depth(const void* __restrict__ p, size_t q, double scale) {
    if (DF == SSF_DEPTH_U16_SCALED) return (float)((double)reinterpret_cast<const uint16_t*>(p)[q] * scale);
    return reinterpret_cast<const float*>(p)[q];
}

// ---- classify: one thread per pixel --------------------------------------------------------------------------------------
template <int DF>
__global__ __launch_bounds__(256) void k_motion_classify(MotionArgs a, const void* __restrict__ depth, double scale,
                                                         const float* __restrict__ model, float* __restrict__ d32,
                                                         uint8_t* __restrict__ cls, unsigned long long* __restrict__ stats) {
    __shared__ int part_s[4], part_u[4];
    const size_t P = (size_t)a.W * a.H, p = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t c = SSF_MOTION_INVALID;
    if (p < P) {
        const float d = motion_load_depth<DF>(depth, p, scale), m = model[p];
        if (isfinite(d) && d >= a.rmin && d <= a.rmax) {
            const float tau = a.front_abs + a.front_quad * (d * d);
            c = (m > 0.0f && (m - d) > tau) ? SSF_MOTION_SEED : (m == 0.0f ? SSF_MOTION_UNKNOWN : SSF_MOTION_STATIC);
        }
        d32[p] = d; cls[p] = c;
    }
    const int ns = block_count256(c == SSF_MOTION_SEED, part_s), nu = block_count256(c == SSF_MOTION_UNKNOWN, part_u);
    if (threadIdx.x == 0 && ns) atomicAdd(&stats[MST_SEED], (unsigned long long)ns);
    if (threadIdx.x == 1 && nu) atomicAdd(&stats[MST_UNKNOWN], (unsigned long long)nu);
}

// ---- label: one workgroup per tile (ssf_ccl.hpp's tile body; the link test is motion_linked on the LDS depths) ---------------------
__global__ __launch_bounds__(256) void k_motion_label(MotionArgs a, const float* __restrict__ d32, const uint8_t* __restrict__ cls,
                                                      int32_t* __restrict__ parent, int32_t* __restrict__ label, uint2* __restrict__ cnt) {
    __shared__ float sd[MT_P];
    __shared__ int sp[MT_P];
    __shared__ uint32_t scs[MT_P], scu[MT_P];
    __shared__ uint8_t sc[MT_P];
    const int tx = blockIdx.x % a.ntx, ty = blockIdx.x / a.ntx, x0 = tx * MT_W, y0 = ty * MT_H;
#pragma unroll
    for (int k = 0; k < MT_P / 256; k++) {
        const int i = k * 256 + threadIdx.x, x = x0 + (i % MT_W), y = y0 + (i / MT_W);
        const bool in = x < a.W && y < a.H;
        const size_t p = (size_t)y * a.W + x;
        sc[i] = in ? cls[p] : (uint8_t)SSF_MOTION_INVALID;
        sd[i] = in ? d32[p] : 0.0f;
        scs[i] = 0u; scu[i] = 0u;
    }
    int root[MT_P / 256];
    ccl_tile_label(sp, false, [&](int i) { return motion_member(sc[i]); }, [&](int i, int j) { return motion_linked(a, sd[i], sd[j]); }, root);
#pragma unroll
    for (int k = 0; k < MT_P / 256; k++)
        if (root[k] >= 0) atomicAdd(sc[k * 256 + threadIdx.x] == SSF_MOTION_SEED ? &scs[root[k]] : &scu[root[k]], 1u);
    __syncthreads();
    ccl_tile_store(a.W, a.H, x0, y0, root, parent, label);
#pragma unroll
    for (int k = 0; k < MT_P / 256; k++) {                 // the counts, at the local roots only (members: inside the image)
        const int i = k * 256 + threadIdx.x;
        if (root[k] == i) cnt[ccl_image_index(a.W, x0, y0, i)] = make_uint2(scs[i], scu[i]);
    }
}

// ---- merge: one thread per pixel on the high side of a tile border, united with its neighbour across it ---------------------------
__global__ __launch_bounds__(256) void k_motion_merge(MotionArgs a, const float* __restrict__ d32, int32_t* parent) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= ccl_border_threads(a.W, a.H, a.ntx, a.nty)) return;
    ccl_merge(parent, a.W, a.H, a.ntx, t, false, [&](int p, int q) { return motion_linked(a, d32[p], d32[q]); });
}

// ---- flatten: the local roots walk to their root, then every other member takes its local root's label ----------------------
__global__ __launch_bounds__(256) void k_motion_roots(MotionArgs a, const int32_t* __restrict__ parent, int32_t* __restrict__ label,
                                                      uint2* __restrict__ cnt) {
    const size_t P = (size_t)a.W * a.H, p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P || !ccl_is_local_root(label, p)) return;
    const int i = ccl_walk(parent, (int)p);
    label[p] = i;
    // a local root that is not the component's root adds its counts to the root's (the root's own words only receive additions,
    // and the only thread that reads them here is the root's, which adds nothing)
    if (i != (int)p) {
        const uint2 c = cnt[p];
        if (c.x) atomicAdd(&cnt[i].x, c.x);
        if (c.y) atomicAdd(&cnt[i].y, c.y);
    }
}
__global__ __launch_bounds__(256) void k_motion_flatten(MotionArgs a, const int32_t* __restrict__ parent, int32_t* __restrict__ label) {
    const size_t P = (size_t)a.W * a.H, p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p < P) ccl_flatten(parent, label, p, label[p]);
}

// ---- decide: one thread per pixel ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_motion_decide(MotionArgs a, const int32_t* __restrict__ label, const uint2* __restrict__ cnt,
                                                       uint8_t* __restrict__ mask, unsigned long long* __restrict__ stats) {
    __shared__ int part_c[4], part_d[4], part_m[4];
    const size_t P = (size_t)a.W * a.H, p = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool dyn = false, is_root = false;
    if (p < P) {
        const int32_t r = label[p];
        if (r >= 0) {
            const uint2 c = cnt[r];
            dyn = c.x >= (uint32_t)a.min_seeds && (long long)c.y <= (long long)a.unknown_per_seed * (long long)c.x;
            is_root = r == (int32_t)p;
        }
        mask[p] = dyn ? 1 : 0;
    }
    const int nc = block_count256(is_root, part_c), nd = block_count256(is_root && dyn, part_d), nm = block_count256(dyn, part_m);
    if (threadIdx.x == 0 && nc) atomicAdd(&stats[MST_COMP], (unsigned long long)nc);
    if (threadIdx.x == 1 && nd) atomicAdd(&stats[MST_DYN], (unsigned long long)nd);
    if (threadIdx.x == 2 && nm) atomicAdd(&stats[MST_MASKED], (unsigned long long)nm);
}

// ---- launches -------------------------------------------------------------------------------------------------------
static void launch_motion_classify(hipStream_t st, const MotionArgs& a, const void* depth, int depth_format, double scale, const float* model,
                                   float* d32, uint8_t* cls, unsigned long long* stats) {
    ScopedKernel sk("motion_classify", st);
    const unsigned nb = (unsigned)(((size_t)a.W * a.H + 255) / 256);
    if (depth_format == SSF_DEPTH_U16_SCALED)
        hipLaunchKernelGGL(k_motion_classify<SSF_DEPTH_U16_SCALED>, dim3(nb), dim3(256), 0, st, a, depth, scale, model, d32, cls, stats);
    else
        hipLaunchKernelGGL(k_motion_classify<SSF_DEPTH_F32_METRES>, dim3(nb), dim3(256), 0, st, a, depth, scale, model, d32, cls, stats);
}
static void launch_motion_label(hipStream_t st, const MotionArgs& a, const float* d32, const uint8_t* cls, int32_t* parent, int32_t* label, uint2* cnt) {
    ScopedKernel sk("motion_label", st);
    hipLaunchKernelGGL(k_motion_label, dim3(a.ntx * a.nty), dim3(256), 0, st, a, d32, cls, parent, label, cnt);
}
static void launch_motion_merge(hipStream_t st, const MotionArgs& a, const float* d32, int32_t* parent) {
    ScopedKernel sk("motion_merge", st);
    const long long n = ccl_border_threads(a.W, a.H, a.ntx, a.nty);
    if (n > 0) hipLaunchKernelGGL(k_motion_merge, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, d32, parent);
}
static void launch_motion_flatten(hipStream_t st, const MotionArgs& a, const int32_t* parent, int32_t* label, uint2* cnt) {
    ScopedKernel sk("motion_flatten", st);
    const unsigned nb = (unsigned)(((size_t)a.W * a.H + 255) / 256);
    hipLaunchKernelGGL(k_motion_roots, dim3(nb), dim3(256), 0, st, a, parent, label, cnt);
    hipLaunchKernelGGL(k_motion_flatten, dim3(nb), dim3(256), 0, st, a, parent, label);
}
static void launch_motion_decide(hipStream_t st, const MotionArgs& a, const int32_t* label, const uint2* cnt, uint8_t* mask,
                                 unsigned long long* stats) {
    ScopedKernel sk("motion_decide", st);
    hipLaunchKernelGGL(k_motion_decide, dim3((unsigned)(((size_t)a.W * a.H + 255) / 256)), dim3(256), 0, st, a, label, cnt, mask, stats);
}

}  // namespace ssf

// ---- host: the entry points of include/ssf_motion.h ------------------------------------------------------------------------
static bool motion_extent_ok(float v) { return std::isfinite(v) && v >= 0.0f; }

// the checks of include/ssf_motion.h on the parameters, and the kernels' argument
static int motion_args(ssf_handle* h, const ssf_motion_params* p, const char* who, MotionArgs& a) {
    auto refuse = [&](const char* what) { h->err = std::string(who) + ": " + what; return SSF_ERR_INVALID_ARG; };
    if (!motion_extent_ok(p->front_abs) || !motion_extent_ok(p->front_quad)) return refuse("front_abs and front_quad must be finite and >= 0");
    if (!motion_extent_ok(p->link_abs) || !motion_extent_ok(p->link_rel)) return refuse("link_abs and link_rel must be finite and >= 0");
    if (p->min_seeds < 1) return refuse("min_seeds must be >= 1");
    if (p->unknown_per_seed < 0) return refuse("unknown_per_seed must be >= 0");
    a.W = h->cam.W; a.H = h->cam.H; a.ntx = (a.W + MT_W - 1) / MT_W; a.nty = (a.H + MT_H - 1) / MT_H;
    a.rmin = h->cfg.range_min; a.rmax = h->cfg.range_max;
    a.front_abs = p->front_abs; a.front_quad = p->front_quad; a.link_abs = p->link_abs; a.link_rel = p->link_rel;
    a.min_seeds = p->min_seeds; a.unknown_per_seed = p->unknown_per_seed;
    return SSF_OK;
}
static size_t motion_depth_bpp(const ssf_handle* h) { return h->in_depth == SSF_DEPTH_U16_SCALED ? 2 : 4; }
static int motion_depth_ok(ssf_handle* h, const void* depth, int on_device, const char* who) {
    if (on_device && (uintptr_t)depth % motion_depth_bpp(h)) {
        h->err = std::string(who) + ": the device depth pointer is not aligned for the input format"; return SSF_ERR_INVALID_ARG;
    }
    return SSF_OK;
}
// the working buffers, all or nothing
static int motion_ws(ssf_handle* h, const char* who) {
    MotionWs& w = h->motion;
    const size_t P = (size_t)h->cam.W * h->cam.H;
    if (w.pixels == P) return SSF_OK;
    if (!w.bufs.grow({{(void**)&w.din, 4 * P}, {(void**)&w.m, 4 * P}, {(void**)&w.d32, 4 * P}, {(void**)&w.cls, P}, {(void**)&w.parent, 4 * P},
                      {(void**)&w.label, 4 * P}, {(void**)&w.cnt, 8 * P}, {(void**)&w.mask, P}, {(void**)&w.last, P},
                      {(void**)&w.stats, MST_WORDS * sizeof(unsigned long long)}})) {
        h->err = std::string(who) + ": allocation of the working buffers failed"; return SSF_ERR_DEVICE;
    }
    w.pixels = P;
    return SSF_OK;
}
// steps 1-7 on a depth image (a device pointer when on_device, else uploaded here) and a model depth in device memory; the
// outputs are copied out of the workspace (enqueued), the five counts into st5; the caller waits for the stream
static int motion_run(ssf_handle* h, const MotionArgs& a, const void* depth, int on_device, const float* d_model, uint8_t* mask, int32_t* label,
                      uint8_t* cls, unsigned long long* st5) {
    MotionWs& w = h->motion;
    hipStream_t st = h->stream;
    const size_t P = (size_t)a.W * a.H;
    const void* d_depth = depth;
    if (!on_device) { HCK(hipMemcpyAsync(w.din, depth, motion_depth_bpp(h) * P, hipMemcpyHostToDevice, st)); d_depth = w.din; }
    HCK(hipMemsetAsync(w.stats, 0, MST_WORDS * sizeof(unsigned long long), st));
    launch_motion_classify(st, a, d_depth, h->in_depth, h->in_scale, d_model, w.d32, w.cls, w.stats);
    launch_motion_label(st, a, w.d32, w.cls, w.parent, w.label, w.cnt);
    launch_motion_merge(st, a, w.d32, w.parent);
    launch_motion_flatten(st, a, w.parent, w.label, w.cnt);
    launch_motion_decide(st, a, w.label, w.cnt, w.mask, w.stats);
    HCK(hipGetLastError());
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (mask) HCK(hipMemcpyAsync(mask, w.mask, P, kind, st));
    if (label) HCK(hipMemcpyAsync(label, w.label, 4 * P, kind, st));
    if (cls) HCK(hipMemcpyAsync(cls, w.cls, P, kind, st));
    HCK(hipMemcpyAsync(st5, w.stats, MST_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    return SSF_OK;
}
static void motion_stats_out(ssf_motion_stats* s, const unsigned long long* st5) {
    s->n_seed = (int64_t)st5[MST_SEED]; s->n_unknown = (int64_t)st5[MST_UNKNOWN]; s->n_components = (int64_t)st5[MST_COMP];
    s->n_dynamic_components = (int64_t)st5[MST_DYN]; s->pixels_masked = (int64_t)st5[MST_MASKED];
}
// the model depth of ssf_motion_mask: ssf_render_model's depth image at `pose` into the workspace
static int motion_render(ssf_handle* h, const ssf_motion_params* p, const float* pose) {
    ssf_render_params rp;
    std::memset(&rp, 0, sizeof(rp));                   // width 0: the handle's camera; z_min = z_max = 0: the configuration's range
    rp.pose = pose; rp.min_conf = p->min_conf; rp.splat_scale = p->splat_scale; rp.visible_only = 0; rp.on_device = 1;
    return ssf_render_model(h, &rp, h->motion.m, nullptr, nullptr, nullptr, nullptr, nullptr);
}
// ssf_motion_mask's body: the render at `pose`, then steps 1-7; on_device: of depth and every output
static int motion_mask_at(ssf_handle* h, const ssf_motion_params* p, const MotionArgs& a, const float* pose, const void* depth, int on_device,
                          uint8_t* mask, int32_t* label, uint8_t* cls, float* model_depth_out, ssf_motion_stats* stats) {
    { int rc = motion_render(h, p, pose); if (rc) return rc; }
    MotionWs& w = h->motion;
    TimerScope ts(h);
    unsigned long long st5[MST_WORDS] = {0, 0, 0, 0, 0};
    { int rc = motion_run(h, a, depth, on_device, w.m, mask, label, cls, st5); if (rc) return rc; }
    if (model_depth_out)
        HCK(hipMemcpyAsync(model_depth_out, w.m, 4 * (size_t)a.W * a.H, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    { int rc = sync_collect(h); if (rc) return rc; }
    if (stats) motion_stats_out(stats, st5);
    return SSF_OK;
}

extern "C" {
int ssf_motion_default_params(const ssf_handle* h, ssf_motion_params* p) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    std::memset(p, 0, sizeof(*p));
    p->min_conf = 0.0f; p->splat_scale = 3.0f;
    p->front_abs = 0.05f; p->front_quad = 0.01f; p->link_abs = 0.02f; p->link_rel = 0.01f;
    p->min_seeds = std::max(1, (int)(((long long)h->cam.W * h->cam.H) / 1024));
    p->unknown_per_seed = 2;
    return SSF_OK;
}

int ssf_motion_segment(ssf_handle* h, const ssf_motion_params* p, const void* depth, const float* model_depth, uint8_t* mask,
                       int32_t* label, uint8_t* cls, ssf_motion_stats* stats) {
    if (!h || !p || !depth || !model_depth) return SSF_ERR_INVALID_ARG;
    if (!mask && !label && !cls) { h->err = "ssf_motion_segment: every output is NULL"; return SSF_ERR_INVALID_ARG; }
    MotionArgs a;
    { int rc = motion_args(h, p, "ssf_motion_segment", a); if (rc) return rc; }
    const int on_device = p->on_device ? 1 : 0;
    { int rc = motion_depth_ok(h, depth, on_device, "ssf_motion_segment"); if (rc) return rc; }
    if (on_device && (uintptr_t)model_depth % 4) { h->err = "ssf_motion_segment: the device model depth is not aligned to 4 bytes"; return SSF_ERR_INVALID_ARG; }
    { int rc = model_at_rest(h, "ssf_motion_segment", "does not detect motion"); if (rc) return rc; }
    { int rc = motion_ws(h, "ssf_motion_segment"); if (rc) return rc; }
    MotionWs& w = h->motion;
    TimerScope ts(h);
    const float* d_model = model_depth;
    if (!on_device) { HCK(hipMemcpyAsync(w.m, model_depth, 4 * (size_t)a.W * a.H, hipMemcpyHostToDevice, h->stream)); d_model = w.m; }
    unsigned long long st5[MST_WORDS] = {0, 0, 0, 0, 0};
    { int rc = motion_run(h, a, depth, on_device, d_model, mask, label, cls, st5); if (rc) return rc; }
    { int rc = sync_collect(h); if (rc) return rc; }
    if (stats) motion_stats_out(stats, st5);
    return SSF_OK;
}

int ssf_motion_mask(ssf_handle* h, const ssf_motion_params* p, const void* depth, uint8_t* mask, int32_t* label, uint8_t* cls,
                    float* model_depth_out, ssf_motion_stats* stats) {
    if (!h || !p || !depth) return SSF_ERR_INVALID_ARG;
    if (!mask && !label && !cls) { h->err = "ssf_motion_mask: every output is NULL"; return SSF_ERR_INVALID_ARG; }
    MotionArgs a;
    { int rc = motion_args(h, p, "ssf_motion_mask", a); if (rc) return rc; }
    const int on_device = p->on_device ? 1 : 0;
    { int rc = motion_depth_ok(h, depth, on_device, "ssf_motion_mask"); if (rc) return rc; }
    { int rc = model_at_rest(h, "ssf_motion_mask", "does not detect motion"); if (rc) return rc; }
    { int rc = motion_ws(h, "ssf_motion_mask"); if (rc) return rc; }
    return motion_mask_at(h, p, a, p->pose, depth, on_device, mask, label, cls, model_depth_out, stats);
}

int ssf_process_frame_motion(ssf_handle* h, const void* rgb, const void* depth, int on_device, const float* prior_pose,
                             const ssf_motion_params* p, ssf_frame_result* out) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    on_device = on_device ? 1 : 0;
    if (!frame_inputs_ok(h, rgb, depth, on_device)) return SSF_ERR_INVALID_ARG;
    MotionArgs a;
    { int rc = motion_args(h, p, "ssf_process_frame_motion", a); if (rc) return rc; }
    { int rc = model_at_rest(h, "ssf_process_frame_motion", "does not detect motion"); if (rc) return rc; }
    { int rc = motion_ws(h, "ssf_process_frame_motion"); if (rc) return rc; }
    MotionWs& w = h->motion;
    // the mask goes into `last` on the device (on_device = 1 for the output, whatever the frame's is: depth is uploaded by
    // motion_run when it is a host image, so the mask is staged through w.mask and copied device to device)
    ssf_motion_stats s;
    { int rc = motion_mask_at(h, p, a, p->pose ? p->pose : prior_pose, depth, on_device, nullptr, nullptr, nullptr, nullptr, &s); if (rc) return rc; }
    HCK(hipMemcpyAsync(w.last, w.mask, (size_t)a.W * a.H, hipMemcpyDeviceToDevice, h->stream));
    HCK(hipStreamSynchronize(h->stream));
    w.last_stats = s; w.have_last = true;
    return process_frame_devmask(h, rgb, depth, on_device, prior_pose, w.last, out);
}

int ssf_get_motion_mask(ssf_handle* h, uint8_t* mask, ssf_motion_stats* stats) {
    if (!h) return SSF_ERR_INVALID_ARG;
    MotionWs& w = h->motion;
    if (!w.have_last) { h->err = "ssf_get_motion_mask: no frame has been processed by ssf_process_frame_motion"; return SSF_ERR_STATE; }
    if (mask) {
        HCK(hipMemcpyAsync(mask, w.last, w.pixels, hipMemcpyDeviceToHost, h->stream));
        HCK(hipStreamSynchronize(h->stream));
    }
    if (stats) *stats = w.last_stats;
    return SSF_OK;
}
}  // extern "C"
