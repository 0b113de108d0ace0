// ssf_odometry.hip -- dense RGB-D odometry (include/ssf_odometry.h) on gfx950: the pyramids and the normal equations.
//
// What is computed is pinned, operation by operation, in include/ssf_odometry.h (the numpy restatement: tests/odometry_ref.py).  How:
//   * pyramid    one bracket "odo_pyramid": k_odo_pyramid_base (one thread per pixel: the input formats are converted where the
//                pixel is loaded; luma, validated depth, the reference's mask), k_odo_pyramid_reduce once per coarser level (one
//                thread per output pixel, the 2 x 2 block of each array), k_odo_gradient once for all levels (they lie in one
//                buffer).  I, D, gx and gy are stored: the linearisation gathers twelve values per pixel as it is, recomputing
//                the gradients at the four neighbours would gather twenty-four.
//   * linearise  k_odo_linearise, one launch per iteration, a grid sized to the level (at most ODO_MAX_BLOCKS workgroups that
//                stride over it).  A thread reads one reference pixel (4-byte coalesced loads of D and I), warps it, gathers the
//                current level (the divergent part) and forms its 29 integer terms one at a time: each goes straight into one of
//                16 LDS copies of the record by a 64-bit LDS atomic (lane & 15, as k_align), so no term stays in a register and
//                the kernel keeps its occupancy.  At the end 29 threads add the copies up and issue one 64-bit global atomic per
//                non-zero word.  Integer sums: the record does not depend on any order.
// The host loop (odo_loop) reads the record back once per iteration and takes the step with ssf_solvers.hpp.  Nothing here writes
// to the handle's stores, counters or scratch: the working set is OdoWs (ssf_handle.hpp).
#include "ssf_slots.hpp"
#include "ssf_handle.hpp"
#include "ssf_solvers.hpp"

namespace ssf {

enum { ODO_MAX_BLOCKS = 1024, ODO_SLOTS = 16 };
#define SSF_ODO_LIM 1099511627776.0            /* 2^40 (SSF_ODO_CLAMP_BITS) */

struct OdoLevel { int W, H; float fx, fy, cx, cy; };
struct OdoLevels { int n; int W[SSF_ODO_MAX_LEVELS], H[SSF_ODO_MAX_LEVELS]; unsigned off[SSF_ODO_MAX_LEVELS + 1]; };

// ---- pyramid ---------------------------------------------------------------------------------------------------------------
template <int CF, int DF>
__global__ __launch_bounds__(256) void k_odo_pyramid_base(int P, const uint8_t* __restrict__ rgb, const void* __restrict__ depth, double scale,
                                                          float rmin, float rmax, const uint8_t* __restrict__ mask, float* __restrict__ I,
                                                          float* __restrict__ D) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    unsigned c0, c1, c2;
    if (CF == SSF_COLOR_RGBA8 || CF == SSF_COLOR_BGRA8) {
        const uint32_t q = reinterpret_cast<const uint32_t*>(rgb)[p];
        c0 = q & 255u; c1 = (q >> 8) & 255u; c2 = (q >> 16) & 255u;
    } else {
        c0 = rgb[3 * (size_t)p]; c1 = rgb[3 * (size_t)p + 1]; c2 = rgb[3 * (size_t)p + 2];
    }
    const unsigned r = (CF == SSF_COLOR_BGR8 || CF == SSF_COLOR_BGRA8) ? c2 : c0, b = (CF == SSF_COLOR_BGR8 || CF == SSF_COLOR_BGRA8) ? c0 : c2;
    I[p] = (float)((77u * r + 150u * c1 + 29u * b) >> 8) * 0.00390625f;
    float d;
    if (DF == SSF_DEPTH_U16_SCALED) d = (float)((double)reinterpret_cast<const uint16_t*>(depth)[p] * scale);
    else d = reinterpret_cast<const float*>(depth)[p];
    const bool ok = isfinite(d) && d >= rmin && d <= rmax && !(mask && mask[p]);
    D[p] = ok ? d : 0.0f;
}

__device__ __forceinline__ float odo_min_valid(float a, float b) { return a == 0.0f ? b : (b == 0.0f ? a : fminf(a, b)); }
// level l (Ws x Hs) -> level l + 1 (Wd x Hd = floor / 2): the 2 x 2 block at (2x, 2y)
__global__ __launch_bounds__(256) void k_odo_pyramid_reduce(int Ws, int Wd, int Hd, const float* __restrict__ Is, const float* __restrict__ Ds,
                                                            float* __restrict__ Id, float* __restrict__ Dd) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= Wd * Hd) return;
    const int x = p % Wd, y = p / Wd;
    const size_t s = (size_t)(2 * y) * Ws + 2 * x;
    const float a = Is[s], b = Is[s + 1], c = Is[s + Ws], d = Is[s + Ws + 1];
    Id[p] = 0.25f * ((a + b) + (c + d));
    Dd[p] = odo_min_valid(odo_min_valid(Ds[s], Ds[s + 1]), odo_min_valid(Ds[s + Ws], Ds[s + Ws + 1]));
}
// every level at once: thread p of [off[l], off[l + 1]) is pixel p - off[l] of level l
__global__ __launch_bounds__(256) void k_odo_gradient(OdoLevels lv, const float* __restrict__ I, float* __restrict__ gx, float* __restrict__ gy) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= lv.off[lv.n]) return;
    int l = 0;
#pragma unroll
    for (int k = 1; k < SSF_ODO_MAX_LEVELS; k++) if (k < lv.n && p >= lv.off[k]) l = k;
    const int W = lv.W[l], H = lv.H[l];
    const unsigned q = p - lv.off[l];
    const int x = (int)(q % (unsigned)W), y = (int)(q / (unsigned)W);
    const float* L = I + lv.off[l];
    const int xp = min(x + 1, W - 1), xm = max(x - 1, 0), yp = min(y + 1, H - 1), ym = max(y - 1, 0);
    gx[p] = 0.5f * (L[(size_t)y * W + xp] - L[(size_t)y * W + xm]);
    gy[p] = 0.5f * (L[(size_t)yp * W + x] - L[(size_t)ym * W + x]);
}

// ---- linearise -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float odo_bilinear(const float* __restrict__ a, size_t i, int W, float ax, float ay) {
    const float p00 = a[i], p10 = a[i + 1], p01 = a[i + W], p11 = a[i + W + 1];
    const float top = p00 + ax * (p10 - p00), bot = p01 + ax * (p11 - p01);
    return top + ay * (bot - top);
}
__device__ __forceinline__ void odo_add(unsigned long long* red, int word, int slot, float v, double scale) {
    atomicAdd(&red[word * ODO_SLOTS + slot], (unsigned long long)fx64((double)v, scale, SSF_ODO_LIM));
}
__global__ __launch_bounds__(256) void k_odo_linearise(OdoLevel lv, float rmin, float rmax, float r_max, float huber, Rt T,
                                                       const float* __restrict__ refI, const float* __restrict__ refD,
                                                       const float* __restrict__ curI, const float* __restrict__ curGx,
                                                       const float* __restrict__ curGy, unsigned long long* __restrict__ rec) {
    __shared__ unsigned long long red[SSF_ODO_RECORD * ODO_SLOTS];
    for (int i = threadIdx.x; i < SSF_ODO_RECORD * ODO_SLOTS; i += 256) red[i] = 0ull;
    __syncthreads();
    const int n = lv.W * lv.H, slot = threadIdx.x & (ODO_SLOTS - 1);
    for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
        const float d = refD[p];
        if (d == 0.0f) continue;
        const int x = p % lv.W, y = p / lv.W;
        const V3 X = v3((((float)x - lv.cx) / lv.fx) * d, (((float)y - lv.cy) / lv.fy) * d, d);
        const V3 Y = v3(dot3(T.R.r0, X) + T.t.x, dot3(T.R.r1, X) + T.t.y, dot3(T.R.r2, X) + T.t.z);
        if (!(Y.z >= rmin && Y.z <= rmax)) continue;
        const float iz = 1.0f / Y.z;
        const float u = ((lv.fx * Y.x) * iz) + lv.cx, v = ((lv.fy * Y.y) * iz) + lv.cy;
        if (!(u >= 0.0f && v >= 0.0f && u < (float)(lv.W - 1) && v < (float)(lv.H - 1))) continue;
        const int x0 = (int)u, y0 = (int)v;                     // in [0, W - 2] x [0, H - 2]: the four neighbours are inside
        const float ax = u - (float)x0, ay = v - (float)y0;
        const size_t i = (size_t)y0 * lv.W + x0;
        const float r = odo_bilinear(curI, i, lv.W, ax, ay) - refI[p];
        const float ar = fabsf(r);
        if (!(ar <= r_max)) continue;
        const float w = ar <= huber ? 1.0f : huber / ar;
        const float a = odo_bilinear(curGx, i, lv.W, ax, ay) * lv.fx, b = odo_bilinear(curGy, i, lv.W, ax, ay) * lv.fy;
        const V3 g = v3(a * iz, b * iz, -((((a * Y.x) + (b * Y.y)) * iz) * iz));
        const V3 c = cross3(Y, g);
        const float J[6] = {c.x, c.y, c.z, g.x, g.y, g.z};
        int k = 0;
#pragma unroll
        for (int a0 = 0; a0 < 6; a0++) {
            const float wj = w * J[a0];
#pragma unroll
            for (int b0 = a0; b0 < 6; b0++, k++) odo_add(red, k, slot, wj * J[b0], (double)(1ll << SSF_ODO_S_A));
            odo_add(red, 21 + a0, slot, wj * r, (double)(1ll << SSF_ODO_S_B));
        }
        odo_add(red, 27, slot, (w * r) * r, (double)(1ll << SSF_ODO_S_C));
        atomicAdd(&red[28 * ODO_SLOTS + slot], 1ull);
    }
    __syncthreads();
    if (threadIdx.x < SSF_ODO_RECORD) {
        unsigned long long tot = 0ull;
#pragma unroll
        for (int s = 0; s < ODO_SLOTS; s++) tot += red[threadIdx.x * ODO_SLOTS + s];
        if (tot) atomicAdd(&rec[threadIdx.x], tot);
    }
}

// ---- launches --------------------------------------------------------------------------------------------------------------
template <int CF>
static void launch_odo_base_cf(hipStream_t st, int P, const void* rgb, const void* depth, int df, double scale, float rmin, float rmax,
                               const uint8_t* mask, float* I, float* D) {
    const unsigned nb = (unsigned)((P + 255) / 256);
    if (df == SSF_DEPTH_U16_SCALED)
        hipLaunchKernelGGL((k_odo_pyramid_base<CF, SSF_DEPTH_U16_SCALED>), dim3(nb), dim3(256), 0, st, P, (const uint8_t*)rgb, depth, scale, rmin, rmax, mask, I, D);
    else
        hipLaunchKernelGGL((k_odo_pyramid_base<CF, SSF_DEPTH_F32_METRES>), dim3(nb), dim3(256), 0, st, P, (const uint8_t*)rgb, depth, scale, rmin, rmax, mask, I, D);
}
static void launch_odo_pyramid(ssf_handle* h, const OdoPyramid& py, const void* d_rgb, const void* d_depth, const uint8_t* d_mask) {
    const OdoWs& w = h->odo;
    hipStream_t st = h->stream;
    ScopedKernel sk("odo_pyramid", st);
    const int P = w.lw[0] * w.lh[0];
    const float rmin = h->cfg.range_min, rmax = h->cfg.range_max;
    switch (h->in_color) {
        case SSF_COLOR_BGR8: launch_odo_base_cf<SSF_COLOR_BGR8>(st, P, d_rgb, d_depth, h->in_depth, h->in_scale, rmin, rmax, d_mask, py.I, py.D); break;
        case SSF_COLOR_RGBA8: launch_odo_base_cf<SSF_COLOR_RGBA8>(st, P, d_rgb, d_depth, h->in_depth, h->in_scale, rmin, rmax, d_mask, py.I, py.D); break;
        case SSF_COLOR_BGRA8: launch_odo_base_cf<SSF_COLOR_BGRA8>(st, P, d_rgb, d_depth, h->in_depth, h->in_scale, rmin, rmax, d_mask, py.I, py.D); break;
        default: launch_odo_base_cf<SSF_COLOR_RGB8>(st, P, d_rgb, d_depth, h->in_depth, h->in_scale, rmin, rmax, d_mask, py.I, py.D); break;
    }
    OdoLevels lv;
    lv.n = w.levels;
    for (int l = 0; l < SSF_ODO_MAX_LEVELS; l++) { lv.W[l] = w.lw[l]; lv.H[l] = w.lh[l]; }
    for (int l = 0; l <= SSF_ODO_MAX_LEVELS; l++) lv.off[l] = (unsigned)w.off[l];
    for (int l = 1; l < w.levels; l++) {
        const int n = w.lw[l] * w.lh[l];
        hipLaunchKernelGGL(k_odo_pyramid_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w.lw[l - 1], w.lw[l], w.lh[l], py.I + w.off[l - 1],
                           py.D + w.off[l - 1], py.I + w.off[l], py.D + w.off[l]);
    }
    hipLaunchKernelGGL(k_odo_gradient, dim3((unsigned)((w.off[w.levels] + 255) / 256)), dim3(256), 0, st, lv, py.I, py.gx, py.gy);
}
static void launch_odo_linearise(ssf_handle* h, const ssf_odometry_params* p, int l, const Rt& T) {
    const OdoWs& w = h->odo;
    hipStream_t st = h->stream;
    ScopedKernel sk("odo_linearise", st);
    OdoLevel lv;
    lv.W = w.lw[l]; lv.H = w.lh[l]; lv.fx = w.lfx[l]; lv.fy = w.lfy[l]; lv.cx = w.lcx[l]; lv.cy = w.lcy[l];
    const OdoPyramid& ref = w.pyr[w.ref]; const OdoPyramid& cur = w.pyr[1 - w.ref];
    const int n = lv.W * lv.H;
    const unsigned nb = (unsigned)std::min((n + 255) / 256, (int)ODO_MAX_BLOCKS);
    hipLaunchKernelGGL(k_odo_linearise, dim3(nb), dim3(256), 0, st, lv, h->cfg.range_min, h->cfg.range_max, p->r_max, p->huber, T, ref.I + w.off[l],
                       ref.D + w.off[l], cur.I + w.off[l], cur.gx + w.off[l], cur.gy + w.off[l], w.rec);
}

}  // namespace ssf

// ---- host: the entry points of include/ssf_odometry.h ----------------------------------------------------------------------
static bool odo_extent_ok(float v) { return std::isfinite(v) && v >= 0.0f; }
static bool odo_finite12(const float* t) { for (int i = 0; i < 12; i++) if (!std::isfinite(t[i])) return false; return true; }

static int odo_params_ok(ssf_handle* h, const ssf_odometry_params* p, const char* who) {
    auto refuse = [&](const char* what) { h->err = std::string(who) + ": " + what; return SSF_ERR_INVALID_ARG; };
    if (p->levels < 1) return refuse("levels must be >= 1");
    for (int l = 0; l < SSF_ODO_MAX_LEVELS; l++) if (p->iters[l] < 0) return refuse("iters must be >= 0");
    if (!odo_extent_ok(p->r_max) || !odo_extent_ok(p->huber) || !odo_extent_ok(p->min_pixel_share)) return refuse("r_max, huber and min_pixel_share must be finite and >= 0");
    if (!odo_extent_ok(p->tol_rot) || !odo_extent_ok(p->tol_trans)) return refuse("tol_rot and tol_trans must be finite and >= 0");
    if (!odo_extent_ok(p->max_translation) || !odo_extent_ok(p->max_rotation)) return refuse("max_translation and max_rotation must be finite and >= 0");
    return SSF_OK;
}
static int odo_levels_used(const ssf_handle* h, const ssf_odometry_params* p) { return std::min(p->levels, h->odo.levels); }
// the level geometry and the working buffers, all or nothing
static int odo_ws(ssf_handle* h, const char* who) {
    OdoWs& w = h->odo;
    const size_t P = (size_t)h->cam.W * h->cam.H;
    if (w.pixels == P) return SSF_OK;
    int lw[SSF_ODO_MAX_LEVELS] = {}, lh[SSF_ODO_MAX_LEVELS] = {}, levels = 0; size_t off[SSF_ODO_MAX_LEVELS + 1] = {};
    for (int l = 0, cw = h->cam.W, ch = h->cam.H; l < SSF_ODO_MAX_LEVELS && (l == 0 || (cw >= SSF_ODO_MIN_W && ch >= SSF_ODO_MIN_H)); l++, cw /= 2, ch /= 2) {
        lw[l] = cw; lh[l] = ch; off[l + 1] = off[l] + (size_t)cw * ch; levels = l + 1;
    }
    for (int l = levels; l < SSF_ODO_MAX_LEVELS; l++) off[l + 1] = off[l];
    const size_t n = 4 * off[levels];
    if (!w.bufs.grow({{(void**)&w.pyr[0].I, n}, {(void**)&w.pyr[0].D, n}, {(void**)&w.pyr[0].gx, n}, {(void**)&w.pyr[0].gy, n},
                      {(void**)&w.pyr[1].I, n}, {(void**)&w.pyr[1].D, n}, {(void**)&w.pyr[1].gx, n}, {(void**)&w.pyr[1].gy, n},
                      {(void**)&w.rgb_in, 4 * P}, {(void**)&w.depth_in, 4 * P}, {(void**)&w.mask_in, P},
                      {(void**)&w.rec, SSF_ODO_RECORD * sizeof(unsigned long long)}})) {
        h->err = std::string(who) + ": allocation of the working buffers failed"; return SSF_ERR_DEVICE;
    }
    w.levels = levels;
    for (int l = 0; l < SSF_ODO_MAX_LEVELS; l++) { w.lw[l] = lw[l]; w.lh[l] = lh[l]; }
    for (int l = 0; l <= SSF_ODO_MAX_LEVELS; l++) w.off[l] = off[l];
    w.lfx[0] = h->cam.fx; w.lfy[0] = h->cam.fy; w.lcx[0] = h->cam.cx; w.lcy[0] = h->cam.cy;
    for (int l = 1; l < levels; l++) {
        w.lfx[l] = w.lfx[l - 1] / 2.0f; w.lfy[l] = w.lfy[l - 1] / 2.0f;
        w.lcx[l] = (w.lcx[l - 1] + 0.5f) / 2.0f - 0.5f; w.lcy[l] = (w.lcy[l - 1] + 0.5f) / 2.0f - 0.5f;
    }
    w.pixels = P; w.ref = 0; w.have_ref = w.have_cur = w.ref_pose_pending = w.have_last = false;
    return SSF_OK;
}
// what every call asks first: the state refusals, then the buffers
static int odo_ready(ssf_handle* h, const char* who) {
    { int rc = model_at_rest(h, who, "has no odometry"); if (rc) return rc; }
    return odo_ws(h, who);
}
// the pyramid of a frame into py (enqueued): host images are uploaded in the input format first
static int odo_build(ssf_handle* h, const OdoPyramid& py, const void* rgb, const void* depth, int on_device, const uint8_t* mask) {
    OdoWs& w = h->odo;
    const size_t P = w.pixels;
    const void* d_rgb = rgb; const void* d_depth = depth; const uint8_t* d_mask = mask;
    if (!on_device) {
        const size_t cb = (h->in_color == SSF_COLOR_RGBA8 || h->in_color == SSF_COLOR_BGRA8) ? 4 : 3, db = h->in_depth == SSF_DEPTH_U16_SCALED ? 2 : 4;
        HCK(hipMemcpyAsync(w.rgb_in, rgb, cb * P, hipMemcpyHostToDevice, h->stream)); d_rgb = w.rgb_in;
        HCK(hipMemcpyAsync(w.depth_in, depth, db * P, hipMemcpyHostToDevice, h->stream)); d_depth = w.depth_in;
        if (mask) { HCK(hipMemcpyAsync(w.mask_in, mask, P, hipMemcpyHostToDevice, h->stream)); d_mask = w.mask_in; }
    }
    launch_odo_pyramid(h, py, d_rgb, d_depth, d_mask);
    HCK(hipGetLastError());
    return SSF_OK;
}
// the reference pose of a pyramid that became the reference by a swap is the handle's pose at the next call (ssf_odometry.h)
static void odo_settle_ref_pose(ssf_handle* h) {
    OdoWs& w = h->odo;
    if (w.ref_pose_pending) { w.ref_pose = h->pose; w.ref_pose_pending = false; }
}
// one record of level l at T (f32) into rec29; waits for the stream
static int odo_record(ssf_handle* h, const ssf_odometry_params* p, int l, const Rt& T, long long* rec29) {
    OdoWs& w = h->odo;
    HCK(hipMemsetAsync(w.rec, 0, SSF_ODO_RECORD * sizeof(unsigned long long), h->stream));
    launch_odo_linearise(h, p, l, T);
    HCK(hipGetLastError());
    HCK(hipMemcpyAsync(rec29, w.rec, SSF_ODO_RECORD * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    HCK(hipStreamSynchronize(h->stream));
    return SSF_OK;
}
// (R, t) -> (R^T, -(R^T t)) on 4 x 4 row-major f64
static void odo_invert(const double* T, double* out) {
    for (int i = 0; i < 16; i++) out[i] = 0.0;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out[i * 4 + j] = T[j * 4 + i];
        out[i * 4 + 3] = -(((T[0 * 4 + i] * T[3]) + (T[1 * 4 + i] * T[7])) + (T[2 * 4 + i] * T[11]));
    }
    out[15] = 1.0;
}
static void odo_from12(const float* p, double* T) {
    for (int i = 0; i < 16; i++) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) T[i * 4 + j] = (double)p[3 * i + j]; T[i * 4 + 3] = (double)p[9 + i]; }
}
static void odo_to12(const double* T, float* p) {
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) p[3 * i + j] = (float)T[i * 4 + j]; p[9 + i] = (float)T[i * 4 + 3]; }
}
// the LOOP of include/ssf_odometry.h on the current pyramid against the reference
static int odo_loop(ssf_handle* h, const ssf_odometry_params* p, const float* init12, float* rel12, ssf_odometry_result* res) {
    const OdoWs& w = h->odo;
    std::memset(res, 0, sizeof(*res));
    const int L = odo_levels_used(h, p);
    res->levels = L;
    double T[16], tmp[16];
    if (init12) { odo_from12(init12, tmp); odo_invert(tmp, T); }
    else for (int i = 0; i < 16; i++) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
    bool failed = false, converged = false;
    for (int l = L - 1; l >= 0 && !failed; l--) {
        const int min_pixels = std::max(1, (int)(p->min_pixel_share * (float)(w.lw[l] * w.lh[l])));
        converged = false;
        for (int it = 0; it < p->iters[l]; it++) {
            float t12[12];
            odo_to12(T, t12);
            long long rec[SSF_ODO_RECORD];
            { int rc = odo_record(h, p, l, pose_from12(t12), rec); if (rc) return rc; }
            res->iters[l]++;
            res->pixels = rec[28];
            res->mean_sq_residual = rec[28] > 0 ? ((double)rec[27] / (double)(1ll << SSF_ODO_S_C)) / (double)rec[28] : 0.0;
            if (rec[28] < (long long)min_pixels) { res->reason = SSF_ODO_TOO_FEW_PIXELS; failed = true; break; }
            double A[36], b[6], delta[6];
            int k = 0;
            for (int i = 0; i < 6; i++) for (int j = i; j < 6; j++, k++) A[i * 6 + j] = A[j * 6 + i] = (double)rec[k] / (double)(1ll << SSF_ODO_S_A);
            for (int i = 0; i < 6; i++) b[i] = -((double)rec[21 + i] / (double)(1ll << SSF_ODO_S_B));
            sym6_ldlt_solve(A, b, delta);
            bool finite = true;
            for (int i = 0; i < 6; i++) finite = finite && std::isfinite(delta[i]);
            if (!finite) { res->reason = SSF_ODO_DEGENERATE; failed = true; break; }
            gn_increment(delta, tmp);
            mat4_lmul(tmp, T);
            const double nr = std::sqrt((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2]);
            const double nt = std::sqrt((delta[3] * delta[3] + delta[4] * delta[4]) + delta[5] * delta[5]);
            if (nr < (double)p->tol_rot && nt < (double)p->tol_trans) { converged = true; break; }
        }
    }
    odo_invert(T, tmp);
    odo_to12(tmp, rel12);
    if (!failed) {
        res->reason = converged ? SSF_ODO_CONVERGED : SSF_ODO_MAX_ITERATIONS;
        const double nt = std::sqrt((tmp[3] * tmp[3] + tmp[7] * tmp[7]) + tmp[11] * tmp[11]);
        const double chord = std::sqrt(std::max(0.0, 3.0 - ((tmp[0] + tmp[5]) + tmp[10])));
        if (nt > (double)p->max_translation || chord > (double)p->max_rotation || !(nt == nt) || !(chord == chord)) res->reason = SSF_ODO_MOTION_GATE;
        else res->valid = 1;
    }
    return SSF_OK;
}
// ssf_odometry_estimate's body after the checks
static int odo_estimate(ssf_handle* h, const ssf_odometry_params* p, const void* rgb, const void* depth, int on_device, const float* init12,
                        float* rel12, ssf_odometry_result* res) {
    OdoWs& w = h->odo;
    odo_settle_ref_pose(h);
    TimerScope ts(h);
    w.have_cur = false;                                 // (until the new pyramid is enqueued whole)
    { int rc = odo_build(h, w.pyr[1 - w.ref], rgb, depth, on_device, nullptr); if (rc) return rc; }
    w.have_cur = true;
    { int rc = odo_loop(h, p, init12, rel12, res); if (rc) return rc; }
    return sync_collect(h);
}
// ssf_odometry_track's body after the checks: the estimate, the prior, the swap; the outcome is kept for ssf_get_odometry
static int odo_track(ssf_handle* h, const ssf_odometry_params* p, const void* rgb, const void* depth, int on_device) {
    OdoWs& w = h->odo;
    float rel[12]; ssf_odometry_result res;
    { int rc = odo_estimate(h, p, rgb, depth, on_device, nullptr, rel, &res); if (rc) return rc; }
    std::memcpy(w.last_rel, rel, sizeof(rel)); w.last_result = res; w.have_last = true;
    std::memset(w.last_prior, 0, sizeof(w.last_prior));
    if (res.valid) {
        const Rt r = pose_from12(rel);
        Rt q; q.R = m3_mul(w.ref_pose.R, r.R); q.t = add(m3_mulv(w.ref_pose.R, r.t), w.ref_pose.t);
        pose_to12(q, w.last_prior);
    }
    w.ref = 1 - w.ref; w.have_cur = false; w.ref_pose_pending = true;      // the current pyramid is the reference now; its pose: see odo_settle_ref_pose
    return SSF_OK;
}

extern "C" {
int ssf_odometry_default_params(const ssf_handle* h, ssf_odometry_params* p) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    std::memset(p, 0, sizeof(*p));
    p->levels = 4;
    const int iters[SSF_ODO_MAX_LEVELS] = {4, 6, 8, 10, 10, 10};
    for (int l = 0; l < SSF_ODO_MAX_LEVELS; l++) p->iters[l] = iters[l];
    p->r_max = 0.5f; p->huber = 0.2f; p->min_pixel_share = 0.05f; p->tol_rot = 1e-4f; p->tol_trans = 1e-4f;
    p->max_translation = 0.3f; p->max_rotation = 0.35f;
    return SSF_OK;
}

int ssf_odometry_set_reference(ssf_handle* h, const void* rgb, const void* depth, int on_device, const uint8_t* ref_mask) {
    if (!h) return SSF_ERR_INVALID_ARG;
    on_device = on_device ? 1 : 0;
    if (!frame_inputs_ok(h, rgb, depth, on_device)) return SSF_ERR_INVALID_ARG;
    { int rc = odo_ready(h, "ssf_odometry_set_reference"); if (rc) return rc; }
    OdoWs& w = h->odo;
    TimerScope ts(h);
    w.have_ref = false;                                 // (until the new pyramid is enqueued whole)
    { int rc = odo_build(h, w.pyr[w.ref], rgb, depth, on_device, ref_mask); if (rc) return rc; }
    w.have_ref = true; w.ref_pose = h->pose; w.ref_pose_pending = false;
    return sync_collect(h);
}

int ssf_odometry_linearise(ssf_handle* h, const ssf_odometry_params* p, int level, const float* T12, int64_t* record) {
    if (!h || !p || !T12 || !record) return SSF_ERR_INVALID_ARG;
    { int rc = odo_params_ok(h, p, "ssf_odometry_linearise"); if (rc) return rc; }
    if (!odo_finite12(T12)) { h->err = "ssf_odometry_linearise: T12 is not finite"; return SSF_ERR_INVALID_ARG; }
    { int rc = odo_ready(h, "ssf_odometry_linearise"); if (rc) return rc; }
    OdoWs& w = h->odo;
    if (level < 0 || level >= odo_levels_used(h, p)) { h->err = "ssf_odometry_linearise: level out of range"; return SSF_ERR_INVALID_ARG; }
    if (!w.have_ref || !w.have_cur) { h->err = "ssf_odometry_linearise: needs a reference and the frame of an ssf_odometry_estimate"; return SSF_ERR_STATE; }
    odo_settle_ref_pose(h);
    TimerScope ts(h);
    long long rec[SSF_ODO_RECORD];
    { int rc = odo_record(h, p, level, pose_from12(T12), rec); if (rc) return rc; }
    for (int i = 0; i < SSF_ODO_RECORD; i++) record[i] = (int64_t)rec[i];
    return sync_collect(h);
}

int ssf_odometry_estimate(ssf_handle* h, const ssf_odometry_params* p, const void* rgb, const void* depth, int on_device, const float* init12,
                          float* rel12, ssf_odometry_result* result) {
    if (!h || !p || !rel12 || !result) return SSF_ERR_INVALID_ARG;
    on_device = on_device ? 1 : 0;
    if (!frame_inputs_ok(h, rgb, depth, on_device)) return SSF_ERR_INVALID_ARG;
    { int rc = odo_params_ok(h, p, "ssf_odometry_estimate"); if (rc) return rc; }
    if (init12 && !odo_finite12(init12)) { h->err = "ssf_odometry_estimate: init12 is not finite"; return SSF_ERR_INVALID_ARG; }
    { int rc = odo_ready(h, "ssf_odometry_estimate"); if (rc) return rc; }
    if (!h->odo.have_ref) { h->err = "ssf_odometry_estimate: no reference (ssf_odometry_set_reference)"; return SSF_ERR_STATE; }
    return odo_estimate(h, p, rgb, depth, on_device, init12, rel12, result);
}

int ssf_odometry_track(ssf_handle* h, const ssf_odometry_params* p, const void* rgb, const void* depth, int on_device, float* prior12,
                       ssf_odometry_result* result) {
    if (!h || !p || !prior12 || !result) return SSF_ERR_INVALID_ARG;
    on_device = on_device ? 1 : 0;
    if (!frame_inputs_ok(h, rgb, depth, on_device)) return SSF_ERR_INVALID_ARG;
    { int rc = odo_params_ok(h, p, "ssf_odometry_track"); if (rc) return rc; }
    { int rc = odo_ready(h, "ssf_odometry_track"); if (rc) return rc; }
    OdoWs& w = h->odo;
    if (!w.have_ref) { h->err = "ssf_odometry_track: no reference (ssf_odometry_set_reference)"; return SSF_ERR_STATE; }
    { int rc = odo_track(h, p, rgb, depth, on_device); if (rc) return rc; }
    *result = w.last_result;
    if (w.last_result.valid) std::memcpy(prior12, w.last_prior, sizeof(w.last_prior));
    return SSF_OK;
}

int ssf_process_frame_odometry(ssf_handle* h, const void* rgb, const void* depth, int on_device, const ssf_odometry_params* p,
                               const ssf_motion_params* motion, ssf_frame_result* out) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    on_device = on_device ? 1 : 0;
    if (!frame_inputs_ok(h, rgb, depth, on_device)) return SSF_ERR_INVALID_ARG;
    { int rc = odo_params_ok(h, p, "ssf_process_frame_odometry"); if (rc) return rc; }
    { int rc = odo_ready(h, "ssf_process_frame_odometry"); if (rc) return rc; }
    OdoWs& w = h->odo;
    const float* prior = nullptr;
    if (!w.have_ref) {                                  // the first frame: it becomes the reference, with the pose it results in
        TimerScope ts(h);
        { int rc = odo_build(h, w.pyr[w.ref], rgb, depth, on_device, nullptr); if (rc) return rc; }
        w.have_ref = true; w.ref_pose_pending = true;
        { int rc = sync_collect(h); if (rc) return rc; }
    } else {
        { int rc = odo_track(h, p, rgb, depth, on_device); if (rc) return rc; }
        if (w.last_result.valid) prior = w.last_prior;
    }
    if (motion) return ssf_process_frame_motion(h, rgb, depth, on_device, prior, motion, out);
    return process_frame_devmask(h, rgb, depth, on_device, prior, nullptr, out);
}

int ssf_get_odometry(ssf_handle* h, float* rel12, float* prior12, ssf_odometry_result* result) {
    if (!h) return SSF_ERR_INVALID_ARG;
    const OdoWs& w = h->odo;
    if (!w.have_last) { h->err = "ssf_get_odometry: no frame has been tracked by ssf_odometry_track"; return SSF_ERR_STATE; }
    if (rel12) std::memcpy(rel12, w.last_rel, sizeof(w.last_rel));
    if (prior12) std::memcpy(prior12, w.last_prior, sizeof(w.last_prior));
    if (result) *result = w.last_result;
    return SSF_OK;
}

int ssf_odometry_get_pyramid(ssf_handle* h, int which, int level, float* intensity, float* depth, float* gx, float* gy, int* width, int* height,
                             float* intrinsics4) {
    if (!h || which < 0 || which > 1) return SSF_ERR_INVALID_ARG;
    { int rc = odo_ready(h, "ssf_odometry_get_pyramid"); if (rc) return rc; }
    const OdoWs& w = h->odo;
    if (level < 0 || level >= w.levels) { h->err = "ssf_odometry_get_pyramid: level out of range"; return SSF_ERR_INVALID_ARG; }
    if (which == 0 ? !w.have_ref : !w.have_cur) { h->err = "ssf_odometry_get_pyramid: that pyramid has not been built"; return SSF_ERR_STATE; }
    const OdoPyramid& py = w.pyr[which == 0 ? w.ref : 1 - w.ref];
    const size_t n = 4 * (size_t)w.lw[level] * w.lh[level], o = w.off[level];
    if (intensity) HCK(hipMemcpyAsync(intensity, py.I + o, n, hipMemcpyDeviceToHost, h->stream));
    if (depth) HCK(hipMemcpyAsync(depth, py.D + o, n, hipMemcpyDeviceToHost, h->stream));
    if (gx) HCK(hipMemcpyAsync(gx, py.gx + o, n, hipMemcpyDeviceToHost, h->stream));
    if (gy) HCK(hipMemcpyAsync(gy, py.gy + o, n, hipMemcpyDeviceToHost, h->stream));
    HCK(hipStreamSynchronize(h->stream));
    if (width) *width = w.lw[level];
    if (height) *height = w.lh[level];
    if (intrinsics4) { intrinsics4[0] = w.lfx[level]; intrinsics4[1] = w.lfy[level]; intrinsics4[2] = w.lcx[level]; intrinsics4[3] = w.lcy[level]; }
    return SSF_OK;
}
}  // extern "C"
