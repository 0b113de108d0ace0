// ssf_navfloor.hip -- the floor plane of the fused model (include/ssf_navfloor.h) on gfx950.
//
// What is computed is pinned, operation by operation, in include/ssf_navfloor.h (the numpy restatement: tests/navfloor_ref.py).
// Everything the device accumulates is an integer count or an exact integer sum: independent of the order in which rows arrive.
//   * prep       k_navfloor_prep: one thread per slot of [visible rows | out-of-view span] (the two stores are read in place, as
//                k_navgrid_prep reads them).  The gates, m and the direction bin; the workgroup's votes go into a 31 x 31 LDS
//                histogram that reaches the global one as one atomic per non-zero bin.  The candidates are written as 32-byte
//                records (p, m, ia | ib << 8) behind ONE cursor atomic per workgroup (block_rank256 gives the place inside the
//                reservation).  The order of the records differs from run to run; nothing downstream depends on it.
//   * direction  k_navfloor_direction: one thread per record: window membership on the stored bin, the three quantised components
//                and the count summed per workgroup (block_sums), one 64-bit atomic per word and workgroup.
//   * height     k_navfloor_height: the alignment test and a 2048-bin LDS histogram (8 KB), one atomic per non-zero bin.
//   * refine     k_navfloor_refine, one launch per round: the inlier test and the ten int64 words, the products taken in integers.
// The host reads a small record after each stage and takes the next decision (ssf_navfloor_solve.hpp, free of HIP): 3 + refine_iters
// waits for the stream per call.  Every global atomic is an integer atomic.  Nothing here writes to the handle's stores, counters or
// scratch: the working set is NavFloorWs (ssf_handle.hpp).
//
// This file is NOT one of the product library's objects, nor of the eleven older libraries: it is linked with libssf_hip_mem.so's
// objects into libssf_hip_floor.so (csrc/Makefile), which is what a caller of the fit loads.
#include "ssf_slots.hpp"
#include "ssf_handle.hpp"
#pragma GCC visibility push(hidden)       // (the host steps are the library's own: no part of what it exports)
#include "ssf_navfloor_solve.hpp"
#pragma GCC visibility pop
#include "../../include/ssf_navfloor.h"

namespace ssf {

// the sums the host reads (unsigned long long words; the signed ones wrap as two's complement)
enum { NF_ROWS = 0, NF_CAND = 1, NF_CURSOR = 2, NF_DIR = 4, NF_ALIGNED = 8, NF_OUT = 9, NF_ROUND = 16, NF_WORDS = 10, NF_STATS = NF_ROUND + 8 * NF_WORDS };
// the histograms' words: the direction's 961 (padded), then the height's 2048
enum { NF_DIR_BINS = 31, NF_DIR_HIST = NF_DIR_BINS * NF_DIR_BINS, NF_HEIGHT_AT = 1024, NF_HEIGHT_BINS = 2048, NF_HIST = NF_HEIGHT_AT + NF_HEIGHT_BINS };

struct NavFloorGate {
    float o[3], u[3], a[3], b[3];
    float tilt_cos, scale, min_conf;
    int32_t ti0, ti1, tl0, tl1;
};
struct NavFloorPlane { float n[3], a[3], b[3]; float d, dist, align_cos; };

__device__ __forceinline__ float nf_dot(float x, float y, float z, const float* w) { return (x * w[0] + y * w[1]) + z * w[2]; }
// step 2: clamp((int)floorf(v * scale + 0.5f) + 15, 0, 30), the clamp made before the cast
__device__ __forceinline__ uint32_t nf_dir_bin(float v, float scale) {
    const float t = floorf(v * scale + 0.5f);
    return !(t > -15.0f) ? 0u : (t >= 15.0f ? 30u : (uint32_t)((int)t + 15));
}
__device__ __forceinline__ long long nf_quant(float v, double scale) { return (long long)rint((double)v * scale); }

// ---- prep: one thread per slot (steps 1 and 2) ------------------------------------------------------------------------------
// rec[2 k], rec[2 k + 1] = (p, bits of the bin), (m, 0) for candidate k; stats[NF_CURSOR] counts the records
__global__ __launch_bounds__(256) void k_navfloor_prep(ModelView mv, NavFloorGate g, float4* __restrict__ rec, uint32_t* __restrict__ dir_hist,
                                                       unsigned long long* __restrict__ stats) {
    __shared__ uint32_t hist[NF_DIR_HIST];
    __shared__ int part[4];
    __shared__ unsigned long long base;
    for (int t = threadIdx.x; t < NF_DIR_HIST; t += 256) hist[t] = 0u;
    __syncthreads();
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    SurfelSoA src; size_t row;
    const bool have = slot_row(mv, s, src, row);
    unsigned long long used = 0;
    bool cand = false;
    float px = 0.0f, py = 0.0f, pz = 0.0f, mx = 0.0f, my = 0.0f, mz = 0.0f;
    uint32_t bin = 0u;
    if (have) {
        const float cx = src.pos[3 * row], cy = src.pos[3 * row + 1], cz = src.pos[3 * row + 2];
        const float conf = src.conf[row], dx = src.dims[2 * row], dy = src.dims[2 * row + 1];
        const int32_t t0 = src.stamps[2 * row], t1 = src.stamps[2 * row + 1];
        const float nx = src.r2[3 * row], ny = src.r2[3 * row + 1], nz = src.r2[3 * row + 2];
        if (finite3(cx, cy, cz) && conf > g.min_conf && t0 >= g.ti0 && t0 <= g.ti1 && t1 >= g.tl0 && t1 <= g.tl1 && dx > 0.0f && dy > 0.0f &&
            isfinite(dx) && isfinite(dy) && fabsf(nx) <= 2.0f && fabsf(ny) <= 2.0f && fabsf(nz) <= 2.0f) {       // (a NaN or infinite n fails <=)
            used = 1;
            px = cx - g.o[0]; py = cy - g.o[1]; pz = cz - g.o[2];
            const float sd = nf_dot(nx, ny, nz, g.u);
            cand = fabsf(sd) >= g.tilt_cos && fabsf(px) < 512.0f && fabsf(py) < 512.0f && fabsf(pz) < 512.0f;
            if (cand) {
                const bool flip = sd < 0.0f;
                mx = flip ? -nx : nx; my = flip ? -ny : ny; mz = flip ? -nz : nz;
                const uint32_t ia = nf_dir_bin(nf_dot(mx, my, mz, g.a), g.scale), ib = nf_dir_bin(nf_dot(mx, my, mz, g.b), g.scale);
                bin = ia | (ib << 8);
                atomicAdd(&hist[ib * NF_DIR_BINS + ia], 1u);
            }
        }
    }
    // the workgroup's records behind one reservation: rank < count, base + count <= the candidates so far <= the slots
    const int rank = block_rank256(cand, part);
    const int count = (part[0] + part[1]) + (part[2] + part[3]);
    if (threadIdx.x == 0 && count) base = atomicAdd(&stats[NF_CURSOR], (unsigned long long)count);
    __syncthreads();                                                  // (base is told; hist is complete)
    if (cand) {
        float4* o = rec + 2 * (size_t)(base + (unsigned long long)rank);
        o[0] = make_float4(px, py, pz, __uint_as_float(bin));
        o[1] = make_float4(mx, my, mz, 0.0f);
    }
    for (int t = threadIdx.x; t < NF_DIR_HIST; t += 256) { const uint32_t c = hist[t]; if (c) atomicAdd(&dir_hist[t], c); }
    block_sums({used, (unsigned long long)cand}, stats, NF_ROWS);
}

// ---- direction: one thread per record (step 2's sums) ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navfloor_direction(const float4* __restrict__ rec, uint32_t n, int ia0, int ib0, unsigned long long* __restrict__ stats) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    unsigned long long in = 0, qx = 0, qy = 0, qz = 0;
    if (k < n) {
        const uint32_t bin = __float_as_uint(rec[2 * (size_t)k].w);
        const int ia = (int)(bin & 255u), ib = (int)(bin >> 8);
        if (abs(ia - ia0) <= 1 && abs(ib - ib0) <= 1) {
            const float4 m = rec[2 * (size_t)k + 1];
            in = 1;
            qx = (unsigned long long)nf_quant(m.x, 1048576.0); qy = (unsigned long long)nf_quant(m.y, 1048576.0); qz = (unsigned long long)nf_quant(m.z, 1048576.0);
        }
    }
    block_sums({in, qx, qy, qz}, stats, NF_DIR);
}

// ---- height: one thread per record (step 3) ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navfloor_height(const float4* __restrict__ rec, uint32_t n, NavFloorPlane P, float height_res,
                                                         uint32_t* __restrict__ height_hist, unsigned long long* __restrict__ stats) {
    __shared__ uint32_t hist[NF_HEIGHT_BINS];
    for (int t = threadIdx.x; t < NF_HEIGHT_BINS; t += 256) hist[t] = 0u;
    __syncthreads();
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    unsigned long long aligned = 0, outside = 0;
    if (k < n) {
        const float4 p = rec[2 * (size_t)k], m = rec[2 * (size_t)k + 1];
        if (nf_dot(m.x, m.y, m.z, P.n) >= P.align_cos) {
            aligned = 1;
            const float t = floorf(nf_dot(p.x, p.y, p.z, P.n) / height_res);
            if (t >= -1024.0f && t < 1024.0f) atomicAdd(&hist[(int)t + 1024], 1u);
            else outside = 1;
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < NF_HEIGHT_BINS; t += 256) { const uint32_t c = hist[t]; if (c) atomicAdd(&height_hist[t], c); }
    block_sums({aligned, outside}, stats, NF_ALIGNED);
}

// ---- refine: one thread per record, one launch per round (step 4) ----------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navfloor_refine(const float4* __restrict__ rec, uint32_t n, NavFloorPlane P, unsigned long long* __restrict__ sums) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    long long N = 0, x = 0, y = 0, z = 0;
    if (k < n) {
        const float4 p = rec[2 * (size_t)k], m = rec[2 * (size_t)k + 1];
        const float zf = nf_dot(p.x, p.y, p.z, P.n) - P.d;
        if (nf_dot(m.x, m.y, m.z, P.n) >= P.align_cos && fabsf(zf) <= P.dist) {
            N = 1;
            x = nf_quant(nf_dot(p.x, p.y, p.z, P.a), 1024.0); y = nf_quant(nf_dot(p.x, p.y, p.z, P.b), 1024.0); z = nf_quant(zf, 1024.0);
        }
    }
    typedef unsigned long long u64;
    block_sums({(u64)N, (u64)x, (u64)y, (u64)z, (u64)(x * x), (u64)(x * y), (u64)(y * y), (u64)(x * z), (u64)(y * z), (u64)(z * z)}, sums, 0);
}

static unsigned nf_blocks(uint32_t n) { return (n + 255u) / 256u; }

}  // namespace ssf

extern "C" {
int ssf_navfloor_default_params(const ssf_handle* h, ssf_navfloor_params* p) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    std::memset(p, 0, sizeof(*p));
    p->up[1] = -1.0f;
    p->tilt_cos = 0.8f; p->align_cos = 0.95f; p->height_res = 0.02f;
    p->min_rows = 32; p->floor_share256 = 64; p->refine_iters = 3;
    p->first_dist = 0.15f; p->inlier_dist = 0.05f;
    p->t_init_min = INT32_MIN; p->t_init_max = INT32_MAX; p->t_last_min = INT32_MIN; p->t_last_max = INT32_MAX;
    p->width = 512; p->height = 512; p->res = 0.05f;
    p->below = 0.5f; p->step = 0.2f; p->body_height = 1.5f;
    return SSF_OK;
}

int ssf_navfloor_fit(ssf_handle* h, const ssf_navfloor_params* p, const ssf_navfloor_out* out, ssf_navfloor_fit_result* res) {
    namespace nf = ssf_navfloor;
    if (!h) return SSF_ERR_INVALID_ARG;
    auto refuse = [&](const char* what) { h->err = std::string("ssf_navfloor_fit: ") + what; return SSF_ERR_INVALID_ARG; };
    if (!p) return refuse("params is NULL");
    if (!res) return refuse("the result is NULL");
    auto positive = [](float v) { return std::isfinite(v) && v > 0.0f; };
    NavFloorGate g{};
    if (!nf::unit_up(p->up, g.u)) return refuse("up must be finite and not zero");
    if (p->origin && !(std::isfinite(p->origin[0]) && std::isfinite(p->origin[1]) && std::isfinite(p->origin[2]))) return refuse("origin must be finite");
    if (!(p->tilt_cos > 0.0f) || !(p->tilt_cos < 1.0f)) return refuse("tilt_cos must be in (0, 1)");
    if (!(p->align_cos > 0.0f) || !(p->align_cos <= 1.0f)) return refuse("align_cos must be in (0, 1]");
    if (!positive(p->height_res)) return refuse("height_res must be finite and > 0");
    if (!positive(p->inlier_dist)) return refuse("inlier_dist must be finite and > 0");
    if (!positive(p->first_dist)) return refuse("first_dist must be finite and > 0");
    if (!positive(p->res)) return refuse("res must be finite and > 0");
    if (!positive(p->below)) return refuse("below must be finite and > 0");
    if (!positive(p->step)) return refuse("step must be finite and > 0");
    if (!positive(p->body_height)) return refuse("body_height must be finite and > 0");
    if (p->refine_iters < 0 || p->refine_iters > SSF_NAVFLOOR_MAX_ROUNDS) return refuse("refine_iters must be 0..8");
    if (p->min_rows < 3) return refuse("min_rows must be >= 3");
    if (p->floor_share256 < 1 || p->floor_share256 > 256) return refuse("floor_share256 must be 1..256");
    if (p->width < 1 || p->width > 4096 || p->height < 1 || p->height > 4096) return refuse("the grid's size must be 1..4096 x 1..4096");
    if (p->t_init_min > p->t_init_max || p->t_last_min > p->t_last_max) return refuse("a stamp range has min > max");
    { int rc = model_at_rest(h, "ssf_navfloor_fit", "has no floor fit"); if (rc) return rc; }

    // step 0: the origin and the hint frame
    const float cam[3] = {h->pose.t.x, h->pose.t.y, h->pose.t.z};
    for (int k = 0; k < 3; k++) g.o[k] = p->origin ? p->origin[k] : cam[k];
    if (!nf::hint_frame(g.u, g.a, g.b)) return refuse("up must be finite and not zero");
    g.tilt_cos = p->tilt_cos; g.scale = nf::vote_scale(p->tilt_cos); g.min_conf = p->min_conf;
    g.ti0 = p->t_init_min; g.ti1 = p->t_init_max; g.tl0 = p->t_last_min; g.tl1 = p->t_last_max;
    const float pc[3] = {cam[0] - g.o[0], cam[1] - g.o[1], cam[2] - g.o[2]};

    const ModelView mv = model_view(h, p->visible_only != 0);
    NavFloorWs& w = h->navfloor;
    {
        const size_t slots = std::max<size_t>(mv.nslots, 256);
        bool ok = true;
        if (slots > w.slots) { ok = w.bufs.grow({{(void**)&w.rec, 32 * slots}}); if (ok) w.slots = slots; }
        if (ok && !w.stats) ok = w.bufs.grow({{(void**)&w.stats, NF_STATS * sizeof(unsigned long long)}, {(void**)&w.hist, NF_HIST * sizeof(uint32_t)}});
        if (!ok) { h->err = "ssf_navfloor_fit: allocation of the working buffers failed"; return SSF_ERR_DEVICE; }
    }

    std::memset(res, 0, sizeof(*res));
    res->width = p->width; res->height = p->height; res->res = p->res;
    res->z_min = -p->below; res->floor_max = p->step; res->z_max = p->body_height;
    std::memcpy(res->origin, g.o, sizeof(g.o));
    float normal[3] = {g.u[0], g.u[1], g.u[2]}, d = 0.0f;
    int status = SSF_NAVFLOOR_NO_FLOOR;
    std::vector<uint32_t> hist(NF_HIST, 0u);
    unsigned long long head[4] = {0, 0, 0, 0}, dir[4] = {0, 0, 0, 0}, hgt[2] = {0, 0};

    hipStream_t st = h->stream;
    TimerScope ts(h);
    HCK(hipMemsetAsync(w.stats, 0, NF_STATS * sizeof(unsigned long long), st));
    HCK(hipMemsetAsync(w.hist, 0, NF_HIST * sizeof(uint32_t), st));
    const int nb = mv.nbv + mv.nbo;
    if (nb > 0) {
        ScopedKernel sk("navfloor_prep", st);
        hipLaunchKernelGGL(k_navfloor_prep, dim3(nb), dim3(256), 0, st, mv, g, w.rec, w.hist, w.stats);
    }
    HCK(hipGetLastError());
    HCK(hipMemcpyAsync(head, w.stats, sizeof(head), hipMemcpyDeviceToHost, st));
    HCK(hipMemcpyAsync(hist.data(), w.hist, NF_DIR_HIST * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HCK(hipStreamSynchronize(st));
    res->rows_used = (int64_t)head[NF_ROWS]; res->candidates = (int64_t)head[NF_CAND];
    const uint32_t n = (uint32_t)head[NF_CAND];
    if (head[NF_CURSOR] != head[NF_CAND] || head[NF_CAND] > (unsigned long long)mv.nslots) {
        h->err = "ssf_navfloor_fit: the candidate records do not match their count"; return SSF_ERR_DEVICE;
    }

    int ia0 = 0, ib0 = 0, jstar = 0;
    uint64_t wrows = 0;
    float n0[3];
    bool go = n > 0 && nf::direction_winner(hist.data(), &ia0, &ib0, &wrows);
    if (go) {
        res->dir_bin[0] = ia0; res->dir_bin[1] = ib0;
        { ScopedKernel sk("navfloor_direction", st);
          hipLaunchKernelGGL(k_navfloor_direction, dim3(nf_blocks(n)), dim3(256), 0, st, w.rec, n, ia0, ib0, w.stats); }
        HCK(hipGetLastError());
        HCK(hipMemcpyAsync(dir, w.stats + NF_DIR, sizeof(dir), hipMemcpyDeviceToHost, st));
        HCK(hipStreamSynchronize(st));
        res->direction_rows = (int64_t)dir[0];
        const int64_t S[3] = {(int64_t)dir[1], (int64_t)dir[2], (int64_t)dir[3]};
        go = nf::direction_normal(S, n0);
    }
    NavFloorPlane P{};
    P.align_cos = p->align_cos;
    if (go) {
        std::memcpy(normal, n0, sizeof(n0));
        std::memcpy(P.n, n0, sizeof(n0));
        { ScopedKernel sk("navfloor_height", st);
          hipLaunchKernelGGL(k_navfloor_height, dim3(nf_blocks(n)), dim3(256), 0, st, w.rec, n, P, p->height_res, w.hist + NF_HEIGHT_AT, w.stats); }
        HCK(hipGetLastError());
        HCK(hipMemcpyAsync(hgt, w.stats + NF_ALIGNED, sizeof(hgt), hipMemcpyDeviceToHost, st));
        HCK(hipMemcpyAsync(hist.data() + NF_HEIGHT_AT, w.hist + NF_HEIGHT_AT, NF_HEIGHT_BINS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HCK(hipStreamSynchronize(st));
        res->aligned = (int64_t)hgt[0]; res->height_out_of_range = (int64_t)hgt[1];
        go = nf::height_winner(hist.data() + NF_HEIGHT_AT, p->min_rows, p->floor_share256, &jstar, &wrows);
    }
    if (go) {
        res->height_bin = jstar; res->height_rows = (int64_t)wrows;
        d = nf::height_of_bin(jstar, p->height_res);
        status = SSF_NAVFLOOR_OK;
        for (int k = 0; k < p->refine_iters; k++) {
            std::memcpy(P.n, normal, sizeof(normal));
            P.d = d; P.dist = k == 0 ? p->first_dist : p->inlier_dist;
            if (!nf::frame(normal, g.a, P.a, P.b)) { status = SSF_NAVFLOOR_DEGENERATE; break; }
            unsigned long long* sums = w.stats + NF_ROUND + NF_WORDS * k;
            { ScopedKernel sk("navfloor_refine", st);
              hipLaunchKernelGGL(k_navfloor_refine, dim3(nf_blocks(n)), dim3(256), 0, st, w.rec, n, P, sums); }
            HCK(hipGetLastError());
            HCK(hipMemcpyAsync(res->sums[k], sums, NF_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            HCK(hipStreamSynchronize(st));
            res->inliers[k] = res->sums[k][0];
            float n_new[3], d_new = 0.0f, rms = 0.0f;
            status = nf::refine_round(res->sums[k], p->min_rows, normal, P.a, P.b, d, n_new, &d_new, &rms);
            if (status != SSF_NAVFLOOR_OK) break;
            std::memcpy(normal, n_new, sizeof(normal));
            d = d_new; res->rms[k] = rms; res->rounds = k + 1;
        }
    }
    { int rc = sync_collect(h); if (rc) return rc; }

    res->status = status;
    std::memcpy(res->normal, normal, sizeof(normal));
    res->d = d;
    res->camera_height = nf::camera_height(pc, normal, d);
    if (!nf::grid_pose(normal, d, g.o, pc, g.a, g.b, p->width, p->height, p->res, res->pose)) {
        h->err = "ssf_navfloor_fit: the fitted normal has no frame"; return SSF_ERR_DEVICE;
    }
    if (out && out->dir_hist) std::memcpy(out->dir_hist, hist.data(), NF_DIR_HIST * sizeof(uint32_t));
    if (out && out->height_hist) std::memcpy(out->height_hist, hist.data() + NF_HEIGHT_AT, NF_HEIGHT_BINS * sizeof(uint32_t));
    return SSF_OK;
}
}  // extern "C"
