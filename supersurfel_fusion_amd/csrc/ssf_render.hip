// ssf_render.hip -- the fused model drawn into a virtual pinhole camera (include/ssf_render.h) on gfx950.
//
// Every supersurfel is a flat two-sided elliptical disc; the nearest disc along a pixel's ray wins (no blending).  What is
// computed is pinned, operation by operation, in include/ssf_render.h (the numpy restatement: tests/render_ref.py).  How:
//   * prep   one thread per slot of [visible rows | out-of-view span] (the two stores are read in place, never materialised):
//            live test, culling, the camera-frame record (C, E1, E2, N, num = N.C, dims, rhs = (k dims.x) dims.y) and a
//            CONSERVATIVE pixel box of the disc; every 16 x 16 screen tile the box touches gets one integer atomic count.
//            A slot's number orders like the logical index ([visible | out-of-view], ssf_get_model's order), so the slot
//            number breaks depth ties in the key; the out-of-view rows' logical index comes from an exclusive scan of their
//            live flags (launch_slots_oov_offsets into own scratch: the handle's Counters and d_bc_oov are not
//            touched).  Slot -> row, the rank inside a block and the scan are the helpers of ssf_slots.hpp (k_render_prep).
//   * scan   launch_slots_scan: exclusive scan of the tile counts (one workgroup, 64-bit total); the host reads the total
//            once and sizes the list buffer.
//   * fill   k_render_fill: (tile -> slot) lists with one returning atomic per list entry; the order inside a list is arbitrary.
//   * tile   k_render_tile: one 256-thread workgroup per tile, one pixel per thread: the tile's records are staged through
//            LDS 256 at a time, every thread keeps the minimum key (bits(z) << 32 | slot) in registers, then resolves its outputs (winner's
//            normal from its record, its colour gathered from the store).  The result depends on the integer minimum only:
//            no float atomics, bitwise reproducible for any list order.
// Statistics are exact integers: fragments and filled pixels are summed per workgroup (one 64-bit atomic each); rows_shown
// counts the slots whose `seen` word a winner exchanges from an older render epoch to the current one.
#include "ssf_slots.hpp"
#include "ssf_handle.hpp"

namespace ssf {

// R = 9 floats row-major and t (camera-to-map, ssf_get_pose's layout); ntx x nty tiles of 16 x 16 pixels; k = s * s
struct RenderCam { float R[9], t[3]; float fx, fy, cx, cy; int W, H, ntx, nty; float zmin, zmax, min_conf, s, k; };
struct RenderView { RenderCam cam; ModelView model; };           // one kernel argument: the camera and the rows drawn
struct RenderOut { float* depth; int32_t* index; uint8_t* rgb8; float* color; float* normal; };      // nullptr = not produced

// ---- prep: one thread per slot ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_render_prep(RenderView rv, const uint32_t* __restrict__ bc, float4* __restrict__ rec,
                                                     uint2* __restrict__ rbox, int32_t* __restrict__ logical,
                                                     uint32_t* __restrict__ tcnt) {
    __shared__ int part[4];
    const RenderCam& K = rv.cam;
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    SurfelSoA src; size_t row;
    const bool have = slot_row(rv.model, s, src, row);
    const int lg = slot_logical256(rv.model, have, bc, part);
    uint2 box = make_uint2(1u, 1u);                       // empty: u0 = 1 > u1 = 0
    if (have) {
        const float conf = src.conf[row], dx = src.dims[2 * row], dy = src.dims[2 * row + 1];
        if (conf > K.min_conf && dx > 0.0f && dy > 0.0f && isfinite(dx) && isfinite(dy)) {
            const float* R = K.R;
            const float px = src.pos[3 * row] - K.t[0], py = src.pos[3 * row + 1] - K.t[1], pz = src.pos[3 * row + 2] - K.t[2];
            // C_j = (R0j d.x + R1j d.y) + R2j d.z (contraction off: one IEEE operation each, in this order)
            const float Cx = (R[0] * px + R[3] * py) + R[6] * pz, Cy = (R[1] * px + R[4] * py) + R[7] * pz, Cz = (R[2] * px + R[5] * py) + R[8] * pz;
            const float* r0 = src.r0 + 3 * row; const float* r1 = src.r1 + 3 * row; const float* r2 = src.r2 + 3 * row;
            const float a0 = r0[0], a1 = r0[1], a2 = r0[2], b0 = r1[0], b1 = r1[1], b2 = r1[2], n0 = r2[0], n1 = r2[1], n2 = r2[2];
            const float E1x = (R[0] * a0 + R[3] * a1) + R[6] * a2, E1y = (R[1] * a0 + R[4] * a1) + R[7] * a2, E1z = (R[2] * a0 + R[5] * a1) + R[8] * a2;
            const float E2x = (R[0] * b0 + R[3] * b1) + R[6] * b2, E2y = (R[1] * b0 + R[4] * b1) + R[7] * b2, E2z = (R[2] * b0 + R[5] * b1) + R[8] * b2;
            const float Nx = (R[0] * n0 + R[3] * n1) + R[6] * n2, Ny = (R[1] * n0 + R[4] * n1) + R[7] * n2, Nz = (R[2] * n0 + R[5] * n1) + R[8] * n2;
            // a non-finite C or N gives no candidate pixel at all (z is then NaN, infinite or 0: include/ssf_render.h)
            if (finite3(Cx, Cy, Cz) && finite3(Nx, Ny, Nz)) {
                int u0 = 0, u1 = K.W - 1, v0 = 0, v1 = K.H - 1;
                bool cull = false;
                if (finite3(E1x, E1y, E1z) && finite3(E2x, E2y, E2z)) {
                    // Conservative box.  A candidate's hit point P = (z qx, z qy, z) has z_min <= P.z <= z_max, lies in the
                    // disc's plane up to ~1e-7 z (rounding of z = num / den) and inside its ellipse up to the rounding of the
                    // inside test: the disc's axis-aligned extent widened by 1e-3 relative + 1e-5 of |C| + hx + hy covers it,
                    // and the projection of that box (clipped to [z_min, z_max]) plus 2 pixels covers its pixels.
                    const float hx = K.s * sqrtf(dx), hy = K.s * sqrtf(dy);
                    const float slack = 1e-5f * (fabsf(Cx) + fabsf(Cy) + fabsf(Cz) + hx + hy) + 1e-6f;
                    const float ex = sqrtf((E1x * hx) * (E1x * hx) + (E2x * hy) * (E2x * hy)) * 1.001f + slack;
                    const float ey = sqrtf((E1y * hx) * (E1y * hx) + (E2y * hy) * (E2y * hy)) * 1.001f + slack;
                    const float ez = sqrtf((E1z * hx) * (E1z * hx) + (E2z * hy) * (E2z * hy)) * 1.001f + slack;
                    const float z0 = fmaxf(Cz - ez, K.zmin), z1 = fminf(Cz + ez, K.zmax);
                    if (!(z0 <= z1)) cull = true;
                    else {
                        const float xl = Cx - ex, xh = Cx + ex, yl = Cy - ey, yh = Cy + ey;
                        const float sxl = fminf(xl / z0, xl / z1), sxh = fmaxf(xh / z0, xh / z1);
                        const float syl = fminf(yl / z0, yl / z1), syh = fmaxf(yh / z0, yh / z1);
                        const float ua = K.fx * sxl + K.cx, ub = K.fx * sxh + K.cx, va = K.fy * syl + K.cy, vb = K.fy * syh + K.cy;
                        const float ulo = fminf(ua, ub) - 2.0f, uhi = fmaxf(ua, ub) + 2.0f, vlo = fminf(va, vb) - 2.0f, vhi = fmaxf(va, vb) + 2.0f;
                        if (!(uhi >= 0.0f) || !(ulo <= (float)(K.W - 1)) || !(vhi >= 0.0f) || !(vlo <= (float)(K.H - 1))) cull = true;
                        else {
                            u0 = (int)floorf(fmaxf(ulo, 0.0f)); u1 = (int)ceilf(fminf(uhi, (float)(K.W - 1)));
                            v0 = (int)floorf(fmaxf(vlo, 0.0f)); v1 = (int)ceilf(fminf(vhi, (float)(K.H - 1)));
                        }
                    }
                }   // (a non-finite in-plane axis: the whole image, the tile pass decides)
                if (!cull) {
                    const float num = (Nx * Cx + Ny * Cy) + Nz * Cz;
                    const float rhs = (K.k * dx) * dy;
                    float4* o = rec + 4 * (size_t)s;
                    o[0] = make_float4(Cx, Cy, Cz, num);
                    o[1] = make_float4(E1x, E1y, E1z, dy);
                    o[2] = make_float4(E2x, E2y, E2z, dx);
                    o[3] = make_float4(Nx, Ny, Nz, rhs);
                    logical[s] = lg;
                    box = make_uint2((uint32_t)u0 | ((uint32_t)u1 << 16), (uint32_t)v0 | ((uint32_t)v1 << 16));
                    for (int ty = v0 >> 4; ty <= (v1 >> 4); ty++)
                        for (int tx = u0 >> 4; tx <= (u1 >> 4); tx++) atomicAdd(&tcnt[ty * K.ntx + tx], 1u);
                }
            }
        }
    }
    if ((int)s < rv.model.nslots) rbox[s] = box;
}

// ---- fill: the (tile -> slot) lists -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_render_fill(RenderView rv, const uint2* __restrict__ rbox, uint32_t* __restrict__ cursor,
                                                     uint32_t* __restrict__ list) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if ((int)s >= rv.model.nslots) return;
    const uint2 b = rbox[s];
    const int u0 = b.x & 0xFFFF, u1 = b.x >> 16, v0 = b.y & 0xFFFF, v1 = b.y >> 16;
    if (u0 > u1 || v0 > v1) return;
    for (int ty = v0 >> 4; ty <= (v1 >> 4); ty++)
        for (int tx = u0 >> 4; tx <= (u1 >> 4); tx++) list[atomicAdd(&cursor[ty * rv.cam.ntx + tx], 1u)] = s;
}

// ---- tile: one workgroup per 16 x 16 tile, one pixel per thread -------------------------------------------------------
__global__ __launch_bounds__(256) void k_render_tile(RenderView rv, const float4* __restrict__ rec, const uint2* __restrict__ rbox,
                                                     const int32_t* __restrict__ logical, const uint32_t* __restrict__ list,
                                                     const uint32_t* __restrict__ toff, RenderOut out, uint32_t* __restrict__ seen,
                                                     uint32_t epoch, unsigned long long* __restrict__ stats) {
    __shared__ float4 sr[4 * 256];
    __shared__ uint2 sb[256];
    __shared__ uint32_t ss[256];
    __shared__ unsigned long long red[3][4];
    const RenderCam& K = rv.cam;
    const int t = blockIdx.x, tx = t % K.ntx, ty = t / K.ntx;
    const int u = tx * 16 + (threadIdx.x & 15), v = ty * 16 + (threadIdx.x >> 4);
    const bool inimg = u < K.W && v < K.H;
    const float qx = ((float)u - K.cx) / K.fx, qy = ((float)v - K.cy) / K.fy;
    const uint32_t uv = (uint32_t)u | ((uint32_t)v << 16);
    unsigned long long best = ~0ull;
    uint32_t frag = 0;
    const uint32_t beg = toff[t], end = toff[t + 1];
    for (uint32_t c0 = beg; c0 < end; c0 += 256) {
        const int n = (int)min(256u, end - c0);
        if ((int)threadIdx.x < n) {
            const uint32_t s = list[c0 + threadIdx.x];
            const float4* r = rec + 4 * (size_t)s;
            sr[4 * threadIdx.x] = r[0]; sr[4 * threadIdx.x + 1] = r[1]; sr[4 * threadIdx.x + 2] = r[2]; sr[4 * threadIdx.x + 3] = r[3];
            sb[threadIdx.x] = rbox[s]; ss[threadIdx.x] = s;
        }
        __syncthreads();
        for (int j = 0; j < n; j++) {
            const uint2 b = sb[j];
            // inside the record's pixel box: u0 <= u <= u1 and v0 <= v <= v1 (16-bit fields, no borrow across them)
            if ((uv & 0xFFFF) < (b.x & 0xFFFF) || (uv & 0xFFFF) > (b.x >> 16) || (uv >> 16) < (b.y & 0xFFFF) || (uv >> 16) > (b.y >> 16)) continue;
            const float4 A = sr[4 * j], B = sr[4 * j + 1], Cc = sr[4 * j + 2], D = sr[4 * j + 3];
            const float den = (D.x * qx + D.y * qy) + D.z;
            const float z = A.w / den;
            if (!(den != 0.0f) || !isfinite(z) || !(z >= K.zmin) || !(z <= K.zmax)) continue;
            const float Px = z * qx, Py = z * qy;
            const float dx = Px - A.x, dy = Py - A.y, dz = z - A.z;
            const float a = (dx * B.x + dy * B.y) + dz * B.z;
            const float bb = (dx * Cc.x + dy * Cc.y) + dz * Cc.z;
            if (!((a * a) * B.w + (bb * bb) * Cc.w <= D.w)) continue;
            frag++;
            const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | ss[j];
            best = key < best ? key : best;
        }
        __syncthreads();
    }
    uint32_t filled = 0, shown = 0;
    if (inimg) {
        const size_t p = (size_t)v * K.W + u;
        float z = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, m0 = 0.0f, m1 = 0.0f, m2 = 0.0f;
        int32_t lg = -1;
        if (best != ~0ull) {
            const uint32_t s = (uint32_t)best;
            z = __uint_as_float((uint32_t)(best >> 32));
            const float4 D = rec[4 * (size_t)s + 3];
            const float den = (D.x * qx + D.y * qy) + D.z;
            m0 = den > 0.0f ? -D.x : D.x; m1 = den > 0.0f ? -D.y : D.y; m2 = den > 0.0f ? -D.z : D.z;
            lg = logical[s];
            SurfelSoA src; size_t row;
            (void)slot_row(rv.model, s, src, row);
            c0 = src.col[3 * row]; c1 = src.col[3 * row + 1]; c2 = src.col[3 * row + 2];
            filled = 1;
            if (atomicExch(&seen[s], epoch) != epoch) shown = 1;
        }
        if (out.depth) out.depth[p] = z;
        if (out.index) out.index[p] = lg;
        if (out.color) { out.color[3 * p] = c0; out.color[3 * p + 1] = c1; out.color[3 * p + 2] = c2; }
        if (out.rgb8) {
            out.rgb8[3 * p] = (uint8_t)fminf(255.0f, fmaxf(0.0f, rintf(c0)));
            out.rgb8[3 * p + 1] = (uint8_t)fminf(255.0f, fmaxf(0.0f, rintf(c1)));
            out.rgb8[3 * p + 2] = (uint8_t)fminf(255.0f, fmaxf(0.0f, rintf(c2)));
        }
        if (out.normal) { out.normal[3 * p] = m0; out.normal[3 * p + 1] = m1; out.normal[3 * p + 2] = m2; }
    }
    const unsigned long long f = wave_sum<unsigned long long>(frag), fl = wave_sum<unsigned long long>(filled), sh = wave_sum<unsigned long long>(shown);
    if (lane() == 0) { red[0][threadIdx.x >> 6] = f; red[1][threadIdx.x >> 6] = fl; red[2][threadIdx.x >> 6] = sh; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned long long sum = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        if (sum) atomicAdd(&stats[threadIdx.x], sum);
    }
}

// ---- launches -------------------------------------------------------------------------------------------------------
// prep (+ the out-of-view live scan into bc[nbo + 1]) and the exclusive scan of the tile counts: tcnt[ntiles + 1] (zeroed by the
// caller) becomes the list offsets, cursor[ntiles] a copy; *total = list entries (64 bits)
static void launch_render_prep(hipStream_t st, const RenderView& rv, uint32_t* bc, float4* rec, uint2* rbox, int32_t* logical, uint32_t* tcnt,
                               uint32_t* cursor, unsigned long long* total) {
    ScopedKernel sk("render_prep", st);
    const ModelView& mv = rv.model;
    launch_slots_oov_offsets(st, mv, bc);
    if (mv.nbv + mv.nbo > 0)
        hipLaunchKernelGGL(k_render_prep, dim3(mv.nbv + mv.nbo), dim3(256), 0, st, rv, bc, rec, rbox, logical, tcnt);
    launch_slots_scan(st, tcnt, rv.cam.ntx * rv.cam.nty, cursor, total);
}
static void launch_render_fill(hipStream_t st, const RenderView& rv, const uint2* rbox, uint32_t* cursor, uint32_t* list) {
    ScopedKernel sk("render_fill", st);
    if (rv.model.nslots > 0) hipLaunchKernelGGL(k_render_fill, dim3(rv.model.nslots / 256), dim3(256), 0, st, rv, rbox, cursor, list);
}
// stats[0..2] += fragments, filled pixels, rows shown (seen[slot] != epoch before this render)
static void launch_render_tile(hipStream_t st, const RenderView& rv, const float4* rec, const uint2* rbox, const int32_t* logical,
                               const uint32_t* list, const uint32_t* toff, const RenderOut& out, uint32_t* seen, uint32_t epoch,
                               unsigned long long* stats) {
    ScopedKernel sk("render_tile", st);
    hipLaunchKernelGGL(k_render_tile, dim3(rv.cam.ntx * rv.cam.nty), dim3(256), 0, st, rv, rec, rbox, logical, list, toff, out, seen,
                       epoch, stats);
}

}  // namespace ssf

// ---- host: the entry points of include/ssf_render.h ------------------------------------------------------------------------
extern "C" {
int ssf_render_default_params(const ssf_handle* h, ssf_render_params* p) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    std::memset(p, 0, sizeof(*p));
    p->width = h->cam.W; p->height = h->cam.H; p->fx = h->cam.fx; p->fy = h->cam.fy; p->cx = h->cam.cx; p->cy = h->cam.cy;
    p->z_min = h->cfg.range_min; p->z_max = h->cfg.range_max; p->min_conf = 0.0f; p->splat_scale = 3.0f;
    return SSF_OK;
}

int ssf_render_model(ssf_handle* h, const ssf_render_params* p, float* depth, int32_t* index, uint8_t* rgb8, float* color,
                     float* normal, ssf_render_stats* stats) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    if (!depth && !index && !rgb8 && !color && !normal) { h->err = "ssf_render_model: every output is NULL"; return SSF_ERR_INVALID_ARG; }
    { int rc = model_at_rest(h, "ssf_render_model", "is not rendered"); if (rc) return rc; }
    RenderCam K;
    const Rt T = p->pose ? pose_from12(p->pose) : h->pose;
    const float R9[9] = {T.R.r0.x, T.R.r0.y, T.R.r0.z, T.R.r1.x, T.R.r1.y, T.R.r1.z, T.R.r2.x, T.R.r2.y, T.R.r2.z};
    std::memcpy(K.R, R9, sizeof(R9)); K.t[0] = T.t.x; K.t[1] = T.t.y; K.t[2] = T.t.z;
    if (p->width == 0) { K.W = h->cam.W; K.H = h->cam.H; K.fx = h->cam.fx; K.fy = h->cam.fy; K.cx = h->cam.cx; K.cy = h->cam.cy; }
    else { K.W = p->width; K.H = p->height; K.fx = p->fx; K.fy = p->fy; K.cx = p->cx; K.cy = p->cy; }
    if (K.W < 1 || K.W > 4096 || K.H < 1 || K.H > 4096) { h->err = "ssf_render_model: the camera size must be 1..4096 x 1..4096"; return SSF_ERR_INVALID_ARG; }
    if (!std::isfinite(K.fx) || !std::isfinite(K.fy) || K.fx == 0.0f || K.fy == 0.0f) { h->err = "ssf_render_model: fx and fy must be finite and non-zero"; return SSF_ERR_INVALID_ARG; }
    K.zmin = p->z_min; K.zmax = p->z_max;
    if (K.zmin == 0.0f && K.zmax == 0.0f) { K.zmin = h->cfg.range_min; K.zmax = h->cfg.range_max; }
    if (!(K.zmin > 0.0f) || !(K.zmax > K.zmin)) { h->err = "ssf_render_model: the depth range needs 0 < z_min < z_max"; return SSF_ERR_INVALID_ARG; }
    K.s = p->splat_scale == 0.0f ? 3.0f : p->splat_scale;
    if (!(K.s >= 0.0f) || !std::isfinite(K.s)) { h->err = "ssf_render_model: splat_scale must be finite and >= 0"; return SSF_ERR_INVALID_ARG; }
    K.k = K.s * K.s; K.min_conf = p->min_conf;
    K.ntx = (K.W + 15) / 16; K.nty = (K.H + 15) / 16;
    const int ntiles = K.ntx * K.nty;

    const RenderView rv{K, model_view(h, p->visible_only != 0)};

    RenderWs& w = h->render;
    const size_t P = (size_t)K.W * K.H;
    RenderOut o{depth, index, rgb8, color, normal};
    StagedIo io;                                                     // host outputs are staged on the device
    if (!p->on_device) {
        io.out(depth, 4 * P, &o.depth); io.out(index, 4 * P, &o.index); io.out(rgb8, 3 * P, &o.rgb8);
        io.out(color, 12 * P, &o.color); io.out(normal, 12 * P, &o.normal);
    }
    const size_t slots = std::max<size_t>(rv.model.nslots, 256);
    bool ok = true;
    if (ok && slots > w.slots) {
        ok = w.bufs.grow({{(void**)&w.rec, 64 * slots}, {(void**)&w.rbox, 8 * slots}, {(void**)&w.logical, 4 * slots},
                          {(void**)&w.seen, 4 * slots}, {(void**)&w.bc, 4 * (slots / 256 + 1)}});
        if (ok) { w.slots = slots; w.epoch = 0; HCK(hipMemsetAsync(w.seen, 0, 4 * slots, h->stream)); }
    }
    if (ok) ok = w.tl.reserve_bins(w.bufs, (size_t)ntiles);
    if (ok && !w.stats) ok = w.bufs.grow({{(void**)&w.stats, 4 * sizeof(unsigned long long)}});
    if (ok) ok = io.reserve(w.bufs, &w.img, &w.img_bytes, io.need());
    if (!ok) { h->err = "ssf_render_model: allocation of the working buffers failed"; return SSF_ERR_DEVICE; }
    if (++w.epoch == 0) { HCK(hipMemsetAsync(w.seen, 0, 4 * w.slots, h->stream)); w.epoch = 1; }

    TimerScope ts(h);
    hipStream_t st = h->stream;
    HCK(hipMemsetAsync(w.tl.off, 0, 4 * ((size_t)ntiles + 1), st));
    HCK(hipMemsetAsync(w.stats, 0, 4 * sizeof(unsigned long long), st));
    launch_render_prep(st, rv, w.bc, w.rec, w.rbox, w.logical, w.tl.off, w.tl.cursor, w.stats + 3);
    HCK(hipGetLastError());
    unsigned long long total = 0;
    HCK(hipMemcpyAsync(&total, w.stats + 3, sizeof(total), hipMemcpyDeviceToHost, st));
    HCK(hipStreamSynchronize(st));
    { int rc = w.tl.reserve_list(w.bufs, total, h->err, "ssf_render_model: more than 2^32 - 1 (tile, row) list entries",
                                 "ssf_render_model: allocation of ", " bytes for the tile lists failed"); if (rc) return rc; }
    if (total > 0) { launch_render_fill(st, rv, w.rbox, w.tl.cursor, w.tl.list); HCK(hipGetLastError()); }
    launch_render_tile(st, rv, w.rec, w.rbox, w.logical, w.tl.list, w.tl.off, o, w.seen, w.epoch, w.stats);
    HCK(hipGetLastError());
    unsigned long long st3[3] = {0, 0, 0};
    HCK(hipMemcpyAsync(st3, w.stats, sizeof(st3), hipMemcpyDeviceToHost, st));
    HCK(io.copy_out(st));
    { int rc = sync_collect(h); if (rc) return rc; }
    if (stats) { stats->fragments = (int64_t)st3[0]; stats->pixels_filled = (int64_t)st3[1]; stats->rows_shown = (int64_t)st3[2]; stats->list_entries = (int64_t)total; }
    return SSF_OK;
}
}  // extern "C"
