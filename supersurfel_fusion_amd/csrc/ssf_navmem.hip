// ssf_navmem.hip -- the live layer with memory (include/ssf_navmem.h) on gfx950: the depth frame stamped into height slices of the
// obstacle band, cleared by the rays that see through a slice, aged by the caller's tick.
//
// What is computed is pinned, operation by operation, in include/ssf_navmem.h (the numpy restatement: tests/navmem_ref.py).
//   * stamp   k_navmem_stamp: the overlay's tile (ssf_navlive.hpp: the tile pixel, its point, the transpose, the run heads -- the SAME
//             code as k_navlive_stamp runs, not a copy) with a second LDS plane for the pixel's slice bit.  The run's bits are OR-ed
//             down to its head (a segmented OR over the wave), and the head issues ONE atomicAdd of the run's length and ONE atomicOr
//             of the run's bits.  The cell and the height come from one nav_grid_point (ssf_navgrid.hpp).
//   * march   k_navmem_march: the overlay's rays (navlive_wave_rays, ssf_navlive.hpp: one ray per wave, NL_RUN consecutive lattice pixels
//             per wave) with this file's march of a ray.  Every accepted sample yields (cell, bit); consecutive lanes in one cell are OR-reduced to
//             their run head, what lane 63's run issued is carried into the next round of 64, and what consecutive rays give the first
//             cells stays merged in registers (pend_cell, pend_bits).  A head issues an atomicOr whose value nobody reads.
//   * cells   k_navmem_cells: one thread per cell: the layer, the state and the cell stats (steps 4 and 5);
// then the clearance of ssf_navgrid.hip (navgrid_columns, navgrid_rows) on that state.  Its working set is NavMemWs (ssf_handle.hpp).
// No result depends on a merge: a rolled camera merges less and counts the same.
//
// This file is NOT one of the product library's objects, nor of the ten older libraries: it is linked with libssf_hip_dyn.so's objects
// into libssf_hip_mem.so (csrc/Makefile), which is what a caller of the update loads.
#include "ssf_navlive.hpp"
#include "../../include/ssf_navmem.h"

namespace ssf {

// the sums the host reads (the unknown cells are the rest of the grid).  Every workgroup adds to them, so each sum has a 128-byte line
// of its own: sum k is word k * NM_PAD (a kernel's sums are consecutive, as block_sums wants them)
enum { NM_VALID = 0, NM_STAMPING, NM_POINTS, NM_STAMP_ATOMICS, NM_CARVING, NM_SAMPLES, NM_MARCH_ATOMICS, NM_RAYS, NM_MARKED, NM_NEWLY, NM_CLEARED,
       NM_EXPIRED, NM_BITS, NM_REMEMBERED, NM_OPENED, NM_FREE, NM_OCC, NM_STATS = 17, NM_PAD = 16 };

// the band cut into slices (ssf_navmem.h step 2)
struct NavMemSlices { float floor_max, slice_h; int top; };          // top = slices - 1

// the bit of the slice that holds the band height z (z > floor_max, so the quotient is >= 0)
__device__ __forceinline__ uint32_t navmem_slice_bit(const NavMemSlices& S, float z) {
    const float q = (z - S.floor_max) / S.slice_h;
    const int k = min(S.top, (int)floorf(q));
    return 1u << k;
}
// the OR of v over the lanes from this one to the end of its run; heads: the ballot of run heads (nav_run_head, ssf_navlive.hpp).
// What a head gets is its whole run's.
__device__ __forceinline__ uint32_t navmem_run_or(uint32_t v, unsigned long long heads) {
    const int len = nav_run_len(heads);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_down(v, d, 64);
        if (d < len) v |= o;                                          // lane ln + d is still of this run
    }
    return v;
}

// ---- stamp: steps 1 to 3 ---------------------------------------------------------------------------------------------------
template <int DF>
__global__ __launch_bounds__(256) void k_navmem_stamp(NavGrid G, NavLiveCam cam, NavMemSlices S, const void* __restrict__ depth, double scale,
                                                      const uint8_t* __restrict__ mask, int mask_mode, uint32_t* __restrict__ hits,
                                                      uint32_t* __restrict__ hit_bits, unsigned long long* __restrict__ stats) {
    __shared__ int s_cell[NL_TILE_LDS];
    __shared__ uint32_t s_bit[NL_TILE_LDS];
    int c = -1;
    uint32_t b = 0u;
    bool valid, stamping;
    float Sx, Sy, Sz, z;
    if (navlive_tile_point<DF>(cam, depth, scale, mask, mask_mode, valid, stamping, Sx, Sy, Sz)) {
        c = nav_cell(G, Sx, Sy, Sz, z);
        if (c >= 0) b = navmem_slice_bit(S, z);
    }
    const int w = navlive_tile_put(), r = navlive_tile_get();
    s_cell[w] = c; s_bit[w] = b;
    __syncthreads();
    const int cc = s_cell[r];
    unsigned long long heads, n_atomics = 0;
    const bool head = nav_run_head(cc, heads);
    const uint32_t bits = navmem_run_or(s_bit[r], heads);
    if (head && cc >= 0) {
        atomicAdd(&hits[cc], (uint32_t)nav_run_len(heads));
        atomicOr(&hit_bits[cc], bits);
        n_atomics = 2;
    }
    block_sums({valid, stamping, c >= 0, n_atomics}, stats, NM_VALID, NM_PAD);
}

// ---- march: the samples of step 1 into the seen bits of step 3 -----------------------------------------------------------------
// one run head's bits into seen[c].  (OR only grows within a call, so a plain load that already shows the bits could spare the atomic.
// That arm was built and measured: it spared two atomics in three and no time, profiles/navmem.txt, and was taken out again.)
__device__ __forceinline__ void navmem_or(uint32_t* __restrict__ seen, int c, uint32_t bits, unsigned long long& n_atomics) {
    atomicOr(&seen[c], bits);
    n_atomics++;
}
// The march of ONE RAY BY ONE WAVE, nav_march_ray's sibling (ssf_navgrid.hpp): samples m = 0 .. M over the lanes, m = lane, lane + 64, ...
// A lane whose sample is accepted holds (cell, bit); a run of lanes with one cell is OR-reduced to its head.  carry: the cell and the
// bits of the run that held lane 63 in the round before, as its head had them -- they are issued or pending, so a run at lane 0 that
// continues that cell with no new bit has nothing to add.  Round 0's heads go through the lane's pending pair, which lives across
// the wave's rays; the caller issues the last one.
__device__ __forceinline__ void navmem_march_ray(const NavGrid& G, const NavMemSlices& S, const NavMarchRay& r, int M, uint32_t* __restrict__ seen,
                                                 int& pend_cell, uint32_t& pend_bits, unsigned long long& n_atomics) {
    const int ln = lane();
    int carry_cell = -1; uint32_t carry_bits = 0u;
    for (int base = 0; base <= M; base += 64) {
        const int m = base + ln;
        int c = -1; uint32_t b = 0u;
        if (m <= M) {
            float z;
            c = nav_sample_cell(G, r, m, z);
            if (c >= 0) b = navmem_slice_bit(S, z);
        }
        unsigned long long heads;
        const bool head = nav_run_head(c, heads);
        const uint32_t bits = navmem_run_or(b, heads);
        const bool covered = ln == 0 && c == carry_cell && (bits & ~carry_bits) == 0u;
        const int last_head = 63 - __builtin_clzll(heads);             // the head of the run that holds lane 63 (heads != 0: lane 0)
        carry_cell = __shfl(c, last_head, 64);
        carry_bits = __shfl(covered ? carry_bits : bits, last_head, 64);
        if (head && c >= 0 && !covered) {
            if (base == 0) {
                if (c == pend_cell) pend_bits |= bits;
                else {
                    if (pend_bits) navmem_or(seen, pend_cell, pend_bits, n_atomics);
                    pend_cell = c; pend_bits = bits;
                }
            } else navmem_or(seen, c, bits, n_atomics);
        }
    }
}

template <int DF>
__global__ __launch_bounds__(256) void k_navmem_march(NavGrid G, NavLiveCam cam, NavMemSlices S, const void* __restrict__ depth, double scale, float margin,
                                                      uint32_t* __restrict__ seen, unsigned long long* __restrict__ stats) {
    unsigned long long n_atomics = 0;
    int pend_cell = -1; uint32_t pend_bits = 0u;
    const NavRayCounts n = navlive_wave_rays<DF>(G.step, cam, depth, scale, margin, [&](const NavMarchRay& r, int M) {
        navmem_march_ray(G, S, r, M, seen, pend_cell, pend_bits, n_atomics);
    });
    if (pend_bits) navmem_or(seen, pend_cell, pend_bits, n_atomics);
    // the sums of the workgroup's four waves (rays and samples: one lane speaks for its wave)
    const bool one = lane() == 0;
    block_sums({one ? n.carving : 0ull, one ? n.samples : 0ull, n_atomics, one ? n.rays : 0ull}, stats, NM_CARVING, NM_PAD);
}

// ---- cells: steps 4 and 5 and the cell stats; one thread per cell -------------------------------------------------------------
// an input of the layer may be nullptr (all zero); each input and its output may be one array, and so may state_in and out_state (a
// thread reads its cell before it writes it)
struct NavMemRule { int min_hits, open_unknown; uint32_t tick, max_mark_age, max_seen_age; };
struct NavMemCellsIo {
    const int8_t* state_in; const uint32_t* marks_in; const uint32_t* mark_tick_in; const uint32_t* seen_tick_in;
    const uint32_t* hits; const uint32_t* hit_bits; const uint32_t* seen_bits;
    uint32_t* marks; uint32_t* mark_tick; uint32_t* seen_tick; uint32_t* out_hits; uint32_t* out_hit_bits; uint32_t* out_seen_bits; int8_t* state;
};
__global__ __launch_bounds__(256) void k_navmem_cells(size_t P, NavMemRule rule, NavMemCellsIo io, unsigned long long* __restrict__ stats) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long nmarked = 0, nnewly = 0, ncleared = 0, nexpired = 0, nbits = 0, nremembered = 0, nopened = 0, nfree = 0, nocc = 0;
    if (p < P) {
        const int8_t in = io.state_in[p];
        const uint32_t m_in = io.marks_in ? io.marks_in[p] : 0u, mt_in = io.mark_tick_in ? io.mark_tick_in[p] : 0u;
        const uint32_t st_in = io.seen_tick_in ? io.seen_tick_in[p] : 0u;
        const uint32_t nh = io.hits[p], hbits = io.hit_bits[p], sb = io.seen_bits[p];
        const uint32_t hb = nh >= (uint32_t)rule.min_hits ? hbits : 0u;
        uint32_t m = (m_in & ~sb) | hb;
        uint32_t mt = hb ? rule.tick : mt_in;
        ncleared = m_in != 0u && m == 0u;
        nbits = (unsigned long long)__popc(m_in & sb & ~hb);
        if (m != 0u && rule.max_mark_age > 0u && rule.tick - mt > rule.max_mark_age) { m = 0u; nexpired = 1; }
        if (m == 0u) mt = 0u;
        uint32_t st = sb ? rule.tick : st_in;
        if (st != 0u && rule.max_seen_age > 0u && rule.tick - st > rule.max_seen_age) st = 0u;
        int8_t s = (int8_t)-1;
        if (in == 100 || m != 0u) s = (int8_t)100;
        else if (in == 0 || (rule.open_unknown && st != 0u)) s = (int8_t)0;
        nmarked = m != 0u; nnewly = m != 0u && m_in == 0u;
        nremembered = s == 100 && in != 100 && hb == 0u;
        nopened = in != 100 && in != 0 && s == 0;
        nocc = s == 100; nfree = s == 0;
        if (io.marks) io.marks[p] = m;
        if (io.mark_tick) io.mark_tick[p] = mt;
        if (io.seen_tick) io.seen_tick[p] = st;
        if (io.out_hits) io.out_hits[p] = nh;
        if (io.out_hit_bits) io.out_hit_bits[p] = hbits;
        if (io.out_seen_bits) io.out_seen_bits[p] = sb;
        if (io.state) io.state[p] = s;
    }
    block_sums({nmarked, nnewly, ncleared, nexpired, nbits, nremembered, nopened, nfree, nocc}, stats, NM_MARKED, NM_PAD);
}

static void launch_navmem_stamp(hipStream_t st, int df, const NavGrid& G, const NavLiveCam& cam, const NavMemSlices& S, const void* depth, double scale,
                                const uint8_t* mask, int mask_mode, uint32_t* hits, uint32_t* hit_bits, unsigned long long* stats) {
    ScopedKernel sk("navmem_stamp", st);
    navlive_by_depth_format(df, [&](auto DF) {
        hipLaunchKernelGGL(k_navmem_stamp<decltype(DF)::value>, dim3(navlive_tiles(cam.W, cam.H)), dim3(256), 0, st, G, cam, S, depth, scale, mask, mask_mode, hits,
                           hit_bits, stats);
    });
}
static void launch_navmem_march(hipStream_t st, int df, const NavGrid& G, const NavLiveCam& cam, const NavMemSlices& S, const void* depth, double scale,
                                float margin, uint32_t* seen, unsigned long long* stats) {
    ScopedKernel sk("navmem_march", st);
    navlive_by_depth_format(df, [&](auto DF) {
        hipLaunchKernelGGL(k_navmem_march<decltype(DF)::value>, dim3(navlive_march_groups(cam)), dim3(256), 0, st, G, cam, S, depth, scale, margin, seen, stats);
    });
}
static void launch_navmem_cells(hipStream_t st, size_t P, const NavMemRule& rule, const NavMemCellsIo& io, unsigned long long* stats) {
    ScopedKernel sk("navmem_cells", st);
    hipLaunchKernelGGL(k_navmem_cells, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, P, rule, io, stats);
}

}  // namespace ssf

extern "C" {
int ssf_navmem_default_params(const ssf_handle* h, ssf_navmem_params* p) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    { int rc = navlive_default_fields(h, p); if (rc) return rc; }
    p->slices = 16; p->tick = 1u; p->max_mark_age = 0u; p->max_seen_age = 0u;
    return SSF_OK;
}

int ssf_navmem_update(ssf_handle* h, const ssf_navmem_params* p, const void* depth, const uint8_t* mask, const int8_t* state_in,
                      const ssf_navmem_layer* layer_in, const ssf_navmem_out* out, ssf_navmem_stats* stats) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    auto refuse = [&](const char* what) { h->err = std::string("ssf_navmem_update: ") + what; return SSF_ERR_INVALID_ARG; };
    if (!depth) return refuse("depth is NULL");
    if (!state_in) return refuse("state_in is NULL");
    if (!out || (!out->marks && !out->mark_tick && !out->seen_tick && !out->live_hits && !out->hit_bits && !out->seen_bits && !out->state && !out->dist2))
        return refuse("every output is NULL");
    // the grid, the memory's own slices, the camera and its lattice (ssf_navlive.hpp: shared with ssf_navlive_overlay)
    ssf_navgrid_params g;
    if (const char* what = navlive_refuse_grid(h, p, g)) return refuse(what);
    if (p->tick == 0u) return refuse("tick must be >= 1");
    if (p->slices < 1 || p->slices > 32) return refuse("slices must be 1..32");
    if (!std::isfinite(p->floor_max) || !std::isfinite(p->z_max)) return refuse("floor_max and z_max must be finite");
    if (!(p->z_max > p->floor_max)) return refuse("z_max must be > floor_max");
    const float slice_h = (p->z_max - p->floor_max) / (float)p->slices;
    if (!std::isfinite(slice_h) || !(slice_h > 0.0f)) return refuse("(z_max - floor_max) / slices must be finite and > 0");
    NavLiveCam cam{};
    size_t bpp = 0;
    if (const char* what = navlive_refuse_camera(h, p, depth, mask, nullptr, cam, bpp)) return refuse(what);
    const int df = h->in_depth;
    const size_t P = (size_t)p->width * p->height, npix = (size_t)cam.W * cam.H;
    const bool dev = p->on_device != 0, fdev = p->frame_on_device != 0;
    const ssf_navmem_layer none{nullptr, nullptr, nullptr};
    const ssf_navmem_layer& L = layer_in ? *layer_in : none;
    // overlaps: the outputs among themselves and with the inputs that live in the same memory; an output of the layer on its own
    // input and state == state_in are the update in place
    {
        const void* a[14] = {out->marks, out->mark_tick, out->seen_tick, out->live_hits, out->hit_bits, out->seen_bits, out->state, out->dist2,
                             L.marks, L.mark_tick, L.seen_tick, state_in, depth, p->mask_mode ? mask : nullptr};
        const size_t n[14] = {4 * P, 4 * P, 4 * P, 4 * P, 4 * P, 4 * P, P, 4 * P, 4 * P, 4 * P, 4 * P, P, bpp * npix, npix};
        const int may[4][2] = {{0, 8}, {1, 9}, {2, 10}, {6, 11}};
        if (navlive_arrays_overlap(a, n, 14, 8, 12, dev != fdev, may, 4))
            return refuse("arrays overlap (only an output of the layer on its own input, and state == state_in, may)");
    }
    { int rc = model_at_rest(h, "ssf_navmem_update", "updates no layer"); if (rc) return rc; }

    float gpose[12];
    NavGrid G{};
    { int rc = navlive_frames(h, &g, p, p->res * 0.5f, G, cam, gpose); if (rc) return rc; }
    const NavMemSlices S{p->floor_max, slice_h, p->slices - 1};

    // the arrays: host ones are staged on the device
    const void* d_depth = depth; const uint8_t* d_mask = p->mask_mode ? mask : nullptr;
    NavMemCellsIo c{};
    c.state_in = state_in; c.marks_in = L.marks; c.mark_tick_in = L.mark_tick; c.seen_tick_in = L.seen_tick;
    c.marks = out->marks; c.mark_tick = out->mark_tick; c.seen_tick = out->seen_tick; c.out_hits = out->live_hits; c.out_hit_bits = out->hit_bits;
    c.out_seen_bits = out->seen_bits; c.state = out->state;
    int32_t* o_dist2 = out->dist2;
    StagedIo io;
    if (!fdev) { io.in(depth, bpp * npix, &d_depth); io.in(d_mask, npix, &d_mask); }
    if (!dev) {
        io.in(state_in, P, &c.state_in); io.in(L.marks, 4 * P, &c.marks_in); io.in(L.mark_tick, 4 * P, &c.mark_tick_in); io.in(L.seen_tick, 4 * P, &c.seen_tick_in);
        io.out(out->marks, 4 * P, &c.marks); io.out(out->mark_tick, 4 * P, &c.mark_tick); io.out(out->seen_tick, 4 * P, &c.seen_tick);
        io.out(out->live_hits, 4 * P, &c.out_hits); io.out(out->hit_bits, 4 * P, &c.out_hit_bits); io.out(out->seen_bits, 4 * P, &c.out_seen_bits);
        io.out(out->state, P, &c.state); io.out(out->dist2, 4 * P, &o_dist2);
    }
    NavMemWs& w = h->navmem;
    bool ok = true;
    if (!w.stats) ok = w.bufs.grow({{(void**)&w.stats, NM_STATS * NM_PAD * sizeof(unsigned long long)}});
    if (ok && P > w.cells) {
        ok = w.bufs.grow({{(void**)&w.hits, 4 * P}, {(void**)&w.hit_bits, 4 * P}, {(void**)&w.seen_bits, 4 * P}, {(void**)&w.colg, 2 * P}, {(void**)&w.state, P}});
        if (ok) w.cells = P;
    }
    if (ok) ok = io.reserve(w.bufs, &w.img, &w.img_bytes, io.need());
    if (!ok) { h->err = "ssf_navmem_update: allocation of the working buffers failed"; return SSF_ERR_DEVICE; }
    c.hits = w.hits; c.hit_bits = w.hit_bits; c.seen_bits = w.seen_bits;

    hipStream_t st = h->stream;
    TimerScope ts(h);
    HCK(io.copy_in(st));
    HCK(hipMemsetAsync(w.stats, 0, NM_STATS * NM_PAD * sizeof(unsigned long long), st));
    HCK(hipMemsetAsync(w.hits, 0, 4 * P, st));
    HCK(hipMemsetAsync(w.hit_bits, 0, 4 * P, st));
    HCK(hipMemsetAsync(w.seen_bits, 0, 4 * P, st));
    launch_navmem_stamp(st, df, G, cam, S, d_depth, h->in_scale, d_mask, p->mask_mode, w.hits, w.hit_bits, w.stats);
    HCK(hipGetLastError());
    launch_navmem_march(st, df, G, cam, S, d_depth, h->in_scale, p->hit_margin_cells * p->res, w.seen_bits, w.stats);
    HCK(hipGetLastError());
    if (o_dist2 && !c.state) c.state = w.state;                       // dist2 alone: the state is still computed, internally
    const NavMemRule rule{p->min_hits, p->open_unknown != 0, p->tick, p->max_mark_age, p->max_seen_age};
    launch_navmem_cells(st, P, rule, c, w.stats);
    HCK(hipGetLastError());
    if (o_dist2) {
        launch_navgrid_clearance(st, c.state, G.W, G.H, p->max_dist_cells, p->unknown_is_obstacle != 0, w.colg, o_dist2);
        HCK(hipGetLastError());
    }
    NavPaddedSums<NM_STATS, NM_PAD> s;
    HCK(s.fetch(w.stats, st));
    HCK(io.copy_out(st));
    { int rc = sync_collect(h); if (rc) return rc; }
    if (stats) {
        stats->pixels_valid = (int64_t)s[NM_VALID]; stats->pixels_stamping = (int64_t)s[NM_STAMPING]; stats->points_in_band = (int64_t)s[NM_POINTS];
        stats->rays = (int64_t)s[NM_RAYS]; stats->rays_carving = (int64_t)s[NM_CARVING]; stats->ray_samples = (int64_t)s[NM_SAMPLES];
        stats->cells_marked = (int64_t)s[NM_MARKED]; stats->cells_newly_marked = (int64_t)s[NM_NEWLY]; stats->cells_cleared = (int64_t)s[NM_CLEARED];
        stats->cells_expired = (int64_t)s[NM_EXPIRED]; stats->bits_cleared = (int64_t)s[NM_BITS]; stats->cells_remembered = (int64_t)s[NM_REMEMBERED];
        stats->cells_opened = (int64_t)s[NM_OPENED]; stats->cells_free = (int64_t)s[NM_FREE]; stats->cells_occupied = (int64_t)s[NM_OCC];
        stats->cells_unknown = (int64_t)P - (int64_t)s[NM_FREE] - (int64_t)s[NM_OCC];
        stats->atomics = (int64_t)(s[NM_STAMP_ATOMICS] + s[NM_MARCH_ATOMICS]);
        std::memcpy(stats->pose, gpose, sizeof(gpose));
    }
    return SSF_OK;
}
}  // extern "C"
