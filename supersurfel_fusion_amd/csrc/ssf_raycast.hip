// ssf_raycast.hip -- rays cast through the fused model (include/ssf_raycast.h) on gfx950: a hashed uniform grid of the model's
// discs that stays on the handle, and the march of the rays through it.
//
// What is computed is pinned, operation by operation, in include/ssf_raycast.h (the numpy restatement, a brute force over
// rays x rows: tests/raycast_ref.py).  The winner of a ray is an integer minimum, so the order inside a bucket does not matter.  How:
//   * prep   k_raycast_prep: one thread per slot of [visible rows | out-of-view span] (slot_row / slot_logical256; the out-of-view
//            blocks' live offsets by launch_slots_oov_offsets into own scratch).  Every slot that holds a row gets one
//            aligned 64-byte record (c, dims.x | n, dims.y | e1, conf | e2, logical index) -- all a candidate test reads -- and a
//            class: not indexed, grid (with its box of cells), oversize.  Rows, oversize rows and entries are summed per workgroup;
//            the box of all indexed cells is taken by integer atomicMin / atomicMax.  The host reads these once, sizes the table
//            (hash_bits 0: from the entry count) and the lists.
//            k_raycast_count (booked under raycast_prep as well): the entries per bucket, through a per-workgroup LDS histogram
//            when the table fits one (RC_HIST buckets), else by global integer atomics.
//   * scan   launch_slots_scan (ssf_slots.hpp) over the bucket counts.
//   * fill   k_raycast_fill: (bucket -> slot) lists, reserved per workgroup and bucket through the same histogram; oversize slots
//            are appended to their list.
//   * march  k_raycast_march: ONE RAY PER WAVE.  The walk's state is the same in every lane (wave-uniform); the 64 lanes test 64
//            entries of a bucket per round; each lane keeps the minimum key (bits(tt) << 32 | logical index) it saw, reduced
//            across the wave when a lane found something.  The oversize list is tested first, in full.
//            The walk (DESIGN.md section 4.12 has the proof) advances in PARAMETER steps t_a -> t_b of at most one cell along the
//            fastest axis and evaluates p_j(t) = O_j + t * D_j with the rule's own two operations.  Both are monotone in t, and so
//            is the cell of a coordinate, floorf(x / cell): the hit point of ANY tt in [t_a, t_b] lies, per axis, between the two
//            ends' cells -- exactly, no rounding argument.  The step visits that box of cells (widened by mu for the hit point's
//            distance from the disc's plane, clipped to the box of indexed cells, without the cells of the previous step).  After
//            a step every candidate with tt <= t_b has been seen: the walk stops once the best tt is <= t_b.  The walk's range is
//            clipped to the indexed cells by a guess that is then VERIFIED with the same monotone functions (else not clipped).
// Nothing here writes to the handle's stores, counters or scratch: the working set is RaycastWs (ssf_handle.hpp).
#include "ssf_slots.hpp"
#include "ssf_raycast.hpp"

namespace ssf {

enum { RC_HIST = 4096, RC_MAX_CELLS = 64, RC_COORD = 32000, RC_BIAS = 32768, RC_RAYS_PER_WG = 4 };
// the sums the host reads (u64): rows indexed, oversize rows, grid entries | per call: hits, invalid rays, cells, candidates
enum { RC_ROWS = 0, RC_OVER = 1, RC_ENTRIES = 2, RC_HIT = 3, RC_INVALID = 4, RC_CELLS = 5, RC_TESTED = 6, RC_TOTAL = 7, RC_STATS = 8 };
enum { RC_NONE = 0u, RC_GRID = 1u, RC_OVERSIZE = 2u };

struct RayCast { float R[9], t0[3]; float tmin, tmax, min_conf; int visible_only, n; };
struct RayOut { float* t; int32_t* index; float* point; float* normal; float* color; };

// the cell of a coordinate: monotone (non-decreasing) in x; clamped so that it fits 16 bits (no row is entered beyond +-RC_COORD)
__device__ __forceinline__ int rc_cell(float x, float cell) {
    const float g = floorf(x / cell);
    return g >= 32767.0f ? 32767 : (g >= -32768.0f ? (int)g : -32768);           // (a NaN: -32768)
}
__device__ __forceinline__ uint32_t rc_hash(int x, int y, int z) {
    return ((uint32_t)x * 73856093u) ^ ((uint32_t)y * 19349663u) ^ ((uint32_t)z * 83492791u);
}
__device__ __forceinline__ float rc_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// ---- prep: one thread per slot ---------------------------------------------------------------------------------------
// rbox[s] = (x0 | x1 << 16, y0 | y1 << 16, z0 | z1 << 16, class), cells biased by RC_BIAS; cbox[0..2] = min, [3..5] = max cell
__global__ __launch_bounds__(256) void k_raycast_prep(ModelView mv, float cell, float s, const uint32_t* __restrict__ bc,
                                                      float4* __restrict__ rec, uint4* __restrict__ rbox, int* __restrict__ cbox,
                                                      unsigned long long* __restrict__ stats) {
    __shared__ int part[4];
    __shared__ unsigned long long red[3][4];
    __shared__ int sbox[6];
    if (threadIdx.x < 6) sbox[threadIdx.x] = threadIdx.x < 3 ? INT32_MAX : INT32_MIN;
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    SurfelSoA src; size_t row;
    const bool have = slot_row(mv, slot, src, row);
    const int lg = slot_logical256(mv, have, bc, part);                  // (holds a __syncthreads(): sbox is set behind it)
    __syncthreads();
    uint4 box = make_uint4(0u, 0u, 0u, RC_NONE);
    unsigned long long n_rows = 0, n_over = 0, n_ent = 0;
    if (have) {
        const float cx = src.pos[3 * row], cy = src.pos[3 * row + 1], cz = src.pos[3 * row + 2];
        const float dx = src.dims[2 * row], dy = src.dims[2 * row + 1];
        const float* r0 = src.r0 + 3 * row; const float* r1 = src.r1 + 3 * row; const float* r2 = src.r2 + 3 * row;
        const float a0 = r0[0], a1 = r0[1], a2 = r0[2], b0 = r1[0], b1 = r1[1], b2 = r1[2], n0 = r2[0], n1 = r2[1], n2 = r2[2];
        float4* o = rec + 4 * (size_t)slot;
        o[0] = make_float4(cx, cy, cz, dx);
        o[1] = make_float4(n0, n1, n2, dy);
        o[2] = make_float4(a0, a1, a2, src.conf[row]);
        o[3] = make_float4(b0, b1, b2, __int_as_float(lg));
        if (finite3(cx, cy, cz) && dx > 0.0f && dy > 0.0f && isfinite(dx) && isfinite(dy)) {
            n_rows = 1;
            const float T = 0.0078125f, tiny = 9.094947017729282e-13f;       // 2^-7, 2^-40
            bool over = dx < tiny || dy < tiny;
            over = over || !(fabsf(rc_dot(a0, a1, a2, a0, a1, a2) - 1.0f) <= T && fabsf(rc_dot(b0, b1, b2, b0, b1, b2) - 1.0f) <= T &&
                             fabsf(rc_dot(n0, n1, n2, n0, n1, n2) - 1.0f) <= T && fabsf(rc_dot(a0, a1, a2, b0, b1, b2)) <= T &&
                             fabsf(rc_dot(a0, a1, a2, n0, n1, n2)) <= T && fabsf(rc_dot(b0, b1, b2, n0, n1, n2)) <= T);
            int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
            if (!over) {
                const float h1 = s * sqrtf(dx), h2 = s * sqrtf(dy), hs = h1 + h2;
                const float c[3] = {cx, cy, cz}, e1[3] = {a0, a1, a2}, e2[3] = {b0, b1, b2};
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const float E = ((fabsf(e1[j]) * h1 + fabsf(e2[j]) * h2) * 1.0625f + hs * 0.03125f) +
                                    (fabsf(c[j]) * 9.5367431640625e-07f + cell * 0.0009765625f);
                    const float glo = (c[j] - E) / cell, ghi = (c[j] + E) / cell;
                    if (!(glo >= -(float)RC_COORD && ghi <= (float)RC_COORD)) over = true;
                    else { lo[j] = (int)floorf(glo); hi[j] = (int)floorf(ghi); }
                }
            }
            long long cells = 0;
            if (!over) {
                cells = (long long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
                if (cells > RC_MAX_CELLS) over = true;
            }
            if (over) { n_over = 1; box.w = RC_OVERSIZE; }
            else {
                n_ent = (unsigned long long)cells;
                box = make_uint4((uint32_t)(lo[0] + RC_BIAS) | ((uint32_t)(hi[0] + RC_BIAS) << 16), (uint32_t)(lo[1] + RC_BIAS) | ((uint32_t)(hi[1] + RC_BIAS) << 16),
                                 (uint32_t)(lo[2] + RC_BIAS) | ((uint32_t)(hi[2] + RC_BIAS) << 16), RC_GRID);
#pragma unroll
                for (int j = 0; j < 3; j++) { atomicMin(&sbox[j], lo[j]); atomicMax(&sbox[3 + j], hi[j]); }
            }
        }
    }
    if ((int)slot < mv.nslots) rbox[slot] = box;
    n_rows = wave_sum(n_rows); n_over = wave_sum(n_over); n_ent = wave_sum(n_ent);
    if (lane() == 0) { red[0][threadIdx.x >> 6] = n_rows; red[1][threadIdx.x >> 6] = n_over; red[2][threadIdx.x >> 6] = n_ent; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned long long sum = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
        if (sum) atomicAdd(&stats[RC_ROWS + threadIdx.x], sum);
    }
    if (threadIdx.x >= 64 && threadIdx.x < 70) {
        const int j = threadIdx.x - 64, v = sbox[j];
        if (j < 3) { if (v != INT32_MAX) atomicMin(&cbox[j], v); } else if (v != INT32_MIN) atomicMax(&cbox[j], v);
    }
}

// ---- count and fill: the (bucket -> slot) lists ------------------------------------------------------------------------
struct RcBox { int x0, x1, y0, y1, z0, z1; uint32_t cls; };
__device__ __forceinline__ RcBox rc_unpack(uint4 b) {
    RcBox r;
    r.x0 = (int)(b.x & 0xFFFF) - RC_BIAS; r.x1 = (int)(b.x >> 16) - RC_BIAS; r.y0 = (int)(b.y & 0xFFFF) - RC_BIAS; r.y1 = (int)(b.y >> 16) - RC_BIAS;
    r.z0 = (int)(b.z & 0xFFFF) - RC_BIAS; r.z1 = (int)(b.z >> 16) - RC_BIAS; r.cls = b.w;
    return r;
}
__global__ __launch_bounds__(256) void k_raycast_count(int nslots, uint32_t mask, const uint4* __restrict__ rbox, uint32_t* __restrict__ cnt) {
    __shared__ uint32_t hist[RC_HIST];
    const bool use_hist = mask < (uint32_t)RC_HIST;                      // block-uniform
    if (use_hist) {
        for (uint32_t t = threadIdx.x; t <= mask; t += 256) hist[t] = 0u;
        __syncthreads();
    }
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    RcBox b; b.cls = RC_NONE;
    if ((int)slot < nslots) b = rc_unpack(rbox[slot]);
    if (b.cls == RC_GRID)
        for (int z = b.z0; z <= b.z1; z++)
            for (int y = b.y0; y <= b.y1; y++)
                for (int x = b.x0; x <= b.x1; x++) atomicAdd(use_hist ? &hist[rc_hash(x, y, z) & mask] : &cnt[rc_hash(x, y, z) & mask], 1u);
    if (use_hist) {
        __syncthreads();
        for (uint32_t t = threadIdx.x; t <= mask; t += 256) { const uint32_t c = hist[t]; if (c) atomicAdd(&cnt[t], c); }
    }
}
// over[0 .. n_over): the oversize slots; over_n: its cursor (zeroed by the caller)
__global__ __launch_bounds__(256) void k_raycast_fill(int nslots, uint32_t mask, const uint4* __restrict__ rbox, uint32_t* __restrict__ cursor,
                                                      uint32_t* __restrict__ list, uint32_t* __restrict__ over, uint32_t* __restrict__ over_n) {
    __shared__ uint32_t hist[RC_HIST], base[RC_HIST];
    const bool use_hist = mask < (uint32_t)RC_HIST;                      // block-uniform
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    RcBox b; b.cls = RC_NONE;
    if ((int)slot < nslots) b = rc_unpack(rbox[slot]);
    if (b.cls == RC_OVERSIZE) over[atomicAdd(over_n, 1u)] = slot;
    const bool any = b.cls == RC_GRID;
    if (!use_hist) {
        if (any)
            for (int z = b.z0; z <= b.z1; z++)
                for (int y = b.y0; y <= b.y1; y++)
                    for (int x = b.x0; x <= b.x1; x++) list[atomicAdd(&cursor[rc_hash(x, y, z) & mask], 1u)] = slot;
        return;
    }
    // the workgroup's entries per bucket, one reservation per bucket in the global list, then the ranks inside the reservation
    for (uint32_t t = threadIdx.x; t <= mask; t += 256) hist[t] = 0u;
    __syncthreads();
    if (any)
        for (int z = b.z0; z <= b.z1; z++)
            for (int y = b.y0; y <= b.y1; y++)
                for (int x = b.x0; x <= b.x1; x++) atomicAdd(&hist[rc_hash(x, y, z) & mask], 1u);
    __syncthreads();
    for (uint32_t t = threadIdx.x; t <= mask; t += 256) {
        const uint32_t c = hist[t];
        if (c) { base[t] = atomicAdd(&cursor[t], c); hist[t] = 0u; }
    }
    __syncthreads();
    if (any)
        for (int z = b.z0; z <= b.z1; z++)
            for (int y = b.y0; y <= b.y1; y++)
                for (int x = b.x0; x <= b.x1; x++) { const uint32_t t = rc_hash(x, y, z) & mask; list[base[t] + atomicAdd(&hist[t], 1u)] = slot; }
}

// ---- march: one ray per wave ---------------------------------------------------------------------------------------------
struct RcRay { float Ox, Oy, Oz, Dx, Dy, Dz; };
// steps 3 to 6 of the rule for one (ray, slot): the lane's minimum key and the slot that gave it
__device__ __forceinline__ void rc_test(const float4* __restrict__ rec, uint32_t slot, const RcRay& r, const RayCast& q, const RayIndex& ix,
                                        unsigned long long& best, uint32_t& best_slot) {
    if (q.visible_only && (int)slot >= ix.nvs) return;
    const float4* p = rec + 4 * (size_t)slot;
    const float4 A = p[0], B = p[1], C = p[2], E = p[3];
    if (!(C.w > q.min_conf)) return;
    const float den = (B.x * r.Dx + B.y * r.Dy) + B.z * r.Dz;
    const float wx = A.x - r.Ox, wy = A.y - r.Oy, wz = A.z - r.Oz;
    const float num = (B.x * wx + B.y * wy) + B.z * wz;
    const float tt = num / den;
    if (!(den != 0.0f) || !isfinite(tt) || !(tt >= q.tmin && tt <= q.tmax)) return;
    const float Px = r.Ox + tt * r.Dx, Py = r.Oy + tt * r.Dy, Pz = r.Oz + tt * r.Dz;
    const float Vx = Px - A.x, Vy = Py - A.y, Vz = Pz - A.z;
    const float a = (Vx * C.x + Vy * C.y) + Vz * C.z, b = (Vx * E.x + Vy * E.y) + Vz * E.z;
    if (!((a * a) * B.w + (b * b) * A.w <= (ix.k * A.w) * B.w)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(tt) << 32) | (uint32_t)__float_as_int(E.w);
    if (key < best) { best = key; best_slot = slot; }
}

// LANE (the laboratory build's other arm, measured against this one in profiles/raycast.txt): one ray per LANE -- every lane walks
// its own ray and tests its buckets' entries one by one; no wave-wide step is taken
template <bool LANE>
__global__ __launch_bounds__(256) void k_raycast_march(RayCast q, RayIndex ix, ModelView mv, const float* __restrict__ rays,
                                                       const float4* __restrict__ rec, const uint32_t* __restrict__ off,
                                                       const uint32_t* __restrict__ list, const uint32_t* __restrict__ over, RayOut out,
                                                       unsigned long long* __restrict__ stats) {
    const int nwaves = LANE ? (int)(gridDim.x * 256) : (int)(gridDim.x * RC_RAYS_PER_WG);             // rays in flight
    const int wave0 = LANE ? (int)(blockIdx.x * 256 + threadIdx.x) : __builtin_amdgcn_readfirstlane((int)(blockIdx.x * RC_RAYS_PER_WG + (threadIdx.x >> 6)));
    const int ln = LANE ? 0 : lane(), width = LANE ? 1 : 64;           // this lane's first entry of a list, and the stride
    const float INF = __uint_as_float(0x7F800000u);
    unsigned long long n_hit = 0, n_invalid = 0, n_cells = 0, n_tested = 0;       // lane 0's are the wave's
    for (int ray = wave0; ray < q.n; ray += nwaves) {
        const float* in = rays + 6 * (size_t)ray;
        const float ox = in[0], oy = in[1], oz = in[2], dx = in[3], dy = in[4], dz = in[5];
        RcRay r;
        r.Ox = ((q.R[0] * ox + q.R[1] * oy) + q.R[2] * oz) + q.t0[0];
        r.Oy = ((q.R[3] * ox + q.R[4] * oy) + q.R[5] * oz) + q.t0[1];
        r.Oz = ((q.R[6] * ox + q.R[7] * oy) + q.R[8] * oz) + q.t0[2];
        r.Dx = (q.R[0] * dx + q.R[1] * dy) + q.R[2] * dz;
        r.Dy = (q.R[3] * dx + q.R[4] * dy) + q.R[5] * dz;
        r.Dz = (q.R[6] * dx + q.R[7] * dy) + q.R[8] * dz;
        const bool valid = finite3(ox, oy, oz) && finite3(dx, dy, dz) && !(r.Dx == 0.0f && r.Dy == 0.0f && r.Dz == 0.0f);
        unsigned long long best = ~0ull; uint32_t best_slot = 0u;
        if (valid) {
            // the oversize list, in full
            for (int e = ln; e < ix.n_over; e += width) rc_test(rec, over[e], r, q, ix, best, best_slot);
            n_tested += (unsigned long long)ix.n_over;
            unsigned long long wbest = LANE ? best : wave_min64(best);
            // the grid.  A non-finite O or D (an overflow of step 1) gives no candidate among the grid's rows: tt is 0, infinite or a NaN
            const float O[3] = {r.Ox, r.Oy, r.Oz}, D[3] = {r.Dx, r.Dy, r.Dz};
            bool walk = ix.cmin[0] <= ix.cmax[0] && finite3(O[0], O[1], O[2]) && finite3(D[0], D[1], D[2]);
            const float Dmax = fmaxf(fmaxf(fabsf(D[0]), fabsf(D[1])), fabsf(D[2]));
            const float Omax = fmaxf(fmaxf(fabsf(O[0]), fabsf(O[1])), fabsf(O[2]));
            // the hit point of an accepted pair is within mu of the disc's box, per axis
            const float mu = 1.52587890625e-05f * ((Omax + ix.cabs) * 2.0f + ix.cell);
            // p_j(t) = O_j + t * D_j is monotone in t, rc_cell in x: `before(t)` true => no step at a parameter <= t touches an indexed cell
            auto before = [&](float t) {
                bool yes = false;
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const float pj = O[j] + t * D[j];
                    yes = yes || (D[j] > 0.0f && rc_cell(pj + mu, ix.cell) < ix.cmin[j]) || (D[j] < 0.0f && rc_cell(pj - mu, ix.cell) > ix.cmax[j]);
                }
                return yes;
            };
            auto after = [&](float t) {
                bool yes = false;
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const float pj = O[j] + t * D[j];
                    yes = yes || (D[j] > 0.0f && rc_cell(pj - mu, ix.cell) > ix.cmax[j]) || (D[j] < 0.0f && rc_cell(pj + mu, ix.cell) < ix.cmin[j]);
                }
                return yes;
            };
            float tlo = q.tmin, thi = q.tmax;
            if (walk) {
                // the range of the walk: per axis a GUESS of where the ray enters and leaves the indexed cells, pushed outwards by a
                // cell and the rounding of the division; used only if the monotone test confirms it, else the range stays [t_min, t_max]
                float ten = -INF, tex = INF;
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    if (D[j] == 0.0f) {                                  // p_j(t) = O_j for every t
                        if (rc_cell(O[j] + mu, ix.cell) < ix.cmin[j] || rc_cell(O[j] - mu, ix.cell) > ix.cmax[j]) walk = false;
                    } else {
                        const float t1 = ((float)ix.cmin[j] * ix.cell - O[j]) / D[j], t2 = ((float)(ix.cmax[j] + 1) * ix.cell - O[j]) / D[j];
                        const float pad = (ix.cell + 4.0f * mu) / fabsf(D[j]);
                        const float en = fminf(t1, t2), ex = fmaxf(t1, t2);
                        ten = fmaxf(ten, en - (pad + fabsf(en) * 1e-4f)); tex = fminf(tex, ex + (pad + fabsf(ex) * 1e-4f));
                    }
                }
                if (walk && (before(q.tmax) || after(q.tmin))) walk = false;
                if (walk) {
                    if (ten > q.tmin && ten < q.tmax && before(ten)) tlo = ten;
                    if (tex > q.tmin && tex < q.tmax && after(tex)) thi = tex;
                    if (tlo > thi) walk = false;                         // every accepted tt is >= tlo and <= thi: none
                }
            }
            if (walk) {
                const float dt = ix.cell / Dmax;
                float ta = tlo;
                float pa[3] = {O[0] + ta * D[0], O[1] + ta * D[1], O[2] + ta * D[2]};
                int plo[3] = {1, 1, 1}, phi[3] = {0, 0, 0};              // the previous step's box (empty)
                while (true) {
                    float tb = ta + dt;
                    if (!(tb > ta)) tb = __uint_as_float(__float_as_uint(ta) + 1u);       // (ta > 0: the next float up)
                    if (!(tb < thi)) tb = thi;
                    const float pb[3] = {O[0] + tb * D[0], O[1] + tb * D[1], O[2] + tb * D[2]};
                    int lo[3], hi[3];
                    bool some = true;
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        lo[j] = max(rc_cell(fminf(pa[j], pb[j]) - mu, ix.cell), ix.cmin[j]);
                        hi[j] = min(rc_cell(fmaxf(pa[j], pb[j]) + mu, ix.cell), ix.cmax[j]);
                        some = some && lo[j] <= hi[j];
                    }
                    bool found = false;
                    if (some) {
                        for (int z = lo[2]; z <= hi[2]; z++)
                            for (int y = lo[1]; y <= hi[1]; y++)
                                for (int x = lo[0]; x <= hi[0]; x++) {
                                    if (x >= plo[0] && x <= phi[0] && y >= plo[1] && y <= phi[1] && z >= plo[2] && z <= phi[2]) continue;
                                    const uint32_t bkt = rc_hash(x, y, z) & ix.mask;
                                    const uint32_t beg = off[bkt], end = off[bkt + 1];
                                    n_cells++; n_tested += end - beg;
                                    for (uint32_t e = beg + ln; e < end; e += width) {
                                        const unsigned long long was = best;
                                        rc_test(rec, list[e], r, q, ix, best, best_slot);
                                        found = found || best != was;
                                    }
                                }
#pragma unroll
                        for (int j = 0; j < 3; j++) { plo[j] = lo[j]; phi[j] = hi[j]; }
                    } else { plo[0] = 1; phi[0] = 0; }
                    if (LANE) wbest = best;
                    else if (__ballot(found)) wbest = wave_min64(best);
                    // every candidate with tt <= tb has been seen: a later one cannot be smaller, nor tie
                    if (wbest != ~0ull && __uint_as_float((uint32_t)(wbest >> 32)) <= tb) break;
                    if (!(tb < thi) || after(tb)) break;                 // (after: the ray has left the indexed cells for good)
                    ta = tb; pa[0] = pb[0]; pa[1] = pb[1]; pa[2] = pb[2];
                }
            }
            if (!LANE) {
                wbest = wave_min64(best);
                best_slot = (uint32_t)__shfl((int)best_slot, (int)(__ffsll((long long)__ballot(best == wbest)) - 1), 64);
                best = wbest;
            }
        } else n_invalid++;
        if (LANE || lane() == 0) {
            const bool hit = best != ~0ull;
            n_hit += hit;
            const float tt = hit ? __uint_as_float((uint32_t)(best >> 32)) : 0.0f;
            if (out.t) out.t[ray] = tt;
            if (out.index) out.index[ray] = hit ? (int32_t)(uint32_t)best : -1;
            if (out.point) {
                float* o = out.point + 3 * (size_t)ray;
                o[0] = hit ? r.Ox + tt * r.Dx : 0.0f; o[1] = hit ? r.Oy + tt * r.Dy : 0.0f; o[2] = hit ? r.Oz + tt * r.Dz : 0.0f;
            }
            if (out.normal) {
                float* o = out.normal + 3 * (size_t)ray;
                float nx = 0.0f, ny = 0.0f, nz = 0.0f;
                if (hit) {
                    const float4 B = rec[4 * (size_t)best_slot + 1];
                    const float den = (B.x * r.Dx + B.y * r.Dy) + B.z * r.Dz;
                    nx = den > 0.0f ? -B.x : B.x; ny = den > 0.0f ? -B.y : B.y; nz = den > 0.0f ? -B.z : B.z;
                }
                o[0] = nx; o[1] = ny; o[2] = nz;
            }
            if (out.color) {
                float* o = out.color + 3 * (size_t)ray;
                float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
                if (hit) {
                    SurfelSoA src; size_t row;
                    (void)slot_row(mv, best_slot, src, row);
                    c0 = src.col[3 * row]; c1 = src.col[3 * row + 1]; c2 = src.col[3 * row + 2];
                }
                o[0] = c0; o[1] = c1; o[2] = c2;
            }
        }
    }
    if (LANE) { n_hit = wave_sum(n_hit); n_invalid = wave_sum(n_invalid); n_cells = wave_sum(n_cells); n_tested = wave_sum(n_tested); }
    if (lane() == 0) {
        if (n_hit) atomicAdd(&stats[RC_HIT], n_hit);
        if (n_invalid) atomicAdd(&stats[RC_INVALID], n_invalid);
        if (n_cells) atomicAdd(&stats[RC_CELLS], n_cells);
        if (n_tested) atomicAdd(&stats[RC_TESTED], n_tested);
    }
}

}  // namespace ssf

// ---- host: the entry points of include/ssf_raycast.h ---------------------------------------------------------------------
using namespace ssf;

// (re)builds the resident index for (cell, s, hash_bits) from the model as it stands
static int raycast_build(ssf_handle* h, float cell, float s, int hash_bits) {
    RaycastWs& w = h->raycast;
    hipStream_t st = h->stream;
    const ModelView mv = model_view(h, false);
    w.built = false;
    const size_t slots = std::max<size_t>(mv.nslots, 256);
    bool ok = true;
    if (slots > w.slots) {
        ok = w.bufs.grow({{(void**)&w.rec, 64 * slots}, {(void**)&w.rbox, 16 * slots}, {(void**)&w.bc, 4 * (slots / 256 + 2)}, {(void**)&w.over, 4 * slots}});
        if (ok) w.slots = slots;
    }
    if (ok && !w.stats) ok = w.bufs.grow({{(void**)&w.stats, RC_STATS * sizeof(unsigned long long)}, {(void**)&w.cbox, 8 * sizeof(int)}});
    if (!ok) { h->err = "ssf_raycast: allocation of the index's per-slot buffers failed"; return SSF_ERR_DEVICE; }
    const int cbox0[8] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN, 0, 0};
    HCK(hipMemsetAsync(w.stats, 0, RC_STATS * sizeof(unsigned long long), st));
    HCK(hipMemcpyAsync(w.cbox, cbox0, sizeof(cbox0), hipMemcpyHostToDevice, st));
    {
        ScopedKernel sk("raycast_prep", st);
        launch_slots_oov_offsets(st, mv, w.bc);
        if (mv.nbv + mv.nbo > 0)
            hipLaunchKernelGGL(k_raycast_prep, dim3(mv.nbv + mv.nbo), dim3(256), 0, st, mv, cell, s, w.bc, w.rec, w.rbox, w.cbox, w.stats);
    }
    HCK(hipGetLastError());
    unsigned long long s3[3] = {0, 0, 0};
    int cbox[8];
    HCK(hipMemcpyAsync(s3, w.stats, sizeof(s3), hipMemcpyDeviceToHost, st));
    HCK(hipMemcpyAsync(cbox, w.cbox, sizeof(cbox), hipMemcpyDeviceToHost, st));
    HCK(hipStreamSynchronize(st));
    const unsigned long long entries = s3[RC_ENTRIES];
    { int rc = w.bl.reserve_list(w.bufs, entries, h->err, "ssf_raycast: more than 2^32 - 1 (cell, row) index entries",
                                 "ssf_raycast: allocation of the index's lists failed"); if (rc) return rc; }
    int bits = hash_bits;
    if (bits == 0) { bits = 10; while (bits < 24 && (1ull << bits) < entries / 32) bits++; }
    const size_t nb = (size_t)1 << bits;
    if (!w.bl.reserve_bins(w.bufs, nb)) { h->err = "ssf_raycast: allocation of the index's table failed"; return SSF_ERR_DEVICE; }
    const uint32_t mask = (uint32_t)(nb - 1);
    HCK(hipMemsetAsync(w.bl.off, 0, 4 * (nb + 1), st));
    HCK(hipMemsetAsync(w.cbox + 6, 0, 4, st));                          // the oversize list's cursor
    if (entries > 0) {
        ScopedKernel sk("raycast_prep", st);
        hipLaunchKernelGGL(k_raycast_count, dim3(mv.nslots / 256), dim3(256), 0, st, mv.nslots, mask, w.rbox, w.bl.off);
    }
    {
        ScopedKernel sk("raycast_scan", st);
        launch_slots_scan(st, w.bl.off, (int)nb, w.bl.cursor, nullptr);
    }
    if (entries > 0 || s3[RC_OVER] > 0) {
        ScopedKernel sk("raycast_fill", st);
        hipLaunchKernelGGL(k_raycast_fill, dim3(mv.nslots / 256), dim3(256), 0, st, mv.nslots, mask, w.rbox, w.bl.cursor, w.bl.list, w.over, (uint32_t*)(w.cbox + 6));
    }
    HCK(hipGetLastError());
    RayIndex& ix = w.ix;
    ix.cell = cell; ix.s = s; ix.k = s * s; ix.mask = mask;
    int cabs_cells = 0;
    for (int j = 0; j < 3; j++) {
        ix.cmin[j] = entries ? cbox[j] : 1; ix.cmax[j] = entries ? cbox[3 + j] : 0;
        if (entries) cabs_cells = std::max(cabs_cells, std::max(std::abs(cbox[j]), std::abs(cbox[3 + j] + 1)));
    }
    ix.cabs = (float)cabs_cells * cell;
    ix.n_over = (int)s3[RC_OVER]; ix.nvs = mv.nvs;
    w.rows_indexed = (long long)s3[RC_ROWS]; w.rows_oversize = (long long)s3[RC_OVER]; w.entries = (long long)entries;
    w.gen = h->model_gen; w.recentres = h->n_recentres; w.cell = cell; w.s = s; w.hash_bits = hash_bits; w.built = true;
    return SSF_OK;
}

const char* raycast_params_refusal(const ssf_handle* h, const ssf_raycast_params* p, RaycastResolved& r) {
    r.tmin = p->t_min; r.tmax = p->t_max;
    if (r.tmin == 0.0f && r.tmax == 0.0f) { r.tmin = h->cfg.range_min; r.tmax = h->cfg.range_max; }
    if (!std::isfinite(r.tmin) || !std::isfinite(r.tmax) || !(r.tmin > 0.0f) || !(r.tmax > r.tmin)) return "the range needs 0 < t_min < t_max, both finite";
    if (std::isnan(p->min_conf)) return "min_conf is a NaN";
    const float lo = 0.0009765625f, hi = 1024.0f;
    r.s = p->splat_scale == 0.0f ? 3.0f : p->splat_scale;
    if (!(r.s >= lo && r.s <= hi)) return "splat_scale must be 0 or in [2^-10, 2^10]";
    r.cell = p->cell == 0.0f ? 0.125f : p->cell;
    if (!(r.cell >= lo && r.cell <= hi)) return "cell must be 0 or in [2^-10, 2^10]";
    if (p->hash_bits != 0 && (p->hash_bits < 4 || p->hash_bits > 24)) return "hash_bits must be 0 or 4..24";
    return nullptr;
}

extern "C" {
int ssf_raycast_default_params(const ssf_handle* h, ssf_raycast_params* p) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    std::memset(p, 0, sizeof(*p));
    return SSF_OK;
}

int ssf_raycast(ssf_handle* h, const ssf_raycast_params* p, const float* rays, int n, float* t, int32_t* index, float* point,
                float* normal, float* color, ssf_raycast_stats* stats) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    auto refuse = [&](const char* what) { h->err = std::string("ssf_raycast: ") + what; return SSF_ERR_INVALID_ARG; };
    if (n < 0) return refuse("n < 0");
    if (!rays && n > 0) return refuse("rays is NULL");
    if (!t && !index && !point && !normal && !color) return refuse("every output is NULL");
    RaycastResolved rr;
    if (const char* what = raycast_params_refusal(h, p, rr)) return refuse(what);
    RayCast q;
    q.tmin = rr.tmin; q.tmax = rr.tmax;
    const float s = rr.s, cell = rr.cell;
    { int rc = model_at_rest(h, "ssf_raycast", "casts no rays"); if (rc) return rc; }
    float pose[12];
    if (p->pose) std::memcpy(pose, p->pose, sizeof(pose)); else pose_to12(h->pose, pose);
    std::memcpy(q.R, pose, 9 * sizeof(float)); q.t0[0] = pose[9]; q.t0[1] = pose[10]; q.t0[2] = pose[11];
    q.min_conf = p->min_conf; q.visible_only = p->visible_only != 0; q.n = n;

    RaycastWs& w = h->raycast;
    TimerScope ts(h);
    hipStream_t st = h->stream;
    const bool rebuild = !(w.built && w.gen == h->model_gen && w.recentres == h->n_recentres && w.cell == cell && w.s == s && w.hash_bits == p->hash_bits);
    if (rebuild) {
        int rc = raycast_build(h, cell, s, p->hash_bits);
        if (rc) { (void)hipStreamSynchronize(st); if (h->cfg.profile == 1) timer_collect(&h->timer); return rc; }
    }
    // the call's buffers: host rays and outputs are staged on the device
    const size_t N = (size_t)n;
    RayOut o{t, index, point, normal, color};
    const float* d_rays = rays;
    StagedIo io;
    if (!p->on_device && n > 0) {
        io.in(rays, 24 * N, &d_rays);
        io.out(t, 4 * N, &o.t); io.out(index, 4 * N, &o.index); io.out(point, 12 * N, &o.point); io.out(normal, 12 * N, &o.normal);
        io.out(color, 12 * N, &o.color);
        if (!io.reserve(w.bufs, &w.io, &w.io_bytes, io.need())) { h->err = "ssf_raycast: allocation of the staging buffer failed"; (void)sync_collect(h); return SSF_ERR_DEVICE; }
        HCK(io.copy_in(st));
    }
    HCK(hipMemsetAsync(w.stats + RC_HIT, 0, 4 * sizeof(unsigned long long), st));
    if (n > 0) {
        ScopedKernel sk("raycast_march", st);
#ifdef SSF_EXPERIMENTS
        if (SSF_ENV_INT("RAYCAST_LANE", 0) != 0)                        // the other arm: one ray per lane
            hipLaunchKernelGGL(k_raycast_march<true>, dim3((unsigned)std::min<size_t>((N + 255) / 256, 16384)), dim3(256), 0, st, q, w.ix, model_view(h, false),
                               d_rays, w.rec, w.bl.off, w.bl.list, w.over, o, w.stats);
        else
#endif
        hipLaunchKernelGGL(k_raycast_march<false>, dim3((unsigned)std::min<size_t>((N + RC_RAYS_PER_WG - 1) / RC_RAYS_PER_WG, 16384)), dim3(256), 0, st, q, w.ix,
                           model_view(h, false), d_rays, w.rec, w.bl.off, w.bl.list, w.over, o, w.stats);
    }
    HCK(hipGetLastError());
    unsigned long long s4[4] = {0, 0, 0, 0};
    HCK(hipMemcpyAsync(s4, w.stats + RC_HIT, sizeof(s4), hipMemcpyDeviceToHost, st));
    HCK(io.copy_out(st));
    { int rc = sync_collect(h); if (rc) return rc; }
    if (stats) {
        stats->rays = n; stats->rays_hit = (int64_t)s4[0]; stats->rays_invalid = (int64_t)s4[1];
        stats->rows_indexed = w.rows_indexed; stats->rows_oversize = w.rows_oversize; stats->index_entries = w.entries;
        stats->cells_visited = (int64_t)s4[2]; stats->candidates_tested = (int64_t)s4[3]; stats->index_rebuilt = rebuild ? 1 : 0;
    }
    return SSF_OK;
}
}  // extern "C"
