// ssf_slots.hpp -- device helpers of the kernels that walk the model one thread per SLOT (ModelView, ssf_device.hpp) and of the
// store upkeep (out-of-view compaction, re-homing): the slot -> row map, live counts and ranks inside a 256-thread block, the
// integer wave reductions, and the one-workgroup exclusive scan that turns per-block counts into offsets.  Included by
// ssf_render.hip, ssf_query.hip, ssf_navgrid.hip, ssf_raycast.hip, ssf_graph.hip, ssf_keyframes.hip and, through ssf_rows.hpp,
// ssf_track_fuse.hip, ssf_upkeep.hip and ssf_p2p.hip.
// The kernels shared by several of these files live in ssf_slots.hip (the library is built without relocatable device
// code), reached through the host launchers declared at the end: k_slots_scan -- the scan of render's and the navigation grid's
// tile counts, the ray cast's bucket counts and of every out-of-view live count; k_slots_scan32, the same body with 32-bit sums
// for the graph's sort histograms -- and k_slots_oov_count.  What does NOT go through them: k_query_scan (two counters plus the record), k_oov_scan and k_rehome_scan
// (ssf_upkeep.hip: a device-side n, store upkeep), k_bin_scan, everything of the per-frame kernels (ICP, association, fuse, partition, row move,
// k_bin_*: their own ballots and scans, tuned to the instruction) and of ssf_extract.hip, and the fill kernels (render's plain
// one, the LDS-histogram ones of the navigation grid and the ray cast with their different bin functions: measured choices).
#pragma once
#include "ssf_device.hpp"

namespace ssf {

__device__ __forceinline__ int lane() { return threadIdx.x & 63; }
__device__ __forceinline__ bool finite3(float a, float b, float c) { return isfinite(a) && isfinite(b) && isfinite(c); }

// the wave's sum of an integer, and its 64-bit minimum, told to every lane (integers: no order can change the result)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_min64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long u = __shfl_xor(v, o, 64); v = u < v ? u : v; }
    return v;
}

// the order-preserving unsigned image of a float (no NaN comes here): a < b <=> enc(a) < enc(b)
__host__ __device__ __forceinline__ uint32_t float_order_bits(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ __forceinline__ uint32_t float_order_bits_inv(uint32_t e) { return (e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e; }

// row head + i of an out-of-view span [head, tail): its physical index, and whether it holds a row (the span has holes, and its
// last 256-block reaches past the tail: the bound comes first, the flag behind the tail is never read)
__device__ __forceinline__ bool span_live(const uint8_t* __restrict__ live, int head, int tail, uint32_t i, size_t& phys) {
    phys = (size_t)head + i;
    return (long long)phys < (long long)tail && live[phys] != 0;
}

// slot -> the store and row it reads, and whether it holds a row of the model: slots [0, nvs) are rows of the visible array,
// then come the 256-wide blocks of the out-of-view span
__device__ __forceinline__ bool slot_row(const ModelView& mv, uint32_t s, SurfelSoA& src, size_t& row) {
    if (s < (uint32_t)mv.nvs) { src = mv.vis; row = s; return s < (uint32_t)mv.n_visible; }
    src = mv.oov.rows;
    const bool lv = span_live(mv.oov.live, mv.oov_head, mv.oov_tail, s - (uint32_t)mv.nvs, row);
    return s < (uint32_t)mv.nslots && lv;
}

// The two block helpers hold a __syncthreads(): ALL 256 threads of a workgroup call them, or none (a block-uniform branch
// around the call is fine, an early return in front of it is not).  part: four words of LDS that nothing else uses.
// the threads of this workgroup with `mine`, told to every thread
__device__ __forceinline__ int block_count256(bool mine, int* part) {
    const int k = __popcll(__ballot(mine));
    if (lane() == 0) part[threadIdx.x >> 6] = k;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}
// the threads of this workgroup with `mine` IN FRONT of this one: the waves before mine, then the lanes below mine
__device__ __forceinline__ int block_rank256(bool mine, int* part) {
    const unsigned long long m = __ballot(mine);
    const int wv = threadIdx.x >> 6;
    if (lane() == 0) part[wv] = __popcll(m);
    __syncthreads();
    int before = __popcll(m & ((1ull << lane()) - 1ull));
    for (int w = 0; w < wv; w++) before += part[w];
    return before;
}

// The sums of N counters over a workgroup of WAVES waves (256 threads unless told otherwise), added to stats[(first + k) * stride];
// a sum of zero adds nothing, so an idle workgroup issues no atomic.  ALL threads call it, as with the two helpers above.  It owns
// its LDS and opens with a barrier, so a kernel may call it more than once; a caller's own LDS is NOT ordered by its barriers.
// Threads 0 .. N - 1 add in ONE atomic instruction (sums that share a cache line then cost one request, not N); thread k < N gets
// sum k back, every other thread 0.  (Integers: no order can change the result.)
template <int N, int WAVES = 4>
__device__ __forceinline__ unsigned long long block_sums(const unsigned long long (&v)[N], unsigned long long* __restrict__ stats, int first, int stride = 1) {
    __shared__ unsigned long long red[N][WAVES];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) { const unsigned long long s = wave_sum(v[k]); if (lane() == 0) red[k][threadIdx.x >> 6] = s; }
    __syncthreads();
    unsigned long long mine = 0;
    if (threadIdx.x < N) {
#pragma unroll
        for (int w = 0; w < WAVES; w++) mine += red[threadIdx.x][w];
        if (mine) atomicAdd(&stats[(first + (int)threadIdx.x) * stride], mine);
    }
    return mine;
}

// the logical index ([visible | out-of-view], ssf_get_model's order) of slot s = blockIdx.x * 256 + threadIdx.x: slot order is
// logical order, so a visible slot is its own index and an out-of-view slot's is n_visible + (live rows in front of it) =
// bc[its block] (exclusive scan of the blocks' live counts) + its rank inside the block.  holds = slot_row's answer.  (The
// branch is uniform per workgroup; block_rank256's rule applies.)
__device__ __forceinline__ int slot_logical256(const ModelView& mv, bool holds, const uint32_t* __restrict__ bc, int* part) {
    if ((int)blockIdx.x < mv.nbv) return (int)(blockIdx.x * 256u + threadIdx.x);
    return mv.n_visible + (int)bc[blockIdx.x - mv.nbv] + block_rank256(holds, part);
}

// Exclusive scan, in place, of NC interleaved counters per element (a[NC i + s], i < n) by ONE workgroup of 1024 threads, one
// element per thread and round (coalesced); copy (nullable) receives the offsets too.  Sums are kept in Acc and stored as their
// low 32 bits; the totals are left in tot[NC] (LDS), valid for every thread on return.
template <int NC, typename Acc>
__device__ __forceinline__ void workgroup_scan(uint32_t* __restrict__ a, int n, uint32_t* __restrict__ copy, Acc* tot) {
    __shared__ Acc wtot[16][NC];
    if (threadIdx.x < NC) tot[threadIdx.x] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + threadIdx.x;
        Acc c[NC], incl[NC];
#pragma unroll
        for (int s = 0; s < NC; s++) c[s] = i < n ? a[NC * i + s] : 0u;
#pragma unroll
        for (int s = 0; s < NC; s++) {
            Acc v = c[s];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const Acc up = __shfl_up(v, o, 64); if (lane() >= o) v += up; }
            incl[s] = v;
            if (lane() == 63) wtot[threadIdx.x >> 6][s] = v;
        }
        __syncthreads();
        Acc before[NC], all[NC];
#pragma unroll
        for (int s = 0; s < NC; s++) { before[s] = 0; all[s] = 0; }
        for (int w = 0; w < 16; w++)
#pragma unroll
            for (int s = 0; s < NC; s++) { const Acc t = wtot[w][s]; if (w < (int)(threadIdx.x >> 6)) before[s] += t; all[s] += t; }
        if (i < n)
#pragma unroll
            for (int s = 0; s < NC; s++) {
                const uint32_t ex = (uint32_t)(tot[s] + before[s] + incl[s] - c[s]);
                a[NC * i + s] = ex;
                if (copy) copy[NC * i + s] = ex;
            }
        __syncthreads();
        if (threadIdx.x < NC) tot[threadIdx.x] += all[threadIdx.x];
        __syncthreads();
    }
}

// ---- the shared kernels' launchers (ssf_slots.hip).  They open no ScopedKernel: the caller's scope books them ---------------
#pragma GCC visibility push(hidden)
// exclusive scan of n counts in place by one workgroup; a[n] = the total's low 32 bits, cursor (nullable) = a copy of the
// offsets, *total (nullable) = the 64-bit total (a list longer than 2^32 - 1 entries is refused by the host, never wrapped)
void launch_slots_scan(hipStream_t st, uint32_t* a, int n, uint32_t* cursor, unsigned long long* total);
// the same with 32-bit running sums, for a total that is known to fit (the graph's sort: ssf_slots.hip says why it is kept)
void launch_slots_scan32(hipStream_t st, uint32_t* a, int n);
// bc[nbo + 1] = the out-of-view blocks' live offsets (slot_logical256's bc): the live counts, then their scan; nothing for nbo == 0
void launch_slots_oov_offsets(hipStream_t st, const ModelView& mv, uint32_t* bc);
#pragma GCC visibility pop

}  // namespace ssf
