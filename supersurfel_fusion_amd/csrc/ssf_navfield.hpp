// ssf_navfield.hpp -- the tile-round cost-to-goal field that the plan (ssf_navplan.hip: cells) and the pose plan (ssf_navpose.hip:
// states (cell, heading bin)) share: the eight moves, the tile flags and the two ends of a relax kernel on the device; the round loop,
// the growth of the working buffers and the copy-out of the starts' results on the host.  The relaxation of a window and the trace stay
// in the two files.  Private to the library's own files: nothing here is exported.
//
// The scheme: a Bellman-Ford over tiles.  A relax kernel is launched once per ROUND with one 256-thread workgroup per tile, which
// leaves at once when its tile is not flagged (navfield_flagged); otherwise it loads the tile's window -- the tile and a rim of one
// cell -- into LDS, relaxes there until nothing changes, writes back the interior values it lowered and flags, for the next round,
// the neighbour tiles whose window holds a lowered edge or corner cell (navfield_publish).  The flags are two ping-pong arrays with
// the number of set words beside each; the host reads that number once per batch of rounds (navfield_rounds).  No device-wide barrier,
// no spinning kernel, no atomics on the field.
//
// Why the racy reads are benign: a workgroup reads its window's rim from the interiors of neighbours that may be lowering them in
// the same round.  Every value ever stored is the cost of a real path -- a real sequence of admissible transitions -- to a goal,
// values only decrease, and whoever lowers a value of an edge cell flags every tile whose window holds that cell for the next round
// (a launch boundary makes the stores visible).  So whichever value was read, the reader runs again on the final one; when no tile
// is flagged, every tile is at its fixed point for the window it would load, and that fixed point is the field: all weights are
// positive.  The field is stored with plain aligned 32-bit stores.
#pragma once
#include "ssf_navgrid.hpp"

namespace ssf {

enum : uint32_t { NAVF_INF = 0xFFFFFFFFu };
// where a caller's sums hold the (round, tile) visits, the last round that worked + 1, and the set words of the two flag arrays
struct NavFieldSums { int visits, rounds, flagged; };

// move k = 0..7: (+1,0), (0,+1), (-1,0), (0,-1), (+1,+1), (-1,+1), (-1,-1), (+1,-1); 10 along an axis, 14 across
__device__ __forceinline__ int navfield_dx(int k) { return (int)((0x8246u >> (2 * k)) & 3u) - 1; }     // dx + 1 = 2 1 0 1 2 0 0 2
__device__ __forceinline__ int navfield_dy(int k) { return (int)((0x0A19u >> (2 * k)) & 3u) - 1; }     // dy + 1 = 1 2 1 0 2 2 0 0
__device__ __forceinline__ uint32_t navfield_w(int k) { return k < 4 ? 10u : 14u; }
// the near-obstacle penalty of a cell at squared clearance d
__device__ __forceinline__ uint32_t navfield_penalty(int d, int soft_dist2, int near_penalty) {
    const int dc = d < 0 ? 0 : (d < soft_dist2 ? d : soft_dist2);
    return soft_dist2 > 0 ? (uint32_t)(near_penalty * (soft_dist2 - dc) / soft_dist2) : 0u;
}

// flag tile t in `flags` (counted once, however many set it)
__device__ __forceinline__ void navfield_flag(uint32_t* __restrict__ flags, unsigned long long* __restrict__ flagged, int t) {
    if (flags[t] == 0u && atomicExch(&flags[t], 1u) == 0u) atomicAdd(flagged, 1ull);      // (a word only goes 0 -> 1 while it is being set)
}
// bit (sy + 1) * 3 + (sx + 1) for every tile offset (sx, sy) whose window holds cell (lx, ly) of a SIDE x SIDE tile (bit 4: the tile itself)
template <int SIDE>
__device__ __forceinline__ uint32_t navfield_seers(int lx, int ly) {
    const int sx = lx == 0 ? -1 : (lx == SIDE - 1 ? 1 : 0), sy = ly == 0 ? -1 : (ly == SIDE - 1 ? 1 : 0);
    uint32_t m = 1u << 4;
    if (sx) m |= 1u << (3 + (sx + 1));
    if (sy) m |= 1u << ((sy + 1) * 3 + 1);
    if (sx && sy) m |= 1u << ((sy + 1) * 3 + (sx + 1));
    return m;
}
__device__ __forceinline__ void navfield_flag_bit(int ntx, int nty, int tx, int ty, int bit, uint32_t* __restrict__ flags,
                                                  unsigned long long* __restrict__ flagged) {
    const int nx = tx + bit % 3 - 1, ny = ty + bit / 3 - 1;
    if (nx >= 0 && nx < ntx && ny >= 0 && ny < nty) navfield_flag(flags, flagged, ny * ntx + nx);
}
// flag every tile whose window holds cell (x, y) of the grid: what sets a goal does
template <int SIDE>
__device__ __forceinline__ void navfield_flag_seers(int ntx, int nty, int x, int y, uint32_t* __restrict__ flags, unsigned long long* __restrict__ flagged) {
    const uint32_t m = navfield_seers<SIDE>(x & (SIDE - 1), y & (SIDE - 1));
    for (int b = 0; b < 9; b++) if ((m >> b) & 1u) navfield_flag_bit(ntx, nty, x / SIDE, y / SIDE, b, flags, flagged);
}

// The two ends of a relax kernel, one workgroup per tile blockIdx.x.  flagged: false when the tile is not flagged -- the same word for
// every thread, nobody clears it before publish's barrier -- and the workgroup leaves at once (the test stays the kernel's first
// instructions: most workgroups of a round end here).  publish: *seers is one word of LDS that the kernel cleared before its last
// barrier; `mine` = the seers of the cells this thread lowered (0: none); the neighbour tiles that see a lowered cell are flagged
// for the next round, the own flag is cleared, the visit is counted.
__device__ __forceinline__ bool navfield_flagged(const uint32_t* fcur) { return fcur[blockIdx.x] != 0u; }
__device__ __forceinline__ void navfield_publish(int ntx, int nty, uint32_t mine, uint32_t* seers, uint32_t* fcur, uint32_t* fnxt,
                                                 unsigned long long* __restrict__ stats, const NavFieldSums& S, int cur, unsigned long long round) {
    const int t = blockIdx.x;
    mine &= ~(1u << 4);
    if (mine) atomicOr(seers, mine);
    __syncthreads();
    if (threadIdx.x < 9 && ((*seers >> threadIdx.x) & 1u)) navfield_flag_bit(ntx, nty, t % ntx, t / ntx, threadIdx.x, fnxt, &stats[S.flagged + (cur ^ 1)]);
    if (threadIdx.x == 0) {
        fcur[t] = 0u;
        atomicAdd(&stats[S.flagged + cur], ~0ull);                    // (- 1)
        atomicAdd(&stats[S.visits], 1ull);
        atomicMax(&stats[S.rounds], round + 1ull);
    }
}

// the maximum of v over a workgroup of 256 into *dst, when it is > 0.  ALL threads call it; it owns its LDS and opens with a barrier,
// as block_sums (ssf_slots.hpp) does
__device__ __forceinline__ void navfield_block_max(unsigned long long v, unsigned long long* __restrict__ dst) {
    __shared__ unsigned long long red[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
    __syncthreads();
    if (lane() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
        if ((a > b ? a : b) > 0ull) atomicMax(dst, a > b ? a : b);
    }
}

}  // namespace ssf

#pragma GCC visibility push(hidden)
// ---- the host's part; Ws is NavPlanWs or NavPoseWs (ssf_handle.hpp), `who` words the errors -------------------------------------
// the buffers of the goals, the starts and the starts' results (`words` per goal or start entry: 2 or 3), the flags of `tiles` tiles,
// and, for a host caller, the paths
template <class Ws>
bool navfield_reserve(Ws& w, size_t n_sums, int words, size_t tiles, size_t path_words) {
    bool ok = true;
    if (!w.stats) ok = w.bufs.grow({{(void**)&w.stats, n_sums * sizeof(unsigned long long)}, {(void**)&w.goals, 65536 * words * sizeof(int32_t)},
                                    {(void**)&w.starts, 4096 * words * sizeof(int32_t)}, {(void**)&w.start_cost, 4096 * sizeof(uint32_t)},
                                    {(void**)&w.start_status, 4096 * sizeof(int32_t)}, {(void**)&w.path_len, 4096 * sizeof(int32_t)}});
    if (ok && tiles > w.tiles) { ok = w.bufs.grow({{(void**)&w.flags, 2 * tiles * sizeof(uint32_t)}}); if (ok) w.tiles = tiles; }
    if (ok && path_words > w.path_words) { ok = w.bufs.grow({{(void**)&w.path, path_words * sizeof(int32_t)}}); if (ok) w.path_words = path_words; }
    return ok;
}

// the rounds: round r reads the flags of array r & 1 and sets those of the other; the host looks at stats[flagged + (r & 1)] once per
// batch.  launch(round, cur) launches round `round` under its own ScopedKernel
template <class Launch>
int navfield_rounds(ssf_handle* h, const char* who, const unsigned long long* stats, int flagged_at, long long limit, int batch, Launch launch) {
    long long round = 0;
    for (;;) {
        unsigned long long flagged = 0;
        HCK(hipMemcpyAsync(&flagged, stats + flagged_at + (round & 1), sizeof(flagged), hipMemcpyDeviceToHost, h->stream));
        { int rc = sync_collect(h); if (rc) return rc; }
        if (flagged == 0) return SSF_OK;
        if (round >= limit) { h->err = std::string(who) + ": the field did not converge"; return SSF_ERR_DEVICE; }
        for (int i = 0; i < batch && round < limit; i++, round++) { launch(round, (int)(round & 1)); HCK(hipGetLastError()); }
    }
}

// the starts' results to the caller, and of each path its first path_len entries of `words` words (entries past path_len are not
// written).  It synchronises; the caller's other copies, queued before it, are done when it returns.  path: nullptr when no host
// caller wants one
template <class Ws>
int navfield_copy_out(ssf_handle* h, const Ws& w, int ns, int max_path, int words, hipMemcpyKind kind, uint32_t* start_cost, int32_t* start_status,
                      int32_t* path_len, int32_t* path) {
    hipStream_t st = h->stream;
    int32_t lens[4096];                                               // (n_starts <= 4096)
    if (ns > 0) {
        if (start_cost) HCK(hipMemcpyAsync(start_cost, w.start_cost, 4 * (size_t)ns, kind, st));
        if (start_status) HCK(hipMemcpyAsync(start_status, w.start_status, 4 * (size_t)ns, kind, st));
        if (path_len) HCK(hipMemcpyAsync(path_len, w.path_len, 4 * (size_t)ns, kind, st));
        if (path) HCK(hipMemcpyAsync(lens, w.path_len, 4 * (size_t)ns, hipMemcpyDeviceToHost, st));
    }
    { int rc = sync_collect(h); if (rc) return rc; }
    if (path) {
        const size_t per = (size_t)max_path * words;
        for (int i = 0; i < ns; i++)
            if (lens[i] > 0) HCK(hipMemcpyAsync(path + i * per, w.path + i * per, 4 * (size_t)words * (size_t)lens[i], hipMemcpyDeviceToHost, st));
        HCK(hipStreamSynchronize(st));
    }
    return SSF_OK;
}
#pragma GCC visibility pop
