// ssf_navpose.hip -- plan over (x, y, heading) on the navigation grid (include/ssf_navpose.h) on gfx950: the cost-to-goal field over
// (cell, heading bin), its projection onto the cells and the state paths down it.
//
// What is computed is pinned in include/ssf_navpose.h (the restatement: tests/navpose_ref.py).  ssf_navpose_field runs
//   * moves    ssf_navpose_moves: host only.  Per bin the eight moves as forward / reverse / none; the kernels get the table as a
//              kernel argument of 2 bits a move (64 bytes), read with the bin as a wave-uniform index;
//   * init     k_navpose_init: one thread per cell: the traversable bins and the penalty packed into one 8-byte word, the cell's B
//              field entries set to the marker; k_navpose_goals: one thread per goal entry: the goal states at 0, and the flags of
//              the 16 x 16-cell tiles whose window holds the goal's cell;
//   * relax    k_navpose_relax, one launch per ROUND, one workgroup per flagged tile: the tile-round scheme of ssf_navfield.hpp, which
//              also says why its racy reads are benign.  The workgroup loads the tile's 18 x 18 window -- the packed word and all B
//              layers of the field -- into LDS and sweeps there until a sweep stores nothing.  A thread owns one cell and walks its
//              column of bins: per bin the moves of that bin from the same layer's neighbours, then the two rotations; an ascending
//              sweep carries a lowered value round the column in one go, a descending sweep of rotations alone does the same the
//              other way.  The column stays in LDS (no dynamically indexed register array, so no scratch).  Rotations stay inside a
//              cell, so they add no reader outside the window;
//   * stats    k_navpose_stats: one thread per cell: cell_cost, cell_bin, the reached states and cells, the largest cost;
//   * trace    k_navpose_trace: one wave per start, lanes 0..9 the ten transitions, a wave minimum over (value, t).
//
// LDS: (2 + B) * 324 words, 41.0 KiB + 2.5 KiB at B = 32, asked for per launch (dynamic), so a smaller B leaves room for more
// workgroups.  It never passes the 64 KiB a workgroup gets without opting into more.
//
// This file is NOT one of the product library's objects.  It is linked, with all of them and the older navigation files, into
// libssf_hip_pose.so.
#include "ssf_navfield.hpp"
#include "../../include/ssf_navpose.h"

namespace ssf {

enum { NQ_TILE = SSF_NAVPOSE_TILE, NQ_WIN = NQ_TILE + 2, NQ_WIN_CELLS = NQ_WIN * NQ_WIN };
enum : uint32_t { NQ_INF = NAVF_INF };
// the sums: traversable states, goal entries used / blocked / outside, reached states, reached cells, largest cost, (round, tile)
// visits, the last round that worked + 1, the set words of the two flag arrays
enum { NQ_NTRAV = 0, NQ_GUSED = 1, NQ_GBLOCKED = 2, NQ_GOUTSIDE = 3, NQ_REACHED = 4, NQ_CELLS = 5, NQ_MAXCOST = 6, NQ_VISITS = 7, NQ_ROUNDS = 8,
       NQ_FLAGGED = 9, NQ_STATS = 12 };
constexpr NavFieldSums NQ_SUMS{NQ_VISITS, NQ_ROUNDS, NQ_FLAGGED};
static_assert((2 + SSF_NAVFOOT_MAX_HEADINGS) * NQ_WIN_CELLS * 4 <= 64 * 1024, "a workgroup's window must fit the LDS it gets without opting into more");

struct NavPoseGrid { int W, H, B, ntx, nty; };
struct NavPoseRule { int min_dist2, soft_dist2, near_penalty, reverse_cost, turn_cost; };
struct NavPoseMoves { uint32_t m[SSF_NAVFOOT_MAX_HEADINGS / 2]; };        // bin b: bits 16 (b & 1) + 2 k: 0 none, 1 forward, 2 reverse

// (the moves k = 0..7 and their weights: ssf_navfield.hpp)
__device__ __forceinline__ uint32_t nq_codes(const NavPoseMoves& mv, int b) { return (mv.m[b >> 1] >> (16 * (b & 1))) & 0xFFFFu; }


// ---- init: one thread per cell (steps 1 and 2); the field set to the marker ---------------------------------------------------------
__global__ __launch_bounds__(256) void k_navpose_init(NavPoseGrid G, NavPoseRule r, const uint32_t* __restrict__ mask, const int32_t* __restrict__ dist2,
                                                      uint2* __restrict__ pk, uint32_t* __restrict__ cost, unsigned long long* __restrict__ stats) {
    const size_t P = (size_t)G.W * G.H, p = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long ntrav = 0;
    if (p < P) {
        const int d = dist2[p];
        const uint32_t all = G.B == 32 ? 0xFFFFFFFFu : (1u << G.B) - 1u;
        const uint32_t tr = d >= r.min_dist2 ? mask[p] & all : 0u;
        pk[p] = make_uint2(tr, navfield_penalty(d, r.soft_dist2, r.near_penalty));
        for (int b = 0; b < G.B; b++) cost[(size_t)b * P + p] = NQ_INF;
        ntrav = (unsigned long long)__popc(tr);
    }
    block_sums({ntrav}, stats, NQ_NTRAV);
}

// goals: one thread per entry of the caller's list (step 6); runs behind k_navpose_init
__global__ __launch_bounds__(256) void k_navpose_goals(NavPoseGrid G, const int32_t* __restrict__ goals, int n, const uint2* __restrict__ pk,
                                                       uint32_t* __restrict__ cost, uint32_t* __restrict__ flags, unsigned long long* __restrict__ stats) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    unsigned long long used = 0, blocked = 0, outside = 0;
    if (g < n) {
        const int x = goals[3 * g], y = goals[3 * g + 1], bin = goals[3 * g + 2];
        if (x < 0 || x >= G.W || y < 0 || y >= G.H || bin < -1 || bin >= G.B) outside = 1;
        else {
            const size_t P = (size_t)G.W * G.H, p = (size_t)y * G.W + x;
            const uint32_t tr = pk[p].x, sel = bin < 0 ? tr : tr & (1u << bin);
            if (!sel) blocked = 1;
            else {
                used = 1;
                for (int b = 0; b < G.B; b++) if ((sel >> b) & 1u) cost[(size_t)b * P + p] = 0u;
                navfield_flag_seers<NQ_TILE>(G.ntx, G.nty, x, y, flags, &stats[NQ_FLAGGED]);
            }
        }
    }
    block_sums({used, blocked, outside}, stats, NQ_GUSED);
}

// ---- relax: one round; one workgroup per tile, gone at once when the tile is not flagged ------------------------------------------
// Thread t owns cell (t & 15, t >> 4) of its tile and that cell's column of bins.  Inside LDS the sweep is racy on purpose: a thread
// may read a neighbour's state before or after its owner lowered it; the loop ends only after a sweep in which NO thread stored, and
// in that sweep every read saw the final values.  Window cells outside the grid hold (no bin traversable, INF); a state that is not
// traversable holds INF for ever, so a finite value read from a neighbour is the cost of a traversable state.
__global__ __launch_bounds__(256) void k_navpose_relax(NavPoseGrid G, NavPoseMoves mv, uint32_t rev, uint32_t turn, const uint2* __restrict__ pk, uint32_t* cost,
                                                       uint32_t* fcur, uint32_t* fnxt, unsigned long long* __restrict__ stats, int cur, unsigned long long round) {
    extern __shared__ uint32_t nq_lds[];
    uint32_t* const sm = nq_lds;                                      // [324] the traversable bins
    uint32_t* const sp = nq_lds + NQ_WIN_CELLS;                       // [324] the penalty
    uint32_t* const sc = nq_lds + 2 * NQ_WIN_CELLS;                   // [B][324] the field
    __shared__ uint32_t seers;
    if (!navfield_flagged(fcur)) return;
    const int B = G.B;
    const size_t P = (size_t)G.W * G.H;
    const int t = blockIdx.x, tx = t % G.ntx, ty = t / G.ntx;
    const int x0 = tx * NQ_TILE - 1, y0 = ty * NQ_TILE - 1;
    for (int i = threadIdx.x; i < NQ_WIN_CELLS; i += 256) {
        const int gx = x0 + i % NQ_WIN, gy = y0 + i / NQ_WIN;
        const bool in = gx >= 0 && gx < G.W && gy >= 0 && gy < G.H;
        const uint2 w = in ? pk[(size_t)gy * G.W + gx] : make_uint2(0u, 0u);
        sm[i] = w.x; sp[i] = w.y;
    }
    if (threadIdx.x == 0) seers = 0u;
    __syncthreads();
    for (int j = threadIdx.x; j < B * NQ_WIN_CELLS; j += 256) {
        const int b = j / NQ_WIN_CELLS, i = j - b * NQ_WIN_CELLS;
        const int gx = x0 + i % NQ_WIN, gy = y0 + i / NQ_WIN;        // (a set bit of sm[i] says the cell is inside the grid)
        sc[j] = (sm[i] >> b) & 1u ? cost[(size_t)b * P + (size_t)gy * G.W + gx] : (uint32_t)NQ_INF;
    }
    __syncthreads();
    const int lx = threadIdx.x & (NQ_TILE - 1), ly = threadIdx.x >> 4;
    const int c = (ly + 1) * NQ_WIN + lx + 1;
    const uint32_t my = sm[c];
    // per move the bins at which it is admissible from this cell (target and, across, the two axial cells traversable) and w + pen
    uint32_t okm[8], add[8];
    {
        const uint32_t right = sm[c + 1], down = sm[c + NQ_WIN], left = sm[c - 1], up = sm[c - NQ_WIN];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int dx = navfield_dx(k), dy = navfield_dy(k), q = c + dy * NQ_WIN + dx;
            uint32_t m = sm[q] & my;
            if (k >= 4) m &= (dx > 0 ? right : left) & (dy > 0 ? down : up);
            okm[k] = m; add[k] = navfield_w(k) + sp[q];
        }
    }
    uint32_t lowered = 0u;
    for (;;) {
        int changed = 0;
        if (my) {
            uint32_t prev = sc[(B - 1) * NQ_WIN_CELLS + c];           // the value of bin b - 1 (for B = 1: the state itself, not used)
            for (int b = 0; b < B; b++) {
                uint32_t have = sc[b * NQ_WIN_CELLS + c];
                if ((my >> b) & 1u) {
                    uint32_t best = have;
                    const uint32_t codes = nq_codes(mv, b);
#pragma unroll
                    for (int k = 0; k < 8; k++) {
                        const uint32_t code = (codes >> (2 * k)) & 3u;
                        if (code && ((okm[k] >> b) & 1u)) {
                            const uint32_t cq = sc[b * NQ_WIN_CELLS + c + navfield_dy(k) * NQ_WIN + navfield_dx(k)];
                            if (cq != NQ_INF) { const uint32_t v = cq + add[k] + (code == 2u ? rev : 0u); best = v < best ? v : best; }
                        }
                    }
                    if (B > 1) {
                        const uint32_t nxt = sc[((b + 1) & (B - 1)) * NQ_WIN_CELLS + c];
                        if (prev != NQ_INF && prev + turn < best) best = prev + turn;
                        if (nxt != NQ_INF && nxt + turn < best) best = nxt + turn;
                    }
                    if (best < have) { sc[b * NQ_WIN_CELLS + c] = best; lowered |= 1u << b; changed = 1; have = best; }
                }
                prev = have;
            }
            if (B > 2) {                                              // the rotations the other way round, carried down the column
                uint32_t nxt = sc[c];
                for (int b = B - 1; b >= 0; b--) {
                    uint32_t have = sc[b * NQ_WIN_CELLS + c];
                    if (((my >> b) & 1u) && nxt != NQ_INF && nxt + turn < have) { have = nxt + turn; sc[b * NQ_WIN_CELLS + c] = have; lowered |= 1u << b; changed = 1; }
                    nxt = have;
                }
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
    if (lowered) {                                                    // (a lowered state is traversable, so its cell is inside the grid)
        const size_t p = (size_t)(y0 + 1 + ly) * G.W + (x0 + 1 + lx);
        for (int b = 0; b < B; b++) if ((lowered >> b) & 1u) cost[(size_t)b * P + p] = sc[b * NQ_WIN_CELLS + c];
    }
    navfield_publish(G.ntx, G.nty, lowered ? navfield_seers<NQ_TILE>(lx, ly) : 0u, &seers, fcur, fnxt, stats, NQ_SUMS, cur, round);
}

// ---- stats and projection: one thread per cell (steps 8 and 10) ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navpose_stats(NavPoseGrid G, const uint32_t* __restrict__ cost, uint32_t* __restrict__ cell_cost,
                                                       uint8_t* __restrict__ cell_bin, unsigned long long* __restrict__ stats) {
    const size_t P = (size_t)G.W * G.H, p = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long reached = 0, cells = 0, mx = 0;
    if (p < P) {
        uint32_t best = NQ_INF; int bin = SSF_NAVPOSE_NO_BIN;
        for (int b = 0; b < G.B; b++) {
            const uint32_t v = cost[(size_t)b * P + p];
            if (v != NQ_INF) { reached++; mx = v > mx ? v : mx; if (v < best) { best = v; bin = b; } }
        }
        cell_cost[p] = best; cell_bin[p] = (uint8_t)bin;
        cells = reached != 0;
    }
    block_sums({reached, cells}, stats, NQ_REACHED);
    navfield_block_max(mx, &stats[NQ_MAXCOST]);
}

// ---- trace: one wave per start (step 9) -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_navpose_trace(NavPoseGrid G, NavPoseMoves mv, uint32_t rev, uint32_t turn, int shift, const uint2* __restrict__ pk,
                                                       const uint32_t* __restrict__ cost, const int32_t* __restrict__ starts, int n, int max_path,
                                                       uint32_t* __restrict__ start_cost, int32_t* __restrict__ start_status, int32_t* __restrict__ path_len,
                                                       int32_t* __restrict__ path) {
    const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (w >= n) return;
    const int ln = lane(), B = G.B;
    const size_t P = (size_t)G.W * G.H;
    int x = starts[3 * w] >> 10, y = starts[3 * w + 1] >> 10;
    int b = (int)(((((uint32_t)starts[3 * w + 2] & 0xFFFFu) + (shift > 0 ? 1u << (shift - 1) : 0u)) >> shift) & (uint32_t)(B - 1));
    int status = 0, len = 0;
    uint32_t c = NQ_INF;
    if (x < 0 || x >= G.W || y < 0 || y >= G.H) status = 1;
    else if (!((pk[(size_t)y * G.W + x].x >> b) & 1u)) status = 2;
    else { c = cost[(size_t)b * P + (size_t)y * G.W + x]; if (c == NQ_INF) status = 3; }
    const uint32_t c0 = c;
    if (status == 0 && max_path > 0) {
        int32_t* out = path + (size_t)w * (size_t)max_path * 3;
        for (;;) {                                                    // (wave-uniform: x, y, b, c, len are the same in every lane)
            if (len == max_path) { status = 4; break; }
            if (ln == 0 && path) { out[3 * (size_t)len] = x; out[3 * (size_t)len + 1] = y; out[3 * (size_t)len + 2] = b; }
            len++;
            if (c == 0u) break;
            unsigned long long key = ~0ull;
            uint32_t cq = NQ_INF;
            if (ln < 8) {
                const uint32_t code = (nq_codes(mv, b) >> (2 * ln)) & 3u;
                const int dx = navfield_dx(ln), dy = navfield_dy(ln), qx = x + dx, qy = y + dy;
                if (code && qx >= 0 && qx < G.W && qy >= 0 && qy < G.H) {
                    const uint2 pq = pk[(size_t)qy * G.W + qx];
                    bool ok = (pq.x >> b) & 1u;
                    if (ok && ln >= 4) ok = ((pk[(size_t)y * G.W + qx].x >> b) & 1u) && ((pk[(size_t)qy * G.W + x].x >> b) & 1u);
                    if (ok) {
                        cq = cost[(size_t)b * P + (size_t)qy * G.W + qx];
                        if (cq != NQ_INF) key = ((unsigned long long)(cq + navfield_w(ln) + pq.y + (code == 2u ? rev : 0u)) << 4) | (unsigned long long)ln;
                    }
                }
            } else if (ln < 10 && B > 1) {
                const int nb = (ln == 8 ? b + 1 : b - 1) & (B - 1);
                if ((pk[(size_t)y * G.W + x].x >> nb) & 1u) {
                    cq = cost[(size_t)nb * P + (size_t)y * G.W + x];
                    if (cq != NQ_INF) key = ((unsigned long long)(cq + turn) << 4) | (unsigned long long)ln;
                }
            }
            key = wave_min64(key);
            if (key == ~0ull) { status = 3; break; }                  // (not on a settled field: a state of finite cost > 0 has such a successor)
            const int k = (int)(key & 15ull);
            c = __shfl(cq, k, 64);
            if (k < 8) { x += navfield_dx(k); y += navfield_dy(k); }
            else b = (k == 8 ? b + 1 : b - 1) & (B - 1);
        }
    }
    if (ln == 0) { start_cost[w] = c0; start_status[w] = status; path_len[w] = len; }
}

// the move table of the header's steps 3 and 5; nullptr when it is made, else what is wrong
static const char* navpose_moves(int B, int move_tol, int allow_reverse, int8_t* out) {
    if (nav_log2_bins(B) < 0) return "n_headings must be 1, 2, 4, 8, 16 or 32";
    if (move_tol < 0 || move_tol > 256) return "move_tol must be 0..256";
    if (allow_reverse != 0 && allow_reverse != 1) return "allow_reverse must be 0 or 1";
    static const int A[8] = {0, 256, 512, 768, 128, 384, 640, 896};
    auto circ = [](int a, int b) { const int u = (a - b) & 1023, v = (b - a) & 1023; return u < v ? u : v; };
    for (int b = 0; b < B; b++)
        for (int k = 0; k < 8; k++) {
            const int kb = b * (1024 / B);
            out[b * 8 + k] = circ(kb, A[k]) <= move_tol ? 1 : (allow_reverse && circ(kb + 512, A[k]) <= move_tol ? 2 : 0);
        }
    return nullptr;
}

}  // namespace ssf

extern "C" {
int ssf_navpose_moves(int n_headings, int move_tol, int allow_reverse, int8_t* out) {
    if (!out) return SSF_ERR_INVALID_ARG;
    return ssf::navpose_moves(n_headings, move_tol, allow_reverse, out) ? SSF_ERR_INVALID_ARG : SSF_OK;
}

int ssf_navpose_default_params(const ssf_handle* h, ssf_navpose_params* p) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    std::memset(p, 0, sizeof(*p));
    p->width = 512; p->height = 512; p->n_headings = 16;
    p->move_tol = 64; p->allow_reverse = 1; p->reverse_cost = 10; p->turn_cost = 5;
    return SSF_OK;
}

int ssf_navpose_field(ssf_handle* h, const ssf_navpose_params* p, const uint32_t* free_mask, const int32_t* dist2, const ssf_navpose_out* out,
                      ssf_navpose_stats* stats) {
    if (!h || !p) return SSF_ERR_INVALID_ARG;
    auto refuse = [&](const char* what) { h->err = std::string("ssf_navpose_field: ") + what; return SSF_ERR_INVALID_ARG; };
    if (!free_mask || !dist2) return refuse("free_mask or dist2 is NULL");
    if (!out || (!out->cost && !out->cell_cost && !out->cell_bin && !out->start_cost && !out->start_status && !out->path_len && !out->path))
        return refuse("every output is NULL");
    const int lg = nav_log2_bins(p->n_headings);
    if (lg < 0) return refuse("n_headings must be 1, 2, 4, 8, 16 or 32");
    if (p->width < 1 || p->width > 4096 || p->height < 1 || p->height > 4096) return refuse("the grid's size must be 1..4096 x 1..4096");
    const size_t P = (size_t)p->width * p->height, N = P * (size_t)p->n_headings;
    if (N > (size_t)SSF_NAVPOSE_MAX_STATES) return refuse("width * height * n_headings must be <= 1 << 26");
    if (p->min_dist2 < 0) return refuse("min_dist2 must be >= 0");
    if (p->soft_dist2 < 0 || p->soft_dist2 > 1024 * 1024) return refuse("soft_dist2 must be 0..1024 * 1024");
    if (p->near_penalty < 0 || p->near_penalty > 1000) return refuse("near_penalty must be 0..1000");
    if (p->move_tol < 0 || p->move_tol > 256) return refuse("move_tol must be 0..256");
    if (p->allow_reverse != 0 && p->allow_reverse != 1) return refuse("allow_reverse must be 0 or 1");
    if (p->reverse_cost < 0 || p->reverse_cost > 1000) return refuse("reverse_cost must be 0..1000");
    if (p->turn_cost < 1 || p->turn_cost > 1000) return refuse("turn_cost must be 1..1000");
    if (p->n_goals < 1 || p->n_goals > 65536) return refuse("n_goals must be 1..65536");
    if (p->n_starts < 0 || p->n_starts > 4096) return refuse("n_starts must be 0..4096");
    if (p->max_path < 0 || p->max_path > (1 << 20)) return refuse("max_path must be 0..1 << 20");
    if (!p->goals) return refuse("goals is NULL");
    if (p->n_starts > 0 && !p->starts) return refuse("starts is NULL");
    const unsigned long long step = (unsigned long long)std::max(14 + p->near_penalty + p->reverse_cost, p->turn_cost);
    if (step * (unsigned long long)N >= 0xFFFFFFFFull)
        return refuse("max(14 + near_penalty + reverse_cost, turn_cost) * width * height * n_headings must be < 2^32 - 1, so that no cost can wrap");
    { int rc = model_at_rest(h, "ssf_navpose_field", "plans on no navigation grid"); if (rc) return rc; }

    const int B = p->n_headings;
    const NavPoseGrid G{p->width, p->height, B, (p->width + NQ_TILE - 1) / NQ_TILE, (p->height + NQ_TILE - 1) / NQ_TILE};
    const NavPoseRule rule{p->min_dist2, p->soft_dist2, p->near_penalty, p->reverse_cost, p->turn_cost};
    NavPoseMoves mv;
    {
        int8_t table[SSF_NAVFOOT_MAX_HEADINGS * 8];
        navpose_moves(B, p->move_tol, p->allow_reverse, table);
        std::memset(&mv, 0, sizeof(mv));
        for (int b = 0; b < B; b++)
            for (int k = 0; k < 8; k++) mv.m[b >> 1] |= (uint32_t)table[b * 8 + k] << (16 * (b & 1) + 2 * k);
    }
    const size_t tiles = (size_t)G.ntx * G.nty;
    const int ns = p->n_starts;
    const bool dev = p->on_device != 0, want_path = out->path && ns > 0 && p->max_path > 0;
    const size_t path_words = want_path ? (size_t)ns * (size_t)p->max_path * 3 : 0;
    // the working buffers; a call with device arrays relaxes the caller's field and projects into the caller's arrays, a host grid
    // is staged on the device
    NavPoseWs& w = h->navpose;
    const bool own_cost = !(dev && out->cost);
    const uint32_t* d_mask = free_mask; const int32_t* d_dist2 = dist2;
    StagedIo io;
    if (!dev) { io.in(free_mask, 4 * P, &d_mask); io.in(dist2, 4 * P, &d_dist2); }
    bool ok = navfield_reserve(w, NQ_STATS, 3, tiles, dev ? 0 : path_words);
    if (ok && P > w.cells) {
        ok = w.bufs.grow({{(void**)&w.pk, 8 * P}, {(void**)&w.cell_cost, 4 * P}, {(void**)&w.cell_bin, P}});
        if (ok) w.cells = P;
    }
    if (ok && own_cost && N > w.states) { ok = w.bufs.grow({{(void**)&w.cost, 4 * N}}); if (ok) w.states = N; }
    if (ok) ok = io.reserve(w.bufs, &w.io, &w.io_bytes, io.need());
    if (!ok) { h->err = "ssf_navpose_field: allocation of the working buffers failed"; return SSF_ERR_DEVICE; }

    hipStream_t st = h->stream;
    TimerScope ts(h);
    HCK(io.copy_in(st));
    uint32_t* d_cost = own_cost ? w.cost : out->cost;
    uint32_t* d_cell_cost = dev && out->cell_cost ? out->cell_cost : w.cell_cost;
    uint8_t* d_cell_bin = dev && out->cell_bin ? out->cell_bin : w.cell_bin;
    uint2* d_pk = (uint2*)w.pk;
    HCK(hipMemcpyAsync(w.goals, p->goals, 3 * sizeof(int32_t) * (size_t)p->n_goals, hipMemcpyHostToDevice, st));
    if (ns > 0) HCK(hipMemcpyAsync(w.starts, p->starts, 3 * sizeof(int32_t) * (size_t)ns, hipMemcpyHostToDevice, st));
    HCK(hipMemsetAsync(w.stats, 0, NQ_STATS * sizeof(unsigned long long), st));
    HCK(hipMemsetAsync(w.flags, 0, 2 * tiles * sizeof(uint32_t), st));
    {
        ScopedKernel sk("navpose_init", st);
        hipLaunchKernelGGL(k_navpose_init, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, G, rule, d_mask, d_dist2, d_pk, d_cost, w.stats);
    }
    HCK(hipGetLastError());
    {
        ScopedKernel sk("navpose_goals", st);
        hipLaunchKernelGGL(k_navpose_goals, dim3((unsigned)((p->n_goals + 255) / 256)), dim3(256), 0, st, G, (const int32_t*)w.goals, p->n_goals,
                           (const uint2*)d_pk, d_cost, w.flags, w.stats);
    }
    HCK(hipGetLastError());
    // the rounds: round r reads the flags of array r & 1 and sets those of the other; the host looks once per batch
    const size_t lds = (size_t)(2 + B) * NQ_WIN_CELLS * sizeof(uint32_t);
    {
        int rc = navfield_rounds(h, "ssf_navpose_field", w.stats, NQ_FLAGGED, (long long)N + 2, SSF_NAVPOSE_ROUND_BATCH, [&](long long round, int cur) {
            ScopedKernel sk("navpose_relax", st);
            hipLaunchKernelGGL(k_navpose_relax, dim3((unsigned)tiles), dim3(256), lds, st, G, mv, (uint32_t)p->reverse_cost, (uint32_t)p->turn_cost,
                               (const uint2*)d_pk, d_cost, w.flags + (size_t)cur * tiles, w.flags + (size_t)(cur ^ 1) * tiles, w.stats, cur,
                               (unsigned long long)round);
        });
        if (rc) return rc;
    }
    {
        ScopedKernel sk("navpose_stats", st);
        hipLaunchKernelGGL(k_navpose_stats, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, G, (const uint32_t*)d_cost, d_cell_cost, d_cell_bin, w.stats);
    }
    HCK(hipGetLastError());
    int32_t* d_path = want_path ? (dev ? out->path : w.path) : nullptr;      // (no path array: the trace still tells length and status)
    if (ns > 0) {
        ScopedKernel sk("navpose_trace", st);
        hipLaunchKernelGGL(k_navpose_trace, dim3((unsigned)((ns + 3) / 4)), dim3(256), 0, st, G, mv, (uint32_t)p->reverse_cost, (uint32_t)p->turn_cost, 16 - lg,
                           (const uint2*)d_pk, (const uint32_t*)d_cost, (const int32_t*)w.starts, ns, p->max_path, w.start_cost, w.start_status, w.path_len,
                           d_path);
    }
    HCK(hipGetLastError());
    // the outputs
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    unsigned long long s[NQ_STATS];
    HCK(hipMemcpyAsync(s, w.stats, sizeof(s), hipMemcpyDeviceToHost, st));
    if (out->cost && out->cost != d_cost) HCK(hipMemcpyAsync(out->cost, d_cost, 4 * N, kind, st));
    if (out->cell_cost && out->cell_cost != d_cell_cost) HCK(hipMemcpyAsync(out->cell_cost, d_cell_cost, 4 * P, kind, st));
    if (out->cell_bin && out->cell_bin != d_cell_bin) HCK(hipMemcpyAsync(out->cell_bin, d_cell_bin, P, kind, st));
    {
        int rc = navfield_copy_out(h, w, ns, p->max_path, 3, kind, out->start_cost, out->start_status, out->path_len, want_path && !dev ? out->path : nullptr);
        if (rc) return rc;
    }
    if (stats) {
        stats->states_traversable = (int64_t)s[NQ_NTRAV]; stats->states_reached = (int64_t)s[NQ_REACHED]; stats->cells_reached = (int64_t)s[NQ_CELLS];
        stats->goals_used = (int64_t)s[NQ_GUSED]; stats->goals_blocked = (int64_t)s[NQ_GBLOCKED]; stats->goals_outside = (int64_t)s[NQ_GOUTSIDE];
        stats->max_cost = (int64_t)s[NQ_MAXCOST]; stats->rounds = (int64_t)s[NQ_ROUNDS]; stats->tile_visits = (int64_t)s[NQ_VISITS];
    }
    return SSF_OK;
}
}  // extern "C"
