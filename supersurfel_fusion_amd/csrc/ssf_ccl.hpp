// ssf_ccl.hpp -- connected components of a raster by a lock-free union-find: the device pieces shared by the motion masks
// (ssf_motion.hip) and the frontier regions (ssf_navfrontier.hip).  Device code only: no kernel, no host function, no symbol.
//
// The scheme: four phases in separate launches (no workgroup ever waits for another), and the marks each leaves for a cell p:
//   * label    one 256-thread workgroup per CCL_TILE x CCL_TILE tile, CCL_PER_THREAD cells per thread: a union-find in LDS over the
//              tile's links (ccl_tile_label).  A tile's row-major order is the image's restricted to it, so a local root is the
//              smallest image index of its local component.  It leaves (ccl_tile_store) parent[p] = the image index of p's local
//              root for a member, CCL_NONE for any other cell; label[p] = p at a local root, CCL_MEMBER at any other member,
//              CCL_NONE elsewhere;
//   * merge    one thread per cell on the high side of a tile border (ccl_border_threads of them) unites across the border on the
//              global parent array (ccl_merge over ccl_border_pairs).  Only local roots' words are rewritten; a member's word is
//              >= 0 for good and any other cell's CCL_NONE for good, so the membership test needs no care about the unions going on;
//   * roots    parent read-only: every local root (ccl_is_local_root) walks to its root (ccl_walk) and stores it as its label;
//   * flatten  parent read-only: every other member takes its local root's label (ccl_flatten): label[p] = the component's root
//              for every member, CCL_NONE elsewhere.
//
// The invariant of every loop here: parent[i] <= i, and atomicMin is the only write to a parent word, so a parent only ever
// decreases.  A walk i -> parent[i] therefore visits strictly decreasing indices >= 0 and ends at an i with parent[i] == i, whatever
// other threads do.  A unite applies atomicMin only to a node that a walk ended at, with the other walk's end as its value; when the
// node had meanwhile been hung elsewhere the atomic returns that older parent and the thread goes on uniting IT with the other
// side, so no link is ever lost; max(a, b) strictly decreases from one round to the next, so it ends.  In the merge every read of a
// parent is an agent-scope load (other workgroups, on any XCD, lower parents in the same launch); a stale read only names an older
// ancestor, and the decision is taken on the value the atomic returns.  Nothing is compressed while others unite: re-pointing a
// node then can cut a set.  Links go from the larger root to the smaller, so a set's root is its smallest index: labels do not
// depend on scheduling.
#pragma once
#include "ssf_slots.hpp"

namespace ssf {

constexpr int CCL_TILE = 32, CCL_CELLS = CCL_TILE * CCL_TILE, CCL_PER_THREAD = CCL_CELLS / 256;
constexpr int32_t CCL_NONE = -1, CCL_MEMBER = -2;

// ---- the primitives: in LDS (label) and in global memory (merge, roots) -------------------------------------------------------------
__device__ __forceinline__ int ccl_lds_find(const volatile int* sp, int i) {
    for (int g; (g = sp[i]) != i;) i = g;
    return i;
}
__device__ __forceinline__ void ccl_lds_unite(int* sp, int a, int b) {
    for (;;) {
        a = ccl_lds_find(sp, a); b = ccl_lds_find(sp, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&sp[a], b);
        if (old == a) return;                         // a was a root and now hangs under b < a
        a = old;                                      // another thread hung a under old < a first: now unite old and b
    }
}
__device__ __forceinline__ int ccl_load(const int32_t* q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ccl_find(const int32_t* parent, int i) {
    for (int g; (g = ccl_load(&parent[i])) != i;) i = g;
    return i;
}
__device__ __forceinline__ void ccl_unite(int32_t* parent, int a, int b) {
    for (;;) {
        a = ccl_find(parent, a); b = ccl_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;
    }
}
// the walk of a launch in which nobody writes parent: plain loads
__device__ __forceinline__ int ccl_walk(const int32_t* __restrict__ parent, int i) {
    for (int g; (g = parent[i]) != i;) i = g;
    return i;
}

// ---- label: the tile body ---------------------------------------------------------------------------------------------------------------
// the image index of local cell i of the tile whose first cell is (x0, y0), in an image W wide
__device__ __forceinline__ int32_t ccl_image_index(int W, int x0, int y0, int i) {
    return (int32_t)((size_t)(y0 + i / CCL_TILE) * W + (x0 + i % CCL_TILE));
}
// ALL 256 threads call it (it holds barriers).  sp: CCL_CELLS words of LDS.  member(i): local cell i is a member (false outside the
// image); linked(i, j): the members i and j, neighbours, link; diag: the two upper diagonals count as neighbours.  Whatever LDS
// member and linked read was written by the caller before the call: the first barrier orders it.  root[k] = the local root of cell
// k * 256 + threadIdx.x, -1 for a cell that is no member.
template <class Member, class Linked>
__device__ __forceinline__ void ccl_tile_label(int* sp, bool diag, Member member, Linked linked, int (&root)[CCL_PER_THREAD]) {
#pragma unroll
    for (int k = 0; k < CCL_PER_THREAD; k++) sp[k * 256 + threadIdx.x] = k * 256 + threadIdx.x;
    __syncthreads();
    auto link = [&](int i, int j) { if (member(j) && linked(i, j)) ccl_lds_unite(sp, i, j); };
#pragma unroll
    for (int k = 0; k < CCL_PER_THREAD; k++) {
        const int i = k * 256 + threadIdx.x, lx = i % CCL_TILE;
        if (!member(i)) continue;
        if (lx > 0) link(i, i - 1);
        if (i >= CCL_TILE) {
            link(i, i - CCL_TILE);
            if (diag && lx > 0) link(i, i - CCL_TILE - 1);
            if (diag && lx + 1 < CCL_TILE) link(i, i - CCL_TILE + 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CCL_PER_THREAD; k++) {
        const int i = k * 256 + threadIdx.x;
        root[k] = member(i) ? ccl_lds_find(sp, i) : -1;                // (no writer any more)
    }
}
// the marks "after label" for the tile's cells inside the W x H image
__device__ __forceinline__ void ccl_tile_store(int W, int H, int x0, int y0, const int (&root)[CCL_PER_THREAD], int32_t* __restrict__ parent,
                                               int32_t* __restrict__ label) {
#pragma unroll
    for (int k = 0; k < CCL_PER_THREAD; k++) {
        const int i = k * 256 + threadIdx.x, r = root[k];
        if (x0 + i % CCL_TILE >= W || y0 + i / CCL_TILE >= H) continue;
        const int32_t p = ccl_image_index(W, x0, y0, i);
        parent[p] = r < 0 ? CCL_NONE : ccl_image_index(W, x0, y0, r);
        label[p] = r < 0 ? CCL_NONE : (r == i ? p : CCL_MEMBER);
    }
}

// ---- merge: one thread per cell on the high side of a tile border -------------------------------------------------------------------------
// threads [0, nv): (x = bx * CCL_TILE, y), bx = 1 .. ntx - 1, with (x - 1, y) and, diag, (x - 1, y - 1) and (x - 1, y + 1);
// threads [nv, nv + nh): (x, y = by * CCL_TILE), by = 1 .. nty - 1, with (x, y - 1) and, diag, (x - 1, y - 1) and (x + 1, y - 1):
// the diagonal pairs along the edge, which at a tile corner are the corner's diagonal pairs.  A diagonal pair across a tile corner
// is met from both lists; uniting twice is harmless.
constexpr long long ccl_border_threads(int W, int H, int ntx, int nty) { return (long long)(ntx - 1) * H + (long long)(nty - 1) * W; }
// f(p, q) for each pair of thread t < ccl_border_threads: p is the thread's cell, the same in every call, q faces it across the border
template <class F>
__device__ __forceinline__ void ccl_border_pairs(int W, int H, int ntx, long long t, bool diag, F f) {
    const long long nv = ccl_border_threads(W, H, ntx, 1);             // (one row of tiles: the vertical borders alone)
    if (t < nv) {
        const int x = (int)(t / H + 1) * CCL_TILE, y = (int)(t % H), p = y * W + x;
        f(p, p - 1);
        if (diag && y > 0) f(p, p - W - 1);
        if (diag && y + 1 < H) f(p, p + W - 1);
    } else {
        t -= nv;
        const int y = (int)(t / W + 1) * CCL_TILE, x = (int)(t % W), p = y * W + x;
        f(p, p - W);
        if (diag && x > 0) f(p, p - W - 1);
        if (diag && x + 1 < W) f(p, p - W + 1);
    }
}
// thread t unites each of its pairs whose two cells are members and for which linked(p, q) holds; the number of such pairs
template <class Linked>
__device__ __forceinline__ int ccl_merge(int32_t* parent, int W, int H, int ntx, long long t, bool diag, Linked linked) {
    int n = 0, pm = -1;                                                // pm: is p a member?  Read at the first pair
    ccl_border_pairs(W, H, ntx, t, diag, [&](int p, int q) {
        if (pm < 0) pm = ccl_load(&parent[p]) >= 0;
        if (pm && ccl_load(&parent[q]) >= 0 && linked(p, q)) { ccl_unite(parent, p, q); n++; }
    });
    return n;
}

// ---- roots and flatten --------------------------------------------------------------------------------------------------------------------
// before the roots launch has walked from p
__device__ __forceinline__ bool ccl_is_local_root(const int32_t* __restrict__ label, size_t p) { return label[p] >= 0; }
// flatten, l = label[p]: label[parent[p]] is a local root's word, written by the roots launch and by nobody in this one; parent[p]
// is p's local root still (the merge never rewrites the word of a cell that is no local root)
__device__ __forceinline__ void ccl_flatten(const int32_t* parent, int32_t* label, size_t p, int32_t l) {
    if (l == CCL_MEMBER) label[p] = label[parent[p]];
}

}  // namespace ssf
