// ssf_rows.hpp -- what ssf_track_fuse.hip (the per-frame chain), ssf_upkeep.hip (between frames) and ssf_p2p.hip (between ranks)
// share, all __device__ __forceinline__ (the library is built without relocatable device code): a row's fields and a row in
// registers, the migrant record, the tile owner, "performed" atomics and the arrival ticket, the ICP record's peer exchange.
#pragma once
#include "ssf_slots.hpp"

namespace ssf {

__device__ __forceinline__ V3 ld3(const float* __restrict__ p, size_t i) { return v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }
__device__ __forceinline__ void st3(float* __restrict__ p, size_t i, V3 v) { p[3 * i] = v.x; p[3 * i + 1] = v.y; p[3 * i + 2] = v.z; }
__device__ __forceinline__ Sym3 ld6(const float* __restrict__ p, size_t i) {
    return sym3(p[6 * i], p[6 * i + 1], p[6 * i + 2], p[6 * i + 3], p[6 * i + 4], p[6 * i + 5]);
}
__device__ __forceinline__ void st6(float* __restrict__ p, size_t i, Sym3 c) {
    p[6 * i] = c.xx; p[6 * i + 1] = c.xy; p[6 * i + 2] = c.xz; p[6 * i + 3] = c.yy; p[6 * i + 4] = c.yz; p[6 * i + 5] = c.zz;
}
// spatial-tile owner of a world position (multi-GPU sharding)
__device__ __forceinline__ int tile_owner(const V3& pw, int nranks, float tile) {
    const int ix = (int)floorf(pw.x / tile), iy = (int)floorf(pw.y / tile), iz = (int)floorf(pw.z / tile);
    const uint32_t h = ((uint32_t)ix * 73856093u) ^ ((uint32_t)iy * 19349663u) ^ ((uint32_t)iz * 83492791u);
    return (int)(h % (uint32_t)nranks);
}
// What a workgroup hands to the LAST workgroup of its launch (the one that sums up and publishes) must have been PERFORMED at
// the coherence point before the workgroup counts its arrival.  For an atomic without return value the wait counter
// (s_waitcnt vmcnt(0)) only says that the request has been accepted: with several handles hammering the fabric side by
// side (tools/p2p_first_frame_stress.py: four ranks of a sharded map on one GPU) the last workgroup was seen reading a
// replica record / a partition total BEFORE another workgroup's add had landed -- one frame in a few hundred came out a
// workgroup's worth short.  The value a RETURNING atomic brings back is the proof that it has been performed; these
// helpers are used for everything the last workgroup of the same launch reads.  (What the NEXT launch reads needs
// nothing: a kernel boundary completes everything.)
template <typename T> __device__ __forceinline__ void atomic_add_done(T* p, T v) {
    const T before = atomicAdd(p, v);
    asm volatile("" :: "v"(before));
}
__device__ __forceinline__ void atomic_store_done(int* p, int v) {
    const int before = __hip_atomic_exchange(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("" :: "v"(before));
}
// Is this the last workgroup of the launch to arrive?  (The middle of an accumulating kernel's three closing steps: icp_fold,
// this, icp_publish -- ssf_track_fuse.hip.)
// two-level arrival count over all workgroups of the grid (a single counter serialises thousands of same-address
// atomics at L2): 64 group counters, the last workgroup of a group reports to the global counter.  Thread 0 only.
#ifndef ARRIVE_GROUPS
#define ARRIVE_GROUPS 64u
#endif
// SSF_ARRIVE_FENCED (an experiment build, tools/build_variant.sh fenced -DSSF_ARRIVE_FENCED): real
// agent-scope release / acquire ordering around the arrival ticket -- one fence per workgroup, not per atomic -- to tell
// whether the first-frame divergence seen with UNCACHED exchange regions (round 2) was the relaxed arrival protocol's.
#if defined(SSF_EXPERIMENTS) && defined(SSF_ARRIVE_FENCED)
#define SSF_ARRIVE_RELEASE() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); } while (0)
#define SSF_ARRIVE_ACQUIRE() __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent")
#else
#define SSF_ARRIVE_RELEASE() do { } while (0)
#define SSF_ARRIVE_ACQUIRE() do { } while (0)
#endif
__device__ __forceinline__ int grid_arrive(unsigned int* ticket) {
    SSF_ARRIVE_RELEASE();
    const unsigned int g = blockIdx.x & (ARRIVE_GROUPS - 1u);
    const unsigned int in_group = (gridDim.x - g + ARRIVE_GROUPS - 1u) / ARRIVE_GROUPS, groups = min(gridDim.x, ARRIVE_GROUPS);
    int last = 0;
    const unsigned int tk = __hip_atomic_fetch_add(&ticket[1 + g], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tk == in_group - 1) {
        __hip_atomic_store(&ticket[1 + g], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned int tg = __hip_atomic_fetch_add(&ticket[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tg == groups - 1) { last = 1; __hip_atomic_store(&ticket[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    }
    if (last) SSF_ARRIVE_ACQUIRE();
    return last;
}
// one model row in registers: all loads are issued before the first store (source and destination arrays may alias as
// far as the compiler knows, so a field-by-field copy is a chain of dependent round trips)
struct RowRegs { V3 pos, col, lab, r0, r1, r2; Sym3 shape; int s0, s1; float d0, d1, conf; };
__device__ __forceinline__ RowRegs load_row(const SurfelSoA& A, size_t i) {
    RowRegs r;
    r.pos = ld3(A.pos, i); r.col = ld3(A.col, i); r.lab = ld3(A.lab, i);
    r.s0 = A.stamps[2 * i]; r.s1 = A.stamps[2 * i + 1];
    r.r0 = ld3(A.r0, i); r.r1 = ld3(A.r1, i); r.r2 = ld3(A.r2, i);
    r.shape = ld6(A.shape, i);
    r.d0 = A.dims[2 * i]; r.d1 = A.dims[2 * i + 1];
    r.conf = A.conf[i];
    return r;
}
__device__ __forceinline__ void store_row(const SurfelSoA& B, size_t j, const RowRegs& r) {
    st3(B.pos, j, r.pos); st3(B.col, j, r.col); st3(B.lab, j, r.lab);
    B.stamps[2 * j] = r.s0; B.stamps[2 * j + 1] = r.s1;
    st3(B.r0, j, r.r0); st3(B.r1, j, r.r1); st3(B.r2, j, r.r2);
    st6(B.shape, j, r.shape);
    B.dims[2 * j] = r.d0; B.dims[2 * j + 1] = r.d1;
    B.conf[j] = r.conf;
}
__device__ __forceinline__ void copy_row(const SurfelSoA& A, size_t i, const SurfelSoA& B, size_t j) { store_row(B, j, load_row(A, i)); }
// The migrant record (SSF_MIGRANT_WORDS int32 words, ssf.h): word 0 = owner + 1 (0: an empty slot), word 1 = the row sat in the
// visible block (re-homing only) -- both the caller's --, then the row's 26 words in this order.  The Lab cache does not
// travel: it is rebuilt from the colour.
__device__ __forceinline__ void migrant_pack(const RowRegs& r, int32_t* w) {
    const float v[26] = {r.pos.x, r.pos.y, r.pos.z, r.col.x, r.col.y, r.col.z, __int_as_float(r.s0), __int_as_float(r.s1),
                         r.r0.x, r.r0.y, r.r0.z, r.r1.x, r.r1.y, r.r1.z, r.r2.x, r.r2.y, r.r2.z,
                         r.shape.xx, r.shape.xy, r.shape.xz, r.shape.yy, r.shape.yz, r.shape.zz, r.d0, r.d1, r.conf};
#pragma unroll
    for (int i = 0; i < 26; i++) w[2 + i] = __float_as_int(v[i]);
}
__device__ __forceinline__ void migrant_unpack(const int32_t* w, RowRegs& row) {
    float v[26];
#pragma unroll
    for (int i = 0; i < 26; i++) v[i] = __int_as_float(w[2 + i]);
    row.pos = v3(v[0], v[1], v[2]); row.col = v3(v[3], v[4], v[5]); row.lab = rgb_to_lab(row.col);
    row.s0 = __float_as_int(v[6]); row.s1 = __float_as_int(v[7]);
    row.r0 = v3(v[8], v[9], v[10]); row.r1 = v3(v[11], v[12], v[13]); row.r2 = v3(v[14], v[15], v[16]);
    row.shape = sym3(v[17], v[18], v[19], v[20], v[21], v[22]); row.d0 = v[23]; row.d1 = v[24]; row.conf = v[25];
}
// ---- peer-to-peer exchange helpers (ssf_device.hpp: P2PView) ----------------------------------------------------------
__device__ __forceinline__ unsigned char* p2p_peer(const P2PView& pv, int r) {       // uniform select chain (no dynamic kernarg indexing)
    unsigned char* v = pv.peer[0];
#pragma unroll
    for (int i = 1; i < SSF_P2P_MAX_RANKS; i++) v = (r == i) ? pv.peer[i] : v;
    return v;
}
__device__ __forceinline__ unsigned long long shfl_u64(unsigned long long v, int src) {
    const unsigned int lo = (unsigned int)__shfl((int)(unsigned int)v, src), hi = (unsigned int)__shfl((int)(unsigned int)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}
// A peer that never arrives must not hang the device: every wait for a peer is bounded by WALL-CLOCK time (the constant-rate
// counter behind wall_clock64(), P2PView::timeout_ticks = ssf_p2p_configure's timeout), not by a spin count -- ranks in
// separate processes reach their first exchange seconds apart (set_model of a large map, graph captures, a cold box).
struct P2PDeadline {
    unsigned long long t0, ticks; unsigned int spins;
    __device__ __forceinline__ explicit P2PDeadline(const P2PView& pv) : t0(wall_clock64()), ticks(pv.timeout_ticks), spins(0u) {}
    // call once per unsuccessful poll; true = give up
    __device__ __forceinline__ bool expired() {
        __builtin_amdgcn_s_sleep(1);
        if ((++spins & 1023u) != 0u) return false;
        return wall_clock64() - t0 > ticks;
    }
};
// Wave 0 of the last workgroup: this rank's record (tot in lanes 0..28) goes into slot [parity][me] of every peer's region
// as five self-validating lines (the format of Mailbox::icp_rec); the records of the others are awaited in this rank's
// own region and added in rank order.  Returns false when a peer's record never arrived.
__device__ __forceinline__ bool p2p_icp_exchange(const P2PView& pv, unsigned long long seq, long long& tot, unsigned long long* pay /* LDS, 30 */) {
    const int l = lane();
    const int par = (int)(seq & 1ull);
    // (the record's encode and decode are icp_record_store's and icp_record_read's, ssf_mailbox.hpp, written out: one encode
    // for all peers, and a wave-wide decode)
    if (l < 29) pay[l] = (unsigned long long)tot;
    const unsigned long long check = (unsigned long long)wsum64(l < 29 ? tot : 0ll) + seq;
    if (l == 0) pay[29] = check;
    __builtin_amdgcn_s_waitcnt(0xc07f);       // lgkmcnt(0): one wave, its LDS writes have landed
    const unsigned long long word = l < 40 ? SSF_ICP_REC_WORD(l, pay, seq) : 0ull;
#pragma unroll
    for (int r = 0; r < SSF_P2P_MAX_RANKS; r++) {
        if (r >= pv.nranks || r == pv.me) continue;
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(pv.peer[r] + p2p_off_icp(par, pv.me));
        if (l < 40) __hip_atomic_store(&dst[l], word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    unsigned char* mine = p2p_peer(pv, pv.me);
    const bool is_seq_word = l < 40 && (l & 7) == 7, is_payload = l < 40 && (l & 7) != 7 && (7 * (l >> 3) + (l & 7)) < 29;
    P2PDeadline deadline(pv);
    for (int r = 0; r < pv.nranks; r++) {
        if (r == pv.me) continue;
        const unsigned long long* src = reinterpret_cast<const unsigned long long*>(mine + p2p_off_icp(par, r));
        for (;;) {
            const unsigned long long w = l < 40 ? __hip_atomic_load(&src[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0ull;
            const bool lines_ok = __ballot(is_seq_word && w != seq) == 0ull;
            const unsigned long long sum = (unsigned long long)wsum64(is_payload ? (long long)w : 0ll) + seq;
            if (lines_ok && sum == shfl_u64(w, SSF_ICP_REC_AT(29))) {                         // (the check word)
                const unsigned long long v = shfl_u64(w, l < 29 ? SSF_ICP_REC_AT(l) : 0);       // payload word l of the peer
                if (l < 29) tot += (long long)v;
                break;
            }
            if (deadline.expired()) return false;
        }
    }
    return true;
}

}  // namespace ssf
