// ssf_p2p.hip -- between the ranks of a sharded map, outside the ICP launches: the peer-to-peer exchanges of the fuse stage
// (shard sizes, association tables, migrant table: P2PView, ssf_device.hpp) and the RCCL path's rank-reduced records on their
// way to the mailbox.  (The ICP record's own exchange runs inside the frame's launches: p2p_icp_exchange, ssf_rows.hpp.)
#include "ssf_rows.hpp"

namespace ssf {

// a 29-value device record (e.g. the rank-reduced ICP system) -> mailbox, as the ICP kernel's tail does
__global__ void k_publish_icp(const long long* __restrict__ rec, Mailbox* mb, unsigned long long seq) {
    __shared__ unsigned long long pay[30];
    icp_record_store(mb->icp_rec, threadIdx.x < 29 ? rec[threadIdx.x] : 0ll, seq, pay, threadIdx.x);       // (one wave: launch_publish_icp)
}
__global__ void k_publish_all_counts(const int* __restrict__ all5, int n, Mailbox* mb, unsigned long long seq) {
    int_record_store(mb->all_cnt, all5, n, &mb->all_check, &mb->all_seq, seq, (int)threadIdx.x);           // (one wave: launch_publish_all_counts)
}

// ---- peer-to-peer exchanges of the fuse stage (ssf_device.hpp: P2PView) ----------------------------------------------------
// shard sizes: one self-validating line per rank (Counters::last, checksum, sequence number) -> every peer; the lines of
// all ranks -> the host mailbox (as k_publish_all_counts).  One wave.
__global__ void k_p2p_counts(P2PView pv, const Counters* __restrict__ cnt, Mailbox* mb, unsigned long long all_seq) {
    const int l = lane();
    const unsigned long long seq = pv.seq;
    const int par = (int)(seq & 1ull);
    const unsigned int a = (unsigned int)cnt->last[0], b = (unsigned int)cnt->last[1], c = (unsigned int)cnt->last[2],
                       d = (unsigned int)cnt->last[3], e = (unsigned int)cnt->last[4];
    const unsigned long long w0 = a | ((unsigned long long)b << 32), w1 = c | ((unsigned long long)d << 32), w2 = e;
    const unsigned long long mine_word = l == 0 ? w0 : l == 1 ? w1 : l == 2 ? w2 : l == 6 ? w0 + w1 + w2 + seq : l == 7 ? seq : 0ull;
#pragma unroll
    for (int r = 0; r < SSF_P2P_MAX_RANKS; r++) {
        if (r >= pv.nranks || r == pv.me) continue;
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(pv.peer[r] + p2p_off_cnt(par, pv.me));
        if (l < 8) __hip_atomic_store(&dst[l], mine_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    unsigned char* mine = p2p_peer(pv, pv.me);
    unsigned long long part = 0;
    P2PDeadline deadline(pv);
    for (int r = 0; r < pv.nranks; r++) {
        unsigned long long w = mine_word;
        if (r != pv.me) {
            const unsigned long long* src = reinterpret_cast<const unsigned long long*>(mine + p2p_off_cnt(par, r));
            for (;;) {
                w = l < 8 ? __hip_atomic_load(&src[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0ull;
                const unsigned long long sum = (unsigned long long)wsum64(l < 3 ? (long long)w : 0ll) + seq;
                if (shfl_u64(w, 7) == seq && shfl_u64(w, 6) == sum) break;
                if (deadline.expired()) return;
            }
        }
        if (l < 3) {
            const int lo = (int)(unsigned int)w, hi = (int)(unsigned int)(w >> 32);
            __hip_atomic_store(&mb->all_cnt[5 * r + 2 * l], lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            part += (unsigned long long)(unsigned int)lo;
            if (l < 2) { __hip_atomic_store(&mb->all_cnt[5 * r + 2 * l + 1], hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); part += (unsigned long long)(unsigned int)hi; }
        }
    }
    int_record_close(part, &mb->all_check, &mb->all_seq, all_seq, l == 0);
}
// thread 0: every peer's flag line of `kind` carries pv.seq (its data stores were acknowledged before the flag left)
__device__ __forceinline__ bool p2p_wait_flags(const P2PView& pv, int kind) {
    unsigned char* mine = p2p_peer(pv, pv.me);
    const int par = (int)(pv.seq & 1ull);
    P2PDeadline deadline(pv);
    for (int r = 0; r < pv.nranks; r++) {
        if (r == pv.me) continue;
        const unsigned long long* f = reinterpret_cast<const unsigned long long*>(mine + p2p_off_flag(kind, par, r));
        while (__hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != pv.seq)
            if (deadline.expired()) return false;
    }
    return true;
}
__device__ __forceinline__ void p2p_raise_flags(const P2PView& pv, int kind) {       // threads 0..nranks-1, after a barrier
    const int par = (int)(pv.seq & 1ull);
    const int r = threadIdx.x;
    if (r < pv.nranks && r != pv.me)
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(p2p_peer(pv, r) + p2p_off_flag(kind, par, pv.me)), pv.seq,
                           __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// association tables: this rank's best[] / matched[] -> every peer, then best := MIN, matched := OR over the ranks.
// One workgroup (S entries of 9 bytes).
__device__ __forceinline__ void p2p_assoc_exchange(const P2PView& pv, unsigned long long* __restrict__ best, uint8_t* __restrict__ matched, int* s_ok, Mailbox* mb) {
    const int par = (int)(pv.seq & 1ull), S = pv.S;
    // (own tables: device-scope atomic loads -- inside k_match they were written by other workgroups of this launch)
#pragma unroll
    for (int r = 0; r < SSF_P2P_MAX_RANKS; r++) {
        if (r >= pv.nranks || r == pv.me) continue;
        unsigned long long* db = reinterpret_cast<unsigned long long*>(pv.peer[r] + p2p_off_best(S, par, pv.me));
        uint8_t* dm = pv.peer[r] + p2p_off_matched(S, par, pv.me);
        // (returning exchanges, not stores: what comes back is the proof that the word has landed in the peer's memory
        // before this rank raises its flag -- see atomic_add_done)
        unsigned int* dm32 = reinterpret_cast<unsigned int*>(dm);
        const unsigned int* m32 = reinterpret_cast<const unsigned int*>(matched);
        unsigned long long sink = 0;
        for (int i = threadIdx.x; i < S; i += blockDim.x)
            sink ^= __hip_atomic_exchange(&db[i], __hip_atomic_load(&best[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        for (int i = threadIdx.x; i < (S + 3) / 4; i += blockDim.x)
            sink ^= __hip_atomic_exchange(&dm32[i], __hip_atomic_load(&m32[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        asm volatile("" :: "v"(sink));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    p2p_raise_flags(pv, P2P_FLAG_ASSOC);
    if (threadIdx.x == 0) {
        *s_ok = p2p_wait_flags(pv, P2P_FLAG_ASSOC) ? 1 : 0;
        if (!*s_ok) __hip_atomic_store(&mb->p2p_timeout, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __syncthreads();
    if (!*s_ok) return;
    unsigned char* mine = p2p_peer(pv, pv.me);
    for (int i = threadIdx.x; i < S; i += blockDim.x) {
        unsigned long long b = __hip_atomic_load(&best[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint8_t m = __hip_atomic_load(&matched[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int r = 0; r < pv.nranks; r++) {
            if (r == pv.me) continue;
            const unsigned long long* sb = reinterpret_cast<const unsigned long long*>(mine + p2p_off_best(S, par, r));
            const uint8_t* sm = mine + p2p_off_matched(S, par, r);
            const unsigned long long ob = __hip_atomic_load(&sb[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            const uint8_t om = __hip_atomic_load(&sm[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            b = ob < b ? ob : b; m = om > m ? om : m;
        }
        best[i] = b; matched[i] = m;
    }
}
__global__ __launch_bounds__(1024) void k_p2p_assoc(P2PView pv, unsigned long long* __restrict__ best, uint8_t* __restrict__ matched, Mailbox* mb) {
    __shared__ int s_ok;
    p2p_assoc_exchange(pv, best, matched, &s_ok, mb);
}
// migrant table: slot f of this rank's table -> slot f of [parity][me] in every peer (an empty slot sends its first two
// words only); the last workgroup to finish raises the flags.  One thread per slot.
__global__ __launch_bounds__(256) void k_p2p_migr_share(P2PView pv, const int32_t* __restrict__ table, unsigned int* ticket) {
    const int par = (int)(pv.seq & 1ull), S = pv.S;
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < S) {
        const unsigned long long* src = reinterpret_cast<const unsigned long long*>(table + (size_t)SSF_MIGRANT_WORDS * f);
        unsigned long long w[SSF_MIGRANT_WORDS / 2];
        w[0] = src[0];
        const bool full = (unsigned int)w[0] != 0u;
#pragma unroll
        for (int k = 1; k < SSF_MIGRANT_WORDS / 2; k++) w[k] = full ? src[k] : 0ull;
#pragma unroll
        for (int r = 0; r < SSF_P2P_MAX_RANKS; r++) {
            if (r >= pv.nranks || r == pv.me) continue;
            unsigned long long* dst = reinterpret_cast<unsigned long long*>(pv.peer[r] + p2p_off_migr(S, par, pv.me)) + (size_t)(SSF_MIGRANT_WORDS / 2) * f;
            unsigned long long sink = __hip_atomic_exchange(&dst[0], w[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);     // (returning: see p2p_assoc_exchange)
            if (full) {
#pragma unroll
                for (int k = 1; k < SSF_MIGRANT_WORDS / 2; k++) sink ^= __hip_atomic_exchange(&dst[k], w[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            asm volatile("" :: "v"(sink));
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __shared__ int s_last;
    if (threadIdx.x == 0) s_last = grid_arrive(ticket);
    __syncthreads();
    if (s_last) p2p_raise_flags(pv, P2P_FLAG_MIGR);
}
// ... and the peers' slots are added into this rank's table (at most one rank fills a slot: the sum is the union)
__global__ __launch_bounds__(256) void k_p2p_migr_gather(P2PView pv, int32_t* __restrict__ table, Mailbox* mb) {
    const int par = (int)(pv.seq & 1ull), S = pv.S;
    __shared__ int s_ok;
    if (threadIdx.x == 0) {
        s_ok = p2p_wait_flags(pv, P2P_FLAG_MIGR) ? 1 : 0;
        if (!s_ok) __hip_atomic_store(&mb->p2p_timeout, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __syncthreads();
    if (!s_ok) return;
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= S) return;
    unsigned char* mine = p2p_peer(pv, pv.me);
    int32_t* own = table + (size_t)SSF_MIGRANT_WORDS * f;
    for (int r = 0; r < pv.nranks; r++) {
        if (r == pv.me) continue;
        const unsigned long long* src = reinterpret_cast<const unsigned long long*>(mine + p2p_off_migr(S, par, r)) + (size_t)(SSF_MIGRANT_WORDS / 2) * f;
        const unsigned long long w0 = __hip_atomic_load(&src[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if ((unsigned int)w0 == 0u) continue;
        own[0] += (int32_t)(unsigned int)w0; own[1] += (int32_t)(unsigned int)(w0 >> 32);
#pragma unroll
        for (int k = 1; k < SSF_MIGRANT_WORDS / 2; k++) {
            const unsigned long long w = __hip_atomic_load(&src[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            own[2 * k] += (int32_t)(unsigned int)w; own[2 * k + 1] += (int32_t)(unsigned int)(w >> 32);
        }
    }
}

// ---- launchers -----------------------------------------------------------------------------------
void launch_p2p_counts(hipStream_t st, const P2PView& pv, const Counters* cnt, Mailbox* mb, unsigned long long all_seq) {
    ScopedKernel sk("p2p_counts", st);
    hipLaunchKernelGGL(k_p2p_counts, dim3(1), dim3(64), 0, st, pv, cnt, mb, all_seq);
}
void launch_p2p_assoc(hipStream_t st, const P2PView& pv, unsigned long long* best, uint8_t* matched, Mailbox* mb) {
    ScopedKernel sk("p2p_assoc", st);
    hipLaunchKernelGGL(k_p2p_assoc, dim3(1), dim3(1024), 0, st, pv, best, matched, mb);
}
void launch_p2p_migrants(hipStream_t st, const P2PView& pv, int32_t* table, unsigned int* ticket, Mailbox* mb) {
    ScopedKernel sk("p2p_migrants", st);
    const int grid = (pv.S + 255) / 256;
    hipLaunchKernelGGL(k_p2p_migr_share, dim3(grid), dim3(256), 0, st, pv, table, ticket);
    hipLaunchKernelGGL(k_p2p_migr_gather, dim3(grid), dim3(256), 0, st, pv, table, mb);
}
void launch_publish_icp(hipStream_t st, const long long* rec, Mailbox* mb, unsigned long long seq) {
    hipLaunchKernelGGL(k_publish_icp, dim3(1), dim3(64), 0, st, rec, mb, seq);
}
void launch_publish_all_counts(hipStream_t st, const int* all5, int nranks, Mailbox* mb, unsigned long long seq) {
    hipLaunchKernelGGL(k_publish_all_counts, dim3(1), dim3(64), 0, st, all5, 5 * nranks, mb, seq);
}

}  // namespace ssf
