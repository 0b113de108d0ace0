// What does a global integer atomic cost on MI355X by SCOPE, for the association's pattern (k_match: N rows, each one
// 64-bit atomicMin onto one of S hot words chosen by a gather) and for a histogram (N 32-bit adds onto S words)?
//   agent scope   (HIP's atomicMin / atomicAdd) and workgroup scope (__hip_atomic_fetch_* with __HIP_MEMORY_SCOPE_WORKGROUP) of a
//                 relaxed no-return RMW compile to the SAME instruction on gfx950 (`global_atomic_umin_x2 v[2:3], v[0:1], off`,
//                 no sc bits: read off the -S output in round 4 and again with the product's shape below) and time the same.
//                 The scope is not what the replica tables gain from.
//   replica tables: one table per XCD -- selected by the hardware's XCC_ID, or by blockIdx & 7, which times the same -- put an
//                 eighth of the bids on every word: same-word collisions are what bounds the pattern.  A kernel boundary, then
//                 a merge (MIN / SUM over 8), in a launch of its own or in the reader's trip (k_read).
// Also: reading the word first (agent-scope load) and skipping an atomic that cannot win.
// `atomic_scope shape` runs the product's shape alone (product_shape: one row per lane, every workgroup bidding at once, one table
// against eight, the table stride, the reader's side): profiles/assoc_replicas.txt.
// Checks every variant against the host's result (an atomicity failure among the CUs of an XCD would show as a wrong
// minimum / a short count), then times them.
//   hipcc --offload-arch=gfx950 -O2 tools/probe/atomic_scope.hip -o /tmp/atomic_scope && /tmp/atomic_scope
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>

#define NO_MATCH 0x7fffffffffffffffull
__device__ __forceinline__ unsigned int xcc_id() { return __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 7u; }   // HW_REG_XCC_ID[3:0]

__global__ void k_min_agent(const uint32_t* tgt, const uint32_t* dist, int n, unsigned long long* best) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    atomicMin(&best[tgt[i]], ((unsigned long long)dist[i] << 32) | (uint32_t)i);
}
__global__ void k_min_agent_filter(const uint32_t* tgt, const uint32_t* dist, int n, unsigned long long* best) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = ((unsigned long long)dist[i] << 32) | (uint32_t)i;
    if (__hip_atomic_load(&best[tgt[i]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(&best[tgt[i]], key);
}
template <bool FILTER>
__global__ void k_min_xcd(const uint32_t* tgt, const uint32_t* dist, int n, unsigned long long* rep, int S) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned long long* mine = rep + (size_t)xcc_id() * S;
    const unsigned long long key = ((unsigned long long)dist[i] << 32) | (uint32_t)i;
    // (the filter's load must not come from the CU's L1, which no other CU's atomic refreshes: sc1 = served by the L2)
    if (FILTER && !(__hip_atomic_load(&mine[tgt[i]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key)) return;
    (void)__hip_atomic_fetch_min(&mine[tgt[i]], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__global__ void k_merge_min(const unsigned long long* rep, unsigned long long* best, int S) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= S) return;
    unsigned long long v = rep[f];
#pragma unroll
    for (int x = 1; x < 8; x++) v = min(v, rep[(size_t)x * S + f]);
    best[f] = v;
}
__global__ void k_fill(unsigned long long* p, unsigned long long v, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
__global__ void k_add_agent(const uint32_t* tgt, int n, uint32_t* cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) atomicAdd(&cnt[tgt[i]], 1u);
}
__global__ void k_add_xcd(const uint32_t* tgt, int n, uint32_t* rep, int S) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) (void)__hip_atomic_fetch_add(&rep[(size_t)xcc_id() * S + tgt[i]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__global__ void k_census(uint32_t* per_xcc) { if (threadIdx.x == 0) atomicAdd(&per_xcc[xcc_id()], 1u); }
// the rows' own loads alone (what every variant pays before its atomic)
__global__ void k_loads_only(const uint32_t* tgt, const uint32_t* dist, int n, unsigned long long* sink) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (tgt[i] == 0xffffffffu && dist[i] == 7u) sink[0] = 1;
}

// ---- the product's shape (k_icp_resident's association): one row per lane, ceil(N / 256) workgroups bidding at the same moment,
// about two thirds of the rows bid (tgt < 0: no bid).  NT tables `stride` words apart: table 0 alone (NT = 1), or tables 1..8
// chosen by XCC_ID (BY_XCC) or by blockIdx & 7; AGENT: HIP's atomicMin, else a workgroup-scope RMW.
template <int NT, bool BY_XCC, bool AGENT>
__global__ void k_bid(const int32_t* tgt, const uint32_t* dist, int n, unsigned long long* tab, int stride) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (NT > 1) tab += (size_t)(1u + (BY_XCC ? xcc_id() : (blockIdx.x & 7u))) * stride;
    if (i >= n) return;
    const int f = tgt[i];
    if (f < 0) return;
    const unsigned long long key = ((unsigned long long)dist[i] << 32) | (uint32_t)i;
    if (AGENT) atomicMin(&tab[f], key);
    else (void)__hip_atomic_fetch_min(&tab[f], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// the reader's side (the visible-row classification of the fuse launch): every bidding row looks up the winner of its word --
// table 0 alone, or the minimum over table 0 and the eight replicas, nine loads in one trip
template <int NT>
__global__ void k_read(const int32_t* tgt, int n, const unsigned long long* tab, int stride, uint32_t* won) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int f = tgt[i];
    if (f < 0) return;
    unsigned long long v = tab[f];
    if (NT > 1) {
        unsigned long long r[8];
#pragma unroll
        for (int x = 0; x < 8; x++) r[x] = tab[(size_t)(1 + x) * stride + f];
#pragma unroll
        for (int x = 0; x < 8; x++) v = min(v, r[x]);
    }
    if ((uint32_t)v == (uint32_t)i) won[i] = 1u;
}

template <typename F> static double time_us(F f, int reps) {
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    for (int i = 0; i < 3; i++) f();
    hipDeviceSynchronize();
    hipEventRecord(a, 0);
    for (int i = 0; i < reps; i++) f();
    hipEventRecord(b, 0); hipEventSynchronize(b);
    float ms = 0; hipEventElapsedTime(&ms, a, b);
    return ms * 1000.0 / reps;
}

// The product's shape: N rows in ceil(N / 256) workgroups, one launch; one table against eight; what the readers then pay.
static int product_shape() {
    const int NMAX = 940000, SMAX = 4800;
    uint32_t st = 777u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return st >> 8; };
    int32_t* d_tgt; uint32_t *d_dist, *d_won; unsigned long long* d_tab;
    const int STRIDE_MAX = SMAX + 16;
    hipMalloc(&d_tgt, NMAX * 4); hipMalloc(&d_dist, NMAX * 4); hipMalloc(&d_won, NMAX * 4); hipMalloc(&d_tab, 9 * STRIDE_MAX * 8);
    const dim3 blk(256);
    int bad = 0;
    printf("product shape: one row per lane, 2 of 3 rows bid, random targets; us per launch (table filled before every launch; fill alone shown)\n");
    for (int S : {1200, 4800}) for (int N : {30000, 123000, 940000}) {
        std::vector<int32_t> tgt(N); std::vector<uint32_t> dist(N);
        for (int i = 0; i < N; i++) { tgt[i] = rnd() % 3 ? (int32_t)(rnd() % S) : -1; dist[i] = 0x3c000000u + (rnd() & 0xfffff); }
        std::vector<unsigned long long> want(S, NO_MATCH);
        for (int i = 0; i < N; i++) if (tgt[i] >= 0) want[tgt[i]] = std::min(want[tgt[i]], ((unsigned long long)dist[i] << 32) | (uint32_t)i);
        hipMemcpy(d_tgt, tgt.data(), N * 4, hipMemcpyHostToDevice); hipMemcpy(d_dist, dist.data(), N * 4, hipMemcpyHostToDevice);
        const dim3 grid((N + 255) / 256);
        // strides: S itself (1200 and 4800 words are whole 128-byte lines already), and S + 8 words, which puts every other
        // table's start in the middle of a line: the last line of one XCD's table is then the first of the next one's
        const int line = (S + 15) & ~15, split = S + 8;
        auto fill = [&](int words) { hipLaunchKernelGGL(k_fill, dim3((words + 255) / 256), blk, 0, 0, d_tab, NO_MATCH, words); };
        std::vector<unsigned long long> got(9 * STRIDE_MAX);
        auto check = [&](const char* what, int stride) {
            hipMemcpy(got.data(), d_tab, (size_t)9 * stride * 8, hipMemcpyDeviceToHost);
            int wrong = 0;
            for (int f = 0; f < S; f++) { unsigned long long v = got[f]; for (int x = 1; x < 9; x++) v = std::min(v, got[(size_t)x * stride + f]); wrong += v != want[f]; }
            if (wrong) { printf("  !! %s: %d of %d minima wrong\n", what, wrong, S); bad++; }
        };
#define BID(NT, BX, AG, stride) hipLaunchKernelGGL((k_bid<NT, BX, AG>), grid, blk, 0, 0, d_tgt, d_dist, N, d_tab, stride)
        for (int r = 0; r < 3; r++) {
            fill(9 * line); BID(1, false, true, line); check("one table", line);
            fill(9 * line); BID(8, true, true, line); check("eight by XCC_ID, agent", line);
            fill(9 * line); BID(8, false, true, line); check("eight by blockIdx & 7, agent", line);
            fill(9 * line); BID(8, true, false, line); check("eight by XCC_ID, workgroup scope", line);
            fill(9 * split); BID(8, true, true, split); check("eight by XCC_ID, lines shared", split);
        }
        const int reps = 50;
        printf("S=%d N=%d (%d workgroups)\n", S, N, (int)grid.x);
        printf("  fill one table / nine tables alone        %7.2f / %7.2f us\n", time_us([&] { fill(S); }, reps), time_us([&] { fill(9 * line); }, reps));
        printf("  fill 1 + loads only                       %7.2f us\n", time_us([&] { fill(S); hipLaunchKernelGGL(k_loads_only, grid, blk, 0, 0, (const uint32_t*)d_tgt, d_dist, N, d_tab + 9 * STRIDE_MAX - 1); }, reps));
        printf("  fill 1 + one table, agent scope           %7.2f us\n", time_us([&] { fill(S); BID(1, false, true, line); }, reps));
        printf("  fill 9 + eight by XCC_ID, agent scope     %7.2f us\n", time_us([&] { fill(9 * line); BID(8, true, true, line); }, reps));
        printf("  fill 9 + eight by blockIdx & 7, agent     %7.2f us\n", time_us([&] { fill(9 * line); BID(8, false, true, line); }, reps));
        printf("  fill 9 + eight by XCC_ID, workgroup scope %7.2f us\n", time_us([&] { fill(9 * line); BID(8, true, false, line); }, reps));
        printf("  fill 9 + eight by XCC_ID, stride S + 8    %7.2f us\n", time_us([&] { fill(9 * split); BID(8, true, true, split); }, reps));
        // the readers: the tables as the bids left them (replicas at the line stride), every bidding row looks its word up
        fill(9 * line); BID(8, true, true, line);
        printf("  reader, table 0 alone                     %7.2f us\n", time_us([&] { hipLaunchKernelGGL(k_read<1>, grid, blk, 0, 0, d_tgt, N, d_tab, line, d_won); }, reps));
        printf("  reader, minimum over nine tables          %7.2f us\n", time_us([&] { hipLaunchKernelGGL(k_read<8>, grid, blk, 0, 0, d_tgt, N, d_tab, line, d_won); }, reps));
#undef BID
    }
    hipFree(d_tgt); hipFree(d_dist); hipFree(d_won); hipFree(d_tab);
    return bad;
}

int main(int argc, char** argv) {
    if (argc > 1 && argv[1][0] == 's') {            // `atomic_scope shape`: the product's shape alone
        const int b = product_shape();
        printf(b ? "FAILED: %d wrong results\n" : "all variants exact (%d)\n", b);
        return b ? 1 : 0;
    }
    const int N = 1000000;
    uint32_t st = 12345u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return st >> 8; };
    uint32_t *d_tgt, *d_dist, *d_cnt, *d_cnt_rep, *d_census; unsigned long long *d_best, *d_rep;
    hipMalloc(&d_tgt, N * 4); hipMalloc(&d_dist, N * 4);
    hipMalloc(&d_best, 8192 * 8); hipMalloc(&d_rep, 8 * 8192 * 8); hipMalloc(&d_cnt, 8192 * 4); hipMalloc(&d_cnt_rep, 8 * 8192 * 4);
    hipMalloc(&d_census, 32); hipMemset(d_census, 0, 32);
    hipLaunchKernelGGL(k_census, dim3(4096), dim3(256), 0, 0, d_census);
    uint32_t census[8]; hipMemcpy(census, d_census, 32, hipMemcpyDeviceToHost);
    printf("workgroups per XCC_ID of a 4096-block launch:");
    for (int x = 0; x < 8; x++) printf(" %u", census[x]);
    printf("\n");
    const dim3 grid((N + 255) / 256), blk(256);
    int bad = 0;
    for (int S : {1200, 4800}) {
        for (int sorted = 0; sorted < 2; sorted++) {
            std::vector<uint32_t> tgt(N), dist(N);
            for (int i = 0; i < N; i++) { tgt[i] = rnd() % S; dist[i] = 0x3c000000u + (rnd() & 0xfffff); }
            if (sorted) std::sort(tgt.begin(), tgt.end());          // rows in image order: neighbours bid for the same word
            std::vector<unsigned long long> want(S, NO_MATCH); std::vector<uint32_t> wcnt(S, 0);
            for (int i = 0; i < N; i++) { want[tgt[i]] = std::min(want[tgt[i]], ((unsigned long long)dist[i] << 32) | (uint32_t)i); wcnt[tgt[i]]++; }
            hipMemcpy(d_tgt, tgt.data(), N * 4, hipMemcpyHostToDevice); hipMemcpy(d_dist, dist.data(), N * 4, hipMemcpyHostToDevice);
            std::vector<unsigned long long> got(S); std::vector<uint32_t> gcnt(S), grep(8 * S);
            auto check = [&](const char* what) {
                hipMemcpy(got.data(), d_best, S * 8, hipMemcpyDeviceToHost);
                int wrong = 0;
                for (int f = 0; f < S; f++) wrong += got[f] != want[f];
                if (wrong) { printf("  !! %s: %d of %d minima wrong\n", what, wrong, S); bad++; }
            };
            auto fill_best = [&] { hipLaunchKernelGGL(k_fill, dim3((S + 255) / 256), blk, 0, 0, d_best, NO_MATCH, S); };
            auto fill_rep = [&] { hipLaunchKernelGGL(k_fill, dim3((8 * S + 255) / 256), blk, 0, 0, d_rep, NO_MATCH, 8 * S); };
            auto merge = [&] { hipLaunchKernelGGL(k_merge_min, dim3((S + 255) / 256), blk, 0, 0, d_rep, d_best, S); };
            // correctness of every variant, 5 runs each
            for (int r = 0; r < 5; r++) {
                fill_best(); hipLaunchKernelGGL(k_min_agent, grid, blk, 0, 0, d_tgt, d_dist, N, d_best); check("agent");
                fill_best(); hipLaunchKernelGGL(k_min_agent_filter, grid, blk, 0, 0, d_tgt, d_dist, N, d_best); check("agent+filter");
                fill_rep(); hipLaunchKernelGGL(k_min_xcd<false>, grid, blk, 0, 0, d_tgt, d_dist, N, d_rep, S); merge(); check("xcd");
                fill_rep(); hipLaunchKernelGGL(k_min_xcd<true>, grid, blk, 0, 0, d_tgt, d_dist, N, d_rep, S); merge(); check("xcd+filter");
                hipMemset(d_cnt, 0, S * 4); hipLaunchKernelGGL(k_add_agent, grid, blk, 0, 0, d_tgt, N, d_cnt);
                hipMemcpy(gcnt.data(), d_cnt, S * 4, hipMemcpyDeviceToHost);
                int wrong = 0; for (int f = 0; f < S; f++) wrong += gcnt[f] != wcnt[f];
                if (wrong) { printf("  !! add agent: %d counts wrong\n", wrong); bad++; }
                hipMemset(d_cnt_rep, 0, 8 * S * 4); hipLaunchKernelGGL(k_add_xcd, grid, blk, 0, 0, d_tgt, N, d_cnt_rep, S);
                hipMemcpy(grep.data(), d_cnt_rep, 8 * S * 4, hipMemcpyDeviceToHost);
                wrong = 0; for (int f = 0; f < S; f++) { uint32_t t = 0; for (int x = 0; x < 8; x++) t += grep[(size_t)x * S + f]; wrong += t != wcnt[f]; }
                if (wrong) { printf("  !! add xcd: %d counts wrong (an add lost between CUs of one XCD)\n", wrong); bad++; }
            }
            const int reps = 20;
            printf("S=%d rows=%d %s\n", S, N, sorted ? "SORTED by target" : "random targets");
            printf("  loads only                               %7.2f us\n", time_us([&] { hipLaunchKernelGGL(k_loads_only, grid, blk, 0, 0, d_tgt, d_dist, N, d_best); }, reps));
            printf("  atomicMin u64 agent scope                %7.2f us\n", time_us([&] { hipLaunchKernelGGL(k_min_agent, grid, blk, 0, 0, d_tgt, d_dist, N, d_best); }, reps));
            printf("  (fill + that)                            %7.2f us\n", time_us([&] { fill_best(); hipLaunchKernelGGL(k_min_agent, grid, blk, 0, 0, d_tgt, d_dist, N, d_best); }, reps));
            printf("  fill + read first, agent atomic if less  %7.2f us\n", time_us([&] { fill_best(); hipLaunchKernelGGL(k_min_agent_filter, grid, blk, 0, 0, d_tgt, d_dist, N, d_best); }, reps));
            printf("  fill + per-XCD replicas (L2) + merge     %7.2f us\n", time_us([&] { fill_rep(); hipLaunchKernelGGL(k_min_xcd<false>, grid, blk, 0, 0, d_tgt, d_dist, N, d_rep, S); merge(); }, reps));
            printf("  fill + per-XCD replicas, read first      %7.2f us\n", time_us([&] { fill_rep(); hipLaunchKernelGGL(k_min_xcd<true>, grid, blk, 0, 0, d_tgt, d_dist, N, d_rep, S); merge(); }, reps));
            printf("  per-XCD replicas kernel alone (no fill)  %7.2f us\n", time_us([&] { hipLaunchKernelGGL(k_min_xcd<false>, grid, blk, 0, 0, d_tgt, d_dist, N, d_rep, S); }, reps));
            printf("  atomicAdd u32 agent scope                %7.2f us\n", time_us([&] { hipLaunchKernelGGL(k_add_agent, grid, blk, 0, 0, d_tgt, N, d_cnt); }, reps));
            printf("  atomicAdd u32 per-XCD replicas (L2)      %7.2f us\n", time_us([&] { hipLaunchKernelGGL(k_add_xcd, grid, blk, 0, 0, d_tgt, N, d_cnt_rep, S); }, reps));
        }
    }
    printf(bad ? "FAILED: %d wrong results\n" : "all variants exact (%d)\n", bad);
    return bad ? 1 : 0;
}
