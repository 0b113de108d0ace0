// ssf_slots.hip -- the kernels that the read-outs of the model share (ssf_slots.hpp says who launches them, and what keeps
// a scan of its own): the out-of-view blocks' live counts and the one-workgroup exclusive scan of 32-bit counts, in two widths.
#include "ssf_slots.hpp"

namespace ssf {

// bc[b] = the live rows of out-of-view block b (256 slots)
__global__ __launch_bounds__(256) void k_slots_oov_count(ModelView mv, uint32_t* __restrict__ bc) {
    __shared__ int part[4];
    size_t phys;
    const int k = block_count256(span_live(mv.oov.live, mv.oov_head, mv.oov_tail, blockIdx.x * 256u + threadIdx.x, phys), part);
    if (threadIdx.x == 0) bc[blockIdx.x] = k;
}

// Acc = the width of the running sums; the stored offsets are their low 32 bits either way
template <typename Acc>
__device__ __forceinline__ void scan_counts(uint32_t* __restrict__ a, int n, uint32_t* __restrict__ cursor, unsigned long long* __restrict__ total) {
    __shared__ Acc tot[1];
    workgroup_scan<1, Acc>(a, n, cursor, tot);
    if (threadIdx.x == 0) { a[n] = (uint32_t)tot[0]; if (total) *total = tot[0]; }
}
__global__ __launch_bounds__(1024) void k_slots_scan(uint32_t* __restrict__ a, int n, uint32_t* __restrict__ cursor,
                                                     unsigned long long* __restrict__ total) {
    scan_counts<unsigned long long>(a, n, cursor, total);
}
// 32-bit sums, no copy, no total: for the graph's sort, whose scan of 256 counts per 2048 slots runs over a hundred rounds per
// pass and whose total is a slot count.  Through k_slots_scan graph_rank took 542 us at 1 M rows (64-bit sums) or 454 us (32-bit
// sums, the nullable arguments tested every round) against this kernel's 447: profiles/readout_scaffold_refactor.txt
__global__ __launch_bounds__(1024) void k_slots_scan32(uint32_t* __restrict__ a, int n) { scan_counts<uint32_t>(a, n, nullptr, nullptr); }

void launch_slots_scan(hipStream_t st, uint32_t* a, int n, uint32_t* cursor, unsigned long long* total) {
    hipLaunchKernelGGL(k_slots_scan, dim3(1), dim3(1024), 0, st, a, n, cursor, total);
}
void launch_slots_scan32(hipStream_t st, uint32_t* a, int n) { hipLaunchKernelGGL(k_slots_scan32, dim3(1), dim3(1024), 0, st, a, n); }
void launch_slots_oov_offsets(hipStream_t st, const ModelView& mv, uint32_t* bc) {
    if (mv.nbo == 0) return;
    hipLaunchKernelGGL(k_slots_oov_count, dim3(mv.nbo), dim3(256), 0, st, mv, bc);
    launch_slots_scan(st, bc, mv.nbo, nullptr, nullptr);
}

}  // namespace ssf
