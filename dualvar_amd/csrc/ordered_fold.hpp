// The ticketed hand-off of the ordered reductions: workgroups pass rows of partial sums to the one that arrives last, which adds
// them in a fixed order -- no float atomics, so the sums do not depend on the order workgroups finish in.  Users: the
// BatchNorm-backward reduces (streaming.hpp: ordered_fold), the same reduce inside the LDS-staged data gradient's epilogue
// (conv_tap.hip: dv_conv3d_dgrad_bn_ws) and the ordered K-split of dv_infonce_fwd (loss.hip: gemm_f32_splitk_kernel).
// Device side only, apart from the ticket / row layout arithmetic below, which the host wrappers size their workspaces with.
#pragma once
#include "common.hpp"

// Rows and tickets travel as agent-scope relaxed atomics (stores / loads with sc1: coherent across the XCDs' L2s on their own),
// ordered by a plain s_waitcnt -- NOT by agent-scope fences: a release fence is a write-back of the whole L2 (buffer_wbl2) and
// an acquire fence an invalidate, from every one of the thousands of blocks of a launch; measured, they took the reduce
// launches of the S3D-G step from 1.4 to 4.0 - 7.9 ms.
// The protocol, spelled out: (1) EVERY store of a handed-off row is an sc1 (write-through, agent-coherent) store; (2) every
// storing wave drains them with s_waitcnt vmcnt(0), then the workgroup's barrier; (3) ONE lane takes the ticket with an
// agent-scope atomic add; (4) only the workgroup whose add returned the last ticket reads, after a barrier its ticket lane
// joins, and EVERY load of the rows is an sc1 load to registers (never cached in the reading CU's L1).  This is the
// "sc1 stores + drained counter + sc1 loads" hand-off measured valid on gfx950 (MI355X_MICROARCH.md, inter-workgroup
// visibility, valid forms); it is NOT a HIP memory-model guarantee and relies on stores retiring under vmcnt on this part.
// Hence the guard: every file that includes this header refuses to build for any other target (the library's host side
// refuses to run elsewhere too: dv_check_device).  A port would replace coherent_store / stores_done / coherent_load by plain
// accesses between __builtin_amdgcn_fence(__ATOMIC_RELEASE / __ATOMIC_ACQUIRE, "agent") -- here, and nowhere else.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "the ordered fold's sc1 / s_waitcnt hand-off is validated on gfx950 only (see the comment above)"
#endif
__device__ __forceinline__ void coherent_store(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float coherent_load(const float* p) {
  return __hip_atomic_load(const_cast<float*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void stores_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Clauses (2) - (4) for a whole workgroup: its rows are drained, thread 0 takes one of the `n` tickets of *ticket, and every
// thread learns whether this workgroup took the last one (and so reads).  `flag` is a word of LDS the caller lends.
__device__ __forceinline__ bool took_last_ticket(uint32_t* ticket, uint32_t n, uint32_t* flag) {
  stores_done();                                     // this workgroup's rows have reached the coherence point ...
  __syncthreads();
  if (threadIdx.x == 0) *flag = (atomicAdd(ticket, 1u) == n - 1) ? 1u : 0u;      // ... before its ticket is taken
  __syncthreads();
  return *flag != 0;
}
// the reader leaves the ticket word zero for the next launch (the host re-zeroes after a failed launch: dualvar_amd/_lib.py,
// register_ticket_workspace)
__device__ __forceinline__ void clear_ticket(uint32_t* ticket) {
  if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Sum of word `src` of n rows `pitch` floats apart, in row order.  All the loads of a batch are in flight together (one trip to
// the coherence point per BATCH rows, not per row); a short batch re-reads its last row and adds 0.f for it -- exact, a running
// fp32 sum that starts at +0 is never -0 under round-to-nearest -- so the order of the additions is the row order.
template <int BATCH>
__device__ __forceinline__ float fold_in_order(const float* src, int n, size_t pitch) {
  float t = 0.f;
  for (int b = 0; b < n; b += BATCH) {
    float v[BATCH];
#pragma unroll
    for (int u = 0; u < BATCH; ++u) v[u] = coherent_load(src + (size_t)min(b + u, n - 1) * pitch);
#pragma unroll
    for (int u = 0; u < BATCH; ++u) t += (b + u < n) ? v[u] : 0.f;
  }
  return t;
}

// Two-level folds (no workgroup walks hundreds of rows): the n rows of an item go in groups of kFoldGroup, each group's last
// arriver adds its rows into a group row, the last of those adds the group rows.  Per item: n rows + fold_groups(n) group
// rows, and one ticket per group + one for the groups, rounded up to 8 words.
constexpr int kFoldGroup = 32;
__host__ __device__ __forceinline__ int fold_groups(int n) { return (n + kFoldGroup - 1) / kFoldGroup; }
__host__ __device__ __forceinline__ int fold_ticket_words(int n) { return (fold_groups(n) + 1 + 7) & ~7; }
__host__ __device__ __forceinline__ int64_t fold_rows_total(int n) { return (int64_t)n + fold_groups(n); }
