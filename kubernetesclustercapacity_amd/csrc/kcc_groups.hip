// kcc_groups.hip — what the cell fits share around their pair loop (kcc_fit_grouped,
// kcc_fit_ext with group ids, kcc_fit_capped): the group sort's
// counting half and the finalize.
//
// Launches (none waits for another workgroup):
//   grp_hist     rows per group (LDS-summed per workgroup, then one device atomic per bin)
//   grp_scan     one workgroup: exclusive scan of the G counts -> the groups' cursors
//   grp_finalize one thread per cell: err = cnt > 0, totals = err ? 0 : acc
// Between scan and finalize run kcc_ext.hip's ext_scatter<R> (the row records in group
// order) and ext_pairs<R> (the pair loop), or kcc_spread.hip's cap_pairs<R> and its own
// finalize.  The grouped fit is their R = 0 instance; it has no kernel of its own.
#include "kcc_internal.h"

namespace kcc {
namespace {

// count[g] += rows of group g.  lds != 0 (G <= GRP_LDS_GROUPS): summed in LDS first.
__global__ __launch_bounds__(GRP_SORT_THREADS) void grp_hist_kernel(
    int64_t n, int64_t G, const int32_t* __restrict__ group, uint32_t* __restrict__ count,
    int lds) {
  __shared__ uint32_t h[GRP_LDS_GROUPS];
  const int64_t i = (int64_t)blockIdx.x * GRP_SORT_THREADS + threadIdx.x;
  const int32_t g = i < n ? group[i] : -1;
  const bool ok = grp_valid(g, G);
  if (!lds) {
    if (ok) atomicAdd(&count[g], 1u);
    return;
  }
  for (int k = threadIdx.x; k < (int)G; k += GRP_SORT_THREADS) h[k] = 0;
  __syncthreads();
  if (ok) atomicAdd(&h[g], 1u);
  __syncthreads();
  for (int k = threadIdx.x; k < (int)G; k += GRP_SORT_THREADS) {
    const uint32_t c = h[k];
    if (c) atomicAdd(&count[k], c);
  }
}

// cursor[g] = rows of the groups before g; *total = the rows of all groups.
__global__ __launch_bounds__(1024) void grp_scan_kernel(int64_t G, const uint32_t* __restrict__ count,
                                                       uint32_t* __restrict__ cursor,
                                                       uint32_t* __restrict__ total) {
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t carry;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < G; base += 1024) {
    const int64_t k = base + tid;
    const uint32_t v = k < G ? count[k] : 0u;
    uint32_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(inc, d, 64);
      if (lane >= d) inc += up;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t off = carry;
    for (int j = 0; j < w; ++j) off += wsum[j];
    if (k < G) cursor[k] = off + inc - v;
    __syncthreads();
    if (tid == 1023) carry = off + inc;
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

__global__ __launch_bounds__(256) void grp_finalize_kernel(int64_t cells, const int64_t* __restrict__ acc,
                                                          const unsigned long long* __restrict__ cnt,
                                                          int64_t* __restrict__ totals,
                                                          int32_t* __restrict__ spec_err) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= cells) return;
  const bool err = cnt[k] != 0;
  totals[k] = err ? 0 : acc[k];
  spec_err[k] = err ? SPEC_ERR_DIV0 : 0;
}

}  // namespace

hipError_t launch_grp_count_scan(int64_t n, int64_t G, const int32_t* group, const GrpWork& w,
                                 hipStream_t s) {
  const int64_t sort_grid = (n + GRP_SORT_THREADS - 1) / GRP_SORT_THREADS;
  const int lds = G <= GRP_LDS_GROUPS ? 1 : 0;
  hipError_t e;
  if ((e = hipMemsetAsync(w.count, 0, 4 * (size_t)G, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(grp_hist_kernel, dim3((unsigned)sort_grid), dim3(GRP_SORT_THREADS), 0, s, n, G,
                     group, w.count, lds);
  hipLaunchKernelGGL(grp_scan_kernel, dim3(1), dim3(1024), 0, s, G, w.count, w.cursor, w.total);
  return hipGetLastError();
}

hipError_t launch_grp_finalize(int64_t cells, const int64_t* acc, const unsigned long long* cnt,
                               int64_t* totals, int32_t* spec_err, hipStream_t s) {
  const int64_t fin_grid = (cells + 255) / 256;
  hipLaunchKernelGGL(grp_finalize_kernel, dim3((unsigned)fin_grid), dim3(256), 0, s, cells, acc,
                     cnt, totals, spec_err);
  return hipGetLastError();
}

}  // namespace kcc
