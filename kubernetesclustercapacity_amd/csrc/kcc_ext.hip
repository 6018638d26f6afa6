// kcc_ext.hip — the cell fit: per node-group x spec totals, with extended resources
// (kcc_fit_grouped, kcc_fit_ext).
//
// totals[g][s] is what the reference's node loop (CC:105-140) gives for spec s on exactly
// the rows of group g, with Go's 64-bit semantics (uint64 CPU division reinterpreted as int,
// truncating int64 memory division with MinInt64 / -1 == MinInt64, signed findMin, the
// pod-slot clamp allocatablePods - len(pods)), and a per-cell flag where Go would panic.
// Besides CPU and memory a row carries R <= EXT_MAX extra int64 resources (device-plugin
// GPUs, ephemeral storage, hugepages: Quantity.Value() of allocatable and of the summed
// requests) and a spec requests x_r of each.  An extra resource is a second memory column
// (CC:125-130: free = alloc <= used ? 0 : alloc - used, wrapping; Go's truncating int64
// division, MinInt64 / -1 == MinInt64; signed findMin) except that a zero request means
// "not requested": no constraint, no panic.  The pod-slot clamp (CC:134-136) follows all
// the mins.  With R = 0 and no group ids this is kcc_fit bit for bit; kcc_fit_grouped is
// R = 0 with group ids, on these kernels.
//
// Launches (none waits for another workgroup):
//   without group ids   ext_rows<R>     one thread per row: the record (free CPU / memory, P,
//                                       clamp, R ExtCol, fast class) in row order
//   with group ids      grp_hist, grp_scan (kcc_groups.hip), then
//                       ext_scatter<R>  one thread per row: the record placed in group order
//                                       (a workgroup reserves each group's slots with one
//                                       atomic on its cursor)
//   ext_pairs<R>        a wave holds 64 specs in its lanes and walks GRP_RUN group-ordered
//                       records (staged in LDS, read as broadcasts); each lane keeps an int64
//                       sum and a divide-by-zero count and the wave flushes them with 64-bit
//                       atomic adds to acc[g][s] / cnt[g][s] on a group change and at the end
//                       of the run (the body is ext_pairs_body<R, false> in kcc_internal.h,
//                       shared with kcc_spread.hip's cap_pairs<R>; its cap and minimum code
//                       does not exist here)
//   grp_finalize        (kcc_groups.hip)
// The order of the rows inside a group is whatever the cursors gave: the sums wrap, so the
// results do not depend on it.  R is a template parameter: x[r] and the record's columns
// are indexed statically, no kernel has a private segment.  LDS of ext_pairs<0>: 256 x
// (48 + 4) B = 13 KiB; of ext_pairs<4>: 256 x (48 + 4 + 4 x 16) B = 29 KiB.
//
// Arithmetic.  The exact path is kcc_rows.hip's, per pair.  The fast path (wave-uniform)
// serves a fast row (fc < 2^31, 0 <= fm < 2^50, every 0 <= fx_r < 2^50) under a wave whose
// 64 specs are all fast (c, m in [1, 2^52], every x_r 0 or in [1, 2^52]): per resource
// grp_div's t = trunc(f * (1/d)) in f64 is within 1 of the quotient, and the remainder
// r = fma(-t, d, f) — exact — says which way (DESIGN.md §4.9 has the proof; the bounds
// are the same per resource).  No rounding mode is changed.  A lane with x_r == 0 divides by
// 1.0 (finite: 1.0 / 0 would be +inf and 0 * inf a NaN) and its quotient is selected away
// before the one conversion; min(...) <= qc <= fc < 2^31 keeps the (int32) conversion in
// range.
#include "kcc_internal.h"

namespace kcc {
namespace {

// The record of row i at slot pos (group g): GrpRow, R ExtCol, and the fast bit over all
// 2 + R free amounts.
template <int R>
__device__ inline void ext_record(int64_t i, int64_t pos, int32_t g, int64_t n,
                                  const uint64_t* __restrict__ alloc_cpu,
                                  const int64_t* __restrict__ alloc_mem,
                                  const int64_t* __restrict__ alloc_pods,
                                  const int64_t* __restrict__ pod_count,
                                  const uint64_t* __restrict__ used_cpu,
                                  const int64_t* __restrict__ used_mem,
                                  const int64_t* __restrict__ alloc_x,
                                  const int64_t* __restrict__ used_x, GrpRow* __restrict__ rec,
                                  ExtCol* __restrict__ xrec, int32_t* __restrict__ rg) {
  const uint64_t ac = alloc_cpu[i], uc = used_cpu[i];
  const int64_t am = alloc_mem[i], um = used_mem[i];
  const int64_t P = alloc_pods[i];
  GrpRow r;
  r.fc = ac > uc ? ac - uc : 0;                                    // CC:119 (uint64 compare)
  r.fm = am > um ? (int64_t)((uint64_t)am - (uint64_t)um) : 0;     // CC:125 (the difference wraps)
  r.P = P;
  r.cl = (int64_t)((uint64_t)P - (uint64_t)pod_count[i]);          // CC:135
  bool fast = r.fc < GRP_FC_MAX && (uint64_t)r.fm < GRP_FM_MAX;
  int64_t fx[R ? R : 1];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int64_t ax = alloc_x[(int64_t)k * n + i], ux = used_x[(int64_t)k * n + i];
    fx[k] = ax > ux ? (int64_t)((uint64_t)ax - (uint64_t)ux) : 0;  // as the memory column
    fast = fast && (uint64_t)fx[k] < GRP_FM_MAX;
  }
  r.fcd = fast ? (double)r.fc : 0.0;
  r.fmd = fast ? (double)r.fm : 0.0;
  rec[pos] = r;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    ExtCol x;
    x.fx = fx[k];
    x.fxd = fast ? (double)fx[k] : 0.0;
    xrec[pos * R + k] = x;
  }
  rg[pos] = g | (fast ? GRP_ROW_FAST : 0);
}

// No group ids: record i is row i, all in group 0.
template <int R>
__global__ __launch_bounds__(256) void ext_rows_kernel(
    int64_t n, const uint64_t* __restrict__ alloc_cpu, const int64_t* __restrict__ alloc_mem,
    const int64_t* __restrict__ alloc_pods, const int64_t* __restrict__ pod_count,
    const uint64_t* __restrict__ used_cpu, const int64_t* __restrict__ used_mem,
    const int64_t* __restrict__ alloc_x, const int64_t* __restrict__ used_x,
    GrpRow* __restrict__ rec, ExtCol* __restrict__ xrec, int32_t* __restrict__ rg) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  ext_record<R>(i, i, 0, n, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
                alloc_x, used_x, rec, xrec, rg);
}

// One thread per row: the record at the next slot of its group (cursor[] starts at the
// exclusive scan of the groups' counts).  lds != 0 (G <= GRP_LDS_GROUPS): a workgroup ranks
// its rows in LDS and reserves each group's slots with one atomic.
template <int R>
__global__ __launch_bounds__(GRP_SORT_THREADS) void ext_scatter_kernel(
    int64_t n, int64_t G, const int32_t* __restrict__ group,
    const uint64_t* __restrict__ alloc_cpu, const int64_t* __restrict__ alloc_mem,
    const int64_t* __restrict__ alloc_pods, const int64_t* __restrict__ pod_count,
    const uint64_t* __restrict__ used_cpu, const int64_t* __restrict__ used_mem,
    const int64_t* __restrict__ alloc_x, const int64_t* __restrict__ used_x,
    uint32_t* __restrict__ cursor, GrpRow* __restrict__ rec, ExtCol* __restrict__ xrec,
    int32_t* __restrict__ rg, int lds) {
  __shared__ uint32_t h[GRP_LDS_GROUPS];
  const int64_t i = (int64_t)blockIdx.x * GRP_SORT_THREADS + threadIdx.x;
  const int32_t g = i < n ? group[i] : -1;
  const bool ok = grp_valid(g, G);
  uint32_t pos = 0;
  if (lds) {
    for (int k = threadIdx.x; k < (int)G; k += GRP_SORT_THREADS) h[k] = 0;
    __syncthreads();
    uint32_t rank = 0;
    if (ok) rank = atomicAdd(&h[g], 1u);
    __syncthreads();
    for (int k = threadIdx.x; k < (int)G; k += GRP_SORT_THREADS) {
      const uint32_t c = h[k];
      if (c) h[k] = atomicAdd(&cursor[k], c);
    }
    __syncthreads();
    if (ok) pos = h[g] + rank;
  } else if (ok) {
    pos = atomicAdd(&cursor[g], 1u);
  }
  if (!ok || (int64_t)pos >= n) return;
  ext_record<R>(i, (int64_t)pos, g, n, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu,
                used_mem, alloc_x, used_x, rec, xrec, rg);
}

// total == nullptr: the n_rec records of the ungrouped pass; else *total (the rows with a
// valid group id, from grp_scan).
template <int R>
__global__ __launch_bounds__(GRP_PAIR_THREADS) void ext_pairs_kernel(
    const uint32_t* __restrict__ total, int64_t n_rec, int64_t S, int64_t sblocks,
    const uint64_t* __restrict__ spec_cpu, const int64_t* __restrict__ spec_mem,
    const int64_t* __restrict__ spec_x, const GrpRow* __restrict__ rec,
    const ExtCol* __restrict__ xrec, const int32_t* __restrict__ rg, int64_t* __restrict__ acc,
    unsigned long long* __restrict__ cnt) {
  ext_pairs_body<R, false>(total, n_rec, S, sblocks, spec_cpu, spec_mem, spec_x, rec, xrec, rg,
                           acc, cnt, nullptr, nullptr);
}

// The launches ahead of the pair loop: acc / cnt zeroed, then the records.
template <int R>
hipError_t launch_records(const FitNodes& nd, int64_t S, const ExtWork& w, hipStream_t s) {
  hipError_t e;
  if ((e = hipMemsetAsync(w.g.acc, 0, 16 * (size_t)(nd.G * S), s)) != hipSuccess) return e;
  if (nd.group) {
    const int64_t sort_grid = (nd.n + GRP_SORT_THREADS - 1) / GRP_SORT_THREADS;
    const int lds = nd.G <= GRP_LDS_GROUPS ? 1 : 0;
    if ((e = launch_grp_count_scan(nd.n, nd.G, nd.group, w.g, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(ext_scatter_kernel<R>, dim3((unsigned)sort_grid), dim3(GRP_SORT_THREADS), 0,
                       s, nd.n, nd.G, nd.group, nd.alloc_cpu, nd.alloc_mem, nd.alloc_pods,
                       nd.pod_count, nd.used_cpu, nd.used_mem, nd.alloc_x, nd.used_x, w.g.cursor,
                       w.g.rec, w.xrec, w.g.rg, lds);
  } else {
    hipLaunchKernelGGL(ext_rows_kernel<R>, dim3((unsigned)((nd.n + 255) / 256)), dim3(256), 0, s,
                       nd.n, nd.alloc_cpu, nd.alloc_mem, nd.alloc_pods, nd.pod_count, nd.used_cpu,
                       nd.used_mem, nd.alloc_x, nd.used_x, w.g.rec, w.xrec, w.g.rg);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_ext_records(const FitNodes& nd, int64_t S, const ExtWork& w, hipStream_t s) {
  if (!ext_sizes_ok(nd, S)) return hipErrorInvalidValue;
  return ext_dispatch(nd.R, [&](auto r) { return launch_records<decltype(r)::value>(nd, S, w, s); });
}

hipError_t launch_fit_ext(const FitNodes& nd, const FitSpecs& sp, const ExtWork& w,
                          int64_t* totals, int32_t* spec_err, hipStream_t s) {
  hipError_t e;
  if ((e = launch_ext_records(nd, sp.S, w, s)) != hipSuccess) return e;
  e = ext_dispatch(nd.R, [&](auto r) {
    return launch_pairs(ext_pairs_kernel<decltype(r)::value>, nd, sp, w, s);
  });
  if (e != hipSuccess) return e;
  const int64_t cells = nd.G * sp.S;
  return launch_grp_finalize(cells, w.g.acc, w.g.cnt(cells), totals, spec_err, s);
}

}  // namespace kcc

