// kcc_ext.hip — the fit with extended resources (kcc_fit_ext).
//
// Besides CPU and memory a row carries R <= EXT_MAX extra int64 resources (device-plugin
// GPUs, ephemeral storage, hugepages: Quantity.Value() of allocatable and of the summed
// requests) and a spec requests x_r of each.  An extra resource is a second memory column
// (CC:125-130: free = alloc <= used ? 0 : alloc - used, wrapping; Go's truncating int64
// division, MinInt64 / -1 == MinInt64; signed findMin) except that a zero request means
// "not requested": no constraint, no panic.  The pod-slot clamp (CC:134-136) follows all
// the mins.  With R = 0 this is kcc_fit / kcc_fit_grouped bit for bit.
//
// Launches (none waits for another workgroup):
//   without group ids   ext_rows<R>     one thread per row: the record in row order
//   with group ids      grp_hist, grp_scan (kcc_groups.hip), then
//                       ext_scatter<R>  grp_scatter with the record widened by R ExtCol
//   ext_pairs<R>        grp_pairs' plan: a wave holds 64 specs, walks GRP_RUN records staged
//                       in LDS (read as broadcasts), per-lane int64 sums, 64-bit atomic adds
//                       on a group change and at the end of the run
//   grp_finalize        (kcc_groups.hip)
// R is a template parameter: x[r] and the record's columns are indexed statically, no
// kernel has a private segment.  LDS of ext_pairs<4>: 256 x (48 + 4 + 4 x 16) B = 29 KiB.
//
// Fast path (wave-uniform, as in grp_pairs): a fast row (fc < 2^31, 0 <= fm < 2^50, every
// 0 <= fx_r < 2^50) under a wave whose 64 specs are all fast (c, m in [1, 2^52], every x_r
// 0 or in [1, 2^52]) takes grp_div per resource — the same bounds as §4.9, so its proof
// holds per resource.  A lane with x_r == 0 divides by 1.0 (finite: 1.0 / 0 would be +inf
// and 0 * inf a NaN) and its quotient is selected away before the one conversion;
// min(...) <= qc <= fc < 2^31 keeps the (int32) conversion in range.
#include "kcc_internal.h"

namespace kcc {
namespace {

// The record of row i at slot pos (group g): GrpRow as grp_scatter builds it, R ExtCol, and
// the fast bit over all 2 + R free amounts.
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

// grp_scatter_kernel with the widened record: one thread per row, the record at the next
// slot of its group (cursor[] starts at the exclusive scan of the groups' counts).
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
  constexpr int RR = R ? R : 1;
  __shared__ GrpRow s_rec[GRP_RUN];
  __shared__ ExtCol s_x[GRP_RUN * RR];
  __shared__ int32_t s_rg[GRP_RUN];
  const int64_t run = (int64_t)blockIdx.x / sblocks;
  const int64_t sb = (int64_t)blockIdx.x - run * sblocks;
  const int64_t M = total ? (int64_t)*total : n_rec;
  const int64_t base = run * GRP_RUN;
  if (base >= M) return;
  const int nr = (int)(M - base < GRP_RUN ? M - base : GRP_RUN);
  for (int j = threadIdx.x; j < nr; j += GRP_PAIR_THREADS) {
    s_rec[j] = rec[base + j];
    s_rg[j] = rg[base + j];
  }
  if constexpr (R > 0) {
    for (int j = threadIdx.x; j < nr * R; j += GRP_PAIR_THREADS) s_x[j] = xrec[base * R + j];
  }
  __syncthreads();

  const int64_t s = sb * GRP_PAIR_THREADS + threadIdx.x;
  const bool live = s < S;  // (a lane past S: c = m = 1, every x = 0 — a fast spec)
  const uint64_t c = live ? spec_cpu[s] : 1;
  const int64_t m = live ? spec_mem[s] : 1;
  bool spec_fast = c >= 1 && c <= GRP_SPEC_MAX && m >= 1 && (uint64_t)m <= GRP_SPEC_MAX;
  int64_t x[RR];
  double xd[RR], rx[RR];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    x[k] = live ? spec_x[(int64_t)k * S + s] : 0;
    spec_fast = spec_fast && (uint64_t)x[k] <= GRP_SPEC_MAX;  // 0 or [1, 2^52]
    xd[k] = x[k] == 0 ? 1.0 : (double)x[k];  // a finite divisor for the unrequested lane
    rx[k] = 1.0 / xd[k];                     // (used on the fast path only)
  }
  const bool wave_fast = __all(spec_fast);
  const double cd = (double)c, md = (double)m;
  const double rc = 1.0 / cd, rm = 1.0 / md;  // (used on the fast path only: c, m >= 1 there)

  int64_t sum = 0;
  unsigned long long z = 0;
  int gcur = __builtin_amdgcn_readfirstlane(s_rg[0]) & (GRP_ROW_FAST - 1);
  for (int j = 0; j < nr; ++j) {
    const int meta = __builtin_amdgcn_readfirstlane(s_rg[j]);
    const int g = meta & (GRP_ROW_FAST - 1);
    if (g != gcur) {  // wave-uniform
      grp_flush(acc, cnt, (int64_t)gcur * S + s, live, sum, z);
      sum = 0;
      z = 0;
      gcur = g;
    }
    const GrpRow r = s_rec[j];
    int64_t q;
    if (wave_fast && (meta & GRP_ROW_FAST)) {  // wave-uniform
      const double tc = grp_div(r.fcd, cd, rc);
      const double tm = grp_div(r.fmd, md, rm);
      double t = tc <= tm ? tc : tm;  // findMin (CC:133)
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const double tx = grp_div(s_x[j * RR + k].fxd, xd[k], rx[k]);
        t = (x[k] != 0 && tx < t) ? tx : t;  // the unrequested lane's quotient is never used
      }
      q = (int64_t)(int32_t)t;  // <= free CPU < 2^31
    } else {
      int64_t qc = 0, qm = 0;
      bool dz = false;
      if (r.fc != 0) {  // CC:119-124 (uint64 division, int() reinterprets)
        if (c == 0) dz = true;
        else qc = (int64_t)(r.fc / c);
      }
      if (r.fm != 0) {  // CC:125-130
        if (m == 0) dz = true;
        else if (m == -1) qm = (int64_t)(0ull - (uint64_t)r.fm);  // MinInt64 / -1 == MinInt64
        else qm = r.fm / m;
      }
      q = qc <= qm ? qc : qm;  // findMin, CC:133
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int64_t fx = s_x[j * RR + k].fx;
        if (x[k] != 0) {  // zero: not requested
          int64_t qx = 0;
          if (fx != 0) qx = x[k] == -1 ? (int64_t)(0ull - (uint64_t)fx) : fx / x[k];
          q = q <= qx ? q : qx;
        }
      }
      z += dz ? 1u : 0u;
    }
    if (q >= r.P) q = r.cl;  // CC:134-136, after all the mins
    sum = (int64_t)((uint64_t)sum + (uint64_t)q);
  }
  grp_flush(acc, cnt, (int64_t)gcur * S + s, live, sum, z);
}

template <int R>
hipError_t launch_ext(int64_t n, const uint64_t* alloc_cpu, const int64_t* alloc_mem,
                      const int64_t* alloc_pods, const int64_t* pod_count,
                      const uint64_t* used_cpu, const int64_t* used_mem, const int64_t* alloc_x,
                      const int64_t* used_x, const int32_t* group, int64_t G, int64_t S,
                      const uint64_t* spec_cpu, const int64_t* spec_mem, const int64_t* spec_x,
                      const ExtWork& w, int64_t* totals, int32_t* spec_err, hipStream_t s) {
  const int64_t cells = G * S;
  const int64_t sblocks = (S + GRP_PAIR_THREADS - 1) / GRP_PAIR_THREADS;
  const int64_t pair_grid = grp_runs(n) * sblocks;
  hipError_t e;
  if ((e = hipMemsetAsync(w.g.acc, 0, 16 * (size_t)cells, s)) != hipSuccess) return e;
  int64_t* acc = w.g.acc;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(w.g.acc + cells);
  if (group) {
    const int64_t sort_grid = (n + GRP_SORT_THREADS - 1) / GRP_SORT_THREADS;
    const int lds = G <= GRP_LDS_GROUPS ? 1 : 0;
    if ((e = launch_grp_count_scan(n, G, group, w.g, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(ext_scatter_kernel<R>, dim3((unsigned)sort_grid), dim3(GRP_SORT_THREADS), 0,
                       s, n, G, group, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu,
                       used_mem, alloc_x, used_x, w.g.cursor, w.g.rec, w.xrec, w.g.rg, lds);
  } else {
    hipLaunchKernelGGL(ext_rows_kernel<R>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n,
                       alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem, alloc_x,
                       used_x, w.g.rec, w.xrec, w.g.rg);
  }
  hipLaunchKernelGGL(ext_pairs_kernel<R>, dim3((unsigned)pair_grid), dim3(GRP_PAIR_THREADS), 0, s,
                     group ? w.g.total : (const uint32_t*)nullptr, n, S, sblocks, spec_cpu,
                     spec_mem, spec_x, w.g.rec, w.xrec, w.g.rg, acc, cnt);
  if ((e = launch_grp_finalize(cells, acc, cnt, totals, spec_err, s)) != hipSuccess) return e;
  return hipGetLastError();
}

}  // namespace

hipError_t launch_fit_ext(int64_t n, const uint64_t* alloc_cpu, const int64_t* alloc_mem,
                          const int64_t* alloc_pods, const int64_t* pod_count,
                          const uint64_t* used_cpu, const int64_t* used_mem, int R,
                          const int64_t* alloc_x, const int64_t* used_x, const int32_t* group,
                          int64_t G, int64_t S, const uint64_t* spec_cpu, const int64_t* spec_mem,
                          const int64_t* spec_x, const ExtWork& w, int64_t* totals,
                          int32_t* spec_err, hipStream_t s) {
  if (n <= 0 || S <= 0 || G <= 0 || R < 0 || R > EXT_MAX || (!group && G != 1))
    return hipErrorInvalidValue;
  const int64_t sblocks = (S + GRP_PAIR_THREADS - 1) / GRP_PAIR_THREADS;
  if (G * S > GRP_MAX_CELLS || n > GRP_MAX_NODES || grp_runs(n) * sblocks > 0x7fffffff)
    return hipErrorInvalidValue;
#define KCC_EXT_CASE(r)                                                                         \
  case r:                                                                                       \
    return launch_ext<r>(n, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,    \
                         alloc_x, used_x, group, G, S, spec_cpu, spec_mem, spec_x, w, totals,   \
                         spec_err, s)
  switch (R) {
    KCC_EXT_CASE(0);
    KCC_EXT_CASE(1);
    KCC_EXT_CASE(2);
    KCC_EXT_CASE(3);
    KCC_EXT_CASE(4);
  }
#undef KCC_EXT_CASE
  return hipErrorInvalidValue;
}

}  // namespace kcc
