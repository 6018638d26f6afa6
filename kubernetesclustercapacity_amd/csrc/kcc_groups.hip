// kcc_groups.hip — grouped fit: per node-group x spec totals in one call.
//
// totals[g][s] is what the reference's node loop (CC:105-140) gives for spec s on exactly
// the rows of group g, with Go's 64-bit semantics (uint64 CPU division reinterpreted as int,
// truncating int64 memory division with MinInt64 / -1 == MinInt64, signed findMin, the
// pod-slot clamp allocatablePods - len(pods)), and a per-cell flag where Go would panic.
//
// Five launches, none of which waits for another workgroup:
//   grp_hist     rows per group (LDS-summed per workgroup, then one device atomic per bin)
//   grp_scan     one workgroup: exclusive scan of the G counts -> the groups' cursors
//   grp_scatter  one thread per row: the row record (free CPU / memory, P, clamp, fast
//                class) placed in group order (a workgroup reserves each group's slots
//                with one atomic on its cursor)
//   grp_pairs    a wave holds 64 specs in its lanes and walks GRP_RUN group-ordered rows
//                (staged in LDS, read as broadcasts); each lane keeps an int64 sum and a
//                divide-by-zero count and the wave flushes them with 64-bit atomic adds to
//                acc[g][s] / cnt[g][s] on a group change and at the end of the run
//   grp_finalize one thread per cell: err = cnt > 0, totals = err ? 0 : acc
// The order of the rows inside a group is whatever the cursors gave: the sums wrap, so the
// results do not depend on it.
//
// Arithmetic.  The exact path is kcc_rows.hip's, per pair.  The fast path serves a fast
// row (free CPU < 2^31, 0 <= free memory < 2^50) under a wave whose 64 specs are all fast
// (1 <= c <= 2^52, 1 <= m <= 2^52): t = trunc(f * (1/d)) in f64 is within 1 of the
// quotient, and the remainder r = fma(-t, d, f) — exact — says which way (DESIGN.md
// §4.9 has the proof).  No rounding mode is changed.
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

// One thread per row: the row's record at the next slot of its group.
__global__ __launch_bounds__(GRP_SORT_THREADS) void grp_scatter_kernel(
    int64_t n, int64_t G, const int32_t* __restrict__ group,
    const uint64_t* __restrict__ alloc_cpu, const int64_t* __restrict__ alloc_mem,
    const int64_t* __restrict__ alloc_pods, const int64_t* __restrict__ pod_count,
    const uint64_t* __restrict__ used_cpu, const int64_t* __restrict__ used_mem,
    uint32_t* __restrict__ cursor, GrpRow* __restrict__ rec, int32_t* __restrict__ rg, int lds) {
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
  const uint64_t ac = alloc_cpu[i], uc = used_cpu[i];
  const int64_t am = alloc_mem[i], um = used_mem[i];
  const int64_t P = alloc_pods[i];
  GrpRow r;
  r.fc = ac > uc ? ac - uc : 0;                                    // CC:119 (uint64 compare)
  r.fm = am > um ? (int64_t)((uint64_t)am - (uint64_t)um) : 0;     // CC:125 (the difference wraps)
  r.P = P;
  r.cl = (int64_t)((uint64_t)P - (uint64_t)pod_count[i]);          // CC:135
  const bool fast = r.fc < GRP_FC_MAX && (uint64_t)r.fm < GRP_FM_MAX;
  r.fcd = fast ? (double)r.fc : 0.0;
  r.fmd = fast ? (double)r.fm : 0.0;
  rec[pos] = r;
  rg[pos] = g | (fast ? GRP_ROW_FAST : 0);
}

__global__ __launch_bounds__(GRP_PAIR_THREADS) void grp_pairs_kernel(
    const uint32_t* __restrict__ total, int64_t S, int64_t sblocks,
    const uint64_t* __restrict__ spec_cpu, const int64_t* __restrict__ spec_mem,
    const GrpRow* __restrict__ rec, const int32_t* __restrict__ rg, int64_t* __restrict__ acc,
    unsigned long long* __restrict__ cnt) {
  __shared__ GrpRow s_rec[GRP_RUN];
  __shared__ int32_t s_rg[GRP_RUN];
  const int64_t run = (int64_t)blockIdx.x / sblocks;
  const int64_t sb = (int64_t)blockIdx.x - run * sblocks;
  const int64_t M = *total;
  const int64_t base = run * GRP_RUN;
  if (base >= M) return;
  const int nr = (int)(M - base < GRP_RUN ? M - base : GRP_RUN);
  for (int j = threadIdx.x; j < nr; j += GRP_PAIR_THREADS) {
    s_rec[j] = rec[base + j];
    s_rg[j] = rg[base + j];
  }
  __syncthreads();

  const int64_t s = sb * GRP_PAIR_THREADS + threadIdx.x;
  const bool live = s < S;
  const uint64_t c = live ? spec_cpu[s] : 1;
  const int64_t m = live ? spec_mem[s] : 1;
  const bool spec_fast = c >= 1 && c <= GRP_SPEC_MAX && m >= 1 && (uint64_t)m <= GRP_SPEC_MAX;
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
      q = (int64_t)(int32_t)(tc <= tm ? tc : tm);  // findMin (CC:133); <= free CPU < 2^31
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
      z += dz ? 1u : 0u;
    }
    if (q >= r.P) q = r.cl;  // CC:134-136
    sum = (int64_t)((uint64_t)sum + (uint64_t)q);
  }
  grp_flush(acc, cnt, (int64_t)gcur * S + s, live, sum, z);
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

hipError_t launch_fit_grouped(int64_t n, const uint64_t* alloc_cpu, const int64_t* alloc_mem,
                              const int64_t* alloc_pods, const int64_t* pod_count,
                              const uint64_t* used_cpu, const int64_t* used_mem,
                              const int32_t* group, int64_t G, int64_t S, const uint64_t* spec_cpu,
                              const int64_t* spec_mem, const GrpWork& w, int64_t* totals,
                              int32_t* spec_err, hipStream_t s) {
  if (n <= 0 || S <= 0 || G <= 0) return hipErrorInvalidValue;
  const int64_t cells = G * S;
  const int64_t sort_grid = (n + GRP_SORT_THREADS - 1) / GRP_SORT_THREADS;
  const int64_t sblocks = (S + GRP_PAIR_THREADS - 1) / GRP_PAIR_THREADS;
  const int64_t pair_grid = grp_runs(n) * sblocks;
  if (cells > GRP_MAX_CELLS || n > GRP_MAX_NODES || pair_grid > 0x7fffffff) return hipErrorInvalidValue;
  const int lds = G <= GRP_LDS_GROUPS ? 1 : 0;
  hipError_t e;
  if ((e = hipMemsetAsync(w.acc, 0, 16 * (size_t)cells, s)) != hipSuccess) return e;
  int64_t* acc = w.acc;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(w.acc + cells);
  if ((e = launch_grp_count_scan(n, G, group, w, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(grp_scatter_kernel, dim3((unsigned)sort_grid), dim3(GRP_SORT_THREADS), 0, s, n,
                     G, group, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
                     w.cursor, w.rec, w.rg, lds);
  hipLaunchKernelGGL(grp_pairs_kernel, dim3((unsigned)pair_grid), dim3(GRP_PAIR_THREADS), 0, s,
                     w.total, S, sblocks, spec_cpu, spec_mem, w.rec, w.rg, acc, cnt);
  if ((e = launch_grp_finalize(cells, acc, cnt, totals, spec_err, s)) != hipSuccess) return e;
  return hipGetLastError();
}

}  // namespace kcc
