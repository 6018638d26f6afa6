// kcc_explain.hip — the fit explained (kcc_fit_explain).  OPT-IN: not the
// reference's arithmetic.
//
// kcc_fit_explain is kcc_fit_capped with the provenance of every pair kept: which term of the
// per-node findMin (CPU, memory, extra resource r, the pod-slot clamp, the per-node cap) holds
// the row's q, counted per cell as rows (why_rows) and as replicas (why_pods), and what stays
// free once the cell holds its total (left).  Launches (none waits for another workgroup):
//   the records       kcc_ext.hip's (launch_ext_records), as every cell fit
//   why_pairs<R>      ext_pairs<R>'s body (ext_pairs_body in kcc_internal.h) with SPREAD and WHY
//                     set: the reason rides on the selects that already encode findMin's tie
//                     rule, R + 4 counters and R + 4 sums per lane (static indices), flushed
//                     beside grp_flush with 64-bit atomic adds into the caller's zeroed
//                     plane-major outputs (a wave's 64 atomics are contiguous)
//   why_free<R>       left needs no per-pair work: modulo 2^64
//                       sum_i (f_i - q_i req) = sum_i f_i - req x totals[cell],
//                     so one pass over the group-ordered records sums fc, fm and fx_r per group
//                     into (2 + R) G words: a wave takes 64 x WHY_FREE_IPL consecutive records,
//                     lane-strided (coalesced; a lane's records stay in group order), a
//                     register sum per lane, an atomic add on a group change and at the end —
//                     or, when the wave's records are all of one group, one wave reduction and
//                     one atomic per plane
//   why_finalize      totals / spec_err as cap_finalize; the flagged cells' why_* entries
//                     zeroed; left[c][cell] = free[c][g] - req_c[s] x totals[cell]
// With only left asked for, the pair loop is kcc_fit_capped's own (launch_fit_capped); with
// nothing asked for the whole call is.
#include "kcc_internal.h"

namespace kcc {
namespace {

template <int R>
__global__ __launch_bounds__(GRP_PAIR_THREADS) void why_pairs_kernel(
    const uint32_t* __restrict__ total, int64_t n_rec, int64_t S, int64_t sblocks,
    const uint64_t* __restrict__ spec_cpu, const int64_t* __restrict__ spec_mem,
    const int64_t* __restrict__ spec_x, const GrpRow* __restrict__ rec,
    const ExtCol* __restrict__ xrec, const int32_t* __restrict__ rg, int64_t* __restrict__ acc,
    unsigned long long* __restrict__ cnt, const int64_t* __restrict__ node_cap,
    unsigned long long* __restrict__ why_rows, unsigned long long* __restrict__ why_pods,
    int64_t cells) {
  ext_pairs_body<R, true, true>(total, n_rec, S, sblocks, spec_cpu, spec_mem, spec_x, rec, xrec,
                                rg, acc, cnt, node_cap, nullptr, why_rows, why_pods, cells);
}

constexpr int WHY_FREE_THREADS = 256;
constexpr int64_t WHY_FREE_CHUNK = 64 * WHY_FREE_IPL;  // records per wave

template <int R>
__device__ inline void free_flush(unsigned long long* __restrict__ free, int64_t G, int g,
                                  const uint64_t (&a)[2 + R]) {
#pragma unroll
  for (int c = 0; c < 2 + R; ++c)
    if (a[c] != 0) atomicAdd(free + (int64_t)c * G + g, (unsigned long long)a[c]);
}

// free[c * G + g] += the free amounts of group g's records (c = 0 CPU, 1 memory, 2 + r extra
// resource r); free is zero before the launch.  total == nullptr: the n_rec records of the
// ungrouped pass; else *total.
template <int R>
__global__ __launch_bounds__(WHY_FREE_THREADS) void why_free_kernel(
    const uint32_t* __restrict__ total, int64_t n_rec, int64_t G, const GrpRow* __restrict__ rec,
    const ExtCol* __restrict__ xrec, const int32_t* __restrict__ rg,
    unsigned long long* __restrict__ free) {
  const int64_t M = total ? (int64_t)*total : n_rec;
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * WHY_FREE_THREADS + threadIdx.x) >> 6;
  const int64_t base = wave * WHY_FREE_CHUNK;
  if (base >= M) return;  // wave-uniform
  const int64_t end = base + WHY_FREE_CHUNK < M ? base + WHY_FREE_CHUNK : M;
  const int g0 = rg[base] & (GRP_ROW_FAST - 1);
  const bool one = (rg[end - 1] & (GRP_ROW_FAST - 1)) == g0;  // wave-uniform: records are in group order
  uint64_t a[2 + R];
#pragma unroll
  for (int c = 0; c < 2 + R; ++c) a[c] = 0;
  int gcur = g0;
  for (int64_t p = base + lane; p < end; p += 64) {
    const int g = rg[p] & (GRP_ROW_FAST - 1);
    if (g != gcur) {  // (never with `one`)
      free_flush<R>(free, G, gcur, a);
#pragma unroll
      for (int c = 0; c < 2 + R; ++c) a[c] = 0;
      gcur = g;
    }
    a[0] += rec[p].fc;
    a[1] += (uint64_t)rec[p].fm;
#pragma unroll
    for (int k = 0; k < R; ++k) a[2 + k] += (uint64_t)xrec[p * R + k].fx;
  }
  if (one) {  // all 64 lanes are here
#pragma unroll
    for (int c = 0; c < 2 + R; ++c) {
      unsigned long long v = a[c];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
      a[c] = lane == 0 ? v : 0;
    }
  }
  free_flush<R>(free, G, gcur, a);
}

// One thread per cell.  totals != nullptr: totals / spec_err as grp_finalize writes them (else
// launch_fit_capped already has).  A flagged cell: every why_* and left entry 0.
__global__ __launch_bounds__(256) void why_finalize_kernel(
    int64_t cells, int64_t S, int64_t G, int R, const int64_t* __restrict__ acc,
    const unsigned long long* __restrict__ cnt, const uint64_t* __restrict__ spec_cpu,
    const int64_t* __restrict__ spec_mem, const int64_t* __restrict__ spec_x,
    const unsigned long long* __restrict__ free, int64_t* __restrict__ totals,
    int32_t* __restrict__ spec_err, int64_t* __restrict__ why_rows,
    int64_t* __restrict__ why_pods, int64_t* __restrict__ left) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= cells) return;
  const bool err = cnt[k] != 0;
  const uint64_t t = err ? 0 : (uint64_t)acc[k];
  if (totals) {
    totals[k] = (int64_t)t;
    spec_err[k] = err ? SPEC_ERR_DIV0 : 0;
  }
  if (err) {
    for (int b = 0; b < WHY_SLOTS; ++b) {
      if (why_rows) why_rows[b * cells + k] = 0;
      if (why_pods) why_pods[b * cells + k] = 0;
    }
  }
  if (!left) return;
  const int64_t g = k / S, s = k - g * S;
  left[k] = err ? 0 : (int64_t)(free[g] - spec_cpu[s] * t);
  left[cells + k] = err ? 0 : (int64_t)(free[G + g] - (uint64_t)spec_mem[s] * t);
  for (int r = 0; r < R; ++r)  // (an unrequested resource: x = 0 leaves its whole free amount)
    left[(2 + r) * cells + k] =
        err ? 0 : (int64_t)(free[(int64_t)(2 + r) * G + g] - (uint64_t)spec_x[(int64_t)r * S + s] * t);
}

}  // namespace

hipError_t launch_fit_explain(const FitNodes& nd, const FitSpecs& sp, const ExtWork& w,
                              unsigned long long* free, int64_t* totals, int32_t* spec_err,
                              int64_t* why_rows, int64_t* why_pods, int64_t* left, hipStream_t s) {
  const bool why = why_rows || why_pods;
  hipError_t e;
  if (!why) {  // kcc_fit_capped's own launches (acc / cnt stay in w.g.acc)
    if ((e = launch_fit_capped(nd, sp, w, nullptr, totals, spec_err, nullptr, nullptr, s)) != hipSuccess)
      return e;
    if (!left) return hipSuccess;
  }
  const int64_t cells = nd.G * sp.S;
  if (why) {
    if (WHY_SLOTS * cells > GRP_MAX_CELLS) return hipErrorInvalidValue;
    if ((e = launch_ext_records(nd, sp.S, w, s)) != hipSuccess) return e;
    const size_t bytes = 8 * (size_t)WHY_SLOTS * (size_t)cells;
    if (why_rows && (e = hipMemsetAsync(why_rows, 0, bytes, s)) != hipSuccess) return e;
    if (why_pods && (e = hipMemsetAsync(why_pods, 0, bytes, s)) != hipSuccess) return e;
    e = ext_dispatch(nd.R, [&](auto r) {
      return launch_pairs(why_pairs_kernel<decltype(r)::value>, nd, sp, w, s, sp.node_cap,
                          reinterpret_cast<unsigned long long*>(why_rows),
                          reinterpret_cast<unsigned long long*>(why_pods), cells);
    });
    if (e != hipSuccess) return e;
  }
  if (left) {
    if (!free) return hipErrorInvalidValue;
    if ((e = hipMemsetAsync(free, 0, 8 * (size_t)((2 + nd.R) * nd.G), s)) != hipSuccess) return e;
    const int64_t waves = (nd.n + WHY_FREE_CHUNK - 1) / WHY_FREE_CHUNK;
    const int64_t grid = (waves * 64 + WHY_FREE_THREADS - 1) / WHY_FREE_THREADS;
    e = ext_dispatch(nd.R, [&](auto r) {
      hipLaunchKernelGGL(why_free_kernel<decltype(r)::value>, dim3((unsigned)grid),
                         dim3(WHY_FREE_THREADS), 0, s,
                         nd.group ? w.g.total : (const uint32_t*)nullptr, nd.n, nd.G, w.g.rec,
                         w.xrec, w.g.rg, free);
      return hipGetLastError();
    });
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(why_finalize_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s,
                     cells, sp.S, nd.G, (int)nd.R, w.g.acc, w.g.cnt(cells), sp.spec_cpu, sp.spec_mem,
                     sp.spec_x, free, why ? totals : (int64_t*)nullptr,
                     why ? spec_err : (int32_t*)nullptr, why_rows, why_pods, left);
  return hipGetLastError();
}

}  // namespace kcc
