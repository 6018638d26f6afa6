// kcc_spread.hip — spread constraints in the fit (kcc_fit_capped, kcc_spread_fold; DESIGN.md
// §4.11).  OPT-IN: not the reference's arithmetic.
//
// kcc_fit_capped is kcc_fit_ext with, per (row, spec) and after the pod-slot clamp, the
// per-cell minimum of q and a per-spec cap on one node's count ("at most k per node":
// required pod anti-affinity on the hostname).  Launches (none waits for another workgroup):
//   the records       kcc_ext.hip's (launch_ext_records): hist, scan, ext_scatter<R> with
//                     group ids; ext_rows<R> without
//   cap_pairs<R>      ext_pairs<R>'s body (ext_pairs_body in kcc_internal.h) with SPREAD set:
//                     two 64-bit compare-and-selects per pair after the one conversion, and a
//                     64-bit atomic min beside grp_flush's atomic add; launched as ext_pairs<R>
//                     is (launch_pairs, R through ext_dispatch, both in kcc_internal.h)
//   cap_finalize      grp_finalize plus cell_min (the cells hold q with the sign bit flipped,
//                     so a byte fill of 0xFF is the identity of the unsigned atomic min)
//   grp_rows          group_rows = grp_hist's counts widened to int64
// With neither a cap nor cell_min the call launches launch_fit_ext itself.
//
// kcc_spread_fold folds the G x S cells to one total per spec under a maxSkew over
// topology domains (zones):
//   fold_cells        a thread owns one spec and a slice of the groups: lanes of adjacent
//                     specs read adjacent cells; the thread sums consecutive groups of one
//                     domain in a register and adds the sum to cap[d][s] (64-bit atomic) on a
//                     domain change and at the end of its slice, as the pair loop does
//   fold_finish       one thread per spec: the min over the present domains, the saturating
//                     limit, the clipped wrapping sum
#include "kcc_internal.h"

namespace kcc {
namespace {

template <int R>
__global__ __launch_bounds__(GRP_PAIR_THREADS) void cap_pairs_kernel(
    const uint32_t* __restrict__ total, int64_t n_rec, int64_t S, int64_t sblocks,
    const uint64_t* __restrict__ spec_cpu, const int64_t* __restrict__ spec_mem,
    const int64_t* __restrict__ spec_x, const GrpRow* __restrict__ rec,
    const ExtCol* __restrict__ xrec, const int32_t* __restrict__ rg, int64_t* __restrict__ acc,
    unsigned long long* __restrict__ cnt, const int64_t* __restrict__ node_cap,
    unsigned long long* __restrict__ qmin) {
  ext_pairs_body<R, true>(total, n_rec, S, sblocks, spec_cpu, spec_mem, spec_x, rec, xrec, rg,
                          acc, cnt, node_cap, qmin);
}

// grp_finalize, and cell_min where asked: a flagged cell 0, else the minimum (a cell with
// no rows keeps the fill: INT64_MAX).
__global__ __launch_bounds__(256) void cap_finalize_kernel(
    int64_t cells, const int64_t* __restrict__ acc, const unsigned long long* __restrict__ cnt,
    const unsigned long long* __restrict__ qmin, int64_t* __restrict__ totals,
    int32_t* __restrict__ spec_err, int64_t* __restrict__ cell_min) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= cells) return;
  const bool err = cnt[k] != 0;
  totals[k] = err ? 0 : acc[k];
  spec_err[k] = err ? SPEC_ERR_DIV0 : 0;
  if (cell_min) cell_min[k] = err ? 0 : (int64_t)(qmin[k] ^ SPREAD_SIGN);
}

// count == nullptr (no group ids): out[0] = n.
__global__ __launch_bounds__(256) void grp_rows_kernel(int64_t G, const uint32_t* __restrict__ count,
                                                      int64_t n, int64_t* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  out[g] = count ? (int64_t)count[g] : n;
}

__global__ __launch_bounds__(256) void fill_i64_kernel(int64_t cells, int64_t v,
                                                      int64_t* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < cells) out[k] = v;
}

constexpr int FOLD_THREADS = 256;
constexpr int64_t FOLD_MIN_THREADS = 1 << 16;  // slices are cut until the grid holds this many

__device__ inline void fold_flush(int64_t* __restrict__ cap, uint32_t* __restrict__ present,
                                  int64_t d, int64_t S, int64_t s, uint64_t sum) {
  if (d < 0) return;
  atomicAdd(reinterpret_cast<unsigned long long*>(cap) + d * S + s, (unsigned long long)sum);
  atomicOr(present + d * S + s, 1u);
}

// Thread (s, slice): groups [slice * len, min(G, (slice + 1) * len)) of spec s.
__global__ __launch_bounds__(FOLD_THREADS) void fold_cells_kernel(
    int64_t G, int64_t S, int64_t len, const int64_t* __restrict__ cell_totals,
    const int32_t* __restrict__ cell_err, const int64_t* __restrict__ group_rows,
    const int32_t* __restrict__ domain_of, int64_t D, const uint8_t* __restrict__ eligible,
    int64_t* __restrict__ cap, uint32_t* __restrict__ present, uint32_t* __restrict__ flag) {
  const int64_t s = (int64_t)blockIdx.x * FOLD_THREADS + threadIdx.x;
  if (s >= S) return;
  const int64_t g0 = (int64_t)blockIdx.y * len;
  const int64_t g1 = g0 + len < G ? g0 + len : G;
  int64_t dcur = -1;
  uint64_t sum = 0;
  bool bad = false;
  for (int64_t g = g0; g < g1; ++g) {
    if (group_rows && group_rows[g] <= 0) continue;  // an empty pool is not a domain
    const int64_t d = domain_of ? (int64_t)domain_of[g] : g;
    if (d < 0 || d >= D) continue;  // skipped, as ids are everywhere in this API
    const int64_t cell = g * S + s;
    if (eligible && eligible[cell] == 0) continue;
    bad = bad || cell_err[cell] != 0;
    if (d != dcur) {
      fold_flush(cap, present, dcur, S, s, sum);
      sum = 0;
      dcur = d;
    }
    sum += (uint64_t)cell_totals[cell];
  }
  fold_flush(cap, present, dcur, S, s, sum);
  if (bad) atomicOr(flag + s, 1u);
}

__global__ __launch_bounds__(FOLD_THREADS) void fold_finish_kernel(
    int64_t S, int64_t D, const int64_t* __restrict__ cap, const uint32_t* __restrict__ present,
    const uint32_t* __restrict__ flag, const int64_t* __restrict__ max_skew,
    int64_t* __restrict__ totals, int32_t* __restrict__ spec_err) {
  const int64_t s = (int64_t)blockIdx.x * FOLD_THREADS + threadIdx.x;
  if (s >= S) return;
  if (flag[s] != 0) {  // select_groups' rule
    totals[s] = 0;
    spec_err[s] = SPEC_ERR_DIV0;
    return;
  }
  const int64_t k = max_skew ? max_skew[s] : 0;
  uint64_t sum = 0;
  int64_t m = INT64_MAX;
  bool any = false;
  for (int64_t d = 0; d < D; ++d) {
    if (present[d * S + s] == 0) continue;
    const int64_t c = cap[d * S + s];
    sum += (uint64_t)c;
    m = c < m ? c : m;
    any = true;
  }
  if (k > 0 && any) {
    const int64_t lim = (m > 0 && k > INT64_MAX - m) ? INT64_MAX : m + k;  // saturates
    sum = 0;
    for (int64_t d = 0; d < D; ++d) {
      if (present[d * S + s] == 0) continue;
      const int64_t c = cap[d * S + s];
      sum += (uint64_t)(c <= lim ? c : lim);
    }
  }
  totals[s] = (int64_t)sum;
  spec_err[s] = 0;
}

}  // namespace

hipError_t launch_fill_i64(int64_t cells, int64_t v, int64_t* out, hipStream_t s) {
  if (cells <= 0) return hipSuccess;
  hipLaunchKernelGGL(fill_i64_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, cells,
                     v, out);
  return hipGetLastError();
}

hipError_t launch_group_rows(int64_t n, int64_t G, const int32_t* group, const GrpWork& w,
                             int64_t* group_rows, hipStream_t s) {
  if (n <= 0 || G <= 0 || n > GRP_MAX_NODES || (!group && G != 1)) return hipErrorInvalidValue;
  hipError_t e;
  if (group && (e = launch_grp_count_scan(n, G, group, w, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(grp_rows_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s, G,
                     group ? w.count : (const uint32_t*)nullptr, n, group_rows);
  return hipGetLastError();
}

hipError_t launch_fit_capped(const FitNodes& nd, const FitSpecs& sp, const ExtWork& w,
                             unsigned long long* qmin, int64_t* totals, int32_t* spec_err,
                             int64_t* cell_min, int64_t* group_rows, hipStream_t s) {
  hipError_t e;
  if (!sp.node_cap && !cell_min) {
    // kcc_fit_ext's own launches (with group ids they leave grp_hist's counts in w.g.count)
    if ((e = launch_fit_ext(nd, sp, w, totals, spec_err, s)) != hipSuccess) return e;
  } else {
    if (cell_min && !qmin) return hipErrorInvalidValue;
    if ((e = launch_ext_records(nd, sp.S, w, s)) != hipSuccess) return e;
    const int64_t cells = nd.G * sp.S;
    unsigned long long* qm = cell_min ? qmin : nullptr;
    if (qm && (e = hipMemsetAsync(qm, 0xFF, 8 * (size_t)cells, s)) != hipSuccess) return e;
    e = ext_dispatch(nd.R, [&](auto r) {
      return launch_pairs(cap_pairs_kernel<decltype(r)::value>, nd, sp, w, s, sp.node_cap, qm);
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cap_finalize_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s,
                       cells, w.g.acc, w.g.cnt(cells), qm, totals, spec_err, cell_min);
  }
  if (group_rows)
    hipLaunchKernelGGL(grp_rows_kernel, dim3((unsigned)((nd.G + 255) / 256)), dim3(256), 0, s, nd.G,
                       nd.group ? w.g.count : (const uint32_t*)nullptr, nd.n, group_rows);
  return hipGetLastError();
}

hipError_t launch_spread_fold(int64_t G, int64_t S, const int64_t* cell_totals,
                              const int32_t* cell_err, const int64_t* group_rows,
                              const int32_t* domain_of, int64_t D, const uint8_t* eligible,
                              const int64_t* max_skew, const FoldWork& w, int64_t* totals,
                              int32_t* spec_err, hipStream_t s) {
  if (G <= 0 || S <= 0 || D <= 0 || G * S > GRP_MAX_CELLS || D * S > GRP_MAX_CELLS ||
      (!domain_of && D != G))
    return hipErrorInvalidValue;
  hipError_t e;
  if ((e = hipMemsetAsync(w.cap, 0, 8 * (size_t)(D * S), s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(w.present, 0, 4 * (size_t)(D * S), s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(w.flag, 0, 4 * (size_t)S, s)) != hipSuccess) return e;
  const int64_t sblocks = (S + FOLD_THREADS - 1) / FOLD_THREADS;
  int64_t slices = (FOLD_MIN_THREADS + sblocks * FOLD_THREADS - 1) / (sblocks * FOLD_THREADS);
  slices = slices < G ? slices : G;
  slices = slices < 65535 ? slices : 65535;
  const int64_t len = (G + slices - 1) / slices;
  slices = (G + len - 1) / len;
  hipLaunchKernelGGL(fold_cells_kernel, dim3((unsigned)sblocks, (unsigned)slices),
                     dim3(FOLD_THREADS), 0, s, G, S, len, cell_totals, cell_err, group_rows,
                     domain_of, D, eligible, w.cap, w.present, w.flag);
  hipLaunchKernelGGL(fold_finish_kernel, dim3((unsigned)sblocks), dim3(FOLD_THREADS), 0, s, S, D,
                     w.cap, w.present, w.flag, max_skew, totals, spec_err);
  return hipGetLastError();
}

}  // namespace kcc
