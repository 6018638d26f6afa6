// kcc_deploy.hip — commit a rollout plan to the node rows (kcc_deploy).
// OPT-IN: not the reference's arithmetic.
//
// A plan is K steps run in order; step k places up to replicas[k] pods of one spec on the
// rows that can hold them and leaves pod_count / used_cpu / used_mem / used_x updated on the
// device for the next step and for the fit that follows.  Rows are cut into tiles of
// DEPLOY_TILE (256 threads x DEPLOY_IPT consecutive rows).  Launches of one step (none waits
// for another workgroup; each reads only what earlier launches finished):
//   dp_rows<R, SPREAD>  one thread per row: q as kcc_fit_ext (64-bit integer arithmetic, the
//                       pod-slot clamp after all the mins), the divide-by-zero rule, then
//                       a = min(cap(max(q, 0)), Rk) (0 for an ineligible row) as uint32; the
//                       tile's sum of a (wave reduce, LDS, one store) and an atomic OR on the
//                       step's flag word where an eligible row would panic.  SPREAD: also
//                       round 0 of the digit search's histogram (the top 7 bits of a)
//   dp_hist (SPREAD)    rounds 1..3 of the digit search for the water level: per 8-bit digit
//                       of the rows under the prefix chosen so far, the count and the sum of
//                       a, summed in LDS and added to 256 global bins.  Every workgroup picks
//                       the previous round's digit from that round's finished bins itself
//   dp_ind (SPREAD)     picks the last digit: t - 1 is known; the tile's count of a >= t
//   dp_scan             one workgroup: exclusive scan of the tile sums
//   dp_apply<R, SPREAD> rescans the tile from its offset, p per row, commits the state, writes
//                       placed_rows, adds into placed[k] / nodes_used[k]; a flagged step
//                       writes zeros and leaves the state alone
// PACK: dp_rows, dp_scan, dp_apply.  SPREAD: dp_rows, dp_hist x 3, dp_ind, dp_scan, dp_apply.
// The plan's values are read on the device by index k: the host loop over k only enqueues.
#include "kcc_internal.h"

namespace kcc {
namespace {

constexpr int DP_THREADS = 256;
constexpr int DP_WAVES = DP_THREADS / 64;
static_assert(DEPLOY_TILE == DP_THREADS * DEPLOY_IPT, "a thread owns DEPLOY_IPT consecutive rows");
static_assert(DEPLOY_SCAN_PASS == DP_THREADS, "dp_scan takes one tile sum per thread and pass");

// Inclusive scan over the wavefront (64 lanes).
__device__ inline uint64_t wave_scan(uint64_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = (uint64_t)__shfl_up((unsigned long long)v, o);
    if (lane >= o) v += t;
  }
  return v;
}

// Exclusive scan of v over the workgroup's DP_THREADS threads; *total = the sum.  s_w: DP_WAVES
// words of LDS (the call synchronises before it writes them and before it returns).
__device__ inline uint64_t block_scan(uint64_t v, uint64_t* s_w, uint64_t* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t inc = wave_scan(v);
  __syncthreads();
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  uint64_t base = 0, all = 0;
#pragma unroll
  for (int j = 0; j < DP_WAVES; ++j) {
    const uint64_t x = s_w[j];
    base += j < w ? x : 0;
    all += x;
  }
  *total = all;
  return base + inc - v;
}

__device__ inline uint64_t block_sum(uint64_t v, uint64_t* s_w) {
  uint64_t total;
  (void)block_scan(v, s_w, &total);
  return total;
}

__device__ inline int64_t step_replicas(const int64_t* __restrict__ replicas, int64_t k) {
  const int64_t r = replicas[k];
  return r < 0 ? 0 : (r > DEPLOY_R_MAX ? DEPLOY_R_MAX : r);
}

// One round of the digit search, by the whole workgroup (thread d owns digit d).  In: st_in
// (the state after the earlier rounds; nullptr before round 0) and the round's finished bins.
// u_d = ((prefix << 8) | d) << shift is the candidate level with this digit and zeros below;
//   f(u_d) = s_below + (sum of a over the prefix's rows with a smaller digit)
//          + u_d (c_above + the prefix's rows with this digit or a larger one)
// is exact, f is monotone, and the digit chosen is the largest with f(u_d) < Rk (digit 0
// qualifies by induction: f(0) = 0 < Rk).  Out (every thread): the state after this round —
// prefix, s_below = the sum of a over the rows below the prefix, c_above = the rows above it,
// f = f(prefix with zeros below).  After round 3 prefix = t - 1, f = f(t - 1) and c_above =
// #{a >= t}.
__device__ inline void dp_pick(int round, const uint64_t* __restrict__ st_in,
                               const uint64_t* __restrict__ bins, uint64_t Rk, uint64_t* s_w,
                               uint64_t* s_out, uint64_t out[DEPLOY_ST_WORDS]) {
  const int d = threadIdx.x;
  const uint64_t prefix = st_in ? st_in[0] : 0, s_below = st_in ? st_in[1] : 0;
  const uint64_t c_above = st_in ? st_in[2] : 0;
  const uint64_t cnt = bins[2 * d], sm = bins[2 * d + 1];
  uint64_t cnt_all, sm_all;
  const uint64_t cnt_lt = block_scan(cnt, s_w, &cnt_all);
  const uint64_t sm_lt = block_scan(sm, s_w, &sm_all);
  const int shift = 24 - 8 * round;
  const uint64_t u = ((prefix << 8) | (uint64_t)d) << shift;
  const uint64_t f = s_below + sm_lt + u * (c_above + (cnt_all - cnt_lt));
  const bool ok = f < Rk && u <= (uint64_t)DEPLOY_R_MAX;  // (round 0 has 7 bits)
  const int n_ok = __syncthreads_count(ok);
  const int pick = n_ok > 0 ? n_ok - 1 : 0;  // n_ok == 0 only with Rk == 0: nothing is placed
  if (d == pick) {
    s_out[0] = (prefix << 8) | (uint64_t)d;
    s_out[1] = s_below + sm_lt;
    s_out[2] = c_above + (cnt_all - cnt_lt) - cnt;
    s_out[3] = f;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < DEPLOY_ST_WORDS; ++j) out[j] = s_out[j];
}

// Adds the workgroup's rows into the round's histogram: rows whose bits above the digit equal
// `prefix` (match), by digit.  s_cnt / s_sum: 256 LDS bins each, zeroed here.
struct HistLds {
  unsigned int cnt[256];
  unsigned long long sum[256];
};
__device__ inline void hist_zero(HistLds& h) {
  h.cnt[threadIdx.x] = 0;
  h.sum[threadIdx.x] = 0;
  __syncthreads();
}
__device__ inline void hist_add(HistLds& h, bool on, uint32_t a, int shift) {
  const unsigned d = (a >> shift) & 255u;
  // a cluster's a values are mostly alike in the upper digits: one lane adds for the wave
  const unsigned d0 = (unsigned)__builtin_amdgcn_readfirstlane((int)d);
  if (__all(on && d == d0)) {
    uint64_t s = a;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += (uint64_t)__shfl_xor((unsigned long long)s, o);
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&h.cnt[d0], 64u);
      atomicAdd(&h.sum[d0], (unsigned long long)s);
    }
  } else if (on) {
    atomicAdd(&h.cnt[d], 1u);
    atomicAdd(&h.sum[d], (unsigned long long)a);
  }
}
__device__ inline void hist_flush(HistLds& h, uint64_t* __restrict__ bins) {
  __syncthreads();
  const unsigned int c = h.cnt[threadIdx.x];
  if (c != 0) {
    atomicAdd(reinterpret_cast<unsigned long long*>(bins) + 2 * threadIdx.x, (unsigned long long)c);
    atomicAdd(reinterpret_cast<unsigned long long*>(bins) + 2 * threadIdx.x + 1, h.sum[threadIdx.x]);
  }
}

struct DpNodes {
  int64_t n;
  const uint64_t* alloc_cpu;
  const int64_t* alloc_mem;
  const int64_t* alloc_pods;
  const int64_t* alloc_x;  // [R, n]
  int64_t* pod_count;
  uint64_t* used_cpu;
  int64_t* used_mem;
  int64_t* used_x;  // [R, n]
  const int32_t* group;
  int64_t G;
  const uint8_t* eligible;  // [G, K]
};
struct DpPlan {
  int64_t K;
  const uint64_t* spec_cpu;
  const int64_t* spec_mem;
  const int64_t* spec_x;  // [R, K]
  const int64_t* replicas;
  const int64_t* node_cap;
};

template <int R, bool SPREAD>
__global__ __launch_bounds__(DP_THREADS) void dp_rows_kernel(DpNodes nd, DpPlan pl, int64_t k,
                                                            uint32_t* __restrict__ a_out,
                                                            uint64_t* __restrict__ tile_sum,
                                                            uint32_t* __restrict__ flag,
                                                            uint64_t* __restrict__ bins0) {
  constexpr int RR = R ? R : 1;
  __shared__ uint64_t s_w[DP_WAVES];
  __shared__ HistLds s_h;
  const uint64_t c = pl.spec_cpu[k];
  const int64_t m = pl.spec_mem[k];
  int64_t x[RR];
#pragma unroll
  for (int r = 0; r < R; ++r) x[r] = pl.spec_x[(int64_t)r * pl.K + k];
  const int64_t Rk = step_replicas(pl.replicas, k);
  const int64_t capk = pl.node_cap ? pl.node_cap[k] : 0;
  if constexpr (SPREAD) hist_zero(s_h);
  const int64_t base = ((int64_t)blockIdx.x * DP_THREADS + threadIdx.x) * DEPLOY_IPT;
  uint64_t sum = 0;
  bool panic = false;
#pragma unroll
  for (int j = 0; j < DEPLOY_IPT; ++j) {
    const int64_t i = base + j;
    const bool in = i < nd.n;
    uint32_t a = 0;
    if (in) {
      bool el = true;
      if (nd.group) {
        const int32_t g = nd.group[i];
        el = grp_valid(g, nd.G);
        if (el && nd.eligible) el = nd.eligible[(int64_t)g * pl.K + k] != 0;
      } else if (nd.eligible) {
        el = nd.eligible[k] != 0;
      }
      if (el) {
        const uint64_t ac = nd.alloc_cpu[i], uc = nd.used_cpu[i];
        const int64_t am = nd.alloc_mem[i], um = nd.used_mem[i];
        const int64_t P = nd.alloc_pods[i], pc = nd.pod_count[i];
        bool z;
        int64_t q = deploy_row_q<R>(ac, uc, am, um, P, pc, c, m, x,
                                    [&](int r, int64_t& ax, int64_t& ux) {
                                      ax = nd.alloc_x[(int64_t)r * nd.n + i];
                                      ux = nd.used_x[(int64_t)r * nd.n + i];
                                    },
                                    z);
        q = (capk > 0 && q > capk) ? capk : q;  // the per-node cap: after the clamp
        q = q > Rk ? Rk : q;
        a = z ? 0u : (uint32_t)q;
        panic = panic || z;
      }
      a_out[i] = a;
    }
    sum += a;
    if constexpr (SPREAD) hist_add(s_h, in, a, 24);
  }
  if (panic) atomicOr(flag, 1u);
  if constexpr (SPREAD) {
    hist_flush(s_h, bins0);
  } else {
    const uint64_t t = block_sum(sum, s_w);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = t;
  }
}

// Rounds 1..3: picks round - 1's digit from its bins, then this round's histogram.  Workgroup 0
// records the state after round - 1 (st[round - 1]) for the next launch.
__global__ __launch_bounds__(DP_THREADS) void dp_hist_kernel(int64_t n, int round,
                                                            const int64_t* __restrict__ replicas,
                                                            int64_t k, const uint32_t* __restrict__ a_in,
                                                            uint64_t* __restrict__ st,
                                                            uint64_t* __restrict__ bins) {
  __shared__ uint64_t s_w[DP_WAVES];
  __shared__ uint64_t s_out[DEPLOY_ST_WORDS];
  __shared__ HistLds s_h;
  uint64_t cur[DEPLOY_ST_WORDS];
  dp_pick(round - 1, round > 1 ? st + (round - 2) * DEPLOY_ST_WORDS : nullptr,
          bins + (int64_t)(round - 1) * 512, (uint64_t)step_replicas(replicas, k), s_w, s_out, cur);
  if (blockIdx.x == 0 && threadIdx.x < DEPLOY_ST_WORDS)
    st[(round - 1) * DEPLOY_ST_WORDS + threadIdx.x] = cur[threadIdx.x];
  hist_zero(s_h);
  const int shift = 24 - 8 * round;
  const int64_t base = ((int64_t)blockIdx.x * DP_THREADS + threadIdx.x) * DEPLOY_IPT;
#pragma unroll
  for (int j = 0; j < DEPLOY_IPT; ++j) {
    const int64_t i = base + j;
    const uint32_t a = i < n ? a_in[i] : 0u;
    const bool on = i < n && ((uint64_t)a >> (shift + 8)) == cur[0];
    hist_add(s_h, on, a, shift);
  }
  hist_flush(s_h, bins + (int64_t)round * 512);
}

// Picks round 3's digit: st[3] = (t - 1, ., #{a >= t}, f(t - 1)); the tile's count of a >= t.
__global__ __launch_bounds__(DP_THREADS) void dp_ind_kernel(int64_t n, const int64_t* __restrict__ replicas,
                                                           int64_t k, const uint32_t* __restrict__ a_in,
                                                           uint64_t* __restrict__ st,
                                                           const uint64_t* __restrict__ bins,
                                                           uint64_t* __restrict__ tile_sum) {
  __shared__ uint64_t s_w[DP_WAVES];
  __shared__ uint64_t s_out[DEPLOY_ST_WORDS];
  uint64_t cur[DEPLOY_ST_WORDS];
  dp_pick(3, st + 2 * DEPLOY_ST_WORDS, bins + 3 * 512, (uint64_t)step_replicas(replicas, k), s_w,
          s_out, cur);
  if (blockIdx.x == 0 && threadIdx.x < DEPLOY_ST_WORDS)
    st[3 * DEPLOY_ST_WORDS + threadIdx.x] = cur[threadIdx.x];
  const uint64_t t = cur[0] + 1;
  const int64_t base = ((int64_t)blockIdx.x * DP_THREADS + threadIdx.x) * DEPLOY_IPT;
  uint64_t cnt = 0;
#pragma unroll
  for (int j = 0; j < DEPLOY_IPT; ++j) {
    const int64_t i = base + j;
    cnt += (i < n && (uint64_t)a_in[i] >= t) ? 1u : 0u;
  }
  const uint64_t all = block_sum(cnt, s_w);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
}

// Exclusive scan of the tile sums by one workgroup, DEPLOY_SCAN_PASS sums a pass.
__global__ __launch_bounds__(DP_THREADS) void dp_scan_kernel(int64_t tiles,
                                                            const uint64_t* __restrict__ tile_sum,
                                                            uint64_t* __restrict__ tile_off) {
  __shared__ uint64_t s_w[DP_WAVES];
  uint64_t carry = 0;
  for (int64_t b = 0; b < tiles; b += DEPLOY_SCAN_PASS) {
    const int64_t j = b + threadIdx.x;
    const uint64_t v = j < tiles ? tile_sum[j] : 0;
    uint64_t all;
    const uint64_t ex = block_scan(v, s_w, &all);
    if (j < tiles) tile_off[j] = carry + ex;
    carry += all;
  }
}

template <int R, bool SPREAD>
__global__ __launch_bounds__(DP_THREADS) void dp_apply_kernel(
    DpNodes nd, DpPlan pl, int64_t k, const uint32_t* __restrict__ a_in,
    const uint64_t* __restrict__ tile_off, const uint32_t* __restrict__ flag,
    const uint64_t* __restrict__ st, int64_t* __restrict__ placed, int64_t* __restrict__ nodes_used,
    int32_t* __restrict__ step_err, int64_t* __restrict__ placed_rows) {
  __shared__ uint64_t s_w[DP_WAVES];
  const bool bad = *flag != 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) step_err[k] = bad ? SPEC_ERR_DIV0 : 0;
  const int64_t base = ((int64_t)blockIdx.x * DP_THREADS + threadIdx.x) * DEPLOY_IPT;
  int64_t* rows_out = placed_rows ? placed_rows + k * nd.n : nullptr;
  if (bad) {  // (uniform over the launch) the state is untouched
    if (rows_out)
      for (int j = 0; j < DEPLOY_IPT; ++j)
        if (base + j < nd.n) rows_out[base + j] = 0;
    return;
  }
  const uint64_t Rk = (uint64_t)step_replicas(pl.replicas, k);
  uint32_t a[DEPLOY_IPT];
  uint64_t mine = 0;  // PACK: the thread's sum of a; SPREAD: its rows with a >= t
  [[maybe_unused]] uint64_t t = 0, rem = 0;
  if constexpr (SPREAD) {
    t = st[3 * DEPLOY_ST_WORDS] + 1;
    rem = Rk - st[3 * DEPLOY_ST_WORDS + 3];  // Rk - f(t - 1): >= 1 when Rk >= 1
  }
#pragma unroll
  for (int j = 0; j < DEPLOY_IPT; ++j) {
    a[j] = base + j < nd.n ? a_in[base + j] : 0u;
    mine += SPREAD ? ((uint64_t)a[j] >= t ? 1u : 0u) : a[j];
  }
  uint64_t all;
  uint64_t before = tile_off[blockIdx.x] + block_scan(mine, s_w, &all);
  const uint64_t c = pl.spec_cpu[k];
  const uint64_t m = (uint64_t)pl.spec_mem[k];
  uint64_t sum_p = 0, used = 0;
#pragma unroll
  for (int j = 0; j < DEPLOY_IPT; ++j) {
    const int64_t i = base + j;
    uint64_t p;
    if constexpr (SPREAD) {
      const bool top = (uint64_t)a[j] >= t;  // the first rem of these rows, in row order, take one more
      p = (top ? t - 1 : (uint64_t)a[j]) + ((top && before < rem) ? 1u : 0u);
      p = Rk == 0 ? 0 : p;
      before += top ? 1u : 0u;
    } else {
      const uint64_t left = Rk > before ? Rk - before : 0;  // first fit in row order
      p = (uint64_t)a[j] < left ? (uint64_t)a[j] : left;
      before += a[j];
    }
    if (i < nd.n) {
      if (p != 0) {  // the sums wrap as the reference's do
        nd.used_cpu[i] += p * c;
        nd.used_mem[i] = (int64_t)((uint64_t)nd.used_mem[i] + p * m);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const uint64_t xr = (uint64_t)pl.spec_x[(int64_t)r * pl.K + k];
          if (xr != 0) {
            int64_t* ux = nd.used_x + (int64_t)r * nd.n + i;
            *ux = (int64_t)((uint64_t)*ux + p * xr);
          }
        }
        nd.pod_count[i] = (int64_t)((uint64_t)nd.pod_count[i] + p);
        sum_p += p;
        used += 1;
      }
      if (rows_out) rows_out[i] = (int64_t)p;
    }
  }
  const uint64_t tp = block_sum(sum_p, s_w);
  const uint64_t tu = block_sum(used, s_w);
  if (threadIdx.x == 0 && tu != 0) {
    atomicAdd(reinterpret_cast<unsigned long long*>(placed) + k, (unsigned long long)tp);
    atomicAdd(reinterpret_cast<unsigned long long*>(nodes_used) + k, (unsigned long long)tu);
  }
}

template <int R, bool SPREAD>
hipError_t launch_step(const DpNodes& nd, const DpPlan& pl, int64_t k, const DeployWork& w,
                       int64_t* placed, int64_t* nodes_used, int32_t* step_err,
                       int64_t* placed_rows, hipStream_t s) {
  const int64_t tiles = deploy_tiles(nd.n);
  const dim3 grid((unsigned)tiles), block(DP_THREADS);
  uint32_t* flag = w.flag + k * DEPLOY_FLAG_STRIDE;
  uint64_t* st = w.st + k * (4 * DEPLOY_ST_WORDS);
  uint64_t* bins = SPREAD ? w.bins + k * DEPLOY_BIN_WORDS : nullptr;
  hipLaunchKernelGGL((dp_rows_kernel<R, SPREAD>), grid, block, 0, s, nd, pl, k, w.a, w.tile_sum, flag,
                     bins);
  if constexpr (SPREAD) {
    for (int round = 1; round < 4; ++round)
      hipLaunchKernelGGL(dp_hist_kernel, grid, block, 0, s, nd.n, round, pl.replicas, k, w.a, st, bins);
    hipLaunchKernelGGL(dp_ind_kernel, grid, block, 0, s, nd.n, pl.replicas, k, w.a, st, bins,
                       w.tile_sum);
  }
  hipLaunchKernelGGL(dp_scan_kernel, dim3(1), block, 0, s, tiles, w.tile_sum, w.tile_off);
  hipLaunchKernelGGL((dp_apply_kernel<R, SPREAD>), grid, block, 0, s, nd, pl, k, w.a, w.tile_off, flag,
                     st, placed, nodes_used, step_err, placed_rows);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_deploy(const FitNodes& fn, int64_t* pod_count, uint64_t* used_cpu, int64_t* used_mem,
                         int64_t* used_x, const uint8_t* eligible, const DeployPlan& plan,
                         const DeployWork& w, int64_t* placed, int64_t* nodes_used,
                         int32_t* step_err, int64_t* placed_rows, hipStream_t s) {
  if (!deploy_sizes_ok(fn, plan.K) || (plan.policy != DEPLOY_PACK && plan.policy != DEPLOY_SPREAD))
    return hipErrorInvalidValue;
  const DpNodes nd{fn.n, fn.alloc_cpu, fn.alloc_mem, fn.alloc_pods, fn.alloc_x, pod_count,
                   used_cpu, used_mem, used_x, fn.group, fn.G, eligible};
  const DpPlan pl{plan.K, plan.spec_cpu, plan.spec_mem, plan.spec_x, plan.replicas, plan.node_cap};
  const bool spread = plan.policy == DEPLOY_SPREAD;
  hipError_t e;
  // the steps' flag words and search states, the bins, and the two outputs the tiles add into
  if ((e = hipMemsetAsync(w.flag, 0, 4 * (size_t)(plan.K * DEPLOY_FLAG_STRIDE), s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(w.st, 0, 8 * (size_t)(plan.K * 4 * DEPLOY_ST_WORDS), s)) != hipSuccess) return e;
  if (spread &&
      (e = hipMemsetAsync(w.bins, 0, 8 * (size_t)(plan.K * DEPLOY_BIN_WORDS), s)) != hipSuccess)
    return e;
  if ((e = hipMemsetAsync(placed, 0, 8 * (size_t)plan.K, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(nodes_used, 0, 8 * (size_t)plan.K, s)) != hipSuccess) return e;
  for (int64_t k = 0; k < plan.K; ++k) {
    e = ext_dispatch(fn.R, [&](auto r) {
      constexpr int RV = decltype(r)::value;
      return spread ? launch_step<RV, true>(nd, pl, k, w, placed, nodes_used, step_err, placed_rows, s)
                    : launch_step<RV, false>(nd, pl, k, w, placed, nodes_used, step_err, placed_rows, s);
    });
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace kcc
