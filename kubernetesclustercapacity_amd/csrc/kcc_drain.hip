// kcc_drain.hip — the pods of drained node rows turned into a rollout plan (kcc_drain;
// DESIGN.md §4.15).  OPT-IN: not the reference's arithmetic.
//
// "These rows go away": the drained rows are left full, the movable pods that ran on them are
// bucketed by request shape (cpu, memory, R extra words) in an open-addressed table, the
// shapes are ranked descending and written as a kcc_deploy plan that kcc::launch_deploy then
// places on the surviving rows.  Launches (none waits for another workgroup; each reads only
// what earlier launches finished):
//   dr_rows        one thread per row: a drained row's state becomes its allocatable amounts;
//                  the drained rows are counted
//   dr_pods<R>     one thread per pod: its row by binary search of the (clamped) CSR offsets;
//                  an evicted pod (drained row, movable) is counted and inserted into the
//                  table.  A slot holds the index of a representative pod, claimed by a
//                  returning compare-and-swap from DR_EMPTY; whoever finds the slot taken
//                  compares its own words with the representative's, read from the pod arrays
//                  (written before the launch, never during it: the claim publishes an index
//                  and nothing else, so no fence is needed and nothing spins), adds to the
//                  slot's count when they are equal and probes the next slot otherwise.  More
//                  claims than max_shapes, or a probe sequence that finds no slot, set the
//                  overflow word
//   dr_plan<R>     one thread per slot: the rank of a claimed slot is the number of claimed
//                  slots with a greater key (keys are distinct: the ranks are a permutation);
//                  the table goes through LDS in chunks of DR_THREADS slots.  The shape
//                  outputs and the deploy plan are written at the rank, zeros and padding
//                  steps (spec (1, 1), 0 replicas) behind the D shapes; on overflow every
//                  shape output is 0 and every step a padding step
//   (kcc::launch_deploy on the plan: the ABI layer, between dr_plan and dr_finish)
//   dr_finish      one workgroup: the steps' placed / nodes_used / step_err masked to j < D
//                  into the shape outputs, their sum and the summary
#include "kcc_internal.h"

namespace kcc {
namespace {

constexpr int DR_THREADS = 256;
constexpr int32_t DR_EMPTY = -1;

template <int R>
struct DrKey {
  uint64_t c;
  int64_t m;
  int64_t x[R ? R : 1];
};

template <int R>
__device__ inline DrKey<R> dr_key(const uint64_t* __restrict__ pod_cpu,
                                  const int64_t* __restrict__ pod_mem,
                                  const int64_t* __restrict__ pod_x, int64_t P, int64_t p) {
  DrKey<R> k;
  k.c = pod_cpu[p];
  k.m = pod_mem[p];
#pragma unroll
  for (int r = 0; r < R; ++r) k.x[r] = pod_x ? pod_x[(int64_t)r * P + p] : 0;
  return k;
}

template <int R>
__device__ inline bool dr_equal(const DrKey<R>& a, const DrKey<R>& b) {
  bool eq = a.c == b.c && a.m == b.m;
#pragma unroll
  for (int r = 0; r < R; ++r) eq = eq && a.x[r] == b.x[r];
  return eq;
}

// a > b, lexicographically: cpu as uint64, every other word as int64
template <int R>
__device__ inline bool dr_greater(const DrKey<R>& a, const DrKey<R>& b) {
  bool gt = false, eq = true;  // over the words so far
  gt = a.c > b.c;
  eq = a.c == b.c;
  gt = gt || (eq && a.m > b.m);
  eq = eq && a.m == b.m;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    gt = gt || (eq && a.x[r] > b.x[r]);
    eq = eq && a.x[r] == b.x[r];
  }
  return gt;
}

__device__ inline uint64_t dr_mix(uint64_t h) {  // splitmix64's finalizer
  h ^= h >> 30;
  h *= 0xbf58476d1ce4e5b9ull;
  h ^= h >> 27;
  h *= 0x94d049bb133111ebull;
  h ^= h >> 31;
  return h;
}

template <int R>
__device__ inline uint32_t dr_hash(const DrKey<R>& k) {
  uint64_t h = dr_mix(k.c + 0x9e3779b97f4a7c15ull);
  h = dr_mix(h ^ (uint64_t)k.m);
#pragma unroll
  for (int r = 0; r < R; ++r) h = dr_mix(h ^ (uint64_t)k.x[r]);
  return (uint32_t)h;
}

// node_pod_ptr[k] clamped into [0, P]: a malformed CSR gives wrong numbers, never a fault
__device__ inline int64_t dr_off(const int64_t* __restrict__ ptr, int64_t k, int64_t P) {
  const int64_t v = ptr[k];
  return v < 0 ? 0 : (v > P ? P : v);
}

__global__ __launch_bounds__(DR_THREADS) void dr_rows_kernel(
    int64_t n, int64_t R, const uint64_t* __restrict__ alloc_cpu,
    const int64_t* __restrict__ alloc_mem, const int64_t* __restrict__ alloc_pods,
    const int64_t* __restrict__ alloc_x, const uint8_t* __restrict__ drain,
    int64_t* __restrict__ pod_count, uint64_t* __restrict__ used_cpu,
    int64_t* __restrict__ used_mem, int64_t* __restrict__ used_x,
    unsigned long long* __restrict__ meta) {
  const int64_t i = (int64_t)blockIdx.x * DR_THREADS + threadIdx.x;
  if (i >= n || drain[i] == 0) return;
  used_cpu[i] = alloc_cpu[i];
  used_mem[i] = alloc_mem[i];
  pod_count[i] = alloc_pods[i];
  for (int64_t r = 0; r < R; ++r) used_x[r * n + i] = alloc_x[r * n + i];
  atomicAdd(meta + DRAIN_META_ROWS, 1ull);  // (one add per wave: the compiler sums the lanes)
}

template <int R>
__global__ __launch_bounds__(DR_THREADS) void dr_pods_kernel(
    int64_t n, int64_t P, const int64_t* __restrict__ node_pod_ptr,
    const uint8_t* __restrict__ drain, const uint64_t* __restrict__ pod_cpu,
    const int64_t* __restrict__ pod_mem, const int64_t* __restrict__ pod_x,
    const uint8_t* __restrict__ movable, int64_t M, uint32_t mask, int32_t* __restrict__ rep,
    uint32_t* __restrict__ cnt, unsigned long long* __restrict__ meta) {
  const int64_t p = (int64_t)blockIdx.x * DR_THREADS + threadIdx.x;
  bool evicted = false;
  if (p < P) {
    // the last row whose first pod is at or before p
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (dr_off(node_pod_ptr, mid, P) <= p) lo = mid;
      else hi = mid;
    }
    evicted = p >= dr_off(node_pod_ptr, lo, P) && p < dr_off(node_pod_ptr, lo + 1, P) &&
              drain[lo] != 0 && (!movable || movable[p] != 0);
  }
  // the workgroup's evicted pods in one add (every thread reaches the barrier)
  const int n_ev = __syncthreads_count(evicted);
  if (threadIdx.x == 0 && n_ev) atomicAdd(meta + DRAIN_META_EVICTED, (unsigned long long)n_ev);
  if (!evicted) return;
  const DrKey<R> key = dr_key<R>(pod_cpu, pod_mem, pod_x, P, p);
  uint32_t h = dr_hash<R>(key) & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    int32_t cur = __hip_atomic_load(rep + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == DR_EMPTY) {
      cur = atomicCAS(rep + h, DR_EMPTY, (int32_t)p);
      if (cur == DR_EMPTY) {  // claimed: this pod represents the slot
        if (atomicAdd(meta + DRAIN_META_CLAIMED, 1ull) >= (unsigned long long)M)
          atomicOr(meta + DRAIN_META_OVERFLOW, 1ull);
        cur = (int32_t)p;
      }
    }
    if (cur == (int32_t)p || dr_equal<R>(key, dr_key<R>(pod_cpu, pod_mem, pod_x, P, cur))) {
      atomicAdd(cnt + h, 1u);
      return;
    }
    h = (h + 1) & mask;
  }
  atomicOr(meta + DRAIN_META_OVERFLOW, 1ull);  // every slot holds another shape
}

template <int R>
__global__ __launch_bounds__(DR_THREADS) void dr_plan_kernel(
    int64_t T, int64_t M, int64_t K, int64_t P, const uint64_t* __restrict__ pod_cpu,
    const int64_t* __restrict__ pod_mem, const int64_t* __restrict__ pod_x,
    const int32_t* __restrict__ rep, const uint32_t* __restrict__ cnt,
    const unsigned long long* __restrict__ meta, uint64_t* __restrict__ shape_cpu,
    int64_t* __restrict__ shape_mem, int64_t* __restrict__ shape_x,
    int64_t* __restrict__ shape_count, uint64_t* __restrict__ plan_cpu,
    int64_t* __restrict__ plan_mem, int64_t* __restrict__ plan_x,
    int64_t* __restrict__ plan_rep) {
  constexpr int RR = R ? R : 1;
  __shared__ int32_t s_rep[DR_THREADS];
  __shared__ uint64_t s_c[DR_THREADS];
  __shared__ int64_t s_m[DR_THREADS];
  __shared__ int64_t s_x[RR][DR_THREADS];
  const int tid = threadIdx.x;
  const int64_t g = (int64_t)blockIdx.x * DR_THREADS + tid;  // < T
  const unsigned long long claimed = meta[DRAIN_META_CLAIMED];
  const bool over = meta[DRAIN_META_OVERFLOW] != 0 || claimed > (unsigned long long)M;
  const int64_t D = over ? 0 : (int64_t)claimed;
  const int32_t mine = rep[g];
  const bool have = !over && mine != DR_EMPTY;
  DrKey<R> key{};
  if (have) key = dr_key<R>(pod_cpu, pod_mem, pod_x, P, mine);
  int64_t rank = 0;
  if (!over) {
    for (int64_t base = 0; base < T; base += DR_THREADS) {
      __syncthreads();
      const int32_t o = rep[base + tid];
      s_rep[tid] = o;
      if (o != DR_EMPTY) {
        const DrKey<R> k = dr_key<R>(pod_cpu, pod_mem, pod_x, P, o);
        s_c[tid] = k.c;
        s_m[tid] = k.m;
#pragma unroll
        for (int r = 0; r < R; ++r) s_x[r][tid] = k.x[r];
      }
      __syncthreads();
      if (have) {
        for (int j = 0; j < DR_THREADS; ++j) {
          if (s_rep[j] == DR_EMPTY) continue;
          DrKey<R> k;
          k.c = s_c[j];
          k.m = s_m[j];
#pragma unroll
          for (int r = 0; r < R; ++r) k.x[r] = s_x[r][j];
          rank += dr_greater<R>(k, key) ? 1 : 0;
        }
      }
    }
  }
  if (have) {  // rank < D <= min(M, K)
    const int64_t c = (int64_t)cnt[g];
    shape_cpu[rank] = key.c;
    shape_mem[rank] = key.m;
    shape_count[rank] = c;
    plan_cpu[rank] = key.c;
    plan_mem[rank] = key.m;
    plan_rep[rank] = c;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      shape_x[(int64_t)r * M + rank] = key.x[r];
      plan_x[(int64_t)r * K + rank] = key.x[r];
    }
  }
  if (g >= D && g < M) {  // behind the shapes: zeros, and the padding steps
    shape_cpu[g] = 0;
    shape_mem[g] = 0;
    shape_count[g] = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) shape_x[(int64_t)r * M + g] = 0;
    if (g < K) {
      plan_cpu[g] = 1;
      plan_mem[g] = 1;
      plan_rep[g] = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) plan_x[(int64_t)r * K + g] = 0;
    }
  }
}

__global__ __launch_bounds__(DR_THREADS) void dr_finish_kernel(
    int64_t M, const unsigned long long* __restrict__ meta, const int64_t* __restrict__ placed,
    const int64_t* __restrict__ nodes_used, const int32_t* __restrict__ step_err,
    int64_t* __restrict__ shape_placed, int64_t* __restrict__ shape_nodes,
    int32_t* __restrict__ shape_err, int64_t* __restrict__ summary) {
  __shared__ unsigned long long s_sum;
  const unsigned long long claimed = meta[DRAIN_META_CLAIMED];
  const bool over = meta[DRAIN_META_OVERFLOW] != 0 || claimed > (unsigned long long)M;
  const int64_t D = over ? 0 : (int64_t)claimed;
  if (threadIdx.x == 0) s_sum = 0;
  __syncthreads();
  unsigned long long sum = 0;
  for (int64_t j = threadIdx.x; j < M; j += DR_THREADS) {
    const bool live = j < D;  // (the steps behind D are padding, or were not run)
    const int64_t pl = live ? placed[j] : 0;
    shape_placed[j] = pl;
    shape_nodes[j] = live ? nodes_used[j] : 0;
    shape_err[j] = live ? step_err[j] : 0;
    sum += (unsigned long long)pl;
  }
  atomicAdd(&s_sum, sum);
  __syncthreads();
  if (threadIdx.x == 0) {
    summary[0] = (int64_t)meta[DRAIN_META_ROWS];
    summary[1] = (int64_t)meta[DRAIN_META_EVICTED];
    summary[2] = over ? -1 : D;
    summary[3] = (int64_t)s_sum;
  }
}

inline unsigned dr_grid(int64_t n) { return (unsigned)((n + DR_THREADS - 1) / DR_THREADS); }

}  // namespace

hipError_t launch_drain_scan(const FitNodes& nd, int64_t* pod_count, uint64_t* used_cpu,
                             int64_t* used_mem, int64_t* used_x, const uint8_t* drain,
                             const DrainPods& pods, int64_t max_shapes, const DrainWork& w,
                             hipStream_t s) {
  if (nd.n <= 0 || nd.n > GRP_MAX_NODES || nd.R < 0 || nd.R > EXT_MAX || pods.P < 0 ||
      pods.P > DRAIN_MAX_PODS || max_shapes < 1 || max_shapes > DRAIN_MAX_SHAPES)
    return hipErrorInvalidValue;
  const int64_t T = drain_table(max_shapes);
  hipError_t e;
  if ((e = hipMemsetAsync(w.rep, 0xff, 4 * (size_t)T, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(w.cnt, 0, 4 * (size_t)T, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(w.meta, 0, 8 * DRAIN_META_WORDS, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(dr_rows_kernel, dim3(dr_grid(nd.n)), dim3(DR_THREADS), 0, s, nd.n, nd.R,
                     nd.alloc_cpu, nd.alloc_mem, nd.alloc_pods, nd.alloc_x, drain, pod_count,
                     used_cpu, used_mem, used_x, w.meta);
  if (pods.P > 0) {
    e = ext_dispatch(nd.R, [&](auto r) {
      constexpr int RV = decltype(r)::value;
      hipLaunchKernelGGL(dr_pods_kernel<RV>, dim3(dr_grid(pods.P)), dim3(DR_THREADS), 0, s, nd.n,
                         pods.P, pods.node_pod_ptr, drain, pods.pod_cpu, pods.pod_mem, pods.pod_x,
                         pods.movable, max_shapes, (uint32_t)(T - 1), w.rep, w.cnt, w.meta);
      return hipSuccess;
    });
    if (e != hipSuccess) return e;
  }
  return hipGetLastError();
}

hipError_t launch_drain_plan(int64_t R, const DrainPods& pods, int64_t max_shapes, int64_t K,
                             const DrainWork& w, const DrainOut& out, hipStream_t s) {
  if (max_shapes < 1 || max_shapes > DRAIN_MAX_SHAPES || K < 0 || K > max_shapes)
    return hipErrorInvalidValue;
  const int64_t T = drain_table(max_shapes);
  const hipError_t e = ext_dispatch(R, [&](auto r) {
    constexpr int RV = decltype(r)::value;
    hipLaunchKernelGGL(dr_plan_kernel<RV>, dim3((unsigned)(T / DR_THREADS)), dim3(DR_THREADS), 0, s,
                       T, max_shapes, K, pods.P, pods.pod_cpu, pods.pod_mem, pods.pod_x, w.rep,
                       w.cnt, w.meta, out.shape_cpu, out.shape_mem, out.shape_x, out.shape_count,
                       w.plan_cpu, w.plan_mem, w.plan_x, w.plan_rep);
    return hipSuccess;
  });
  return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_drain_finish(int64_t max_shapes, const DrainWork& w, const DrainOut& out,
                               hipStream_t s) {
  hipLaunchKernelGGL(dr_finish_kernel, dim3(1), dim3(DR_THREADS), 0, s, max_shapes, w.meta, w.placed,
                     w.nodes_used, w.step_err, out.shape_placed, out.shape_nodes, out.shape_err,
                     out.summary);
  return hipGetLastError();
}

}  // namespace kcc
