// kcc_consolidate.hip — "which of these nodes could I remove?": each candidate row's movable
// pods re-placed on the rest of the cluster as it stands (kcc_consolidate).
// OPT-IN: not the reference's arithmetic.
//
// The what-ifs are independent: one workgroup per candidate, the node state read only.  The
// workgroup takes its candidate's evicted pods in order; each is one kcc_deploy step of one
// replica under KCC_DEPLOY_PACK, i.e. the pod goes to the first eligible row in row order whose
// count a_i (deploy_row_q, kcc_internal.h: the one copy of the step arithmetic) is at least 1.
//   the walk     rows in chunks of CONS_CHUNK (CONS_THREADS threads x CONS_IPT rows, CONS_THREADS
//                apart: a wave's loads are contiguous); a thread evaluates its rows on the base
//                state plus the overlay, a 64-bit ballot per row slice gives the wave's first
//                hit, the waves' firsts go through LDS (two buffers, one barrier per chunk) and
//                every thread takes their minimum; the walk stops at the first chunk with a hit
//   the overlay  the rows this candidate has placed pods on (at most CONS_MAX_PODS) with the
//                sums of what it placed there, in LDS: accumulator slots in the order of first
//                touch, found through an open-addressed table of 2 x CONS_MAX_PODS uint16 slot
//                numbers keyed by the row (linear probing at a load of at most 1/2).  Thread 0
//                inserts and adds, a barrier publishes it to the next pod's walk
//   the shortcut a pod whose shape equals the previously tried pod's is not placed if that one
//                was not, and else starts its walk at that pod's row: the rows before it are
//                unchanged since a walk found a_i = 0 there
// Nothing here waits on another workgroup; duplicates of a candidate write the same values.
#include "kcc_internal.h"

namespace kcc {
namespace {

constexpr int CS_WAVES = CONS_THREADS / 64;
constexpr int CS_SLOTS = 2 * CONS_MAX_PODS;  // the table: a power of two
constexpr int32_t CS_NONE = 0x7fffffff;
static_assert(CONS_MAX_PODS < 65535, "the table holds slot numbers + 1 as uint16");

// node_pod_ptr[k] clamped into [0, P]: a malformed CSR gives wrong numbers, never a fault
__device__ inline int64_t cs_off(const int64_t* __restrict__ ptr, int64_t k, int64_t P) {
  const int64_t v = ptr[k];
  return v < 0 ? 0 : (v > P ? P : v);
}

__device__ inline uint32_t cs_hash(int32_t row) {
  return ((uint32_t)row * 0x9e3779b1u) >> (32 - 11);
}
static_assert(CS_SLOTS == 1 << 11, "cs_hash keeps 11 bits");

template <int R>
struct CsOverlay {
  uint16_t tab[CS_SLOTS];      // slot number + 1 of the row hashed here (0: empty)
  int32_t row[CONS_MAX_PODS];  // by slot: the row,
  uint32_t cnt[CONS_MAX_PODS];  //          the pods placed on it
  uint64_t cpu[CONS_MAX_PODS];  //          and their summed requests (wrapping)
  uint64_t mem[CONS_MAX_PODS];
  uint64_t x[R ? R : 1][CONS_MAX_PODS];
};

// the slot of `row`, or -1
template <int R>
__device__ inline int cs_find(const CsOverlay<R>& ov, int32_t row) {
  uint32_t h = cs_hash(row);
  for (;;) {  // ends: at most CONS_MAX_PODS of the CS_SLOTS entries are taken
    const uint32_t e = ov.tab[h];
    if (e == 0) return -1;
    if (ov.row[e - 1] == row) return (int)e - 1;
    h = (h + 1) & (CS_SLOTS - 1);
  }
}

template <int R>
__global__ __launch_bounds__(CONS_THREADS) void cs_walk_kernel(
    int64_t n, const uint64_t* __restrict__ alloc_cpu, const int64_t* __restrict__ alloc_mem,
    const int64_t* __restrict__ alloc_pods, const int64_t* __restrict__ alloc_x,
    const int64_t* __restrict__ pod_count, const uint64_t* __restrict__ used_cpu,
    const int64_t* __restrict__ used_mem, const int64_t* __restrict__ used_x,
    const uint8_t* __restrict__ target, int64_t P, const int64_t* __restrict__ node_pod_ptr,
    const uint64_t* __restrict__ pod_cpu, const int64_t* __restrict__ pod_mem,
    const int64_t* __restrict__ pod_x, const uint8_t* __restrict__ movable,
    const int64_t* __restrict__ cand, int64_t* __restrict__ cand_evicted,
    int64_t* __restrict__ cand_placed, int64_t* __restrict__ cand_zero,
    int32_t* __restrict__ cand_err, int64_t* __restrict__ pod_target) {
  constexpr int RR = R ? R : 1;
  __shared__ CsOverlay<R> ov;
  __shared__ int32_t s_first[2][CS_WAVES];
  __shared__ int s_touched;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t j = blockIdx.x;
  const int64_t c_row = cand[j];
  if (c_row < 0 || c_row >= n) {  // (uniform over the workgroup)
    if (tid == 0) {
      cand_evicted[j] = 0;
      cand_placed[j] = 0;
      cand_zero[j] = 0;
      cand_err[j] = CAND_BADROW;
    }
    return;
  }
  const int64_t lo = cs_off(node_pod_ptr, c_row, P);
  int64_t hi = cs_off(node_pod_ptr, c_row + 1, P);
  hi = hi < lo ? lo : hi;
  int64_t evicted = hi - lo;
  if (movable) {
    evicted = 0;
    for (int64_t b = lo; b < hi; b += CONS_THREADS)
      evicted += __syncthreads_count(b + tid < hi && movable[b + tid] != 0);
  }
  if (evicted > CONS_MAX_PODS) {
    if (tid == 0) {
      cand_evicted[j] = evicted;
      cand_placed[j] = 0;
      cand_zero[j] = 0;
      cand_err[j] = CAND_TOOMANY;
    }
    return;
  }
  for (int k = tid; k < CS_SLOTS; k += CONS_THREADS) ov.tab[k] = 0;
  __syncthreads();

  int touched = 0;  // overlay slots in use (every thread keeps the count: the walk is uniform)
  int64_t placed = 0, zero = 0;
  bool have_prev = false;
  uint64_t prev_c = 0;
  int64_t prev_m = 0, prev_x[RR] = {}, prev_row = -1;
  unsigned it = 0;  // chunks walked so far: the parity picks s_first's buffer
  for (int64_t p = lo; p < hi; ++p) {
    if (movable && movable[p] == 0) continue;  // goes away with its node
    const uint64_t c = pod_cpu[p];
    const int64_t m = pod_mem[p];
    int64_t x[RR] = {};
#pragma unroll
    for (int r = 0; r < R; ++r) x[r] = pod_x ? pod_x[(int64_t)r * P + p] : 0;
    if (c == 0 || m == 0) {  // not tried: no row pass, the state untouched
      ++zero;
      if (tid == 0 && pod_target) pod_target[p] = -3;
      continue;
    }
    bool same = have_prev && c == prev_c && m == prev_m;
#pragma unroll
    for (int r = 0; r < R; ++r) same = same && x[r] == prev_x[r];
    int64_t found = -1;
    if (!same || prev_row >= 0) {
      const int64_t start = same ? prev_row : 0;
      for (int64_t base = start - start % CONS_CHUNK; base < n; base += CONS_CHUNK, ++it) {
        uint64_t ac[CONS_IPT], uc[CONS_IPT];
        int64_t am[CONS_IPT], um[CONS_IPT], ap[CONS_IPT], pc[CONS_IPT];
        bool el[CONS_IPT];
#pragma unroll
        for (int q = 0; q < CONS_IPT; ++q) {  // the loads of the thread's rows, all in flight
          const int64_t i = base + q * CONS_THREADS + tid;
          el[q] = i < n && i >= start && i != c_row && (!target || target[i] != 0);
          const int64_t k = i < n ? i : n - 1;
          ac[q] = alloc_cpu[k];
          uc[q] = used_cpu[k];
          am[q] = alloc_mem[k];
          um[q] = used_mem[k];
          ap[q] = alloc_pods[k];
          pc[q] = pod_count[k];
        }
        int32_t first = CS_NONE;
#pragma unroll
        for (int q = 0; q < CONS_IPT; ++q) {
          const int64_t i = base + q * CONS_THREADS + tid;
          bool hit = false;
          if (el[q]) {
            const int slot = touched ? cs_find<R>(ov, (int32_t)i) : -1;
            if (slot >= 0) {  // kcc_deploy's commits of this candidate's earlier pods
              uc[q] += ov.cpu[slot];
              um[q] = (int64_t)((uint64_t)um[q] + ov.mem[slot]);
              pc[q] = (int64_t)((uint64_t)pc[q] + ov.cnt[slot]);
            }
            bool z;
            const int64_t a = deploy_row_q<R>(
                ac[q], uc[q], am[q], um[q], ap[q], pc[q], c, m, x,
                [&](int r, int64_t& ax, int64_t& ux) {
                  ax = alloc_x[(int64_t)r * n + i];
                  ux = used_x[(int64_t)r * n + i];
                  if (slot >= 0) ux = (int64_t)((uint64_t)ux + ov.x[r][slot]);
                },
                z);
            hit = a >= 1;  // (z is false: c and m are not zero)
          }
          const unsigned long long b = __ballot(hit);
          if (b != 0 && first == CS_NONE)
            first = (int32_t)(base + q * CONS_THREADS + wave * 64) + __builtin_ctzll(b);
        }
        if (lane == 0) s_first[it & 1][wave] = first;
        __syncthreads();
        int32_t best = CS_NONE;
#pragma unroll
        for (int w = 0; w < CS_WAVES; ++w) {
          const int32_t f = s_first[it & 1][w];
          best = f < best ? f : best;
        }
        if (best != CS_NONE) {
          found = best;
          ++it;
          break;
        }
      }
    }
    if (found >= 0) {  // (uniform) the commit with p_i = 1, into the overlay
      if (tid == 0) {
        int slot = touched ? cs_find<R>(ov, (int32_t)found) : -1;
        s_touched = slot < 0 ? touched + 1 : touched;
        if (slot < 0) {  // touched < CONS_MAX_PODS: one new slot per placed pod at most
          slot = touched;
          ov.row[slot] = (int32_t)found;
          ov.cnt[slot] = 0;
          ov.cpu[slot] = 0;
          ov.mem[slot] = 0;
#pragma unroll
          for (int r = 0; r < R; ++r) ov.x[r][slot] = 0;
          uint32_t h = cs_hash((int32_t)found);
          while (ov.tab[h] != 0) h = (h + 1) & (CS_SLOTS - 1);
          ov.tab[h] = (uint16_t)(slot + 1);
        }
        ov.cnt[slot] += 1;
        ov.cpu[slot] += c;
        ov.mem[slot] += (uint64_t)m;
#pragma unroll
        for (int r = 0; r < R; ++r) ov.x[r][slot] += (uint64_t)x[r];
        if (pod_target) pod_target[p] = found;
      }
      ++placed;
      // the overlay's new contents, and its slot count, before the next walk reads them (thread
      // 0 writes s_touched again only behind a later walk's barrier)
      __syncthreads();
      touched = s_touched;
    } else if (tid == 0 && pod_target) {
      pod_target[p] = -1;
    }
    have_prev = true;
    prev_c = c;
    prev_m = m;
#pragma unroll
    for (int r = 0; r < R; ++r) prev_x[r] = x[r];
    prev_row = found;
  }
  if (tid == 0) {
    cand_evicted[j] = evicted;
    cand_placed[j] = placed;
    cand_zero[j] = zero;
    cand_err[j] = CAND_OK;
  }
}

}  // namespace

hipError_t launch_consolidate(const FitNodes& nd, const uint8_t* target, const DrainPods& pods,
                              int64_t C, const int64_t* cand, const ConsOut& out, hipStream_t s) {
  if (nd.n <= 0 || nd.n > GRP_MAX_NODES || nd.R < 0 || nd.R > EXT_MAX || pods.P < 0 ||
      pods.P > DRAIN_MAX_PODS || C <= 0 || C > CONS_MAX_CAND)
    return hipErrorInvalidValue;
  hipError_t e;
  if (out.pod_target && pods.P > 0 &&
      (e = launch_fill_i64(pods.P, -2, out.pod_target, s)) != hipSuccess)
    return e;
  e = ext_dispatch(nd.R, [&](auto r) {
    constexpr int RV = decltype(r)::value;
    hipLaunchKernelGGL(cs_walk_kernel<RV>, dim3((unsigned)C), dim3(CONS_THREADS), 0, s, nd.n,
                       nd.alloc_cpu, nd.alloc_mem, nd.alloc_pods, nd.alloc_x, nd.pod_count,
                       nd.used_cpu, nd.used_mem, nd.used_x, target, pods.P, pods.node_pod_ptr,
                       pods.pod_cpu, pods.pod_mem, pods.pod_x, pods.movable, cand, out.evicted,
                       out.placed, out.zero, out.err, out.pod_target);
    return hipSuccess;
  });
  return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace kcc
