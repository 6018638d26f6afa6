// kcc_levels.hip — preemption what-if (kcc_reduce_requests_levels, kcc_fit_levels; DESIGN.md
// §4.14).  OPT-IN: not the reference's arithmetic.
//
// The node state per priority level: plane l of used_cpu / used_mem / pod_count [L, N] holds
// the pods a spec of level l cannot evict (pod_level >= l), so plane 0 is every pod and each
// plane is the suffix sum, top level down, of the pods of exactly that level.  The suffix sum
// is linear, so every partial sum of a node is turned into its L suffix sums in registers
// before it leaves the workgroup: no [L, N] pass follows the stream.
//
//   levels_reduce   one lane per pod, 256 pods a tile, LV_TILES_MAX consecutive tiles a
//                   workgroup.  A lane sums its pod's containers (loads batched as
//                   pod_requests_kernel's), finds its node in a window of node_pod_ptr staged in
//                   LDS (a global binary search beyond it) and adds into LDS bins
//                   [level][rank of the node within the tile].  A thread per rank then writes
//                   the node's suffix sums with plain stores; the tile's last node is carried
//                   in LDS into the next tile, and only the workgroup's first and last node —
//                   the ones another workgroup may share — go out as 64-bit atomic adds onto
//                   the zeroed outputs (wrapping adds commute: bit-exact).  A node of any length
//                   is spread over lanes and tiles like any other run of pods.
//   cells_pack_x    spec_x [R, S] to one [R, S_l] block per level (the pair loop strides by S)
//   cells_place     a level's [G, S_l] cells to columns level_ptr[l].. of the [G, S] outputs
// No kernel waits on another workgroup: none sets or reads the fault words.
#include "kcc_internal.h"

namespace kcc {
namespace {

constexpr int LV_BATCH = 4;  // containers loaded per round trip (POD_BATCH of kcc_pods.hip)

struct LvCarry {  // thread 0's view of the node carried from the previous tile
  bool valid;
  bool shared;  // it is the workgroup's first node: another workgroup may hold pods of it
  int64_t node;
};

// Column `col` (stride `stride`) of exact-level sums to node's L suffix sums, top level down.
template <bool ATOMIC>
__device__ __forceinline__ void lv_emit(int L, int64_t N, int64_t node,
                                        const unsigned long long* bc, const unsigned long long* bm,
                                        const uint32_t* bn, int col, int stride,
                                        uint64_t* __restrict__ used_cpu,
                                        int64_t* __restrict__ used_mem,
                                        int64_t* __restrict__ pod_count) {
  unsigned long long ac = 0, am = 0, an = 0;
  for (int l = L - 1; l >= 0; --l) {
    ac += bc[l * stride + col];
    am += bm[l * stride + col];
    an += bn[l * stride + col];
    const int64_t o = (int64_t)l * N + node;
    if (ATOMIC) {
      atomicAdd(reinterpret_cast<unsigned long long*>(used_cpu) + o, ac);
      atomicAdd(reinterpret_cast<unsigned long long*>(used_mem) + o, am);
      atomicAdd(reinterpret_cast<unsigned long long*>(pod_count) + o, an);
    } else {
      used_cpu[o] = ac;
      used_mem[o] = (int64_t)am;
      pod_count[o] = (int64_t)an;
    }
  }
}

// Dynamic LDS: bc [L][LV_WG] u64, bm [L][LV_WG] u64, bn [L][LV_WG] u32 (zero between tiles).
__global__ __launch_bounds__(LV_WG) void levels_reduce_kernel(
    int64_t N, int64_t n_pods, int64_t n_cont, int L, int tiles_per_wg,
    const int64_t* __restrict__ node_pod_ptr, const int64_t* __restrict__ pod_ptr,
    const uint64_t* __restrict__ cpu_req, const int64_t* __restrict__ mem_req,
    const uint8_t* __restrict__ pod_level, uint64_t* __restrict__ used_cpu,
    int64_t* __restrict__ used_mem, int64_t* __restrict__ pod_count) {
  extern __shared__ unsigned long long lv_lds[];
  unsigned long long* const bc = lv_lds;
  unsigned long long* const bm = bc + L * LV_WG;
  uint32_t* const bn = reinterpret_cast<uint32_t*>(bm + L * LV_WG);
  __shared__ int64_t win[LV_WG + 1];     // node_pod_ptr[n0 .. n0 + LV_WG], INT64_MAX from N on
  __shared__ int64_t rank_node[LV_WG];   // the node of each rank of the tile
  __shared__ unsigned long long cc[LEVELS_MAX], cm[LEVELS_MAX];  // the carried node's sums
  __shared__ uint32_t cn[LEVELS_MAX];
  __shared__ int wave_heads[LV_WG / 64];
  __shared__ int64_t next_n0;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int l = 0; l < L; ++l) {
    bc[l * LV_WG + tid] = 0;
    bm[l * LV_WG + tid] = 0;
    bn[l * LV_WG + tid] = 0;
  }
  const int64_t wg_p0 = (int64_t)blockIdx.x * tiles_per_wg * LV_WG;
  // the node of the workgroup's first pod: the largest i in [0, N) with node_pod_ptr[i] <= p
  int64_t n0 = 0;
  {
    int64_t hi = N;
    while (hi - n0 > 1) {
      const int64_t mid = n0 + ((hi - n0) >> 1);
      if (node_pod_ptr[mid] <= wg_p0) n0 = mid; else hi = mid;
    }
  }
  LvCarry carry{false, false, 0};  // thread 0's alone

  for (int t = 0; t < tiles_per_wg; ++t) {
    const int64_t p0 = wg_p0 + (int64_t)t * LV_WG;
    if (p0 >= n_pods) break;  // (uniform)
    const int64_t p = p0 + tid;
    const bool live = p < n_pods;
    // the window of node offsets from the tile's first node on
    for (int j = tid; j <= LV_WG; j += LV_WG) win[j] = n0 + j < N ? node_pod_ptr[n0 + j] : INT64_MAX;
    // the pod's containers (offsets clamped: a malformed CSR gives wrong sums, never a fault)
    uint64_t sc = 0, sm = 0;
    int lvl = 0;
    if (live) {
      int64_t lo = pod_ptr[p], hi = pod_ptr[p + 1];
      lo = lo < 0 ? 0 : (lo > n_cont ? n_cont : lo);
      hi = hi < lo ? lo : (hi > n_cont ? n_cont : hi);
      lvl = pod_level[p];
      lvl = lvl >= L ? L - 1 : lvl;
      for (int64_t c = lo; c < hi; c += LV_BATCH) {
        uint64_t vc[LV_BATCH], vm[LV_BATCH];
#pragma unroll
        for (int u = 0; u < LV_BATCH; ++u) {
          vc[u] = 0;
          vm[u] = 0;
          if (c + u < hi) {
            vc[u] = cpu_req[c + u];
            vm[u] = (uint64_t)mem_req[c + u];
          }
        }
#pragma unroll
        for (int u = 0; u < LV_BATCH; ++u) {
          sc += vc[u];
          sm += vm[u];
        }
      }
    }
    __syncthreads();  // win is staged; the bins are zero
    // the pod's node: the largest j in [0, LV_WG) with win[j] <= p, or beyond the window
    int64_t node = n0;
    bool head = false;
    if (live) {
      int j = 0;
#pragma unroll
      for (int step = LV_WG / 2; step > 0; step >>= 1)
        if (win[j + step] <= p) j += step;
      node = n0 + j;
      int64_t first = win[j];
      if (win[LV_WG] <= p) {  // more than LV_WG nodes (empty ones) within the tile
        int64_t a = n0 + LV_WG, b = N;
        while (b - a > 1) {
          const int64_t mid = a + ((b - a) >> 1);
          if (node_pod_ptr[mid] <= p) a = mid; else b = mid;
        }
        node = a;
        first = node_pod_ptr[a];
      }
      head = tid == 0 || first == p;  // the first pod of its node, or of the tile
    }
    const unsigned long long hb = __ballot(head);
    if (lane == 0) wave_heads[wave] = __popcll(hb);
    if (tid == LV_WG - 1) next_n0 = node;  // (a tile cut short by n_pods is the last one)
    __syncthreads();
    int rank = __popcll(hb & ((2ull << lane) - 1)) - 1, nr = 0;
#pragma unroll
    for (int w = 0; w < LV_WG / 64; ++w) {
      rank += w < wave ? wave_heads[w] : 0;
      nr += wave_heads[w];
    }
    if (live) {
      rank = rank < 0 ? 0 : rank;  // (a wave without a head before this lane: malformed offsets)
      if (head) rank_node[rank] = node;
      atomicAdd(&bc[lvl * LV_WG + rank], (unsigned long long)sc);
      atomicAdd(&bm[lvl * LV_WG + rank], (unsigned long long)sm);
      atomicAdd(&bn[lvl * LV_WG + rank], 1u);
    }
    n0 = next_n0;
    __syncthreads();  // the bins and rank_node are complete
    if (tid == 0) {
      bool shared0 = true;  // no carry: rank 0 is the workgroup's first node
      if (carry.valid) {
        if (carry.node == rank_node[0]) {  // the carried node goes on in this tile
          for (int l = 0; l < L; ++l) {
            bc[l * LV_WG] += cc[l];
            bm[l * LV_WG] += cm[l];
            bn[l * LV_WG] += cn[l];
          }
          shared0 = carry.shared;
        } else {  // it ended with the previous tile
          if (carry.shared)
            lv_emit<true>(L, N, carry.node, cc, cm, cn, 0, 1, used_cpu, used_mem, pod_count);
          else
            lv_emit<false>(L, N, carry.node, cc, cm, cn, 0, 1, used_cpu, used_mem, pod_count);
          shared0 = false;
        }
      }
      if (nr > 1) {
        if (shared0)
          lv_emit<true>(L, N, rank_node[0], bc, bm, bn, 0, LV_WG, used_cpu, used_mem, pod_count);
        else
          lv_emit<false>(L, N, rank_node[0], bc, bm, bn, 0, LV_WG, used_cpu, used_mem, pod_count);
      }
      // the tile's last node may go on in the next tile
      for (int l = 0; l < L; ++l) {
        cc[l] = bc[l * LV_WG + nr - 1];
        cm[l] = bm[l * LV_WG + nr - 1];
        cn[l] = bn[l * LV_WG + nr - 1];
      }
      carry = LvCarry{true, nr > 1 ? false : shared0, rank_node[nr - 1]};
    } else if (tid < nr - 1) {  // a node that begins and ends within the tile
      lv_emit<false>(L, N, rank_node[tid], bc, bm, bn, tid, LV_WG, used_cpu, used_mem, pod_count);
    }
    __syncthreads();  // the columns are read
    if (tid < nr) {
      for (int l = 0; l < L; ++l) {
        bc[l * LV_WG + tid] = 0;
        bm[l * LV_WG + tid] = 0;
        bn[l * LV_WG + tid] = 0;
      }
    }
  }
  // the workgroup's last node: the next workgroup may go on with it
  if (tid == 0 && carry.valid)
    lv_emit<true>(L, N, carry.node, cc, cm, cn, 0, 1, used_cpu, used_mem, pod_count);
}

__global__ __launch_bounds__(256) void cells_pack_x_kernel(int64_t R, int64_t S, LevelPtr lp,
                                                          const int64_t* __restrict__ spec_x,
                                                          int64_t* __restrict__ packed) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= R * S) return;
  const int64_t r = k / S, s = k - r * S;
  int l = 0;
  while (l + 1 < lp.L && s >= lp.ptr[l + 1]) ++l;
  const int64_t o = lp.ptr[l], Sl = lp.ptr[l + 1] - o;
  packed[R * o + r * Sl + (s - o)] = spec_x[k];
}

__global__ __launch_bounds__(256) void cells_place_kernel(int64_t G, int64_t S, int64_t Sl,
                                                         int64_t col0,
                                                         const int64_t* __restrict__ cell_tot,
                                                         const int32_t* __restrict__ cell_err,
                                                         int64_t* __restrict__ totals,
                                                         int32_t* __restrict__ spec_err) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= G * Sl) return;
  const int64_t g = k / Sl, s = k - g * Sl;
  totals[g * S + col0 + s] = cell_tot[k];
  spec_err[g * S + col0 + s] = cell_err[k];
}

}  // namespace

hipError_t launch_levels_reduce(int64_t N, int64_t n_pods, int64_t n_cont, int L,
                                const int64_t* node_pod_ptr, const int64_t* pod_ptr,
                                const uint64_t* cpu_req, const int64_t* mem_req,
                                const uint8_t* pod_level, uint64_t* used_cpu, int64_t* used_mem,
                                int64_t* pod_count, hipStream_t s) {
  if (N <= 0) return hipSuccess;
  if (L < 1 || L > LEVELS_MAX || n_pods < 0) return hipErrorInvalidValue;
  const size_t plane = (size_t)L * (size_t)N;
  hipError_t e;
  if ((e = hipMemsetAsync(used_cpu, 0, 8 * plane, s)) != hipSuccess ||
      (e = hipMemsetAsync(used_mem, 0, 8 * plane, s)) != hipSuccess ||
      (e = hipMemsetAsync(pod_count, 0, 8 * plane, s)) != hipSuccess)
    return e;
  if (n_pods == 0) return hipSuccess;
  const int64_t tiles = (n_pods + LV_WG - 1) / LV_WG;
  int64_t k = tiles / LV_MIN_GRID;  // tiles a workgroup: fewer shared nodes, a grid that still fills the chip
  k = k < 1 ? 1 : (k > LV_TILES_MAX ? LV_TILES_MAX : k);
  const int64_t grid = (tiles + k - 1) / k;
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  const size_t lds = (size_t)L * LV_WG * (8 + 8 + 4);
  hipLaunchKernelGGL(levels_reduce_kernel, dim3((unsigned)grid), dim3(LV_WG), lds, s, N, n_pods,
                     n_cont, L, (int)k, node_pod_ptr, pod_ptr, cpu_req, mem_req, pod_level,
                     used_cpu, used_mem, pod_count);
  return hipGetLastError();
}

hipError_t launch_cells_pack_x(int64_t R, int64_t S, const LevelPtr& lp, const int64_t* spec_x,
                               int64_t* packed, hipStream_t s) {
  if (R <= 0 || S <= 0) return hipSuccess;
  hipLaunchKernelGGL(cells_pack_x_kernel, dim3((unsigned)((R * S + 255) / 256)), dim3(256), 0, s, R,
                     S, lp, spec_x, packed);
  return hipGetLastError();
}

hipError_t launch_cells_place(int64_t G, int64_t S, int64_t Sl, int64_t col0,
                              const int64_t* cell_tot, const int32_t* cell_err, int64_t* totals,
                              int32_t* spec_err, hipStream_t s) {
  if (G <= 0 || Sl <= 0) return hipSuccess;
  hipLaunchKernelGGL(cells_place_kernel, dim3((unsigned)((G * Sl + 255) / 256)), dim3(256), 0, s, G,
                     S, Sl, col0, cell_tot, cell_err, totals, spec_err);
  return hipGetLastError();
}

}  // namespace kcc
