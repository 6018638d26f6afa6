// kcc_internal.h — launch interface between the C-ABI layer (kcc_abi.cpp) and the
// gfx950 kernels (kcc_kernels.hip).  Internal: not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

// Diagnostic knobs produce wrong results by design (no stores, loads only), add stamp
// stores, or make every bounded wait give up (the fault-path test build): only experiment
// builds (csrc/Makefile `variant` / `faultdiag`, which define KCC_VARIANT_BUILD and write a
// separate .so) may set them.  The tuning choices are constants here: the variants that
// lost their A/B were deleted (DESIGN.md §10 lists them with their numbers and commits).
#if !defined(KCC_VARIANT_BUILD) &&                                                       \
    (defined(KCC_DIAG_RED_NOSTORE) || defined(KCC_DIAG_RED_LOADONLY) ||                  \
     defined(KCC_TIMELINE) || defined(KCC_DIAG_RED_GIVEUP) || defined(KCC_DIAG_P2P_GIVEUP) || \
     defined(KCC_DIAG_INLIB_COMM) || defined(KCC_DIAG_GA_NOATOM) ||                     \
     defined(KCC_DIAG_NP_NOSC1))
#error "a diagnostic KCC_* knob in a release build: use `make variant` (KCC_VARIANT_BUILD)"
#endif

namespace kcc {

struct RankArgs;   // below: spec ranks, run as extra workgroups of a reduce launch
struct NpArgs;     // below: node prep (clamp in the fit) behind a reduce launch's workgroups

// ---- (a) segmented request reduce -------------------------------------------
// One wavefront owns a contiguous range of reduce_range() containers and walks it in
// tiles of RED_TILE (RED_IPL containers per lane: two 16-B loads per lane per array).
// The launch is self-contained (no marking pass, no zeroing, no atomics): a wave finds
// the node owning its first container by a 64-ary search of the CSR offsets, stores
// every node that ends inside its range, and a node cut by range boundaries is
// assembled by the wave where it ends from the pieces its predecessors publish
// (decoupled look-back over per-wave tail records: each record is published at most once
// per launch and consumed by exactly one wave, which clears its tag — every tag is 0
// between launches, so nothing in the launch depends on host state and a captured graph
// replays correctly).
// tiles in flight ahead of the one being reduced (1-6 measured equal: ping-pong)
constexpr int RED_PREFETCH = 1;
// containers per lane per tile: 8 halves the per-tile work (scan, node walk, stores) per
// container against 4, at 125 VGPRs (4 waves per SIMD instead of 6): C4 reduce 136.4 ->
// 131.1 us, 8-way shard 20.2 -> 19.5 us (A/B in one process, outputs identical)
constexpr int RED_IPL = 8;
constexpr int RED_TILE = 64 * RED_IPL;  // 512
constexpr int RED_WAVES_PER_BLOCK = 4;
// the reduce stores through 32-bit buffer offsets (8 B per node, < 2^31)
constexpr int64_t RED_MAX_NODES = (int64_t)1 << 28;
// per-wave tail record: the NA values of the node open at the range end, then the tag
constexpr int RED_TAIL_WORDS = 8;  // 64 B: one line per wave
constexpr int RED_TAIL_TAG = 7;
constexpr uint64_t RED_TAG_READY = 1;  // published (0: free; the consumer clears it)

// Device fault words (one 64-B line per device, zero until a wait gives up; sticky until
// kcc_clear_faults): the reduce's look-back waits and the exchange's flag waits that gave
// up.  Every finalize reads them and marks every spec KCC_SPEC_FAULT while either is set,
// and the synchronous entry points return KCC_EFAULT.
enum { FAULT_RED = 0, FAULT_P2P = 1, FAULT_WORDS = 8 };
constexpr int32_t SPEC_ERR_DIV0 = 1;   // include/kcc.h KCC_SPEC_DIVZERO
constexpr int32_t SPEC_ERR_FAULT = 2;  // include/kcc.h KCC_SPEC_FAULT
// The fault travels with the data: a fit launched while its device is faulted adds
// SPEC_FAULT_MARK to every spec's div-by-zero count in partial[S..2S), once per spec, so
// every consumer of the partial — this device's finalize, the p2p exchange, an RCCL or
// torch.distributed all-reduce summed into another rank's finalize, the in-library device
// fold — sees a count >= SPEC_FAULT_MARK and marks the spec KCC_SPEC_FAULT.  Real counts
// are < 2^28 per device (one per node row); the marks of up to 2^14 launches x ranks sum
// without wrapping.
constexpr uint64_t SPEC_FAULT_MARK = 1ull << 48;

// Containers per wave range: whole tiles, sized so the waves fill the device's resident
// wave slots (occupancy API) in KCC_RED_ROUNDS rounds: one round of equal, long ranges
// leaves no half-empty second round (9672 waves of 4096 containers at C4 ran 1.6 rounds
// of 6144 resident waves).  Small inputs get one tile per wave.  `limits` selects the
// 4-array kernel (more registers, fewer resident waves).
// reserve_waves: resident wave slots left to other work of the same launch (the spec
// rank workgroups in front of the reduce's)
int32_t reduce_range(int64_t n_containers, bool limits, int64_t reserve_waves = 0);
inline int64_t reduce_n_waves(int64_t n_containers, bool limits, int64_t reserve_waves = 0) {
  const int64_t r = reduce_range(n_containers, limits, reserve_waves);
  return (n_containers + r - 1) / r;
}
// tail records a launch may need: an upper bound of reduce_n_waves (one range per
// resident wave slot at most)
int64_t reduce_tail_records();

// One reduce launch: nodes [0, n_nodes) of `ptr` (the caller offsets ptr and the
// per-node outputs for a node range) and containers [c0, c_end); the offsets in ptr and
// the container arrays stay absolute (ptr[0] == c0), so a node range of one CSR is
// reduced without rebasing anything.  Every output of [0, n_nodes) is written.
struct RedArgs {
  int64_t n_nodes, c0, c_end;
  int32_t range;
  const int64_t* ptr;
  const uint64_t* in[4];
  uint64_t* out[4];
  uint64_t* tail;                  // [reduce_tail_records()][RED_TAIL_WORDS], tags 0
  unsigned long long* faults;      // the device's fault words (FAULT_RED: look-back give-ups)
  int32_t ranks_last;              // the spec ranks' workgroups behind the reduce's (else in front)
};
// rank != nullptr (with rank->n_blocks > 0): the spec ranks run as that many extra
// workgroups beside the reduce's (independent work, one launch fewer per step): behind them
// on long reduces (>= KCC_RED_RANKS_LAST_MIN containers: they take the slots of the first
// waves to finish; C4 step 0.3059 -> 0.3030 ms), in front on short ones (the 8-way C4 rank:
// behind, they lengthened its 23 us reduce by 3 us).
hipError_t launch_reduce(int64_t n_nodes, int64_t c0, int64_t n_containers, const int64_t* node_ptr,
                         const uint64_t* cpu_req, const int64_t* mem_req,
                         const uint64_t* cpu_lim, const int64_t* mem_lim,
                         uint64_t* used_cpu, int64_t* used_mem, uint64_t* lim_cpu, int64_t* lim_mem,
                         uint64_t* tail, unsigned long long* faults, hipStream_t s,
                         const RankArgs* rank = nullptr, const NpArgs* np = nullptr,
                         hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
// (ev_start / ev_stop, kcc_profile_*: the kernel's own dispatch timestamps, hipExtLaunchKernel —
// event packets around the launch also timed the dispatch, ~3 us per launch)

// ---- (b) fit -----------------------------------------------------------------
// Node streams of the fit kernel: groups of FIT_GROUP nodes, field-major inside the
// group.  The per-node values arrive through the scalar cache and feed the VALU as
// SGPR operands.  The fast loops sum min(findMin(qc, qm), P) — the pod-slot clamp
// itself (CC:134-136) is added back per spec by the clamp correction (ClampWork).
// Rows outside the fast-path bounds, and the padding of the last group, hold all-zero
// fields (they contribute exactly 0) and are listed in slow_list for the exact path.
//
// FitGroupA — class-A spec waves: the integers themselves, which the
// VALU reads as IEEE denormals (an integer k < 2^23 is the f32 bit pattern of
// k * 2^-149, k < 2^52 the f64 pattern of k * 2^-1074).
constexpr int FIT_GROUP = 8;
struct __attribute__((aligned(32))) FitGroupA {
  uint64_t fm[FIT_GROUP];  // free memory (bytes), < 2^50
  uint32_t fc[FIT_GROUP];  // free CPU (millicores), < 2^23
  uint32_t P[FIT_GROUP];   // max(allocatable pods, 0), <= 2^20
};
static_assert(sizeof(FitGroupA) == 128, "FitGroupA must be 128 B");
// FitGroup — class-B spec waves (memory request < 2^18): f64 values for the biased
// FMA path; written by node_prep only when such specs exist.
constexpr double FIT_BIAS = 4503599627370496.0;  // 2^52: integers in [2^52, 2^53) have ulp 1
struct __attribute__((aligned(32))) FitGroup {
  double fc[FIT_GROUP];  // free CPU (millicores), exact in f64
  double fm[FIT_GROUP];  // free memory (bytes), exact in f64
  double Pb[FIT_GROUP];  // 2^52 + max(allocatable pods, 0) (<= 2^20: exact)
};
static_assert(sizeof(FitGroup) == 192, "FitGroup must be 192 B");
__host__ __device__ inline int64_t fit_groups(int64_t n_nodes) { return (n_nodes + FIT_GROUP - 1) / FIT_GROUP; }

// Raw per-node values for the exact path (fc/fm are 0 where the reference's
// `alloc <= used` branch yields 0, i.e. no division happens).
struct __attribute__((aligned(32))) SlowNode {
  uint64_t fc;
  int64_t fm;
  int64_t P;
  int64_t cl;
};
static_assert(sizeof(SlowNode) == 32, "SlowNode must be 32 B");

// One 48-B record per spec, in the kernel's internal (partitioned) order: class A
// first, then B, then the exact-path specs (so at most two wavefronts mix classes;
// a wave runs the most general class among its lanes).
enum SpecClass : int32_t { SPEC_A = 0, SPEC_B = 1, SPEC_EXACT = 2 };
struct __attribute__((aligned(16))) SpecRec {
  uint64_t c;    // cpu request (millicores)
  int64_t m;     // memory request (bytes)
  double rc;     // smallest f64 >= 1/c (classes A, B)
  double rm;     // smallest f64 >= 1/m (classes A, B)
  float rcf;     // smallest f32 >= 1/c (class A)
  int32_t cls;   // SpecClass
  int64_t pad;
};
static_assert(sizeof(SpecRec) == 48, "SpecRec must be 48 B");

struct SpecPrep {
  SpecRec* rec;    // by internal position
  int32_t* perm;   // internal index -> caller index
};

// Clamp correction.  On the fast paths the fit kernel sums
// min(findMin(qc, qm), P) and leaves out the pod-slot clamp of CC:134-136; the clamp is
// added back per spec as  partial[s] -= D_s,  D_s = Σ_i w_i [x_is >= P_i],  w_i = P_i - cl_i
// (the pod count; for P_i <= 0 rows, clamped for every spec, w_i = -cl_i).  For P_i >= 1,
// x_is >= P_i  <=>  c_s <= U_i = fc_i / P_i  and  m_s <= V_i = fm_i / P_i  (integer
// quotients): a 2-D dominance sum.  The nN normal specs (classes A and B) get an x-rank by
// (c, index) and a y-rank by (m, index) (permutations of 0..nN-1); row i dominates exactly
// the specs with x < L_i = #{c <= U_i} and y < b_i = #{m <= V_i}.  Both axes are cut into
// blocks of 64 ranks (T = ceil(nN / 64)):
//   - coarse: C[L_i >> 6][b_i >> 6] += w_i, a (T+2) x (T+2) table (P <= 0 rows in cell
//     [T+1][T+1]); spec s collects Σ_{GX > x_s>>6, GY > y_s>>6} C;
//   - x-group: the rows with L_i >> 6 == g, r = L_i & 63 > 0, in H2[g][k][r] with
//     k = #{specs of x-group g with y < b_i}; spec s (x-group g) collects
//     Σ_{k > kpos_s, r > x_s & 63} H2[g][k][r], kpos_s = #{specs of x-group g, y < y_s};
//   - y-block: the rows with b_i >> 6 == Y, r = b_i & 63 > 0, L_i >> 6 > 0, in H3[Y][j][r]
//     with j = #{specs of y-block Y whose x-group < L_i >> 6}; spec s collects
//     Σ_{j > jpos_s, r > y_s & 63} H3[Y][j][r], jpos_s = #{specs of y-block Y, x < x_s}.
// All tables are O(S) (the tables of round 1 grew as S^2/64: 270 MB at S = 16384).  C has
// one copy per XCD, H2/H3 two (node_prep's atomics spread over more cache lines); every
// copy is zero between calls: clamp_prep zeroes what it reads.
struct ClampWork {
  uint32_t* rank;    // [rank_words(S)] by caller index: x-ranks [0, S), y-ranks [S, 2S),
                     // then each slice's share of the x-rank and the y-rank
  uint32_t* bcnt;    // [ceil(S/64)][2] class A / class B specs per block of 64 (caller order)
  uint64_t* cs;      // [S] normal specs' cpu requests by x-rank (ascending)
  int64_t* ms;       // [S] memory requests by y-rank (ascending)
  uint32_t* mr_c;    // [64 * T] y-rank by x-rank (padding 0xffffffff)
  uint32_t* cr_m;    // [64 * T] x-rank by y-rank (padding 0xffffffff)
  int32_t* dperm;    // [S] x-rank -> internal position
  int64_t* C;        // [C_COPIES][c_stride]: (T+2) x (T+2), cell GX * (T+2) + GY
  int64_t* H2;       // [H2_COPIES][h_stride]: T x 65 x 64, cell (g * 65 + k) * 64 + r
  int64_t* H3;       // [H2_COPIES][h_stride]: T x 65 x 64, cell (Y * 65 + j) * 64 + r
  int64_t* Crow;     // [c_stride]: C summed over the copies, suffix sums along GY
  // binned form of H2 / H3 (clamp_binned(S)): node_prep writes each pass's
  // (cell, w) records sorted by bin (x-group g: bin g; y-block Y: bin T + Y) into the
  // pass's own slot range, and the bins' starts into dir; clamp_apply's workgroup for a
  // bin sums that bin's records of every pass into LDS.  No global atomics.
  uint64_t* rec;     // [n_pass][pass_recs]: cell | (int32 w) << 32
  uint32_t* dir;     // [n_pass][d_stride]: a pass's bin starts (exclusive prefix) + its total
  int64_t c_stride;  // cells per C copy (clamp_c_cells(S) of the workspace)
  int64_t h_stride;  // cells per H2 / H3 copy (clamp_h_cells(S))
  int64_t d_stride;  // clamp_d_stride(S) of the workspace
  int64_t n_pass;    // passes of the call's node rows (set by launch_clamp_apply)
  int64_t pass_recs; // record slots per pass: 2 x clamp_pass_rows (set by launch_clamp_apply)
};
// specs per call
constexpr int64_t MAX_SPECS = (int64_t)1 << 26;
__host__ __device__ inline int64_t clamp_c_cells(int64_t S) { return (S / 64 + 3) * (S / 64 + 3); }
inline int64_t clamp_h_cells(int64_t S) { return (S / 64 + 1) * 65 * 64; }
// copies of the coarse table: node_prep flushes its LDS-summed table once per workgroup
// (S <= 4096), so two spread the flushes enough; clamp_apply's x-group workgroups read
// every copy (C4 8-way shard, fit prepare + run: 8 copies 60.4 us, 2: 58.2, 1: 58.5; C5's
// global-memory atomics need more than one: 544.8 / 545.5 / 557.8 us)
constexpr int C_COPIES = 2;
constexpr int H2_COPIES = 2;
// binned H2 / H3 (ClampWork::rec): node_prep's passes of clamp_pass_rows(n) rows (1 or 4
// per thread) emit at most one record of each table per row; up to CLAMP_BIN_T_MAX
// x-groups (S <= 16384), larger S adds to the H2 / H3 copies with device atomics
constexpr int CLAMP_PASS_ROWS_MIN = 1024;
constexpr int CLAMP_PASS_ROWS_MAX = 4096;  // chunks of a pipelined call are multiples of it
// Rows per node_prep pass for a call of n_nodes rows: 4096 when such passes still fill
// the chip (one node_prep workgroup per CU), else 1024 — 4x the workgroups on small
// shards (C4's 8-way shard: 123 instead of 31).  Fewer, larger passes keep clamp_apply's
// heavy bins cheap: a bin's records are read pass by pass, and at C4 one bin held 34k
// records (12.9 us to consume over 245 passes, 28.5 us over 977).
inline int64_t clamp_pass_rows(int64_t n_nodes) {
  return n_nodes >= (int64_t)200 * CLAMP_PASS_ROWS_MAX ? CLAMP_PASS_ROWS_MAX : CLAMP_PASS_ROWS_MIN;
}
constexpr int64_t CLAMP_BIN_T_MAX = 256;
__host__ __device__ inline bool clamp_binned(int64_t S) { return (S + 63) / 64 <= CLAMP_BIN_T_MAX; }
inline int64_t clamp_d_stride(int64_t S) { return 2 * ((S + 63) / 64) + 1; }
inline int64_t clamp_passes(int64_t n_nodes) {
  const int64_t pr = clamp_pass_rows(n_nodes);
  return (n_nodes + pr - 1) / pr;
}
// up to this many specs node_prep's search and count tables live in LDS; larger S
// searches the same tables in global memory
constexpr int64_t CLAMP_LDS_SPECS = 4096;

// Spec ranks (spec_rank): the x-rank by (c, index) and the y-rank by (m, index) of every
// normal spec, by sort and search: workgroup (query block of RANK_L, slice of RANK_L
// candidates), rank_slices(S)^2 workgroups; each sorts its slice's keys in registers and LDS
// and finds each query's count below it by binary search.  Each slice stores its x and y
// counts (rank[S + (slice * 2 + r) * S + i], write-through) and adds to its query block's
// arrival counter; the last slice to arrive (the counter's returned value) sums the
// slices and writes the sorted arrays itself — cs[x] = c, ms[y] = m, mr_c[x] = y,
// cr_m[y] = x — and rank[i] = x, rank[S + i] = y, then resets the counter.  The slice-0 workgroups store
// the class-A / class-B counts of each block of 64 queries (bcnt).  The rank workgroups
// also zero the counters (all but CNT_SPECS_A / CNT_SPECS_B, set by spec_place) and the
// coarse clamp table's cells: the first launch of a step, ahead of every reader.
constexpr int64_t RANK_L = 1024;         // candidates per slice: 16 KiB of 16-B keys
constexpr int64_t RANK_FULL_MAX = 4096;  // up to this S the ranks count (above: sort + search)
__host__ __device__ inline int64_t rank_slices(int64_t S) { return (S + RANK_L - 1) / RANK_L; }
// u32 words of ClampWork::rank for S specs: the x- and y-ranks, then the slices' counts
__host__ __device__ inline int64_t rank_words(int64_t S) { return 2 * S + 2 * S * rank_slices(S); }
struct RankArgs {
  int64_t S;
  const uint64_t* c_in;
  const int64_t* m_in;
  uint32_t* part;      // ClampWork::rank
  uint32_t* arrive;    // [rank_slices(S)] per query block: slices arrived (zero between calls)
  uint32_t* bcnt;      // ClampWork::bcnt
  uint64_t* cs;        // ClampWork::cs / ms / mr_c / cr_m
  int64_t* ms;
  uint32_t* mr_c;
  uint32_t* cr_m;
  int64_t* C;          // ClampWork::C: cells [0, c_cells) of each copy are zeroed
  int64_t c_stride, c_cells;
  unsigned long long* counters;
  int32_t n_blocks;    // 256-thread workgroups: rank_slices(S)^2 (0: none)
  // 1: the clamp in the fit needs no ranks — one workgroup that zeroes the counters and
  // writes the block class counts (bcnt) alone (PlaceArgs::no_ranks)
  int32_t zero_only;
  // zero_only with node prep in the same launch (NpArgs): the counters and bcnt written
  // through (sc1), then *done_flag = 1 for the node-prep workgroups
  uint32_t* done_flag;      // NpArgs::sync (the epoch at NP_EPOCH, the flag at NP_DONE)
};
RankArgs rank_args(int64_t n_specs, const uint64_t* spec_cpu, const int64_t* spec_mem,
                   const ClampWork& cw, unsigned long long* counters, uint32_t* arrive,
                   bool zero_only = false);
hipError_t launch_spec_rank(const RankArgs& ra, hipStream_t s);

// spec_place's work (one thread per spec), run as extra workgroups in front of the
// node_prep launch (node_prep reads only the arrays spec_rank wrote, and not the padding
// spec_place writes): the stable 3-way partition position, the
// SpecRec / perm there, dperm, mr_c / cr_m's padding, partial[0..2S) zeroed,
// CNT_SPECS_A / CNT_SPECS_B set.
struct PlaceArgs {
  int64_t S;
  const uint64_t* c_in;
  const int64_t* m_in;
  SpecPrep sp;
  ClampWork cw;
  int64_t* partial;
  unsigned long long* counters;
  int32_t n_blocks;  // workgroups of the launch's block size (0: none)
  const unsigned long long* faults;  // set: partial[S + i] starts at SPEC_FAULT_MARK
  // 1 (the clamp in the fit, S <= CLAMP_LDS_SPECS): no spec ranks ran (only bcnt was
  // written): nothing rank-indexed is read or written
  int32_t no_ranks;
};


// Node prep of the clamp in the fit (one node chunk, S <= CLAMP_LDS_SPECS, not dense, at
// least one node and one container) as workgroups behind a reduce launch's: n_place
// workgroups of spec_place (after the zero_only rank workgroup's flag), then n_rows
// workgroups of 1024 rows each (np_rows: the row pass it shares with node_prep_kernel, each
// after the reduce waves that store its rows have signalled).  Every call with the clamp in
// the fit runs it here; node_prep_kernel serves the clamp-correction layout alone.  The reduce's node sums go
// out write-through (sc1) and each reduce wave adds 1 to sync[16] when done (its stores
// performed); the node-prep workgroups read them at agent scope.  The last of them resets
// the sync words.  Dispatch order makes the waits safe: on every XCD all the reduce's
// workgroups are dispatched before any node-prep workgroup, and no reduce wave waits on
// one.  Every wait is bounded; a give-up counts in faults[FAULT_RED].
struct NpArgs {
  int32_t n_place, n_rows;  // workgroups (256 threads)
  uint32_t* sync;           // NP_EPOCH, NP_DONE, NP_ARRIVE, NP_FLAGS (reduce_tail_records() words)
  // set by launch_reduce: the reduce's CSR offsets, first container, range and wave count
  const int64_t* ptr;
  int64_t c0;
  int32_t range, red_waves;
  PlaceArgs pa;
  int64_t n;                // rows
  const uint64_t* alloc_cpu;
  const int64_t* alloc_mem;
  const int64_t* alloc_pods;
  const int64_t* pod_count;
  const uint64_t* used_cpu;
  const int64_t* used_mem;
  FitGroupA* fast_a;
  FitGroup* fast_b;
  SlowNode* slow;
  int64_t* slow_list;
  int32_t* fast_cl;
  unsigned long long* counters;
  const uint32_t* bcnt;
  int64_t S;
  unsigned long long* faults;
};
constexpr int NP_ROWS_PER_WG = 1024;  // 256 threads x 4 rows
// NpArgs::sync (uint32 words, 64-B lines): [NP_EPOCH] the last launch's epoch (a launch's
// epoch E is one past it; its last node-prep workgroup to finish publishes E), [NP_DONE]
// the spec ranks' done flag (= E), [NP_ARRIVE] the node-prep arrivals (zero between
// launches), then [NP_FLAGS + w] reduce wave w's flag (= E once its node sums are stored).
// Epoch flags need no reset, and a node-prep workgroup waits for the waves that store its
// rows alone: one counter of every wave's arrival took the ~3200 same-address atomics of
// the 8-way C4 rank serially (~25 ns apiece, 80 us)
constexpr int NP_EPOCH = 0, NP_DONE = 16, NP_ARRIVE = 32, NP_FLAGS = 64;

// counters (CNT_*): exact-path (node, spec) pairs, class-B specs, and per node chunk
// of a pipelined call (kcc_capacity_partial_async) the rows in that chunk's slow_list.
// spec_rank zeroes the counters, spec_place sets the class counts and zeroes
// partial[0..2S); node_prep appends to slow_list and the fit streams.
constexpr int FIT_MAX_CHUNKS = 16;
enum {
  CNT_SLOW_PAIRS = 0,  // (node, spec) pairs evaluated on the exact path
  CNT_SPECS_A = 1,     // class-A specs (internal positions [0, nA))
  CNT_SPECS_B = 2,     // class-B specs (internal positions [nA, nA + nB))
  CNT_CLAMP_ALL = 3,   // clamp in the fit: Σ (max(P, 0) - clamp) of the rows clamped for
                       // every spec (P <= 0), subtracted from every normal spec by the fit
  CNT_SLOW_ROWS = 4,   // + chunk: rows in that node chunk's slow_list
  CNT_STREAM = 4 + FIT_MAX_CHUNKS,  // + chunk: node rows in that chunk's fit stream (x 8)
  CNT_N = 4 + 2 * FIT_MAX_CHUNKS
};
// The clamp correction after every node_prep of the call (n_nodes: the call's rows, for
// the binned records' pass count): partial[s] -= D_s for the normal specs of clamp-free
// waves; leaves the table copies zero.
// fin != nullptr (one rank, the call's last kernel): the launch's last workgroup to finish
// (an arrival counter, zero between launches) also finalizes — totals[perm[i]] = err ? 0 :
// partial[i], spec_err[perm[i]] = err — instead of a fit_finalize launch.
struct FinArgs {
  const int32_t* perm;
  int64_t* totals;
  int32_t* spec_err;
  uint32_t* arrive;
  const unsigned long long* faults;  // the device's fault words: set -> KCC_SPEC_FAULT
};
hipError_t launch_clamp_apply(int64_t n_specs, int64_t n_nodes, ClampWork cw,
                              const unsigned long long* counters, int64_t* partial, hipStream_t s,
                              const FinArgs* fin = nullptr);
int64_t clamp_apply_blocks(int64_t n_specs);  // clamp_apply_kernel's grid
// the spec ranks' workgroups of a fused reduce launch go behind the reduce's workgroups on
// launches of at least this many containers, in front of them on shorter ones
constexpr int64_t RED_RANKS_LAST_MIN = (int64_t)16 << 20;

// The fit's node stream (FitGroupA / FitGroup records) holds the rows that can contribute
// to the fast sum Σ min(findMin(qc, qm), P): fast-bound rows with free CPU, free memory
// and P >= 1 (every other row adds exactly 0 there: qc = 0 or qm = 0 makes x = 0, and
// P <= 0 rows are the clamp correction's), compacted per workgroup pass into
// counters[CNT_STREAM + chunk] rows (padded to whole groups).  dense: stream every row (the
// round-1 layout's cost: zero fields for the rows that add nothing).  row0: the launch's
// first row within the call (a multiple of CLAMP_PASS_ROWS_MAX; the binned records'
// passes), call_nodes: the call's rows (its pass size, clamp_pass_rows).
// Needs the sorted spec arrays (spec_rank's) on the stream before it.  place != nullptr:
// spec_place runs as extra workgroups of this launch (place->n_blocks is set here).
// The clamp-correction layout only: a call with the clamp in the fit launches none (below).
hipError_t launch_node_prep(int64_t n_nodes, const uint64_t* alloc_cpu,
                            const int64_t* alloc_mem, const int64_t* alloc_pods,
                            const int64_t* pod_count, const uint64_t* used_cpu,
                            const int64_t* used_mem, FitGroupA* fast_a, FitGroup* fast_b,
                            SlowNode* slow, int64_t* slow_list, int64_t n_specs, ClampWork cw,
                            unsigned long long* counters, int chunk, int64_t row0,
                            int64_t call_nodes, hipStream_t s, bool dense = false,
                            const PlaceArgs* place = nullptr);
// Clamp in the fit (one node chunk, S <= CLAMP_LDS_SPECS, not dense, at least one node and
// one container; no launch_node_prep): node prep in the reduce launch (NpArgs) streams each
// row's clamp value (allocatable pods - pod count, CC:135) beside its FitGroupA
// (fast_cl[row position]) and builds no clamp tables; the fit (fast_cl != nullptr) computes the
// reference's x >= P ? clamp : x itself (5 VALU per node x wave instead of 3) and
// subtracts counters[CNT_CLAMP_ALL] from every normal spec; no clamp_apply launch.  The
// choice for small shards, where clamp_apply's fixed cost exceeds the fit's extra issue.
// node rows x specs at most: the C4 8-way (5.1e8) and 4-way (1.0e9) shards
constexpr int64_t CLAMP_IN_FIT_PAIRS = 1100000000LL;
inline bool clamp_in_fit_auto(int64_t n_nodes, int64_t n_specs) {
  return n_specs <= CLAMP_LDS_SPECS && n_nodes * n_specs <= CLAMP_IN_FIT_PAIRS;
}

// partial[0..S) += Σ_i q(i,s), partial[S..2S) += #div-by-zero rows (internal order).
hipError_t launch_fit(int64_t n_nodes, const FitGroupA* fast_a, const FitGroup* fast_b,
                      const SlowNode* slow,
                      const int64_t* slow_list, int64_t n_specs, SpecPrep sp, int64_t* partial,
                      unsigned long long* counters, uint32_t* queue, int chunk,
                      int64_t grid_nodes, hipStream_t s, const unsigned long long* faults,
                      const int32_t* fast_cl = nullptr, hipEvent_t ev_start = nullptr,
                      hipEvent_t ev_stop = nullptr);
// the fit's work queues: fit_queue_words(S) uint32 (a 64-B line per spec column of 256 and
// sub-queue), zero before the first launch (each launch leaves them zero)
constexpr int64_t FIT_QSUBS_MAX = 32;
inline int64_t fit_queue_words(int64_t S) { return (S + 255) / 256 * FIT_QSUBS_MAX * 16; }

// totals[perm[i]] = err ? 0 : partial[i], spec_err[perm[i]] = err (KCC_SPEC_DIVZERO when
// partial[S + i] != 0; KCC_SPEC_FAULT for every spec while a fault word is set)
hipError_t launch_fit_finalize(int64_t n_specs, const int64_t* partial,
                               const int32_t* perm, int64_t* totals, int32_t* spec_err,
                               const unsigned long long* faults, hipStream_t s);
// dst[k] += src[k] (wrapping int64), k < n: folds one node shard's partial vector into
// another on the same device (the host-array entry points with more shards than devices)
hipError_t launch_partial_add(int64_t n, int64_t* dst, const int64_t* src, hipStream_t s);

// ---- one-shot exchange of the per-spec partials over xGMI peer memory (kcc_p2p_*) -----
// One process per GPU, W <= P2P_MAX_RANKS.  Every rank owns a mailbox in its own HBM,
// exported as an IPC handle and mapped by every peer:
//   flags [2][W][8] u64 (parity, sender: one 64-B line each; the sender's epoch),
//   data  [2][W][2 smax] i64 (parity, sender: the sender's partial — sums, then div-by-zero
//         counts).
// exchange_finalize_kernel (one launch per step, replacing the RCCL all-reduce and
// fit_finalize): thread i pushes spec i's two partial words into every mailbox (remote
// stores over xGMI, its own included), the launch's last workgroup to finish pushing
// (arrival counter) publishes the epoch into every mailbox's flag of this sender (system
// scope, after every pushing thread's system-scope fence), every workgroup waits for all
// W flags of this epoch in its own mailbox, then sums the W vectors and finalizes
// (totals[perm[i]], spec_err[perm[i]]).  Parity = epoch & 1: a rank can only push epoch
// e + 2 after every peer pushed e + 1, i.e. after every peer's launch for e read its data.
// The epoch lives in device memory (the last workgroup to push advances it), so every
// launch — a replay of a captured graph included — uses the next one.
constexpr int P2P_MAX_RANKS = 8;
__host__ __device__ inline size_t p2p_flag_words(int W) { return (size_t)2 * W * 8; }
inline size_t p2p_mbox_bytes(int W, int64_t smax) {
  return 8 * (p2p_flag_words(W) + (size_t)2 * W * 2 * (size_t)smax);
}
struct P2PArgs {
  int64_t S, smax;
  int32_t W, rank;
  uint64_t* epoch;                        // this rank's last pushed epoch (device word, 0 at
                                          // export; the launch pushes *epoch + 1)
  const int64_t* partial;                 // [2S] this rank's (internal order)
  unsigned char* mbox[P2P_MAX_RANKS];     // rank p's mailbox (this rank's own at [rank])
  const int32_t* perm;                    // internal -> caller index (this rank's fit)
  int64_t* totals;
  int32_t* spec_err;
  uint32_t* arrive;                       // this rank's push arrivals (zero between launches)
  unsigned long long* faults;             // the device's fault words (FAULT_P2P: flag waits
                                          // that gave up; a workgroup that gave up marks its
                                          // specs KCC_SPEC_FAULT)
};
hipError_t launch_exchange_finalize(const P2PArgs& a, hipStream_t s);

// ---- quantity-string parse (kcc_parse.hip) ------------------------
enum ParseMode : int { PARSE_MODE_CPU_MILLIS = 0, PARSE_MODE_BYTES = 1, PARSE_MODE_QUANTITY = 2 };
// per-string status (include/kcc.h KCC_PARSE_*)
enum ParseStatus : int8_t {
  PARSE_OK = 1,           // value as the reference computes it
  PARSE_ERR = 0,          // the reference reports an error and uses 0
  PARSE_UNSUPPORTED = -1, // outside the device parser's exact domain (value 0)
  PARSE_BADOFF = -2       // offsets outside [0, n_bytes] or decreasing (value 0)
};
int64_t parse_grid(int64_t n);
// string i = bytes[offsets[i], offsets[i+1]); bytes 4-byte aligned
hipError_t launch_parse(int mode, int64_t n, const uint8_t* bytes, int64_t n_bytes,
                        const int64_t* offsets, int64_t* out, int8_t* status, hipStream_t s);

// ---- keyed (list-order) reduce (kcc_keyed.hip) --------------------
// Bucketed path: rows in buckets of KB_ROWS, containers in tiles of about KB_TILE.
constexpr int KB_SHIFT = 12;  // 4096 rows per bucket: ~1 KB runs per tile and array
constexpr int KB_ROWS = 1 << KB_SHIFT;
// containers per scatter workgroup (about; keyed_tile cuts whole rounds): at C4 65536
// (3 rounds, 768 tiles) took the keyed call 0.392 -> 0.340 and 0.395 -> 0.372 ms on two
// boxes against 32768 (5 rounds); 131072 equal, 262144 slower
constexpr int KB_TILE = 65536;
constexpr int64_t KB_NB_MAX = 4096;  // buckets (LDS cursors): n_keys <= 16M rows
struct KeyedWork {
  uint32_t* counts;   // [keyed_tiles(n) * keyed_buckets(n_keys)] (one-sweep path: the tiles'
                      // bucket starts, u16 entries in blocks of 32 buckets, kcc_keyed.hip kb_tab_at)
  uint32_t* tot;      // [keyed_buckets(n_keys)]
  uint64_t* sr;       // [n] scattered 8-B records: row within the bucket, low 20 cpu
                      // bits, memory / 64 (kcc_keyed.hip kb_record)
  uint64_t* sv;       // [n][2] the limit values, element-major (NA = 4 only)
  uint32_t* esc_n;    // escape list: what the records cannot hold (cpu >= 2^20: its high
  int32_t* esc_row;   // [n]   bits; memory not a multiple of 64 in [0, 2^38): all of it)
  uint64_t* esc_cpu;  // [n]
  uint64_t* esc_mem;  // [n]
  // one-sweep path (kb_sweep + kb_gather): a bucket group's records are gathered by
  // keyed_sweep_parts(nb) workgroups; parts > 1 sum through part_acc: every part but the
  // last to arrive (arrive[b]) publishes its rows and counts itself (arrive[groups + b]),
  // the last adds them and writes the group's outputs
  uint64_t* part_acc; // [groups][parts][NACC][KB_GA_ROWS]
  uint32_t* arrive;   // [2 x groups]: arrivals, then the published parts (zero between calls)
  unsigned long long* faults;  // the device's fault words (a gather wait that gave up)
};
// One-sweep keyed reduce (NA = 0 counts, 2 requests): each tile of KB_SW_TILE containers
// is counting-sorted by bucket in LDS and written contiguously into its own region of sr
// (whole lines), with the bucket starts in its table row — no global histogram pass, no
// scan, keys read once.  kb_gather then sums bucket b's segments of every tile into LDS
// rows.  The four-kernel bucketed path (kb_hist / kb_scan / kb_scatter / kb_accum) serves
// only the calls with limits (NA = 4).
constexpr int KB_SW_THREADS = 1024;
constexpr int KB_SW_PER = 8;  // containers per thread (the next tile's loads in registers)
constexpr int64_t KB_SW_TILE = (int64_t)KB_SW_THREADS * KB_SW_PER;  // 8192
// containers per sweep tile: KB_SW_TILE, or (beyond one round of one tile per CU) cut so
// the tiles make whole rounds (C4: 2418 tiles = 9.4 rounds -> 2560 of 15472 = 10); a
// tile's records keep the KB_SW_TILE stride in the staging buffer
int64_t keyed_sweep_tile(int64_t n);
int64_t keyed_sweep_tiles(int64_t n);
int keyed_sweep_parts(int64_t nb);
// sizes of the KeyedWork arrays for a call (either path): u32 words of counts, u64
// record slots of sr, u64 words of part_acc
int64_t keyed_counts_words(int64_t n_keys, int64_t n);
int64_t keyed_sr_slots(int64_t n);
int64_t keyed_part_words(int64_t n_keys, int na);
int64_t keyed_tile(int64_t n);   // containers per scatter workgroup (whole CU rounds)
int64_t keyed_tiles(int64_t n);
int64_t keyed_buckets(int64_t n_keys);
bool keyed_bucketed(int64_t n_keys, int64_t n);
// Writes every per-key output (zero where no container), adding every container with
// 0 <= key < n_keys (wrapping sums are order-independent).  kw == nullptr or too many keys:
// memsets + device atomics.  key/value arrays 16-B aligned.
hipError_t launch_reduce_keyed(int64_t n_keys, int64_t n, const int32_t* key, const uint64_t* cpu,
                               const int64_t* mem, const uint64_t* cpul, const int64_t* meml,
                               uint64_t* used_cpu, int64_t* used_mem, uint64_t* lim_cpu,
                               int64_t* lim_mem, const KeyedWork* kw, hipStream_t s);
// count[k] = #{i : key[i] == k}
hipError_t launch_count_keyed(int64_t n_keys, int64_t n, const int32_t* key, int64_t* count,
                              const KeyedWork* kw, hipStream_t s);

// ---- per-row q of one spec (kcc_rows.hip) -------------------------
hipError_t launch_fit_rows(int64_t n, const uint64_t* alloc_cpu, const int64_t* alloc_mem,
                           const int64_t* alloc_pods, const int64_t* pod_count,
                           const uint64_t* used_cpu, const int64_t* used_mem, uint64_t spec_cpu,
                           int64_t spec_mem, int64_t* q, int32_t* err, hipStream_t s);

// ---- the cell fits: per node-group x spec totals -------------
// kcc_fit_grouped, kcc_fit_ext and kcc_fit_capped are one path: the records (kcc_ext.hip:
// ext_rows<R>, or kcc_groups.hip's hist / scan and ext_scatter<R> with group ids), one pair
// loop (ext_pairs_body below, as ext_pairs<R>, kcc_spread.hip's cap_pairs<R> or
// kcc_explain.hip's why_pairs<R>) and a finalize.  The grouped fit is the R = 0 instance with group ids.
//
// The record of one node row, placed in group order: the exact path's integers (fc / fm
// are 0 where the reference's `alloc <= used` branch divides nothing) and, for a fast row
// (fc < 2^31, 0 <= fm < 2^50), the same two values as f64 (0.0 otherwise).
struct __attribute__((aligned(16))) GrpRow {
  uint64_t fc;
  int64_t fm;
  int64_t P;
  int64_t cl;   // allocatable pods - pod count (wraps), CC:135
  double fcd;
  double fmd;
};
static_assert(sizeof(GrpRow) == 48, "GrpRow must be 48 B");
// R: group-ordered rows one pair-loop workgroup walks (tests/test_groups.py restates it).
// A wave flushes 64 x 8 B of atomics per run and group change, 8 S (N / R + G) bytes a call
// (twice that for the cells that count a divide by zero): at 1M rows x 4096 specs x 1024
// groups 162 MB, for 4.1e9 pairs.
constexpr int GRP_RUN = 256;
constexpr int GRP_PAIR_THREADS = 256;  // 4 waves x 64 specs per pair-loop workgroup
constexpr int GRP_LDS_GROUPS = 4096;   // up to this G the sort's per-workgroup counts live in LDS
constexpr int64_t GRP_MAX_CELLS = (int64_t)1 << 28;  // G x S
constexpr int64_t GRP_MAX_NODES = ((int64_t)1 << 31) - 4096;
inline int64_t grp_runs(int64_t n_nodes) { return (n_nodes + GRP_RUN - 1) / GRP_RUN; }
inline int64_t grp_sblocks(int64_t S) { return (S + GRP_PAIR_THREADS - 1) / GRP_PAIR_THREADS; }
struct GrpWork {
  uint32_t* count;   // [G] rows per group
  uint32_t* cursor;  // [G] next free slot of each group (starts at the exclusive scan)
  uint32_t* total;   // [1] rows with a valid group id
  GrpRow* rec;       // [n] records in group order
  int32_t* rg;       // [n] the record's group | fast-row bit
  int64_t* acc;      // [2 G S] the pre-finalize pair: wrapping sums, then divide-by-zero counts
  unsigned long long* cnt(int64_t cells) const {
    return reinterpret_cast<unsigned long long*>(acc + cells);
  }
};

// The sort's constants, the launches of kcc_groups.hip's kernels and the pair loop's
// device helpers.
constexpr int GRP_SORT_THREADS = 1024;  // rows per workgroup of the hist / scatter kernels
constexpr int GRP_ROW_FAST = 1 << 30;   // rg[]: the row's group, and this bit for a fast row
constexpr uint64_t GRP_FC_MAX = 1ull << 31;  // fast rows: free CPU below this
constexpr uint64_t GRP_FM_MAX = 1ull << 50;  // fast rows: free memory below this (and >= 0)
constexpr uint64_t GRP_SPEC_MAX = 1ull << 52;  // fast specs: 1 <= c, m <= this
// grp_hist + grp_scan: w.count zeroed, then count / cursor / total filled from group[0..n).
hipError_t launch_grp_count_scan(int64_t n, int64_t G, const int32_t* group, const GrpWork& w,
                                 hipStream_t s);
// grp_finalize over acc / cnt [cells].
hipError_t launch_grp_finalize(int64_t cells, const int64_t* acc, const unsigned long long* cnt,
                               int64_t* totals, int32_t* spec_err, hipStream_t s);

#if defined(__HIPCC__)
__device__ inline bool grp_valid(int32_t g, int64_t G) { return g >= 0 && (int64_t)g < G; }

// floor(f / d) for integers 0 <= f < 2^50, 1 <= d <= 2^52 held exactly in f64; rd = 1.0 / d.
__device__ inline double grp_div(double f, double d, double rd) {
  double t = __builtin_trunc(f * rd);
  const double r = __builtin_fma(-t, d, f);  // exact: an integer of magnitude < 2 d
  t = r < 0.0 ? t - 1.0 : t;
  t = r >= d ? t + 1.0 : t;
  return t;
}

__device__ inline void grp_flush(int64_t* __restrict__ acc, unsigned long long* __restrict__ cnt,
                                 int64_t cell, bool live, int64_t sum, unsigned long long z) {
  if (live) atomicAdd(reinterpret_cast<unsigned long long*>(acc) + cell, (unsigned long long)sum);
  if (__any(z != 0) && live) atomicAdd(cnt + cell, z);
}
#endif

// ---- extended-resource fit (kcc_ext.hip) ---------------------------
// Up to EXT_MAX extra int64 resources per row (resource-major columns) join findMin; a
// zero request leaves its resource out.  The row record is GrpRow plus, per resource, one
// ExtCol: the free amount (0 where alloc <= used) and, for a fast row (GrpRow's bounds and
// 0 <= fx < 2^50 for every resource), the same value as f64.
constexpr int EXT_MAX = 4;
struct __attribute__((aligned(16))) ExtCol {
  int64_t fx;
  double fxd;
};
static_assert(sizeof(ExtCol) == 16, "ExtCol must be 16 B");
struct ExtWork {
  GrpWork g;    // count / cursor / total are used only with group ids
  ExtCol* xrec;  // [n * R] record-major: the R columns of record p at xrec[p * R ...]
};
// The two sides of a cell fit as the host code hands them on (kernels take scalars and
// pointers).  The arrays are device pointers at the launchers, host or device in kcc_abi.cpp.
struct FitNodes {
  int64_t n;
  const uint64_t* alloc_cpu;
  const int64_t* alloc_mem;
  const int64_t* alloc_pods;
  const int64_t* pod_count;
  const uint64_t* used_cpu;
  const int64_t* used_mem;
  int64_t R;               // extra resources, 0 .. EXT_MAX
  const int64_t* alloc_x;  // [R, n] (not read with R = 0)
  const int64_t* used_x;
  const int32_t* group;    // nullptr: every row in group 0 (G must be 1), records in row order
  int64_t G;
};
struct FitSpecs {
  int64_t S;
  const uint64_t* spec_cpu;
  const int64_t* spec_mem;
  const int64_t* spec_x;     // [R, S]
  const int64_t* node_cap;   // [S], kcc_fit_capped alone (nullable; <= 0: no cap)
};
// What one call takes: n, G, S >= 1, 0 <= R <= EXT_MAX, G S <= GRP_MAX_CELLS, n <=
// GRP_MAX_NODES and a pair-loop grid of at most 2^31 - 1 workgroups.
inline bool ext_sizes_ok(const FitNodes& nd, int64_t S) {
  if (nd.n <= 0 || S <= 0 || nd.G <= 0 || nd.R < 0 || nd.R > EXT_MAX || (!nd.group && nd.G != 1))
    return false;
  return nd.G <= GRP_MAX_CELLS && S <= GRP_MAX_CELLS && nd.G * S <= GRP_MAX_CELLS &&
         nd.n <= GRP_MAX_NODES && grp_runs(nd.n) * grp_sblocks(S) <= 0x7fffffff;
}
// f(std::integral_constant<int, R>) for a runtime R: R is a template argument of the kernels.
template <class F>
inline hipError_t ext_dispatch(int64_t R, F&& f) {
  static_assert(EXT_MAX == 4, "one case per R");
  switch (R) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
  }
  return hipErrorInvalidValue;
}
// Every cell of totals / spec_err [G * S] is written.  hipErrorInvalidValue unless
// ext_sizes_ok; sp.node_cap is not read.
hipError_t launch_fit_ext(const FitNodes& nd, const FitSpecs& sp, const ExtWork& w,
                          int64_t* totals, int32_t* spec_err, hipStream_t s);
// The launches of launch_fit_ext ahead of its pair loop: acc / cnt [2 G S] zeroed, then the
// records (hist, scan and scatter with group ids; one row pass without).
hipError_t launch_ext_records(const FitNodes& nd, int64_t S, const ExtWork& w, hipStream_t s);

#if defined(__HIPCC__)
constexpr unsigned long long SPREAD_SIGN = 1ull << 63;  // qmin[] cells: q ^ SPREAD_SIGN, unsigned order

// The pair loop of ext_pairs<R> (kcc_ext.hip) and of cap_pairs<R> (kcc_spread.hip): one body,
// so the two cannot drift apart.  SPREAD adds, after the one conversion and after the
// pod-slot clamp, the per-lane minimum of q and the per-node cap (integer compare-and-
// selects), and flushes the minimum with a 64-bit atomic min where grp_flush runs; without
// SPREAD none of that code exists.  total == nullptr: the n_rec records of the ungrouped
// pass; else *total (the rows with a valid group id, from grp_scan).
// WHY (kcc_explain.hip's why_pairs<R>, with SPREAD) carries the term that won
// each pair's findMin along: b in [0, R + 4) — CPU, memory, extra resource r at 2 + r, then
// the pod-slot clamp and the cap — under findMin's tie rule (the earlier term keeps an equal
// quotient; the clamp fires on equality, the cap does not).  Per lane R + 4 row counters and
// R + 4 sums of q, indexed statically, flushed where grp_flush runs into the plane-major
// why_rows / why_pods [KCC_WHY_SLOTS][cells] (either may be nullptr); without WHY none of
// that code exists.
constexpr int WHY_SLOTS = 8;  // include/kcc.h KCC_WHY_SLOTS
constexpr int WHY_PODS = 6, WHY_CAP = 7;
static_assert(2 + EXT_MAX <= WHY_PODS, "the extra resources' slots end below KCC_WHY_PODS");

template <int R>
__device__ inline void why_flush(unsigned long long* __restrict__ why_rows,
                                 unsigned long long* __restrict__ why_pods, int64_t cells,
                                 int64_t cell, bool live, uint32_t (&wr)[R + 4],
                                 uint64_t (&wp)[R + 4]) {
#pragma unroll
  for (int k = 0; k < R + 4; ++k) {
    const int64_t slot = k < R + 2 ? k : WHY_PODS + (k - (R + 2));
    if (live && wr[k] != 0) {  // (no rows: the sum is 0 too)
      if (why_rows) atomicAdd(why_rows + slot * cells + cell, (unsigned long long)wr[k]);
      if (why_pods) atomicAdd(why_pods + slot * cells + cell, (unsigned long long)wp[k]);
    }
    wr[k] = 0;
    wp[k] = 0;
  }
}

template <int R, bool SPREAD, bool WHY = false>
__device__ inline void ext_pairs_body(
    const uint32_t* __restrict__ total, int64_t n_rec, int64_t S, int64_t sblocks,
    const uint64_t* __restrict__ spec_cpu, const int64_t* __restrict__ spec_mem,
    const int64_t* __restrict__ spec_x, const GrpRow* __restrict__ rec,
    const ExtCol* __restrict__ xrec, const int32_t* __restrict__ rg, int64_t* __restrict__ acc,
    unsigned long long* __restrict__ cnt, const int64_t* __restrict__ node_cap,
    unsigned long long* __restrict__ qmin, unsigned long long* __restrict__ why_rows = nullptr,
    unsigned long long* __restrict__ why_pods = nullptr, int64_t cells = 0) {
  static_assert(!WHY || SPREAD, "WHY is built on the capped loop");
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
  [[maybe_unused]] int64_t capv = INT64_MAX;  // SPREAD: no cap (NULL or <= 0) is a cap nothing exceeds
  if constexpr (SPREAD) {
    const int64_t k = (node_cap && live) ? node_cap[s] : 0;
    capv = k > 0 ? k : INT64_MAX;
  }

  int64_t sum = 0;
  [[maybe_unused]] int64_t mn = INT64_MAX;
  unsigned long long z = 0;
  [[maybe_unused]] uint32_t wr[R + 4];
  [[maybe_unused]] uint64_t wp[R + 4];
  if constexpr (WHY) {
#pragma unroll
    for (int k = 0; k < R + 4; ++k) {
      wr[k] = 0;
      wp[k] = 0;
    }
  }
  int gcur = __builtin_amdgcn_readfirstlane(s_rg[0]) & (GRP_ROW_FAST - 1);
  for (int j = 0; j < nr; ++j) {
    const int meta = __builtin_amdgcn_readfirstlane(s_rg[j]);
    const int g = meta & (GRP_ROW_FAST - 1);
    if (g != gcur) {  // wave-uniform
      grp_flush(acc, cnt, (int64_t)gcur * S + s, live, sum, z);
      if constexpr (SPREAD) {
        if (qmin && live) atomicMin(qmin + (int64_t)gcur * S + s, (unsigned long long)mn ^ SPREAD_SIGN);
        mn = INT64_MAX;
      }
      if constexpr (WHY) why_flush<R>(why_rows, why_pods, cells, (int64_t)gcur * S + s, live, wr, wp);
      sum = 0;
      z = 0;
      gcur = g;
    }
    const GrpRow r = s_rec[j];
    int64_t q;
    [[maybe_unused]] int b = 0;  // WHY: the term that holds q (the selects below are findMin's tie rule)
    if (wave_fast && (meta & GRP_ROW_FAST)) {  // wave-uniform
      const double tc = grp_div(r.fcd, cd, rc);
      const double tm = grp_div(r.fmd, md, rm);
      double t = tc <= tm ? tc : tm;  // findMin (CC:133)
      if constexpr (WHY) b = tc <= tm ? 0 : 1;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const double tx = grp_div(s_x[j * RR + k].fxd, xd[k], rx[k]);
        if constexpr (WHY) b = (x[k] != 0 && tx < t) ? 2 + k : b;
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
      if constexpr (WHY) b = qc <= qm ? 0 : 1;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int64_t fx = s_x[j * RR + k].fx;
        if (x[k] != 0) {  // zero: not requested
          int64_t qx = 0;
          if (fx != 0) qx = x[k] == -1 ? (int64_t)(0ull - (uint64_t)fx) : fx / x[k];
          if constexpr (WHY) b = q <= qx ? b : 2 + k;
          q = q <= qx ? q : qx;
        }
      }
      z += dz ? 1u : 0u;
    }
    if constexpr (WHY) b = q >= r.P ? R + 2 : b;
    if (q >= r.P) q = r.cl;  // CC:134-136, after all the mins
    if constexpr (SPREAD) {
      mn = q < mn ? q : mn;      // the cell's minimum: before the cap
      if constexpr (WHY) b = q > capv ? R + 3 : b;
      q = q > capv ? capv : q;   // at most node_cap[s] on one node: after the clamp
    }
    sum = (int64_t)((uint64_t)sum + (uint64_t)q);
    if constexpr (WHY) {
#pragma unroll
      for (int k = 0; k < R + 4; ++k) {  // static indices: the arrays stay in registers
        wr[k] += b == k ? 1u : 0u;
        wp[k] += b == k ? (uint64_t)q : 0ull;
      }
    }
  }
  grp_flush(acc, cnt, (int64_t)gcur * S + s, live, sum, z);
  if constexpr (SPREAD) {
    if (qmin && live) atomicMin(qmin + (int64_t)gcur * S + s, (unsigned long long)mn ^ SPREAD_SIGN);
  }
  if constexpr (WHY) why_flush<R>(why_rows, why_pods, cells, (int64_t)gcur * S + s, live, wr, wp);
}

// The pair loop's launch: kernel is ext_pairs_kernel<R>, or cap_pairs_kernel<R> with its two
// last arguments (node_cap, qmin) in tail.  The caller has passed ext_sizes_ok.
template <class Kernel, class... Tail>
inline hipError_t launch_pairs(Kernel kernel, const FitNodes& nd, const FitSpecs& sp,
                               const ExtWork& w, hipStream_t s, Tail... tail) {
  const int64_t sblocks = grp_sblocks(sp.S);
  hipLaunchKernelGGL(kernel, dim3((unsigned)(grp_runs(nd.n) * sblocks)), dim3(GRP_PAIR_THREADS), 0,
                     s, nd.group ? w.g.total : (const uint32_t*)nullptr, nd.n, sp.S, sblocks,
                     sp.spec_cpu, sp.spec_mem, sp.spec_x, w.g.rec, w.xrec, w.g.rg, w.g.acc,
                     w.g.cnt(nd.G * sp.S), tail...);
  return hipGetLastError();
}
#endif

// ---- spread constraints in the fit (kcc_spread.hip) ----------------
// kcc_fit_capped: launch_fit_ext with sp.node_cap, qmin [G S] (workspace of cell_min; unused
// when cell_min is nullptr), and the nullable outputs cell_min [G S] and group_rows [G].
// node_cap and cell_min both nullptr: the launches of launch_fit_ext themselves.
hipError_t launch_fit_capped(const FitNodes& nd, const FitSpecs& sp, const ExtWork& w,
                             unsigned long long* qmin, int64_t* totals, int32_t* spec_err,
                             int64_t* cell_min, int64_t* group_rows, hipStream_t s);
// group_rows alone (no specs): grp_hist's counts widened; group == nullptr: out[0] = n.
hipError_t launch_group_rows(int64_t n, int64_t G, const int32_t* group, const GrpWork& w,
                             int64_t* group_rows, hipStream_t s);
// out[0 .. cells) = v (the cells of cell_min when there are no rows).
hipError_t launch_fill_i64(int64_t cells, int64_t v, int64_t* out, hipStream_t s);
// kcc_spread_fold: G x S cells to one total per spec.  G, S, D >= 1; G S, D S <= 2^28.
struct FoldWork {
  int64_t* cap;       // [D S] wrapping sum of the live cells of domain d, spec s
  uint32_t* present;  // [D S] nonzero: domain d has a live group for spec s
  uint32_t* flag;     // [S] nonzero: a live cell of spec s is flagged
};
hipError_t launch_spread_fold(int64_t G, int64_t S, const int64_t* cell_totals,
                              const int32_t* cell_err, const int64_t* group_rows,
                              const int32_t* domain_of, int64_t D, const uint8_t* eligible,
                              const int64_t* max_skew, const FoldWork& w, int64_t* totals,
                              int32_t* spec_err, hipStream_t s);

// ---- the fit explained (kcc_explain.hip) ---------------------------
// kcc_fit_explain: launch_fit_capped's totals / spec_err and three nullable plane-major
// outputs: why_rows / why_pods [WHY_SLOTS][G S] (rows and replicas of each cell by the term
// that holds the row's q) and left [2 + R][G S] (what stays free: per group the free amounts
// summed, less request x total).  free: [(2 + R) G] workspace of left.  All three nullptr:
// the launches of launch_fit_capped themselves.  why_rows / why_pods are zeroed here and
// accumulated into directly; the finalize zeroes the flagged cells.
constexpr int WHY_FREE_IPL = 16;  // records per lane of why_free (a wave: 64 x 16, lane-strided)
hipError_t launch_fit_explain(const FitNodes& nd, const FitSpecs& sp, const ExtWork& w,
                              unsigned long long* free, int64_t* totals, int32_t* spec_err,
                              int64_t* why_rows, int64_t* why_pods, int64_t* left, hipStream_t s);

// ---- a rollout plan committed to the node rows (kcc_deploy.hip) ------
// Rows in tiles of DEPLOY_TILE: 256 threads x DEPLOY_IPT consecutive rows (kcc_deploy.hip).
// The tile sums (at most 2^21 of them) are scanned by one workgroup, DEPLOY_SCAN_PASS a pass.
constexpr int DEPLOY_IPT = 4;
constexpr int DEPLOY_TILE = 256 * DEPLOY_IPT;  // 1024 (_lib.KCC_DEPLOY_TILE restates it)
constexpr int DEPLOY_SCAN_PASS = 256;          // (_lib.KCC_DEPLOY_SCAN_PASS)
constexpr int64_t DEPLOY_R_MAX = 0x7fffffff;   // replicas[k] is clamped to [0, this]
constexpr int DEPLOY_PACK = 0, DEPLOY_SPREAD = 1;  // include/kcc.h KCC_DEPLOY_*
constexpr int64_t DEPLOY_MAX_STEPS = (int64_t)1 << 20;
// Per step: a flag word (an eligible row would panic), the digit search's state after each of
// its four rounds (prefix, sum of a below it, rows above it, f at the prefix) and the four
// rounds' 256 bins of (count, sum of a).
constexpr int DEPLOY_FLAG_STRIDE = 16;  // uint32 words: one 64-B line per step
constexpr int DEPLOY_ST_WORDS = 4;
constexpr int64_t DEPLOY_BIN_WORDS = 4 * 256 * 2;
inline int64_t deploy_tiles(int64_t n) { return (n + DEPLOY_TILE - 1) / DEPLOY_TILE; }
struct DeployPlan {
  int64_t K;
  const uint64_t* spec_cpu;   // [K]
  const int64_t* spec_mem;    // [K]
  const int64_t* spec_x;      // [R, K]
  const int64_t* replicas;    // [K]
  const int64_t* node_cap;    // [K], nullable; <= 0: no cap
  int policy;                 // DEPLOY_PACK / DEPLOY_SPREAD
};
struct DeployWork {
  uint32_t* a;         // [n] what row i can take of the step at most (< 2^31)
  uint64_t* tile_sum;  // [deploy_tiles(n)]
  uint64_t* tile_off;  // [deploy_tiles(n)] exclusive scan of tile_sum
  uint32_t* flag;      // [K * DEPLOY_FLAG_STRIDE]
  uint64_t* st;        // [K][4][DEPLOY_ST_WORDS]
  uint64_t* bins;      // [K][DEPLOY_BIN_WORDS] (DEPLOY_SPREAD alone)
};
// n, K, G >= 1, 0 <= R <= EXT_MAX, n <= GRP_MAX_NODES, G K <= GRP_MAX_CELLS, K <=
// DEPLOY_MAX_STEPS.
inline bool deploy_sizes_ok(const FitNodes& nd, int64_t K) {
  if (nd.n <= 0 || K <= 0 || nd.G <= 0 || nd.R < 0 || nd.R > EXT_MAX || (!nd.group && nd.G != 1))
    return false;
  return nd.n <= GRP_MAX_NODES && K <= DEPLOY_MAX_STEPS && nd.G <= GRP_MAX_CELLS &&
         nd.G * K <= GRP_MAX_CELLS;
}
#if defined(__HIPCC__)
// What one row can take of one deploy step, before the per-node cap and the replica count:
// kcc_fit_ext's q on the row's current state (64-bit integer arithmetic), the pod-slot clamp
// after all the mins (CC:134-136), a negative value counted as 0.  z: the row would panic (a
// zero cpu or memory request against free CPU or memory); the value returned is then not used.
// load_x(r, ax, ux) fetches the row's allocatable and used amounts of extra resource r, and is
// called for the requested resources alone.  The one copy of the step arithmetic: dp_rows
// (kcc_deploy.hip) and the removal what-if's walk (kcc_consolidate.hip) both call it.
template <int R, class LoadX>
__device__ inline int64_t deploy_row_q(uint64_t ac, uint64_t uc, int64_t am, int64_t um, int64_t P,
                                       int64_t pc, uint64_t c, int64_t m, const int64_t* x,
                                       LoadX&& load_x, bool& z) {
  z = false;
  int64_t qc = 0, qm = 0;
  if (ac > uc) {  // CC:119-124 (uint64 compare and division, int() reinterprets)
    if (c == 0) z = true;
    else qc = (int64_t)((ac - uc) / c);
  }
  if (am > um) {  // CC:125-130 (int64, the difference wraps)
    const int64_t fm = (int64_t)((uint64_t)am - (uint64_t)um);
    if (m == 0) z = true;
    else if (m == -1) qm = (int64_t)(0ull - (uint64_t)fm);  // MinInt64 / -1 == MinInt64
    else qm = fm / m;
  }
  int64_t q = qc <= qm ? qc : qm;  // findMin, CC:133
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (x[r] != 0) {  // zero: not requested
      int64_t ax, ux;
      load_x(r, ax, ux);
      int64_t qx = 0;
      if (ax > ux) {
        const int64_t fx = (int64_t)((uint64_t)ax - (uint64_t)ux);
        qx = x[r] == -1 ? (int64_t)(0ull - (uint64_t)fx) : fx / x[r];
      }
      q = q <= qx ? q : qx;
    }
  }
  if (q >= P) q = (int64_t)((uint64_t)P - (uint64_t)pc);  // CC:134-136, after all the mins
  return q < 0 ? 0 : q;                                   // a negative clamp value holds nothing
}
#endif
// The plan's K steps on s, in order.  nd's pod_count / used_* are not read: the state arrays
// are the four pointers after it, updated in place.  placed / nodes_used / step_err [K] are
// written; placed_rows [K n] is nullable.  eligible [G K] uint8, nullable.
hipError_t launch_deploy(const FitNodes& nd, int64_t* pod_count, uint64_t* used_cpu, int64_t* used_mem,
                         int64_t* used_x, const uint8_t* eligible, const DeployPlan& plan,
                         const DeployWork& w, int64_t* placed, int64_t* nodes_used,
                         int32_t* step_err, int64_t* placed_rows, hipStream_t s);

// ---- drain what-if: the pods of drained rows as a deploy plan (kcc_drain.hip)
constexpr int64_t DRAIN_MAX_SHAPES = 4096;                     // include/kcc.h KCC_DRAIN_MAX_SHAPES
constexpr int64_t DRAIN_MAX_PODS = ((int64_t)1 << 31) - 4096;  // a slot holds a pod index (int32)
// the call's counters, zeroed by launch_drain_scan: drained rows, evicted pods, claimed
// slots, and the overflow word (more than max_shapes shapes, or a probe that found no slot)
enum { DRAIN_META_ROWS = 0, DRAIN_META_EVICTED = 1, DRAIN_META_CLAIMED = 2, DRAIN_META_OVERFLOW = 3,
       DRAIN_META_WORDS = 8 };
// slots of the shape table: a power of two, at least twice max_shapes and one workgroup's 256
inline int64_t drain_table(int64_t max_shapes) {
  int64_t T = 256;
  while (T < 2 * max_shapes) T <<= 1;
  return T;
}
struct DrainPods {
  int64_t P;
  const int64_t* node_pod_ptr;  // [n + 1], clamped into [0, P] where read
  const uint64_t* pod_cpu;      // [P]
  const int64_t* pod_mem;       // [P]
  const int64_t* pod_x;         // [R, P], nullable: zeros
  const uint8_t* movable;       // [P], nullable: every pod movable
};
struct DrainWork {
  int32_t* rep;               // [drain_table(M)] a slot's representative pod (-1: empty)
  uint32_t* cnt;              // [drain_table(M)] the slot's pods
  unsigned long long* meta;   // [DRAIN_META_WORDS]
  // the plan kcc::launch_deploy reads (M = max_shapes entries each, plan_x [R, K]) and the
  // steps' outputs
  uint64_t* plan_cpu;
  int64_t* plan_mem;
  int64_t* plan_x;
  int64_t* plan_rep;
  int64_t* placed;
  int64_t* nodes_used;
  int32_t* step_err;
};
struct DrainOut {
  int64_t* summary;  // [4]
  uint64_t* shape_cpu;
  int64_t* shape_mem;
  int64_t* shape_x;  // [R, M]
  int64_t* shape_count;
  int64_t* shape_placed;
  int64_t* shape_nodes;
  int32_t* shape_err;
};
// The table and counters reset, dr_rows (the drained rows of the four state arrays left full)
// and dr_pods.  nd.n >= 1; nd's pod_count / used_* are not read.
hipError_t launch_drain_scan(const FitNodes& nd, int64_t* pod_count, uint64_t* used_cpu,
                             int64_t* used_mem, int64_t* used_x, const uint8_t* drain,
                             const DrainPods& pods, int64_t max_shapes, const DrainWork& w,
                             hipStream_t s);
// dr_plan: the shape key outputs [max_shapes] and a plan of K <= max_shapes steps (K >= D; the
// steps behind D are padding steps).  On overflow every step is a padding step.
hipError_t launch_drain_plan(int64_t R, const DrainPods& pods, int64_t max_shapes, int64_t K,
                             const DrainWork& w, const DrainOut& out, hipStream_t s);
// dr_finish: the steps' outputs masked to j < D, and the summary.
hipError_t launch_drain_finish(int64_t max_shapes, const DrainWork& w, const DrainOut& out,
                               hipStream_t s);

// ---- removal what-if: each candidate row's pods re-placed on the rest (kcc_consolidate.hip,
// DESIGN.md §4.16)
constexpr int CONS_MAX_PODS = 1024;  // include/kcc.h KCC_CONS_MAX_PODS: a candidate's evicted pods
constexpr int CONS_THREADS = 256;
constexpr int CONS_IPT = 4;          // rows of a chunk per thread, CONS_THREADS apart
constexpr int CONS_CHUNK = CONS_THREADS * CONS_IPT;  // 1024 (_lib.KCC_CONS_CHUNK restates it)
constexpr int32_t CAND_OK = 0, CAND_BADROW = 1, CAND_TOOMANY = 2;  // include/kcc.h KCC_CAND_*
constexpr int64_t CONS_MAX_CAND = ((int64_t)1 << 31) - 4096;       // one workgroup per candidate
struct ConsOut {
  int64_t* evicted;     // [C]
  int64_t* placed;      // [C]
  int64_t* zero;        // [C]
  int32_t* err;         // [C]
  int64_t* pod_target;  // [P], nullable
};
// pod_target (when given) filled with -2, then one workgroup per candidate.  nd.n, C >= 1; nd's
// six state / allocatable arrays and alloc_x / used_x are read, nothing of them is written;
// nd.group is not read.
hipError_t launch_consolidate(const FitNodes& nd, const uint8_t* target, const DrainPods& pods,
                              int64_t C, const int64_t* cand, const ConsOut& out, hipStream_t s);

// ---- opt-in scheduler request model (kcc_pods.hip) ---------------
hipError_t launch_pod_requests(int64_t n_pods, int64_t n_cont, int64_t n_init,
                               const int64_t* pod_ptr, const uint64_t* cpu_req,
                               const int64_t* mem_req, const int64_t* init_ptr,
                               const uint64_t* init_cpu, const int64_t* init_mem,
                               const uint8_t* restartable, const uint64_t* ovh_cpu,
                               const int64_t* ovh_mem, uint64_t* pod_cpu, int64_t* pod_mem,
                               hipStream_t s);

// ---- preemption what-if (kcc_levels.hip) ---------------------------
constexpr int LEVELS_MAX = 8;     // include/kcc.h KCC_LEVELS_MAX
constexpr int LV_WG = 256;        // pods per tile: one lane each
constexpr int LV_TILES_MAX = 8;   // consecutive tiles of one workgroup, at most
constexpr int LV_MIN_GRID = 256;  // workgroups the grid keeps before a workgroup takes more tiles
// kcc_reduce_requests_levels: used_cpu / used_mem / pod_count [L, N], plane l the pods with
// min(pod_level, L - 1) >= l.  The three outputs are zeroed on s first; offsets are clamped.
// N <= 0: nothing; n_pods == 0: the zeroes.  1 <= L <= LEVELS_MAX.
hipError_t launch_levels_reduce(int64_t N, int64_t n_pods, int64_t n_cont, int L,
                                const int64_t* node_pod_ptr, const int64_t* pod_ptr,
                                const uint64_t* cpu_req, const int64_t* mem_req,
                                const uint8_t* pod_level, uint64_t* used_cpu, int64_t* used_mem,
                                int64_t* pod_count, hipStream_t s);
// kcc_fit_levels: the specs' level offsets (host values, passed to the kernels by value).
struct LevelPtr {
  int L;
  int64_t ptr[LEVELS_MAX + 1];
};
// spec_x [R, S] to one [R, S_l] block per level, level l's at packed + R * lp.ptr[l].
hipError_t launch_cells_pack_x(int64_t R, int64_t S, const LevelPtr& lp, const int64_t* spec_x,
                               int64_t* packed, hipStream_t s);
// cell_tot / cell_err [G, Sl] to columns col0 .. col0 + Sl of totals / spec_err [G, S].
hipError_t launch_cells_place(int64_t G, int64_t S, int64_t Sl, int64_t col0,
                              const int64_t* cell_tot, const int32_t* cell_err, int64_t* totals,
                              int32_t* spec_err, hipStream_t s);

}  // namespace kcc
