// kcc_abi.cpp — the C-ABI of libkcc.so (include/kcc.h): contexts, device
// workspaces, host<->device staging, node sharding over devices and the RCCL
// all-reduce of per-spec totals.  No CPU compute path: every result comes from
// the gfx950 kernels in kcc_kernels.hip.
#include "kcc.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kcc_internal.h"

namespace {

// A device allocation and its owner: move-only, freed with the object (the context's
// teardown has synchronised the streams by then).  It only ever grows (ensure).
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) {
    o.p = nullptr;
    o.bytes = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      bytes = o.bytes;
      o.p = nullptr;
      o.bytes = 0;
    }
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

hipError_t ensure(DevBuf& b, size_t bytes) {
  if (bytes == 0) bytes = 16;
  if (b.bytes >= bytes) return hipSuccess;
  b.release();
  hipError_t e = hipMalloc(&b.p, bytes);
  if (e == hipSuccess) b.bytes = bytes;
  return e;
}

// Fine-grained, uncached device memory (the p2p mailbox): peers write it over xGMI while
// this device's kernel polls it, and a line of ordinary (coarse-grained) memory may be
// served stale from this device's L2 — coarse-grained memory is only coherent with other
// devices at synchronisation points.  Uncached loads and stores go to memory.
hipError_t ensure_uncached(DevBuf& b, size_t bytes) {
  if (bytes == 0) bytes = 16;
  if (b.bytes >= bytes) return hipSuccess;
  b.release();
  hipError_t e = hipExtMallocWithFlags(&b.p, bytes, hipDeviceMallocUncached);
  if (e == hipSuccess) b.bytes = bytes;
  return e;
}

template <class T>
T* as(DevBuf& b) {
  return static_cast<T*>(b.p);
}

// Timing of the pipelined entry point (kcc_profile_*): event pairs recorded around each
// reduce (side stream) and each fit launch (caller stream), read back on demand.
struct ProfPair {
  hipEvent_t a, b;
  int kind;  // 0 reduce (mark + reduce), 1 fit
};

struct Dev {
  int device = 0;
  hipStream_t stream = nullptr;
  // pipelined capacity (kcc_capacity_partial_async): node chunk k's reduce runs on `side`
  // while the caller's stream fits chunk k-1
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr;
  hipEvent_t ev_red[kcc::FIT_MAX_CHUNKS] = {};
  bool prof_on = false;
  std::vector<ProfPair> prof_pending;
  std::vector<hipEvent_t> prof_free;
  double prof_ms[2] = {0.0, 0.0};
  int64_t prof_n[2] = {0, 0};
  // workspace of the *_async entry points
  DevBuf fast_a, fast_b, slow, slow_list, srec, sperm, counters;
  // the reduce's per-wave tail records (look-back): zeroed when allocated, and every
  // launch leaves their tags 0 (each record is cleared by the wave that consumes it)
  DevBuf red_tail;
  // the device's fault words (kcc::FAULT_*): reduce look-back / exchange flag waits that
  // gave up; sticky until kcc_clear_faults
  DevBuf faults;
  DevBuf rank_arrive;  // spec_rank's per-query-block arrival counters (zero between calls)
  DevBuf fit_q;          // the fit's per-column work queues (zero between launches)
  bool fitq_dirty = true;
  // spec setup + clamp correction (kcc::ClampWork)
  DevBuf c_rank, c_bcnt, c_cs, c_ms, c_mrc, c_crm, c_dperm;
  DevBuf c_C, c_H2, c_H3, c_Crow, c_rec, c_dir;
  // the table copies C / H2 / H3 not known to be all zero (fresh allocation or an
  // interrupted call)
  bool clamp_dirty = true;
  int64_t last_pairs = 0;  // node x spec pairs of the last fit_prepare on this device
  int64_t c_stride = 0;    // cells per copy of the clamp table C
  int64_t h_stride = 0;    // cells per copy of the clamp tables H2 / H3
  int64_t d_stride = 0;    // words per pass of the binned records' directory
  bool fit_dense = false;  // kcc_set_fit_dense: stream every node row through the fit
  int clamp_in_fit = -1;   // kcc_set_clamp_in_fit: -1 by size (clamp_in_fit_auto), 0 never, 1 always
  bool last_nc = false;    // the last capacity call applied the clamp in the fit
  DevBuf fast_cl;          // the clamp in the fit: each streamed row's clamp value
  int stream_chunks = 0;   // node chunks of the last fit prepare (their stream counters)
  int64_t prep_nodes = -1, prep_specs = -1;  // sizes the workspace was last prepared for
  // staging of the host-array entry points (Stage): the k-th array a call stages takes slot
  // k; the slots only grow, and a synchronous call has let go of them when it returns
  std::vector<DevBuf> slots;
  DevBuf partial;                                         // the fit's per-spec partials [2 S] per shard
  DevBuf g_count, g_cursor, g_total, g_rec, g_rg, g_acc;  // kcc::GrpWork (grouped fit)
  DevBuf x_rec;                    // kcc::ExtWork::xrec (the other buffers are GrpWork's)
  DevBuf sp_qmin;                  // kcc_fit_capped: the pre-finalize minima [G S]
  DevBuf ex_free;                  // kcc_fit_explain: the groups' free amounts [(2 + R) G]
  DevBuf lv_tot, lv_err, lv_x;     // kcc_fit_levels: one level's cells [G S_l], spec_x by level
  DevBuf f_cap, f_present, f_flag;   // kcc::FoldWork (kcc_spread_fold)
  DevBuf dp_a, dp_tsum, dp_toff, dp_flag, dp_st, dp_bins;  // kcc::DeployWork (kcc_deploy)
  DevBuf dr_tab, dr_plan;  // kcc::DrainWork (kcc_drain): meta / cnt / rep; the plan and its outputs
  DevBuf kb_counts, kb_tot, kb_sr, kb_sv;  // kcc::KeyedWork (bucketed keyed reduce)
  DevBuf kb_part, kb_arrive;               // one-sweep gather: part rows, arrivals (zeroed)
  DevBuf kb_esc_n, kb_esc_row, kb_esc_cpu, kb_esc_mem;
  // one-shot exchange over xGMI peer memory (kcc_p2p_*): this rank's mailbox (exported),
  // the push arrival counter (u32 word 0) and the last pushed epoch (u64 word 1, advanced
  // by the kernel); the peers' mapped mailboxes
  DevBuf p2p_mbox, p2p_arrive;
  DevBuf clamp_arrive;  // clamp_apply's fused finalize: arrivals (zero between launches)
  DevBuf np_sync;       // node prep in the reduce launch: epoch and flag words (NpArgs::sync)
  unsigned char* p2p_peer[kcc::P2P_MAX_RANKS] = {};  // opened peer mailboxes (own: p2p_mbox)
  int p2p_W = 0, p2p_rank = -1;
  int64_t p2p_smax = 0;
  bool p2p_ready = false;
};

}  // namespace

struct kcc_ctx {
  std::vector<Dev> devs;
  std::vector<ncclComm_t> comms;  // in-process devices (kcc_create with n_gpus > 1)
  ncclComm_t proc_comm = nullptr;  // one rank of a multi-process run (kcc_comm_init)
  int proc_ranks = 0, proc_rank = 0;
  int node_shards = 0;  // host-array entry points: node shards (0 = one per device)
  std::string err;
  double slow_frac = -1.0;
  // kcc_fit / kcc_capacity: each shard's counters, copied into pinned host memory on the
  // shard's stream (pageable copies could block the host between devices) and summed
  // after the final synchronisation: exact-path pairs and streamed rows of every shard
  unsigned long long* host_cnt = nullptr;
  size_t host_cnt_n = 0;
  int64_t host_stream_rows = -1;  // streamed rows of the last host-array fit (-1: none)
  // the in-library all-reduce (comms) has been checked against a host-side sum of the
  // devices' partials (the first host-array call of the context does it)
  bool allreduce_verified = false;
  bool allreduce_verify_every = false;  // kcc_set_allreduce_verify(ctx, 1)
};

namespace {

thread_local std::string g_create_error;

int fail(kcc_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

#define KCC_HIP(ctx, expr)                                                              \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail((ctx), e_ == hipErrorOutOfMemory ? KCC_ENOMEM : KCC_EHIP,             \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                   \
  } while (0)

#define KCC_NCCL(ctx, expr)                                                             \
  do {                                                                                  \
    ncclResult_t r_ = (expr);                                                           \
    if (r_ != ncclSuccess)                                                              \
      return fail((ctx), KCC_ERCCL, std::string(#expr) + ": " + ncclGetErrorString(r_)); \
  } while (0)

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// CSR sanity on the host (the host-array entry points): a malformed offset array is
// rejected here instead of reaching the device.
int check_csr(kcc_ctx* ctx, int64_t n_nodes, int64_t n_cont, const int64_t* ptr) {
  if (n_nodes < 0 || n_cont < 0) return fail(ctx, KCC_EINVAL, "negative size");
  if (n_nodes == 0) {
    if (n_cont != 0) return fail(ctx, KCC_EINVAL, "containers without nodes");
    return KCC_OK;
  }
  if (!ptr) return fail(ctx, KCC_EINVAL, "node_ptr is NULL");
  if (ptr[0] != 0) return fail(ctx, KCC_EINVAL, "node_ptr[0] != 0");
  for (int64_t i = 0; i < n_nodes; ++i)
    if (ptr[i + 1] < ptr[i]) return fail(ctx, KCC_EINVAL, "node_ptr is not non-decreasing");
  if (ptr[n_nodes] != n_cont) return fail(ctx, KCC_EINVAL, "node_ptr[n_nodes] != n_containers");
  return KCC_OK;
}

// Entries of a CSR offset array that are read: none without rows (check_csr asks for no
// array then).
int64_t csr_len(int64_t n) { return n > 0 ? n + 1 : 0; }

// Contiguous node ranges, balanced by node count (the fit dominates).
void shard_nodes(int64_t n_nodes, int n, std::vector<int64_t>& lo, std::vector<int64_t>& hi) {
  lo.resize(n);
  hi.resize(n);
  for (int d = 0; d < n; ++d) {
    lo[d] = n_nodes * d / n;
    hi[d] = n_nodes * (d + 1) / n;
  }
}

// ---- device-level pipeline pieces (no host sync, no allocation beyond growth) ----

// The device's fault words, zeroed when allocated (synchronously: kcc_reserve does it
// ahead of any capture).
int faults_ws(kcc_ctx* ctx, Dev& dv, hipStream_t s) {
  if (dv.faults.p) return KCC_OK;
  KCC_HIP(ctx, ensure(dv.faults, 8 * kcc::FAULT_WORDS));
  KCC_HIP(ctx, hipMemsetAsync(dv.faults.p, 0, 8 * kcc::FAULT_WORDS, s));
  KCC_HIP(ctx, hipStreamSynchronize(s));
  return KCC_OK;
}

// The reduce's look-back workspace: tail records for every wave a launch may have, zeroed
// when (re)allocated — synchronously: a stale tag would hand a wave a piece that was
// never published (allocation happens only when the workspace grows; kcc_reserve does it
// ahead of any capture).  Every launch leaves the tags 0.
int reduce_ws(kcc_ctx* ctx, Dev& dv, hipStream_t s) {
  const size_t tb = sizeof(uint64_t) * kcc::RED_TAIL_WORDS * (size_t)kcc::reduce_tail_records();
  if (dv.red_tail.bytes < tb) {
    KCC_HIP(ctx, ensure(dv.red_tail, tb));
    KCC_HIP(ctx, hipMemsetAsync(dv.red_tail.p, 0, dv.red_tail.bytes, s));
    KCC_HIP(ctx, hipStreamSynchronize(s));
  }
  return faults_ws(ctx, dv, s);
}

// After a synchronous entry point's final synchronisation: a set fault word means some
// wait of this (or an earlier, async) call gave up and results are not trustworthy.
int check_faults(kcc_ctx* ctx) {
  unsigned long long red = 0, p2p = 0;
  for (Dev& dv : ctx->devs) {
    if (!dv.faults.p) continue;
    unsigned long long f[2] = {0, 0};
    KCC_HIP(ctx, hipSetDevice(dv.device));
    KCC_HIP(ctx, hipMemcpy(f, dv.faults.p, sizeof(f), hipMemcpyDeviceToHost));
    red += f[kcc::FAULT_RED];
    p2p += f[kcc::FAULT_P2P];
  }
  if (red == 0 && p2p == 0) return KCC_OK;
  return fail(ctx, KCC_EFAULT,
              "device fault: " + std::to_string(red) + " reduce-side wait(s) (look-back, node prep, keyed gather) and " +
                  std::to_string(p2p) +
                  " exchange flag wait(s) gave up; results are not valid (every spec is marked "
                  "KCC_SPEC_FAULT) until kcc_clear_faults");
}

// One host-array call's staging on dv.stream.  The k-th array the call stages takes
// dv.slots[k].  Every operation takes a nullable host pointer and a count, and leaves the
// pointer naming the device copy: NULL stays NULL, a count of 0 copies nothing.
class Stage {
 public:
  Stage(kcc_ctx* ctx, Dev& dv) : ctx_(ctx), dv_(dv) {}

  template <class T>
  int in(const T*& p, int64_t count) {  // an input: copied to its slot
    if (!p) return KCC_OK;
    const size_t bytes = size_of<T>(count);
    void* d = nullptr;
    const int rc = slot(bytes, &d);
    if (rc) return rc;
    if (bytes) KCC_HIP(ctx_, hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, dv_.stream));
    p = static_cast<const T*>(d);
    return KCC_OK;
  }
  template <class T>
  int out(T*& p, int64_t count) {  // an output: finish() copies its slot back
    if (!p) return KCC_OK;
    T* const host = p;
    const int rc = tmp(p, count);
    if (!rc && count > 0) back_.push_back({host, p, size_of<T>(count)});
    return rc;
  }
  template <class T>
  int inout(T*& p, int64_t count) {  // state the call updates in place: both of the above
    T* const host = p;
    const T* d = p;
    const int rc = in(d, count);
    if (!rc && host && count > 0) back_.push_back({host, d, size_of<T>(count)});
    p = const_cast<T*>(d);
    return rc;
  }
  template <class T>
  int tmp(T*& p, int64_t count) {  // device only: one launch's output, the next one's input
    void* d = nullptr;
    const int rc = slot(size_of<T>(count), &d);
    p = static_cast<T*>(d);
    return rc;
  }
  // Back to slot 0 (run_host, per node shard: a device's shards reuse the same slots, in
  // stream order).
  void rewind() { next_ = 0; }
  // Every output back to the host, then the call's one synchronisation.
  int finish(bool faults = false) {
    for (const Back& b : back_)
      KCC_HIP(ctx_, hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, dv_.stream));
    back_.clear();
    KCC_HIP(ctx_, hipStreamSynchronize(dv_.stream));
    return faults ? check_faults(ctx_) : KCC_OK;
  }

 private:
  struct Back {
    void* host;
    const void* dev;
    size_t bytes;
  };
  template <class T>
  static size_t size_of(int64_t count) {
    return sizeof(T) * (size_t)(count > 0 ? count : 0);
  }
  int slot(size_t bytes, void** d) {
    if (next_ == dv_.slots.size()) dv_.slots.emplace_back();
    DevBuf& b = dv_.slots[next_++];
    KCC_HIP(ctx_, ensure(b, bytes));
    *d = b.p;
    return KCC_OK;
  }
  kcc_ctx* ctx_;
  Dev& dv_;
  size_t next_ = 0;
  std::vector<Back> back_;
};

// Argument checks of the reduce's two entry points (host or device pointers alike).
int check_reduce(kcc_ctx* ctx, int64_t n_nodes, int64_t n_cont, const int64_t* ptr,
                 const uint64_t* cpu, const int64_t* mem, const uint64_t* cpul,
                 const int64_t* meml, const uint64_t* used_cpu, const int64_t* used_mem,
                 const uint64_t* lim_cpu, const int64_t* lim_mem) {
  if (n_nodes < 0 || n_cont < 0) return fail(ctx, KCC_EINVAL, "negative size");
  if (n_nodes == 0) return n_cont == 0 ? KCC_OK : fail(ctx, KCC_EINVAL, "containers without nodes");
  if (n_nodes >= kcc::RED_MAX_NODES)
    return fail(ctx, KCC_EINVAL, "too many nodes per device (max 2^28 - 1)");
  if (!ptr || !used_cpu || !used_mem) return fail(ctx, KCC_EINVAL, "NULL node_ptr/output");
  if (n_cont > 0 && (!cpu || !mem)) return fail(ctx, KCC_EINVAL, "NULL cpu_req/mem_req");
  if ((cpul || meml) && (!cpul || !meml || !lim_cpu || !lim_mem))
    return fail(ctx, KCC_EINVAL, "limits need cpu_lim, mem_lim, lim_cpu and lim_mem");
  return KCC_OK;
}

int reduce_async_dev(kcc_ctx* ctx, Dev& dv, int64_t n_nodes, int64_t n_cont, const int64_t* ptr,
                     const uint64_t* cpu, const int64_t* mem, const uint64_t* cpul,
                     const int64_t* meml, uint64_t* used_cpu, int64_t* used_mem,
                     uint64_t* lim_cpu, int64_t* lim_mem, hipStream_t s) {
  int rc = check_reduce(ctx, n_nodes, n_cont, ptr, cpu, mem, cpul, meml, used_cpu, used_mem,
                        lim_cpu, lim_mem);
  if (rc || n_nodes == 0) return rc;
  const bool lim = cpul != nullptr;
  if (!aligned16(cpu) || !aligned16(mem) || (lim && (!aligned16(cpul) || !aligned16(meml))))
    return fail(ctx, KCC_EINVAL, "container arrays must be 16-byte aligned");
  if ((rc = reduce_ws(ctx, dv, s))) return rc;
  KCC_HIP(ctx, kcc::launch_reduce(n_nodes, 0, n_cont, ptr, cpu, mem, lim ? cpul : nullptr,
                                  lim ? meml : nullptr, used_cpu, used_mem, lim ? lim_cpu : nullptr,
                                  lim ? lim_mem : nullptr, as<uint64_t>(dv.red_tail),
                                  as<unsigned long long>(dv.faults), s));
  return KCC_OK;
}

kcc::SpecPrep spec_prep_of(Dev& dv) {
  kcc::SpecPrep sp;
  sp.rec = as<kcc::SpecRec>(dv.srec);
  sp.perm = as<int32_t>(dv.sperm);
  return sp;
}

int reserve_dev(kcc_ctx* ctx, Dev& dv, int64_t n_nodes, int64_t n_cont, int64_t n_specs) {
  KCC_HIP(ctx, hipSetDevice(dv.device));
  const size_t N = (size_t)(n_nodes > 0 ? n_nodes : 1);
  const size_t S = (size_t)(n_specs > 0 ? n_specs : 1);
  (void)n_cont;  // the reduce's workspace does not depend on the container count
  {
    int rc = reduce_ws(ctx, dv, dv.stream);
    if (rc) return rc;
  }
  KCC_HIP(ctx, ensure(dv.fast_a, sizeof(kcc::FitGroupA) * (size_t)kcc::fit_groups((int64_t)N)));
  KCC_HIP(ctx, ensure(dv.fast_b, sizeof(kcc::FitGroup) * (size_t)kcc::fit_groups((int64_t)N)));
  KCC_HIP(ctx, ensure(dv.fast_cl, sizeof(int32_t) * kcc::FIT_GROUP * (size_t)kcc::fit_groups((int64_t)N)));
  KCC_HIP(ctx, ensure(dv.slow, sizeof(kcc::SlowNode) * N));
  KCC_HIP(ctx, ensure(dv.slow_list, sizeof(int64_t) * N));
  KCC_HIP(ctx, ensure(dv.srec, sizeof(kcc::SpecRec) * S));
  KCC_HIP(ctx, ensure(dv.sperm, 4 * S));
  KCC_HIP(ctx, ensure(dv.counters, sizeof(unsigned long long) * kcc::CNT_N));
  if (!dv.np_sync.p) {  // node prep in the reduce launch: epoch words (kcc::NpArgs::sync)
    const size_t bytes = 4 * (kcc::NP_FLAGS + (size_t)kcc::reduce_tail_records());
    KCC_HIP(ctx, ensure(dv.np_sync, bytes));
    KCC_HIP(ctx, hipMemsetAsync(dv.np_sync.p, 0, bytes, dv.stream));
    // the fused reduce runs on the caller's stream, which nothing orders after dv.stream:
    // the zeroing completes here, on its own
    KCC_HIP(ctx, hipStreamSynchronize(dv.stream));
  }
  if (!dv.clamp_arrive.p) {  // the fused finalize's arrivals: every launch leaves them zero
    KCC_HIP(ctx, ensure(dv.clamp_arrive, 64));
    KCC_HIP(ctx, hipMemsetAsync(dv.clamp_arrive.p, 0, 64, dv.stream));
    KCC_HIP(ctx, hipStreamSynchronize(dv.stream));
  }
  // (a new allocation is a larger one: compare sizes, hipMalloc may hand back the address)
  const size_t q_before = dv.fit_q.bytes;
  KCC_HIP(ctx, ensure(dv.fit_q, 4 * (size_t)kcc::fit_queue_words((int64_t)S)));
  if (dv.fit_q.bytes != q_before) dv.fitq_dirty = true;
  const size_t S64 = (S + 63) / 64 * 64;
  KCC_HIP(ctx, ensure(dv.c_bcnt, 8 * (S64 / 64)));
  KCC_HIP(ctx, ensure(dv.c_cs, 8 * S));
  KCC_HIP(ctx, ensure(dv.c_ms, 8 * S));
  KCC_HIP(ctx, ensure(dv.c_mrc, 4 * S64));
  KCC_HIP(ctx, ensure(dv.c_crm, 4 * S64));
  KCC_HIP(ctx, ensure(dv.c_dperm, 4 * S));
  // the table copies stay all-zero between calls (clamp_prep zeroes what it reads); a
  // new or grown allocation, or a layout change, is zeroed before its first use
  const int64_t cs_ = kcc::clamp_c_cells((int64_t)S), hs = kcc::clamp_h_cells((int64_t)S);
  const size_t before[3] = {dv.c_C.bytes, dv.c_H2.bytes, dv.c_H3.bytes};
  // the spec ranks' per-slice counts: [rank_slices(S)][2][S] u32 (plain stores, nothing
  // to keep zero)
  KCC_HIP(ctx, ensure(dv.c_rank, 4 * (size_t)kcc::rank_words((int64_t)S)));
  if (dv.rank_arrive.bytes < 4 * (S64 / 64)) {  // every call leaves them zero
    KCC_HIP(ctx, ensure(dv.rank_arrive, 4 * (S64 / 64)));
    KCC_HIP(ctx, hipMemsetAsync(dv.rank_arrive.p, 0, dv.rank_arrive.bytes, dv.stream));
    KCC_HIP(ctx, hipStreamSynchronize(dv.stream));
  }
  KCC_HIP(ctx, ensure(dv.c_C, 8 * (size_t)kcc::C_COPIES * (size_t)cs_));
  KCC_HIP(ctx, ensure(dv.c_H2, 8 * (size_t)kcc::H2_COPIES * (size_t)hs));
  KCC_HIP(ctx, ensure(dv.c_H3, 8 * (size_t)kcc::H2_COPIES * (size_t)hs));
  KCC_HIP(ctx, ensure(dv.c_Crow, 8 * (size_t)cs_));
  if (kcc::clamp_binned((int64_t)S)) {  // node_prep's binned H2 / H3 records
    // the most passes (and record slots) any call of up to N rows makes
    const size_t passes = (size_t)((N + kcc::CLAMP_PASS_ROWS_MIN - 1) / kcc::CLAMP_PASS_ROWS_MIN);
    const size_t recs = (size_t)((N + kcc::CLAMP_PASS_ROWS_MAX - 1) / kcc::CLAMP_PASS_ROWS_MAX) *
                        2 * kcc::CLAMP_PASS_ROWS_MAX;  // >= passes(n) x 2 pass_rows(n) for any n <= N
    KCC_HIP(ctx, ensure(dv.c_rec, 8 * recs));
    KCC_HIP(ctx, ensure(dv.c_dir, 4 * (size_t)kcc::clamp_d_stride((int64_t)S) * passes));
  }
  if (dv.c_C.bytes != before[0] || dv.c_H2.bytes != before[1] || dv.c_H3.bytes != before[2] ||
      dv.c_stride != cs_ || dv.h_stride != hs)
    dv.clamp_dirty = true;
  dv.c_stride = cs_;
  dv.h_stride = hs;
  dv.d_stride = kcc::clamp_d_stride((int64_t)S);
  return KCC_OK;
}

// Zero the table copies when they are not known to be zero (before node_prep adds to them).
int clamp_clean(kcc_ctx* ctx, Dev& dv, hipStream_t s) {
  if (dv.fitq_dirty) {  // a new allocation of the fit queues (every launch leaves them zero)
    KCC_HIP(ctx, hipMemsetAsync(dv.fit_q.p, 0, dv.fit_q.bytes, s));
    dv.fitq_dirty = false;
  }
  if (!dv.clamp_dirty) return KCC_OK;
  KCC_HIP(ctx, hipMemsetAsync(dv.c_C.p, 0, dv.c_C.bytes, s));
  KCC_HIP(ctx, hipMemsetAsync(dv.c_H2.p, 0, dv.c_H2.bytes, s));
  KCC_HIP(ctx, hipMemsetAsync(dv.c_H3.p, 0, dv.c_H3.bytes, s));
  dv.clamp_dirty = false;
  return KCC_OK;
}

kcc::ClampWork clamp_of(Dev& dv) {
  kcc::ClampWork cw;
  cw.rank = as<uint32_t>(dv.c_rank);
  cw.bcnt = as<uint32_t>(dv.c_bcnt);
  cw.cs = as<uint64_t>(dv.c_cs);
  cw.ms = as<int64_t>(dv.c_ms);
  cw.mr_c = as<uint32_t>(dv.c_mrc);
  cw.cr_m = as<uint32_t>(dv.c_crm);
  cw.dperm = as<int32_t>(dv.c_dperm);
  cw.C = as<int64_t>(dv.c_C);
  cw.H2 = as<int64_t>(dv.c_H2);
  cw.H3 = as<int64_t>(dv.c_H3);
  cw.Crow = as<int64_t>(dv.c_Crow);
  cw.rec = as<uint64_t>(dv.c_rec);
  cw.dir = as<uint32_t>(dv.c_dir);
  cw.c_stride = dv.c_stride;
  cw.h_stride = dv.h_stride;
  cw.d_stride = dv.d_stride;
  cw.n_pass = 0;
  return cw;
}

// The spec-side workspace a call of S specs writes (host-side guard before any launch: a
// kernel writing past an allocation faults the device).
int check_spec_ws(kcc_ctx* ctx, Dev& dv, int64_t S) {
  const size_t S64 = (size_t)(S + 63) / 64 * 64;
  const bool ok = dv.c_rank.bytes >= 4 * (size_t)kcc::rank_words(S) &&
                  dv.c_bcnt.bytes >= 8 * (S64 / 64) && dv.c_mrc.bytes >= 4 * S64 &&
                  dv.rank_arrive.bytes >= 4 * (S64 / 64) &&
                  dv.c_crm.bytes >= 4 * S64 && dv.c_cs.bytes >= 8 * (size_t)S &&
                  dv.c_ms.bytes >= 8 * (size_t)S && dv.c_dperm.bytes >= 4 * (size_t)S &&
                  dv.srec.bytes >= sizeof(kcc::SpecRec) * (size_t)S &&
                  dv.sperm.bytes >= 4 * (size_t)S &&
                  dv.counters.bytes >= sizeof(unsigned long long) * kcc::CNT_N &&
                  dv.c_C.bytes >= 8 * (size_t)kcc::C_COPIES * (size_t)dv.c_stride &&
                  dv.c_stride >= kcc::clamp_c_cells(S);
  return ok ? KCC_OK : fail(ctx, KCC_EINVAL, "internal: spec workspace smaller than the call");
}

kcc::PlaceArgs place_args(Dev& dv, int64_t n_specs, const uint64_t* spec_cpu,
                          const int64_t* spec_mem, int64_t* partial) {
  return kcc::PlaceArgs{n_specs, spec_cpu, spec_mem, spec_prep_of(dv), clamp_of(dv), partial,
                        as<unsigned long long>(dv.counters), 0,
                        as<const unsigned long long>(dv.faults), 0};
}

int fit_prepare_dev(kcc_ctx* ctx, Dev& dv, int64_t n_nodes, const uint64_t* alloc_cpu,
                    const int64_t* alloc_mem, const int64_t* alloc_pods,
                    const int64_t* pod_count, const uint64_t* used_cpu,
                    const int64_t* used_mem, int64_t n_specs, const uint64_t* spec_cpu,
                    const int64_t* spec_mem, int64_t* partial, hipStream_t s) {
  ctx->host_stream_rows = -1;  // (kcc_fit_stream_rows: this call's device counters)
  if (n_nodes < 0 || n_specs < 0) return fail(ctx, KCC_EINVAL, "negative size");
  if (n_specs >= kcc::MAX_SPECS) return fail(ctx, KCC_EINVAL, "too many specs (max 2^26 - 1)");
  if (n_specs > 0 && (!spec_cpu || !spec_mem || !partial))
    return fail(ctx, KCC_EINVAL, "NULL spec array / partial");
  if (n_nodes > 0 && (!alloc_cpu || !alloc_mem || !alloc_pods || !pod_count || !used_cpu || !used_mem))
    return fail(ctx, KCC_EINVAL, "NULL node array");
  int rc = reserve_dev(ctx, dv, n_nodes, 0, n_specs);
  if (rc) return rc;
  dv.last_pairs = n_nodes * n_specs;
  dv.prep_nodes = n_nodes;
  dv.prep_specs = n_specs;
  if (n_specs == 0) return KCC_OK;
  if ((rc = check_spec_ws(ctx, dv, n_specs))) return rc;
  rc = clamp_clean(ctx, dv, s);
  if (rc) return rc;
  dv.clamp_dirty = true;  // until every kernel that leaves the tables zero is queued
  // spec_rank zeroes the counters and the coarse clamp table; spec_place zeroes
  // `partial` (no memset launches) and rides in the node_prep launch (node_prep reads
  // only the sorted arrays the ranks wrote)
  KCC_HIP(ctx, kcc::launch_spec_rank(kcc::rank_args(n_specs, spec_cpu, spec_mem, clamp_of(dv),
                                                    as<unsigned long long>(dv.counters),
                                                    as<uint32_t>(dv.rank_arrive)),
                                     s));
  const kcc::PlaceArgs pa = place_args(dv, n_specs, spec_cpu, spec_mem, partial);
  KCC_HIP(ctx, kcc::launch_node_prep(n_nodes, alloc_cpu, alloc_mem, alloc_pods, pod_count,
                                       used_cpu, used_mem, as<kcc::FitGroupA>(dv.fast_a),
                                       as<kcc::FitGroup>(dv.fast_b), as<kcc::SlowNode>(dv.slow),
                                       as<int64_t>(dv.slow_list), n_specs, clamp_of(dv),
                                       as<unsigned long long>(dv.counters), 0, 0,
                                       n_nodes, s, dv.fit_dense, &pa));
  if (n_nodes == 0) {
    dv.clamp_dirty = false;
    return KCC_OK;
  }
  dv.stream_chunks = 1;
  KCC_HIP(ctx, kcc::launch_clamp_apply(n_specs, n_nodes, clamp_of(dv),
                                       as<unsigned long long>(dv.counters), partial, s));
  dv.clamp_dirty = false;
  return KCC_OK;
}

int fit_run_dev(kcc_ctx* ctx, Dev& dv, int64_t n_nodes, int64_t n_specs, int64_t* partial,
                hipStream_t s) {
  if (n_nodes != dv.prep_nodes || n_specs != dv.prep_specs)
    return fail(ctx, KCC_EINVAL, "fit_run sizes differ from the preceding fit_prepare");
  if (n_nodes == 0 || n_specs == 0) return KCC_OK;
  if (!partial) return fail(ctx, KCC_EINVAL, "NULL partial");
  KCC_HIP(ctx, kcc::launch_fit(n_nodes, as<kcc::FitGroupA>(dv.fast_a), as<kcc::FitGroup>(dv.fast_b),
                               as<kcc::SlowNode>(dv.slow),
                               as<int64_t>(dv.slow_list), n_specs, spec_prep_of(dv), partial,
                               as<unsigned long long>(dv.counters), as<uint32_t>(dv.fit_q), 0,
                               n_nodes, s, as<const unsigned long long>(dv.faults)));
  return KCC_OK;
}

int fit_partial_dev(kcc_ctx* ctx, Dev& dv, int64_t n_nodes, const uint64_t* alloc_cpu,
                    const int64_t* alloc_mem, const int64_t* alloc_pods,
                    const int64_t* pod_count, const uint64_t* used_cpu,
                    const int64_t* used_mem, int64_t n_specs, const uint64_t* spec_cpu,
                    const int64_t* spec_mem, int64_t* partial, hipStream_t s) {
  int rc = fit_prepare_dev(ctx, dv, n_nodes, alloc_cpu, alloc_mem, alloc_pods, pod_count,
                           used_cpu, used_mem, n_specs, spec_cpu, spec_mem, partial, s);
  if (rc) return rc;
  return fit_run_dev(ctx, dv, n_nodes, n_specs, partial, s);
}

int fit_finalize_dev(kcc_ctx* ctx, Dev& dv, int64_t n_specs, const int64_t* partial,
                     int64_t* totals, int32_t* spec_err, hipStream_t s) {
  if (n_specs < 0) return fail(ctx, KCC_EINVAL, "negative size");
  if (n_specs == 0) return KCC_OK;
  if (!partial || !totals || !spec_err) return fail(ctx, KCC_EINVAL, "NULL partial/totals/err");
  if (dv.sperm.bytes < sizeof(int32_t) * (size_t)n_specs)
    return fail(ctx, KCC_EINVAL, "finalize without a matching fit_partial");
  KCC_HIP(ctx, kcc::launch_fit_finalize(n_specs, partial, as<int32_t>(dv.sperm), totals,
                                        spec_err, as<const unsigned long long>(dv.faults), s));
  return KCC_OK;
}


// ---- pipelined reduce + fit (kcc_capacity_partial_async) ---------------------------

hipError_t prof_event(Dev& dv, hipEvent_t* ev) {
  if (!dv.prof_free.empty()) {
    *ev = dv.prof_free.back();
    dv.prof_free.pop_back();
    return hipSuccess;
  }
  // device-scope release only: a timing event between two kernels of one stream needs no
  // system-scope fence (with it, hipEventCreate's default, every record left a ~5.5 us gap
  // on the stream)
  return hipEventCreateWithFlags(ev, hipEventDisableSystemFence);
}

// Chunk boundaries: node ranges of ~equal node count, multiples of CHUNK_ALIGN (a
// multiple of FIT_GROUP: the fit's node groups do not straddle two chunks); at least
// `min_nodes` nodes per chunk.
constexpr int64_t CHUNK_ALIGN = kcc::CLAMP_PASS_ROWS_MAX;  // whole node_prep passes
int plan_chunks(int64_t n_nodes, int want, int64_t min_nodes, std::vector<int64_t>& lo,
                std::vector<int64_t>& hi) {
  int k = want;
  if (k > kcc::FIT_MAX_CHUNKS) k = kcc::FIT_MAX_CHUNKS;
  while (k > 1 && n_nodes / k < min_nodes) --k;
  if (k < 1) k = 1;
  lo.assign(k, 0);
  hi.assign(k, 0);
  for (int c = 0; c < k; ++c) {
    lo[c] = c == 0 ? 0 : hi[c - 1];
    hi[c] = c == k - 1 ? n_nodes : (n_nodes * (c + 1) / k) / CHUNK_ALIGN * CHUNK_ALIGN;
    if (hi[c] < lo[c]) hi[c] = lo[c];
  }
  return k;
}

// Overlapping the reduce of chunk k with the fit of chunk k-1 measured SLOWER at C4
// (0.80 / 0.85 / 0.88 ms per step at 1 / 2 / 4 chunks): the fit keeps every SIMD's
// VALU issue ~90 % busy and the concurrent reduce's waves slow it by more than the
// reduce's own time.  Default: one chunk, everything on the caller's stream.
constexpr int KCC_DEFAULT_CHUNKS = 1;
constexpr int64_t KCC_MIN_CHUNK_NODES = 32768;

int capacity_partial_dev(kcc_ctx* ctx, Dev& dv, int64_t n_nodes, int64_t n_cont,
                         const int64_t* h_ptr, const int64_t* ptr, const uint64_t* cpu,
                         const int64_t* mem, const uint64_t* alloc_cpu, const int64_t* alloc_mem,
                         const int64_t* alloc_pods, const int64_t* pod_count, uint64_t* used_cpu,
                         int64_t* used_mem, int64_t n_specs, const uint64_t* spec_cpu,
                         const int64_t* spec_mem, int64_t* partial, int n_chunks, hipStream_t s,
                         int64_t* totals = nullptr, int32_t* spec_err = nullptr) {
  ctx->host_stream_rows = -1;  // (kcc_fit_stream_rows: this call's device counters)
  if (n_nodes < 0 || n_cont < 0 || n_specs < 0) return fail(ctx, KCC_EINVAL, "negative size");
  if (n_nodes >= kcc::RED_MAX_NODES)
    return fail(ctx, KCC_EINVAL, "too many nodes per device (max 2^28 - 1)");
  if (n_specs >= kcc::MAX_SPECS) return fail(ctx, KCC_EINVAL, "too many specs (max 2^26 - 1)");
  if (n_nodes == 0 && n_cont != 0) return fail(ctx, KCC_EINVAL, "containers without nodes");
  if (n_nodes > 0 && (!ptr || !used_cpu || !used_mem || !alloc_cpu || !alloc_mem || !alloc_pods ||
                      !pod_count))
    return fail(ctx, KCC_EINVAL, "NULL node array");
  if (n_cont > 0 && (!cpu || !mem)) return fail(ctx, KCC_EINVAL, "NULL cpu_req/mem_req");
  if (!aligned16(cpu) || !aligned16(mem))
    return fail(ctx, KCC_EINVAL, "container arrays must be 16-byte aligned");
  if (n_specs > 0 && (!spec_cpu || !spec_mem || !partial))
    return fail(ctx, KCC_EINVAL, "NULL spec array / partial");
  std::vector<int64_t> lo, hi;
  const int k = plan_chunks(n_nodes, h_ptr ? (n_chunks > 0 ? n_chunks : KCC_DEFAULT_CHUNKS) : 1,
                            KCC_MIN_CHUNK_NODES, lo, hi);
  std::vector<int64_t> c0(k), c1(k);
  for (int c = 0; c < k; ++c) {
    if (k == 1) {
      c0[c] = 0;
      c1[c] = n_cont;
    } else {
      c0[c] = h_ptr[lo[c]];
      c1[c] = h_ptr[hi[c]];
      if (c0[c] < 0 || c1[c] < c0[c] || c1[c] > n_cont)
        return fail(ctx, KCC_EINVAL, "h_node_ptr is not a CSR of n_containers");
    }
  }
  int rc = reserve_dev(ctx, dv, n_nodes, n_cont, n_specs);
  if (rc) return rc;
  if (n_specs > 0 && (rc = check_spec_ws(ctx, dv, n_specs))) return rc;
  for (int c = 0; c < k; ++c)
    if (!dv.ev_red[c]) KCC_HIP(ctx, hipEventCreateWithFlags(&dv.ev_red[c], hipEventDisableTiming));
  dv.last_pairs = n_nodes * n_specs;
  dv.stream_chunks = k;
  dv.prep_nodes = -1;  // the split fit_run API must not reuse this call's workspace state
  dv.prep_specs = -1;
  // k > 1: the reduces run on the side stream, forked from s (they wait for everything
  // already queued on s: the previous call's fits still read used_* and the node
  // streams); k == 1: everything on s
  hipStream_t rs = k > 1 ? dv.side : s;
  if (k > 1) {
    KCC_HIP(ctx, hipEventRecord(dv.ev_fork, s));
    KCC_HIP(ctx, hipStreamWaitEvent(dv.side, dv.ev_fork, 0));
  }
  // k == 1: the spec ranks ride in the reduce launch (extra workgroups in front of the
  // reduce's: independent work) and spec_place in the node_prep launch (node_prep reads
  // only the arrays the ranks wrote): four launches per call — reduce + rank, node_prep +
  // place, fit, clamp_apply
  const bool fuse_place = n_specs > 0;
  const bool fuse_rank = k == 1 && fuse_place && n_nodes > 0 && n_cont > 0;
  // the clamp in the fit (one node chunk, S <= CLAMP_LDS_SPECS, not dense, at least one node
  // and one container: the ranks ride in the reduce launch): no clamp_apply
  const bool nc = fuse_rank && n_specs <= kcc::CLAMP_LDS_SPECS && !dv.fit_dense &&
                  (dv.clamp_in_fit == 1 ||
                   (dv.clamp_in_fit < 0 && kcc::clamp_in_fit_auto(n_nodes, n_specs)));
  int32_t* const fast_cl = nc ? as<int32_t>(dv.fast_cl) : nullptr;
  dv.last_nc = nc;
  // the clamp in the fit needs no spec ranks (no clamp tables): the reduce launch carries
  // one workgroup that zeroes the counters, and spec_place counts the classes itself
  kcc::RankArgs ra = kcc::rank_args(n_specs, spec_cpu, spec_mem, clamp_of(dv),
                                    as<unsigned long long>(dv.counters),
                                    as<uint32_t>(dv.rank_arrive), nc);
  kcc::PlaceArgs pa = place_args(dv, n_specs, spec_cpu, spec_mem, partial);
  pa.no_ranks = nc ? 1 : 0;
  // spec_place and node prep's row pass ride in the reduce launch too, behind the reduce's
  // workgroups (kcc::NpArgs): no node_prep launch
  kcc::NpArgs np{};
  if (nc) {
    ra.done_flag = as<uint32_t>(dv.np_sync);
    np.n_place = (int32_t)((n_specs + 255) / 256);
    np.n_rows = (int32_t)((n_nodes + kcc::NP_ROWS_PER_WG - 1) / kcc::NP_ROWS_PER_WG);
    np.sync = as<uint32_t>(dv.np_sync);
    np.pa = pa;
    np.n = n_nodes;
    np.alloc_cpu = alloc_cpu;
    np.alloc_mem = alloc_mem;
    np.alloc_pods = alloc_pods;
    np.pod_count = pod_count;
    np.used_cpu = used_cpu;
    np.used_mem = used_mem;
    np.fast_a = as<kcc::FitGroupA>(dv.fast_a);
    np.fast_b = as<kcc::FitGroup>(dv.fast_b);
    np.slow = as<kcc::SlowNode>(dv.slow);
    np.slow_list = as<int64_t>(dv.slow_list);
    np.fast_cl = fast_cl;
    np.counters = as<unsigned long long>(dv.counters);
    np.bcnt = clamp_of(dv).bcnt;
    np.S = n_specs;
    np.faults = as<unsigned long long>(dv.faults);
  }
  if (n_specs > 0) {
    rc = clamp_clean(ctx, dv, s);
    if (rc) return rc;
    dv.clamp_dirty = true;  // until every kernel that leaves the tables zero is queued
    if (!fuse_rank) KCC_HIP(ctx, kcc::launch_spec_rank(ra, s));
  }
  for (int c = 0; c < k; ++c) {
    const int64_t n = hi[c] - lo[c];
    ProfPair pp{};
    if (dv.prof_on) {  // (the launch's own dispatch timestamps: no event packets around it)
      KCC_HIP(ctx, prof_event(dv, &pp.a));
      KCC_HIP(ctx, prof_event(dv, &pp.b));
    }
    KCC_HIP(ctx, kcc::launch_reduce(n, c0[c], c1[c] - c0[c], ptr + lo[c], cpu, mem, nullptr, nullptr,
                                    used_cpu + lo[c], used_mem + lo[c], nullptr, nullptr,
                                    as<uint64_t>(dv.red_tail),
                                    as<unsigned long long>(dv.faults), rs,
                                    fuse_rank ? &ra : nullptr, nc ? &np : nullptr,
                                    dv.prof_on ? pp.a : nullptr, dv.prof_on ? pp.b : nullptr));
    if (dv.prof_on) {
      pp.kind = 0;
      dv.prof_pending.push_back(pp);
    }
    if (k > 1) KCC_HIP(ctx, hipEventRecord(dv.ev_red[c], dv.side));
  }
  const bool fuse_fin = totals && n_nodes > 0;
  const kcc::FinArgs fin{as<int32_t>(dv.sperm), totals, spec_err, as<uint32_t>(dv.clamp_arrive),
                         as<const unsigned long long>(dv.faults)};
  for (int c = 0; c < k; ++c) {
    if (k > 1) KCC_HIP(ctx, hipStreamWaitEvent(s, dv.ev_red[c], 0));  // also joins the side stream
    const int64_t n = hi[c] - lo[c];
    const bool place_here = fuse_place && c == 0;
    if (n_specs == 0 || (n == 0 && !place_here)) continue;
    if (!nc)  // (else: in the reduce launch)
    KCC_HIP(ctx, kcc::launch_node_prep(n, alloc_cpu + lo[c], alloc_mem + lo[c], alloc_pods + lo[c],
                                       pod_count + lo[c], used_cpu + lo[c], used_mem + lo[c],
                                       as<kcc::FitGroupA>(dv.fast_a) + lo[c] / kcc::FIT_GROUP,
                                       as<kcc::FitGroup>(dv.fast_b) + lo[c] / kcc::FIT_GROUP,
                                       as<kcc::SlowNode>(dv.slow) + lo[c],
                                       as<int64_t>(dv.slow_list) + lo[c], n_specs, clamp_of(dv),
                                       as<unsigned long long>(dv.counters),
                                       c, lo[c], n_nodes, s, dv.fit_dense,
                                       place_here ? &pa : nullptr));
    if (n == 0) continue;
    ProfPair pp{};
    if (dv.prof_on) {
      KCC_HIP(ctx, prof_event(dv, &pp.a));
      KCC_HIP(ctx, prof_event(dv, &pp.b));
    }
    KCC_HIP(ctx, kcc::launch_fit(n, as<kcc::FitGroupA>(dv.fast_a) + lo[c] / kcc::FIT_GROUP,
                                 as<kcc::FitGroup>(dv.fast_b) + lo[c] / kcc::FIT_GROUP,
                                 as<kcc::SlowNode>(dv.slow) + lo[c],
                                 as<int64_t>(dv.slow_list) + lo[c], n_specs, spec_prep_of(dv),
                                 partial, as<unsigned long long>(dv.counters),
                                 as<uint32_t>(dv.fit_q), c, n_nodes, s,
                                 as<const unsigned long long>(dv.faults), fast_cl,
                                 dv.prof_on ? pp.a : nullptr, dv.prof_on ? pp.b : nullptr));
    if (dv.prof_on) {
      pp.kind = 1;
      dv.prof_pending.push_back(pp);
    }
  }
  // the pod-slot clamp of every chunk's fast rows, added back per spec; totals != nullptr:
  // the clamp launch's last workgroup also finalizes (no fit_finalize launch)
  if (n_specs > 0 && nc) {  // the fit applied the clamp: no clamp_apply, nothing dirty
    dv.clamp_dirty = false;
    if (totals) return fit_finalize_dev(ctx, dv, n_specs, partial, totals, spec_err, s);
    return KCC_OK;
  }
  if (n_specs > 0) {
    // (clamp_arrive is allocated and zeroed by reserve_dev; every launch leaves it zero)
    if (n_nodes > 0)
      KCC_HIP(ctx, kcc::launch_clamp_apply(n_specs, n_nodes, clamp_of(dv),
                                           as<unsigned long long>(dv.counters), partial, s,
                                           fuse_fin ? &fin : nullptr));
    dv.clamp_dirty = false;
    if (totals && !fuse_fin)
      return fit_finalize_dev(ctx, dv, n_specs, partial, totals, spec_err, s);
  }
  return KCC_OK;
}

// Host-array pipeline shared by kcc_fit / kcc_capacity: per device upload its node
// shard (and container shard), reduce (optional), fit_partial; all-reduce partials
// over RCCL when sharded; finalize on device 0; copy back.
int run_host(kcc_ctx* ctx, bool with_reduce, int64_t n_nodes, int64_t n_cont,
             const int64_t* node_ptr, const uint64_t* cpu_req, const int64_t* mem_req,
             const uint64_t* alloc_cpu, const int64_t* alloc_mem, const int64_t* alloc_pods,
             const int64_t* pod_count, const uint64_t* used_cpu_in, const int64_t* used_mem_in,
             int64_t n_specs, const uint64_t* spec_cpu, const int64_t* spec_mem,
             int64_t* totals, int32_t* spec_err) {
  if (n_nodes < 0 || n_specs < 0) return fail(ctx, KCC_EINVAL, "negative size");
  if (n_specs > 0 && (!spec_cpu || !spec_mem || !totals || !spec_err))
    return fail(ctx, KCC_EINVAL, "NULL spec array / output");
  if (n_nodes > 0 && (!alloc_cpu || !alloc_mem || !alloc_pods || !pod_count))
    return fail(ctx, KCC_EINVAL, "NULL node array");
  if (with_reduce) {
    int rc = check_csr(ctx, n_nodes, n_cont, node_ptr);
    if (rc) return rc;
    if (n_cont > 0 && (!cpu_req || !mem_req)) return fail(ctx, KCC_EINVAL, "NULL container array");
  } else if (n_nodes > 0 && (!used_cpu_in || !used_mem_in)) {
    return fail(ctx, KCC_EINVAL, "NULL used array");
  }
  if (n_specs == 0) return KCC_OK;
  const int nd = (int)ctx->devs.size();
  // node shards: one per device, or ctx->node_shards (kcc_set_node_shards) dealt
  // round-robin over the devices; a device's shards run one after the other on its
  // stream, each into its own slot of the device's partial buffer, and the slots are
  // summed on the device before the RCCL all-reduce over devices
  const int ns = ctx->node_shards > nd ? ctx->node_shards : nd;
  const int slots = (ns + nd - 1) / nd;
  std::vector<int64_t> lo, hi;
  shard_nodes(n_nodes, ns, lo, hi);
  std::vector<std::vector<int64_t>> rebased(ns);  // per shard: copies may still be in flight
  if (ctx->host_cnt_n < (size_t)ns * kcc::CNT_N) {
    if (ctx->host_cnt) (void)hipHostFree(ctx->host_cnt);
    ctx->host_cnt = nullptr;
    ctx->host_cnt_n = 0;
    KCC_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->host_cnt),
                               sizeof(unsigned long long) * (size_t)ns * kcc::CNT_N, hipHostMallocDefault));
    ctx->host_cnt_n = (size_t)ns * kcc::CNT_N;
  }
  ctx->host_stream_rows = -1;
  for (int d = 0; d < nd; ++d) {
    Dev& dv = ctx->devs[d];
    KCC_HIP(ctx, hipSetDevice(dv.device));
    KCC_HIP(ctx, ensure(dv.partial, sizeof(int64_t) * 2 * (size_t)n_specs * (size_t)slots));
  }
  std::vector<Stage> stages;  // one per device, rewound per shard
  stages.reserve(nd);
  for (Dev& dv : ctx->devs) stages.emplace_back(ctx, dv);
  for (int sh = 0; sh < ns; ++sh) {
    Dev& dv = ctx->devs[sh % nd];
    Stage& st = stages[sh % nd];
    st.rewind();
    int64_t* part = as<int64_t>(dv.partial) + (size_t)(sh / nd) * 2 * (size_t)n_specs;
    KCC_HIP(ctx, hipSetDevice(dv.device));
    const int64_t n = hi[sh] - lo[sh];
    const uint64_t *a_cpu = alloc_cpu + lo[sh], *s_cpu = spec_cpu;
    const int64_t *a_mem = alloc_mem + lo[sh], *a_pods = alloc_pods + lo[sh];
    const int64_t *pods = pod_count + lo[sh], *s_mem = spec_mem;
    int rc;
    if ((rc = st.in(a_cpu, n)) || (rc = st.in(a_mem, n)) || (rc = st.in(a_pods, n)) ||
        (rc = st.in(pods, n)) || (rc = st.in(s_cpu, n_specs)) || (rc = st.in(s_mem, n_specs)))
      return rc;
    const uint64_t* u_cpu = nullptr;
    const int64_t* u_mem = nullptr;
    if (with_reduce) {
      // the shard's containers [c0, c1) with its CSR offsets rebased to 0
      const int64_t c0 = n > 0 ? node_ptr[lo[sh]] : 0, c1 = n > 0 ? node_ptr[hi[sh]] : 0;
      std::vector<int64_t>& rb = rebased[sh];
      rb.resize((size_t)n + 1);
      for (int64_t k = 0; k <= n; ++k) rb[k] = n > 0 ? node_ptr[lo[sh] + k] - c0 : 0;
      const int64_t* ptr = rb.data();
      const uint64_t* cpu = cpu_req + c0;
      const int64_t* mem = mem_req + c0;
      uint64_t* r_cpu = nullptr;
      int64_t* r_mem = nullptr;
      if ((rc = st.in(ptr, n + 1)) || (rc = st.in(cpu, c1 - c0)) || (rc = st.in(mem, c1 - c0)) ||
          (rc = st.tmp(r_cpu, n)) || (rc = st.tmp(r_mem, n)) ||
          (rc = reduce_async_dev(ctx, dv, n, c1 - c0, ptr, cpu, mem, nullptr, nullptr, r_cpu, r_mem,
                                 nullptr, nullptr, dv.stream)))
        return rc;
      u_cpu = r_cpu;
      u_mem = r_mem;
    } else {
      u_cpu = used_cpu_in + lo[sh];
      u_mem = used_mem_in + lo[sh];
      if ((rc = st.in(u_cpu, n)) || (rc = st.in(u_mem, n))) return rc;
    }
    rc = fit_partial_dev(ctx, dv, n, a_cpu, a_mem, a_pods, pods, u_cpu, u_mem, n_specs, s_cpu, s_mem,
                         part, dv.stream);
    if (rc) return rc;
    // exact-path pair count of this shard (the next shard's spec setup zeroes it)
    KCC_HIP(ctx, hipMemcpyAsync(ctx->host_cnt + (size_t)sh * kcc::CNT_N, dv.counters.p,
                                sizeof(unsigned long long) * kcc::CNT_N, hipMemcpyDeviceToHost,
                                dv.stream));
    if (sh >= nd)  // fold this slot into the device's slot 0 (wrapping int64 adds)
      KCC_HIP(ctx, kcc::launch_partial_add(2 * n_specs, as<int64_t>(dv.partial), part, dv.stream));
  }
  if (!ctx->comms.empty()) {
    // the context's first all-reduce proves itself (as bench.py's exchange does before it
    // is timed): every device's result must equal the host's wrapping sum of the devices'
    // partials (CC:138 summed over devices), else KCC_ERCCL.  Later calls are checked only
    // with kcc_set_allreduce_verify(ctx, 1) (two device-to-host copies and stream syncs
    // per device and call)
    const bool verify = !ctx->allreduce_verified || ctx->allreduce_verify_every;
    const size_t words = 2 * (size_t)n_specs;
    std::vector<uint64_t> expect, got;
    if (verify) {
      expect.assign(words, 0);
      got.resize(words);
      for (int d = 0; d < nd; ++d) {
        Dev& dv = ctx->devs[d];
        KCC_HIP(ctx, hipSetDevice(dv.device));
        KCC_HIP(ctx, hipMemcpyAsync(got.data(), dv.partial.p, 8 * words, hipMemcpyDeviceToHost,
                                    dv.stream));
        KCC_HIP(ctx, hipStreamSynchronize(dv.stream));
        for (size_t i = 0; i < words; ++i) expect[i] += got[i];
      }
    }
    KCC_NCCL(ctx, ncclGroupStart());
    for (int d = 0; d < nd; ++d) {
      Dev& dv = ctx->devs[d];
      KCC_NCCL(ctx, ncclAllReduce(dv.partial.p, dv.partial.p, words, ncclInt64,
                                  ncclSum, ctx->comms[d], dv.stream));
    }
    KCC_NCCL(ctx, ncclGroupEnd());
#ifdef KCC_DIAG_INLIB_COMM
    // the drill (variant builds only): a corrupted all-reduce result on the last device
    if (std::getenv("KCC_DRILL_CORRUPT_ALLREDUCE")) {
      Dev& dv = ctx->devs[nd - 1];
      KCC_HIP(ctx, hipSetDevice(dv.device));
      KCC_HIP(ctx, hipMemsetAsync(dv.partial.p, 0x5a, 8, dv.stream));
    }
#endif
    if (verify) {
      for (int d = 0; d < nd; ++d) {
        Dev& dv = ctx->devs[d];
        KCC_HIP(ctx, hipSetDevice(dv.device));
        KCC_HIP(ctx, hipMemcpyAsync(got.data(), dv.partial.p, 8 * words, hipMemcpyDeviceToHost,
                                    dv.stream));
        KCC_HIP(ctx, hipStreamSynchronize(dv.stream));
        for (size_t i = 0; i < words; ++i)
          if (got[i] != expect[i])
            return fail(ctx, KCC_ERCCL,
                        "in-library all-reduce verification failed on device " +
                            std::to_string(dv.device) + ": word " + std::to_string(i) + " is " +
                            std::to_string(got[i]) + ", the host sum of the devices' partials " +
                            std::to_string(expect[i]) + "; results not returned");
      }
      ctx->allreduce_verified = true;
    }
  }
  // finalize on device 0; its stream is synchronised last, by the staging's finish
  for (int d = nd - 1; d > 0; --d) {
    KCC_HIP(ctx, hipSetDevice(ctx->devs[d].device));
    KCC_HIP(ctx, hipStreamSynchronize(ctx->devs[d].stream));
  }
  Dev& d0 = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(d0.device));
  int rc;
  if ((rc = stages[0].out(totals, n_specs)) || (rc = stages[0].out(spec_err, n_specs)) ||
      (rc = fit_finalize_dev(ctx, d0, n_specs, as<int64_t>(d0.partial), totals, spec_err,
                             d0.stream)) ||
      (rc = stages[0].finish()))
    return rc;
  unsigned long long slow_pairs = 0;
  int64_t streamed = 0;
  for (int sh = 0; sh < ns; ++sh) {
    slow_pairs += ctx->host_cnt[(size_t)sh * kcc::CNT_N + kcc::CNT_SLOW_PAIRS];
    streamed += (int64_t)ctx->host_cnt[(size_t)sh * kcc::CNT_N + kcc::CNT_STREAM];
  }
  ctx->host_stream_rows = streamed;
  const double pairs = (double)n_nodes * (double)n_specs;
  ctx->slow_frac = pairs > 0 ? (double)slow_pairs / pairs : 0.0;
  return check_faults(ctx);
}

}  // namespace

extern "C" {

int kcc_abi_version(void) { return KCC_ABI_VERSION; }

int kcc_set_allreduce_verify(kcc_ctx* ctx, int every_call) {
  if (!ctx) return KCC_EINVAL;
  ctx->allreduce_verify_every = every_call != 0;
  return KCC_OK;
}

// The knobs an experiment build was compiled with (csrc/Makefile `variant` passes them in
// KCC_VARIANT_FLAGS); the release library takes none (the Makefile refuses EXTRA there).
#ifdef KCC_VARIANT_BUILD
const char* kcc_build_info(void) { return "variant: " KCC_VARIANT_FLAGS; }
#else
const char* kcc_build_info(void) { return "release"; }
#endif

const char* kcc_create_error(void) { return g_create_error.c_str(); }

int kcc_create(kcc_ctx** out, int first_device, int n_gpus) {
  g_create_error.clear();
  if (!out) { g_create_error = "out is NULL"; return KCC_EINVAL; }
  *out = nullptr;
  if (n_gpus <= 0 || first_device < 0) {
    g_create_error = "n_gpus must be >= 1 and first_device >= 0 (there is no CPU backend)";
    return KCC_EINVAL;
  }
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    g_create_error = std::string("no HIP device: ") + hipGetErrorString(e);
    return KCC_ENODEV;
  }
  if (first_device + n_gpus > count) {
    g_create_error = "requested devices [" + std::to_string(first_device) + ", " +
                     std::to_string(first_device + n_gpus) + ") but only " +
                     std::to_string(count) + " visible";
    return KCC_ENODEV;
  }
  kcc_ctx* ctx = new kcc_ctx();
  ctx->devs.resize(n_gpus);
  std::vector<int> ids(n_gpus);
  for (int d = 0; d < n_gpus; ++d) {
    Dev& dv = ctx->devs[d];
    dv.device = first_device + d;
    ids[d] = dv.device;
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, dv.device)) != hipSuccess ||
        std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
      g_create_error = "device " + std::to_string(dv.device) + " is not gfx950 (" +
                       (e == hipSuccess ? std::string(prop.gcnArchName)
                                        : std::string(hipGetErrorString(e))) +
                       "): libkcc is built for MI355X only";
      kcc_destroy(ctx);
      return KCC_ENODEV;
    }
    if ((e = hipSetDevice(dv.device)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&dv.stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&dv.side, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&dv.ev_fork, hipEventDisableTiming)) != hipSuccess) {
      g_create_error = std::string("stream creation failed: ") + hipGetErrorString(e);
      kcc_destroy(ctx);
      return KCC_EHIP;
    }
  }
#ifdef KCC_DIAG_INLIB_COMM
  const bool inlib_comm = true;  // (variant builds: one device goes through RCCL too)
#else
  const bool inlib_comm = n_gpus > 1;
#endif
  if (inlib_comm) {
    ctx->comms.resize(n_gpus);
    ncclResult_t r = ncclCommInitAll(ctx->comms.data(), n_gpus, ids.data());
    if (r != ncclSuccess) {
      ctx->comms.clear();
      g_create_error = std::string("ncclCommInitAll: ") + ncclGetErrorString(r);
      kcc_destroy(ctx);
      return KCC_ERCCL;
    }
  }
  *out = ctx;
  return KCC_OK;
}

void kcc_destroy(kcc_ctx* ctx) {
  if (!ctx) return;
  for (auto& c : ctx->comms) ncclCommDestroy(c);
  if (ctx->proc_comm) {
    (void)hipSetDevice(ctx->devs[0].device);
    (void)hipDeviceSynchronize();  // its all-reduces ran on caller streams
    ncclCommDestroy(ctx->proc_comm);
  }
  for (Dev& dv : ctx->devs) {
    (void)hipSetDevice(dv.device);
    if (dv.stream) (void)hipStreamSynchronize(dv.stream);
    if (dv.p2p_W > 0) {
      (void)hipDeviceSynchronize();  // exchanges ran on caller streams
      for (int p = 0; p < dv.p2p_W; ++p)
        if (p != dv.p2p_rank && dv.p2p_peer[p]) (void)hipIpcCloseMemHandle(dv.p2p_peer[p]);
    }
    if (dv.stream) (void)hipStreamDestroy(dv.stream);
    if (dv.side) {
      (void)hipStreamSynchronize(dv.side);
      (void)hipStreamDestroy(dv.side);
    }
    if (dv.ev_fork) (void)hipEventDestroy(dv.ev_fork);
    for (hipEvent_t ev : dv.ev_red)
      if (ev) (void)hipEventDestroy(ev);
    for (const ProfPair& pp : dv.prof_pending) {
      (void)hipEventDestroy(pp.a);
      (void)hipEventDestroy(pp.b);
    }
    for (hipEvent_t ev : dv.prof_free) (void)hipEventDestroy(ev);
  }
  if (ctx->host_cnt) (void)hipHostFree(ctx->host_cnt);
  delete ctx;  // every DevBuf frees its memory: the streams are idle, the peers' handles closed
}

const char* kcc_last_error(const kcc_ctx* ctx) { return ctx ? ctx->err.c_str() : "NULL context"; }

int kcc_reserve(kcc_ctx* ctx, int64_t max_nodes, int64_t max_containers, int64_t max_specs) {
  if (!ctx) return KCC_EINVAL;
  if (max_nodes < 0 || max_containers < 0 || max_specs < 0)
    return fail(ctx, KCC_EINVAL, "negative size");
  return reserve_dev(ctx, ctx->devs[0], max_nodes, max_containers, max_specs);
}

int kcc_reduce_requests_async(kcc_ctx* ctx, int64_t n_nodes, int64_t n_containers,
                              const int64_t* d_node_ptr, const uint64_t* d_cpu_req,
                              const int64_t* d_mem_req, const uint64_t* d_cpu_lim,
                              const int64_t* d_mem_lim, uint64_t* d_used_cpu,
                              int64_t* d_used_mem, uint64_t* d_lim_cpu, int64_t* d_lim_mem,
                              void* stream) {
  if (!ctx) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  return reduce_async_dev(ctx, dv, n_nodes, n_containers, d_node_ptr, d_cpu_req, d_mem_req,
                          d_cpu_lim, d_mem_lim, d_used_cpu, d_used_mem, d_lim_cpu, d_lim_mem,
                          static_cast<hipStream_t>(stream));
}

int kcc_reduce_requests(kcc_ctx* ctx, int64_t n_nodes, int64_t n_containers,
                        const int64_t* node_ptr, const uint64_t* cpu_req, const int64_t* mem_req,
                        const uint64_t* cpu_lim, const int64_t* mem_lim, uint64_t* used_cpu,
                        int64_t* used_mem, uint64_t* lim_cpu, int64_t* lim_mem) {
  if (!ctx) return KCC_EINVAL;
  int rc = check_reduce(ctx, n_nodes, n_containers, node_ptr, cpu_req, mem_req, cpu_lim, mem_lim,
                        used_cpu, used_mem, lim_cpu, lim_mem);
  if (rc || (rc = check_csr(ctx, n_nodes, n_containers, node_ptr))) return rc;
  if (!cpu_lim) {  // no limits: their sums are not written
    lim_cpu = nullptr;
    lim_mem = nullptr;
  }
  // the reduce is cheap next to the fit: run it on the first device
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  Stage st(ctx, dv);
  if ((rc = st.in(node_ptr, csr_len(n_nodes))) || (rc = st.in(cpu_req, n_containers)) ||
      (rc = st.in(mem_req, n_containers)) || (rc = st.in(cpu_lim, n_containers)) ||
      (rc = st.in(mem_lim, n_containers)) || (rc = st.out(used_cpu, n_nodes)) ||
      (rc = st.out(used_mem, n_nodes)) || (rc = st.out(lim_cpu, n_nodes)) ||
      (rc = st.out(lim_mem, n_nodes)) ||
      (rc = reduce_async_dev(ctx, dv, n_nodes, n_containers, node_ptr, cpu_req, mem_req, cpu_lim,
                             mem_lim, used_cpu, used_mem, lim_cpu, lim_mem, dv.stream)))
    return rc;
  return st.finish(true);
}

int kcc_fit(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu, const int64_t* alloc_mem,
            const int64_t* alloc_pods, const int64_t* pod_count, const uint64_t* used_cpu,
            const int64_t* used_mem, int64_t n_specs, const uint64_t* spec_cpu,
            const int64_t* spec_mem, int64_t* totals, int32_t* spec_err) {
  if (!ctx) return KCC_EINVAL;
  return run_host(ctx, false, n_nodes, 0, nullptr, nullptr, nullptr, alloc_cpu, alloc_mem,
                  alloc_pods, pod_count, used_cpu, used_mem, n_specs, spec_cpu, spec_mem, totals,
                  spec_err);
}

int kcc_capacity(kcc_ctx* ctx, int64_t n_nodes, int64_t n_containers, const int64_t* node_ptr,
                 const uint64_t* cpu_req, const int64_t* mem_req, const uint64_t* alloc_cpu,
                 const int64_t* alloc_mem, const int64_t* alloc_pods, const int64_t* pod_count,
                 int64_t n_specs, const uint64_t* spec_cpu, const int64_t* spec_mem,
                 int64_t* totals, int32_t* spec_err) {
  if (!ctx) return KCC_EINVAL;
  return run_host(ctx, true, n_nodes, n_containers, node_ptr, cpu_req, mem_req, alloc_cpu,
                  alloc_mem, alloc_pods, pod_count, nullptr, nullptr, n_specs, spec_cpu, spec_mem,
                  totals, spec_err);
}

int kcc_fit_partial_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                          const int64_t* d_alloc_mem, const int64_t* d_alloc_pods,
                          const int64_t* d_pod_count, const uint64_t* d_used_cpu,
                          const int64_t* d_used_mem, int64_t n_specs, const uint64_t* d_spec_cpu,
                          const int64_t* d_spec_mem, int64_t* d_partial, void* stream) {
  if (!ctx) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  return fit_partial_dev(ctx, dv, n_nodes, d_alloc_cpu, d_alloc_mem, d_alloc_pods, d_pod_count,
                         d_used_cpu, d_used_mem, n_specs, d_spec_cpu, d_spec_mem, d_partial,
                         static_cast<hipStream_t>(stream));
}

int kcc_fit_prepare_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                          const int64_t* d_alloc_mem, const int64_t* d_alloc_pods,
                          const int64_t* d_pod_count, const uint64_t* d_used_cpu,
                          const int64_t* d_used_mem, int64_t n_specs, const uint64_t* d_spec_cpu,
                          const int64_t* d_spec_mem, int64_t* d_partial, void* stream) {
  if (!ctx) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  return fit_prepare_dev(ctx, dv, n_nodes, d_alloc_cpu, d_alloc_mem, d_alloc_pods, d_pod_count,
                         d_used_cpu, d_used_mem, n_specs, d_spec_cpu, d_spec_mem, d_partial,
                         static_cast<hipStream_t>(stream));
}

int kcc_fit_run_async(kcc_ctx* ctx, int64_t n_nodes, int64_t n_specs, int64_t* d_partial,
                      void* stream) {
  if (!ctx) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  return fit_run_dev(ctx, dv, n_nodes, n_specs, d_partial, static_cast<hipStream_t>(stream));
}

int kcc_fit_finalize_async(kcc_ctx* ctx, int64_t n_specs, const int64_t* d_partial,
                           int64_t* d_totals, int32_t* d_spec_err, void* stream) {
  if (!ctx) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  return fit_finalize_dev(ctx, dv, n_specs, d_partial, d_totals, d_spec_err,
                          static_cast<hipStream_t>(stream));
}

int kcc_fit_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                  const int64_t* d_alloc_mem, const int64_t* d_alloc_pods,
                  const int64_t* d_pod_count, const uint64_t* d_used_cpu,
                  const int64_t* d_used_mem, int64_t n_specs, const uint64_t* d_spec_cpu,
                  const int64_t* d_spec_mem, int64_t* d_totals, int32_t* d_spec_err,
                  void* stream) {
  if (!ctx) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  KCC_HIP(ctx, ensure(dv.partial, sizeof(int64_t) * 2 * (size_t)(n_specs > 0 ? n_specs : 1)));
  const hipStream_t s = static_cast<hipStream_t>(stream);
  int rc = fit_partial_dev(ctx, dv, n_nodes, d_alloc_cpu, d_alloc_mem, d_alloc_pods, d_pod_count,
                           d_used_cpu, d_used_mem, n_specs, d_spec_cpu, d_spec_mem,
                           as<int64_t>(dv.partial), s);
  if (rc) return rc;
  return fit_finalize_dev(ctx, dv, n_specs, as<int64_t>(dv.partial), d_totals, d_spec_err, s);
}

int kcc_capacity_partial_async(kcc_ctx* ctx, int64_t n_nodes, int64_t n_containers,
                               const int64_t* h_node_ptr, const int64_t* d_node_ptr,
                               const uint64_t* d_cpu_req, const int64_t* d_mem_req,
                               const uint64_t* d_alloc_cpu, const int64_t* d_alloc_mem,
                               const int64_t* d_alloc_pods, const int64_t* d_pod_count,
                               uint64_t* d_used_cpu, int64_t* d_used_mem, int64_t n_specs,
                               const uint64_t* d_spec_cpu, const int64_t* d_spec_mem,
                               int64_t* d_partial, int n_chunks, void* stream) {
  if (!ctx) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  return capacity_partial_dev(ctx, dv, n_nodes, n_containers, h_node_ptr, d_node_ptr, d_cpu_req,
                              d_mem_req, d_alloc_cpu, d_alloc_mem, d_alloc_pods, d_pod_count,
                              d_used_cpu, d_used_mem, n_specs, d_spec_cpu, d_spec_mem, d_partial,
                              n_chunks, static_cast<hipStream_t>(stream));
}

int kcc_capacity_async(kcc_ctx* ctx, int64_t n_nodes, int64_t n_containers,
                       const int64_t* h_node_ptr, const int64_t* d_node_ptr,
                       const uint64_t* d_cpu_req, const int64_t* d_mem_req,
                       const uint64_t* d_alloc_cpu, const int64_t* d_alloc_mem,
                       const int64_t* d_alloc_pods, const int64_t* d_pod_count,
                       uint64_t* d_used_cpu, int64_t* d_used_mem, int64_t n_specs,
                       const uint64_t* d_spec_cpu, const int64_t* d_spec_mem, int64_t* d_totals,
                       int32_t* d_spec_err, void* stream) {
  if (!ctx) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  if (n_specs > 0 && (!d_totals || !d_spec_err)) return fail(ctx, KCC_EINVAL, "NULL totals/err");
  KCC_HIP(ctx, ensure(dv.partial, sizeof(int64_t) * 2 * (size_t)(n_specs > 0 ? n_specs : 1)));
  return capacity_partial_dev(ctx, dv, n_nodes, n_containers, h_node_ptr, d_node_ptr, d_cpu_req,
                              d_mem_req, d_alloc_cpu, d_alloc_mem, d_alloc_pods, d_pod_count,
                              d_used_cpu, d_used_mem, n_specs, d_spec_cpu, d_spec_mem,
                              as<int64_t>(dv.partial), 1, static_cast<hipStream_t>(stream),
                              d_totals, d_spec_err);
}

int kcc_profile_enable(kcc_ctx* ctx, int on) {
  if (!ctx) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  KCC_HIP(ctx, hipDeviceSynchronize());
  for (const ProfPair& pp : dv.prof_pending) {
    dv.prof_free.push_back(pp.a);
    dv.prof_free.push_back(pp.b);
  }
  dv.prof_pending.clear();
  dv.prof_on = on != 0;
  dv.prof_ms[0] = dv.prof_ms[1] = 0.0;
  dv.prof_n[0] = dv.prof_n[1] = 0;
  return KCC_OK;
}

int kcc_profile_read(kcc_ctx* ctx, double* reduce_ms, int64_t* reduce_launches, double* fit_ms,
                     int64_t* fit_launches) {
  if (!ctx) return KCC_EINVAL;
  if (!reduce_ms || !reduce_launches || !fit_ms || !fit_launches)
    return fail(ctx, KCC_EINVAL, "NULL output");
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  for (const ProfPair& pp : dv.prof_pending) {
    KCC_HIP(ctx, hipEventSynchronize(pp.b));
    float ms = 0.0f;
    KCC_HIP(ctx, hipEventElapsedTime(&ms, pp.a, pp.b));
    dv.prof_ms[pp.kind] += ms;
    dv.prof_n[pp.kind] += 1;
    dv.prof_free.push_back(pp.a);
    dv.prof_free.push_back(pp.b);
  }
  dv.prof_pending.clear();
  *reduce_ms = dv.prof_ms[0];
  *reduce_launches = dv.prof_n[0];
  *fit_ms = dv.prof_ms[1];
  *fit_launches = dv.prof_n[1];
  return KCC_OK;
}

double kcc_last_slow_fraction(const kcc_ctx* ctx) { return ctx ? ctx->slow_frac : -1.0; }

int kcc_fit_slow_pairs(kcc_ctx* ctx, int64_t* slow_pairs, int64_t* pairs) {
  if (!ctx || !slow_pairs || !pairs) return ctx ? fail(ctx, KCC_EINVAL, "NULL output") : KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  KCC_HIP(ctx, hipDeviceSynchronize());
  unsigned long long c = 0;
  if (dv.counters.p) KCC_HIP(ctx, hipMemcpy(&c, dv.counters.p, sizeof(c), hipMemcpyDeviceToHost));
  *slow_pairs = (int64_t)c;
  *pairs = dv.last_pairs;
  return KCC_OK;
}

int kcc_set_fit_dense(kcc_ctx* ctx, int dense) {
  if (!ctx) return KCC_EINVAL;
  for (Dev& dv : ctx->devs) dv.fit_dense = dense != 0;
  return KCC_OK;
}

int kcc_clamp_in_fit_used(kcc_ctx* ctx, int* used) {
  if (!ctx || !used) return KCC_EINVAL;
  *used = 0;
  for (const Dev& dv : ctx->devs) *used |= dv.last_nc ? 1 : 0;
  return KCC_OK;
}

int kcc_set_clamp_in_fit(kcc_ctx* ctx, int mode) {
  if (!ctx) return KCC_EINVAL;
  if (mode < -1 || mode > 1) return fail(ctx, KCC_EINVAL, "mode: -1 (by size), 0 or 1");
  for (Dev& dv : ctx->devs) dv.clamp_in_fit = mode;
  return KCC_OK;
}

int kcc_fit_stream_rows(kcc_ctx* ctx, int64_t* streamed) {
  if (!ctx || !streamed) return ctx ? fail(ctx, KCC_EINVAL, "NULL output") : KCC_EINVAL;
  if (ctx->host_stream_rows >= 0) {  // the last fit was kcc_fit / kcc_capacity: every shard
    *streamed = ctx->host_stream_rows;
    return KCC_OK;
  }
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  KCC_HIP(ctx, hipDeviceSynchronize());
  unsigned long long c[kcc::CNT_N] = {};
  if (dv.counters.p)
    KCC_HIP(ctx, hipMemcpy(c, dv.counters.p, sizeof(c), hipMemcpyDeviceToHost));
  int64_t t = 0;
  for (int k = 0; k < dv.stream_chunks && k < kcc::FIT_MAX_CHUNKS; ++k) t += (int64_t)c[kcc::CNT_STREAM + k];
  *streamed = t;
  return KCC_OK;
}

int kcc_reduce_faults(kcc_ctx* ctx, int64_t* faults) {
  if (!ctx || !faults) return ctx ? fail(ctx, KCC_EINVAL, "NULL output") : KCC_EINVAL;
  int64_t t = 0;
  for (Dev& dv : ctx->devs) {
    if (!dv.faults.p) continue;
    KCC_HIP(ctx, hipSetDevice(dv.device));
    KCC_HIP(ctx, hipDeviceSynchronize());
    unsigned long long f = 0;
    KCC_HIP(ctx, hipMemcpy(&f, as<unsigned long long>(dv.faults) + kcc::FAULT_RED, sizeof(f),
                           hipMemcpyDeviceToHost));
    t += (int64_t)f;
  }
  *faults = t;
  return KCC_OK;
}

int kcc_clear_faults(kcc_ctx* ctx) {
  if (!ctx) return KCC_EINVAL;
  for (Dev& dv : ctx->devs) {
    KCC_HIP(ctx, hipSetDevice(dv.device));
    KCC_HIP(ctx, hipDeviceSynchronize());
    if (dv.faults.p) KCC_HIP(ctx, hipMemset(dv.faults.p, 0, dv.faults.bytes));
    // a wait that gave up left its record published: every tag back to free
    if (dv.red_tail.p) KCC_HIP(ctx, hipMemset(dv.red_tail.p, 0, dv.red_tail.bytes));
    // and every counter a launch leaves zero: a gather part that gave up can have
    // published its ready count after the last part reset it
    for (DevBuf* b : {&dv.kb_arrive, &dv.rank_arrive, &dv.fit_q, &dv.clamp_arrive})
      if (b->p) KCC_HIP(ctx, hipMemset(b->p, 0, b->bytes));
    KCC_HIP(ctx, hipDeviceSynchronize());
  }
  return KCC_OK;
}

int kcc_set_node_shards(kcc_ctx* ctx, int n_shards) {
  if (!ctx) return KCC_EINVAL;
  if (n_shards < 0) return fail(ctx, KCC_EINVAL, "n_shards must be >= 0");
  ctx->node_shards = n_shards;
  return KCC_OK;
}

// ---- one rank of a multi-process run (one process per GPU) --------------------------

int kcc_comm_unique_id(uint8_t* id) {
  if (!id) return KCC_EINVAL;
  static_assert(sizeof(ncclUniqueId) == KCC_COMM_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId u;
  if (ncclGetUniqueId(&u) != ncclSuccess) return KCC_ERCCL;
  std::memcpy(id, &u, sizeof(u));
  return KCC_OK;
}

int kcc_comm_init(kcc_ctx* ctx, const uint8_t* id, int n_ranks, int rank) {
  if (!ctx) return KCC_EINVAL;
  if (!id || n_ranks < 1 || rank < 0 || rank >= n_ranks)
    return fail(ctx, KCC_EINVAL, "need an id, n_ranks >= 1 and 0 <= rank < n_ranks");
  if (ctx->devs.size() != 1)
    return fail(ctx, KCC_EINVAL, "a multi-process rank drives exactly one device");
  if (ctx->proc_comm) return fail(ctx, KCC_EINVAL, "communicator already initialised");
  KCC_HIP(ctx, hipSetDevice(ctx->devs[0].device));
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  KCC_NCCL(ctx, ncclCommInitRank(&ctx->proc_comm, n_ranks, u, rank));
  ctx->proc_ranks = n_ranks;
  ctx->proc_rank = rank;
  return KCC_OK;
}

int kcc_allreduce_partial_async(kcc_ctx* ctx, int64_t n_specs, int64_t* d_partial, void* stream) {
  if (!ctx) return KCC_EINVAL;
  if (n_specs < 0) return fail(ctx, KCC_EINVAL, "negative size");
  if (!ctx->proc_comm) return fail(ctx, KCC_EINVAL, "no communicator (kcc_comm_init)");
  if (n_specs == 0) return KCC_OK;
  if (!d_partial) return fail(ctx, KCC_EINVAL, "NULL partial");
  KCC_HIP(ctx, hipSetDevice(ctx->devs[0].device));
  KCC_NCCL(ctx, ncclAllReduce(d_partial, d_partial, 2 * (size_t)n_specs, ncclInt64, ncclSum,
                              ctx->proc_comm, static_cast<hipStream_t>(stream)));
  return KCC_OK;
}

// ---- one-shot exchange over xGMI peer memory (kcc_p2p_*) ---------------------------

int kcc_p2p_export(kcc_ctx* ctx, int n_ranks, int64_t max_specs, uint8_t* handle) {
  if (!ctx) return KCC_EINVAL;
  if (!handle || n_ranks < 1 || n_ranks > kcc::P2P_MAX_RANKS || max_specs < 1 ||
      max_specs > KCC_P2P_MAX_SPECS)
    return fail(ctx, KCC_EINVAL, "need a handle buffer, 1 <= n_ranks <= 8, 1 <= max_specs <= 2^20");
  if (ctx->devs.size() != 1)
    return fail(ctx, KCC_EINVAL, "a multi-process rank drives exactly one device");
  Dev& dv = ctx->devs[0];
  if (dv.p2p_W > 0) return fail(ctx, KCC_EINVAL, "mailbox already exported");
  KCC_HIP(ctx, hipSetDevice(dv.device));
  const size_t bytes = kcc::p2p_mbox_bytes(n_ranks, max_specs);
  {
    int rc = faults_ws(ctx, dv, dv.stream);
    if (rc) return rc;
  }
  KCC_HIP(ctx, ensure_uncached(dv.p2p_mbox, bytes));
  KCC_HIP(ctx, ensure(dv.p2p_arrive, 64));
  KCC_HIP(ctx, hipMemset(dv.p2p_mbox.p, 0, bytes));  // flags 0: no epoch seen
  KCC_HIP(ctx, hipMemset(dv.p2p_arrive.p, 0, 64));   // no arrivals, epoch 0 pushed
  KCC_HIP(ctx, hipDeviceSynchronize());
  static_assert(sizeof(hipIpcMemHandle_t) == KCC_P2P_HANDLE_BYTES, "IPC handle size");
  hipIpcMemHandle_t h;
  KCC_HIP(ctx, hipIpcGetMemHandle(&h, dv.p2p_mbox.p));
  std::memcpy(handle, &h, sizeof(h));
  dv.p2p_W = n_ranks;
  dv.p2p_smax = max_specs;
  return KCC_OK;
}

int kcc_p2p_open(kcc_ctx* ctx, int rank, const uint8_t* handles) {
  if (!ctx) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  if (dv.p2p_W == 0) return fail(ctx, KCC_EINVAL, "kcc_p2p_export first");
  if (dv.p2p_ready) return fail(ctx, KCC_EINVAL, "peers already opened");
  if (!handles || rank < 0 || rank >= dv.p2p_W) return fail(ctx, KCC_EINVAL, "need handles and 0 <= rank < n_ranks");
  KCC_HIP(ctx, hipSetDevice(dv.device));
  for (int p = 0; p < dv.p2p_W; ++p) {
    if (p == rank) {
      dv.p2p_peer[p] = static_cast<unsigned char*>(dv.p2p_mbox.p);
      continue;
    }
    hipIpcMemHandle_t h;
    std::memcpy(&h, handles + (size_t)p * KCC_P2P_HANDLE_BYTES, sizeof(h));
    void* ptr = nullptr;
    const hipError_t e = hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) {
      for (int q = 0; q < p; ++q)
        if (q != rank && dv.p2p_peer[q]) (void)hipIpcCloseMemHandle(dv.p2p_peer[q]);
      for (auto& q : dv.p2p_peer) q = nullptr;
      return fail(ctx, KCC_EHIP, std::string("hipIpcOpenMemHandle(rank ") + std::to_string(p) +
                                     "): " + hipGetErrorString(e));
    }
    dv.p2p_peer[p] = static_cast<unsigned char*>(ptr);
  }
  dv.p2p_rank = rank;
  dv.p2p_ready = true;
  return KCC_OK;
}

int kcc_exchange_finalize_async(kcc_ctx* ctx, int64_t n_specs, const int64_t* d_partial,
                                int64_t* d_totals, int32_t* d_spec_err, void* stream) {
  if (!ctx) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  if (!dv.p2p_ready) return fail(ctx, KCC_EINVAL, "no peers (kcc_p2p_export + kcc_p2p_open)");
  if (n_specs < 0 || n_specs > dv.p2p_smax)
    return fail(ctx, KCC_EINVAL, "n_specs outside [0, the mailbox's max_specs]");
  if (n_specs == 0) return KCC_OK;
  if (!d_partial || !d_totals || !d_spec_err) return fail(ctx, KCC_EINVAL, "NULL partial/totals/err");
  if (dv.sperm.bytes < sizeof(int32_t) * (size_t)n_specs)
    return fail(ctx, KCC_EINVAL, "exchange without a matching fit_partial");
  KCC_HIP(ctx, hipSetDevice(dv.device));
  kcc::P2PArgs a{};
  a.S = n_specs;
  a.smax = dv.p2p_smax;
  a.W = dv.p2p_W;
  a.rank = dv.p2p_rank;
  a.epoch = as<uint64_t>(dv.p2p_arrive) + 1;  // (word 0: the arrival counter)
  a.partial = d_partial;
  for (int p = 0; p < dv.p2p_W; ++p) a.mbox[p] = dv.p2p_peer[p];
  a.perm = as<int32_t>(dv.sperm);
  a.totals = d_totals;
  a.spec_err = d_spec_err;
  a.arrive = as<uint32_t>(dv.p2p_arrive);
  a.faults = as<unsigned long long>(dv.faults);
  KCC_HIP(ctx, kcc::launch_exchange_finalize(a, static_cast<hipStream_t>(stream)));
  return KCC_OK;
}

int kcc_p2p_faults(kcc_ctx* ctx, int64_t* faults) {
  if (!ctx || !faults) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  *faults = 0;
  if (!dv.faults.p) return KCC_OK;
  KCC_HIP(ctx, hipSetDevice(dv.device));
  KCC_HIP(ctx, hipDeviceSynchronize());
  unsigned long long f = 0;
  KCC_HIP(ctx, hipMemcpy(&f, as<unsigned long long>(dv.faults) + kcc::FAULT_P2P, sizeof(f),
                         hipMemcpyDeviceToHost));
  *faults = (int64_t)f;
  return KCC_OK;
}

}  // extern "C"


// ---- quantity-string parse --------------------------------------

namespace {

// Argument checks of the parsers' entry points (host or device pointers alike).
int check_parse(kcc_ctx* ctx, int64_t n, const char* bytes, int64_t n_bytes,
                const int64_t* offsets, const int64_t* out, const int8_t* status) {
  if (n < 0 || n_bytes < 0) return fail(ctx, KCC_EINVAL, "negative size");
  if (n > 0 && (!offsets || !out || !status || (n_bytes > 0 && !bytes)))
    return fail(ctx, KCC_EINVAL, "NULL bytes/offsets/out/status");
  return KCC_OK;
}

int parse_async_dev(kcc_ctx* ctx, int mode, int64_t n, const char* bytes, int64_t n_bytes,
                    const int64_t* offsets, int64_t* out, int8_t* status, hipStream_t s) {
  const int rc = check_parse(ctx, n, bytes, n_bytes, offsets, out, status);
  if (rc || n == 0) return rc;
  if ((reinterpret_cast<uintptr_t>(bytes) & 3u) != 0)
    return fail(ctx, KCC_EINVAL, "bytes must be 4-byte aligned");
  KCC_HIP(ctx, kcc::launch_parse(mode, n, reinterpret_cast<const uint8_t*>(bytes), n_bytes,
                                 offsets, out, status, s));
  return KCC_OK;
}

int parse_host(kcc_ctx* ctx, int mode, int64_t n, const char* bytes, int64_t n_bytes,
               const int64_t* offsets, int64_t* out, int8_t* status) {
  if (!ctx) return KCC_EINVAL;
  int rc = check_parse(ctx, n, bytes, n_bytes, offsets, out, status);
  if (rc) return rc;
  if (n > 0 && (offsets[0] < 0 || offsets[n] > n_bytes))
    return fail(ctx, KCC_EINVAL, "offsets outside [0, n_bytes]");
  for (int64_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return fail(ctx, KCC_EINVAL, "offsets are not non-decreasing");
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  Stage st(ctx, dv);
  if ((rc = st.in(bytes, n_bytes)) || (rc = st.in(offsets, csr_len(n))) || (rc = st.out(out, n)) ||
      (rc = st.out(status, n)) ||
      (rc = parse_async_dev(ctx, mode, n, bytes, n_bytes, offsets, out, status, dv.stream)))
    return rc;
  return st.finish();
}

}  // namespace

int kcc_parse_cpu_millis(kcc_ctx* ctx, int64_t n, const char* bytes, int64_t n_bytes,
                         const int64_t* offsets, uint64_t* out, int8_t* status) {
  return parse_host(ctx, kcc::PARSE_MODE_CPU_MILLIS, n, bytes, n_bytes, offsets,
                    reinterpret_cast<int64_t*>(out), status);
}

int kcc_parse_bytes(kcc_ctx* ctx, int64_t n, const char* bytes, int64_t n_bytes,
                    const int64_t* offsets, int64_t* out, int8_t* status) {
  return parse_host(ctx, kcc::PARSE_MODE_BYTES, n, bytes, n_bytes, offsets, out, status);
}

int kcc_parse_quantity(kcc_ctx* ctx, int64_t n, const char* bytes, int64_t n_bytes,
                       const int64_t* offsets, int64_t* out, int8_t* status) {
  return parse_host(ctx, kcc::PARSE_MODE_QUANTITY, n, bytes, n_bytes, offsets, out, status);
}

int kcc_parse_quantity_async(kcc_ctx* ctx, int64_t n, const char* d_bytes, int64_t n_bytes,
                             const int64_t* d_offsets, int64_t* d_out, int8_t* d_status,
                             void* stream) {
  if (!ctx) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  return parse_async_dev(ctx, kcc::PARSE_MODE_QUANTITY, n, d_bytes, n_bytes, d_offsets, d_out,
                         d_status, static_cast<hipStream_t>(stream));
}

int kcc_parse_cpu_millis_async(kcc_ctx* ctx, int64_t n, const char* d_bytes, int64_t n_bytes,
                               const int64_t* d_offsets, uint64_t* d_out, int8_t* d_status,
                               void* stream) {
  if (!ctx) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  return parse_async_dev(ctx, kcc::PARSE_MODE_CPU_MILLIS, n, d_bytes, n_bytes, d_offsets,
                         reinterpret_cast<int64_t*>(d_out), d_status,
                         static_cast<hipStream_t>(stream));
}

int kcc_parse_bytes_async(kcc_ctx* ctx, int64_t n, const char* d_bytes, int64_t n_bytes,
                          const int64_t* d_offsets, int64_t* d_out, int8_t* d_status,
                          void* stream) {
  if (!ctx) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  return parse_async_dev(ctx, kcc::PARSE_MODE_BYTES, n, d_bytes, n_bytes, d_offsets, d_out,
                         d_status, static_cast<hipStream_t>(stream));
}


// ---- list-order (keyed) reduce ------------------------------------

namespace {

// Workspace of the bucketed keyed reduce (grows on demand); nullptr when the keys do not
// fit the bucketed path (the kernels then fall back to device atomics).
int keyed_work(kcc_ctx* ctx, Dev& dv, int64_t n_keys, int64_t n, int na, kcc::KeyedWork& kw,
               const kcc::KeyedWork** out) {
  *out = nullptr;
  if (!kcc::keyed_bucketed(n_keys, n)) return KCC_OK;
  {
    int rc = faults_ws(ctx, dv, dv.stream);  // (the gather's bounded wait reports here)
    if (rc) return rc;
  }
  const size_t nb = (size_t)kcc::keyed_buckets(n_keys);
  const size_t m = (size_t)(n > 0 ? n : 1);
  KCC_HIP(ctx, ensure(dv.kb_counts, 4 * (size_t)kcc::keyed_counts_words(n_keys, n)));
  KCC_HIP(ctx, ensure(dv.kb_tot, 4 * nb));
  KCC_HIP(ctx, ensure(dv.kb_sr, 8 * (size_t)kcc::keyed_sr_slots(n)));
  KCC_HIP(ctx, ensure(dv.kb_part, 8 * (size_t)kcc::keyed_part_words(n_keys, na > 2 ? 2 : na)));
  if (dv.kb_arrive.bytes < 8 * nb) {  // [arrivals | published parts]: every gather leaves them zero
    KCC_HIP(ctx, ensure(dv.kb_arrive, 8 * nb));
    KCC_HIP(ctx, hipMemsetAsync(dv.kb_arrive.p, 0, dv.kb_arrive.bytes, dv.stream));
    KCC_HIP(ctx, hipStreamSynchronize(dv.stream));
  }
  if (na > 2) KCC_HIP(ctx, ensure(dv.kb_sv, 8 * (size_t)(na - 2) * m));
  if (na >= 2) {
    const size_t ne = (size_t)(n > 0 ? n : 1);
    if (!dv.kb_esc_n.p) {  // [0] list length, [1] kb_escape's arrivals: zero between calls
      KCC_HIP(ctx, ensure(dv.kb_esc_n, 16));
      KCC_HIP(ctx, hipMemsetAsync(dv.kb_esc_n.p, 0, 16, dv.stream));
      KCC_HIP(ctx, hipStreamSynchronize(dv.stream));
    }
    KCC_HIP(ctx, ensure(dv.kb_esc_row, 4 * ne));
    KCC_HIP(ctx, ensure(dv.kb_esc_cpu, 8 * ne));
    KCC_HIP(ctx, ensure(dv.kb_esc_mem, 8 * ne));
  }
  kw.counts = as<uint32_t>(dv.kb_counts);
  kw.tot = as<uint32_t>(dv.kb_tot);
  kw.sr = as<uint64_t>(dv.kb_sr);
  kw.sv = na > 2 ? as<uint64_t>(dv.kb_sv) : nullptr;
  kw.esc_n = na >= 2 ? as<uint32_t>(dv.kb_esc_n) : nullptr;
  kw.esc_row = na >= 2 ? as<int32_t>(dv.kb_esc_row) : nullptr;
  kw.esc_cpu = na >= 2 ? as<uint64_t>(dv.kb_esc_cpu) : nullptr;
  kw.esc_mem = na >= 2 ? as<uint64_t>(dv.kb_esc_mem) : nullptr;
  kw.part_acc = as<uint64_t>(dv.kb_part);
  kw.arrive = as<uint32_t>(dv.kb_arrive);
  kw.faults = as<unsigned long long>(dv.faults);
  *out = &kw;
  return KCC_OK;
}

// Argument checks of the keyed reduce's two entry points (host or device pointers alike).
int check_keyed(kcc_ctx* ctx, int64_t n_keys, int64_t n, const int32_t* key, const uint64_t* cpu,
                const int64_t* mem, const uint64_t* cpul, const int64_t* meml,
                const uint64_t* used_cpu, const int64_t* used_mem, const uint64_t* lim_cpu,
                const int64_t* lim_mem) {
  if (n_keys < 0 || n < 0) return fail(ctx, KCC_EINVAL, "negative size");
  if (n_keys > 0x7fffffff) return fail(ctx, KCC_EINVAL, "more than 2^31 - 1 keys");
  if (n_keys > 0 && (!used_cpu || !used_mem)) return fail(ctx, KCC_EINVAL, "NULL output");
  if (n > 0 && (!key || !cpu || !mem)) return fail(ctx, KCC_EINVAL, "NULL key/cpu_req/mem_req");
  if ((cpul || meml) && (!cpul || !meml || (n_keys > 0 && (!lim_cpu || !lim_mem))))
    return fail(ctx, KCC_EINVAL, "limits need cpu_lim, mem_lim, lim_cpu and lim_mem");
  return KCC_OK;
}

int keyed_async_dev(kcc_ctx* ctx, Dev& dv, int64_t n_keys, int64_t n, const int32_t* key,
                    const uint64_t* cpu, const int64_t* mem, const uint64_t* cpul,
                    const int64_t* meml, uint64_t* used_cpu, int64_t* used_mem, uint64_t* lim_cpu,
                    int64_t* lim_mem, hipStream_t s) {
  int rc = check_keyed(ctx, n_keys, n, key, cpu, mem, cpul, meml, used_cpu, used_mem, lim_cpu,
                       lim_mem);
  if (rc) return rc;
  const bool lim = cpul != nullptr;
  if (!aligned16(key) || !aligned16(cpu) || !aligned16(mem) ||
      (lim && (!aligned16(cpul) || !aligned16(meml))))
    return fail(ctx, KCC_EINVAL, "key and container arrays must be 16-byte aligned");
  kcc::KeyedWork kw{};
  const kcc::KeyedWork* kwp = nullptr;
  if ((rc = keyed_work(ctx, dv, n_keys, n, lim ? 4 : 2, kw, &kwp))) return rc;
  KCC_HIP(ctx, kcc::launch_reduce_keyed(n_keys, n, key, cpu, mem, lim ? cpul : nullptr,
                                        lim ? meml : nullptr, used_cpu, used_mem,
                                        lim ? lim_cpu : nullptr, lim ? lim_mem : nullptr, kwp, s));
  return KCC_OK;
}

// Argument checks of kcc_count_by_key's two entry points (host or device pointers alike).
int check_count(kcc_ctx* ctx, int64_t n_keys, int64_t n, const int32_t* key, const int64_t* count) {
  if (n_keys < 0 || n < 0) return fail(ctx, KCC_EINVAL, "negative size");
  if (n_keys > 0x7fffffff) return fail(ctx, KCC_EINVAL, "more than 2^31 - 1 keys");
  if ((n_keys > 0 && !count) || (n > 0 && !key)) return fail(ctx, KCC_EINVAL, "NULL key/count");
  return KCC_OK;
}

int count_async_dev(kcc_ctx* ctx, Dev& dv, int64_t n_keys, int64_t n, const int32_t* key,
                    int64_t* count, hipStream_t s) {
  int rc = check_count(ctx, n_keys, n, key, count);
  if (rc) return rc;
  if (!aligned16(key)) return fail(ctx, KCC_EINVAL, "key must be 16-byte aligned");
  kcc::KeyedWork kw{};
  const kcc::KeyedWork* kwp = nullptr;
  if ((rc = keyed_work(ctx, dv, n_keys, n, 0, kw, &kwp))) return rc;
  KCC_HIP(ctx, kcc::launch_count_keyed(n_keys, n, key, count, kwp, s));
  return KCC_OK;
}

}  // namespace

extern "C" {

int kcc_reduce_requests_keyed_async(kcc_ctx* ctx, int64_t n_keys, int64_t n_containers,
                                    const int32_t* d_key, const uint64_t* d_cpu_req,
                                    const int64_t* d_mem_req, const uint64_t* d_cpu_lim,
                                    const int64_t* d_mem_lim, uint64_t* d_used_cpu,
                                    int64_t* d_used_mem, uint64_t* d_lim_cpu, int64_t* d_lim_mem,
                                    void* stream) {
  if (!ctx) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  return keyed_async_dev(ctx, dv, n_keys, n_containers, d_key, d_cpu_req, d_mem_req, d_cpu_lim,
                         d_mem_lim, d_used_cpu, d_used_mem, d_lim_cpu, d_lim_mem,
                         static_cast<hipStream_t>(stream));
}

int kcc_reduce_requests_keyed(kcc_ctx* ctx, int64_t n_keys, int64_t n_containers,
                              const int32_t* key, const uint64_t* cpu_req, const int64_t* mem_req,
                              const uint64_t* cpu_lim, const int64_t* mem_lim,
                              uint64_t* used_cpu, int64_t* used_mem, uint64_t* lim_cpu,
                              int64_t* lim_mem) {
  if (!ctx) return KCC_EINVAL;
  int rc = check_keyed(ctx, n_keys, n_containers, key, cpu_req, mem_req, cpu_lim, mem_lim, used_cpu,
                       used_mem, lim_cpu, lim_mem);
  if (rc) return rc;
  if (!cpu_lim) {  // no limits: their sums are not written
    lim_cpu = nullptr;
    lim_mem = nullptr;
  }
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  Stage st(ctx, dv);
  if ((rc = st.in(key, n_containers)) || (rc = st.in(cpu_req, n_containers)) ||
      (rc = st.in(mem_req, n_containers)) || (rc = st.in(cpu_lim, n_containers)) ||
      (rc = st.in(mem_lim, n_containers)) || (rc = st.out(used_cpu, n_keys)) ||
      (rc = st.out(used_mem, n_keys)) || (rc = st.out(lim_cpu, n_keys)) ||
      (rc = st.out(lim_mem, n_keys)) ||
      (rc = keyed_async_dev(ctx, dv, n_keys, n_containers, key, cpu_req, mem_req, cpu_lim, mem_lim,
                            used_cpu, used_mem, lim_cpu, lim_mem, dv.stream)))
    return rc;
  return st.finish(true);
}

int kcc_count_by_key_async(kcc_ctx* ctx, int64_t n_keys, int64_t n, const int32_t* d_key,
                           int64_t* d_count, void* stream) {
  if (!ctx) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  return count_async_dev(ctx, dv, n_keys, n, d_key, d_count, static_cast<hipStream_t>(stream));
}

int kcc_count_by_key(kcc_ctx* ctx, int64_t n_keys, int64_t n, const int32_t* key, int64_t* count) {
  if (!ctx) return KCC_EINVAL;
  int rc = check_count(ctx, n_keys, n, key, count);
  if (rc) return rc;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  Stage st(ctx, dv);
  if ((rc = st.in(key, n)) || (rc = st.out(count, n_keys)) ||
      (rc = count_async_dev(ctx, dv, n_keys, n, key, count, dv.stream)))
    return rc;
  return st.finish(true);
}

}  // extern "C"


// ---- per-row q of one spec -----------------------------------------

extern "C" int kcc_fit_rows(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu,
                            const int64_t* alloc_mem, const int64_t* alloc_pods,
                            const int64_t* pod_count, const uint64_t* used_cpu,
                            const int64_t* used_mem, uint64_t spec_cpu, int64_t spec_mem,
                            int64_t* q, int32_t* row_err) {
  if (!ctx) return KCC_EINVAL;
  if (n_nodes < 0) return fail(ctx, KCC_EINVAL, "negative size");
  if (n_nodes == 0) return KCC_OK;
  if (!alloc_cpu || !alloc_mem || !alloc_pods || !pod_count || !used_cpu || !used_mem || !q ||
      !row_err)
    return fail(ctx, KCC_EINVAL, "NULL node array / output");
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  Stage st(ctx, dv);
  int rc;
  if ((rc = st.in(alloc_cpu, n_nodes)) || (rc = st.in(alloc_mem, n_nodes)) ||
      (rc = st.in(alloc_pods, n_nodes)) || (rc = st.in(pod_count, n_nodes)) ||
      (rc = st.in(used_cpu, n_nodes)) || (rc = st.in(used_mem, n_nodes)) ||
      (rc = st.out(q, n_nodes)) || (rc = st.out(row_err, n_nodes)))
    return rc;
  KCC_HIP(ctx, kcc::launch_fit_rows(n_nodes, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu,
                                    used_mem, spec_cpu, spec_mem, q, row_err, dv.stream));
  return st.finish();
}


// ---- the cell fits: per node-group x spec totals (kcc_ext.hip, kcc_spread.hip) ---------
// kcc_fit_grouped, kcc_fit_ext and kcc_fit_capped are one path.  The extended fit is the
// capped one without node_cap, cell_min and group_rows; the grouped fit is the extended one
// with n_ext = 0 and group ids it insists on (need_group).

namespace {

// Argument checks of the six entry points (host or device pointers alike).
int check_cells(kcc_ctx* ctx, const kcc::FitNodes& nd, const kcc::FitSpecs& sp, bool need_group,
                const int64_t* totals, const int32_t* spec_err) {
  if (nd.n < 0 || sp.S < 0) return fail(ctx, KCC_EINVAL, "negative size");
  if (nd.R < 0 || nd.R > KCC_EXT_MAX) return fail(ctx, KCC_EINVAL, "n_ext must be in [0, KCC_EXT_MAX]");
  if (nd.G < 1) return fail(ctx, KCC_EINVAL, "n_groups must be at least 1");
  if (!need_group && !nd.group && nd.G != 1)
    return fail(ctx, KCC_EINVAL, "group is NULL: n_groups must be 1");
  if (nd.n > kcc::GRP_MAX_NODES) return fail(ctx, KCC_EINVAL, "too many nodes (max 2^31 - 4096)");
  if (sp.S > kcc::GRP_MAX_CELLS || nd.G > kcc::GRP_MAX_CELLS || nd.G * sp.S > kcc::GRP_MAX_CELLS)
    return fail(ctx, KCC_EINVAL, "too many cells: n_groups x n_specs must not exceed 2^28");
  if (sp.S > 0 && (!sp.spec_cpu || !sp.spec_mem || !totals || !spec_err))
    return fail(ctx, KCC_EINVAL, "NULL spec array / output");
  if (nd.n > 0 && (!nd.alloc_cpu || !nd.alloc_mem || !nd.alloc_pods || !nd.pod_count ||
                   !nd.used_cpu || !nd.used_mem))
    return fail(ctx, KCC_EINVAL, "NULL node array");
  if (need_group && nd.n > 0 && !nd.group) return fail(ctx, KCC_EINVAL, "group is NULL");
  if (nd.R > 0 && ((nd.n > 0 && (!nd.alloc_x || !nd.used_x)) || (sp.S > 0 && !sp.spec_x)))
    return fail(ctx, KCC_EINVAL, "NULL extra-resource array with n_ext > 0");
  return KCC_OK;
}

// Device level: the degenerate cases, the grid limit, the workspaces and the launches on s.
// cell_min [G S] and group_rows [G] are kcc_fit_capped's outputs (nullptr elsewhere).
int fit_cells_dev(kcc_ctx* ctx, Dev& dv, const kcc::FitNodes& nd, const kcc::FitSpecs& sp,
                  bool need_group, int64_t* totals, int32_t* spec_err, int64_t* cell_min,
                  int64_t* group_rows, hipStream_t s) {
  int rc = check_cells(ctx, nd, sp, need_group, totals, spec_err);
  if (rc) return rc;
  const size_t cells = (size_t)(nd.G * sp.S);
  if (nd.n == 0) {  // no rows: every cell empty, every group empty
    if (sp.S > 0) {
      KCC_HIP(ctx, hipMemsetAsync(totals, 0, 8 * cells, s));
      KCC_HIP(ctx, hipMemsetAsync(spec_err, 0, 4 * cells, s));
      if (cell_min) KCC_HIP(ctx, kcc::launch_fill_i64((int64_t)cells, INT64_MAX, cell_min, s));
    }
    if (group_rows) KCC_HIP(ctx, hipMemsetAsync(group_rows, 0, 8 * (size_t)nd.G, s));
    return KCC_OK;
  }
  if (sp.S == 0 && !group_rows) return KCC_OK;  // no cells; the groups' rows are still counted
  if (sp.S > 0 && !kcc::ext_sizes_ok(nd, sp.S))  // (check_cells has passed everything else)
    return fail(ctx, KCC_EINVAL, "n_nodes x n_specs beyond one launch (2^31 - 1 workgroups of 256 x 256 pairs)");
  if (nd.group) {
    KCC_HIP(ctx, ensure(dv.g_count, 4 * (size_t)nd.G));
    KCC_HIP(ctx, ensure(dv.g_cursor, 4 * (size_t)nd.G));
    KCC_HIP(ctx, ensure(dv.g_total, 16));
  }
  if (sp.S > 0) {
    KCC_HIP(ctx, ensure(dv.g_rec, sizeof(kcc::GrpRow) * (size_t)nd.n));
    KCC_HIP(ctx, ensure(dv.g_rg, 4 * (size_t)nd.n));
    KCC_HIP(ctx, ensure(dv.g_acc, 16 * cells));
    if (nd.R > 0) KCC_HIP(ctx, ensure(dv.x_rec, sizeof(kcc::ExtCol) * (size_t)nd.n * (size_t)nd.R));
    if (cell_min) KCC_HIP(ctx, ensure(dv.sp_qmin, 8 * cells));
  }
  const kcc::ExtWork w{{as<uint32_t>(dv.g_count), as<uint32_t>(dv.g_cursor), as<uint32_t>(dv.g_total),
                        as<kcc::GrpRow>(dv.g_rec), as<int32_t>(dv.g_rg), as<int64_t>(dv.g_acc)},
                       as<kcc::ExtCol>(dv.x_rec)};
  if (sp.S == 0)
    KCC_HIP(ctx, kcc::launch_group_rows(nd.n, nd.G, nd.group, w.g, group_rows, s));
  else
    KCC_HIP(ctx, kcc::launch_fit_capped(nd, sp, w, as<unsigned long long>(dv.sp_qmin), totals,
                                        spec_err, cell_min, group_rows, s));
  return KCC_OK;
}

int fit_cells_async(kcc_ctx* ctx, const kcc::FitNodes& nd, const kcc::FitSpecs& sp,
                    bool need_group, int64_t* totals, int32_t* spec_err, int64_t* cell_min,
                    int64_t* group_rows, void* stream) {
  if (!ctx) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  return fit_cells_dev(ctx, dv, nd, sp, need_group, totals, spec_err, cell_min, group_rows,
                       static_cast<hipStream_t>(stream));
}

// The cell fits' thirteen input arrays, staged.
int stage_cells(Stage& st, kcc::FitNodes& nd, kcc::FitSpecs& sp) {
  const int64_t n = nd.n, S = sp.S;
  int rc;
  if ((rc = st.in(nd.alloc_cpu, n)) || (rc = st.in(nd.alloc_mem, n)) ||
      (rc = st.in(nd.alloc_pods, n)) || (rc = st.in(nd.pod_count, n)) ||
      (rc = st.in(nd.used_cpu, n)) || (rc = st.in(nd.used_mem, n)) ||
      (rc = st.in(nd.alloc_x, nd.R * n)) || (rc = st.in(nd.used_x, nd.R * n)) ||
      (rc = st.in(nd.group, n)) || (rc = st.in(sp.spec_cpu, S)) || (rc = st.in(sp.spec_mem, S)) ||
      (rc = st.in(sp.spec_x, nd.R * S)) || (rc = st.in(sp.node_cap, S)))
    return rc;
  return KCC_OK;
}

// Host level: checks, stages, runs fit_cells_dev and copies the outputs back.
int fit_cells_host(kcc_ctx* ctx, kcc::FitNodes nd, kcc::FitSpecs sp, bool need_group,
                   int64_t* totals, int32_t* spec_err, int64_t* cell_min, int64_t* group_rows) {
  if (!ctx) return KCC_EINVAL;
  int rc = check_cells(ctx, nd, sp, need_group, totals, spec_err);
  if (rc) return rc;
  const int64_t cells = nd.G * sp.S;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  Stage st(ctx, dv);
  if ((rc = stage_cells(st, nd, sp)) || (rc = st.out(totals, cells)) ||
      (rc = st.out(spec_err, cells)) || (rc = st.out(cell_min, cells)) ||
      (rc = st.out(group_rows, nd.G)) ||
      (rc = fit_cells_dev(ctx, dv, nd, sp, need_group, totals, spec_err, cell_min, group_rows,
                          dv.stream)))
    return rc;
  return st.finish();
}

}  // namespace

extern "C" {

int kcc_fit_grouped_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                          const int64_t* d_alloc_mem, const int64_t* d_alloc_pods,
                          const int64_t* d_pod_count, const uint64_t* d_used_cpu,
                          const int64_t* d_used_mem, const int32_t* d_group, int64_t n_groups,
                          int64_t n_specs, const uint64_t* d_spec_cpu, const int64_t* d_spec_mem,
                          int64_t* d_totals, int32_t* d_spec_err, void* stream) {
  return fit_cells_async(ctx,
                         {n_nodes, d_alloc_cpu, d_alloc_mem, d_alloc_pods, d_pod_count, d_used_cpu,
                          d_used_mem, 0, nullptr, nullptr, d_group, n_groups},
                         {n_specs, d_spec_cpu, d_spec_mem, nullptr, nullptr}, true, d_totals,
                         d_spec_err, nullptr, nullptr, stream);
}

int kcc_fit_grouped(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu,
                    const int64_t* alloc_mem, const int64_t* alloc_pods, const int64_t* pod_count,
                    const uint64_t* used_cpu, const int64_t* used_mem, const int32_t* group,
                    int64_t n_groups, int64_t n_specs, const uint64_t* spec_cpu,
                    const int64_t* spec_mem, int64_t* totals, int32_t* spec_err) {
  return fit_cells_host(ctx,
                        {n_nodes, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem, 0,
                         nullptr, nullptr, group, n_groups},
                        {n_specs, spec_cpu, spec_mem, nullptr, nullptr}, true, totals, spec_err,
                        nullptr, nullptr);
}

int kcc_fit_ext_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                      const int64_t* d_alloc_mem, const int64_t* d_alloc_pods,
                      const int64_t* d_pod_count, const uint64_t* d_used_cpu,
                      const int64_t* d_used_mem, int64_t n_ext, const int64_t* d_alloc_x,
                      const int64_t* d_used_x, const int32_t* d_group, int64_t n_groups,
                      int64_t n_specs, const uint64_t* d_spec_cpu, const int64_t* d_spec_mem,
                      const int64_t* d_spec_x, int64_t* d_totals, int32_t* d_spec_err,
                      void* stream) {
  return fit_cells_async(ctx,
                         {n_nodes, d_alloc_cpu, d_alloc_mem, d_alloc_pods, d_pod_count, d_used_cpu,
                          d_used_mem, n_ext, d_alloc_x, d_used_x, d_group, n_groups},
                         {n_specs, d_spec_cpu, d_spec_mem, d_spec_x, nullptr}, false, d_totals,
                         d_spec_err, nullptr, nullptr, stream);
}

int kcc_fit_ext(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu, const int64_t* alloc_mem,
                const int64_t* alloc_pods, const int64_t* pod_count, const uint64_t* used_cpu,
                const int64_t* used_mem, int64_t n_ext, const int64_t* alloc_x,
                const int64_t* used_x, const int32_t* group, int64_t n_groups, int64_t n_specs,
                const uint64_t* spec_cpu, const int64_t* spec_mem, const int64_t* spec_x,
                int64_t* totals, int32_t* spec_err) {
  return fit_cells_host(ctx,
                        {n_nodes, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
                         n_ext, alloc_x, used_x, group, n_groups},
                        {n_specs, spec_cpu, spec_mem, spec_x, nullptr}, false, totals, spec_err,
                        nullptr, nullptr);
}

int kcc_fit_capped_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                         const int64_t* d_alloc_mem, const int64_t* d_alloc_pods,
                         const int64_t* d_pod_count, const uint64_t* d_used_cpu,
                         const int64_t* d_used_mem, int64_t n_ext, const int64_t* d_alloc_x,
                         const int64_t* d_used_x, const int32_t* d_group, int64_t n_groups,
                         int64_t n_specs, const uint64_t* d_spec_cpu, const int64_t* d_spec_mem,
                         const int64_t* d_spec_x, int64_t* d_totals, int32_t* d_spec_err,
                         const int64_t* d_node_cap, int64_t* d_cell_min, int64_t* d_group_rows,
                         void* stream) {
  return fit_cells_async(ctx,
                         {n_nodes, d_alloc_cpu, d_alloc_mem, d_alloc_pods, d_pod_count, d_used_cpu,
                          d_used_mem, n_ext, d_alloc_x, d_used_x, d_group, n_groups},
                         {n_specs, d_spec_cpu, d_spec_mem, d_spec_x, d_node_cap}, false, d_totals,
                         d_spec_err, d_cell_min, d_group_rows, stream);
}

int kcc_fit_capped(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu,
                   const int64_t* alloc_mem, const int64_t* alloc_pods, const int64_t* pod_count,
                   const uint64_t* used_cpu, const int64_t* used_mem, int64_t n_ext,
                   const int64_t* alloc_x, const int64_t* used_x, const int32_t* group,
                   int64_t n_groups, int64_t n_specs, const uint64_t* spec_cpu,
                   const int64_t* spec_mem, const int64_t* spec_x, int64_t* totals,
                   int32_t* spec_err, const int64_t* node_cap, int64_t* cell_min,
                   int64_t* group_rows) {
  return fit_cells_host(ctx,
                        {n_nodes, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
                         n_ext, alloc_x, used_x, group, n_groups},
                        {n_specs, spec_cpu, spec_mem, spec_x, node_cap}, false, totals, spec_err,
                        cell_min, group_rows);
}

}  // extern "C"


// ---- the fit explained: kcc_fit_capped with each pair's binding term kept (kcc_explain.hip) --

namespace {

// The three nullable plane-major outputs of kcc_fit_explain.
struct ExplainOut {
  int64_t* why_rows;  // [KCC_WHY_SLOTS][G S]
  int64_t* why_pods;  // [KCC_WHY_SLOTS][G S]
  int64_t* left;      // [2 + R][G S]
};

int check_explain(kcc_ctx* ctx, const kcc::FitNodes& nd, const kcc::FitSpecs& sp,
                  const int64_t* totals, const int32_t* spec_err, const ExplainOut& o) {
  const int rc = check_cells(ctx, nd, sp, false, totals, spec_err);
  if (rc) return rc;
  if ((o.why_rows || o.why_pods) && KCC_WHY_SLOTS * nd.G * sp.S > kcc::GRP_MAX_CELLS)
    return fail(ctx, KCC_EINVAL, "too many cells: KCC_WHY_SLOTS x n_groups x n_specs must not exceed 2^28");
  return KCC_OK;
}

// Device level (the caller has passed check_explain): the degenerate cases, the grid limit,
// the workspaces and the launches on s.
int fit_explain_dev(kcc_ctx* ctx, Dev& dv, const kcc::FitNodes& nd, const kcc::FitSpecs& sp,
                    int64_t* totals, int32_t* spec_err, const ExplainOut& o, hipStream_t s) {
  if (!o.why_rows && !o.why_pods && !o.left)  // kcc_fit_capped itself
    return fit_cells_dev(ctx, dv, nd, sp, false, totals, spec_err, nullptr, nullptr, s);
  if (sp.S == 0) return KCC_OK;  // no cells
  const size_t cells = (size_t)(nd.G * sp.S);
  if (nd.n == 0) {  // no rows: every cell empty
    KCC_HIP(ctx, hipMemsetAsync(totals, 0, 8 * cells, s));
    KCC_HIP(ctx, hipMemsetAsync(spec_err, 0, 4 * cells, s));
    if (o.why_rows) KCC_HIP(ctx, hipMemsetAsync(o.why_rows, 0, 8 * KCC_WHY_SLOTS * cells, s));
    if (o.why_pods) KCC_HIP(ctx, hipMemsetAsync(o.why_pods, 0, 8 * KCC_WHY_SLOTS * cells, s));
    if (o.left) KCC_HIP(ctx, hipMemsetAsync(o.left, 0, 8 * (size_t)(2 + nd.R) * cells, s));
    return KCC_OK;
  }
  if (!kcc::ext_sizes_ok(nd, sp.S))
    return fail(ctx, KCC_EINVAL, "n_nodes x n_specs beyond one launch (2^31 - 1 workgroups of 256 x 256 pairs)");
  if (nd.group) {
    KCC_HIP(ctx, ensure(dv.g_count, 4 * (size_t)nd.G));
    KCC_HIP(ctx, ensure(dv.g_cursor, 4 * (size_t)nd.G));
    KCC_HIP(ctx, ensure(dv.g_total, 16));
  }
  KCC_HIP(ctx, ensure(dv.g_rec, sizeof(kcc::GrpRow) * (size_t)nd.n));
  KCC_HIP(ctx, ensure(dv.g_rg, 4 * (size_t)nd.n));
  KCC_HIP(ctx, ensure(dv.g_acc, 16 * cells));
  if (nd.R > 0) KCC_HIP(ctx, ensure(dv.x_rec, sizeof(kcc::ExtCol) * (size_t)nd.n * (size_t)nd.R));
  if (o.left) KCC_HIP(ctx, ensure(dv.ex_free, 8 * (size_t)(2 + nd.R) * (size_t)nd.G));
  const kcc::ExtWork w{{as<uint32_t>(dv.g_count), as<uint32_t>(dv.g_cursor), as<uint32_t>(dv.g_total),
                        as<kcc::GrpRow>(dv.g_rec), as<int32_t>(dv.g_rg), as<int64_t>(dv.g_acc)},
                       as<kcc::ExtCol>(dv.x_rec)};
  KCC_HIP(ctx, kcc::launch_fit_explain(nd, sp, w, as<unsigned long long>(dv.ex_free), totals,
                                       spec_err, o.why_rows, o.why_pods, o.left, s));
  return KCC_OK;
}

}  // namespace

extern "C" {

int kcc_fit_explain_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                          const int64_t* d_alloc_mem, const int64_t* d_alloc_pods,
                          const int64_t* d_pod_count, const uint64_t* d_used_cpu,
                          const int64_t* d_used_mem, int64_t n_ext, const int64_t* d_alloc_x,
                          const int64_t* d_used_x, const int32_t* d_group, int64_t n_groups,
                          int64_t n_specs, const uint64_t* d_spec_cpu, const int64_t* d_spec_mem,
                          const int64_t* d_spec_x, const int64_t* d_node_cap, int64_t* d_totals,
                          int32_t* d_spec_err, int64_t* d_why_rows, int64_t* d_why_pods,
                          int64_t* d_left, void* stream) {
  if (!ctx) return KCC_EINVAL;
  const kcc::FitNodes nd{n_nodes, d_alloc_cpu, d_alloc_mem, d_alloc_pods, d_pod_count, d_used_cpu,
                         d_used_mem, n_ext, d_alloc_x, d_used_x, d_group, n_groups};
  const kcc::FitSpecs sp{n_specs, d_spec_cpu, d_spec_mem, d_spec_x, d_node_cap};
  const ExplainOut o{d_why_rows, d_why_pods, d_left};
  const int rc = check_explain(ctx, nd, sp, d_totals, d_spec_err, o);
  if (rc) return rc;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  return fit_explain_dev(ctx, dv, nd, sp, d_totals, d_spec_err, o, static_cast<hipStream_t>(stream));
}

int kcc_fit_explain(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu,
                    const int64_t* alloc_mem, const int64_t* alloc_pods, const int64_t* pod_count,
                    const uint64_t* used_cpu, const int64_t* used_mem, int64_t n_ext,
                    const int64_t* alloc_x, const int64_t* used_x, const int32_t* group,
                    int64_t n_groups, int64_t n_specs, const uint64_t* spec_cpu,
                    const int64_t* spec_mem, const int64_t* spec_x, const int64_t* node_cap,
                    int64_t* totals, int32_t* spec_err, int64_t* why_rows, int64_t* why_pods,
                    int64_t* left) {
  if (!ctx) return KCC_EINVAL;
  kcc::FitNodes nd{n_nodes, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
                   n_ext, alloc_x, used_x, group, n_groups};
  kcc::FitSpecs sp{n_specs, spec_cpu, spec_mem, spec_x, node_cap};
  ExplainOut o{why_rows, why_pods, left};
  int rc = check_explain(ctx, nd, sp, totals, spec_err, o);
  if (rc) return rc;
  const int64_t cells = n_groups * n_specs;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  Stage st(ctx, dv);
  if ((rc = stage_cells(st, nd, sp)) || (rc = st.out(totals, cells)) ||
      (rc = st.out(spec_err, cells)) || (rc = st.out(o.why_rows, KCC_WHY_SLOTS * cells)) ||
      (rc = st.out(o.why_pods, KCC_WHY_SLOTS * cells)) || (rc = st.out(o.left, (2 + n_ext) * cells)) ||
      (rc = fit_explain_dev(ctx, dv, nd, sp, totals, spec_err, o, dv.stream)))
    return rc;
  return st.finish();
}

}  // extern "C"


// ---- spread fold: G x S cells to one total per spec (kcc_spread.hip) --------------------

namespace {

// Argument checks of both fold entry points (host or device pointers alike).
int check_fold(kcc_ctx* ctx, int64_t n_groups, int64_t n_specs, const int64_t* cell_totals,
               const int32_t* cell_err, const int32_t* domain_of, int64_t n_domains,
               const int64_t* totals, const int32_t* spec_err) {
  if (n_groups < 0 || n_specs < 0) return fail(ctx, KCC_EINVAL, "negative size");
  if (n_specs > 0 && (!totals || !spec_err)) return fail(ctx, KCC_EINVAL, "NULL output");
  if (n_groups == 0 || n_specs == 0) return KCC_OK;  // no cells: nothing else is looked at
  if (n_domains < 1) return fail(ctx, KCC_EINVAL, "n_domains must be at least 1");
  if (!domain_of && n_domains != n_groups)
    return fail(ctx, KCC_EINVAL, "domain_of is NULL: n_domains must equal n_groups");
  if (n_specs > kcc::GRP_MAX_CELLS || n_groups > kcc::GRP_MAX_CELLS ||
      n_domains > kcc::GRP_MAX_CELLS || n_groups * n_specs > kcc::GRP_MAX_CELLS ||
      n_domains * n_specs > kcc::GRP_MAX_CELLS)
    return fail(ctx, KCC_EINVAL, "too many cells: n_groups x n_specs and n_domains x n_specs must not exceed 2^28");
  if (!cell_totals || !cell_err) return fail(ctx, KCC_EINVAL, "NULL cell array");
  return KCC_OK;
}

int spread_fold_dev(kcc_ctx* ctx, Dev& dv, int64_t n_groups, int64_t n_specs,
                    const int64_t* cell_totals, const int32_t* cell_err,
                    const int64_t* group_rows, const int32_t* domain_of, int64_t n_domains,
                    const uint8_t* eligible, const int64_t* max_skew, int64_t* totals,
                    int32_t* spec_err, hipStream_t s) {
  int rc = check_fold(ctx, n_groups, n_specs, cell_totals, cell_err, domain_of, n_domains, totals,
                      spec_err);
  if (rc || n_specs == 0) return rc;
  if (n_groups == 0) {  // no cells: every total 0, no spec flagged
    KCC_HIP(ctx, hipMemsetAsync(totals, 0, 8 * (size_t)n_specs, s));
    KCC_HIP(ctx, hipMemsetAsync(spec_err, 0, 4 * (size_t)n_specs, s));
    return KCC_OK;
  }
  const size_t dcells = (size_t)(n_domains * n_specs);
  KCC_HIP(ctx, ensure(dv.f_cap, 8 * dcells));
  KCC_HIP(ctx, ensure(dv.f_present, 4 * dcells));
  KCC_HIP(ctx, ensure(dv.f_flag, 4 * (size_t)n_specs));
  const kcc::FoldWork w{as<int64_t>(dv.f_cap), as<uint32_t>(dv.f_present), as<uint32_t>(dv.f_flag)};
  KCC_HIP(ctx, kcc::launch_spread_fold(n_groups, n_specs, cell_totals, cell_err, group_rows,
                                       domain_of, n_domains, eligible, max_skew, w, totals,
                                       spec_err, s));
  return KCC_OK;
}

}  // namespace

extern "C" {

int kcc_spread_fold_async(kcc_ctx* ctx, int64_t n_groups, int64_t n_specs,
                          const int64_t* d_cell_totals, const int32_t* d_cell_err,
                          const int64_t* d_group_rows, const int32_t* d_domain_of,
                          int64_t n_domains, const uint8_t* d_eligible, const int64_t* d_max_skew,
                          int64_t* d_totals, int32_t* d_spec_err, void* stream) {
  if (!ctx) return KCC_EINVAL;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  return spread_fold_dev(ctx, dv, n_groups, n_specs, d_cell_totals, d_cell_err, d_group_rows,
                         d_domain_of, n_domains, d_eligible, d_max_skew, d_totals, d_spec_err,
                         static_cast<hipStream_t>(stream));
}

int kcc_spread_fold(kcc_ctx* ctx, int64_t n_groups, int64_t n_specs, const int64_t* cell_totals,
                    const int32_t* cell_err, const int64_t* group_rows, const int32_t* domain_of,
                    int64_t n_domains, const uint8_t* eligible, const int64_t* max_skew,
                    int64_t* totals, int32_t* spec_err) {
  if (!ctx) return KCC_EINVAL;
  int rc = check_fold(ctx, n_groups, n_specs, cell_totals, cell_err, domain_of, n_domains, totals,
                      spec_err);
  if (rc) return rc;
  const int64_t cells = n_groups * n_specs;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  Stage st(ctx, dv);
  if ((rc = st.in(cell_totals, cells)) || (rc = st.in(cell_err, cells)) ||
      (rc = st.in(group_rows, n_groups)) || (rc = st.in(domain_of, n_groups)) ||
      (rc = st.in(eligible, cells)) || (rc = st.in(max_skew, n_specs)) ||
      (rc = st.out(totals, n_specs)) || (rc = st.out(spec_err, n_specs)) ||
      (rc = spread_fold_dev(ctx, dv, n_groups, n_specs, cell_totals, cell_err, group_rows,
                            domain_of, n_domains, eligible, max_skew, totals, spec_err,
                            dv.stream)))
    return rc;
  return st.finish();
}

}  // extern "C"


// ---- a rollout plan committed to the node rows (kcc_deploy.hip) -------------------------

namespace {

struct DeployArgs {
  kcc::FitNodes nd;  // pod_count / used_* left nullptr: the state is the four pointers below
  int64_t* pod_count;
  uint64_t* used_cpu;
  int64_t* used_mem;
  int64_t* used_x;
  const uint8_t* eligible;
  kcc::DeployPlan plan;
  int64_t* placed;
  int64_t* nodes_used;
  int32_t* step_err;
  int64_t* placed_rows;
};

// Argument checks of both entry points (host or device pointers alike).
int check_deploy(kcc_ctx* ctx, const DeployArgs& a) {
  const kcc::FitNodes& nd = a.nd;
  const int64_t K = a.plan.K;
  if (nd.n < 0 || K < 0) return fail(ctx, KCC_EINVAL, "negative size");
  if (a.plan.policy != KCC_DEPLOY_PACK && a.plan.policy != KCC_DEPLOY_SPREAD)
    return fail(ctx, KCC_EINVAL, "policy must be KCC_DEPLOY_PACK or KCC_DEPLOY_SPREAD");
  if (nd.R < 0 || nd.R > KCC_EXT_MAX) return fail(ctx, KCC_EINVAL, "n_ext must be in [0, KCC_EXT_MAX]");
  if (nd.G < 1) return fail(ctx, KCC_EINVAL, "n_groups must be at least 1");
  if (!nd.group && nd.G != 1) return fail(ctx, KCC_EINVAL, "group is NULL: n_groups must be 1");
  if (nd.n > kcc::GRP_MAX_NODES) return fail(ctx, KCC_EINVAL, "too many nodes (max 2^31 - 4096)");
  if (K > kcc::DEPLOY_MAX_STEPS) return fail(ctx, KCC_EINVAL, "too many steps (max 2^20)");
  if (nd.G > kcc::GRP_MAX_CELLS || nd.G * K > kcc::GRP_MAX_CELLS)
    return fail(ctx, KCC_EINVAL, "too many cells: n_groups x n_steps must not exceed 2^28");
  if (K > 0 && (!a.plan.spec_cpu || !a.plan.spec_mem || !a.plan.replicas || !a.placed ||
                !a.nodes_used || !a.step_err))
    return fail(ctx, KCC_EINVAL, "NULL plan array / output");
  if (nd.n > 0 && (!nd.alloc_cpu || !nd.alloc_mem || !nd.alloc_pods || !a.pod_count ||
                   !a.used_cpu || !a.used_mem))
    return fail(ctx, KCC_EINVAL, "NULL node array");
  if (nd.R > 0 && ((nd.n > 0 && (!nd.alloc_x || !a.used_x)) || (K > 0 && !a.plan.spec_x)))
    return fail(ctx, KCC_EINVAL, "NULL extra-resource array with n_ext > 0");
  return KCC_OK;
}

// Device level: the checks, the degenerate cases, the workspaces (they only grow) and the
// launches on s.
int deploy_dev(kcc_ctx* ctx, Dev& dv, const DeployArgs& a, hipStream_t s) {
  const int rc = check_deploy(ctx, a);
  if (rc || a.plan.K == 0) return rc;  // no steps: nothing is written
  if (a.nd.n == 0) {  // no rows: nothing placed, no step flagged
    KCC_HIP(ctx, hipMemsetAsync(a.placed, 0, 8 * (size_t)a.plan.K, s));
    KCC_HIP(ctx, hipMemsetAsync(a.nodes_used, 0, 8 * (size_t)a.plan.K, s));
    KCC_HIP(ctx, hipMemsetAsync(a.step_err, 0, 4 * (size_t)a.plan.K, s));
    return KCC_OK;
  }
  const size_t tiles = (size_t)kcc::deploy_tiles(a.nd.n), K = (size_t)a.plan.K;
  KCC_HIP(ctx, ensure(dv.dp_a, 4 * (size_t)a.nd.n));
  KCC_HIP(ctx, ensure(dv.dp_tsum, 8 * tiles));
  KCC_HIP(ctx, ensure(dv.dp_toff, 8 * tiles));
  KCC_HIP(ctx, ensure(dv.dp_flag, 4 * K * kcc::DEPLOY_FLAG_STRIDE));
  KCC_HIP(ctx, ensure(dv.dp_st, 8 * K * 4 * kcc::DEPLOY_ST_WORDS));
  if (a.plan.policy == KCC_DEPLOY_SPREAD)
    KCC_HIP(ctx, ensure(dv.dp_bins, 8 * K * (size_t)kcc::DEPLOY_BIN_WORDS));
  const kcc::DeployWork w{as<uint32_t>(dv.dp_a),    as<uint64_t>(dv.dp_tsum), as<uint64_t>(dv.dp_toff),
                          as<uint32_t>(dv.dp_flag), as<uint64_t>(dv.dp_st),   as<uint64_t>(dv.dp_bins)};
  KCC_HIP(ctx, kcc::launch_deploy(a.nd, a.pod_count, a.used_cpu, a.used_mem, a.used_x, a.eligible,
                                  a.plan, w, a.placed, a.nodes_used, a.step_err, a.placed_rows, s));
  return KCC_OK;
}

}  // namespace

extern "C" {

int kcc_deploy_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                     const int64_t* d_alloc_mem, const int64_t* d_alloc_pods, int64_t n_ext,
                     const int64_t* d_alloc_x, int64_t* d_pod_count, uint64_t* d_used_cpu,
                     int64_t* d_used_mem, int64_t* d_used_x, const int32_t* d_group,
                     int64_t n_groups, const uint8_t* d_eligible, int64_t n_steps,
                     const uint64_t* d_spec_cpu, const int64_t* d_spec_mem,
                     const int64_t* d_spec_x, const int64_t* d_replicas,
                     const int64_t* d_node_cap, int policy, int64_t* d_placed,
                     int64_t* d_nodes_used, int32_t* d_step_err, int64_t* d_placed_rows,
                     void* stream) {
  if (!ctx) return KCC_EINVAL;
  const DeployArgs a{{n_nodes, d_alloc_cpu, d_alloc_mem, d_alloc_pods, nullptr, nullptr, nullptr,
                      n_ext, d_alloc_x, nullptr, d_group, n_groups},
                     d_pod_count, d_used_cpu, d_used_mem, d_used_x, d_eligible,
                     {n_steps, d_spec_cpu, d_spec_mem, d_spec_x, d_replicas, d_node_cap, policy},
                     d_placed, d_nodes_used, d_step_err, d_placed_rows};
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  return deploy_dev(ctx, dv, a, static_cast<hipStream_t>(stream));
}

int kcc_deploy(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu, const int64_t* alloc_mem,
               const int64_t* alloc_pods, int64_t n_ext, const int64_t* alloc_x,
               int64_t* pod_count, uint64_t* used_cpu, int64_t* used_mem, int64_t* used_x,
               const int32_t* group, int64_t n_groups, const uint8_t* eligible, int64_t n_steps,
               const uint64_t* spec_cpu, const int64_t* spec_mem, const int64_t* spec_x,
               const int64_t* replicas, const int64_t* node_cap, int policy, int64_t* placed,
               int64_t* nodes_used, int32_t* step_err, int64_t* placed_rows) {
  if (!ctx) return KCC_EINVAL;
  DeployArgs a{{n_nodes, alloc_cpu, alloc_mem, alloc_pods, nullptr, nullptr, nullptr, n_ext,
                alloc_x, nullptr, group, n_groups},
               pod_count, used_cpu, used_mem, used_x, eligible,
               {n_steps, spec_cpu, spec_mem, spec_x, replicas, node_cap, policy},
               placed, nodes_used, step_err, placed_rows};
  int rc = check_deploy(ctx, a);
  if (rc) return rc;
  const int64_t n = n_nodes, K = n_steps, R = n_ext;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  Stage st(ctx, dv);
  if ((rc = st.in(a.nd.alloc_cpu, n)) || (rc = st.in(a.nd.alloc_mem, n)) ||
      (rc = st.in(a.nd.alloc_pods, n)) || (rc = st.in(a.nd.alloc_x, R * n)) ||
      (rc = st.in(a.nd.group, n)) || (rc = st.in(a.eligible, n_groups * K)) ||
      (rc = st.in(a.plan.spec_cpu, K)) || (rc = st.in(a.plan.spec_mem, K)) ||
      (rc = st.in(a.plan.spec_x, R * K)) || (rc = st.in(a.plan.replicas, K)) ||
      (rc = st.in(a.plan.node_cap, K)) || (rc = st.inout(a.pod_count, n)) ||
      (rc = st.inout(a.used_cpu, n)) || (rc = st.inout(a.used_mem, n)) ||
      (rc = st.inout(a.used_x, R * n)) || (rc = st.out(a.placed, K)) ||
      (rc = st.out(a.nodes_used, K)) || (rc = st.out(a.step_err, K)) ||
      (rc = st.out(a.placed_rows, K * n)) || (rc = deploy_dev(ctx, dv, a, dv.stream)))
    return rc;
  return st.finish();
}

}  // extern "C"


// ---- opt-in scheduler request model (kcc_pods.hip) ------------------

namespace {

struct PodArgs {
  int64_t n_pods, n_cont, n_init;
  const int64_t* pod_ptr;
  const uint64_t* cpu_req;
  const int64_t* mem_req;
  const int64_t* init_ptr;
  const uint64_t* init_cpu;
  const int64_t* init_mem;
  const uint8_t* restartable;
  const uint64_t* ovh_cpu;
  const int64_t* ovh_mem;
};

// Argument checks of the pod model's entry points (host or device pointers alike).
int check_pods(kcc_ctx* ctx, const PodArgs& a, const uint64_t* pod_cpu, const int64_t* pod_mem) {
  if (a.n_pods < 0 || a.n_cont < 0 || a.n_init < 0) return fail(ctx, KCC_EINVAL, "negative size");
  if (a.n_pods == 0) return KCC_OK;
  if (!a.pod_ptr || !pod_cpu || !pod_mem) return fail(ctx, KCC_EINVAL, "NULL pod_ptr/output");
  if (a.n_cont > 0 && (!a.cpu_req || !a.mem_req))
    return fail(ctx, KCC_EINVAL, "NULL cpu_req/mem_req");
  if (a.init_ptr && a.n_init > 0 && (!a.init_cpu || !a.init_mem))
    return fail(ctx, KCC_EINVAL, "NULL init_cpu/init_mem");
  return KCC_OK;
}

// The host forms read the offsets: both CSR arrays are well formed, and there are no init
// container arrays without init_ptr.
int check_pods_csr(kcc_ctx* ctx, const PodArgs& a) {
  const int rc = check_csr(ctx, a.n_pods, a.n_cont, a.pod_ptr);
  if (rc) return rc;
  if (a.init_ptr) return check_csr(ctx, a.n_pods, a.n_init, a.init_ptr);
  if (a.n_init != 0 || a.init_cpu || a.init_mem || a.restartable)
    return fail(ctx, KCC_EINVAL, "init container arrays without init_ptr");
  return KCC_OK;
}

int pods_async_dev(kcc_ctx* ctx, const PodArgs& a, uint64_t* pod_cpu, int64_t* pod_mem,
                   hipStream_t s) {
  const int rc = check_pods(ctx, a, pod_cpu, pod_mem);
  if (rc) return rc;
  KCC_HIP(ctx, kcc::launch_pod_requests(a.n_pods, a.n_cont, a.init_ptr ? a.n_init : 0, a.pod_ptr,
                                        a.cpu_req, a.mem_req, a.init_ptr, a.init_cpu, a.init_mem,
                                        a.init_ptr ? a.restartable : nullptr, a.ovh_cpu, a.ovh_mem,
                                        pod_cpu, pod_mem, s));
  return KCC_OK;
}

// Stages the pod-level inputs and enqueues the per-pod kernel into pod_cpu / pod_mem (device).
int pods_stage_run(kcc_ctx* ctx, Dev& dv, Stage& st, PodArgs a, uint64_t* pod_cpu,
                   int64_t* pod_mem) {
  const int64_t n_init = a.init_ptr ? a.n_init : 0;
  int rc;
  if ((rc = st.in(a.pod_ptr, csr_len(a.n_pods))) || (rc = st.in(a.cpu_req, a.n_cont)) ||
      (rc = st.in(a.mem_req, a.n_cont)) || (rc = st.in(a.init_ptr, csr_len(a.n_pods))) ||
      (rc = st.in(a.init_cpu, n_init)) || (rc = st.in(a.init_mem, n_init)) ||
      (rc = st.in(a.restartable, n_init)) || (rc = st.in(a.ovh_cpu, a.n_pods)) ||
      (rc = st.in(a.ovh_mem, a.n_pods)))
    return rc;
  return pods_async_dev(ctx, a, pod_cpu, pod_mem, dv.stream);
}

}  // namespace

extern "C" {

int kcc_pod_requests_async(kcc_ctx* ctx, int64_t n_pods, int64_t n_containers, int64_t n_init,
                           const int64_t* d_pod_ptr, const uint64_t* d_cpu_req,
                           const int64_t* d_mem_req, const int64_t* d_init_ptr,
                           const uint64_t* d_init_cpu, const int64_t* d_init_mem,
                           const uint8_t* d_restartable, const uint64_t* d_ovh_cpu,
                           const int64_t* d_ovh_mem, uint64_t* d_pod_cpu, int64_t* d_pod_mem,
                           void* stream) {
  if (!ctx) return KCC_EINVAL;
  KCC_HIP(ctx, hipSetDevice(ctx->devs[0].device));
  return pods_async_dev(ctx,
                        {n_pods, n_containers, n_init, d_pod_ptr, d_cpu_req, d_mem_req, d_init_ptr,
                         d_init_cpu, d_init_mem, d_restartable, d_ovh_cpu, d_ovh_mem},
                        d_pod_cpu, d_pod_mem, static_cast<hipStream_t>(stream));
}

int kcc_pod_requests(kcc_ctx* ctx, int64_t n_pods, int64_t n_containers, int64_t n_init,
                     const int64_t* pod_ptr, const uint64_t* cpu_req, const int64_t* mem_req,
                     const int64_t* init_ptr, const uint64_t* init_cpu, const int64_t* init_mem,
                     const uint8_t* restartable, const uint64_t* ovh_cpu,
                     const int64_t* ovh_mem, uint64_t* pod_cpu, int64_t* pod_mem) {
  if (!ctx) return KCC_EINVAL;
  const PodArgs a{n_pods, n_containers, n_init, pod_ptr, cpu_req, mem_req, init_ptr,
                  init_cpu, init_mem, restartable, ovh_cpu, ovh_mem};
  int rc = check_pods(ctx, a, pod_cpu, pod_mem);
  if (rc || (rc = check_pods_csr(ctx, a))) return rc;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  Stage st(ctx, dv);
  if ((rc = st.out(pod_cpu, n_pods)) || (rc = st.out(pod_mem, n_pods)) ||
      (rc = pods_stage_run(ctx, dv, st, a, pod_cpu, pod_mem)))
    return rc;
  return st.finish();
}

int kcc_reduce_requests_pods(kcc_ctx* ctx, int64_t n_nodes, int64_t n_pods,
                             int64_t n_containers, int64_t n_init, const int64_t* node_pod_ptr,
                             const int64_t* pod_ptr, const uint64_t* cpu_req,
                             const int64_t* mem_req, const int64_t* init_ptr,
                             const uint64_t* init_cpu, const int64_t* init_mem,
                             const uint8_t* restartable, const uint64_t* ovh_cpu,
                             const int64_t* ovh_mem, uint64_t* used_cpu, int64_t* used_mem) {
  if (!ctx) return KCC_EINVAL;
  const PodArgs a{n_pods, n_containers, n_init, pod_ptr, cpu_req, mem_req, init_ptr,
                  init_cpu, init_mem, restartable, ovh_cpu, ovh_mem};
  // (the pod sums stay on the device: the node sums stand in for them in the pod checks)
  int rc = check_csr(ctx, n_nodes, n_pods, node_pod_ptr);
  if (rc || (rc = check_pods(ctx, a, used_cpu, used_mem)) || (rc = check_pods_csr(ctx, a)))
    return rc;
  if (n_nodes > 0 && (!used_cpu || !used_mem)) return fail(ctx, KCC_EINVAL, "NULL output");
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  Stage st(ctx, dv);
  // the pods of each node are the "containers" of the ordinary segmented reduce
  uint64_t* pod_cpu = nullptr;
  int64_t* pod_mem = nullptr;
  if ((rc = st.tmp(pod_cpu, n_pods)) || (rc = st.tmp(pod_mem, n_pods))) return rc;
  if ((rc = st.in(node_pod_ptr, csr_len(n_nodes))) || (rc = st.out(used_cpu, n_nodes)) ||
      (rc = st.out(used_mem, n_nodes)) || (rc = pods_stage_run(ctx, dv, st, a, pod_cpu, pod_mem)) ||
      (rc = reduce_async_dev(ctx, dv, n_nodes, n_pods, node_pod_ptr, pod_cpu, pod_mem, nullptr,
                             nullptr, used_cpu, used_mem, nullptr, nullptr, dv.stream)))
    return rc;
  return st.finish(true);
}

}  // extern "C"


// ---- preemption what-if: per-priority node state and a levelled fit (kcc_levels.hip) ------

namespace {

struct LevelsReduceArgs {
  int64_t n_nodes, n_pods, n_cont;
  const int64_t* node_pod_ptr;
  const int64_t* pod_ptr;
  const uint64_t* cpu_req;
  const int64_t* mem_req;
  const uint8_t* pod_level;
  int64_t L;
  uint64_t* used_cpu;
  int64_t* used_mem;
  int64_t* pod_count;
};

// Argument checks of both reduce forms (host or device pointers alike).
int check_levels_reduce(kcc_ctx* ctx, const LevelsReduceArgs& a) {
  if (a.n_nodes < 0 || a.n_pods < 0 || a.n_cont < 0) return fail(ctx, KCC_EINVAL, "negative size");
  if (a.L < 1 || a.L > KCC_LEVELS_MAX)
    return fail(ctx, KCC_EINVAL, "n_levels must be in [1, KCC_LEVELS_MAX]");
  if (a.n_nodes == 0)
    return a.n_pods == 0 && a.n_cont == 0 ? KCC_OK : fail(ctx, KCC_EINVAL, "pods without nodes");
  if (a.n_nodes > kcc::GRP_MAX_NODES) return fail(ctx, KCC_EINVAL, "too many nodes (max 2^31 - 4096)");
  if (!a.used_cpu || !a.used_mem || !a.pod_count) return fail(ctx, KCC_EINVAL, "NULL output");
  if (!a.node_pod_ptr) return fail(ctx, KCC_EINVAL, "node_pod_ptr is NULL");
  if (a.n_pods > 0 && (!a.pod_ptr || !a.pod_level)) return fail(ctx, KCC_EINVAL, "NULL pod_ptr/pod_level");
  if (a.n_pods == 0 && a.n_cont != 0) return fail(ctx, KCC_EINVAL, "containers without pods");
  if (a.n_cont > 0 && (!a.cpu_req || !a.mem_req)) return fail(ctx, KCC_EINVAL, "NULL cpu_req/mem_req");
  return KCC_OK;
}

int levels_reduce_dev(kcc_ctx* ctx, const LevelsReduceArgs& a, hipStream_t s) {
  KCC_HIP(ctx, kcc::launch_levels_reduce(a.n_nodes, a.n_pods, a.n_cont, (int)a.L, a.node_pod_ptr,
                                         a.pod_ptr, a.cpu_req, a.mem_req, a.pod_level, a.used_cpu,
                                         a.used_mem, a.pod_count, s));
  return KCC_OK;
}

// Plane l of the levelled node state: an ordinary FitNodes.
kcc::FitNodes level_plane(const kcc::FitNodes& nd, int64_t l) {
  kcc::FitNodes p = nd;
  if (nd.n > 0) {
    p.pod_count = nd.pod_count + l * nd.n;
    p.used_cpu = nd.used_cpu + l * nd.n;
    p.used_mem = nd.used_mem + l * nd.n;
    if (nd.R > 0) p.used_x = nd.used_x + l * nd.R * nd.n;
  }
  return p;
}

// Argument checks of both fit forms: kcc_fit_capped's, n_levels and the host array level_ptr.
int check_fit_levels(kcc_ctx* ctx, const kcc::FitNodes& nd, const kcc::FitSpecs& sp, int64_t L,
                     const int64_t* level_ptr, const int64_t* totals, const int32_t* spec_err) {
  if (L < 1 || L > KCC_LEVELS_MAX)
    return fail(ctx, KCC_EINVAL, "n_levels must be in [1, KCC_LEVELS_MAX]");
  const int rc = check_cells(ctx, nd, sp, false, totals, spec_err);
  if (rc) return rc;
  if (!level_ptr) return fail(ctx, KCC_EINVAL, "level_ptr is NULL");
  if (level_ptr[0] != 0) return fail(ctx, KCC_EINVAL, "level_ptr[0] != 0");
  for (int64_t l = 0; l < L; ++l)
    if (level_ptr[l + 1] < level_ptr[l]) return fail(ctx, KCC_EINVAL, "level_ptr is not non-decreasing");
  if (level_ptr[L] != sp.S) return fail(ctx, KCC_EINVAL, "level_ptr[n_levels] != n_specs");
  return KCC_OK;
}

// Device level (the caller has passed check_fit_levels): one kcc_fit_capped per non-empty
// level on that level's plane, its cells placed into the level's columns.  The launches
// depend on (N, G, R, L, level_ptr) alone.
int fit_levels_dev(kcc_ctx* ctx, Dev& dv, const kcc::FitNodes& nd, const kcc::FitSpecs& sp,
                   int64_t L, const int64_t* level_ptr, int64_t* totals, int32_t* spec_err,
                   hipStream_t s) {
  if (nd.n == 0 || sp.S == 0)  // kcc_fit_capped's degenerate cases
    return fit_cells_dev(ctx, dv, nd, sp, false, totals, spec_err, nullptr, nullptr, s);
  int64_t s_max = 0;
  for (int64_t l = 0; l < L; ++l) {
    const int64_t sl = level_ptr[l + 1] - level_ptr[l];
    s_max = sl > s_max ? sl : s_max;
    if (sl == sp.S)  // one level holds every spec: kcc_fit_capped on its plane, no copy
      return fit_cells_dev(ctx, dv, level_plane(nd, l), sp, false, totals, spec_err, nullptr,
                           nullptr, s);
  }
  KCC_HIP(ctx, ensure(dv.lv_tot, 8 * (size_t)(nd.G * s_max)));
  KCC_HIP(ctx, ensure(dv.lv_err, 4 * (size_t)(nd.G * s_max)));
  if (nd.R > 0) {  // the pair loop strides spec_x by its S: a level's block is [R, S_l]
    kcc::LevelPtr lp;
    lp.L = (int)L;
    for (int64_t l = 0; l <= KCC_LEVELS_MAX; ++l) lp.ptr[l] = level_ptr[l < L ? l : L];
    KCC_HIP(ctx, ensure(dv.lv_x, 8 * (size_t)(nd.R * sp.S)));
    KCC_HIP(ctx, kcc::launch_cells_pack_x(nd.R, sp.S, lp, sp.spec_x, as<int64_t>(dv.lv_x), s));
  }
  for (int64_t l = 0; l < L; ++l) {
    const int64_t o = level_ptr[l], sl = level_ptr[l + 1] - o;
    if (sl == 0) continue;
    const kcc::FitSpecs spl{sl, sp.spec_cpu + o, sp.spec_mem + o,
                            nd.R > 0 ? as<int64_t>(dv.lv_x) + nd.R * o : nullptr,
                            sp.node_cap ? sp.node_cap + o : nullptr};
    const int rc = fit_cells_dev(ctx, dv, level_plane(nd, l), spl, false, as<int64_t>(dv.lv_tot),
                                 as<int32_t>(dv.lv_err), nullptr, nullptr, s);
    if (rc) return rc;
    KCC_HIP(ctx, kcc::launch_cells_place(nd.G, sp.S, sl, o, as<int64_t>(dv.lv_tot),
                                         as<int32_t>(dv.lv_err), totals, spec_err, s));
  }
  return KCC_OK;
}

}  // namespace

extern "C" {

int kcc_reduce_requests_levels_async(kcc_ctx* ctx, int64_t n_nodes, int64_t n_pods,
                                     int64_t n_containers, const int64_t* d_node_pod_ptr,
                                     const int64_t* d_pod_ptr, const uint64_t* d_cpu_req,
                                     const int64_t* d_mem_req, const uint8_t* d_pod_level,
                                     int64_t n_levels, uint64_t* d_used_cpu, int64_t* d_used_mem,
                                     int64_t* d_pod_count, void* stream) {
  if (!ctx) return KCC_EINVAL;
  const LevelsReduceArgs a{n_nodes, n_pods, n_containers, d_node_pod_ptr, d_pod_ptr, d_cpu_req,
                           d_mem_req, d_pod_level, n_levels, d_used_cpu, d_used_mem, d_pod_count};
  const int rc = check_levels_reduce(ctx, a);
  if (rc || n_nodes == 0) return rc;
  KCC_HIP(ctx, hipSetDevice(ctx->devs[0].device));
  return levels_reduce_dev(ctx, a, static_cast<hipStream_t>(stream));
}

int kcc_reduce_requests_levels(kcc_ctx* ctx, int64_t n_nodes, int64_t n_pods, int64_t n_containers,
                               const int64_t* node_pod_ptr, const int64_t* pod_ptr,
                               const uint64_t* cpu_req, const int64_t* mem_req,
                               const uint8_t* pod_level, int64_t n_levels, uint64_t* used_cpu,
                               int64_t* used_mem, int64_t* pod_count) {
  if (!ctx) return KCC_EINVAL;
  LevelsReduceArgs a{n_nodes, n_pods, n_containers, node_pod_ptr, pod_ptr, cpu_req,
                     mem_req, pod_level, n_levels, used_cpu, used_mem, pod_count};
  int rc = check_levels_reduce(ctx, a);
  if (rc || n_nodes == 0) return rc;
  // the host form reads the offsets: both CSR arrays are well formed
  if ((rc = check_csr(ctx, n_nodes, n_pods, node_pod_ptr)) ||
      (rc = check_csr(ctx, n_pods, n_containers, pod_ptr)))
    return rc;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  Stage st(ctx, dv);
  const int64_t planes = n_levels * n_nodes;
  if ((rc = st.in(a.node_pod_ptr, csr_len(n_nodes))) || (rc = st.in(a.pod_ptr, csr_len(n_pods))) ||
      (rc = st.in(a.cpu_req, n_containers)) || (rc = st.in(a.mem_req, n_containers)) ||
      (rc = st.in(a.pod_level, n_pods)) || (rc = st.out(a.used_cpu, planes)) ||
      (rc = st.out(a.used_mem, planes)) || (rc = st.out(a.pod_count, planes)) ||
      (rc = levels_reduce_dev(ctx, a, dv.stream)))
    return rc;
  return st.finish();
}

int kcc_fit_levels_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                         const int64_t* d_alloc_mem, const int64_t* d_alloc_pods, int64_t n_levels,
                         const int64_t* d_pod_count, const uint64_t* d_used_cpu,
                         const int64_t* d_used_mem, int64_t n_ext, const int64_t* d_alloc_x,
                         const int64_t* d_used_x, const int32_t* d_group, int64_t n_groups,
                         int64_t n_specs, const uint64_t* d_spec_cpu, const int64_t* d_spec_mem,
                         const int64_t* d_spec_x, const int64_t* d_node_cap,
                         const int64_t* h_level_ptr, int64_t* d_totals, int32_t* d_spec_err,
                         void* stream) {
  if (!ctx) return KCC_EINVAL;
  const kcc::FitNodes nd{n_nodes, d_alloc_cpu, d_alloc_mem, d_alloc_pods, d_pod_count, d_used_cpu,
                         d_used_mem, n_ext, d_alloc_x, d_used_x, d_group, n_groups};
  const kcc::FitSpecs sp{n_specs, d_spec_cpu, d_spec_mem, d_spec_x, d_node_cap};
  const int rc = check_fit_levels(ctx, nd, sp, n_levels, h_level_ptr, d_totals, d_spec_err);
  if (rc) return rc;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  return fit_levels_dev(ctx, dv, nd, sp, n_levels, h_level_ptr, d_totals, d_spec_err,
                        static_cast<hipStream_t>(stream));
}

int kcc_fit_levels(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu,
                   const int64_t* alloc_mem, const int64_t* alloc_pods, int64_t n_levels,
                   const int64_t* pod_count, const uint64_t* used_cpu, const int64_t* used_mem,
                   int64_t n_ext, const int64_t* alloc_x, const int64_t* used_x,
                   const int32_t* group, int64_t n_groups, int64_t n_specs,
                   const uint64_t* spec_cpu, const int64_t* spec_mem, const int64_t* spec_x,
                   const int64_t* node_cap, const int64_t* level_ptr, int64_t* totals,
                   int32_t* spec_err) {
  if (!ctx) return KCC_EINVAL;
  kcc::FitNodes nd{n_nodes, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
                   n_ext, alloc_x, used_x, group, n_groups};
  kcc::FitSpecs sp{n_specs, spec_cpu, spec_mem, spec_x, node_cap};
  int rc = check_fit_levels(ctx, nd, sp, n_levels, level_ptr, totals, spec_err);
  if (rc) return rc;
  const int64_t n = n_nodes, S = n_specs, cells = n_groups * n_specs, ln = n_levels * n_nodes;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  Stage st(ctx, dv);
  if ((rc = st.in(nd.alloc_cpu, n)) || (rc = st.in(nd.alloc_mem, n)) ||
      (rc = st.in(nd.alloc_pods, n)) || (rc = st.in(nd.pod_count, ln)) ||
      (rc = st.in(nd.used_cpu, ln)) || (rc = st.in(nd.used_mem, ln)) ||
      (rc = st.in(nd.alloc_x, nd.R * n)) || (rc = st.in(nd.used_x, nd.R * ln)) ||
      (rc = st.in(nd.group, n)) || (rc = st.in(sp.spec_cpu, S)) || (rc = st.in(sp.spec_mem, S)) ||
      (rc = st.in(sp.spec_x, nd.R * S)) || (rc = st.in(sp.node_cap, S)) ||
      (rc = st.out(totals, cells)) || (rc = st.out(spec_err, cells)) ||
      (rc = fit_levels_dev(ctx, dv, nd, sp, n_levels, level_ptr, totals, spec_err, dv.stream)))
    return rc;
  return st.finish();
}

}  // extern "C"


// ---- drain what-if: the pods of drained rows re-placed (kcc_drain.hip) --------------------

namespace {

struct DrainArgs {
  kcc::FitNodes nd;  // pod_count / used_* left nullptr: the state is the four pointers below
  int64_t* pod_count;
  uint64_t* used_cpu;
  int64_t* used_mem;
  int64_t* used_x;
  const uint8_t* drain;
  kcc::DrainPods pods;
  int policy;
  int64_t max_shapes;
  kcc::DrainOut out;
};

// Argument checks of both entry points (host or device pointers alike).
int check_drain(kcc_ctx* ctx, const DrainArgs& a) {
  const kcc::FitNodes& nd = a.nd;
  const int64_t P = a.pods.P;
  if (nd.n < 0 || P < 0) return fail(ctx, KCC_EINVAL, "negative size");
  if (a.policy != KCC_DEPLOY_PACK && a.policy != KCC_DEPLOY_SPREAD)
    return fail(ctx, KCC_EINVAL, "policy must be KCC_DEPLOY_PACK or KCC_DEPLOY_SPREAD");
  if (nd.R < 0 || nd.R > KCC_EXT_MAX) return fail(ctx, KCC_EINVAL, "n_ext must be in [0, KCC_EXT_MAX]");
  if (a.max_shapes < 1 || a.max_shapes > KCC_DRAIN_MAX_SHAPES)
    return fail(ctx, KCC_EINVAL, "max_shapes must be in [1, KCC_DRAIN_MAX_SHAPES]");
  if (nd.n > kcc::GRP_MAX_NODES) return fail(ctx, KCC_EINVAL, "too many nodes (max 2^31 - 4096)");
  if (P > kcc::DRAIN_MAX_PODS) return fail(ctx, KCC_EINVAL, "too many pods (max 2^31 - 4096)");
  if (nd.n == 0 && P != 0) return fail(ctx, KCC_EINVAL, "pods without nodes");
  const kcc::DrainOut& o = a.out;
  if (!o.summary || !o.shape_cpu || !o.shape_mem || !o.shape_count || !o.shape_placed ||
      !o.shape_nodes || !o.shape_err || (nd.R > 0 && !o.shape_x))
    return fail(ctx, KCC_EINVAL, "NULL output");
  if (nd.n > 0 && (!nd.alloc_cpu || !nd.alloc_mem || !nd.alloc_pods || !a.pod_count ||
                   !a.used_cpu || !a.used_mem || !a.drain || !a.pods.node_pod_ptr))
    return fail(ctx, KCC_EINVAL, "NULL node array");
  if (nd.R > 0 && nd.n > 0 && (!nd.alloc_x || !a.used_x))
    return fail(ctx, KCC_EINVAL, "NULL extra-resource array with n_ext > 0");
  if (P > 0 && (!a.pods.pod_cpu || !a.pods.pod_mem)) return fail(ctx, KCC_EINVAL, "NULL pod array");
  return KCC_OK;
}

// Device level: the checks, the degenerate case, the workspaces (they only grow) and the
// launches on s.  host_form: D is read back after the pod pass (one synchronisation of s) and
// the plan has D steps; else max_shapes steps, the ones behind D padding.
int drain_dev(kcc_ctx* ctx, Dev& dv, const DrainArgs& a, hipStream_t s, bool host_form) {
  const int rc = check_drain(ctx, a);
  if (rc) return rc;
  const size_t M = (size_t)a.max_shapes, R = (size_t)a.nd.R;
  const kcc::DrainOut& o = a.out;
  if (a.nd.n == 0) {  // no rows: nothing drained, nothing evicted
    KCC_HIP(ctx, hipMemsetAsync(o.summary, 0, 8 * KCC_DRAIN_SUMMARY, s));
    KCC_HIP(ctx, hipMemsetAsync(o.shape_cpu, 0, 8 * M, s));
    KCC_HIP(ctx, hipMemsetAsync(o.shape_mem, 0, 8 * M, s));
    if (R) KCC_HIP(ctx, hipMemsetAsync(o.shape_x, 0, 8 * R * M, s));
    KCC_HIP(ctx, hipMemsetAsync(o.shape_count, 0, 8 * M, s));
    KCC_HIP(ctx, hipMemsetAsync(o.shape_placed, 0, 8 * M, s));
    KCC_HIP(ctx, hipMemsetAsync(o.shape_nodes, 0, 8 * M, s));
    KCC_HIP(ctx, hipMemsetAsync(o.shape_err, 0, 4 * M, s));
    return KCC_OK;
  }
  const size_t T = (size_t)kcc::drain_table(a.max_shapes);
  KCC_HIP(ctx, ensure(dv.dr_tab, 8 * kcc::DRAIN_META_WORDS + 8 * T));
  // plan_cpu, plan_mem, plan_rep, placed, nodes_used [M], plan_x [R M] (int64), step_err [M]
  KCC_HIP(ctx, ensure(dv.dr_plan, 8 * M * (5 + R) + 4 * M));
  kcc::DrainWork w;
  w.meta = as<unsigned long long>(dv.dr_tab);
  w.cnt = reinterpret_cast<uint32_t*>(w.meta + kcc::DRAIN_META_WORDS);
  w.rep = reinterpret_cast<int32_t*>(w.cnt + T);
  w.plan_cpu = as<uint64_t>(dv.dr_plan);
  w.plan_mem = reinterpret_cast<int64_t*>(w.plan_cpu + M);
  w.plan_rep = w.plan_mem + M;
  w.placed = w.plan_rep + M;
  w.nodes_used = w.placed + M;
  w.plan_x = w.nodes_used + M;
  w.step_err = reinterpret_cast<int32_t*>(w.plan_x + R * M);
  KCC_HIP(ctx, kcc::launch_drain_scan(a.nd, a.pod_count, a.used_cpu, a.used_mem, a.used_x, a.drain,
                                      a.pods, a.max_shapes, w, s));
  int64_t K = a.max_shapes;
  if (host_form) {
    unsigned long long meta[kcc::DRAIN_META_WORDS];
    KCC_HIP(ctx, hipMemcpyAsync(meta, w.meta, sizeof(meta), hipMemcpyDeviceToHost, s));
    KCC_HIP(ctx, hipStreamSynchronize(s));
    const bool over = meta[kcc::DRAIN_META_OVERFLOW] != 0 ||
                      meta[kcc::DRAIN_META_CLAIMED] > (unsigned long long)a.max_shapes;
    K = over ? 0 : (int64_t)meta[kcc::DRAIN_META_CLAIMED];
  }
  KCC_HIP(ctx, kcc::launch_drain_plan(a.nd.R, a.pods, a.max_shapes, K, w, o, s));
  if (K > 0) {
    const DeployArgs d{{a.nd.n, a.nd.alloc_cpu, a.nd.alloc_mem, a.nd.alloc_pods, nullptr, nullptr,
                        nullptr, a.nd.R, a.nd.alloc_x, nullptr, nullptr, 1},
                       a.pod_count, a.used_cpu, a.used_mem, a.used_x, nullptr,
                       {K, w.plan_cpu, w.plan_mem, w.plan_x, w.plan_rep, nullptr, a.policy},
                       w.placed, w.nodes_used, w.step_err, nullptr};
    const int drc = deploy_dev(ctx, dv, d, s);
    if (drc) return drc;
  }
  KCC_HIP(ctx, kcc::launch_drain_finish(a.max_shapes, w, o, s));
  return KCC_OK;
}

}  // namespace

extern "C" {

int kcc_drain_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                    const int64_t* d_alloc_mem, const int64_t* d_alloc_pods, int64_t n_ext,
                    const int64_t* d_alloc_x, int64_t* d_pod_count, uint64_t* d_used_cpu,
                    int64_t* d_used_mem, int64_t* d_used_x, const uint8_t* d_drain,
                    int64_t n_pods, const int64_t* d_node_pod_ptr, const uint64_t* d_pod_cpu,
                    const int64_t* d_pod_mem, const int64_t* d_pod_x,
                    const uint8_t* d_pod_movable, int policy, int64_t max_shapes,
                    int64_t* d_summary, uint64_t* d_shape_cpu, int64_t* d_shape_mem,
                    int64_t* d_shape_x, int64_t* d_shape_count, int64_t* d_shape_placed,
                    int64_t* d_shape_nodes, int32_t* d_shape_err, void* stream) {
  if (!ctx) return KCC_EINVAL;
  const DrainArgs a{{n_nodes, d_alloc_cpu, d_alloc_mem, d_alloc_pods, nullptr, nullptr, nullptr,
                     n_ext, d_alloc_x, nullptr, nullptr, 1},
                    d_pod_count, d_used_cpu, d_used_mem, d_used_x, d_drain,
                    {n_pods, d_node_pod_ptr, d_pod_cpu, d_pod_mem, d_pod_x, d_pod_movable},
                    policy, max_shapes,
                    {d_summary, d_shape_cpu, d_shape_mem, d_shape_x, d_shape_count, d_shape_placed,
                     d_shape_nodes, d_shape_err}};
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  return drain_dev(ctx, dv, a, static_cast<hipStream_t>(stream), false);
}

int kcc_drain(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu, const int64_t* alloc_mem,
              const int64_t* alloc_pods, int64_t n_ext, const int64_t* alloc_x,
              int64_t* pod_count, uint64_t* used_cpu, int64_t* used_mem, int64_t* used_x,
              const uint8_t* drain, int64_t n_pods, const int64_t* node_pod_ptr,
              const uint64_t* pod_cpu, const int64_t* pod_mem, const int64_t* pod_x,
              const uint8_t* pod_movable, int policy, int64_t max_shapes, int64_t* summary,
              uint64_t* shape_cpu, int64_t* shape_mem, int64_t* shape_x, int64_t* shape_count,
              int64_t* shape_placed, int64_t* shape_nodes, int32_t* shape_err) {
  if (!ctx) return KCC_EINVAL;
  DrainArgs a{{n_nodes, alloc_cpu, alloc_mem, alloc_pods, nullptr, nullptr, nullptr, n_ext,
               alloc_x, nullptr, nullptr, 1},
              pod_count, used_cpu, used_mem, used_x, drain,
              {n_pods, node_pod_ptr, pod_cpu, pod_mem, pod_x, pod_movable},
              policy, max_shapes,
              {summary, shape_cpu, shape_mem, shape_x, shape_count, shape_placed, shape_nodes,
               shape_err}};
  int rc = check_drain(ctx, a);
  if (rc) return rc;
  // the host form reads the offsets: the CSR is well formed
  if ((rc = check_csr(ctx, n_nodes, n_pods, node_pod_ptr))) return rc;
  const int64_t n = n_nodes, P = n_pods, R = n_ext, M = max_shapes;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  Stage st(ctx, dv);
  kcc::DrainOut& o = a.out;
  if ((rc = st.in(a.nd.alloc_cpu, n)) || (rc = st.in(a.nd.alloc_mem, n)) ||
      (rc = st.in(a.nd.alloc_pods, n)) || (rc = st.in(a.nd.alloc_x, R * n)) ||
      (rc = st.in(a.drain, n)) || (rc = st.in(a.pods.node_pod_ptr, csr_len(n))) ||
      (rc = st.in(a.pods.pod_cpu, P)) || (rc = st.in(a.pods.pod_mem, P)) ||
      (rc = st.in(a.pods.pod_x, R * P)) || (rc = st.in(a.pods.movable, P)) ||
      (rc = st.inout(a.pod_count, n)) || (rc = st.inout(a.used_cpu, n)) ||
      (rc = st.inout(a.used_mem, n)) || (rc = st.inout(a.used_x, R * n)) ||
      (rc = st.out(o.summary, KCC_DRAIN_SUMMARY)) || (rc = st.out(o.shape_cpu, M)) ||
      (rc = st.out(o.shape_mem, M)) || (rc = st.out(o.shape_x, R * M)) ||
      (rc = st.out(o.shape_count, M)) || (rc = st.out(o.shape_placed, M)) ||
      (rc = st.out(o.shape_nodes, M)) || (rc = st.out(o.shape_err, M)) ||
      (rc = drain_dev(ctx, dv, a, dv.stream, true)))
    return rc;
  return st.finish();
}

}  // extern "C"


// ---- removal what-if: each candidate row's pods re-placed on the rest (kcc_consolidate.hip) ----

namespace {

struct ConsArgs {
  kcc::FitNodes nd;  // the state is read only: nd's own pod_count / used_* pointers
  const uint8_t* target;
  kcc::DrainPods pods;
  int64_t C;
  const int64_t* cand;
  kcc::ConsOut out;
};

// Argument checks of both entry points (host or device pointers alike).
int check_consolidate(kcc_ctx* ctx, const ConsArgs& a) {
  const kcc::FitNodes& nd = a.nd;
  const int64_t P = a.pods.P;
  if (nd.n < 0 || P < 0 || a.C < 0) return fail(ctx, KCC_EINVAL, "negative size");
  if (nd.R < 0 || nd.R > KCC_EXT_MAX) return fail(ctx, KCC_EINVAL, "n_ext must be in [0, KCC_EXT_MAX]");
  if (nd.n > kcc::GRP_MAX_NODES) return fail(ctx, KCC_EINVAL, "too many nodes (max 2^31 - 4096)");
  if (P > kcc::DRAIN_MAX_PODS) return fail(ctx, KCC_EINVAL, "too many pods (max 2^31 - 4096)");
  if (a.C > kcc::CONS_MAX_CAND) return fail(ctx, KCC_EINVAL, "too many candidates (max 2^31 - 4096)");
  if (nd.n == 0 && P != 0) return fail(ctx, KCC_EINVAL, "pods without nodes");
  const kcc::ConsOut& o = a.out;
  if (a.C > 0 && (!a.cand || !o.evicted || !o.placed || !o.zero || !o.err))
    return fail(ctx, KCC_EINVAL, "NULL candidate array");
  if (nd.n > 0 && (!nd.alloc_cpu || !nd.alloc_mem || !nd.alloc_pods || !nd.pod_count ||
                   !nd.used_cpu || !nd.used_mem || !a.pods.node_pod_ptr))
    return fail(ctx, KCC_EINVAL, "NULL node array");
  if (nd.R > 0 && nd.n > 0 && (!nd.alloc_x || !nd.used_x))
    return fail(ctx, KCC_EINVAL, "NULL extra-resource array with n_ext > 0");
  if (P > 0 && (!a.pods.pod_cpu || !a.pods.pod_mem)) return fail(ctx, KCC_EINVAL, "NULL pod array");
  return KCC_OK;
}

// Device level: the checks, the degenerate cases and the launches on s.  No workspace.
int consolidate_dev(kcc_ctx* ctx, const ConsArgs& a, hipStream_t s) {
  const int rc = check_consolidate(ctx, a);
  if (rc) return rc;
  const kcc::ConsOut& o = a.out;
  if (a.nd.n == 0 || a.C == 0) {  // nobody is evaluated: zeros, and every pod a non-candidate's
    const size_t C = (size_t)a.C;
    if (C) {
      KCC_HIP(ctx, hipMemsetAsync(o.evicted, 0, 8 * C, s));
      KCC_HIP(ctx, hipMemsetAsync(o.placed, 0, 8 * C, s));
      KCC_HIP(ctx, hipMemsetAsync(o.zero, 0, 8 * C, s));
      KCC_HIP(ctx, hipMemsetAsync(o.err, 0, 4 * C, s));
    }
    if (o.pod_target && a.pods.P > 0)
      KCC_HIP(ctx, kcc::launch_fill_i64(a.pods.P, -2, o.pod_target, s));
    return KCC_OK;
  }
  KCC_HIP(ctx, kcc::launch_consolidate(a.nd, a.target, a.pods, a.C, a.cand, o, s));
  return KCC_OK;
}

}  // namespace

extern "C" {

int kcc_consolidate_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                          const int64_t* d_alloc_mem, const int64_t* d_alloc_pods, int64_t n_ext,
                          const int64_t* d_alloc_x, const int64_t* d_pod_count,
                          const uint64_t* d_used_cpu, const int64_t* d_used_mem,
                          const int64_t* d_used_x, const uint8_t* d_target, int64_t n_pods,
                          const int64_t* d_node_pod_ptr, const uint64_t* d_pod_cpu,
                          const int64_t* d_pod_mem, const int64_t* d_pod_x,
                          const uint8_t* d_pod_movable, int64_t n_cand, const int64_t* d_cand,
                          int64_t* d_cand_evicted, int64_t* d_cand_placed, int64_t* d_cand_zero,
                          int32_t* d_cand_err, int64_t* d_pod_target, void* stream) {
  if (!ctx) return KCC_EINVAL;
  const ConsArgs a{{n_nodes, d_alloc_cpu, d_alloc_mem, d_alloc_pods, d_pod_count, d_used_cpu,
                    d_used_mem, n_ext, d_alloc_x, d_used_x, nullptr, 1},
                   d_target,
                   {n_pods, d_node_pod_ptr, d_pod_cpu, d_pod_mem, d_pod_x, d_pod_movable},
                   n_cand, d_cand,
                   {d_cand_evicted, d_cand_placed, d_cand_zero, d_cand_err, d_pod_target}};
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  return consolidate_dev(ctx, a, static_cast<hipStream_t>(stream));
}

int kcc_consolidate(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu,
                    const int64_t* alloc_mem, const int64_t* alloc_pods, int64_t n_ext,
                    const int64_t* alloc_x, const int64_t* pod_count, const uint64_t* used_cpu,
                    const int64_t* used_mem, const int64_t* used_x, const uint8_t* target,
                    int64_t n_pods, const int64_t* node_pod_ptr, const uint64_t* pod_cpu,
                    const int64_t* pod_mem, const int64_t* pod_x, const uint8_t* pod_movable,
                    int64_t n_cand, const int64_t* cand, int64_t* cand_evicted,
                    int64_t* cand_placed, int64_t* cand_zero, int32_t* cand_err,
                    int64_t* pod_target) {
  if (!ctx) return KCC_EINVAL;
  ConsArgs a{{n_nodes, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem, n_ext,
              alloc_x, used_x, nullptr, 1},
             target,
             {n_pods, node_pod_ptr, pod_cpu, pod_mem, pod_x, pod_movable},
             n_cand, cand,
             {cand_evicted, cand_placed, cand_zero, cand_err, pod_target}};
  int rc = check_consolidate(ctx, a);
  if (rc) return rc;
  // the host form reads the offsets: the CSR is well formed
  if ((rc = check_csr(ctx, n_nodes, n_pods, node_pod_ptr))) return rc;
  const int64_t n = n_nodes, P = n_pods, R = n_ext, C = n_cand;
  Dev& dv = ctx->devs[0];
  KCC_HIP(ctx, hipSetDevice(dv.device));
  Stage st(ctx, dv);
  kcc::FitNodes& nd = a.nd;
  kcc::ConsOut& o = a.out;
  if ((rc = st.in(nd.alloc_cpu, n)) || (rc = st.in(nd.alloc_mem, n)) ||
      (rc = st.in(nd.alloc_pods, n)) || (rc = st.in(nd.alloc_x, R * n)) ||
      (rc = st.in(nd.pod_count, n)) || (rc = st.in(nd.used_cpu, n)) ||
      (rc = st.in(nd.used_mem, n)) || (rc = st.in(nd.used_x, R * n)) ||
      (rc = st.in(a.target, n)) || (rc = st.in(a.pods.node_pod_ptr, csr_len(n))) ||
      (rc = st.in(a.pods.pod_cpu, P)) || (rc = st.in(a.pods.pod_mem, P)) ||
      (rc = st.in(a.pods.pod_x, R * P)) || (rc = st.in(a.pods.movable, P)) ||
      (rc = st.in(a.cand, C)) || (rc = st.out(o.evicted, C)) || (rc = st.out(o.placed, C)) ||
      (rc = st.out(o.zero, C)) || (rc = st.out(o.err, C)) || (rc = st.out(o.pod_target, P)) ||
      (rc = consolidate_dev(ctx, a, dv.stream)))
    return rc;
  return st.finish();
}

}  // extern "C"
