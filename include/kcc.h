/*
 * kcc.h — C-ABI of the MI355X capacity engine (libkcc.so).
 *
 * This is the drop-in boundary for the hot path of
 * AshutoshNirkhe/KubernetesClusterCapacity, src/KubeAPI/ClusterCapacity.go (CC):
 *
 *   (a) the per-container request summation inside getPodCPUMemoryRequestsLimits
 *       (CC:255-299, the adds at CC:290-293)           -> kcc_reduce_requests*
 *   (b) the per-node fit + pod-slot clamp + total in main's node loop
 *       (CC:101-140, findMin CC:159-164)               -> kcc_fit*
 *
 * generalised from the reference's single pod spec to a batch of S what-if specs.
 * The Go host keeps flags, client-go listing and printing; a cgo package binds
 * these symbols.  Every result is bit-exact to the Go integer
 * arithmetic (uint64/int64 wrap, Go `int` = int64 on amd64, signed min, clamp quirk).
 *
 * Conventions
 *   - Return 0 (KCC_OK) on success, a negative KCC_E* code otherwise; the message
 *     is available from kcc_last_error(ctx) until the next call on ctx.
 *   - Host-array entry points (no suffix) are synchronous: they copy inputs to the
 *     device, run, copy results back and never retain a caller pointer.
 *   - *_async entry points take DEVICE pointers and a hipStream_t (as void*, NULL =
 *     the null stream) and only enqueue work: they never synchronise, and allocate
 *     only when the context workspace must grow — call kcc_reserve first and they
 *     can be captured into a hipGraph and replayed (no launch depends on host-side
 *     state that a replay would freeze: the reduce's look-back records are left free by
 *     every launch, the exchange's epoch is a device word).  Container arrays must be
 *     16-byte aligned.
 *   - Device faults: the reduce's look-back and node-prep waits, the keyed gather's
 *     part wait and the exchange's flag waits are bounded; one that gives up (never on
 *     a healthy device) sets a sticky fault word of the device.  While it is set every
 *     finalize marks every spec KCC_SPEC_FAULT (totals 0) and the synchronous entry
 *     points (the keyed ones included) return KCC_EFAULT; kcc_clear_faults resets it
 *     and every device counter a give-up can leave set.  The fault also travels with the data: a partial produced on a
 *     faulted device (kcc_*_partial_async, kcc_fit_run_async) carries a fault mark in
 *     its per-spec counts, so every rank that sums it — over the p2p exchange, an RCCL
 *     or any other all-reduce, the in-library device fold — marks every spec
 *     KCC_SPEC_FAULT too, without reading the faulted device's words.
 *     kcc_reduce_requests_async alone has no per-spec output: check kcc_reduce_faults
 *     after synchronising.
 *   - A context is not thread-safe; every entry calls hipSetDevice(ctx device), so
 *     Go OS-thread migration between cgo calls is harmless.
 *   - There is no CPU backend: without a usable gfx950 device kcc_create fails.
 */
#ifndef KCC_H
#define KCC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5): kcc_fit_mskip_groups removed; partial[S..2S) carries the device fault mark
 * (a count >= 2^48, see kcc_fit_partial_async).  1: the first release. */
#define KCC_ABI_VERSION 2

enum {
  KCC_OK = 0,
  KCC_EINVAL = -1,   /* bad argument (null pointer, negative size, malformed CSR) */
  KCC_ENOMEM = -2,   /* device allocation failed                                  */
  KCC_EHIP = -3,     /* HIP runtime error                                         */
  KCC_ENODEV = -4,   /* no usable device                                          */
  KCC_ERCCL = -5,    /* RCCL error (multi-GPU contexts)                           */
  KCC_EFAULT = -6    /* a bounded device wait gave up: results invalid (see above) */
};

/* spec_err values of the fit entry points */
enum {
  KCC_SPEC_OK = 0,
  KCC_SPEC_DIVZERO = 1, /* Go would panic with an integer divide by zero; total 0    */
  KCC_SPEC_FAULT = 2    /* the device faulted (kcc_clear_faults); total 0, not valid */
};

typedef struct kcc_ctx kcc_ctx;

/* Library / ABI version (KCC_ABI_VERSION). */
int kcc_abi_version(void);
/* Build flavour: "release" for the product library; an experiment build (csrc/Makefile
 * `variant`, its own .so) returns "variant" plus the knobs it was compiled with. */
const char* kcc_build_info(void);

/* Create a context on `n_gpus` devices starting at `first_device`.
 * n_gpus == 1: one device.  n_gpus > 1: nodes are sharded in contiguous ranges
 * over devices first_device .. first_device+n_gpus-1 and the per-spec totals are
 * combined with an RCCL int64 all-reduce (replaces nothing in the reference: the
 * reference is single-threaded, CC:105).  n_gpus <= 0 is KCC_EINVAL. */
int kcc_create(kcc_ctx** out, int first_device, int n_gpus);
void kcc_destroy(kcc_ctx* ctx);
const char* kcc_last_error(const kcc_ctx* ctx);
/* Thread-local message of the last failed kcc_create (ctx did not exist yet). */
const char* kcc_create_error(void);

/* In-library all-reduce check (contexts of n_gpus > 1, host-array entry points): the
 * context's FIRST all-reduce is verified against the host's sum of the devices' partials
 * (KCC_ERCCL on a mismatch); later calls are not, unless every_call != 0 (then every call
 * pays two device-to-host copies and stream syncs per device).  Default 0. */
int kcc_set_allreduce_verify(kcc_ctx* ctx, int every_call);

/* Pre-size the device workspace used by the *_async entry points (device 0 of ctx). */
int kcc_reserve(kcc_ctx* ctx, int64_t max_nodes, int64_t max_containers, int64_t max_specs);

/* ---------------------------------------------------------------------------
 * (a) Segmented request reduction.  Replaces the accumulation at CC:290-293:
 *       cpuRequestsMiliTotal     += cpuRequestsMili     (uint64, wraps)
 *       cpuLimitsMiliTotal       += cpuLimitsMili       (uint64, wraps)
 *       memoryRequestsBytesTotal += memoryRequestsBytes (int64,  wraps)
 *       memoryLimitsBytesTotal   += memoryLimitsBytes   (int64,  wraps)
 *     over every container of every non-terminated pod of a node.
 *   Containers are grouped by node in CSR form: node i owns containers
 *   [node_ptr[i], node_ptr[i+1]); node_ptr[0] == 0, non-decreasing,
 *   node_ptr[n_nodes] == n_containers.  Empty nodes get 0 sums.
 *   At most 2^28 - 1 nodes per device (per call, or per shard for a multi-GPU ctx).
 *   cpu_lim/mem_lim may both be NULL (then lim_cpu/lim_mem are ignored): the limit
 *   sums are only printed by the reference (CC:110, CC:115-117).
 * ------------------------------------------------------------------------- */
int kcc_reduce_requests(kcc_ctx* ctx, int64_t n_nodes, int64_t n_containers,
                        const int64_t* node_ptr, const uint64_t* cpu_req,
                        const int64_t* mem_req, const uint64_t* cpu_lim,
                        const int64_t* mem_lim, uint64_t* used_cpu, int64_t* used_mem,
                        uint64_t* lim_cpu, int64_t* lim_mem);

int kcc_reduce_requests_async(kcc_ctx* ctx, int64_t n_nodes, int64_t n_containers,
                              const int64_t* d_node_ptr, const uint64_t* d_cpu_req,
                              const int64_t* d_mem_req, const uint64_t* d_cpu_lim,
                              const int64_t* d_mem_lim, uint64_t* d_used_cpu,
                              int64_t* d_used_mem, uint64_t* d_lim_cpu,
                              int64_t* d_lim_mem, void* stream);

/* ---------------------------------------------------------------------------
 * (b) Fit.  Replaces main's node loop CC:105-140 for S specs at once:
 *   for every node row i (zero rows for unhealthy nodes included, CC:221-226):
 *     qc = alloc_cpu[i] <= used_cpu[i] ? 0 : int((alloc_cpu[i]-used_cpu[i]) / spec_cpu[s])   CC:119-124
 *     qm = alloc_mem[i] <= used_mem[i] ? 0 :     (alloc_mem[i]-used_mem[i]) / spec_mem[s]    CC:125-130
 *     q  = findMin(qc, qm)                                                                   CC:133
 *     if q >= alloc_pods[i] { q = alloc_pods[i] - pod_count[i] }                             CC:134-136
 *     totals[s] += q                                                                         CC:138
 *   spec_err[s] = KCC_SPEC_DIVZERO (1) iff the Go code would panic with an integer divide
 *   by zero (spec_cpu[s] == 0 reached on a row with free CPU, or spec_mem[s] == 0 on a
 *   row with free memory); totals[s] is then 0.  KCC_SPEC_FAULT (2): a device fault, see
 *   the conventions above.  pod_count = len(pods) (CC:106, CC:135).
 *   The verdict (CC:144) is totals[s] >= replicas[s], left to the caller.
 *   At most 2^26 - 1 specs per call.
 * ------------------------------------------------------------------------- */
int kcc_fit(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu,
            const int64_t* alloc_mem, const int64_t* alloc_pods,
            const int64_t* pod_count, const uint64_t* used_cpu, const int64_t* used_mem,
            int64_t n_specs, const uint64_t* spec_cpu, const int64_t* spec_mem,
            int64_t* totals, int32_t* spec_err);

/* Fused (a)+(b): containers -> used sums -> fit, one device round trip. */
int kcc_capacity(kcc_ctx* ctx, int64_t n_nodes, int64_t n_containers,
                 const int64_t* node_ptr, const uint64_t* cpu_req, const int64_t* mem_req,
                 const uint64_t* alloc_cpu, const int64_t* alloc_mem,
                 const int64_t* alloc_pods, const int64_t* pod_count, int64_t n_specs,
                 const uint64_t* spec_cpu, const int64_t* spec_mem, int64_t* totals,
                 int32_t* spec_err);

/* Device-level fit, split so that a node-sharded caller can all-reduce in between:
 *   kcc_fit_partial_async: partial[0..S)  = wrapping Σ over this call's nodes of q(i,s)
 *                          partial[S..2S) = number of divide-by-zero rows (< 2^48), or
 *                          on a faulted device that count plus one or more fault marks
 *                          of 2^48 (a count >= 2^48 after any sum over shards means a
 *                          faulted shard; a host-side finalize must test it BEFORE
 *                          count > 0 -> DIVZERO; kcc_fit_finalize -> KCC_SPEC_FAULT)
 *                          (both in an internal spec order; zeroed by this call)
 *   <optional all-reduce(sum, int64) of partial[0..2S) over node shards>
 *   kcc_fit_finalize_async: totals[s], spec_err[s] in caller order.
 * All ranks of a sharded run must pass the same specs.  `d_partial` holds 2*S int64. */
int kcc_fit_partial_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                          const int64_t* d_alloc_mem, const int64_t* d_alloc_pods,
                          const int64_t* d_pod_count, const uint64_t* d_used_cpu,
                          const int64_t* d_used_mem, int64_t n_specs,
                          const uint64_t* d_spec_cpu, const int64_t* d_spec_mem,
                          int64_t* d_partial, void* stream);
int kcc_fit_finalize_async(kcc_ctx* ctx, int64_t n_specs, const int64_t* d_partial,
                           int64_t* d_totals, int32_t* d_spec_err, void* stream);
/* kcc_fit_partial_async == kcc_fit_prepare_async + kcc_fit_run_async:
 *   prepare: zero d_partial, partition the specs (fast-path specs first) and build
 *            the per-node free-capacity records in the context workspace;
 *   run:     the nodes x specs fit kernel alone (what a profiler should attribute
 *            to the fit), accumulating into d_partial.
 * run must follow prepare on the same stream with the same sizes. */
int kcc_fit_prepare_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                          const int64_t* d_alloc_mem, const int64_t* d_alloc_pods,
                          const int64_t* d_pod_count, const uint64_t* d_used_cpu,
                          const int64_t* d_used_mem, int64_t n_specs,
                          const uint64_t* d_spec_cpu, const int64_t* d_spec_mem,
                          int64_t* d_partial, void* stream);
int kcc_fit_run_async(kcc_ctx* ctx, int64_t n_nodes, int64_t n_specs, int64_t* d_partial,
                      void* stream);

/* Convenience: partial + finalize on one device. */
int kcc_fit_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                  const int64_t* d_alloc_mem, const int64_t* d_alloc_pods,
                  const int64_t* d_pod_count, const uint64_t* d_used_cpu,
                  const int64_t* d_used_mem, int64_t n_specs, const uint64_t* d_spec_cpu,
                  const int64_t* d_spec_mem, int64_t* d_totals, int32_t* d_spec_err,
                  void* stream);

/* ---------------------------------------------------------------------------
 * Pipelined (a)+(b) on one device: reduce + fit partial of the whole hot path in one
 * call, d_partial as kcc_fit_partial_async (follow with an optional all-reduce and
 * kcc_fit_finalize_async).  n_chunks > 1 cuts the nodes into that many contiguous
 * ranges (fewer when chunks would be small) and runs the reduce of range k on a
 * library-owned side stream while `stream` fits range k-1; 0 = library default (1:
 * the overlap measured slower on MI355X).  h_node_ptr is a HOST copy
 * of the CSR offsets in d_node_ptr (used only to place the chunk boundaries; NULL =
 * one chunk).  The
 * per-node request sums land in d_used_cpu / d_used_mem (CC:290-293).  Everything is
 * ordered after the work already queued on `stream`, and `stream` waits for the side
 * stream before the call's last kernel: capturable into a hipGraph.
 * ------------------------------------------------------------------------- */
int kcc_capacity_partial_async(kcc_ctx* ctx, int64_t n_nodes, int64_t n_containers,
                               const int64_t* h_node_ptr, const int64_t* d_node_ptr,
                               const uint64_t* d_cpu_req, const int64_t* d_mem_req,
                               const uint64_t* d_alloc_cpu, const int64_t* d_alloc_mem,
                               const int64_t* d_alloc_pods, const int64_t* d_pod_count,
                               uint64_t* d_used_cpu, int64_t* d_used_mem, int64_t n_specs,
                               const uint64_t* d_spec_cpu, const int64_t* d_spec_mem,
                               int64_t* d_partial, int n_chunks, void* stream);
/* The whole step on one device without a cross-GPU exchange: kcc_capacity_partial_async
 * (one chunk, the partial in a library buffer) followed by the finalize, which rides in
 * the clamp correction's launch (its last workgroup to finish writes d_totals / d_spec_err):
 * the same results as partial + kcc_fit_finalize_async, one launch fewer
 * (ClusterCapacity.go:101-140 for a batch of specs, all on the device). */
int kcc_capacity_async(kcc_ctx* ctx, int64_t n_nodes, int64_t n_containers,
                       const int64_t* h_node_ptr, const int64_t* d_node_ptr,
                       const uint64_t* d_cpu_req, const int64_t* d_mem_req,
                       const uint64_t* d_alloc_cpu, const int64_t* d_alloc_mem,
                       const int64_t* d_alloc_pods, const int64_t* d_pod_count,
                       uint64_t* d_used_cpu, int64_t* d_used_mem, int64_t n_specs,
                       const uint64_t* d_spec_cpu, const int64_t* d_spec_mem, int64_t* d_totals,
                       int32_t* d_spec_err, void* stream);

/* ---------------------------------------------------------------------------
 * Node sharding.  Nodes are independent and each per-spec total is a
 * wrapping int64 sum, so a cluster splits into contiguous node ranges whose partial
 * vectors (kcc_fit_partial_async / kcc_capacity_partial_async) add up to the whole.
 *
 * kcc_set_node_shards: the host-array entry points (kcc_fit, kcc_capacity) cut the
 *   nodes into max(n_shards, devices) contiguous ranges (balanced by node count),
 *   dealt round-robin over the context's devices; a device's shards run one after the
 *   other and their partials are summed on it before the RCCL all-reduce over devices.
 *   0 (default) = one shard per device.  Same results for every shard count; more
 *   shards than devices rehearse a multi-GPU split on fewer GPUs.
 *
 * One process per GPU (the Go host as one process per device, or torchrun): every
 *   rank owns one node range and a single-device context; rank 0 creates an id with
 *   kcc_comm_unique_id and hands it to the other ranks (any channel: the bytes are
 *   opaque), every rank calls kcc_comm_init (collective: blocks until all joined), and
 *   each step runs kcc_capacity_partial_async -> kcc_allreduce_partial_async ->
 *   kcc_fit_finalize_async on one stream: an RCCL all-reduce (sum, int64) of the 2*S
 *   partial vector over xGMI, the only exchange.  Every rank must pass the same specs.
 * ------------------------------------------------------------------------- */
#define KCC_COMM_ID_BYTES 128
int kcc_set_node_shards(kcc_ctx* ctx, int n_shards);
int kcc_comm_unique_id(uint8_t* id /* [KCC_COMM_ID_BYTES] */);
int kcc_comm_init(kcc_ctx* ctx, const uint8_t* id, int n_ranks, int rank);
int kcc_allreduce_partial_async(kcc_ctx* ctx, int64_t n_specs, int64_t* d_partial, void* stream);

/* One-shot exchange over xGMI peer memory: the MI355X-native replacement for
 * kcc_allreduce_partial_async + kcc_fit_finalize_async when each rank is one process on
 * its own GPU (<= 8 ranks, a 2*S int64 payload: latency-bound, so one push over the
 * full mesh beats a ring).  Setup, once: kcc_p2p_export allocates this rank's mailbox
 * (2 parities x n_ranks x (2 * max_specs) int64 + flags) in fine-grained, uncached device
 * memory (peers write it while this GPU polls it) and returns its IPC handle;
 * every rank's handle travels to every rank (any channel: the bytes are opaque);
 * kcc_p2p_open maps the peers' mailboxes.  Each step: kcc_exchange_finalize_async (one
 * kernel on the caller's stream, after kcc_capacity_partial_async) pushes this rank's
 * partial into every mailbox, waits for every peer's push of the same step, sums and
 * finalizes totals / spec_err exactly as the all-reduce + finalize do.  Every rank must
 * call it the same number of times with the same specs.  A wait for a peer that never
 * pushes gives up after seconds and is counted (kcc_p2p_faults): that launch and every
 * finalize after it mark every spec KCC_SPEC_FAULT (see the conventions above); tests
 * and the bench assert 0.  Replaces RCCL only where its
 * ncclAllReduce(partial) stood (ClusterCapacity.go:138, the total over nodes). */
#define KCC_P2P_HANDLE_BYTES 64
#define KCC_P2P_MAX_SPECS (1 << 20)
int kcc_p2p_export(kcc_ctx* ctx, int n_ranks, int64_t max_specs,
                   uint8_t* handle /* [KCC_P2P_HANDLE_BYTES] */);
int kcc_p2p_open(kcc_ctx* ctx, int rank, const uint8_t* handles /* [n_ranks][64] */);
int kcc_exchange_finalize_async(kcc_ctx* ctx, int64_t n_specs, const int64_t* d_partial,
                                int64_t* d_totals, int32_t* d_spec_err, void* stream);
int kcc_p2p_faults(kcc_ctx* ctx, int64_t* faults);

/* Per-launch timing of kcc_capacity_partial_async (HIP events recorded on the stream
 * each kernel runs on): enable (1) / disable (0) resets the sums; read synchronises
 * and returns the summed durations and launch counts of the reduces (mark + reduce,
 * one per chunk) and of the fit kernel (one per chunk). */
int kcc_profile_enable(kcc_ctx* ctx, int on);
int kcc_profile_read(kcc_ctx* ctx, double* reduce_ms, int64_t* reduce_launches, double* fit_ms,
                     int64_t* fit_launches);

/* Look-back waits of the segmented reduce that gave up (summed over the context's
 * devices since the last kcc_clear_faults; synchronises).  A reduce launch assembles a
 * node cut by wave ranges from pieces the other waves publish; a wait that never sees
 * its piece (not expected on a healthy device) is counted here instead of hanging, and
 * the affected node's sums are then wrong.  Tests and the bench assert 0. */
int kcc_reduce_faults(kcc_ctx* ctx, int64_t* faults);
/* Reset the context's fault words and the reduce's look-back records (synchronises).
 * After an exchange fault (kcc_p2p_faults > 0) a late peer push may still land in the
 * mailbox: re-create the mailboxes (a new context) before exchanging again. */
int kcc_clear_faults(kcc_ctx* ctx);

/* The fit streams only the node rows that can add to its fast sum (free CPU, free
 * memory and allocatable pods > 0, within the fast bounds): every other row contributes
 * exactly 0 there (x = findMin(qc, qm) = 0; P <= 0 rows are applied by the clamp
 * correction; rows outside the bounds take the exact path), so the totals are the same
 * bit for bit.  kcc_set_fit_dense(ctx, 1) streams every row instead (diagnostic / A-B).
 * kcc_fit_stream_rows: node rows (padded to groups of 8) the last fit streamed, summed
 * over its node chunks (synchronises the device). */
int kcc_set_fit_dense(kcc_ctx* ctx, int dense);
/* Where the pod-slot clamp (CC:134-135, x >= allocatable pods ? allocatable - pod count : x)
 * is applied by kcc_capacity_partial_async / kcc_capacity_async: by the clamp correction
 * (a dominance count over the specs, one launch of its own; the fit's loop stays at 3 VALU
 * per node and spec wave) or inside the fit (5 VALU, no clamp launch, no clamp tables:
 * cheaper on small shards).  mode -1 (default): inside the fit when node rows x specs <=
 * 1.1e9 and specs <= 4096; 0: never; 1: whenever specs <= 4096 (one node chunk, not dense,
 * at least one node and one container).  A call that does not qualify applies the clamp by
 * the correction in every mode, and kcc_clamp_in_fit_used reports 0 for it.
 * The totals are the same bit for bit either way. */
int kcc_set_clamp_in_fit(kcc_ctx* ctx, int mode);
/* 1 when the last kcc_capacity_partial_async / kcc_capacity_async of the context applied
 * the clamp inside the fit (its VALU accounting per node x 64-spec wave: 5 for class-A
 * specs and 6.5 for class B, against 3 and 4.5 with the clamp correction). */
int kcc_clamp_in_fit_used(kcc_ctx* ctx, int* used);
int kcc_fit_stream_rows(kcc_ctx* ctx, int64_t* streamed);

/* Fraction of (node, spec) pairs of the last kcc_fit* call that took the exact
 * 64-bit path instead of the saturating fast path (diagnostic; host-computed from
 * the class counters the fit kernel keeps).  -1 if unknown. */
double kcc_last_slow_fraction(const kcc_ctx* ctx);

/* Same counter for the last kcc_fit_partial_async / kcc_fit_async on device 0 of
 * ctx: (node, spec) pairs that took the exact path, and all pairs.  Synchronises
 * the device. */
int kcc_fit_slow_pairs(kcc_ctx* ctx, int64_t* slow_pairs, int64_t* pairs);

/* ---------------------------------------------------------------------------
 * Quantity strings -> int64 (the caller side of (a)).
 * Strings are packed Arrow-style: string i = bytes[offsets[i], offsets[i+1]),
 * offsets non-decreasing, 0 <= offsets[i] <= n_bytes (n + 1 offsets).  Per string,
 * out[i] is the reference's value and status[i] one of KCC_PARSE_*; the call itself
 * returns KCC_OK unless an argument is invalid (the reference prints per-string errors
 * and carries on with 0, CC:315-316, CC:203-206).
 *
 *   kcc_parse_cpu_millis: convertCPUToMilis (CC:301-319) — one trailing 'm' means
 *     millicores, else cores x 1000 (Go int multiply, wraps); strconv.Atoi failure ->
 *     KCC_PARSE_ERR, value 0.  Replaces the per-container calls at CC:280 and CC:283
 *     (on cpuRequests.String() / cpuLimits.String()) and the node's at CC:197.
 *   kcc_parse_bytes: bytefmt.ToBytes (BF:75-105) — base-2 multiples for K/M/G/T with
 *     the reference's accepted spellings (KI and MI but not GI/TI), ParseFloat > 0,
 *     int64(float64 * multiple) with amd64 overflow (0x8000000000000000).  Replaces
 *     the node allocatable-memory conversion at CC:203 (and the flag parse, CC:78-81).
 *     KCC_PARSE_UNSUPPORTED marks the rare inputs outside the device's exact
 *     ParseFloat domain (more than 19 significant digits below 10^19, or a value at
 *     the float64 overflow / underflow edge); never a silently different value.
 * The *_async forms take device pointers (bytes 4-byte aligned) and a stream.
 * ------------------------------------------------------------------------- */
enum {
  KCC_PARSE_OK = 1,
  KCC_PARSE_ERR = 0,          /* the reference reports an error and uses 0 */
  KCC_PARSE_UNSUPPORTED = -1, /* outside the exact device domain; value 0  */
  KCC_PARSE_BADOFF = -2       /* malformed offsets (async forms only)      */
};
int kcc_parse_cpu_millis(kcc_ctx* ctx, int64_t n, const char* bytes, int64_t n_bytes,
                         const int64_t* offsets, uint64_t* out, int8_t* status);
int kcc_parse_bytes(kcc_ctx* ctx, int64_t n, const char* bytes, int64_t n_bytes,
                    const int64_t* offsets, int64_t* out, int8_t* status);
/* resource.Quantity.Value() of ParseQuantity(s) (CC:285-286, the containers' memory
 * requests): [+-] digits [. digits] + "", Ki..Ei, n u m k M G T P E or e<int> suffix;
 * rounded up away from zero, binary (Ki..Ei) magnitudes capped at 2^63 - 1.  Restated
 * from k8s.io/apimachinery's published algorithm, which is not vendored in the reference
 * (version unpinned): parity unpinned.  KCC_PARSE_ERR for strings
 * ParseQuantity rejects; KCC_PARSE_UNSUPPORTED (value 0) for a decimal amount beyond
 * 2^63 - 1 (k8s wraps it), a negative amount off ParseQuantity's int64 fast path and
 * binary-suffixed fractions with more than 19 significant digits. */
int kcc_parse_quantity(kcc_ctx* ctx, int64_t n, const char* bytes, int64_t n_bytes,
                       const int64_t* offsets, int64_t* out, int8_t* status);
int kcc_parse_quantity_async(kcc_ctx* ctx, int64_t n, const char* d_bytes, int64_t n_bytes,
                             const int64_t* d_offsets, int64_t* d_out, int8_t* d_status,
                             void* stream);
int kcc_parse_cpu_millis_async(kcc_ctx* ctx, int64_t n, const char* d_bytes, int64_t n_bytes,
                               const int64_t* d_offsets, uint64_t* d_out, int8_t* d_status,
                               void* stream);
int kcc_parse_bytes_async(kcc_ctx* ctx, int64_t n, const char* d_bytes, int64_t n_bytes,
                          const int64_t* d_offsets, int64_t* d_out, int8_t* d_status,
                          void* stream);

/* ---------------------------------------------------------------------------
 * Per-node sums from containers in LIST order.  A cluster-wide
 * Pods("").List (one call instead of the per-node List of CC:236) returns pods in
 * namespace/name order; key[i] is the row of container i's node (<0 or >= n_keys:
 * skipped).  Same sums as kcc_reduce_requests on the grouped (CSR) containers, bit for
 * bit (wrapping addition does not depend on order).  kcc_count_by_key gives
 * len(pods) per row (CC:106, CC:135) from the pods' keys.  Arrays 16-byte aligned.
 * ------------------------------------------------------------------------- */
int kcc_reduce_requests_keyed(kcc_ctx* ctx, int64_t n_keys, int64_t n_containers,
                              const int32_t* key, const uint64_t* cpu_req, const int64_t* mem_req,
                              const uint64_t* cpu_lim, const int64_t* mem_lim,
                              uint64_t* used_cpu, int64_t* used_mem, uint64_t* lim_cpu,
                              int64_t* lim_mem);
int kcc_reduce_requests_keyed_async(kcc_ctx* ctx, int64_t n_keys, int64_t n_containers,
                                    const int32_t* d_key, const uint64_t* d_cpu_req,
                                    const int64_t* d_mem_req, const uint64_t* d_cpu_lim,
                                    const int64_t* d_mem_lim, uint64_t* d_used_cpu,
                                    int64_t* d_used_mem, uint64_t* d_lim_cpu, int64_t* d_lim_mem,
                                    void* stream);
int kcc_count_by_key(kcc_ctx* ctx, int64_t n_keys, int64_t n, const int32_t* key, int64_t* count);
int kcc_count_by_key_async(kcc_ctx* ctx, int64_t n_keys, int64_t n, const int32_t* d_key,
                           int64_t* d_count, void* stream);

/* ---------------------------------------------------------------------------
 * Per-row "Max replicas" of one spec (the verbose report's
 * CC:137 line for every node row, CC:119-136): q[i] = row i's contribution to the total,
 * row_err[i] = 1 where Go would panic with an integer divide by zero at that row (q[i]
 * is then 0; the reference stops at the first such row).
 * ------------------------------------------------------------------------- */
int kcc_fit_rows(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu,
                 const int64_t* alloc_mem, const int64_t* alloc_pods, const int64_t* pod_count,
                 const uint64_t* used_cpu, const int64_t* used_mem, uint64_t spec_cpu,
                 int64_t spec_mem, int64_t* q, int32_t* row_err);

/* ---------------------------------------------------------------------------
 * Grouped fit: the totals of (b) broken down by node group, for S specs and G groups in one
 * call.  The reference notes that its node loop "needs be modified depending what label
 * selectors are applied to masters/nodes" (CC:188-194): a pod with a nodeSelector, node
 * affinity or missing tolerations fits only some pools, and its answer is the sum of the
 * eligible groups' cells.  group[i] (int32) is the group of node row i.
 *   totals[g * S + s] = what kcc_fit returns for spec s on exactly the rows with
 *     group[i] == g: CC:105-140 run on that sub-cluster, bit for bit — uint64 / int64 wrap,
 *     int(uint64) reinterpretation (CC:119-124), truncating signed memory division with
 *     MinInt64 / -1 == MinInt64 (CC:125-130), signed findMin (CC:133, CC:159-164), the
 *     allocatablePods - len(pods) clamp (CC:134-136), the wrapping total (CC:138).
 *   spec_err[g * S + s] = KCC_SPEC_DIVZERO iff Go would panic on that sub-cluster: some row
 *     of g has free CPU and spec_cpu[s] == 0, or free memory and spec_mem[s] == 0; totals is
 *     then 0 for that cell only.  A group made only of full rows does not panic on a zero
 *     request.
 *   Rows with group[i] < 0 or >= n_groups are skipped (as kcc_reduce_requests_keyed skips
 *   keys); an empty group gives total 0, err 0; the ids need not be sorted.
 *   For a spec with no flagged cell, the wrapping sum of its cells over the groups equals
 *   kcc_fit on the rows that were not skipped.
 * 1 <= n_groups, n_groups * n_specs <= 2^28, n_nodes <= 2^31 - 4096 (else KCC_EINVAL);
 * n_nodes == 0 or n_specs == 0: KCC_OK, every output 0.  The host-array form runs on the
 * context's device 0 and retains no caller pointer; the async form takes device pointers,
 * only enqueues on `stream`, allocates only when a size exceeds every earlier call's and
 * never synchronises.  No kernel of it waits on another workgroup: it cannot set a fault
 * word, and it does not read them.
 * ------------------------------------------------------------------------- */
int kcc_fit_grouped(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu,
                    const int64_t* alloc_mem, const int64_t* alloc_pods, const int64_t* pod_count,
                    const uint64_t* used_cpu, const int64_t* used_mem, const int32_t* group,
                    int64_t n_groups, int64_t n_specs, const uint64_t* spec_cpu,
                    const int64_t* spec_mem, int64_t* totals /* [G * S] */,
                    int32_t* spec_err /* [G * S] */);
int kcc_fit_grouped_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                          const int64_t* d_alloc_mem, const int64_t* d_alloc_pods,
                          const int64_t* d_pod_count, const uint64_t* d_used_cpu,
                          const int64_t* d_used_mem, const int32_t* d_group, int64_t n_groups,
                          int64_t n_specs, const uint64_t* d_spec_cpu, const int64_t* d_spec_mem,
                          int64_t* d_totals, int32_t* d_spec_err, void* stream);

/* ---------------------------------------------------------------------------
 * Fit with extended resources.  The reference counts CPU and memory only (CC:119-133); a
 * pod also requests ephemeral-storage, hugepages-* and device-plugin resources
 * (amd.com/gpu, nvidia.com/gpu), and min(freeCPU / c, freeMem / m, freeGPU / g, ...) per
 * node is not a sum of anything the other entry points return.  OPT-IN: with n_ext == 0
 * this is kcc_fit (group == NULL) or kcc_fit_grouped, bit for bit.
 *   n_ext = R extra resources, 0 <= R <= KCC_EXT_MAX, all int64 (Quantity.Value()):
 *     alloc_x[r * n_nodes + i], used_x[r * n_nodes + i]  node row i, resource r
 *     spec_x[r * n_specs + s]                             spec s, resource r
 *   An extra resource behaves as the memory column (CC:125-130) except that a zero request
 *   means "not requested": no constraint and no panic.  For row i and spec s:
 *     qc, qm and the divide-by-zero rule exactly as kcc_fit;  q = findMin(qc, qm)  (CC:133)
 *     for each r with x = spec_x[r][s] != 0:
 *       fx = alloc_x <= used_x ? 0 : alloc_x - used_x         (int64, the difference wraps)
 *       qx = fx == 0 ? 0 : fx / x   (Go int64 '/': truncating, MinInt64 / -1 == MinInt64)
 *       q  = findMin(q, qx)                                                       (signed)
 *     if q >= alloc_pods[i]: q = alloc_pods[i] - pod_count[i]     (CC:134-136, after the mins)
 *     totals[s] += q                                                               (wraps)
 *   A negative x takes the arithmetic of a negative memory request.  spec_err is
 *   KCC_SPEC_DIVZERO under kcc_fit's rule only; an extra resource never raises it.
 *   group / n_groups as in kcc_fit_grouped (cells [g * S + s], ids outside [0, G) skipped,
 *   a per-cell flag, an empty group 0 / 0); group == NULL requires n_groups == 1 and puts
 *   every row in group 0 (no sort is run).
 * n_groups * n_specs <= 2^28, n_nodes <= 2^31 - 4096; n_ext outside [0, KCC_EXT_MAX], a NULL
 * extra array with n_ext > 0, group == NULL with n_groups != 1: KCC_EINVAL.  n_nodes == 0 or
 * n_specs == 0: KCC_OK, every output 0.  Host and async forms as kcc_fit_grouped's: the
 * host form runs on the context's device 0 and retains no caller pointer; the async form
 * only enqueues, allocates only when a size exceeds every earlier call's, never
 * synchronises.  No kernel of it waits on another workgroup: it neither sets nor reads the
 * fault words.
 * ------------------------------------------------------------------------- */
#define KCC_EXT_MAX 4
int kcc_fit_ext(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu, const int64_t* alloc_mem,
                const int64_t* alloc_pods, const int64_t* pod_count, const uint64_t* used_cpu,
                const int64_t* used_mem, int64_t n_ext, const int64_t* alloc_x /* [R * N] */,
                const int64_t* used_x /* [R * N] */, const int32_t* group /* nullable */,
                int64_t n_groups, int64_t n_specs, const uint64_t* spec_cpu,
                const int64_t* spec_mem, const int64_t* spec_x /* [R * S] */,
                int64_t* totals /* [G * S] */, int32_t* spec_err /* [G * S] */);
int kcc_fit_ext_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                      const int64_t* d_alloc_mem, const int64_t* d_alloc_pods,
                      const int64_t* d_pod_count, const uint64_t* d_used_cpu,
                      const int64_t* d_used_mem, int64_t n_ext, const int64_t* d_alloc_x,
                      const int64_t* d_used_x, const int32_t* d_group, int64_t n_groups,
                      int64_t n_specs, const uint64_t* d_spec_cpu, const int64_t* d_spec_mem,
                      const int64_t* d_spec_x, int64_t* d_totals, int32_t* d_spec_err,
                      void* stream);

/* ---------------------------------------------------------------------------
 * Spread constraints in the fit: a per-node cap and a maxSkew over topology domains.  A
 * Deployment with required pod anti-affinity on the hostname ("at most k per node") or with
 * topologySpreadConstraints (whenUnsatisfiable: DoNotSchedule) holds fewer replicas than the
 * plain sum the other entry points report: three zones with room for 10, 4 and 7 and
 * maxSkew 1 hold 5 + 4 + 5 = 14, not 21.  OPT-IN, not the reference's arithmetic: with
 * node_cap, cell_min and group_rows all NULL, kcc_fit_capped is kcc_fit_ext bit for bit (it
 * launches the same kernels).
 *
 * kcc_fit_capped: kcc_fit_ext's arguments in its order, then
 *   node_cap[s]      (nullable) cap on one node's count for spec s; <= 0 or NULL: no cap
 *   cell_min[g*S+s]  (nullable output) the minimum of q over the cell's rows, before the cap
 *   group_rows[g]    (nullable output) rows with group id g; group == NULL: group_rows[0] =
 *                    n_nodes
 * For row i and spec s:
 *     q as kcc_fit_ext up to and including the pod-slot clamp (CC:134-136, after all the mins)
 *     qmin[cell] = signed min(qmin[cell], q)                            (before the cap)
 *     if node_cap[s] > 0 and q > node_cap[s]: q = node_cap[s]    (signed, after the clamp)
 *     totals[cell] += q                                                          (wraps)
 *   The cap follows the clamp because the clamp's value allocatablePods - len(pods) is a
 *   count of pods on that node too.  spec_err follows kcc_fit's rule unchanged; a flagged
 *   cell has totals 0 and cell_min 0; a cell with no rows has totals 0, err 0 and cell_min
 *   INT64_MAX (the identity of the min).  Argument errors and size limits are kcc_fit_ext's.
 *   n_nodes == 0: totals / spec_err 0, cell_min INT64_MAX, group_rows 0.  n_specs == 0: no
 *   cell is written; group_rows still is.
 *
 * kcc_spread_fold: the G x S cells (of kcc_fit_capped, kcc_fit_ext or kcc_fit_grouped) to
 * one total per spec.  domain_of[g] (int32, nullable: group g is its own domain, and then
 * n_domains must equal n_groups) maps groups to D topology domains, many to one, so that a
 * selector and a spread combine: groups are (pool, zone) pairs, domains are zones, eligible
 * picks the pools.  Per spec s:
 *   group g is live iff group_rows[g] > 0 (NULL: every group), eligible[g*S+s] != 0 (uint8;
 *     NULL: all) and domain_of[g] in [0, D) (other ids are skipped);
 *   spec_err[s] = KCC_SPEC_DIVZERO and totals[s] = 0 iff a live group's cell is flagged;
 *   cap_d = the wrapping sum of the live cells of domain d; d is present iff it has a live
 *     group (an empty pool is not a domain; a pool whose nodes are all full is one, with
 *     cap 0 — that is why spread constraints bite);
 *   no present domain: totals[s] = 0;
 *   max_skew[s] <= 0 (or max_skew NULL): totals[s] = the wrapping sum of the present cap_d
 *     (the sum of the live cells: the selector's answer);
 *   else m = signed min of cap_d over the present domains, lim = m + max_skew[s] saturating
 *     at INT64_MAX, totals[s] = the wrapping sum over the present domains of
 *     (cap_d <= lim ? cap_d : lim).
 * n_groups * n_specs <= 2^28, 1 <= n_domains, n_domains * n_specs <= 2^28, domain_of == NULL
 * with n_domains != n_groups, a negative size: KCC_EINVAL.  n_groups == 0 or n_specs == 0
 * (checked before n_domains): KCC_OK, outputs 0.
 *
 * Host and async forms as kcc_fit_ext's: the host forms run on the context's device 0 and
 * retain no caller pointer; the async forms take device pointers, only enqueue, allocate
 * only when a size exceeds every earlier call's and never synchronise (no readback between
 * the pair pass and the fold: both can be captured into one graph).  No kernel of either
 * waits on another workgroup: they neither set nor read the fault words.
 * ------------------------------------------------------------------------- */
int kcc_fit_capped(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu,
                   const int64_t* alloc_mem, const int64_t* alloc_pods, const int64_t* pod_count,
                   const uint64_t* used_cpu, const int64_t* used_mem, int64_t n_ext,
                   const int64_t* alloc_x /* [R * N] */, const int64_t* used_x /* [R * N] */,
                   const int32_t* group /* nullable */, int64_t n_groups, int64_t n_specs,
                   const uint64_t* spec_cpu, const int64_t* spec_mem,
                   const int64_t* spec_x /* [R * S] */, int64_t* totals /* [G * S] */,
                   int32_t* spec_err /* [G * S] */, const int64_t* node_cap /* [S], nullable */,
                   int64_t* cell_min /* [G * S], nullable */,
                   int64_t* group_rows /* [G], nullable */);
int kcc_fit_capped_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                         const int64_t* d_alloc_mem, const int64_t* d_alloc_pods,
                         const int64_t* d_pod_count, const uint64_t* d_used_cpu,
                         const int64_t* d_used_mem, int64_t n_ext, const int64_t* d_alloc_x,
                         const int64_t* d_used_x, const int32_t* d_group, int64_t n_groups,
                         int64_t n_specs, const uint64_t* d_spec_cpu, const int64_t* d_spec_mem,
                         const int64_t* d_spec_x, int64_t* d_totals, int32_t* d_spec_err,
                         const int64_t* d_node_cap, int64_t* d_cell_min, int64_t* d_group_rows,
                         void* stream);
int kcc_spread_fold(kcc_ctx* ctx, int64_t n_groups, int64_t n_specs,
                    const int64_t* cell_totals /* [G * S] */, const int32_t* cell_err /* [G * S] */,
                    const int64_t* group_rows /* [G], nullable */,
                    const int32_t* domain_of /* [G], nullable */, int64_t n_domains,
                    const uint8_t* eligible /* [G * S], nullable */,
                    const int64_t* max_skew /* [S], nullable */, int64_t* totals /* [S] */,
                    int32_t* spec_err /* [S] */);
int kcc_spread_fold_async(kcc_ctx* ctx, int64_t n_groups, int64_t n_specs,
                          const int64_t* d_cell_totals, const int32_t* d_cell_err,
                          const int64_t* d_group_rows, const int32_t* d_domain_of,
                          int64_t n_domains, const uint8_t* d_eligible, const int64_t* d_max_skew,
                          int64_t* d_totals, int32_t* d_spec_err, void* stream);

/* ---------------------------------------------------------------------------
 * The fit explained: which resource binds each node, and what is left over.  Every fit above
 * answers "how many replicas fit"; a planner asks next what stops them and what is stranded
 * when they stop.  That depends on which term won each node's findMin — not a sum of anything
 * another entry point returns.  OPT-IN, not the reference's arithmetic; no other call changes.
 *
 * kcc_fit_explain: kcc_fit_capped's input arguments in its order (node_cap included), then
 * totals / spec_err [G * S] — kcc_fit_capped's, bit for bit — and three nullable outputs,
 * plane-major (each plane an ordinary G x S cell array that kcc_spread_fold and a selector
 * can consume):
 *   why_rows[(b*G + g)*S + s]  rows of cell (g, s) whose reason is b          (KCC_WHY_SLOTS planes)
 *   why_pods[(b*G + g)*S + s]  the wrapping sum of the final q over those rows
 *   left[(c*G + g)*S + s]      what stays free once the cell holds its total: plane 0 CPU,
 *                              1 memory, 2 + r extra resource r                (2 + n_ext planes)
 * Reasons: KCC_WHY_CPU, KCC_WHY_MEM, KCC_WHY_EXT0 + r (r < KCC_EXT_MAX), KCC_WHY_PODS (the
 * pod-slot clamp), KCC_WHY_CAP (node_cap).  For row i and spec s, kcc_fit_capped's arithmetic
 * with the reason carried along; ties keep the earlier term, as findMin (CC:159-164) returns
 * its first argument on equality:
 *     q = qc, b = CPU;  if !(qc <= qm): q = qm, b = MEM
 *     for r = 0..R-1 with x_r != 0:  if !(q <= qx_r): q = qx_r, b = EXT0 + r
 *     if q >= alloc_pods[i]: q = alloc_pods[i] - pod_count[i], b = PODS   (CC:134-136: equality fires)
 *     if node_cap[s] > 0 and q > node_cap[s]: q = node_cap[s], b = CAP      (equality does not)
 *     why_rows[b][cell] += 1;  why_pods[b][cell] += q (wraps);  totals[cell] += q (wraps)
 *     left[0][cell] += fc_i - q * c            (uint64 wrap, stored as its int64 bits)
 *     left[1][cell] += fm_i - q * m
 *     left[2 + r][cell] += fx_r,i - q * x_r    (an unrequested resource leaves its whole fx)
 *   fc, fm, fx are the free amounts the fit uses (0 where alloc <= used, else the wrapping
 *   difference).  A row with no free CPU has qc = 0 and, unless a negative quotient beats it,
 *   reason CPU.  A flagged cell (kcc_fit's divide-by-zero rule) and an empty cell have every
 *   why_* and left entry 0; slots KCC_WHY_EXT0 + r with r >= n_ext are written 0.  With all
 *   three outputs NULL the call launches exactly kcc_fit_capped's kernels.
 * Argument errors and limits are kcc_fit_capped's, plus KCC_WHY_SLOTS * n_groups * n_specs <=
 * 2^28 when a why_* output is asked for (else KCC_EINVAL).  n_nodes == 0 or n_specs == 0:
 * KCC_OK, every output 0.  Host and async forms as kcc_fit_capped's: the async form only
 * enqueues, allocates only when a size exceeds every earlier call's, never synchronises and
 * reads no device value on the host (capturable into one graph on one stream).  No kernel of
 * it waits on another workgroup: it neither sets nor reads the fault words.
 * ------------------------------------------------------------------------- */
#define KCC_WHY_SLOTS 8
#define KCC_WHY_CPU 0
#define KCC_WHY_MEM 1
#define KCC_WHY_EXT0 2
#define KCC_WHY_PODS 6
#define KCC_WHY_CAP 7
int kcc_fit_explain(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu,
                    const int64_t* alloc_mem, const int64_t* alloc_pods, const int64_t* pod_count,
                    const uint64_t* used_cpu, const int64_t* used_mem, int64_t n_ext,
                    const int64_t* alloc_x /* [R * N] */, const int64_t* used_x /* [R * N] */,
                    const int32_t* group /* nullable */, int64_t n_groups, int64_t n_specs,
                    const uint64_t* spec_cpu, const int64_t* spec_mem,
                    const int64_t* spec_x /* [R * S] */, const int64_t* node_cap /* [S], nullable */,
                    int64_t* totals /* [G * S] */, int32_t* spec_err /* [G * S] */,
                    int64_t* why_rows /* [8 * G * S], nullable */,
                    int64_t* why_pods /* [8 * G * S], nullable */,
                    int64_t* left /* [(2 + R) * G * S], nullable */);
int kcc_fit_explain_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                          const int64_t* d_alloc_mem, const int64_t* d_alloc_pods,
                          const int64_t* d_pod_count, const uint64_t* d_used_cpu,
                          const int64_t* d_used_mem, int64_t n_ext, const int64_t* d_alloc_x,
                          const int64_t* d_used_x, const int32_t* d_group, int64_t n_groups,
                          int64_t n_specs, const uint64_t* d_spec_cpu, const int64_t* d_spec_mem,
                          const int64_t* d_spec_x, const int64_t* d_node_cap, int64_t* d_totals,
                          int32_t* d_spec_err, int64_t* d_why_rows, int64_t* d_why_pods,
                          int64_t* d_left, void* stream);

/* ---------------------------------------------------------------------------
 * A rollout plan placed on the nodes before the fit.  Every fit above answers "how many
 * replicas of one spec fit into the cluster as it stands"; its S specs are S independent
 * what-ifs.  "We roll out 40 of A and 200 of B; what fits after that, and where did they
 * land?" is sequential: kcc_deploy commits a plan of K steps to the node rows, in order, and
 * leaves the node state (on the device, in the async form) for the fit that follows.  OPT-IN,
 * not the reference's arithmetic; no other entry point changes.
 *
 *   Node arrays as kcc_fit_ext's: alloc_cpu, alloc_mem, alloc_pods, n_ext = R, alloc_x [R * N].
 *   State, updated in place: pod_count [N], used_cpu [N], used_mem [N], used_x [R * N].
 *   group [N] (nullable: n_groups must be 1, every row in group 0), n_groups = G and
 *     eligible [g * K + k] (uint8, nullable: every group eligible; the fold's convention with K
 *     in place of S): row i is eligible for step k iff group[i] is in [0, G) and its group's
 *     byte is nonzero.
 *   The plan: spec_cpu [K], spec_mem [K], spec_x [R * K], replicas [K], node_cap [K] (nullable;
 *     <= 0: no cap).  policy: KCC_DEPLOY_PACK or KCC_DEPLOY_SPREAD, one per call (a plan of
 *     mixed policies is several calls on one stream).
 *   Outputs: placed [K], nodes_used [K] (int64), step_err [K] (int32), placed_rows [K * N]
 *     (int64, nullable).
 *
 * Steps k = 0 .. K - 1 run in order; each sees the state the earlier steps left:
 *     Rk = clamp(replicas[k], 0, 2^31 - 1)
 *     for each eligible row i: q_i as kcc_fit_ext's for row i and spec k on the current state,
 *       up to and including the pod-slot clamp (CC:134-136, after all the mins); z_i = kcc_fit's
 *       divide-by-zero rule for that row
 *     if any eligible row has z_i: step_err[k] = KCC_SPEC_DIVZERO, placed[k] = nodes_used[k] = 0,
 *       its placed_rows 0, the state untouched; the next step runs.  An ineligible row never
 *       raises the flag.
 *     else a_i = 0 for an ineligible row; for an eligible one max(q_i, 0) (a negative clamp
 *       value holds nothing), then at most node_cap[k] where node_cap[k] > 0 (after the clamp, as
 *       kcc_fit_capped's), then at most Rk.  T = sum of a_i (< 2^62: nothing wraps).
 *     the placement p_i:
 *       Rk >= T: p_i = a_i.  Rk == 0: p_i = 0.
 *       PACK:   p_i = min(a_i, max(0, Rk - sum of a_j over j < i)): first fit in row order, the
 *               reference's own node order (CC:105)
 *       SPREAD (1 <= Rk < T): t = the smallest t >= 1 with sum of min(a_i, t) >= Rk;
 *               b_i = min(a_i, t - 1), rem = Rk - sum of b_i (1 <= rem <= #{a_i >= t}); the first
 *               rem rows in row order with a_i >= t get b_i + 1, every other row b_i: the even
 *               fill, each replica into an emptiest node that has room
 *     commit (wrapping as the reference's sums; with sane inputs nothing wraps):
 *       used_cpu[i] += p_i * spec_cpu[k] (uint64), used_mem[i] += p_i * spec_mem[k] (int64),
 *       used_x[r][i] += p_i * spec_x[r][k] for each requested r (a zero request leaves used_x[r]
 *       alone), pod_count[i] += p_i
 *     placed[k] = sum of p_i, nodes_used[k] = #{p_i > 0}, step_err[k] = KCC_SPEC_OK.
 *
 * Argument errors and size limits are kcc_fit_ext's with K in place of S (n_groups * K <= 2^28,
 * n_nodes <= 2^31 - 4096, K <= 2^20); a policy outside {0, 1}: KCC_EINVAL.  K == 0 or
 * n_nodes == 0: KCC_OK, outputs 0, the state untouched.  The host form runs on the context's
 * device 0, retains no caller pointer and writes the four state arrays back.  The async form
 * takes device pointers and only enqueues: it allocates only when a size exceeds every earlier
 * call's, never synchronises and never reads a device value on the host (the plan's values are
 * read on the device by index k); the number and kind of its launches depend only on (N, K, R,
 * policy), so it can be captured into a hipGraph with the kcc_fit*_async call that follows it.
 * No kernel of it waits on another workgroup: it neither sets nor reads the fault words.
 * ------------------------------------------------------------------------- */
#define KCC_DEPLOY_PACK 0
#define KCC_DEPLOY_SPREAD 1
int kcc_deploy(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu, const int64_t* alloc_mem,
               const int64_t* alloc_pods, int64_t n_ext, const int64_t* alloc_x /* [R * N] */,
               int64_t* pod_count, uint64_t* used_cpu, int64_t* used_mem,
               int64_t* used_x /* [R * N] */, const int32_t* group /* nullable */,
               int64_t n_groups, const uint8_t* eligible /* [G * K], nullable */, int64_t n_steps,
               const uint64_t* spec_cpu, const int64_t* spec_mem,
               const int64_t* spec_x /* [R * K] */, const int64_t* replicas,
               const int64_t* node_cap /* [K], nullable */, int policy, int64_t* placed /* [K] */,
               int64_t* nodes_used /* [K] */, int32_t* step_err /* [K] */,
               int64_t* placed_rows /* [K * N], nullable */);
int kcc_deploy_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                     const int64_t* d_alloc_mem, const int64_t* d_alloc_pods, int64_t n_ext,
                     const int64_t* d_alloc_x, int64_t* d_pod_count, uint64_t* d_used_cpu,
                     int64_t* d_used_mem, int64_t* d_used_x, const int32_t* d_group,
                     int64_t n_groups, const uint8_t* d_eligible, int64_t n_steps,
                     const uint64_t* d_spec_cpu, const int64_t* d_spec_mem,
                     const int64_t* d_spec_x, const int64_t* d_replicas,
                     const int64_t* d_node_cap, int policy, int64_t* d_placed,
                     int64_t* d_nodes_used, int32_t* d_step_err, int64_t* d_placed_rows,
                     void* stream);

/* ---------------------------------------------------------------------------
 * OPT-IN scheduler request model — explicitly NOT the
 * reference's semantics: the reference sums only the app containers of a node's pods
 * (CC:276-294, kcc_reduce_requests above; that stays the default).  This gives the
 * kube-scheduler's effective pod request instead (k8s pkg/api/v1/resource PodRequests,
 * sidecar-aware form; that dependency is absent here, parity unpinned beyond the
 * hand-derived cases of tests/test_pods.py), per resource, in the engine's 64-bit
 * wrapping domain (cpu uint64 with unsigned max, memory int64 with signed max):
 *   app = sum of the pod's app containers; side = 0; init = identity of max
 *   for each init container k of the pod, in order:
 *     restartable[k] (a sidecar): app += r_k; side += r_k; init = max(init, side)
 *     otherwise:                  init = max(init, r_k + side)
 *   req(p) = max(app, init) + overhead(p)
 * pod_ptr[P+1] / init_ptr[P+1]: CSR offsets of each pod's app / init containers.
 * init_ptr (with init_cpu, init_mem), restartable and the overhead pair are nullable
 * (absent = no init containers / none restartable / no overhead).
 * kcc_pod_requests: req(p) per pod.  kcc_reduce_requests_pods: also sums the pods of each
 * node (node_pod_ptr[N+1], pods grouped by node) into used_cpu / used_mem, the inputs
 * kcc_fit takes.  The *_async forms take device pointers (offsets must be in range;
 * the kernel clamps them, so a malformed CSR gives wrong sums, never a fault).
 * ------------------------------------------------------------------------- */
int kcc_pod_requests(kcc_ctx* ctx, int64_t n_pods, int64_t n_containers, int64_t n_init,
                     const int64_t* pod_ptr, const uint64_t* cpu_req, const int64_t* mem_req,
                     const int64_t* init_ptr, const uint64_t* init_cpu, const int64_t* init_mem,
                     const uint8_t* restartable, const uint64_t* ovh_cpu,
                     const int64_t* ovh_mem, uint64_t* pod_cpu, int64_t* pod_mem);
int kcc_pod_requests_async(kcc_ctx* ctx, int64_t n_pods, int64_t n_containers, int64_t n_init,
                           const int64_t* d_pod_ptr, const uint64_t* d_cpu_req,
                           const int64_t* d_mem_req, const int64_t* d_init_ptr,
                           const uint64_t* d_init_cpu, const int64_t* d_init_mem,
                           const uint8_t* d_restartable, const uint64_t* d_ovh_cpu,
                           const int64_t* d_ovh_mem, uint64_t* d_pod_cpu, int64_t* d_pod_mem,
                           void* stream);
int kcc_reduce_requests_pods(kcc_ctx* ctx, int64_t n_nodes, int64_t n_pods,
                             int64_t n_containers, int64_t n_init, const int64_t* node_pod_ptr,
                             const int64_t* pod_ptr, const uint64_t* cpu_req,
                             const int64_t* mem_req, const int64_t* init_ptr,
                             const uint64_t* init_cpu, const int64_t* init_mem,
                             const uint8_t* restartable, const uint64_t* ovh_cpu,
                             const int64_t* ovh_mem, uint64_t* used_cpu, int64_t* used_mem);

/* ---------------------------------------------------------------------------
 * Preemption what-if: per-priority request sums and a levelled fit.  Every fit above treats
 * the running pods as immovable; the kube-scheduler lets a pod of priority p that does not
 * fit evict pods of lower priority.  A planner asks both "how many replicas fit as things
 * stand" and "how many fit if everything below my priority makes way".  OPT-IN, not the
 * reference's arithmetic; no other entry point changes.
 *
 * A level is the rank of a priority class, 0 = lowest; 1 <= n_levels = L <= KCC_LEVELS_MAX.
 * Plane l of the node state holds the pods a spec of level l cannot evict: those with
 * pod_level >= l.  Plane 0 is every pod (today's answer); a spec above every pod uses a plane
 * that holds nothing.  This is an UPPER BOUND: every lower-priority pod yields.
 * PodDisruptionBudgets, preemptionPolicy: Never and the scheduler's minimal-victim choice are
 * out of scope.
 *
 * kcc_reduce_requests_levels: node_pod_ptr[N+1] (pods grouped by node), pod_ptr[P+1] (each
 * pod's app containers), cpu_req / mem_req per container as kcc_reduce_requests_pods';
 * pod_level[P] (uint8; a level >= L counts as L - 1).  Outputs, plane-major [L * N]:
 *   used_cpu[l*N + i]   the wrapping uint64 sum of cpu_req over the containers of the pods of
 *                       node i with pod_level >= l
 *   used_mem[l*N + i]   the same in int64
 *   pod_count[l*N + i]  the number of such pods (a pod without containers counts: CC:106
 *                       counts pods)
 * The app-container sum only (CC:276-294): the opt-in init / sidecar / overhead model above is
 * not combined here.  Plane 0 of used_* equals kcc_reduce_requests on the flattened CSR bit
 * for bit, plane 0 of pod_count equals the differences of node_pod_ptr.  Both adds wrap, so an
 * extended resource needs no entry point of its own: a second call with two extra columns in
 * the cpu_req / mem_req places gives two planes of used_x.
 * The host form validates both CSR arrays (offset 0 first, non-decreasing, the size last) and
 * 1 <= L <= KCC_LEVELS_MAX, else KCC_EINVAL; pods without nodes: KCC_EINVAL.  n_nodes == 0:
 * KCC_OK, nothing written; n_pods == 0: every output 0.  n_nodes <= 2^31 - 4096.  The async
 * form takes device pointers and clamps the offsets into range (a malformed CSR gives wrong
 * sums, never a fault); it only enqueues, allocates nothing and never synchronises.  No kernel
 * of it waits on another workgroup: it neither sets nor reads the fault words.
 *
 * kcc_fit_levels: kcc_fit_capped on the plane of each spec's level.  Node side: alloc_cpu,
 * alloc_mem, alloc_pods [N]; n_levels; pod_count, used_cpu, used_mem [L * N] (the planes
 * above); n_ext = R, alloc_x [R * N], used_x [L * R * N] (plane l an ordinary [R * N] block:
 * a caller without per-level data repeats its block); group, n_groups.  Spec side: n_specs,
 * spec_cpu, spec_mem, spec_x [R * S], node_cap (nullable) as kcc_fit_capped's, and
 * level_ptr[L+1], a HOST array in both forms: the specs are given sorted by level, specs
 * [level_ptr[l], level_ptr[l+1]) have level l.  level_ptr[0] == 0, non-decreasing,
 * level_ptr[L] == n_specs, else KCC_EINVAL.
 *   For each level l, columns [level_ptr[l], level_ptr[l+1]) of every group row of totals /
 *   spec_err [G * S] are exactly kcc_fit_capped's totals and spec_err for those specs on plane
 *   l's node arrays: the pod-slot clamp uses plane l's pod_count; the divide-by-zero rule,
 *   empty groups and skipped ids are kcc_fit_capped's.  With L == 1 the call is kcc_fit_capped
 *   bit for bit, on the same launches.
 * The intended use: pass a spec twice, at level 0 and at its own level, and read "as things
 * stand" and "with preemption" side by side.
 * Size limits and argument errors are kcc_fit_capped's.  n_nodes == 0 or n_specs == 0: KCC_OK,
 * outputs 0.  Host and async forms as kcc_fit_capped's: the async form only enqueues,
 * allocates only when a size exceeds every earlier call's, never synchronises and reads no
 * device value on the host; the number and kind of its launches depend only on (N, G, R, L,
 * level_ptr), so it can be captured into one graph behind kcc_reduce_requests_levels_async.
 * No kernel of it waits on another workgroup.
 * ------------------------------------------------------------------------- */
#define KCC_LEVELS_MAX 8
int kcc_reduce_requests_levels(kcc_ctx* ctx, int64_t n_nodes, int64_t n_pods, int64_t n_containers,
                               const int64_t* node_pod_ptr, const int64_t* pod_ptr,
                               const uint64_t* cpu_req, const int64_t* mem_req,
                               const uint8_t* pod_level, int64_t n_levels,
                               uint64_t* used_cpu /* [L * N] */, int64_t* used_mem /* [L * N] */,
                               int64_t* pod_count /* [L * N] */);
int kcc_reduce_requests_levels_async(kcc_ctx* ctx, int64_t n_nodes, int64_t n_pods,
                                     int64_t n_containers, const int64_t* d_node_pod_ptr,
                                     const int64_t* d_pod_ptr, const uint64_t* d_cpu_req,
                                     const int64_t* d_mem_req, const uint8_t* d_pod_level,
                                     int64_t n_levels, uint64_t* d_used_cpu, int64_t* d_used_mem,
                                     int64_t* d_pod_count, void* stream);
int kcc_fit_levels(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu,
                   const int64_t* alloc_mem, const int64_t* alloc_pods, int64_t n_levels,
                   const int64_t* pod_count /* [L * N] */, const uint64_t* used_cpu /* [L * N] */,
                   const int64_t* used_mem /* [L * N] */, int64_t n_ext,
                   const int64_t* alloc_x /* [R * N] */, const int64_t* used_x /* [L * R * N] */,
                   const int32_t* group /* nullable */, int64_t n_groups, int64_t n_specs,
                   const uint64_t* spec_cpu, const int64_t* spec_mem,
                   const int64_t* spec_x /* [R * S] */, const int64_t* node_cap /* [S], nullable */,
                   const int64_t* level_ptr /* [L + 1], host */, int64_t* totals /* [G * S] */,
                   int32_t* spec_err /* [G * S] */);
int kcc_fit_levels_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                         const int64_t* d_alloc_mem, const int64_t* d_alloc_pods, int64_t n_levels,
                         const int64_t* d_pod_count, const uint64_t* d_used_cpu,
                         const int64_t* d_used_mem, int64_t n_ext, const int64_t* d_alloc_x,
                         const int64_t* d_used_x, const int32_t* d_group, int64_t n_groups,
                         int64_t n_specs, const uint64_t* d_spec_cpu, const int64_t* d_spec_mem,
                         const int64_t* d_spec_x, const int64_t* d_node_cap,
                         const int64_t* h_level_ptr /* [L + 1], host */, int64_t* d_totals,
                         int32_t* d_spec_err, void* stream);

/* ---------------------------------------------------------------------------
 * Drain what-if: the pods of drained nodes re-placed before the fit.  Every call above treats
 * the node set as fixed.  "I cordon and drain this pool, or zone b goes dark: do the pods that
 * ran there still fit on the rest, and what is left for my spec afterwards?" takes rows away:
 * kcc_drain leaves the drained rows full, turns the pods that ran on them into a kcc_deploy
 * plan — one step per distinct request shape, big shapes first — places it on the surviving
 * rows and leaves the node state (on the device, in the async form) for the fit that follows.
 * OPT-IN, not the reference's arithmetic; no other entry point changes.
 * It is A placement the scheduler could make, not THE one it will make: the evicted pods' own
 * selectors, affinities, PodDisruptionBudgets and priorities are out of scope.
 *
 *   Node arrays as kcc_deploy's: alloc_cpu, alloc_mem, alloc_pods, n_ext = R, alloc_x [R * N].
 *   State, updated in place: pod_count [N], used_cpu [N], used_mem [N], used_x [R * N].
 *   drain [N] (uint8): row i is drained iff drain[i] != 0.
 *   The pods, grouped by node: node_pod_ptr [N + 1] (row i runs pods [node_pod_ptr[i],
 *     node_pod_ptr[i+1])), pod_cpu [P], pod_mem [P], pod_x [R * P] (nullable: zeros),
 *     pod_movable [P] (uint8, nullable: every pod movable).
 *   policy: KCC_DEPLOY_PACK or KCC_DEPLOY_SPREAD.  1 <= max_shapes = M <= KCC_DRAIN_MAX_SHAPES.
 *   Outputs: summary [KCC_DRAIN_SUMMARY]; shape_cpu, shape_mem, shape_count, shape_placed,
 *     shape_nodes (int64 but shape_cpu, uint64) and shape_err (int32), each [M]; shape_x [R * M].
 *
 *   1. The evicted pods are the pods p of the drained rows with pod_movable == NULL or
 *      pod_movable[p] != 0.  An unmovable pod (DaemonSet, static pod) goes away with its node.
 *      summary[0] = the drained rows, summary[1] = the evicted pods.
 *   2. A drained row is left full: used_cpu[i] = alloc_cpu[i], used_mem[i] = alloc_mem[i],
 *      used_x[r][i] = alloc_x[r][i] for every r, pod_count[i] = alloc_pods[i].  Every fit of
 *      this library then gives the row exactly 0 for every spec and never raises the
 *      divide-by-zero flag on it (no free CPU or memory: qc = qm = qx = 0; the clamp, if it
 *      fires, gives alloc_pods - pod_count = 0), and a deploy step places nothing on it: the
 *      state alone carries the drain into whatever call follows, the alloc_* arrays stay as
 *      they are.  kcc_fit_explain counts such a row under KCC_WHY_CPU with 0 replicas and 0
 *      left over.
 *   3. The shape of pod p is (pod_cpu[p], pod_mem[p], pod_x[0][p], ..., pod_x[R-1][p]); two pods
 *      share a shape iff all 2 + R words are equal.  D = the distinct shapes among the evicted
 *      pods, ordered DESCENDING, lexicographically, cpu compared as uint64 and every other
 *      word as int64 (big pods first: first-fit decreasing).  shape_cpu[j], shape_mem[j],
 *      shape_x[r * M + j] are shape j's words, shape_count[j] the evicted pods of that shape.
 *   4. For j = 0 .. D - 1 in that order, one kcc_deploy step on the current state, exactly as
 *      defined above: spec = shape j, replicas = shape_count[j], no node_cap, no groups (every
 *      row is eligible; the drained ones are full), the call's policy.  shape_placed[j],
 *      shape_nodes[j], shape_err[j] are that step's placed, nodes_used and step_err.  A shape
 *      with a zero cpu or memory request that meets a row with free CPU or memory is a flagged
 *      step (KCC_SPEC_DIVZERO, nothing placed), as everywhere in this library; the steps after
 *      it run.  summary[2] = D, summary[3] = the sum of shape_placed.  Entries j >= D of all
 *      seven shape arrays are 0.
 *   5. D > M: summary[2] = -1, summary[3] = 0, all seven shape arrays 0, nothing placed; the
 *      drained rows are still left full and summary[0], summary[1] still hold.
 *
 * n_nodes, n_ext and policy as kcc_deploy's; max_shapes outside [1, KCC_DRAIN_MAX_SHAPES],
 * n_pods outside [0, 2^31 - 4096], a NULL required array (drain with n_nodes > 0 included):
 * KCC_EINVAL.  n_nodes == 0: KCC_OK, summary and shape outputs 0 (pods without nodes:
 * KCC_EINVAL).  n_pods == 0: the drained rows are left full, summary = {rows, 0, 0, 0}.
 * The host form validates the CSR (offset 0 first, non-decreasing, n_pods last; else
 * KCC_EINVAL), runs on the context's device 0, retains no caller pointer, writes the four state
 * arrays back, and enqueues the D steps alone (it reads D back).  The async form takes device
 * pointers and clamps the CSR offsets into range (a malformed CSR gives wrong numbers, never a
 * fault); it only enqueues, never reads a device value on the host and allocates only when a
 * size exceeds every earlier call's.  It runs max_shapes deploy steps, the ones past D being
 * padding steps (spec (1, 1), 0 replicas) that place nothing, so the number and kind of its
 * launches depend only on (N, P, R, policy, max_shapes) and it can be captured into one linear
 * graph with the kcc_fit*_async call that follows: size max_shapes to the cluster, every
 * padding step costs a deploy step's launches.  Both forms give identical outputs.  No kernel
 * of it waits on another workgroup: it neither sets nor reads the fault words.
 * ------------------------------------------------------------------------- */
#define KCC_DRAIN_MAX_SHAPES 4096
#define KCC_DRAIN_SUMMARY 4 /* drained rows, evicted pods, shapes (or -1), placed pods */
int kcc_drain(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu, const int64_t* alloc_mem,
              const int64_t* alloc_pods, int64_t n_ext, const int64_t* alloc_x /* [R * N] */,
              int64_t* pod_count, uint64_t* used_cpu, int64_t* used_mem,
              int64_t* used_x /* [R * N] */, const uint8_t* drain /* [N] */, int64_t n_pods,
              const int64_t* node_pod_ptr /* [N + 1] */, const uint64_t* pod_cpu /* [P] */,
              const int64_t* pod_mem /* [P] */, const int64_t* pod_x /* [R * P], nullable */,
              const uint8_t* pod_movable /* [P], nullable */, int policy, int64_t max_shapes,
              int64_t* summary /* [KCC_DRAIN_SUMMARY] */, uint64_t* shape_cpu, int64_t* shape_mem,
              int64_t* shape_x /* [R * max_shapes] */, int64_t* shape_count,
              int64_t* shape_placed, int64_t* shape_nodes,
              int32_t* shape_err /* each [max_shapes] */);
int kcc_drain_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                    const int64_t* d_alloc_mem, const int64_t* d_alloc_pods, int64_t n_ext,
                    const int64_t* d_alloc_x, int64_t* d_pod_count, uint64_t* d_used_cpu,
                    int64_t* d_used_mem, int64_t* d_used_x, const uint8_t* d_drain,
                    int64_t n_pods, const int64_t* d_node_pod_ptr, const uint64_t* d_pod_cpu,
                    const int64_t* d_pod_mem, const int64_t* d_pod_x,
                    const uint8_t* d_pod_movable, int policy, int64_t max_shapes,
                    int64_t* d_summary, uint64_t* d_shape_cpu, int64_t* d_shape_mem,
                    int64_t* d_shape_x, int64_t* d_shape_count, int64_t* d_shape_placed,
                    int64_t* d_shape_nodes, int32_t* d_shape_err, void* stream);

/* ---------------------------------------------------------------------------
 * Removal what-if: each candidate node's pods re-placed on the rest.  "Which of these nodes
 * could I remove?" — the question of a cluster autoscaler's scale-down and of every cost
 * review — asks, for each candidate node ON ITS OWN, whether the pods that run there fit on
 * the rest of the cluster as it stands.  With every node as a candidate the same call answers
 * "does the cluster survive the loss of any single node?".  kcc_drain answers it for one set of
 * rows per call and rewrites the state; kcc_consolidate evaluates C candidates independently
 * in one launch and leaves the state alone.  OPT-IN, not the reference's arithmetic; no other
 * entry point changes.
 * It is A placement the scheduler could make, not THE one it will make.
 *
 *   Node arrays as kcc_deploy's: alloc_cpu, alloc_mem, alloc_pods, n_ext = R, alloc_x [R * N].
 *   The state, READ ONLY here: pod_count [N], used_cpu [N], used_mem [N], used_x [R * N].
 *   target [N] (uint8, nullable): row i may receive pods iff target[i] != 0 (NULL: every row).
 *   The pods, grouped by node, as kcc_drain's: node_pod_ptr [N + 1], pod_cpu [P], pod_mem [P],
 *     pod_x [R * P] (nullable: zeros), pod_movable [P] (uint8, nullable: every pod movable).
 *   cand [C]: the candidates' row indices.
 *   Outputs: cand_evicted, cand_placed, cand_zero (int64) and cand_err (int32), each [C];
 *     pod_target [P] (int64, nullable).
 *
 * Candidates are evaluated INDEPENDENTLY: each sees the state as passed in, none sees another's
 * placements, and the other candidates are ordinary target rows.  For candidate j with row
 * c = cand[j]:
 *   1. c outside [0, N): cand_err[j] = KCC_CAND_BADROW, the three counts are 0 and pod_target
 *      is not touched.
 *   2. The evicted pods are the pods p in [node_pod_ptr[c], node_pod_ptr[c+1]), in that order,
 *      with pod_movable == NULL or pod_movable[p] != 0.  An unmovable pod (DaemonSet, static
 *      pod) goes away with its node.  cand_evicted[j] = their number.  Above KCC_CONS_MAX_PODS:
 *      cand_err[j] = KCC_CAND_TOOMANY, cand_placed[j] = cand_zero[j] = 0 and the candidate's
 *      pods keep -2 in pod_target.
 *   3. An evicted pod with pod_cpu[p] == 0 or pod_mem[p] == 0 is counted in cand_zero[j] and
 *      not tried (as a kcc_deploy step it is either flagged or places nothing; here it is
 *      skipped without a row pass and the state is untouched either way).  pod_target[p] = -3.
 *   4. The remaining evicted pods, in order, are placed exactly as kcc_deploy would place a
 *      plan of one step per pod — spec = the pod's (cpu, mem, x[0..R)), replicas = 1, no
 *      node_cap, KCC_DEPLOY_PACK — on a PRIVATE copy of the state.  Row i is eligible iff
 *      i != c and (target == NULL or target[i] != 0).  A pod goes to the first eligible row in
 *      row order whose a_i >= 1, a_i being kcc_deploy's: kcc_fit_ext's q on the current private
 *      state, through the pod-slot clamp quirk of CC:134-136 (after all the mins; a row whose
 *      q reaches alloc_pods takes alloc_pods - pod_count instead), negatives counted as 0.  Its
 *      commit is kcc_deploy's with p_i = 1: used_cpu += cpu (uint64 wrap), used_mem += mem,
 *      used_x[r] += x_r for each requested resource, pod_count += 1.  A pod with no such row is
 *      not placed, and the pods after it are still tried.  cand_placed[j] = the placed pods;
 *      pod_target[p] = the row, or -1.  cand_err[j] = KCC_CAND_OK.
 *   5. pod_target, when given, is filled with -2 first: -2 marks a pod of a row that is no
 *      candidate, an unmovable pod, or a pod of a KCC_CAND_TOOMANY candidate.
 *   6. Duplicate entries of cand are allowed: each has its own output slot, and they write
 *      identical pod_target values.
 * Reading the result.  Strict: the node is removable iff cand_err == KCC_CAND_OK and
 * cand_placed == cand_evicted.  Lenient: cand_placed + cand_zero == cand_evicted (best-effort
 * pods, which request nothing, fit anywhere).  Nodes that are removable ONE AT A TIME need not
 * be removable TOGETHER: two candidates may both count on the same free room.  kcc_drain with
 * the chosen rows as its mask is the joint check.
 * Out of scope: the pods' selectors, affinities, PodDisruptionBudgets and priorities are not
 * read, as in kcc_drain.  There is no spread policy: an emptiest-row choice needs a full pass
 * over the rows per pod, where first fit stops at the first row that holds the pod.
 *
 * KCC_EINVAL: n_ext outside [0, KCC_EXT_MAX]; n_nodes > 2^31 - 4096; n_pods outside
 * [0, 2^31 - 4096]; n_cand negative or above 2^31 - 4096; a NULL required array (target, pod_x,
 * pod_movable and pod_target may be NULL); pods without nodes.  n_cand == 0 or n_nodes == 0:
 * KCC_OK, the per-candidate outputs 0 (err KCC_CAND_OK), pod_target still filled with -2.
 * The host form validates the CSR (offset 0 first, non-decreasing, n_pods last; else
 * KCC_EINVAL), runs on the context's device 0 and retains no caller pointer.  The async form
 * takes device pointers and clamps the CSR offsets into range (a malformed CSR gives wrong
 * numbers, never a fault); it only enqueues, never reads a device value on the host and
 * allocates nothing; its launches — the fill of pod_target and one workgroup per candidate —
 * depend only on (N, P, C, R), so it can be captured into one graph.  Both forms give
 * identical outputs.  No kernel of it waits on another workgroup: it neither sets nor reads
 * the fault words.
 * ------------------------------------------------------------------------- */
#define KCC_CONS_MAX_PODS 1024 /* evicted pods one candidate may have */
enum { KCC_CAND_OK = 0, KCC_CAND_BADROW = 1, KCC_CAND_TOOMANY = 2 };
int kcc_consolidate(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* alloc_cpu,
                    const int64_t* alloc_mem, const int64_t* alloc_pods, int64_t n_ext,
                    const int64_t* alloc_x /* [R * N] */, const int64_t* pod_count,
                    const uint64_t* used_cpu, const int64_t* used_mem,
                    const int64_t* used_x /* [R * N] */, const uint8_t* target /* [N]; nullable */,
                    int64_t n_pods, const int64_t* node_pod_ptr /* [N + 1] */,
                    const uint64_t* pod_cpu /* [P] */, const int64_t* pod_mem /* [P] */,
                    const int64_t* pod_x /* [R * P]; nullable */,
                    const uint8_t* pod_movable /* [P]; nullable */, int64_t n_cand,
                    const int64_t* cand /* [C] */, int64_t* cand_evicted, int64_t* cand_placed,
                    int64_t* cand_zero, int32_t* cand_err /* each [C] */,
                    int64_t* pod_target /* [P]; nullable */);
int kcc_consolidate_async(kcc_ctx* ctx, int64_t n_nodes, const uint64_t* d_alloc_cpu,
                          const int64_t* d_alloc_mem, const int64_t* d_alloc_pods, int64_t n_ext,
                          const int64_t* d_alloc_x, const int64_t* d_pod_count,
                          const uint64_t* d_used_cpu, const int64_t* d_used_mem,
                          const int64_t* d_used_x, const uint8_t* d_target, int64_t n_pods,
                          const int64_t* d_node_pod_ptr, const uint64_t* d_pod_cpu,
                          const int64_t* d_pod_mem, const int64_t* d_pod_x,
                          const uint8_t* d_pod_movable, int64_t n_cand, const int64_t* d_cand,
                          int64_t* d_cand_evicted, int64_t* d_cand_placed, int64_t* d_cand_zero,
                          int32_t* d_cand_err, int64_t* d_pod_target, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KCC_H */
