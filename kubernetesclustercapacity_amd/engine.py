"""Python face of libkcc.so: the reference's hot-path operations, batched.

Names follow the reference (AshutoshNirkhe/KubernetesClusterCapacity,
src/KubeAPI/ClusterCapacity.go = CC):

  get_pod_cpu_memory_requests_limits  <- getPodCPUMemoryRequestsLimits (CC:255-299)
  total_possible_max_replicas          <- main's node loop (CC:101-140)
  convert_cpu_to_milis                 <- convertCPUToMilis (CC:301-319), batched
  to_bytes                             <- bytefmt.ToBytes (BF:75-105), batched
  get_pod_cpu_memory_requests_limits_keyed  <- CC:255-299 over one cluster-wide pod List

Every call goes through the C-ABI into the gfx950 kernels; nothing is computed here.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib

COMM_ID_BYTES = 128  # KCC_COMM_ID_BYTES
P2P_HANDLE_BYTES = 64  # KCC_P2P_HANDLE_BYTES


class KccError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{_lib.ERROR_NAMES.get(code, code)}: {msg}")
        self.code = code


def _arr(x, dtype) -> np.ndarray:
    a = np.ascontiguousarray(x, dtype=dtype)
    return a


def _p(a) -> C.c_void_p | None:
    if a is None:
        return None
    return C.c_void_p(a.ctypes.data) if a.size else C.c_void_p(a.ctypes.data or 16)


def _dp(t) -> C.c_void_p | None:
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


@dataclass
class RequestSums:
    """Per-node sums, in the return order of getPodCPUMemoryRequestsLimits (CC:298)
    but as arrays: (cpu limits, cpu requests, memory limits, memory requests)."""
    cpu_limits: np.ndarray | None
    cpu_requests: np.ndarray
    memory_limits: np.ndarray | None
    memory_requests: np.ndarray


@dataclass
class DeployResult:
    """What CapacityEngine.deploy returns: per step the replicas placed, the nodes that took
    some and the flag (KCC_SPEC_*); the node state after the plan; rows[k, i] = replicas of
    step k on row i (None unless asked for)."""
    placed: np.ndarray
    nodes_used: np.ndarray
    err: np.ndarray
    pod_count: np.ndarray
    used_cpu: np.ndarray
    used_mem: np.ndarray
    used_x: np.ndarray
    rows: np.ndarray | None


@dataclass
class DrainResult:
    """What CapacityEngine.drain returns: the summary (drained rows, evicted pods, distinct
    shapes — -1 when they exceed max_shapes and nothing was placed — and placed pods), the
    shape arrays trimmed to the shapes found (descending; shape_x is [R, D]) and the node state
    after the drain."""
    drained_rows: int
    evicted: int
    shapes: int
    placed: int
    shape_cpu: np.ndarray
    shape_mem: np.ndarray
    shape_x: np.ndarray
    shape_count: np.ndarray
    shape_placed: np.ndarray
    shape_nodes: np.ndarray
    shape_err: np.ndarray
    pod_count: np.ndarray
    used_cpu: np.ndarray
    used_mem: np.ndarray
    used_x: np.ndarray


@dataclass
class ConsolidateResult:
    """What CapacityEngine.consolidate returns, per candidate: the evicted pods, how many of
    them were placed on the rest, how many request nothing (not tried) and the flag
    (KCC_CAND_*); pod_target[p] = the row pod p went to, -1 not placed, -2 not evicted by any
    candidate evaluated, -3 no requests (None unless asked for)."""
    evicted: np.ndarray
    placed: np.ndarray
    zero: np.ndarray
    err: np.ndarray
    pod_target: np.ndarray | None

    @property
    def removable(self) -> np.ndarray:
        """Strict: every evicted pod was placed."""
        return (self.err == _lib.KCC_CAND_OK) & (self.placed == self.evicted)

    @property
    def removable_lenient(self) -> np.ndarray:
        """Pods without requests count as placed: they fit anywhere."""
        return (self.err == _lib.KCC_CAND_OK) & (self.placed + self.zero == self.evicted)


@dataclass
class ExplainResult:
    """What CapacityEngine.fit_explain returns: fit_capped's totals / err, the rows and the
    replicas of each cell by reason ([KCC_WHY_SLOTS, G, S]) and what stays free ([2 + R, G, S]);
    without group ids the G axis is dropped.  A field not asked for is None."""
    totals: np.ndarray
    err: np.ndarray
    why_rows: np.ndarray | None
    why_pods: np.ndarray | None
    left: np.ndarray | None


class CapacityEngine:
    """One libkcc context (one device, or n_gpus devices with node sharding + RCCL)."""

    def __init__(self, device: int = 0, n_gpus: int = 1, lib_path: str | None = None):
        self._lib = _lib.lib(lib_path)
        h = C.c_void_p()
        rc = self._lib.kcc_create(C.byref(h), device, n_gpus)
        if rc != 0:
            raise KccError(rc, self._lib.kcc_create_error().decode())
        self._h = h
        self.device = device
        self.n_gpus = n_gpus

    # -- lifecycle -------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.kcc_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise KccError(rc, self._lib.kcc_last_error(self._h).decode())

    def reserve(self, max_nodes: int, max_containers: int, max_specs: int):
        self._check(self._lib.kcc_reserve(self._h, max_nodes, max_containers, max_specs))

    # -- host-array API (synchronous) -----------------------------------------
    def get_pod_cpu_memory_requests_limits(self, node_ptr, cpu_req, mem_req, cpu_lim=None,
                                           mem_lim=None) -> RequestSums:
        """CC:255-299 for every node at once: containers grouped per node (CSR)."""
        node_ptr = _arr(node_ptr, np.int64)
        n = node_ptr.size - 1
        if n < 0:
            raise ValueError("node_ptr must hold n_nodes + 1 offsets")
        cpu_req = _arr(cpu_req, np.uint64)
        mem_req = _arr(mem_req, np.int64)
        lim = cpu_lim is not None or mem_lim is not None
        if lim and (cpu_lim is None or mem_lim is None):
            raise ValueError("pass both cpu_lim and mem_lim, or neither")
        cpu_lim = _arr(cpu_lim, np.uint64) if lim else None
        mem_lim = _arr(mem_lim, np.int64) if lim else None
        nc = cpu_req.size
        if mem_req.size != nc or (lim and (cpu_lim.size != nc or mem_lim.size != nc)):
            raise ValueError("container arrays differ in length")
        used_cpu = np.zeros(max(n, 0), np.uint64)
        used_mem = np.zeros(max(n, 0), np.int64)
        lim_cpu = np.zeros(max(n, 0), np.uint64) if lim else None
        lim_mem = np.zeros(max(n, 0), np.int64) if lim else None
        self._check(self._lib.kcc_reduce_requests(
            self._h, n, nc, _p(node_ptr), _p(cpu_req), _p(mem_req), _p(cpu_lim), _p(mem_lim),
            _p(used_cpu), _p(used_mem), _p(lim_cpu), _p(lim_mem)))
        return RequestSums(lim_cpu, used_cpu, lim_mem, used_mem)

    def total_possible_max_replicas(self, alloc_cpu, alloc_mem, alloc_pods, pod_count,
                                    used_cpu, used_mem, spec_cpu, spec_mem):
        """CC:101-140 for S specs.  Returns (totals int64[S], spec_err int32[S])."""
        a = [_arr(alloc_cpu, np.uint64), _arr(alloc_mem, np.int64), _arr(alloc_pods, np.int64),
             _arr(pod_count, np.int64), _arr(used_cpu, np.uint64), _arr(used_mem, np.int64)]
        n = a[0].size
        if any(x.size != n for x in a):
            raise ValueError("node arrays differ in length")
        sc, sm = _arr(spec_cpu, np.uint64), _arr(spec_mem, np.int64)
        if sc.size != sm.size:
            raise ValueError("spec arrays differ in length")
        totals = np.zeros(sc.size, np.int64)
        err = np.zeros(sc.size, np.int32)
        self._check(self._lib.kcc_fit(self._h, n, *[_p(x) for x in a], sc.size, _p(sc), _p(sm),
                                      _p(totals), _p(err)))
        return totals, err

    def _cell_args(self, rows6, spec_cpu, spec_mem, group, n_groups, alloc_x=None, used_x=None,
                   spec_x=None):
        """What fit_grouped, fit_ext and fit_capped share: coercion, the shape checks and the
        [G, S] outputs.  Returns (a, R, ax, ux, group, G, sc, sm, sx, totals, err): a the six
        node columns; alloc_x / used_x / spec_x None: no extra resource (R = 0)."""
        a = [_arr(x, t) for x, t in zip(rows6, (np.uint64, np.int64, np.int64, np.int64,
                                                np.uint64, np.int64))]
        n = a[0].size
        if group is not None:
            group = _key32(group)
        if any(x.size != n for x in a) or (group is not None and group.size != n):
            raise ValueError("node arrays differ in length")
        sc, sm = _arr(spec_cpu, np.uint64), _arr(spec_mem, np.int64)
        if sc.size != sm.size:
            raise ValueError("spec arrays differ in length")
        S = sc.size
        ax = _arr(np.zeros((0, n)) if alloc_x is None else alloc_x, np.int64)
        ux = _arr(np.zeros((0, n)) if used_x is None else used_x, np.int64)
        sx = _arr(np.zeros((0, S)) if spec_x is None else spec_x, np.int64)
        if ax.ndim != 2 or ux.shape != ax.shape or ax.shape[1] != n:
            raise ValueError("alloc_x and used_x must both be [R, N]")
        R = ax.shape[0]
        if sx.shape != (R, S):
            raise ValueError("spec_x must be [R, S]")
        G = int(n_groups)
        totals = np.zeros((max(G, 0), S), np.int64)
        err = np.zeros((max(G, 0), S), np.int32)
        return a, R, ax, ux, group, G, sc, sm, sx, totals, err

    def fit_grouped(self, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
                    group, n_groups, spec_cpu, spec_mem):
        """CC:101-140 per node group: totals[g, s] is total_possible_max_replicas on the rows
        with group[i] == g (ids < 0 or >= n_groups: skipped), err[g, s] = 1 where Go would
        panic on that sub-cluster.  Returns (totals int64[G, S], err int32[G, S]); a
        selector's answer is select_groups over its eligible groups."""
        a, _, _, _, group, G, sc, sm, _, totals, err = self._cell_args(
            (alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem), spec_cpu, spec_mem,
            group, n_groups)
        self._check(self._lib.kcc_fit_grouped(self._h, a[0].size, *[_p(x) for x in a], _p(group),
                                              G, sc.size, _p(sc), _p(sm), _p(totals), _p(err)))
        return totals, err

    def fit_grouped_async(self, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
                          group, n_groups, spec_cpu, spec_mem, totals, spec_err, stream=None):
        """Device form of fit_grouped (torch tensors on the engine's device; group int32,
        totals int64 / spec_err int32 of n_groups * n_specs elements).  The arguments go to
        the C-ABI as they are (None: NULL), which validates them."""
        n = 0 if alloc_cpu is None else alloc_cpu.numel()
        s = 0 if spec_cpu is None else spec_cpu.numel()
        self._check(self._lib.kcc_fit_grouped_async(
            self._h, n, _dp(alloc_cpu), _dp(alloc_mem), _dp(alloc_pods), _dp(pod_count),
            _dp(used_cpu), _dp(used_mem), _dp(group), int(n_groups), s, _dp(spec_cpu),
            _dp(spec_mem), _dp(totals), _dp(spec_err), _stream(stream)))

    def fit_ext(self, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
                alloc_x, used_x, spec_cpu, spec_mem, spec_x, group=None, n_groups=1):
        """The fit with R extra resources (GPUs, ephemeral storage, hugepages; opt-in, not
        the reference's two-resource arithmetic): alloc_x / used_x int64 [R, N], spec_x
        int64 [R, S].  An extra resource joins findMin as a second memory column, except
        that a zero request leaves it out (no constraint, no panic); the pod-slot clamp
        follows all the mins.  R = 0 is total_possible_max_replicas (group None) or
        fit_grouped.  Returns (totals int64, err int32) of shape [S] without group ids and
        [n_groups, S] with them."""
        a, R, ax, ux, group, G, sc, sm, sx, totals, err = self._cell_args(
            (alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem), spec_cpu, spec_mem,
            group, n_groups, alloc_x, used_x, spec_x)
        self._check(self._lib.kcc_fit_ext(self._h, a[0].size, *[_p(x) for x in a], R, _p(ax),
                                          _p(ux), _p(group), G, sc.size, _p(sc), _p(sm), _p(sx),
                                          _p(totals), _p(err)))
        if group is None:
            return totals[0], err[0]
        return totals, err

    def fit_ext_async(self, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
                      n_ext, alloc_x, used_x, group, n_groups, spec_cpu, spec_mem, spec_x,
                      totals, spec_err, stream=None):
        """Device form of fit_ext (torch tensors on the engine's device; alloc_x / used_x
        int64 of n_ext * N elements, spec_x of n_ext * S, resource-major; group int32 or
        None; totals int64 / spec_err int32 of n_groups * S elements).  The arguments go to
        the C-ABI as they are (None: NULL), which validates them."""
        n = 0 if alloc_cpu is None else alloc_cpu.numel()
        s = 0 if spec_cpu is None else spec_cpu.numel()
        self._check(self._lib.kcc_fit_ext_async(
            self._h, n, _dp(alloc_cpu), _dp(alloc_mem), _dp(alloc_pods), _dp(pod_count),
            _dp(used_cpu), _dp(used_mem), int(n_ext), _dp(alloc_x), _dp(used_x), _dp(group),
            int(n_groups), s, _dp(spec_cpu), _dp(spec_mem), _dp(spec_x), _dp(totals),
            _dp(spec_err), _stream(stream)))

    # -- spread constraints (opt-in; include/kcc.h) -----------------
    def fit_capped(self, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
                   alloc_x, used_x, spec_cpu, spec_mem, spec_x, group=None, n_groups=1,
                   node_cap=None, want_min=True, want_rows=True):
        """fit_ext with a per-spec cap on one node's count (node_cap int64 [S]; <= 0 or None:
        no cap; "at most k per node", applied after the pod-slot clamp), the minimum of q
        over each cell's rows before the cap (cell_min) and the rows of each group
        (group_rows).  Opt-in, not the reference's arithmetic; with node_cap None and
        want_min / want_rows False it is fit_ext bit for bit.  alloc_x / used_x / spec_x may
        be None (no extra resource).  Returns (totals int64, err int32, cell_min int64 or
        None, group_rows int64 [n_groups] or None); the first three are [S] without group ids
        and [n_groups, S] with them.  A flagged cell has cell_min 0, a cell with no rows
        INT64_MAX."""
        a, R, ax, ux, group, G, sc, sm, sx, totals, err = self._cell_args(
            (alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem), spec_cpu, spec_mem,
            group, n_groups, alloc_x, used_x, spec_x)
        S = sc.size
        cap = None if node_cap is None else _arr(node_cap, np.int64)
        if cap is not None and cap.shape != (S,):
            raise ValueError("node_cap must be [S]")
        cmin = np.zeros((max(G, 0), S), np.int64) if want_min else None
        grows = np.zeros(max(G, 0), np.int64) if want_rows else None
        self._check(self._lib.kcc_fit_capped(self._h, a[0].size, *[_p(x) for x in a], R, _p(ax),
                                             _p(ux), _p(group), G, S, _p(sc), _p(sm), _p(sx),
                                             _p(totals), _p(err), _p(cap), _p(cmin), _p(grows)))
        if group is None:
            return totals[0], err[0], None if cmin is None else cmin[0], grows
        return totals, err, cmin, grows

    def fit_capped_async(self, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
                         n_ext, alloc_x, used_x, group, n_groups, spec_cpu, spec_mem, spec_x,
                         totals, spec_err, node_cap=None, cell_min=None, group_rows=None,
                         stream=None):
        """Device form of fit_capped (torch tensors on the engine's device, as
        fit_ext_async's; node_cap int64 [S], cell_min int64 of n_groups * S elements,
        group_rows int64 [n_groups]).  The arguments go to the C-ABI as they are (None:
        NULL), which validates them."""
        n = 0 if alloc_cpu is None else alloc_cpu.numel()
        s = 0 if spec_cpu is None else spec_cpu.numel()
        self._check(self._lib.kcc_fit_capped_async(
            self._h, n, _dp(alloc_cpu), _dp(alloc_mem), _dp(alloc_pods), _dp(pod_count),
            _dp(used_cpu), _dp(used_mem), int(n_ext), _dp(alloc_x), _dp(used_x), _dp(group),
            int(n_groups), s, _dp(spec_cpu), _dp(spec_mem), _dp(spec_x), _dp(totals),
            _dp(spec_err), _dp(node_cap), _dp(cell_min), _dp(group_rows), _stream(stream)))

    def spread_fold(self, cell_totals, cell_err, group_rows=None, domain_of=None,
                    n_domains=None, eligible=None, max_skew=None):
        """The G x S cells to one total per spec under a maxSkew over topology domains
        (topologySpreadConstraints, DoNotSchedule; opt-in).  domain_of int32 [G] maps groups
        to domains, many to one (None: each group its own domain); a group is live when
        group_rows[g] > 0 (None: all), eligible (bool [G, S] or [G]; None: all) and its
        domain id lies in [0, n_domains).  max_skew int64 [S] (None or <= 0:
        unconstrained, the sum of the live cells — select_groups' answer).  Returns
        (totals int64[S], err int32[S]); err[s] = 1 (totals 0) when a live cell is flagged."""
        t = _arr(cell_totals, np.int64)
        e = _arr(cell_err, np.int32)
        if t.ndim != 2 or e.shape != t.shape:
            raise ValueError("cell_totals and cell_err must both be [G, S]")
        G, S = t.shape
        gr = None if group_rows is None else _arr(group_rows, np.int64)
        dom = None if domain_of is None else _key32(domain_of)
        for v in (gr, dom):
            if v is not None and v.shape != (G,):
                raise ValueError("group_rows and domain_of must be [G]")
        if n_domains is None:
            n_domains = G if dom is None else max(int(dom.max(initial=0)) + 1, 1)
        el = None
        if eligible is not None:
            m = np.asarray(eligible, bool)
            if m.shape == (G,):
                m = np.broadcast_to(m[:, None], t.shape)
            if m.shape != t.shape:
                raise ValueError("eligible must be [G, S] or [G]")
            el = _arr(m, np.uint8)
        sk = None if max_skew is None else _arr(max_skew, np.int64)
        if sk is not None and sk.shape != (S,):
            raise ValueError("max_skew must be [S]")
        totals = np.zeros(S, np.int64)
        err = np.zeros(S, np.int32)
        self._check(self._lib.kcc_spread_fold(self._h, G, S, _p(t), _p(e), _p(gr), _p(dom),
                                              int(n_domains), _p(el), _p(sk), _p(totals),
                                              _p(err)))
        return totals, err

    def spread_fold_async(self, n_groups, n_specs, cell_totals, cell_err, group_rows, domain_of,
                          n_domains, eligible, max_skew, totals, spec_err, stream=None):
        """Device form of spread_fold (torch tensors: cells int64 / int32 of G * S elements,
        group_rows int64 [G], domain_of int32 [G], eligible uint8 of G * S, max_skew int64
        [S], totals int64 / spec_err int32 [S]; None: NULL).  No readback: it can follow
        fit_capped_async on one stream, or in one captured graph."""
        self._check(self._lib.kcc_spread_fold_async(
            self._h, int(n_groups), int(n_specs), _dp(cell_totals), _dp(cell_err),
            _dp(group_rows), _dp(domain_of), int(n_domains), _dp(eligible), _dp(max_skew),
            _dp(totals), _dp(spec_err), _stream(stream)))

    def fit_spread(self, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
                   alloc_x, used_x, spec_cpu, spec_mem, spec_x, group=None, n_groups=1,
                   node_cap=None, zone_of=None, max_skew=None, eligible=None,
                   host_max_skew=None, n_zones=None):
        """Replicas per spec under spread constraints, in one call: fit_capped, then
        spread_fold with zone_of as the groups' domains.
          node_cap       int64 [S]: at most this many on one node (<= 0: no cap)
          zone_of        int32 [G]: the zone of each group (None: each group its own domain)
          max_skew       int64 [S]: maxSkew over the zones (None or <= 0: unconstrained)
          eligible       bool [G, S] or [G]: the groups a spec's selector admits
          host_max_skew  int64 [S]: maxSkew with topologyKey kubernetes.io/hostname
          n_zones        zones (None: the largest id in zone_of + 1); ids outside are skipped
        host_max_skew takes two pair passes: the first gives cell_min; m[s] is its minimum
        over the live eligible groups (a node over its pod limit counts as holding 0), and
        the second pass caps a node at max(m[s], 0) + host_max_skew[s] (saturating), combined
        with node_cap by min.  That minimum over G x S numbers is the only host arithmetic
        here, like select_groups'.  Returns (totals int64[S], err int32[S])."""
        rows6 = (alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem)
        S = np.asarray(spec_cpu).size
        G = int(n_groups)
        cap = None if node_cap is None else _arr(node_cap, np.int64)
        two = host_max_skew is not None
        t, e, cmin, grows = self.fit_capped(*rows6, alloc_x, used_x, spec_cpu, spec_mem, spec_x,
                                            group, G, cap, want_min=two)
        if two:
            hk = _arr(host_max_skew, np.int64)
            if hk.shape != (S,):
                raise ValueError("host_max_skew must be [S]")
            live = np.broadcast_to((grows > 0)[:, None], (G, S))
            if zone_of is not None:
                z = np.asarray(zone_of, np.int64)
                nz = int(n_zones) if n_zones is not None else max(int(z.max(initial=0)) + 1, 1)
                live = live & ((z >= 0) & (z < nz))[:, None]
            if eligible is not None:
                m = np.asarray(eligible, bool)
                live = live & (m[:, None] if m.ndim == 1 else m)
            big = np.iinfo(np.int64).max
            m = np.where(live, cmin.reshape(G, S), big).min(axis=0, initial=big)
            m = np.maximum(m, 0)
            hcap = np.where(hk > big - m, big, m + np.minimum(hk, big - m))  # saturating
            cap2 = np.where(hk > 0, hcap, 0)
            if cap is not None:
                cap2 = np.where(cap > 0, np.where(cap2 > 0, np.minimum(cap, cap2), cap), cap2)
            t, e, _, grows = self.fit_capped(*rows6, alloc_x, used_x, spec_cpu, spec_mem, spec_x,
                                             group, G, cap2, want_min=False)
        return self.spread_fold(t.reshape(G, S), e.reshape(G, S), grows, zone_of, n_zones,
                                eligible, max_skew)

    # -- the fit explained (opt-in; include/kcc.h) ----------------------
    def fit_explain(self, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
                    alloc_x, used_x, spec_cpu, spec_mem, spec_x, group=None, n_groups=1,
                    node_cap=None, want_rows=True, want_pods=True, want_left=True
                    ) -> "ExplainResult":
        """fit_capped with the term that binds each node kept: per cell the rows (why_rows) and
        the replicas (why_pods) by reason — slot KCC_WHY_CPU, KCC_WHY_MEM, KCC_WHY_EXT0 + r,
        KCC_WHY_PODS (the pod-slot clamp), KCC_WHY_CAP (node_cap); ties keep the earlier term —
        and what stays free once the cell holds its total (left: plane 0 CPU, 1 memory, 2 + r
        extra resource r).  Opt-in, not the reference's arithmetic; totals / err are
        fit_capped's bit for bit.  A flagged or empty cell has every entry 0.  want_* False:
        that field is None (all three False: fit_capped's own kernels).  alloc_x / used_x /
        spec_x may be None (no extra resource)."""
        a, R, ax, ux, group, G, sc, sm, sx, totals, err = self._cell_args(
            (alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem), spec_cpu, spec_mem,
            group, n_groups, alloc_x, used_x, spec_x)
        S = sc.size
        cap = None if node_cap is None else _arr(node_cap, np.int64)
        if cap is not None and cap.shape != (S,):
            raise ValueError("node_cap must be [S]")
        g0 = max(G, 0)
        wr = np.zeros((_lib.KCC_WHY_SLOTS, g0, S), np.int64) if want_rows else None
        wp = np.zeros((_lib.KCC_WHY_SLOTS, g0, S), np.int64) if want_pods else None
        left = np.zeros((2 + R, g0, S), np.int64) if want_left else None
        self._check(self._lib.kcc_fit_explain(self._h, a[0].size, *[_p(x) for x in a], R, _p(ax),
                                              _p(ux), _p(group), G, S, _p(sc), _p(sm), _p(sx),
                                              _p(cap), _p(totals), _p(err), _p(wr), _p(wp),
                                              _p(left)))
        if group is None:
            def drop(v, axis):
                return None if v is None else v.take(0, axis=axis)
            return ExplainResult(totals[0], err[0], drop(wr, 1), drop(wp, 1), drop(left, 1))
        return ExplainResult(totals, err, wr, wp, left)

    def fit_explain_async(self, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
                          n_ext, alloc_x, used_x, group, n_groups, spec_cpu, spec_mem, spec_x,
                          node_cap, totals, spec_err, why_rows=None, why_pods=None, left=None,
                          stream=None):
        """Device form of fit_explain (torch tensors on the engine's device, as
        fit_capped_async's; why_rows / why_pods int64 of KCC_WHY_SLOTS * n_groups * S elements,
        left of (2 + n_ext) * n_groups * S, plane-major).  The arguments go to the C-ABI as
        they are (None: NULL), which validates them."""
        n = 0 if alloc_cpu is None else alloc_cpu.numel()
        s = 0 if spec_cpu is None else spec_cpu.numel()
        self._check(self._lib.kcc_fit_explain_async(
            self._h, n, _dp(alloc_cpu), _dp(alloc_mem), _dp(alloc_pods), _dp(pod_count),
            _dp(used_cpu), _dp(used_mem), int(n_ext), _dp(alloc_x), _dp(used_x), _dp(group),
            int(n_groups), s, _dp(spec_cpu), _dp(spec_mem), _dp(spec_x), _dp(node_cap),
            _dp(totals), _dp(spec_err), _dp(why_rows), _dp(why_pods), _dp(left),
            _stream(stream)))

    # -- a rollout plan placed on the nodes (opt-in; include/kcc.h) ----
    def deploy(self, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
               spec_cpu, spec_mem, replicas, policy=_lib.KCC_DEPLOY_PACK, alloc_x=None,
               used_x=None, spec_x=None, node_cap=None, group=None, n_groups=1, eligible=None,
               want_rows=True) -> "DeployResult":
        """Commits a plan of K steps to the node rows, in order: step k places up to
        replicas[k] pods of (spec_cpu[k], spec_mem[k], spec_x[:, k]) on the eligible rows that
        can hold them (fit_ext's per-row count after the pod-slot clamp, never negative, at
        most node_cap[k] where that is > 0), first fit in row order (KCC_DEPLOY_PACK) or as an
        even fill (KCC_DEPLOY_SPREAD), and adds them to pod_count / used_cpu / used_mem /
        used_x, which the next step and the fit that follows see.  eligible: bool [G, K] or
        [G] (None: every group); rows with a group id outside [0, n_groups) take nothing.  A
        step on which Go would panic on an eligible row is flagged (err[k] = 1) and places
        nothing.  The inputs are not modified: the result carries the updated state."""
        a = [_arr(x, t) for x, t in zip((alloc_cpu, alloc_mem, alloc_pods),
                                        (np.uint64, np.int64, np.int64))]
        st = [np.array(x, dtype=t, order="C", copy=True)
              for x, t in zip((pod_count, used_cpu, used_mem), (np.int64, np.uint64, np.int64))]
        n = a[0].size
        if group is not None:
            group = _key32(group)
        if any(x.shape != (n,) for x in a + st) or (group is not None and group.size != n):
            raise ValueError("node arrays differ in length")
        sc, sm, rep = _arr(spec_cpu, np.uint64), _arr(spec_mem, np.int64), _arr(replicas, np.int64)
        K = sc.size
        if sm.shape != (K,) or rep.shape != (K,):
            raise ValueError("plan arrays differ in length")
        ax = _arr(np.zeros((0, n)) if alloc_x is None else alloc_x, np.int64)
        ux = np.array(np.zeros((0, n)) if used_x is None else used_x, dtype=np.int64, order="C",
                      copy=True)
        sx = _arr(np.zeros((0, K)) if spec_x is None else spec_x, np.int64)
        if ax.ndim != 2 or ux.shape != ax.shape or ax.shape[1] != n:
            raise ValueError("alloc_x and used_x must both be [R, N]")
        R = ax.shape[0]
        if sx.shape != (R, K):
            raise ValueError("spec_x must be [R, K]")
        cap = None if node_cap is None else _arr(node_cap, np.int64)
        if cap is not None and cap.shape != (K,):
            raise ValueError("node_cap must be [K]")
        G = int(n_groups)
        el = None
        if eligible is not None:
            m = np.asarray(eligible, bool)
            if m.shape == (G,):
                m = np.broadcast_to(m[:, None], (G, K))
            if m.shape != (G, K):
                raise ValueError("eligible must be [G, K] or [G]")
            el = _arr(m, np.uint8)
        placed = np.zeros(K, np.int64)
        nodes_used = np.zeros(K, np.int64)
        err = np.zeros(K, np.int32)
        rows = np.zeros((K, n), np.int64) if want_rows else None
        self._check(self._lib.kcc_deploy(
            self._h, n, *[_p(x) for x in a], R, _p(ax), _p(st[0]), _p(st[1]), _p(st[2]), _p(ux),
            _p(group), G, _p(el), K, _p(sc), _p(sm), _p(sx), _p(rep), _p(cap), int(policy),
            _p(placed), _p(nodes_used), _p(err), _p(rows)))
        return DeployResult(placed, nodes_used, err, st[0], st[1], st[2], ux, rows)

    def deploy_async(self, alloc_cpu, alloc_mem, alloc_pods, n_ext, alloc_x, pod_count, used_cpu,
                     used_mem, used_x, group, n_groups, eligible, spec_cpu, spec_mem, spec_x,
                     replicas, node_cap, policy, placed, nodes_used, step_err, placed_rows=None,
                     stream=None):
        """Device form of deploy (torch tensors on the engine's device): pod_count, used_cpu,
        used_mem and used_x (n_ext * N, resource-major) are updated in place; eligible uint8 of
        n_groups * K elements; placed / nodes_used int64 [K], step_err int32 [K], placed_rows
        int64 of K * N elements or None.  Only enqueues on `stream`: it can be captured into
        one graph with the fit_*_async call that follows it.  The arguments go to the C-ABI
        as they are (None: NULL), which validates them."""
        n = 0 if alloc_cpu is None else alloc_cpu.numel()
        k = 0 if spec_cpu is None else spec_cpu.numel()
        self._check(self._lib.kcc_deploy_async(
            self._h, n, _dp(alloc_cpu), _dp(alloc_mem), _dp(alloc_pods), int(n_ext), _dp(alloc_x),
            _dp(pod_count), _dp(used_cpu), _dp(used_mem), _dp(used_x), _dp(group), int(n_groups),
            _dp(eligible), k, _dp(spec_cpu), _dp(spec_mem), _dp(spec_x), _dp(replicas),
            _dp(node_cap), int(policy), _dp(placed), _dp(nodes_used), _dp(step_err),
            _dp(placed_rows), _stream(stream)))

    # -- drain what-if: the pods of drained rows re-placed (opt-in) -------
    def drain(self, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem, drain,
              node_pod_ptr, pod_cpu, pod_mem, policy=_lib.KCC_DEPLOY_SPREAD, alloc_x=None,
              used_x=None, pod_x=None, pod_movable=None,
              max_shapes=_lib.KCC_DRAIN_MAX_SHAPES) -> "DrainResult":
        """Rows with drain[i] != 0 go away: their state is left full (used = allocatable, so
        every fit gives them 0), and the movable pods that ran on them (pods grouped by node,
        node_pod_ptr [N + 1]; pod_movable None: all) are bucketed by request shape (pod_cpu,
        pod_mem, pod_x[:, p]) and placed on the other rows, one deploy step per shape, biggest
        shape first, under `policy`.  More than max_shapes distinct shapes: shapes = -1, nothing
        placed.  The inputs are not modified: the result carries the updated state."""
        a = [_arr(x, t) for x, t in zip((alloc_cpu, alloc_mem, alloc_pods),
                                        (np.uint64, np.int64, np.int64))]
        st = [np.array(x, dtype=t, order="C", copy=True)
              for x, t in zip((pod_count, used_cpu, used_mem), (np.int64, np.uint64, np.int64))]
        n = a[0].size
        dr = _arr(np.asarray(drain) != 0, np.uint8)
        if any(x.shape != (n,) for x in a + st + [dr]):
            raise ValueError("node arrays differ in length")
        pc, pm = _arr(pod_cpu, np.uint64), _arr(pod_mem, np.int64)
        P = pc.size
        if pc.shape != (P,) or pm.shape != (P,):
            raise ValueError("pod arrays differ in length")
        ptr = _arr(node_pod_ptr, np.int64)
        if n > 0 and ptr.shape != (n + 1,):
            raise ValueError("node_pod_ptr must be [N + 1]")
        ax = _arr(np.zeros((0, n)) if alloc_x is None else alloc_x, np.int64)
        ux = np.array(np.zeros((0, n)) if used_x is None else used_x, dtype=np.int64, order="C",
                      copy=True)
        if ax.ndim != 2 or ux.shape != ax.shape or ax.shape[1] != n:
            raise ValueError("alloc_x and used_x must both be [R, N]")
        R = ax.shape[0]
        px = None if pod_x is None else _arr(pod_x, np.int64)
        if px is not None and px.shape != (R, P):
            raise ValueError("pod_x must be [R, P]")
        mv = None if pod_movable is None else _arr(np.asarray(pod_movable) != 0, np.uint8)
        if mv is not None and mv.shape != (P,):
            raise ValueError("pod_movable must be [P]")
        M = int(max_shapes)
        m = max(M, 0)
        summary = np.zeros(_lib.KCC_DRAIN_SUMMARY, np.int64)
        s_cpu = np.zeros(m, np.uint64)
        s_mem, s_cnt, s_pl, s_nd = (np.zeros(m, np.int64) for _ in range(4))
        s_x = np.zeros((R, m), np.int64)
        s_err = np.zeros(m, np.int32)
        self._check(self._lib.kcc_drain(
            self._h, n, *[_p(x) for x in a], R, _p(ax), _p(st[0]), _p(st[1]), _p(st[2]), _p(ux),
            _p(dr), P, _p(ptr), _p(pc), _p(pm), _p(px), _p(mv), int(policy), M, _p(summary),
            _p(s_cpu), _p(s_mem), _p(s_x), _p(s_cnt), _p(s_pl), _p(s_nd), _p(s_err)))
        D = max(int(summary[2]), 0)
        return DrainResult(int(summary[0]), int(summary[1]), int(summary[2]), int(summary[3]),
                           s_cpu[:D].copy(), s_mem[:D].copy(), s_x[:, :D].copy(), s_cnt[:D].copy(),
                           s_pl[:D].copy(), s_nd[:D].copy(), s_err[:D].copy(), st[0], st[1], st[2],
                           ux)

    def drain_async(self, alloc_cpu, alloc_mem, alloc_pods, n_ext, alloc_x, pod_count, used_cpu,
                    used_mem, used_x, drain, node_pod_ptr, pod_cpu, pod_mem, pod_x, pod_movable,
                    policy, max_shapes, summary, shape_cpu, shape_mem, shape_x, shape_count,
                    shape_placed, shape_nodes, shape_err, stream=None):
        """Device form of drain (torch tensors on the engine's device): pod_count, used_cpu,
        used_mem and used_x (n_ext * N, resource-major) are updated in place; drain and
        pod_movable uint8; summary int64 [4]; the shape arrays int64 [max_shapes] (shape_x
        n_ext * max_shapes, shape_err int32), untrimmed: entries behind summary[2] are 0.  Only
        enqueues on `stream`, max_shapes deploy steps whatever the pods hold: it can be captured
        into one graph with the fit_*_async call that follows it.  The arguments go to the
        C-ABI as they are (None: NULL), which validates them."""
        n = 0 if alloc_cpu is None else alloc_cpu.numel()
        p = 0 if pod_cpu is None else pod_cpu.numel()
        self._check(self._lib.kcc_drain_async(
            self._h, n, _dp(alloc_cpu), _dp(alloc_mem), _dp(alloc_pods), int(n_ext), _dp(alloc_x),
            _dp(pod_count), _dp(used_cpu), _dp(used_mem), _dp(used_x), _dp(drain), p,
            _dp(node_pod_ptr), _dp(pod_cpu), _dp(pod_mem), _dp(pod_x), _dp(pod_movable),
            int(policy), int(max_shapes), _dp(summary), _dp(shape_cpu), _dp(shape_mem),
            _dp(shape_x), _dp(shape_count), _dp(shape_placed), _dp(shape_nodes), _dp(shape_err),
            _stream(stream)))

    # -- removal what-if: each candidate row's pods re-placed on the rest (opt-in; DESIGN.md
    # §4.16) ---------------------------------------------------------------------------------
    def consolidate(self, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem, cand,
                    node_pod_ptr, pod_cpu, pod_mem, alloc_x=None, used_x=None, pod_x=None,
                    pod_movable=None, target=None, want_targets=True) -> "ConsolidateResult":
        """For each row of `cand`, on its own: do the movable pods that run there (pods grouped
        by node, node_pod_ptr [N + 1]; pod_movable None: all) fit on the other rows as they
        stand (target None: every row may receive pods)?  Each pod goes to the first row in row
        order that holds it, as a kcc_deploy step of one replica would place it; a candidate
        sees only its own placements.  The state is read, never written."""
        a = [_arr(x, t) for x, t in zip((alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu,
                                         used_mem),
                                        (np.uint64, np.int64, np.int64, np.int64, np.uint64,
                                         np.int64))]
        n = a[0].size
        if any(x.shape != (n,) for x in a):
            raise ValueError("node arrays differ in length")
        pc, pm = _arr(pod_cpu, np.uint64), _arr(pod_mem, np.int64)
        P = pc.size
        if pc.shape != (P,) or pm.shape != (P,):
            raise ValueError("pod arrays differ in length")
        ptr = _arr(node_pod_ptr, np.int64)
        if n > 0 and ptr.shape != (n + 1,):
            raise ValueError("node_pod_ptr must be [N + 1]")
        ax = _arr(np.zeros((0, n)) if alloc_x is None else alloc_x, np.int64)
        ux = _arr(np.zeros((0, n)) if used_x is None else used_x, np.int64)
        if ax.ndim != 2 or ux.shape != ax.shape or ax.shape[1] != n:
            raise ValueError("alloc_x and used_x must both be [R, N]")
        R = ax.shape[0]
        px = None if pod_x is None else _arr(pod_x, np.int64)
        if px is not None and px.shape != (R, P):
            raise ValueError("pod_x must be [R, P]")
        mv = None if pod_movable is None else _arr(np.asarray(pod_movable) != 0, np.uint8)
        if mv is not None and mv.shape != (P,):
            raise ValueError("pod_movable must be [P]")
        tg = None if target is None else _arr(np.asarray(target) != 0, np.uint8)
        if tg is not None and tg.shape != (n,):
            raise ValueError("target must be [N]")
        cd = _arr(cand, np.int64)
        if cd.ndim != 1:
            raise ValueError("cand must be one-dimensional")
        C_ = cd.size
        ev, pl, ze = (np.zeros(C_, np.int64) for _ in range(3))
        er = np.zeros(C_, np.int32)
        tgt = np.zeros(P, np.int64) if want_targets else None
        self._check(self._lib.kcc_consolidate(
            self._h, n, _p(a[0]), _p(a[1]), _p(a[2]), R, _p(ax), _p(a[3]), _p(a[4]), _p(a[5]),
            _p(ux), _p(tg), P, _p(ptr), _p(pc), _p(pm), _p(px), _p(mv), C_, _p(cd), _p(ev),
            _p(pl), _p(ze), _p(er), _p(tgt)))
        return ConsolidateResult(ev, pl, ze, er, tgt)

    def consolidate_async(self, alloc_cpu, alloc_mem, alloc_pods, n_ext, alloc_x, pod_count,
                          used_cpu, used_mem, used_x, target, node_pod_ptr, pod_cpu, pod_mem,
                          pod_x, pod_movable, cand, cand_evicted, cand_placed, cand_zero,
                          cand_err, pod_target, stream=None):
        """Device form of consolidate (torch tensors on the engine's device): target and
        pod_movable uint8 (or None), cand and the three counts int64 [C], cand_err int32 [C],
        pod_target int64 [P] (or None).  Only enqueues on `stream`, the same launches whatever
        the arrays hold: it can be captured into a graph.  The arguments go to the C-ABI as
        they are (None: NULL), which validates them."""
        n = 0 if alloc_cpu is None else alloc_cpu.numel()
        p = 0 if pod_cpu is None else pod_cpu.numel()
        c = 0 if cand is None else cand.numel()
        self._check(self._lib.kcc_consolidate_async(
            self._h, n, _dp(alloc_cpu), _dp(alloc_mem), _dp(alloc_pods), int(n_ext), _dp(alloc_x),
            _dp(pod_count), _dp(used_cpu), _dp(used_mem), _dp(used_x), _dp(target), p,
            _dp(node_pod_ptr), _dp(pod_cpu), _dp(pod_mem), _dp(pod_x), _dp(pod_movable), c,
            _dp(cand), _dp(cand_evicted), _dp(cand_placed), _dp(cand_zero), _dp(cand_err),
            _dp(pod_target), _stream(stream)))

    def capacity(self, node_ptr, cpu_req, mem_req, alloc_cpu, alloc_mem, alloc_pods, pod_count,
                 spec_cpu, spec_mem):
        """Fused (a)+(b) on host arrays.  Returns (totals, spec_err)."""
        node_ptr = _arr(node_ptr, np.int64)
        n = node_ptr.size - 1
        cpu_req, mem_req = _arr(cpu_req, np.uint64), _arr(mem_req, np.int64)
        a = [_arr(alloc_cpu, np.uint64), _arr(alloc_mem, np.int64), _arr(alloc_pods, np.int64),
             _arr(pod_count, np.int64)]
        if any(x.size != n for x in a):
            raise ValueError("node arrays differ in length")
        if cpu_req.size != mem_req.size:
            raise ValueError("container arrays differ in length")
        sc, sm = _arr(spec_cpu, np.uint64), _arr(spec_mem, np.int64)
        totals = np.zeros(sc.size, np.int64)
        err = np.zeros(sc.size, np.int32)
        self._check(self._lib.kcc_capacity(
            self._h, n, cpu_req.size, _p(node_ptr), _p(cpu_req), _p(mem_req),
            *[_p(x) for x in a], sc.size, _p(sc), _p(sm), _p(totals), _p(err)))
        return totals, err

    # -- list-order containers ---------------------------------
    def get_pod_cpu_memory_requests_limits_keyed(self, n_keys, key, cpu_req, mem_req,
                                                 cpu_lim=None, mem_lim=None) -> RequestSums:
        """CC:255-299 for every row at once from containers in list order: key[i] is the
        row of container i's node (<0 or >= n_keys: not on a listed row)."""
        key = _key32(key)
        cpu_req, mem_req = _arr(cpu_req, np.uint64), _arr(mem_req, np.int64)
        lim = cpu_lim is not None or mem_lim is not None
        if lim and (cpu_lim is None or mem_lim is None):
            raise ValueError("pass both cpu_lim and mem_lim, or neither")
        cpu_lim = _arr(cpu_lim, np.uint64) if lim else None
        mem_lim = _arr(mem_lim, np.int64) if lim else None
        nc = key.size
        if cpu_req.size != nc or mem_req.size != nc or (lim and (cpu_lim.size != nc or
                                                                 mem_lim.size != nc)):
            raise ValueError("container arrays differ in length")
        used_cpu, used_mem = np.zeros(n_keys, np.uint64), np.zeros(n_keys, np.int64)
        lim_cpu = np.zeros(n_keys, np.uint64) if lim else None
        lim_mem = np.zeros(n_keys, np.int64) if lim else None
        self._check(self._lib.kcc_reduce_requests_keyed(
            self._h, n_keys, nc, _p(key), _p(cpu_req), _p(mem_req), _p(cpu_lim), _p(mem_lim),
            _p(used_cpu), _p(used_mem), _p(lim_cpu), _p(lim_mem)))
        return RequestSums(lim_cpu, used_cpu, lim_mem, used_mem)

    def count_by_key(self, n_keys, key):
        """len(pods) per row (CC:106, CC:135) from the pods' row keys."""
        key = _key32(key)
        count = np.zeros(n_keys, np.int64)
        self._check(self._lib.kcc_count_by_key(self._h, n_keys, key.size, _p(key), _p(count)))
        return count

    def reduce_requests_keyed_async(self, n_keys, key, cpu_req, mem_req, used_cpu, used_mem,
                                    stream=None, cpu_lim=None, mem_lim=None, lim_cpu=None,
                                    lim_mem=None, n=None):
        """Device form of get_pod_cpu_memory_requests_limits_keyed (torch tensors on the
        engine's device, 16-byte aligned; outputs of n_keys elements, every row written).
        The arguments go to the C-ABI as they are (None: NULL), which validates them; n:
        the container count when it is not key.numel()."""
        n = (0 if key is None else key.numel()) if n is None else n
        self._check(self._lib.kcc_reduce_requests_keyed_async(
            self._h, n_keys, n, _dp(key), _dp(cpu_req), _dp(mem_req), _dp(cpu_lim), _dp(mem_lim),
            _dp(used_cpu), _dp(used_mem), _dp(lim_cpu), _dp(lim_mem), _stream(stream)))

    def count_by_key_async(self, n_keys, key, count, stream=None, n=None):
        """Device form of count_by_key: count[0:n_keys] (int64) = pods per row."""
        n = (0 if key is None else key.numel()) if n is None else n
        self._check(self._lib.kcc_count_by_key_async(
            self._h, n_keys, n, _dp(key), _dp(count), _stream(stream)))

    def pod_requests_async(self, pod_ptr, cpu_req, mem_req, pod_cpu, pod_mem, init_ptr=None,
                           init_cpu=None, init_mem=None, restartable=None, ovh_cpu=None,
                           ovh_mem=None, stream=None):
        """Device form of pod_requests (torch tensors; SURVEY §8f row 4, opt-in)."""
        n_init = 0 if init_cpu is None else init_cpu.numel()
        self._check(self._lib.kcc_pod_requests_async(
            self._h, pod_ptr.numel() - 1, cpu_req.numel(), n_init, _dp(pod_ptr), _dp(cpu_req),
            _dp(mem_req), _dp(init_ptr), _dp(init_cpu), _dp(init_mem), _dp(restartable),
            _dp(ovh_cpu), _dp(ovh_mem), _dp(pod_cpu), _dp(pod_mem), _stream(stream)))

    # -- quantity strings -------------------------------------
    def _parse(self, fn, strings, dtype):
        if isinstance(strings, tuple):
            buf, off = strings
        else:
            from .quantity import pack_strings
            buf, off = pack_strings(strings)
        buf = _arr(buf, np.uint8)
        off = _arr(off, np.int64)
        n = off.size - 1
        if n < 0:
            raise ValueError("offsets must hold n + 1 entries")
        out = np.zeros(n, dtype)
        st = np.zeros(n, np.int8)
        self._check(fn(self._h, n, _p(buf), buf.size, _p(off), _p(out), _p(st)))
        return out, st

    def convert_cpu_to_milis(self, strings):
        """convertCPUToMilis (CC:301-319) over a batch: `strings` is a sequence of str or
        a packed (bytes uint8, offsets int64) pair.  Returns (uint64 values, int8
        status: 1 ok, 0 where the reference prints an error and uses 0)."""
        return self._parse(self._lib.kcc_parse_cpu_millis, strings, np.uint64)

    def to_bytes(self, strings):
        """bytefmt.ToBytes (BF:75-105) over a batch.  Returns (int64 values, int8
        status: 1 ok, 0 error (value 0), -1 outside the device's exact ParseFloat
        domain — see include/kcc.h)."""
        return self._parse(self._lib.kcc_parse_bytes, strings, np.int64)

    def max_replicas_per_row(self, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu,
                             used_mem, spec_cpu: int, spec_mem: int):
        """CC:119-137 per node row for one spec ("Max replicas" of the verbose report).
        Returns (q int64[N], row_err int32[N]: 1 where Go would panic at that row)."""
        a = [_arr(alloc_cpu, np.uint64), _arr(alloc_mem, np.int64), _arr(alloc_pods, np.int64),
             _arr(pod_count, np.int64), _arr(used_cpu, np.uint64), _arr(used_mem, np.int64)]
        n = a[0].size
        if any(x.size != n for x in a):
            raise ValueError("node arrays differ in length")
        q = np.zeros(n, np.int64)
        err = np.zeros(n, np.int32)
        self._check(self._lib.kcc_fit_rows(self._h, n, *[_p(x) for x in a],
                                           int(spec_cpu) % (1 << 64), int(spec_mem), _p(q),
                                           _p(err)))
        return q, err

    @staticmethod
    def _pod_args(pod_ptr, cpu_req, mem_req, init_ptr, init_cpu, init_mem, restartable,
                  ovh_cpu, ovh_mem):
        pp = _arr(pod_ptr, np.int64)
        if pp.size < 1:
            raise ValueError("pod_ptr needs n_pods + 1 entries")
        n_pods = pp.size - 1
        cr, mr = _arr(cpu_req, np.uint64), _arr(mem_req, np.int64)
        if cr.size != mr.size:
            raise ValueError("container arrays differ in length")
        ip = ic = im = rs = None
        n_init = 0
        if init_ptr is not None:
            ip, ic, im = _arr(init_ptr, np.int64), _arr(init_cpu, np.uint64), _arr(init_mem, np.int64)
            if ip.size != n_pods + 1 or ic.size != im.size:
                raise ValueError("init arrays do not match pod_ptr")
            n_init = ic.size
            if restartable is not None:
                rs = _arr(restartable, np.uint8)
                if rs.size != n_init:
                    raise ValueError("restartable differs in length from the init arrays")
        elif restartable is not None or init_cpu is not None or init_mem is not None:
            raise ValueError("init container arrays without init_ptr")
        oc = None if ovh_cpu is None else _arr(ovh_cpu, np.uint64)
        om = None if ovh_mem is None else _arr(ovh_mem, np.int64)
        for o in (oc, om):
            if o is not None and o.size != n_pods:
                raise ValueError("overhead arrays need one entry per pod")
        return n_pods, cr.size, n_init, [pp, cr, mr, ip, ic, im, rs, oc, om]

    def pod_requests(self, pod_ptr, cpu_req, mem_req, init_ptr=None, init_cpu=None,
                     init_mem=None, restartable=None, ovh_cpu=None, ovh_mem=None):
        """OPT-IN scheduler request model (NOT the reference, which sums
        app containers only, CC:276-294): per pod max(app sum, init max incl. sidecars) +
        overhead — see include/kcc.h.  Returns (uint64 cpu[P], int64 mem[P])."""
        n_pods, n_cont, n_init, a = self._pod_args(pod_ptr, cpu_req, mem_req, init_ptr,
                                                   init_cpu, init_mem, restartable, ovh_cpu,
                                                   ovh_mem)
        pc, pm = np.zeros(n_pods, np.uint64), np.zeros(n_pods, np.int64)
        self._check(self._lib.kcc_pod_requests(self._h, n_pods, n_cont, n_init,
                                               *[_p(x) for x in a], _p(pc), _p(pm)))
        return pc, pm

    def reduce_requests_pods(self, node_pod_ptr, pod_ptr, cpu_req, mem_req, init_ptr=None,
                             init_cpu=None, init_mem=None, restartable=None, ovh_cpu=None,
                             ovh_mem=None):
        """Per-node sums of the opt-in pod requests (pods grouped by node, CSR
        node_pod_ptr[N+1]): the used_cpu / used_mem kcc_fit takes."""
        npp = _arr(node_pod_ptr, np.int64)
        if npp.size < 1:
            raise ValueError("node_pod_ptr needs n_nodes + 1 entries")
        n_nodes = npp.size - 1
        n_pods, n_cont, n_init, a = self._pod_args(pod_ptr, cpu_req, mem_req, init_ptr,
                                                   init_cpu, init_mem, restartable, ovh_cpu,
                                                   ovh_mem)
        uc, um = np.zeros(n_nodes, np.uint64), np.zeros(n_nodes, np.int64)
        self._check(self._lib.kcc_reduce_requests_pods(self._h, n_nodes, n_pods, n_cont, n_init,
                                                       _p(npp), *[_p(x) for x in a], _p(uc),
                                                       _p(um)))
        return uc, um

    # -- preemption what-if (opt-in; include/kcc.h) ------------------
    def reduce_requests_levels(self, node_pod_ptr, pod_ptr, cpu_req, mem_req, pod_level,
                               n_levels):
        """Per-node sums per priority level in one pass over the containers (pods grouped by
        node, CSR node_pod_ptr[N+1]; containers by pod, pod_ptr[P+1]; pod_level uint8 [P], a
        level >= n_levels counts as n_levels - 1).  Plane l holds the pods a spec of level l
        cannot evict (pod_level >= l); plane 0 is every pod.  An upper bound: every
        lower-priority pod yields (no PodDisruptionBudgets, no preemptionPolicy).  Opt-in, not
        the reference's arithmetic.  Returns (used_cpu uint64, used_mem int64, pod_count int64),
        each [n_levels, N]."""
        npp, pp = _arr(node_pod_ptr, np.int64), _arr(pod_ptr, np.int64)
        if npp.size < 1 or pp.size < 1:
            raise ValueError("node_pod_ptr / pod_ptr need n + 1 entries")
        n, P = npp.size - 1, pp.size - 1
        cr, mr = _arr(cpu_req, np.uint64), _arr(mem_req, np.int64)
        lv = _arr(pod_level, np.uint8)
        if cr.size != mr.size:
            raise ValueError("container arrays differ in length")
        if lv.size != P:
            raise ValueError("pod_level needs one entry per pod")
        L = int(n_levels)
        shape = (max(L, 0), n)
        uc, um, pc = np.zeros(shape, np.uint64), np.zeros(shape, np.int64), np.zeros(shape, np.int64)
        self._check(self._lib.kcc_reduce_requests_levels(
            self._h, n, P, cr.size, _p(npp), _p(pp), _p(cr), _p(mr), _p(lv), L, _p(uc), _p(um),
            _p(pc)))
        return uc, um, pc

    def reduce_requests_levels_async(self, node_pod_ptr, pod_ptr, cpu_req, mem_req, pod_level,
                                     n_levels, used_cpu, used_mem, pod_count, stream=None):
        """Device form of reduce_requests_levels (torch tensors on the engine's device; the
        outputs hold n_levels * N elements, plane-major).  Offsets are clamped on the device."""
        self._check(self._lib.kcc_reduce_requests_levels_async(
            self._h, node_pod_ptr.numel() - 1, pod_ptr.numel() - 1,
            0 if cpu_req is None else cpu_req.numel(), _dp(node_pod_ptr), _dp(pod_ptr),
            _dp(cpu_req), _dp(mem_req), _dp(pod_level), int(n_levels), _dp(used_cpu),
            _dp(used_mem), _dp(pod_count), _stream(stream)))

    def fit_levels(self, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
                   alloc_x, used_x, spec_cpu, spec_mem, spec_x, spec_level=None, group=None,
                   n_groups=1, node_cap=None, level_ptr=None):
        """fit_capped with node state that depends on the spec's priority level: pod_count,
        used_cpu and used_mem are [L, N] planes (reduce_requests_levels'), used_x [L, R, N] or
        one [R, N] block for every level, and spec s is fitted on plane spec_level[s].  The
        specs come in any order: they are sorted stably by level for the call and the outputs
        returned in the caller's order (level_ptr [L + 1] instead of spec_level: the specs are
        sorted already).  The intended use passes a spec twice, at level 0 and at its own
        level: "as things stand" beside "with preemption".  Returns (totals int64, err int32),
        [S] without group ids and [n_groups, S] with them."""
        pc, uc, um = _arr(pod_count, np.int64), _arr(used_cpu, np.uint64), _arr(used_mem, np.int64)
        if pc.ndim != 2 or uc.shape != pc.shape or um.shape != pc.shape:
            raise ValueError("pod_count, used_cpu and used_mem must all be [L, N]")
        L, n = pc.shape
        sc = _arr(spec_cpu, np.uint64)
        S = sc.size
        if (spec_level is None) == (level_ptr is None):
            raise ValueError("pass spec_level or level_ptr")
        if level_ptr is None:
            lv = _arr(spec_level, np.int64)
            if lv.shape != (S,) or (S and (lv.min() < 0 or lv.max() >= L)):
                raise ValueError("spec_level must be [S] with values in [0, L)")
            order = np.argsort(lv, kind="stable")
            lp = np.concatenate([[0], np.cumsum(np.bincount(lv, minlength=L))]).astype(np.int64)
        else:
            order = np.arange(S)
            lp = _arr(level_ptr, np.int64)
            if lp.shape != (L + 1,):
                raise ValueError("level_ptr must be [L + 1]")
        ux = None if used_x is None else _arr(used_x, np.int64)
        if ux is not None and ux.ndim == 2:
            ux = np.ascontiguousarray(np.broadcast_to(ux, (L,) + ux.shape))
        if ux is not None and (ux.ndim != 3 or ux.shape[0] != L):
            raise ValueError("used_x must be [R, N] or [L, R, N]")
        sx = None if spec_x is None else _arr(spec_x, np.int64)
        a, R, ax, _, group, G, sc, sm, sx, totals, err = self._cell_args(
            (alloc_cpu, alloc_mem, alloc_pods, pc[0] if L else np.zeros(n), uc[0] if L else np.zeros(n),
             um[0] if L else np.zeros(n)), sc[order], _arr(spec_mem, np.int64)[order], group,
            n_groups, alloc_x, None if ux is None else ux[0],
            None if sx is None else (sx[:, order] if sx.ndim == 2 else sx))
        cap = None if node_cap is None else _arr(node_cap, np.int64)
        if cap is not None and cap.shape != (S,):
            raise ValueError("node_cap must be [S]")
        cap = None if cap is None else np.ascontiguousarray(cap[order])
        if ux is None:
            ux = np.zeros((L, 0, n), np.int64)
        self._check(self._lib.kcc_fit_levels(
            self._h, n, _p(a[0]), _p(a[1]), _p(a[2]), L, _p(pc), _p(uc), _p(um), R, _p(ax), _p(ux),
            _p(group), G, S, _p(sc), _p(sm), _p(sx), _p(cap), _p(lp), _p(totals), _p(err)))
        back_t, back_e = np.empty_like(totals), np.empty_like(err)
        back_t[:, order] = totals
        back_e[:, order] = err
        if group is None:
            return back_t[0], back_e[0]
        return back_t, back_e

    def fit_levels_async(self, alloc_cpu, alloc_mem, alloc_pods, n_levels, pod_count, used_cpu,
                         used_mem, n_ext, alloc_x, used_x, group, n_groups, spec_cpu, spec_mem,
                         spec_x, node_cap, level_ptr, totals, spec_err, stream=None):
        """Device form of fit_levels (torch tensors on the engine's device: pod_count / used_cpu
        / used_mem of n_levels * N elements, used_x of n_levels * n_ext * N, the rest as
        fit_capped_async's).  level_ptr is a HOST sequence of n_levels + 1 offsets into the
        specs, which are sorted by level.  The arguments go to the C-ABI as they are (None:
        NULL), which validates them."""
        n = 0 if alloc_cpu is None else alloc_cpu.numel()
        s = 0 if spec_cpu is None else spec_cpu.numel()
        lp = None if level_ptr is None else _arr(level_ptr, np.int64)
        if lp is not None and lp.size != int(n_levels) + 1 and 1 <= int(n_levels) <= _lib.KCC_LEVELS_MAX:
            raise ValueError("level_ptr must hold n_levels + 1 offsets")
        self._check(self._lib.kcc_fit_levels_async(
            self._h, n, _dp(alloc_cpu), _dp(alloc_mem), _dp(alloc_pods), int(n_levels),
            _dp(pod_count), _dp(used_cpu), _dp(used_mem), int(n_ext), _dp(alloc_x), _dp(used_x),
            _dp(group), int(n_groups), s, _dp(spec_cpu), _dp(spec_mem), _dp(spec_x),
            _dp(node_cap), _p(lp), _dp(totals), _dp(spec_err), _stream(stream)))

    def quantity_value(self, strings):
        """resource.Quantity.Value() of ParseQuantity (CC:285-286, parity unpinned: see
        include/kcc.h) over a batch.  Returns (int64 values, int8 status)."""
        return self._parse(self._lib.kcc_parse_quantity, strings, np.int64)

    def last_slow_fraction(self) -> float:
        return float(self._lib.kcc_last_slow_fraction(self._h))

    # -- device API (torch tensors, enqueue on `stream`) -------------------------
    def reduce_requests_async(self, node_ptr, cpu_req, mem_req, used_cpu, used_mem,
                              cpu_lim=None, mem_lim=None, lim_cpu=None, lim_mem=None,
                              stream=None):
        n = node_ptr.numel() - 1
        self._check(self._lib.kcc_reduce_requests_async(
            self._h, n, cpu_req.numel(), _dp(node_ptr), _dp(cpu_req), _dp(mem_req),
            _dp(cpu_lim), _dp(mem_lim), _dp(used_cpu), _dp(used_mem), _dp(lim_cpu),
            _dp(lim_mem), _stream(stream)))

    def fit_prepare_async(self, alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
                          spec_cpu, spec_mem, partial, stream=None):
        self._check(self._lib.kcc_fit_prepare_async(
            self._h, alloc_cpu.numel(), _dp(alloc_cpu), _dp(alloc_mem), _dp(alloc_pods),
            _dp(pod_count), _dp(used_cpu), _dp(used_mem), spec_cpu.numel(), _dp(spec_cpu),
            _dp(spec_mem), _dp(partial), _stream(stream)))

    def fit_run_async(self, n_nodes, n_specs, partial, stream=None):
        self._check(self._lib.kcc_fit_run_async(self._h, n_nodes, n_specs, _dp(partial),
                                                _stream(stream)))

    def fit_finalize_async(self, n_specs, partial, totals, spec_err, stream=None):
        self._check(self._lib.kcc_fit_finalize_async(self._h, n_specs, _dp(partial),
                                                     _dp(totals), _dp(spec_err),
                                                     _stream(stream)))

    def capacity_partial_async(self, h_node_ptr, node_ptr, cpu_req, mem_req, alloc_cpu,
                               alloc_mem, alloc_pods, pod_count, used_cpu, used_mem, spec_cpu,
                               spec_mem, partial, n_chunks=0, stream=None):
        """Pipelined reduce + fit partial (kcc_capacity_partial_async): h_node_ptr is the
        host copy (numpy int64) of node_ptr, used only to place the chunk boundaries."""
        h = None if h_node_ptr is None else np.ascontiguousarray(h_node_ptr, np.int64)
        if h is not None and h.size != node_ptr.numel():
            raise ValueError("h_node_ptr and node_ptr differ in length")
        self._check(self._lib.kcc_capacity_partial_async(
            self._h, node_ptr.numel() - 1, cpu_req.numel(), _p(h), _dp(node_ptr), _dp(cpu_req),
            _dp(mem_req), _dp(alloc_cpu), _dp(alloc_mem), _dp(alloc_pods), _dp(pod_count),
            _dp(used_cpu), _dp(used_mem), spec_cpu.numel(), _dp(spec_cpu), _dp(spec_mem),
            _dp(partial), int(n_chunks), _stream(stream)))

    def capacity_async(self, h_node_ptr, node_ptr, cpu_req, mem_req, alloc_cpu, alloc_mem,
                       alloc_pods, pod_count, used_cpu, used_mem, spec_cpu, spec_mem, totals,
                       spec_err, stream=None):
        """The whole one-device step (kcc_capacity_async): reduce + fit + clamp correction
        with the finalize fused into the last launch -> totals (int64) / spec_err (int32)."""
        h = None if h_node_ptr is None else np.ascontiguousarray(h_node_ptr, np.int64)
        self._check(self._lib.kcc_capacity_async(
            self._h, node_ptr.numel() - 1, cpu_req.numel(), _p(h), _dp(node_ptr), _dp(cpu_req),
            _dp(mem_req), _dp(alloc_cpu), _dp(alloc_mem), _dp(alloc_pods), _dp(pod_count),
            _dp(used_cpu), _dp(used_mem), spec_cpu.numel(), _dp(spec_cpu), _dp(spec_mem),
            _dp(totals), _dp(spec_err), _stream(stream)))

    def parse_cpu_millis_async(self, buf, off, out, status, stream=None):
        self._check(self._lib.kcc_parse_cpu_millis_async(
            self._h, off.numel() - 1, _dp(buf), buf.numel(), _dp(off), _dp(out), _dp(status),
            _stream(stream)))

    def parse_bytes_async(self, buf, off, out, status, stream=None):
        self._check(self._lib.kcc_parse_bytes_async(
            self._h, off.numel() - 1, _dp(buf), buf.numel(), _dp(off), _dp(out), _dp(status),
            _stream(stream)))

    def parse_quantity_async(self, buf, off, out, status, stream=None):
        self._check(self._lib.kcc_parse_quantity_async(
            self._h, off.numel() - 1, _dp(buf), buf.numel(), _dp(off), _dp(out), _dp(status),
            _stream(stream)))

    # -- node sharding ------------------------------------------------
    def set_node_shards(self, n_shards: int):
        """Host-array entry points: cut the nodes into this many contiguous shards
        (round-robin over the context's devices; 0 = one per device)."""
        self._check(self._lib.kcc_set_node_shards(self._h, int(n_shards)))

    @staticmethod
    def comm_unique_id() -> bytes:
        """Rank 0 of a one-process-per-GPU run: the RCCL id every rank passes to
        comm_init (opaque bytes, distributed by the caller)."""
        buf = C.create_string_buffer(COMM_ID_BYTES)
        rc = _lib.lib().kcc_comm_unique_id(C.cast(buf, C.c_void_p))  # (release build)
        if rc != 0:
            raise KccError(rc, "ncclGetUniqueId failed")
        return buf.raw

    def comm_init(self, uid: bytes, n_ranks: int, rank: int):
        """Join the ranks' RCCL communicator (collective: blocks until every rank joined)."""
        if len(uid) != COMM_ID_BYTES:
            raise ValueError(f"the id holds {COMM_ID_BYTES} bytes")
        buf = C.create_string_buffer(uid, COMM_ID_BYTES)
        self._check(self._lib.kcc_comm_init(self._h, C.cast(buf, C.c_void_p), n_ranks, rank))

    def allreduce_partial_async(self, n_specs, partial, stream=None):
        """RCCL all-reduce (sum, int64) of the 2*S partial vector, on `stream`."""
        self._check(self._lib.kcc_allreduce_partial_async(self._h, n_specs, _dp(partial),
                                                          _stream(stream)))

    def p2p_export(self, n_ranks: int, max_specs: int) -> bytes:
        """One-shot xGMI exchange, setup step 1: allocate this rank's mailbox and return
        its IPC handle (opaque bytes every rank must receive)."""
        buf = C.create_string_buffer(P2P_HANDLE_BYTES)
        self._check(self._lib.kcc_p2p_export(self._h, int(n_ranks), int(max_specs),
                                             C.cast(buf, C.c_void_p)))
        return buf.raw

    def p2p_open(self, rank: int, handles):
        """Setup step 2: map every peer's mailbox (handles: every rank's export, by rank)."""
        blob = b"".join(handles)
        if len(blob) != P2P_HANDLE_BYTES * len(handles):
            raise ValueError(f"each handle holds {P2P_HANDLE_BYTES} bytes")
        buf = C.create_string_buffer(blob, len(blob))
        self._check(self._lib.kcc_p2p_open(self._h, int(rank), C.cast(buf, C.c_void_p)))

    def exchange_finalize_async(self, n_specs, partial, totals, spec_err, stream=None):
        """Each step: push this rank's partial to every peer's mailbox, wait for theirs,
        sum and finalize (replaces allreduce_partial_async + fit_finalize_async)."""
        self._check(self._lib.kcc_exchange_finalize_async(self._h, n_specs, _dp(partial),
                                                          _dp(totals), _dp(spec_err),
                                                          _stream(stream)))

    def p2p_faults(self) -> int:
        """Flag waits of the exchange that gave up (0 on a healthy run)."""
        v = C.c_int64()
        self._check(self._lib.kcc_p2p_faults(self._h, C.byref(v)))
        return v.value

    def profile_enable(self, on: bool = True):
        self._check(self._lib.kcc_profile_enable(self._h, 1 if on else 0))

    def profile_read(self):
        """(reduce_ms_total, reduce_launches, fit_ms_total, fit_launches) of the pipelined
        calls since profile_enable (synchronises)."""
        rm, rn, fm, fn = C.c_double(), C.c_int64(), C.c_double(), C.c_int64()
        self._check(self._lib.kcc_profile_read(self._h, C.byref(rm), C.byref(rn), C.byref(fm),
                                               C.byref(fn)))
        return rm.value, rn.value, fm.value, fn.value

    def set_fit_dense(self, dense: bool):
        """Stream every node row through the fit (diagnostic); default: only the rows
        that can add to its fast sum."""
        self._check(self._lib.kcc_set_fit_dense(self._h, 1 if dense else 0))

    def set_clamp_in_fit(self, mode: int):
        """-1: the pod-slot clamp inside the fit on small shards (default), 0: always the
        clamp correction launch, 1: inside the fit whenever specs <= 4096."""
        self._check(self._lib.kcc_set_clamp_in_fit(self._h, int(mode)))

    def clamp_in_fit_used(self) -> bool:
        """Whether the last capacity call applied the clamp inside the fit."""
        v = C.c_int()
        self._check(self._lib.kcc_clamp_in_fit_used(self._h, C.byref(v)))
        return bool(v.value)

    def fit_stream_rows(self) -> int:
        """Node rows (padded to groups of 8) the last fit streamed."""
        v = C.c_int64()
        self._check(self._lib.kcc_fit_stream_rows(self._h, C.byref(v)))
        return v.value

    def reduce_faults(self) -> int:
        """Look-back waits of the segmented reduce that gave up (0 on a healthy device)."""
        v = C.c_int64()
        self._check(self._lib.kcc_reduce_faults(self._h, C.byref(v)))
        return v.value

    def clear_faults(self):
        """Reset the device fault words and the reduce's look-back records."""
        self._check(self._lib.kcc_clear_faults(self._h))

    def fit_slow_pairs(self):
        a, b = C.c_int64(), C.c_int64()
        self._check(self._lib.kcc_fit_slow_pairs(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value


def _key32(key) -> np.ndarray:
    """Row keys as int32 (the C-ABI's type); wider keys must fit, never wrap silently."""
    k = np.asarray(key)
    if k.dtype != np.int32 and k.size and (k.max() > np.iinfo(np.int32).max or
                                           k.min() < np.iinfo(np.int32).min):
        raise ValueError("row keys must fit int32")
    return np.ascontiguousarray(k, np.int32)


def _stream(stream):
    if stream is None:
        return None
    h = getattr(stream, "cuda_stream", stream)
    return C.c_void_p(int(h)) if h else None


def select_groups(totals, err, eligible):
    """The reference run on the nodes of the eligible groups, from fit_grouped's cells (host
    arithmetic on G x S numbers).  eligible: bool [G, S] (per spec) or [G].  Returns
    (totals int64[S], err int32[S]): err[s] = 1 when an eligible cell of spec s is flagged
    (Go would panic on that sub-cluster), totals[s] = the wrapping sum of the eligible
    cells, 0 where err[s] is set."""
    t = np.asarray(totals, np.int64)
    e = np.asarray(err, np.int32)
    if t.ndim != 2 or e.shape != t.shape:
        raise ValueError("totals and err must both be [G, S]")
    m = np.asarray(eligible, bool)
    if m.shape == t.shape[:1]:
        m = np.broadcast_to(m[:, None], t.shape)
    if m.shape != t.shape:
        raise ValueError("eligible must be [G, S] or [G]")
    flagged = ((e != 0) & m).any(axis=0)
    # uint64 addition wraps as Go's int64 does
    s = np.where(m, t, 0).astype(np.int64).view(np.uint64).sum(axis=0, dtype=np.uint64)
    out = np.where(flagged, np.uint64(0), s).astype(np.uint64).view(np.int64)
    return out, flagged.astype(np.int32)


def explain_groups(res, eligible, group_rows=None):
    """fit_explain's cells folded over the eligible live groups, per plane (host arithmetic on
    G x S numbers, like select_groups, whose flag rule it uses).  res: a grouped ExplainResult;
    eligible: bool [G, S] or [G]; group_rows int64 [G] (None: every group is live; else the
    groups with no row are left out — their cells cannot flag a spec).  Returns an
    ExplainResult without the G axis: totals / err as select_groups gives them, every plane
    the wrapping sum of its eligible live cells, 0 where err[s] is set."""
    t = np.asarray(res.totals, np.int64)
    if t.ndim != 2:
        raise ValueError("res must hold [G, S] cells")
    m = np.asarray(eligible, bool)
    if m.shape == t.shape[:1]:
        m = np.broadcast_to(m[:, None], t.shape)
    if m.shape != t.shape:
        raise ValueError("eligible must be [G, S] or [G]")
    if group_rows is not None:
        gr = np.asarray(group_rows, np.int64)
        if gr.shape != t.shape[:1]:
            raise ValueError("group_rows must be [G]")
        m = m & (gr > 0)[:, None]
    totals, err = select_groups(t, res.err, m)

    def fold(planes):
        if planes is None:
            return None
        p = np.asarray(planes, np.int64)
        if p.ndim != 3 or p.shape[1:] != t.shape:
            raise ValueError("planes must be [K, G, S]")
        s = np.where(m[None], p, 0).astype(np.int64).view(np.uint64).sum(axis=1, dtype=np.uint64)
        return np.where((err != 0)[None], np.uint64(0), s).astype(np.uint64).view(np.int64)

    return ExplainResult(totals, err, fold(res.why_rows), fold(res.why_pods), fold(res.left))


def verdict(totals, replicas):
    """CC:144: `totalPossibleMaxReplicas >= replicas`, per spec."""
    return np.asarray(totals, np.int64) >= np.asarray(replicas, np.int64)
