"""Preemption what-if (kcc_reduce_requests_levels, kcc_fit_levels) restated
with numpy and the existing Python models.

TEST INFRASTRUCTURE ONLY (not a test module).  The reduce is vectorised (wrapping uint64 /
int64 prefix sums), so it takes the long-node cases; the fit is tests/ext_model.pair_table and
tests/spread_model.capped_cells per level, exactly as include/kcc.h states it: columns
[level_ptr[l], level_ptr[l+1]) are kcc_fit_capped on plane l.
"""
from __future__ import annotations

import numpy as np

from tests import ext_model as xm
from tests import spread_model as sm_


def _segment_sums(values, ptr):
    """The wrapping sum of values[ptr[i]:ptr[i+1]] for every i (empty segments: 0)."""
    ptr = np.asarray(ptr, np.int64)
    with np.errstate(over="ignore"):
        cs = np.concatenate([np.zeros(1, values.dtype), np.cumsum(values, dtype=values.dtype)])
        return cs[ptr[1:]] - cs[ptr[:-1]]


def reduce_levels(node_pod_ptr, pod_ptr, cpu_req, mem_req, pod_level, n_levels):
    """(used_cpu uint64, used_mem int64, pod_count int64), each [L, N]: plane l sums the pods
    with min(pod_level, L - 1) >= l; a pod without containers still counts."""
    L = int(n_levels)
    npp = np.asarray(node_pod_ptr, np.int64)
    N = npp.size - 1
    pod_c = _segment_sums(np.asarray(cpu_req, np.uint64), pod_ptr)
    pod_m = _segment_sums(np.asarray(mem_req, np.int64), pod_ptr)
    lv = np.minimum(np.asarray(pod_level, np.int64), L - 1)
    uc = np.zeros((L, N), np.uint64)
    um = np.zeros((L, N), np.int64)
    pc = np.zeros((L, N), np.int64)
    for l in range(L):
        keep = lv >= l
        uc[l] = _segment_sums(np.where(keep, pod_c, np.uint64(0)), npp)
        um[l] = _segment_sums(np.where(keep, pod_m, np.int64(0)), npp)
        pc[l] = _segment_sums(keep.astype(np.int64), npp)
    return uc, um, pc


def level_ptr_of(spec_level, n_levels):
    """(order, level_ptr): the stable sort of the specs by level and the offsets of the levels."""
    lv = np.asarray(spec_level, np.int64)
    order = np.argsort(lv, kind="stable")
    lp = np.concatenate([[0], np.cumsum(np.bincount(lv, minlength=int(n_levels)))]).astype(np.int64)
    return order, lp


def fit_levels(alloc3, pod_count, used_cpu, used_mem, alloc_x, used_x, spec_cpu, spec_mem, spec_x,
               level_ptr, group=None, n_groups=1, node_cap=None):
    """(totals int64 [G, S], err int32 [G, S]) for specs sorted by level.  alloc3: alloc_cpu,
    alloc_mem, alloc_pods; pod_count / used_cpu / used_mem [L, N]; used_x [L, R, N]."""
    L = pod_count.shape[0]
    S, G = len(spec_cpu), int(n_groups)
    totals = np.zeros((G, S), np.int64)
    err = np.zeros((G, S), np.int32)
    for l in range(L):
        lo, hi = int(level_ptr[l]), int(level_ptr[l + 1])
        if lo == hi:
            continue
        rows = list(alloc3) + [pod_count[l], used_cpu[l], used_mem[l]]
        q, dz = xm.pair_table(rows, alloc_x, used_x[l], spec_cpu[lo:hi], spec_mem[lo:hi],
                              spec_x[:, lo:hi])
        cap = None if node_cap is None else node_cap[lo:hi]
        t, e, _, _ = sm_.capped_cells(q, dz, group, G, cap)
        totals[:, lo:hi] = t
        err[:, lo:hi] = e
    return totals, err
