"""The removal what-if (kcc_consolidate) restated on tests/deploy_model.

TEST INFRASTRUCTURE ONLY (not a test module).  Per candidate ONE deploy call on the state as
passed in: K = the candidate's tried pods in order (evicted, with a cpu and a memory request),
spec = the pod's words, replicas = 1, KCC_DEPLOY_PACK, no cap; the ineligible rows (the
candidate itself, rows outside `target`) carry group id -1.  A pod's target is the row of its
step's Result.rows, each exactly as include/kcc.h states it.

  consolidate      on deploy_model.deploy: every input, small cases only
  consolidate_np   on deploy_model.deploy_np, for large N; valid only on plain inputs
                   (deploy_np's conditions, for the rows and for the pods)

Layouts as the C-ABI's: alloc_x / used_x are [R][N], pod_x is [R][P] (None: zeros).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import deploy_model as dm

MAX_PODS = 1024
OK, BADROW, TOOMANY = 0, 1, 2


@dataclass
class Result:
    evicted: np.ndarray     # int64 [C]
    placed: np.ndarray      # int64 [C]
    zero: np.ndarray        # int64 [C]
    err: np.ndarray         # int32 [C]
    pod_target: np.ndarray  # int64 [P]

    @property
    def removable(self):
        return (self.err == OK) & (self.placed == self.evicted)

    @property
    def removable_lenient(self):
        return (self.err == OK) & (self.placed + self.zero == self.evicted)


def _consolidate(deploy, rows, alloc_x, used_x, cand, node_pod_ptr, pod_cpu, pod_mem, pod_x,
                 pod_movable, target) -> Result:
    n, R, P = len(rows[0]), len(alloc_x), len(pod_cpu)
    C = len(cand)
    ax = np.array(alloc_x, np.int64).reshape(R, n)
    ux = np.array(used_x, np.int64).reshape(R, n)
    evicted, placed, zero = (np.zeros(C, np.int64) for _ in range(3))
    err = np.zeros(C, np.int32)
    tgt = np.full(P, -2, np.int64)
    for j, c in enumerate(int(v) for v in cand):
        if not 0 <= c < n:
            err[j] = BADROW
            continue
        ev = [p for p in range(int(node_pod_ptr[c]), int(node_pod_ptr[c + 1]))
              if pod_movable is None or pod_movable[p]]
        evicted[j] = len(ev)
        if len(ev) > MAX_PODS:
            err[j] = TOOMANY
            continue
        tried = []
        for p in ev:
            if int(pod_cpu[p]) == 0 or int(pod_mem[p]) == 0:
                zero[j] += 1
                tgt[p] = -3
            else:
                tried.append(p)
        if not tried:
            continue
        K = len(tried)
        group = np.zeros(n, np.int32)
        if target is not None:
            group[np.asarray(target) == 0] = -1
        group[c] = -1
        sc = np.array([int(pod_cpu[p]) for p in tried], np.uint64)
        sm = np.array([int(pod_mem[p]) for p in tried], np.int64)
        sx = np.array([[0 if pod_x is None else int(pod_x[r][p]) for p in tried]
                       for r in range(R)], np.int64).reshape(R, K)
        res = deploy(rows, ax, ux, sc, sm, sx, np.ones(K, np.int64), dm.PACK, group=group,
                     n_groups=1)
        assert not res.err.any() and res.placed.max() <= 1  # no zero request is tried
        placed[j] = int(res.placed.sum())
        for k, p in enumerate(tried):
            hit = np.flatnonzero(res.rows[k])
            assert hit.size == int(res.placed[k])
            tgt[p] = int(hit[0]) if hit.size else -1
    return Result(evicted, placed, zero, err, tgt)


def consolidate(rows, alloc_x, used_x, cand, node_pod_ptr, pod_cpu, pod_mem, pod_x=None,
                pod_movable=None, target=None) -> Result:
    """rows = (alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem) as the fits take
    them.  Nothing passed in is modified."""
    return _consolidate(dm.deploy, rows, alloc_x, used_x, cand, node_pod_ptr, pod_cpu, pod_mem,
                        pod_x, pod_movable, target)


def consolidate_np(rows, alloc_x, used_x, cand, node_pod_ptr, pod_cpu, pod_mem, pod_x=None,
                   pod_movable=None, target=None) -> Result:
    """consolidate() on deploy_np, for PLAIN inputs only (deploy_np's conditions: values in
    [0, 2^62), every tried pod's cpu and memory request >= 1, extra requests >= 0)."""
    return _consolidate(dm.deploy_np, rows, alloc_x, used_x, cand, node_pod_ptr, pod_cpu,
                        pod_mem, pod_x, pod_movable, target)
