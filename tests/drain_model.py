"""The drain what-if (kcc_drain) restated in Python integers.

TEST INFRASTRUCTURE ONLY (not a test module).  Built on tests/deploy_model: the evicted pods
(the movable pods of the drained rows) are bucketed by request shape in a dict, the shapes
sorted descending (cpu as uint64, every other word as int64), the drained rows left full, and
the shapes placed by ONE deploy call of K = D steps (spec = the shape, replicas = its count, no
cap, no groups), each exactly as include/kcc.h states it.

  drain      on deploy_model.deploy: every input, small cases only
  drain_np   on deploy_model.deploy_np, for large N; valid only on plain inputs (deploy_np's
             conditions, for the rows and for the pod shapes)

Layouts as the C-ABI's: alloc_x / used_x are [R][N], pod_x is [R][P] (None: zeros).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle.pyoracle import i64, u64
from tests import deploy_model as dm

PACK, SPREAD = dm.PACK, dm.SPREAD


@dataclass
class Result:
    drained_rows: int
    evicted: int
    shapes: int             # D, or -1 when D > max_shapes (nothing placed, the arrays empty)
    placed: int
    shape_cpu: np.ndarray   # uint64 [D]
    shape_mem: np.ndarray   # int64 [D]
    shape_x: np.ndarray     # int64 [R, D]
    shape_count: np.ndarray
    shape_placed: np.ndarray
    shape_nodes: np.ndarray
    shape_err: np.ndarray   # int32 [D]
    pod_count: np.ndarray   # int64 [N]
    used_cpu: np.ndarray    # uint64 [N]
    used_mem: np.ndarray    # int64 [N]
    used_x: np.ndarray      # int64 [R, N]

    @property
    def summary(self):
        return np.array([self.drained_rows, self.evicted, self.shapes, self.placed], np.int64)


def evicted_shapes(drain, node_pod_ptr, pod_cpu, pod_mem, pod_x, pod_movable, R):
    """(drained rows, evicted pods, {shape tuple: count}) — a shape is (cpu as uint64, memory,
    x[0..R)) in Python ints."""
    shapes: dict = {}
    rows = evicted = 0
    for i, d in enumerate(drain):
        if not d:
            continue
        rows += 1
        for p in range(int(node_pod_ptr[i]), int(node_pod_ptr[i + 1])):
            if pod_movable is not None and not pod_movable[p]:
                continue  # goes away with its node
            key = (u64(int(pod_cpu[p])), i64(int(pod_mem[p]))) + tuple(
                0 if pod_x is None else i64(int(pod_x[r][p])) for r in range(R))
            shapes[key] = shapes.get(key, 0) + 1
            evicted += 1
    return rows, evicted, shapes


def fill_drained(rows, alloc_x, used_x, drain):
    """The state with the drained rows left full: (pod_count, used_cpu, used_mem, used_x)."""
    ac, am, ap, pc, uc, um = rows
    d = np.asarray(drain) != 0
    R, n = len(alloc_x), len(ac)
    ax = np.array(alloc_x, np.int64).reshape(R, n)
    ux = np.array(used_x, np.int64).reshape(R, n).copy()
    pc = np.where(d, np.asarray(ap, np.int64), np.asarray(pc, np.int64))
    uc = np.where(d, np.asarray(ac, np.uint64), np.asarray(uc, np.uint64))
    um = np.where(d, np.asarray(am, np.int64), np.asarray(um, np.int64))
    ux[:, d] = ax[:, d]
    return pc, uc, um, ux


def _drain(deploy, rows, alloc_x, used_x, drain, node_pod_ptr, pod_cpu, pod_mem, pod_x,
           pod_movable, policy, max_shapes) -> Result:
    R, n = len(alloc_x), len(rows[0])
    n_rows, evicted, shapes = evicted_shapes(drain, node_pod_ptr, pod_cpu, pod_mem, pod_x,
                                             pod_movable, R)
    pc, uc, um, ux = fill_drained(rows, alloc_x, used_x, drain)
    order = sorted(shapes, reverse=True)  # tuples of (unsigned cpu, signed words): lexicographic
    D = len(order)
    if D > max_shapes:
        e64 = np.zeros(0, np.int64)
        return Result(n_rows, evicted, -1, 0, np.zeros(0, np.uint64), e64, np.zeros((R, 0), np.int64),
                      e64, e64, e64, np.zeros(0, np.int32), pc, uc, um, ux)
    sc = np.array([k[0] for k in order], np.uint64)
    sm = np.array([k[1] for k in order], np.int64)
    sx = np.array([[k[2 + r] for k in order] for r in range(R)], np.int64).reshape(R, D)
    cnt = np.array([shapes[k] for k in order], np.int64)
    state = [rows[0], rows[1], rows[2], pc, uc, um]
    res = deploy(state, np.array(alloc_x, np.int64).reshape(R, n), ux, sc, sm, sx, cnt, policy)
    return Result(n_rows, evicted, D, int(res.placed.sum()), sc, sm, sx, cnt, res.placed,
                  res.nodes_used, res.err, res.pod_count, res.used_cpu, res.used_mem, res.used_x)


def drain(rows, alloc_x, used_x, drain, node_pod_ptr, pod_cpu, pod_mem, pod_x=None,
          pod_movable=None, policy=SPREAD, max_shapes=4096) -> Result:
    """rows = (alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem) as the fits take
    them.  Nothing passed in is modified."""
    return _drain(dm.deploy, rows, alloc_x, used_x, drain, node_pod_ptr, pod_cpu, pod_mem, pod_x,
                  pod_movable, policy, max_shapes)


def drain_np(rows, alloc_x, used_x, drain, node_pod_ptr, pod_cpu, pod_mem, pod_x=None,
             pod_movable=None, policy=SPREAD, max_shapes=4096) -> Result:
    """drain() on deploy_np, for PLAIN inputs only (deploy_np's conditions: values in
    [0, 2^62), every evicted shape's cpu and memory request >= 1, extra requests >= 0)."""
    return _drain(dm.deploy_np, rows, alloc_x, used_x, drain, node_pod_ptr, pod_cpu, pod_mem,
                  pod_x, pod_movable, policy, max_shapes)
