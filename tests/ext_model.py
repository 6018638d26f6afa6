"""The extended-resource fit (kcc_fit_ext) restated in Python integers.

TEST INFRASTRUCTURE ONLY (not a test module).  Built on oracle.pyoracle's u64 / i64 /
go_div_i64 / find_min / fit_one: a row and spec with no requested extra resource go through
fit_one itself; otherwise the two reference quotients are restated as fit_one has them
(CC:119-130), each requested extra resource joins findMin as a second memory column, and
the pod-slot clamp (CC:134-136) follows all the mins.

Layouts as the C-ABI's: alloc_x / used_x are [R][N], spec_x is [R][S] (any nested sequence
or 2-D array).  Pure-Python loops: small cases only.
"""
from __future__ import annotations

import numpy as np

from oracle.pyoracle import find_min, fit_one, go_div_i64, i64, u64

FC_MAX = 1 << 31    # fast rows: free CPU below this
FX_MAX = 1 << 50    # fast rows: 0 <= free memory, free extra resource < this
SPEC_MAX = 1 << 52  # fast specs: c, m in [1, this]; x in {0} or [1, this]


def free_signed(alloc: int, used: int) -> int:
    """The memory column's free amount (CC:125): 0 where alloc <= used, else the wrapping
    int64 difference."""
    alloc, used = i64(alloc), i64(used)
    return 0 if alloc <= used else i64(alloc - used)


def free_cpu(alloc: int, used: int) -> int:
    alloc, used = u64(alloc), u64(used)
    return 0 if alloc <= used else alloc - used


def ext_quotient(alloc: int, used: int, x: int) -> int:
    """qx of one requested (x != 0) extra resource."""
    fx = free_signed(alloc, used)
    return 0 if fx == 0 else go_div_i64(fx, i64(x))


def fit_one_ext(alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem, alloc_x,
                used_x, spec_cpu, spec_mem, spec_x) -> int:
    """One row, one spec; alloc_x / used_x / spec_x are the R values of that row / spec.
    Raises ZeroDivisionError where Go panics (kcc_fit's rule: the extras never do)."""
    req = [r for r in range(len(spec_x)) if int(spec_x[r]) != 0]
    if not req:
        return fit_one(alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem,
                       spec_cpu, spec_mem)
    fc = free_cpu(alloc_cpu, used_cpu)
    if fc == 0:
        qc = 0
    else:
        if u64(spec_cpu) == 0:
            raise ZeroDivisionError("integer divide by zero")
        qc = i64(fc // u64(spec_cpu))  # int(uint64) reinterprets
    fm = free_signed(alloc_mem, used_mem)
    qm = 0 if fm == 0 else go_div_i64(fm, i64(spec_mem))  # raises on a zero request
    q = find_min(qc, qm)
    for r in req:
        q = find_min(q, ext_quotient(int(alloc_x[r]), int(used_x[r]), int(spec_x[r])))
    if q >= i64(alloc_pods):
        q = i64(alloc_pods - pod_count)
    return q


def pair_table(rows, alloc_x, used_x, spec_cpu, spec_mem, spec_x):
    """q of every (row, spec): (q int64 [N, S], panics bool [N, S])."""
    ac, am, ap, pc, uc, um = [[int(v) for v in a] for a in rows]
    ax = [[int(v) for v in col] for col in alloc_x]
    ux = [[int(v) for v in col] for col in used_x]
    sx = [[int(v) for v in col] for col in spec_x]
    n, S, R = len(ac), len(spec_cpu), len(ax)
    q = np.zeros((n, S), np.int64)
    dz = np.zeros((n, S), bool)
    for s in range(S):
        c, m = int(spec_cpu[s]), int(spec_mem[s])
        xs = [sx[r][s] for r in range(R)]
        for i in range(n):
            try:
                q[i, s] = fit_one_ext(ac[i], am[i], ap[i], pc[i], uc[i], um[i],
                                      [ax[r][i] for r in range(R)],
                                      [ux[r][i] for r in range(R)], c, m, xs)
            except ZeroDivisionError:
                dz[i, s] = True
    return q, dz


def totals_from_pairs(q, dz, group=None, n_groups=1):
    """The cells of kcc_fit_ext from pair_table's output: (totals int64, err int32) of
    shape [S] without group ids and [G, S] with them (ids outside [0, G) skipped; a cell
    with a panicking row is flagged and its total 0; the sums wrap)."""
    n, S = q.shape
    G = int(n_groups)
    gid = np.zeros(n, np.int64) if group is None else np.asarray(group, np.int64)
    tot = np.zeros((G, S), np.uint64)
    err = np.zeros((G, S), np.int32)
    qu = q.view(np.uint64)
    for g in np.unique(gid[(gid >= 0) & (gid < G)]):
        sel = gid == g
        tot[g] = qu[sel].sum(axis=0, dtype=np.uint64)  # wraps as Go's int64 does
        err[g] = dz[sel].any(axis=0)
    tot[err != 0] = 0
    tot = tot.view(np.int64)
    return (tot[0], err[0]) if group is None else (tot, err)


def fit_ext(rows, alloc_x, used_x, spec_cpu, spec_mem, spec_x, group=None, n_groups=1):
    q, dz = pair_table(rows, alloc_x, used_x, spec_cpu, spec_mem, spec_x)
    return totals_from_pairs(q, dz, group, n_groups)


def row_is_fast(alloc_cpu, alloc_mem, used_cpu, used_mem, alloc_x, used_x) -> bool:
    if not free_cpu(alloc_cpu, used_cpu) < FC_MAX:
        return False
    frees = [free_signed(alloc_mem, used_mem)]
    frees += [free_signed(int(a), int(u)) for a, u in zip(alloc_x, used_x)]
    return all(0 <= f < FX_MAX for f in frees)


def spec_is_fast(spec_cpu, spec_mem, spec_x) -> bool:
    return (1 <= u64(spec_cpu) <= SPEC_MAX and 1 <= i64(spec_mem) <= SPEC_MAX and
            all(i64(int(x)) == 0 or 1 <= i64(int(x)) <= SPEC_MAX for x in spec_x))
