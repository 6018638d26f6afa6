"""A rollout plan placed on the nodes (kcc_deploy) restated in Python
integers.

TEST INFRASTRUCTURE ONLY (not a test module).  Built on tests/ext_model.fit_one_ext (q of one
row and one spec, the pod-slot clamp after all the mins, ZeroDivisionError where Go panics):
per step the counts a_i, the placement p_i under KCC_DEPLOY_PACK or KCC_DEPLOY_SPREAD and the
commit to pod_count / used_cpu / used_mem / used_x, each exactly as include/kcc.h states it.

  deploy      pure-Python loops over Python integers: every input, small cases only
  deploy_np   numpy-vectorised, for large N; valid only on plain inputs (non-negative values,
              positive cpu and memory requests, nothing wraps, nothing panics); the CPU suite
              checks it against deploy at small N

Layouts as the C-ABI's: alloc_x / used_x are [R][N], spec_x is [R][K], eligible [G][K].
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle.pyoracle import i64, u64
from tests.ext_model import fit_one_ext

PACK, SPREAD = 0, 1
R_MAX = (1 << 31) - 1


@dataclass
class Result:
    placed: np.ndarray      # int64 [K]
    nodes_used: np.ndarray  # int64 [K]
    err: np.ndarray         # int32 [K]
    pod_count: np.ndarray   # int64 [N]
    used_cpu: np.ndarray    # uint64 [N]
    used_mem: np.ndarray    # int64 [N]
    used_x: np.ndarray      # int64 [R, N]
    rows: np.ndarray        # int64 [K, N]


def clamp_replicas(r: int) -> int:
    return min(max(int(r), 0), R_MAX)


def water_level(a, Rk: int) -> int:
    """The smallest t >= 1 with sum(min(a_i, t)) >= Rk (1 <= Rk <= sum(a))."""
    lo, hi = 1, max(a)  # f(hi) = sum(a) >= Rk
    while lo < hi:
        mid = (lo + hi) // 2
        if sum(min(v, mid) for v in a) >= Rk:
            hi = mid
        else:
            lo = mid + 1
    return lo


def place(a, Rk: int, policy: int):
    """p_i from the counts a_i (Python ints >= 0) and the clamped replica count."""
    T = sum(a)
    if Rk >= T:
        return list(a)
    if Rk == 0:
        return [0] * len(a)
    if policy == PACK:  # first fit in row order
        p, before = [], 0
        for v in a:
            p.append(min(v, max(0, Rk - before)))
            before += v
        return p
    t = water_level(a, Rk)
    p = [min(v, t - 1) for v in a]
    rem = Rk - sum(p)
    assert 1 <= rem <= sum(1 for v in a if v >= t)
    for i, v in enumerate(a):
        if rem and v >= t:
            p[i] += 1
            rem -= 1
    return p


def _eligibility(n, K, group, n_groups, eligible):
    """el[k][i]: row i is eligible for step k."""
    G = int(n_groups)
    gid = [0] * n if group is None else [int(g) for g in group]
    el = None
    if eligible is not None:
        el = np.asarray(eligible, bool)
        if el.ndim == 1:
            el = np.broadcast_to(el[:, None], (G, K))
    return [[0 <= g < G and (el is None or bool(el[g, k])) for g in gid] for k in range(K)]


def counts(state, alloc, k_spec, Rk, cap, el_k):
    """One step's a_i on the current state, or None when an eligible row panics.
    state = (pod_count, used_cpu, used_mem, used_x[R]), alloc = (alloc_cpu, alloc_mem,
    alloc_pods, alloc_x[R]), k_spec = (c, m, x[R]); all Python ints."""
    pc, uc, um, ux = state
    ac, am, ap, ax = alloc
    c, m, x = k_spec
    R = len(x)
    a = []
    for i in range(len(ac)):
        if not el_k[i]:
            a.append(0)
            continue
        try:
            q = fit_one_ext(ac[i], am[i], ap[i], pc[i], uc[i], um[i], [ax[r][i] for r in range(R)],
                            [ux[r][i] for r in range(R)], c, m, x)
        except ZeroDivisionError:
            return None
        v = max(q, 0)                 # a negative clamp value holds nothing
        if cap > 0:
            v = min(v, cap)           # after the clamp
        a.append(min(v, Rk))
    return a


def deploy(rows, alloc_x, used_x, spec_cpu, spec_mem, spec_x, replicas, policy, node_cap=None,
           group=None, n_groups=1, eligible=None) -> Result:
    """rows = (alloc_cpu, alloc_mem, alloc_pods, pod_count, used_cpu, used_mem) as the fits
    take them.  Nothing passed in is modified."""
    ac, am, ap, pc, uc, um = [[int(v) for v in col] for col in rows]
    ax = [[int(v) for v in col] for col in alloc_x]
    ux = [[int(v) for v in col] for col in used_x]
    sx = [[int(v) for v in col] for col in spec_x]
    n, K, R = len(ac), len(spec_cpu), len(ax)
    el = _eligibility(n, K, group, n_groups, eligible)
    placed, used_n, err = np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros(K, np.int32)
    out_rows = np.zeros((K, n), np.int64)
    for k in range(K):
        Rk = clamp_replicas(replicas[k])
        c, m = int(spec_cpu[k]), int(spec_mem[k])
        x = [sx[r][k] for r in range(R)]
        cap = 0 if node_cap is None else int(node_cap[k])
        a = counts((pc, uc, um, ux), (ac, am, ap, ax), (c, m, x), Rk, cap, el[k])
        if a is None:
            err[k] = 1
            continue
        p = place(a, Rk, policy)
        for i, v in enumerate(p):
            if v == 0:
                continue
            uc[i] = u64(uc[i] + v * u64(c))
            um[i] = i64(um[i] + v * i64(m))
            for r in range(R):
                if x[r] != 0:
                    ux[r][i] = i64(ux[r][i] + v * i64(x[r]))
            pc[i] = i64(pc[i] + v)
        placed[k] = sum(p)
        used_n[k] = sum(1 for v in p if v > 0)
        out_rows[k] = p
    return Result(placed, used_n, err, np.array(pc, np.int64),
                  np.array([u64(v) for v in uc], np.uint64), np.array(um, np.int64),
                  np.array(ux, np.int64).reshape(R, n), out_rows)


def place_np(a, Rk: int, policy: int):
    """place() on an int64 array."""
    T = int(a.sum())
    if Rk >= T:
        return a.copy()
    if Rk == 0:
        return np.zeros_like(a)
    if policy == PACK:
        before = np.cumsum(a) - a
        return np.minimum(a, np.maximum(0, Rk - before))
    lo, hi = 1, int(a.max())
    while lo < hi:
        mid = (lo + hi) // 2
        if int(np.minimum(a, mid).sum()) >= Rk:
            hi = mid
        else:
            lo = mid + 1
    p = np.minimum(a, lo - 1)
    rem = Rk - int(p.sum())
    top = np.flatnonzero(a >= lo)
    p[top[:rem]] += 1
    return p


def deploy_np(rows, alloc_x, used_x, spec_cpu, spec_mem, spec_x, replicas, policy, node_cap=None,
              group=None, n_groups=1, eligible=None) -> Result:
    """deploy() in numpy int64, for PLAIN inputs only: every value in [0, 2^62), cpu and
    memory requests >= 1, extra requests >= 0 — nothing wraps, nothing panics."""
    ac, am, ap, pc, uc, um = [np.array(col).astype(np.int64) for col in rows]
    n, K, R = ac.size, len(spec_cpu), len(alloc_x)
    ax = np.array(alloc_x, np.int64).reshape(R, n)
    ux = np.array(used_x, np.int64).reshape(R, n)
    sx = np.array(spec_x, np.int64).reshape(R, K)
    G = int(n_groups)
    gid = np.zeros(n, np.int64) if group is None else np.asarray(group, np.int64)
    valid = (gid >= 0) & (gid < G)
    el = None
    if eligible is not None:
        el = np.asarray(eligible, bool)
        if el.ndim == 1:
            el = np.broadcast_to(el[:, None], (G, K))
    placed, used_n, err = np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros(K, np.int32)
    out_rows = np.zeros((K, n), np.int64)
    for k in range(K):
        Rk = clamp_replicas(replicas[k])
        c, m = int(spec_cpu[k]), int(spec_mem[k])
        assert c >= 1 and m >= 1
        q = np.minimum(np.maximum(ac - uc, 0) // c, np.maximum(am - um, 0) // m)
        for r in range(R):
            if sx[r, k] != 0:
                q = np.minimum(q, np.maximum(ax[r] - ux[r], 0) // int(sx[r, k]))
        q = np.where(q >= ap, ap - pc, q)
        a = np.maximum(q, 0)
        if node_cap is not None and int(node_cap[k]) > 0:
            a = np.minimum(a, int(node_cap[k]))
        a = np.minimum(a, Rk)
        ok = valid.copy()
        if el is not None:
            ok &= el[np.where(valid, gid, 0), k]
        a = np.where(ok, a, 0)
        p = place_np(a, Rk, policy)
        uc += p * c
        um += p * m
        for r in range(R):
            ux[r] += p * int(sx[r, k])
        pc += p
        placed[k] = p.sum()
        used_n[k] = (p > 0).sum()
        out_rows[k] = p
    return Result(placed, used_n, err, pc, uc.astype(np.uint64), um, ux, out_rows)
