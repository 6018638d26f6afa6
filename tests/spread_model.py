"""Spread constraints in the fit (kcc_fit_capped, kcc_spread_fold) restated
in Python integers.

TEST INFRASTRUCTURE ONLY (not a test module).  Built on tests/ext_model.pair_table's q /
panic table: the per-node cap after the pod-slot clamp, the per-cell minimum before the cap,
the groups' row counts, and the fold of the cells to one total per spec, each exactly as
include/kcc.h states it.  Pure-Python loops: small cases only.
"""
from __future__ import annotations

import numpy as np

from oracle.pyoracle import i64

I64_MAX = (1 << 63) - 1


def capped_cells(q, dz, group=None, n_groups=1, node_cap=None):
    """kcc_fit_capped from ext_model.pair_table's (q [N, S], panics [N, S]): (totals int64,
    err int32, cell_min int64, group_rows int64 [G]); the first three [S] without group ids
    and [G, S] with them."""
    n, S = q.shape
    G = int(n_groups)
    gid = [0] * n if group is None else [int(g) for g in group]
    cap = [0] * S if node_cap is None else [int(k) for k in node_cap]
    tot = [[0] * S for _ in range(G)]
    mn = [[I64_MAX] * S for _ in range(G)]
    err = np.zeros((G, S), np.int32)
    rows = np.zeros(G, np.int64)
    ql = q.tolist()
    for i in range(n):
        g = gid[i]
        if g < 0 or g >= G:
            continue
        rows[g] += 1
        tg, mg, qi = tot[g], mn[g], ql[i]
        for s in range(S):
            v = qi[s]
            if v < mg[s]:
                mg[s] = v                      # before the cap
            if cap[s] > 0 and v > cap[s]:
                v = cap[s]                     # signed, after the clamp
            tg[s] += v
        err[g] |= dz[i]
    t = np.array([[i64(v) for v in r] for r in tot], np.int64).reshape(G, S)  # wraps
    m = np.array(mn, np.int64).reshape(G, S)
    t[err != 0] = 0
    m[err != 0] = 0
    if group is None:
        return t[0], err[0], m[0], rows
    return t, err, m, rows


def fold(cell_totals, cell_err, group_rows=None, domain_of=None, n_domains=None, eligible=None,
         max_skew=None):
    """kcc_spread_fold: (totals int64 [S], err int32 [S], caps) where caps[s] is the dict
    {present domain: cap_d} of spec s (empty when the spec is flagged)."""
    t = np.asarray(cell_totals, np.int64)
    e = np.asarray(cell_err)
    G, S = t.shape
    D = G if n_domains is None else int(n_domains)
    el = None
    if eligible is not None:
        el = np.asarray(eligible, bool)
        if el.ndim == 1:
            el = np.broadcast_to(el[:, None], (G, S))
    totals = np.zeros(S, np.int64)
    err = np.zeros(S, np.int32)
    caps = []
    for s in range(S):
        cap = {}
        flagged = False
        for g in range(G):
            if group_rows is not None and int(group_rows[g]) <= 0:
                continue
            d = g if domain_of is None else int(domain_of[g])
            if d < 0 or d >= D:
                continue
            if el is not None and not el[g, s]:
                continue
            flagged = flagged or int(e[g, s]) != 0
            cap[d] = i64(cap.get(d, 0) + int(t[g, s]))  # wraps
        if flagged:
            err[s] = 1
            caps.append({})
            continue
        caps.append(cap)
        k = 0 if max_skew is None else int(max_skew[s])
        if not cap:
            continue
        if k <= 0:
            totals[s] = i64(sum(cap.values()))
            continue
        lim = min(min(cap.values()) + k, I64_MAX)  # saturates
        totals[s] = i64(sum(c if c <= lim else lim for c in cap.values()))
    return totals, err, caps


def host_cap(cell_min, group_rows, host_max_skew, node_cap=None, domain_of=None, n_domains=None,
             eligible=None):
    """The second pass's cap of fit_spread(host_max_skew=...): m[s] = min of cell_min over the
    live eligible groups, cap = max(m, 0) + host_max_skew[s] saturating (<= 0: none),
    combined with node_cap by min."""
    cm = np.asarray(cell_min, np.int64)
    G, S = cm.shape
    D = G if n_domains is None else int(n_domains)
    el = None
    if eligible is not None:
        el = np.asarray(eligible, bool)
        if el.ndim == 1:
            el = np.broadcast_to(el[:, None], (G, S))
    out = np.zeros(S, np.int64)
    for s in range(S):
        m = I64_MAX
        for g in range(G):
            if int(group_rows[g]) <= 0 or (el is not None and not el[g, s]):
                continue
            if domain_of is not None and not 0 <= int(domain_of[g]) < D:
                continue
            m = min(m, int(cm[g, s]))
        k = int(host_max_skew[s])
        c = min(max(m, 0) + k, I64_MAX) if k > 0 else 0
        if node_cap is not None and int(node_cap[s]) > 0:
            c = min(c, int(node_cap[s])) if c > 0 else int(node_cap[s])
        out[s] = c
    return out
