"""The fit explained (kcc_fit_explain) restated in Python integers.

TEST INFRASTRUCTURE ONLY (not a test module).  Built on oracle.pyoracle's u64 / i64 /
go_div_i64 and tests/ext_model.py's free amounts: per (row, spec) the quotients of
kcc_fit_capped, findMin with the reason carried along (ties keep the earlier term, CC:159-164),
the pod-slot clamp (equality fires, CC:134-136), the per-node cap (equality does not), and per
cell the rows and replicas by reason and what stays free — `left` summed ROW BY ROW, as
include/kcc.h defines it (the device uses sum(free) - request x total instead).

Layouts as the C-ABI's: alloc_x / used_x [R][N], spec_x [R][S]; the outputs are plane-major
[planes, G, S].  Pure-Python loops: keep N x S <= 5e4 per case.
"""
from __future__ import annotations

import numpy as np

from oracle.pyoracle import go_div_i64, i64, u64
from tests.ext_model import free_cpu, free_signed

SLOTS, CPU, MEM, EXT0, PODS, CAP = 8, 0, 1, 2, 6, 7  # include/kcc.h KCC_WHY_*
M64 = (1 << 64) - 1


def explain_one(fc, fm, fx, alloc_pods, pod_count, c, m, x, cap):
    """One row (its free amounts), one spec: (q, reason, qc, qm, qx list or None per resource,
    q before the clamp).  Raises ZeroDivisionError where Go panics (kcc_fit's rule)."""
    c, m = u64(c), i64(m)
    qc = qm = 0
    if fc != 0:
        if c == 0:
            raise ZeroDivisionError("integer divide by zero")
        qc = i64(fc // c)          # int(uint64) reinterprets
    if fm != 0:
        qm = go_div_i64(fm, m)     # raises on a zero request
    q, b = qc, CPU
    if not qc <= qm:
        q, b = qm, MEM
    qxs = []
    for r, xr in enumerate(x):
        xr = i64(int(xr))
        if xr == 0:
            qxs.append(None)       # not requested
            continue
        qx = 0 if fx[r] == 0 else go_div_i64(fx[r], xr)
        qxs.append(qx)
        if not q <= qx:
            q, b = qx, EXT0 + r
    qmin = q
    P = i64(alloc_pods)
    if q >= P:
        q, b = i64(P - i64(pod_count)), PODS
    if cap > 0 and q > cap:
        q, b = cap, CAP
    return q, b, qc, qm, qxs, qmin


def frees(rows, alloc_x, used_x):
    """(fc [N], fm [N], fx [R][N]) as Python integers."""
    ac, am, _, _, uc, um = [[int(v) for v in a] for a in rows]
    n = len(ac)
    fc = [free_cpu(ac[i], uc[i]) for i in range(n)]
    fm = [free_signed(am[i], um[i]) for i in range(n)]
    fx = [[free_signed(int(a), int(u)) for a, u in zip(ca, cu)] for ca, cu in zip(alloc_x, used_x)]
    return fc, fm, fx


def explain_table(rows, alloc_x, used_x, spec_cpu, spec_mem, spec_x, node_cap=None):
    """Every (row, spec): dict of q int64 [N, S], b int8 [N, S], dz bool [N, S], and `ties`, a
    dict of counts of the pairs on which a tie decided (or could have decided) the reason."""
    n, S, R = len(rows[0]), len(spec_cpu), len(alloc_x)
    fc, fm, fx = frees(rows, alloc_x, used_x)
    ap = [int(v) for v in rows[2]]
    pc = [int(v) for v in rows[3]]
    sx = [[int(v) for v in col] for col in spec_x]
    cap = [0] * S if node_cap is None else [int(k) for k in node_cap]
    q = np.zeros((n, S), np.int64)
    b = np.zeros((n, S), np.int8)
    dz = np.zeros((n, S), bool)
    ties = {"qc==qm": 0, "q==qx": 0, "q==alloc_pods": 0, "q==node_cap": 0}
    for s in range(S):
        c, m = int(spec_cpu[s]), int(spec_mem[s])
        xs = [sx[r][s] for r in range(R)]
        for i in range(n):
            try:
                v, w, qc, qm, qxs, qmin = explain_one(fc[i], fm[i], [fx[r][i] for r in range(R)],
                                                      ap[i], pc[i], c, m, xs, cap[s])
            except ZeroDivisionError:
                dz[i, s] = True
                continue
            q[i, s], b[i, s] = v, w
            ties["qc==qm"] += qc == qm
            run = qc if qc <= qm else qm
            for qx in qxs:
                if qx is not None:
                    ties["q==qx"] += run == qx
                    run = run if run <= qx else qx
            ties["q==alloc_pods"] += qmin == i64(ap[i])
            if cap[s] > 0 and w != CAP:
                ties["q==node_cap"] += v == cap[s]
    return {"q": q, "b": b, "dz": dz, "ties": ties, "free": (fc, fm, fx)}


def explain_cells(tab, spec_cpu, spec_mem, spec_x, group=None, n_groups=1):
    """kcc_fit_explain's outputs from explain_table's: (totals int64 [G, S], err int32 [G, S],
    why_rows int64 [8, G, S], why_pods [8, G, S], left [2 + R, G, S]); `left` row by row."""
    q, b, dz = tab["q"].tolist(), tab["b"].tolist(), tab["dz"]
    fc, fm, fx = tab["free"]
    n, S, R, G = len(q), len(spec_cpu), len(fx), int(n_groups)
    gid = [0] * n if group is None else [int(g) for g in group]
    c = [u64(int(v)) for v in spec_cpu]
    m = [i64(int(v)) for v in spec_mem]
    x = [[i64(int(v)) for v in col] for col in spec_x]
    tot = [[0] * S for _ in range(G)]
    wr = [[[0] * S for _ in range(G)] for _ in range(SLOTS)]
    wp = [[[0] * S for _ in range(G)] for _ in range(SLOTS)]
    left = [[[0] * S for _ in range(G)] for _ in range(2 + R)]
    err = np.zeros((G, S), np.int32)
    for i in range(n):
        g = gid[i]
        if g < 0 or g >= G:
            continue
        err[g] |= dz[i]
        for s in range(S):
            v, w = q[i][s], b[i][s]
            tot[g][s] += v
            wr[w][g][s] += 1
            wp[w][g][s] += v
            left[0][g][s] += fc[i] - v * c[s]
            left[1][g][s] += fm[i] - v * m[s]
            for r in range(R):
                left[2 + r][g][s] += fx[r][i] - v * x[r][s]

    def arr(planes):
        a = np.array([[[i64(v) for v in row] for row in p] for p in planes], np.int64)
        a = a.reshape(len(planes), G, S)
        a[:, err != 0] = 0  # a flagged cell: every entry 0
        return a

    t = arr([tot])[0]
    return t, err, arr(wr), arr(wp), arr(left)


def left_by_identity(tab, totals, err, spec_cpu, spec_mem, spec_x, group=None, n_groups=1):
    """left [2 + R, G, S] as the device computes it: sum of the group's free amounts less
    request x total, modulo 2^64; a flagged cell 0."""
    fc, fm, fx = tab["free"]
    n, S, R, G = len(fc), len(spec_cpu), len(fx), int(n_groups)
    gid = [0] * n if group is None else [int(g) for g in group]
    cols = [fc, fm] + list(fx)
    req = [[u64(int(v)) for v in spec_cpu], [i64(int(v)) for v in spec_mem]]
    req += [[i64(int(v)) for v in col] for col in spec_x]
    t = np.asarray(totals, np.int64).reshape(G, S).tolist()
    out = np.zeros((2 + R, G, S), np.int64)
    for k in range(2 + R):
        fsum = [0] * G
        for i in range(n):
            if 0 <= gid[i] < G:
                fsum[gid[i]] += cols[k][i]
        for g in range(G):
            for s in range(S):
                out[k, g, s] = i64(fsum[g] - req[k][s] * t[g][s])
    out[:, np.asarray(err).reshape(G, S) != 0] = 0
    return out


def fold_groups(cells, eligible, group_rows=None):
    """explain_groups: the planes of explain_cells' output folded over the eligible live groups
    (select_groups' flag rule).  Returns (totals [S], err [S], why_rows [8, S], why_pods [8, S],
    left [2 + R, S])."""
    t, e, wr, wp, left = cells
    G, S = t.shape
    el = np.asarray(eligible, bool)
    if el.ndim == 1:
        el = np.broadcast_to(el[:, None], (G, S))
    live = [True] * G if group_rows is None else [int(r) > 0 for r in group_rows]
    err = np.zeros(S, np.int32)
    for s in range(S):
        err[s] = any(live[g] and el[g, s] and int(e[g, s]) != 0 for g in range(G))

    def fold(p):
        out = np.zeros((p.shape[0], S), np.int64)
        for k in range(p.shape[0]):
            for s in range(S):
                if not err[s]:
                    out[k, s] = i64(sum(int(p[k, g, s]) for g in range(G) if live[g] and el[g, s]))
        return out

    return fold(t[None])[0], err, fold(wr), fold(wp), fold(left)
