"""Grouped fit on the GPU (kcc_fit_grouped): every cell of totals / err
against the C oracle run on exactly the rows of that group (coracle.fit on the row subset,
coracle.fit_one for crafted rows) — adversarial rows and specs, sizes around the 64-lane
wave, the 1024-row sort workgroup and the R-row pair-loop run, one to 1000 groups with
skipped ids, the per-group panic rule, degenerate inputs, workspace reuse, the device form
and the argument errors."""
import ctypes as C

import numpy as np
import pytest

from kubernetesclustercapacity_amd import KccError, _lib, synth
from oracle import coracle

U64 = 1 << 64
R = 256  # kcc_internal.h GRP_RUN: group-ordered rows one pair-loop workgroup walks
I64 = np.iinfo(np.int64)

SMALL_N = [1, 63, 64, 65, R - 1, R, R + 1, 1023, 1024, 1025]
SMALL_S = [1, 63, 64, 65]
GROUPS = [1, 2, 7, 1000]


@pytest.fixture(scope="module")
def eng():
    from tests.conftest import init_torch_first
    init_torch_first()
    from kubernetesclustercapacity_amd import CapacityEngine
    with CapacityEngine(0, 1) as e:
        yield e


def rows_case(n, seed=3):
    """tests/test_rows.py::rows_case for any n: the adversarial cluster plus raw extremes
    on up to 40 rows.  Returns the six node-row arrays."""
    c = synth.make_cluster(n, n * 20, seed=seed, chunk=1024, adversarial=True)
    uc, um, _, _ = coracle.reduce_requests(c.node_ptr, c.cpu_req, c.mem_req)
    rng = np.random.default_rng(seed)
    k = rng.choice(n, min(n, 40), replace=False)
    c.alloc_mem[k[:10]] = I64.max
    um[k[:10]] = I64.min + 5                 # am - um wraps negative
    c.alloc_cpu[k[10:20]] = np.uint64(U64 - 1)
    c.pod_count[k[20:30]] = I64.min          # P - pc wraps
    c.alloc_pods[k[30:40]] = -3
    return [c.alloc_cpu, c.alloc_mem, c.alloc_pods, c.pod_count, uc, um]


def group_ids(n, G, seed):
    """Uniform ids, 3 % of them invalid (-1 or G + 5)."""
    rng = np.random.default_rng([seed, G, n])
    gid = rng.integers(0, G, n).astype(np.int32)
    bad = rng.random(n) < 0.03
    gid[bad] = np.where(rng.random(int(bad.sum())) < 0.5, -1, G + 5)
    return gid


def expected(rows, gid, G, sc, sm):
    tot = np.zeros((G, sc.size), np.int64)
    err = np.zeros((G, sc.size), np.int32)
    order = np.argsort(gid, kind="stable")
    g_sorted = gid[order]
    lo = np.searchsorted(g_sorted, np.arange(G), "left")
    hi = np.searchsorted(g_sorted, np.arange(G), "right")
    for g in np.flatnonzero(hi > lo):
        sel = order[lo[g]:hi[g]]
        tot[g], err[g] = coracle.fit(*[a[sel] for a in rows], sc, sm)
    return tot, err


_ROWS = {}


def cached_rows(n):
    if n not in _ROWS:
        _ROWS[n] = rows_case(n)
    return _ROWS[n]


def check_case(eng, n, S, G):
    rows = cached_rows(n)
    sc, sm = synth.make_specs(S, seed=3, adversarial=True)
    gid = group_ids(n, G, 3)
    t, e = eng.fit_grouped(*rows, gid, G, sc, sm)
    ot, oe = expected(rows, gid, G, sc, sm)
    assert t.shape == e.shape == (G, S)
    assert np.array_equal(e, oe), (n, S, G)
    assert np.array_equal(t, ot), (n, S, G)
    return t, e


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL_N)
def test_gpu_grouped_matches_oracle_small(eng, n):
    flagged = unflagged = 0
    for S in SMALL_S:
        for G in GROUPS:
            _, e = check_case(eng, n, S, G)
            flagged += int((e != 0).sum())
            unflagged += int((e == 0).sum())
    assert flagged > 0 and unflagged > 0


@pytest.mark.gpu
@pytest.mark.parametrize("G", GROUPS)
def test_gpu_grouped_matches_oracle_5000x300(eng, G):
    t, e = check_case(eng, 5000, 300, G)
    assert (e != 0).any() and (e == 0).any()
    assert (t < 0).any() and (t > 0).any()
    # the cells of an unflagged spec sum (wrapping) to the fit of the rows not skipped
    rows = cached_rows(5000)
    sc, sm = synth.make_specs(300, seed=3, adversarial=True)
    keep = (group_ids(5000, G, 3) >= 0) & (group_ids(5000, G, 3) < G)
    wt, we = coracle.fit(*[a[keep] for a in rows], sc, sm)
    ok = ~(e != 0).any(axis=0)
    assert ok.any() and np.array_equal(we != 0, ~ok)
    assert np.array_equal(t.view(np.uint64).sum(axis=0, dtype=np.uint64)[ok], wt.view(np.uint64)[ok])


@pytest.mark.gpu
@pytest.mark.parametrize("n,S,G", [(1025, 64, 7), (R + 1, 300, 2), (5000, 128, 1000)])
def test_gpu_grouped_ordinary_specs_take_the_fast_path(eng, n, S, G):
    """Ordinary specs (every wave of 64 all fast) over the adversarial rows: fast rows go
    through the f64 reciprocal path, the wrapped and huge rows through the exact one."""
    rows = cached_rows(n)
    sc, sm = synth.make_specs(S, seed=5)
    gid = group_ids(n, G, 5)
    t, e = eng.fit_grouped(*rows, gid, G, sc, sm)
    ot, oe = expected(rows, gid, G, sc, sm)
    assert not oe.any() and np.array_equal(e, oe) and np.array_equal(t, ot)
    assert (t > 0).any()


@pytest.mark.gpu
def test_gpu_grouped_fast_path_bound_edges(eng):
    """Rows and specs on both edges of every fast-path bound (free CPU < 2^31, free memory
    < 2^50, 1 <= c, m <= 2^52) and one step outside, exact multiples and their neighbours;
    the pod-slot limit is out of the way (2^62) so the quotients themselves are compared."""
    fcs = [0, 1, 2, 999, 1000, 1001, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 52) + 3]
    fms = [0, 1, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, 3 * (1 << 40) - 1, 3 * (1 << 40),
           (1 << 50) - 1, 1 << 50, (1 << 50) + 1, (1 << 62) + 12345]
    ac, am = [np.array(x).ravel() for x in np.meshgrid(np.array(fcs, np.uint64),
                                                      np.array(fms, np.int64))]
    n = ac.size
    used_c = np.full(n, 7, np.uint64)
    used_m = np.full(n, 9, np.int64)
    ac = ac + used_c
    am = am + used_m
    am[am <= 9] = 9  # (free memory 0: alloc == used)
    ap = np.full(n, 1 << 62, np.int64)
    ap[::7] = 5      # some rows clamp
    pc = np.full(n, 2, np.int64)
    rows = [ac, am, ap, pc, used_c, used_m]
    cs = [1, 2, 3, 1000, (1 << 31) - 1, 1 << 31, (1 << 52) - 1, 1 << 52]
    ms = [1, 2, 3, 1 << 30, 3 * (1 << 40), (1 << 50) - 1, (1 << 52) - 1, 1 << 52]
    sc, sm = [np.array(x).ravel() for x in np.meshgrid(np.array(cs, np.uint64),
                                                      np.array(ms, np.int64))]
    assert sc.size == 64  # one all-fast wave
    gid = (np.arange(n) % 3).astype(np.int32)
    t, e = eng.fit_grouped(*rows, gid, 3, sc, sm)
    ot, oe = expected(rows, gid, 3, sc, sm)
    assert not oe.any() and np.array_equal(e, oe) and np.array_equal(t, ot)
    # the same rows one group each: every row's q by itself
    t, e = eng.fit_grouped(*rows, np.arange(n, dtype=np.int32), n, sc, sm)
    ot, oe = expected(rows, np.arange(n, dtype=np.int32), n, sc, sm)
    assert np.array_equal(e, oe) and np.array_equal(t, ot)
    # one step outside the spec bounds (the wave turns exact): same answers
    sc2, sm2 = sc.copy(), sm.copy()
    sc2[-1] = np.uint64((1 << 52) + 1)
    sm2[-2] = (1 << 52) + 1
    t, e = eng.fit_grouped(*rows, gid, 3, sc2, sm2)
    ot, oe = expected(rows, gid, 3, sc2, sm2)
    assert np.array_equal(e, oe) and np.array_equal(t, ot)


@pytest.mark.gpu
def test_gpu_grouped_panic_rule_is_per_group(eng):
    """Group 0 holds only full rows (among them allocatable pods -3 with 4 pods: -7): a
    zero request divides nothing there.  Group 1 has free CPU but no free memory: flagged
    for a zero cpu request only.  Groups 2 and 3 have both."""
    ac = np.array([1000, 500, 0, 4000, 4000, 8000, 8000, 16000], np.uint64)
    uc = np.array([1000, 900, 0, 1000, 500, 1000, 2000, 100], np.uint64)
    am = np.array([1 << 30, 1 << 20, 0, 1 << 30, 1 << 31, 1 << 34, 1 << 34, 1 << 35], np.int64)
    um = np.array([1 << 30, 1 << 21, 5, 1 << 30, 1 << 32, 1 << 30, 1 << 31, 1 << 20], np.int64)
    ap = np.array([-3, 0, 110, 110, 2, 110, 110, 3], np.int64)
    pc = np.array([4, 5, 7, 9, 1, 20, 30, 1], np.int64)
    gid = np.array([0, 0, 0, 1, 1, 2, 3, 3], np.int32)
    sc = np.array([0, 100, 200], np.uint64)
    sm = np.array([1 << 20, 0, 1 << 28], np.int64)
    rows = [ac, am, ap, pc, uc, um]
    assert coracle.fit_one(1000, 1 << 30, -3, 4, 1000, 1 << 30, 0, 1 << 20) == (-7, 0)
    t, e = eng.fit_grouped(*rows, gid, 4, sc, sm)
    ot, oe = expected(rows, gid, 4, sc, sm)
    assert np.array_equal(t, ot) and np.array_equal(e, oe)
    assert e[0].tolist() == [0, 0, 0] and t[0].tolist() == [-12, -12, -12]  # -7 + -5 + 0
    assert e[1].tolist() == [1, 0, 0]
    assert e[2].tolist() == [1, 1, 0] and e[3].tolist() == [1, 1, 0]
    assert t[1, 0] == 0 and t[2, 1] == 0


@pytest.mark.gpu
def test_gpu_grouped_degenerate(eng):
    n, S = 300, 70
    rows = cached_rows(1025)
    rows = [a[:n] for a in rows]
    sc, sm = synth.make_specs(S, seed=3, adversarial=True)
    # all ids invalid
    t, e = eng.fit_grouped(*rows, np.full(n, -1, np.int32), 3, sc, sm)
    assert not t.any() and not e.any()
    t, e = eng.fit_grouped(*rows, np.full(n, 3, np.int32), 3, sc, sm)
    assert not t.any() and not e.any()
    # empty groups, and more groups than rows
    gid = (np.arange(n) % 2 * 4).astype(np.int32)  # groups 0 and 4 of 6
    t, e = eng.fit_grouped(*rows, gid, 6, sc, sm)
    ot, oe = expected(rows, gid, 6, sc, sm)
    assert np.array_equal(t, ot) and np.array_equal(e, oe)
    assert not t[[1, 2, 3, 5]].any() and not e[[1, 2, 3, 5]].any()
    gid = group_ids(n, 1000, 8)
    t, e = eng.fit_grouped(*rows, gid, 1000, sc, sm)
    ot, oe = expected(rows, gid, 1000, sc, sm)
    assert np.array_equal(t, ot) and np.array_equal(e, oe)
    # every row in one group: the whole-cluster fit
    t, e = eng.fit_grouped(*rows, np.zeros(n, np.int32), 1, sc, sm)
    wt, we = eng.total_possible_max_replicas(*rows, sc, sm)
    assert np.array_equal(t[0], wt) and np.array_equal(e[0], we)
    # no rows, no specs
    empty = [a[:0] for a in rows]
    t, e = eng.fit_grouped(*empty, np.zeros(0, np.int32), 5, sc, sm)
    assert t.shape == (5, S) and not t.any() and not e.any()
    t, e = eng.fit_grouped(*rows, np.zeros(n, np.int32), 5, sc[:0], sm[:0])
    assert t.shape == (5, 0) and e.shape == (5, 0)
    # sorted ids and a permutation of the same rows
    gid = group_ids(n, 7, 9)
    order = np.argsort(gid, kind="stable")
    perm = np.random.default_rng(4).permutation(n)
    a = eng.fit_grouped(*[x[order] for x in rows], gid[order], 7, sc, sm)
    b = eng.fit_grouped(*[x[perm] for x in rows], gid[perm], 7, sc, sm)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    ot, oe = expected(rows, gid, 7, sc, sm)
    assert np.array_equal(a[0], ot) and np.array_equal(a[1], oe)


@pytest.mark.gpu
def test_gpu_grouped_workspace_reuse():
    """The small call on a fresh engine, and again after a call that grew every buffer."""
    from kubernetesclustercapacity_amd import CapacityEngine
    rows = cached_rows(65)
    sc, sm = synth.make_specs(63, seed=3, adversarial=True)
    gid = group_ids(65, 7, 3)
    with CapacityEngine(0, 1) as fresh:
        first = fresh.fit_grouped(*rows, gid, 7, sc, sm)
    with CapacityEngine(0, 1) as used:
        big = cached_rows(5000)
        bc, bm = synth.make_specs(300, seed=3, adversarial=True)
        used.fit_grouped(*big, group_ids(5000, 1000, 3), 1000, bc, bm)
        again = used.fit_grouped(*rows, gid, 7, sc, sm)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    ot, oe = expected(rows, gid, 7, sc, sm)
    assert np.array_equal(first[0], ot) and np.array_equal(first[1], oe)


@pytest.mark.gpu
def test_gpu_grouped_async_two_calls_one_stream(eng):
    import torch
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(  # noqa: E731
        np.int64 if a.dtype == np.uint64 else a.dtype)).to(dev)
    cases = []
    for n, S, G in [(1025, 65, 7), (257, 64, 1000)]:
        rows = cached_rows(n)
        sc, sm = synth.make_specs(S, seed=3, adversarial=True)
        gid = group_ids(n, G, 3)
        d = [T(a) for a in rows] + [T(gid), G, T(sc), T(sm)]
        out = (torch.full((G * S,), 77, dtype=torch.int64, device=dev),
               torch.full((G * S,), 77, dtype=torch.int32, device=dev))
        cases.append((d, out, eng.fit_grouped(*rows, gid, G, sc, sm), (G, S)))
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        for d, out, _, _ in cases:
            eng.fit_grouped_async(*d, out[0], out[1], stream=stream)
    stream.synchronize()
    for _, out, host, shape in cases:
        assert np.array_equal(out[0].cpu().numpy().reshape(shape), host[0])
        assert np.array_equal(out[1].cpu().numpy().reshape(shape), host[1])


@pytest.mark.gpu
def test_gpu_grouped_argument_errors(eng):
    a = [np.zeros(4, t) for t in (np.uint64, np.int64, np.int64, np.int64, np.uint64, np.int64)]
    gid = np.zeros(4, np.int32)
    sc, sm = np.ones(2, np.uint64), np.ones(2, np.int64)
    t, e = np.zeros(8, np.int64), np.zeros(8, np.int32)
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)  # noqa: E731

    def call(group, G, S):
        rc = eng._lib.kcc_fit_grouped(eng._h, 4, *[p(x) for x in a], p(group), G, S, p(sc), p(sm),
                                      p(t), p(e))
        return rc, eng._lib.kcc_last_error(eng._h).decode()

    # (None, 1, 2): kcc_fit_ext takes a NULL group with one group; the grouped call does not
    for group, G, S in [(gid, 0, 2), (gid, -1, 2), (gid, (1 << 27) + 1, 2), (gid, 1 << 28, 2),
                        (gid, 1 << 62, 1 << 62), (None, 4, 2), (None, 1, 2)]:
        rc, msg = call(group, G, S)
        assert rc == _lib.KCC_EINVAL and msg, (G, S)
    rc, msg = call(gid, 4, 2)  # the same buffers with valid sizes
    assert rc == 0, msg
    # the device form with a NULL group pointer
    import torch
    dev = torch.device("cuda", 0)
    d = [torch.zeros(4, dtype=torch.int64, device=dev) for _ in range(6)]
    dsc, dsm = [torch.ones(2, dtype=torch.int64, device=dev) for _ in range(2)]
    dt = torch.zeros(8, dtype=torch.int64, device=dev)
    de = torch.zeros(8, dtype=torch.int32, device=dev)
    for G in (1, 4):
        with pytest.raises(KccError) as ei:
            eng.fit_grouped_async(*d, None, G, dsc, dsm, dt, de)
        assert ei.value.code == _lib.KCC_EINVAL
        assert eng._lib.kcc_last_error(eng._h).decode()
    torch.cuda.synchronize()


def _raw_cells(eng, entry, rows, gid, G, sc, sm):
    """kcc_fit_ext (n_ext = 0) or kcc_fit_capped (every optional pointer NULL) through the
    C-ABI itself; the outputs start at 77 so a cell left unwritten shows."""
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)  # noqa: E731
    rows = [np.ascontiguousarray(a, d) for a, d in zip(rows, (np.uint64, np.int64, np.int64,
                                                              np.int64, np.uint64, np.int64))]
    sc, sm = np.ascontiguousarray(sc, np.uint64), np.ascontiguousarray(sm, np.int64)
    n, S = rows[0].size, sc.size
    t = np.full((G, S), 77, np.int64)
    e = np.full((G, S), 77, np.int32)
    args = [eng._h, n, *[p(a) for a in rows], 0, None, None, p(gid), G, S, p(sc), p(sm), None,
            p(t), p(e)]
    if entry == "kcc_fit_capped":
        args += [None, None, None]
    rc = getattr(eng._lib, entry)(*args)
    assert rc == 0, eng._lib.kcc_last_error(eng._h).decode()
    return t, e


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 3, 4097])
def test_gpu_three_entry_points_are_one_path(eng, G):
    """kcc_fit_grouped, kcc_fit_ext with n_ext = 0 and kcc_fit_capped with no cap, no cell_min
    and no group_rows give the same bits in every cell, and they are the oracle's.  n = 1025:
    two scatter workgroups of 1024 rows and five pair-loop runs of 256, the last of one row;
    S = 65: a second wave with one live lane; G = 4097 > GRP_LDS_GROUPS sorts with global
    atomics; 3 % of the ids lie outside [0, G)."""
    n, S = 1025, 65
    rows = cached_rows(n)
    sc, sm = synth.make_specs(S, seed=3, adversarial=True)
    gid = group_ids(n, G, 3)
    assert ((gid < 0) | (gid >= G)).any()
    t, e = eng.fit_grouped(*rows, gid, G, sc, sm)
    ot, oe = expected(rows, gid, G, sc, sm)
    assert t.shape == e.shape == ot.shape == (G, S)
    assert np.array_equal(e, oe) and np.array_equal(t, ot)
    for entry in ("kcc_fit_ext", "kcc_fit_capped"):
        xt, xe = _raw_cells(eng, entry, rows, gid, G, sc, sm)
        assert np.array_equal(xe, e) and np.array_equal(xt, t), entry
    assert (e != 0).any() and (e == 0).any()
