"""Extended-resource fit on the GPU (kcc_fit_ext): every cell against
tests/ext_model.py (the semantics in Python integers) — adversarial rows, extra columns and
requests; sizes around the 64-lane wave, the 256-record run and the 1024-row sort
workgroup; R = 1, 2, 4; no groups and 2 to N groups with skipped ids; an all-fast cluster
with a GPU and a storage column; the fast path's bounds; the identities with kcc_fit and
kcc_fit_grouped; degenerate inputs, argument errors, workspace reuse and the device form.
All comparisons are integer equality."""
import ctypes as C

import numpy as np
import pytest

from kubernetesclustercapacity_amd import _lib, synth
from oracle import coracle
from tests import ext_model as xm
from tests.test_groups import group_ids, rows_case

I64 = np.iinfo(np.int64)
GIB = 1 << 30
RUN = 256  # kcc_internal.h GRP_RUN

ALL_N = [1, 63, 64, 65, RUN - 1, RUN, RUN + 1, 1023, 1024, 1025]
ALL_S = [1, 63, 64, 65, 257]
ALL_R = [1, 2, 4]


@pytest.fixture(scope="module")
def eng():
    from tests.conftest import init_torch_first
    init_torch_first()
    from kubernetesclustercapacity_amd import CapacityEngine
    with CapacityEngine(0, 1) as e:
        yield e


# ---- inputs (computed once, never modified) ------------------------------------------------
_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        v = fn()
        for a in (v if isinstance(v, (tuple, list)) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def rows(n):
    return cached(("rows", n), lambda: rows_case(n))


def ext_columns(n, R, seed=3):
    """alloc_x / used_x [R, n]: ordinary amounts (a third of the rows full or over-used),
    and on up to 50 rows per resource the extremes: alloc <= used by one and by a lot,
    used = MinInt64 with alloc = 0 (the difference wraps to MinInt64), alloc = MaxInt64 with
    a negative used (wraps negative), free amounts on both sides of 2^50."""
    rng = np.random.default_rng([seed, n, R, 0xE7])
    ax = rng.integers(0, 1 << 40, (R, n), dtype=np.int64)
    ux = (ax * rng.random((R, n))).astype(np.int64)
    full = rng.random((R, n)) < 0.33
    ux[full] = ax[full] + rng.integers(0, 5, int(full.sum()))
    small = rng.random((R, n)) < 0.3  # device-count sized
    ax[small] = rng.integers(0, 9, int(small.sum()))
    ux[small] = rng.integers(0, 9, int(small.sum()))
    for r in range(R):
        k = rng.choice(n, min(n, 50), replace=False)
        ax[r, k[0:8]], ux[r, k[0:8]] = 0, I64.min
        ax[r, k[8:16]], ux[r, k[8:16]] = I64.max, -rng.integers(1, 1 << 62, len(k[8:16]))
        ax[r, k[16:24]], ux[r, k[16:24]] = I64.max, 0
        ax[r, k[24:32]], ux[r, k[24:32]] = -5, -5 - rng.integers(0, 3, len(k[24:32]))
        ax[r, k[32:40]], ux[r, k[32:40]] = I64.min, I64.max
        ax[r, k[40:50]] = (1 << 50) + rng.integers(-2, 3, len(k[40:50])) + 7
        ux[r, k[40:50]] = 7
    return ax, ux


def ext_requests(S, R, seed=3, ordinary=False):
    """spec_x [R, S]: 0, ordinary amounts and (unless `ordinary`) 1, -1, other negatives and
    amounts past 2^52."""
    rng = np.random.default_rng([seed, S, R, 0x5E])
    sx = rng.integers(1, 1 << 34, (R, S), dtype=np.int64)
    few = rng.random((R, S)) < 0.3  # device-count sized
    sx[few] = rng.integers(1, 9, int(few.sum()))
    kind = rng.random((R, S))
    sx[kind < 0.25] = 0
    if not ordinary:
        sx[(kind >= 0.25) & (kind < 0.32)] = 1
        sx[(kind >= 0.32) & (kind < 0.39)] = -1
        neg = (kind >= 0.39) & (kind < 0.47)
        sx[neg] = -rng.integers(2, 1 << 45, int(neg.sum()))
        big = (kind >= 0.47) & (kind < 0.55)
        sx[big] = rng.integers((1 << 52) + 1, 1 << 62, int(big.sum()))
    return sx


def case_inputs(n, S, R, ordinary=False):
    def make():
        ax, ux = ext_columns(n, R)
        sc, sm = synth.make_specs(S, seed=5 if ordinary else 3, adversarial=not ordinary)
        sx = ext_requests(S, R, ordinary=ordinary)
        return ax, ux, sc, sm, sx
    return cached(("in", n, S, R, ordinary), make)


def pairs(n, S, R, ordinary=False):
    """ext_model's q / panic table of the case: one Python pass per (n, S, R)."""
    def make():
        ax, ux, sc, sm, sx = case_inputs(n, S, R, ordinary)
        return xm.pair_table(rows(n), ax, ux, sc, sm, sx)
    return cached(("pairs", n, S, R, ordinary), make)


def check_case(eng, n, S, R, G=None, ordinary=False):
    """One device call against the model; G None: no group ids."""
    ax, ux, sc, sm, sx = case_inputs(n, S, R, ordinary)
    q, dz = pairs(n, S, R, ordinary)
    gid = None if G is None else group_ids(n, G, 3)
    t, e = eng.fit_ext(*rows(n), ax, ux, sc, sm, sx, gid, 1 if G is None else G)
    mt, me = xm.totals_from_pairs(q, dz, gid, 1 if G is None else G)
    assert t.shape == e.shape == mt.shape, (n, S, R, G)
    assert np.array_equal(e, me), (n, S, R, G)
    assert np.array_equal(t, mt), (n, S, R, G)
    return t, e


# ---- parity --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", ALL_N)
def test_gpu_ext_every_n(eng, n):
    t, e = check_case(eng, n, 65, 2)
    check_case(eng, n, 65, 2, G=7)
    check_case(eng, n, 65, 2, ordinary=True)
    assert (e != 0).any() or n < 63  # (the zero-request specs panic once a row has free CPU)


@pytest.mark.gpu
@pytest.mark.parametrize("S", ALL_S)
def test_gpu_ext_every_s(eng, S):
    check_case(eng, 257, S, 2)
    check_case(eng, 257, S, 2, G=7)
    check_case(eng, 257, S, 2, ordinary=True)


@pytest.mark.gpu
@pytest.mark.parametrize("R", ALL_R)
@pytest.mark.parametrize("G", [None, 2, 7, 1000, 1025])
def test_gpu_ext_every_r_and_group_form(eng, R, G):
    n, S = 1025, 65
    t, e = check_case(eng, n, S, R, G)
    assert (e != 0).any() and (e == 0).any() and (t < 0).any() and (t > 0).any()
    t, e = check_case(eng, n, S, R, G, ordinary=True)
    assert not e.any() and (t > 0).any()


def test_parity_inputs_cover_the_listed_extremes():
    """(No GPU.)  The generated columns hold every extreme the parity cases are meant to
    carry, and the extra resources lower some pairs and leave others."""
    ax, ux = ext_columns(1025, 2)
    f = np.array([[xm.free_signed(int(a), int(u)) for a, u in zip(ax[r], ux[r])] for r in range(2)])
    assert (ax <= ux).any() and (f == I64.min).any() and (f < 0).any()
    assert ((ux == I64.min) & (ax == 0)).any() and ((ax == I64.max) & (ux < 0)).any()
    assert (f == (1 << 50) - 1).any() and (f == 1 << 50).any()
    sx = ext_requests(65, 2)
    assert (sx == 0).any() and (sx == 1).any() and (sx == -1).any() and (sx < -1).any()
    assert (sx > 1 << 52).any()
    r6 = rows(1025)
    fast = [xm.row_is_fast(int(r6[0][i]), int(r6[1][i]), int(r6[4][i]), int(r6[5][i]),
                           ax[:, i], ux[:, i]) for i in range(1025)]
    assert 100 < sum(fast) < 1000  # both row classes, well populated


# ---- an ordinary accelerator cluster: every pair on the fast path --------------------------
def gpu_storage_case():
    def make():
        n, S = 1025, 65
        c = synth.make_cluster(n, 20500, seed=3, chunk=1024)
        uc, um, _, _ = coracle.reduce_requests(c.node_ptr, c.cpu_req, c.mem_req)
        sc, sm = synth.make_specs(S, seed=3)
        rng = np.random.default_rng(3)
        ax = np.zeros((2, n), np.int64)
        ux = np.zeros((2, n), np.int64)
        ax[0] = np.where(rng.random(n) < 0.25, 8, 0)         # 8 GPUs on a quarter of the nodes
        ux[0] = rng.integers(0, 9, n)                          # 0..8 in use
        ax[1] = rng.integers(50, 2001, n) * GIB                # 50-2000 GiB of storage
        ux[1] = (ax[1] * rng.random(n)).astype(np.int64)       # a uniform share used
        sx = np.zeros((2, S), np.int64)
        sx[0] = rng.choice(np.array([0, 0, 1, 2, 4, 8]), S)
        sx[1] = np.where(rng.random(S) < 0.3, 0, rng.integers(1, 50, S) * GIB)
        r6 = [c.alloc_cpu, c.alloc_mem, c.alloc_pods, c.pod_count, uc, um]
        return r6, ax, ux, sc, sm, sx
    return cached("gpu_storage", make)


def gpu_storage_expected():
    def make():
        r6, ax, ux, sc, sm, sx = gpu_storage_case()
        q, dz = xm.pair_table(r6, ax, ux, sc, sm, sx)
        q0, dz0 = xm.pair_table(r6, ax, ux, sc, sm, np.zeros_like(sx))
        return q, dz, q0, dz0
    return cached("gpu_storage_expected", make)


def test_gpu_storage_case_is_all_fast_and_binds():
    """(No GPU.)  From the model: every row and every spec of the case is fast, and the two
    extra columns change the total of at least a quarter of the specs and leave at least
    one as it was."""
    r6, ax, ux, sc, sm, sx = gpu_storage_case()
    n, S = r6[0].size, sc.size
    assert all(xm.row_is_fast(int(r6[0][i]), int(r6[1][i]), int(r6[4][i]), int(r6[5][i]),
                              ax[:, i], ux[:, i]) for i in range(n))
    assert all(xm.spec_is_fast(int(sc[s]), int(sm[s]), sx[:, s]) for s in range(S))
    q, dz, q0, dz0 = gpu_storage_expected()
    assert not dz.any() and not dz0.any()
    t, _ = xm.totals_from_pairs(q, dz)
    t0, _ = xm.totals_from_pairs(q0, dz0)
    changed = int((t != t0).sum())
    print("specs changed / unchanged:", changed, S - changed,
          "pairs lowered: %.1f %%" % (100.0 * (q != q0).mean()))
    assert 4 * changed >= S and changed < S


@pytest.mark.gpu
def test_gpu_ext_gpu_and_storage_columns_all_fast(eng):
    r6, ax, ux, sc, sm, sx = gpu_storage_case()
    q, dz, q0, dz0 = gpu_storage_expected()
    t, e = eng.fit_ext(*r6, ax, ux, sc, sm, sx)
    mt, me = xm.totals_from_pairs(q, dz)
    assert np.array_equal(e, me) and np.array_equal(t, mt) and not e.any()
    t0, e0 = eng.total_possible_max_replicas(*r6, sc, sm)
    changed = int((t != t0).sum())
    assert 4 * changed >= sc.size and changed < sc.size
    gid = group_ids(r6[0].size, 7, 3)
    t, e = eng.fit_ext(*r6, ax, ux, sc, sm, sx, gid, 7)
    mt, me = xm.totals_from_pairs(q, dz, gid, 7)
    assert np.array_equal(e, me) and np.array_equal(t, mt)


# ---- the fast path's bounds ----------------------------------------------------------------
def edge_case():
    """Rows whose free extra amount is k x + {-1, 0, 1} for every edge divisor x, up to
    2^50 - 1, and the first non-fast amount 2^50; free CPU 2^31 - 1 and free memory 2^50 - 1
    under c = m = 1, so the extra quotient decides wherever it is below 2^31 - 1; the pod
    limit is out of the way (2^62) except on every seventh row."""
    def make():
        xs = [1, 3, (1 << 26) - 1, (1 << 26) + 1, (1 << 52) - 1, 1 << 52]
        top = (1 << 50) - 1
        fx = {0, 1, 2, top - 1, top, top + 1}
        for x in xs:
            for k in (0, 1, 2, 1000, (1 << 31) - 2, (1 << 31) - 1, top // x):
                fx.update(v for v in (k * x - 1, k * x, k * x + 1) if 0 <= v <= top)
        fx = np.array(sorted(fx), np.int64)
        n = fx.size
        used = np.full(n, 9, np.int64)
        r6 = [np.full(n, (1 << 31) - 1 + 7, np.uint64), np.full(n, (1 << 50) - 1 + 9, np.int64),
              np.where(np.arange(n) % 7 == 0, 5, 1 << 62).astype(np.int64),
              np.full(n, 2, np.int64), np.full(n, 7, np.uint64), used]
        ax = np.stack([fx + 9, fx[::-1] + 9])
        ux = np.stack([used, used])
        # 70 specs: one full wave mixing unrequested and requested lanes, and six lanes
        # beside the lanes past S
        S = 70
        x0 = np.array([(xs + [0])[s % 7] for s in range(S)], np.int64)
        x1 = np.array([([0] + xs)[(s // 7) % 7] for s in range(S)], np.int64)
        sc = np.ones(S, np.uint64)
        sm = np.ones(S, np.int64)
        sc[5::11] = 1000
        sm[3::13] = 1 << 30
        return r6, ax, ux, sc, sm, np.stack([x0, x1])
    return cached("edge", make)


@pytest.mark.gpu
def test_gpu_ext_fast_path_bound_edges(eng):
    r6, ax, ux, sc, sm, sx = edge_case()
    n, S = r6[0].size, sc.size
    assert all(xm.spec_is_fast(int(sc[s]), int(sm[s]), sx[:, s]) for s in range(S))
    fast = [xm.row_is_fast(int(r6[0][i]), int(r6[1][i]), int(r6[4][i]), int(r6[5][i]),
                           ax[:, i], ux[:, i]) for i in range(n)]
    assert sum(fast) == n - 2  # 2^50 once in each column: the first non-fast rows
    q, dz = cached("edge_pairs", lambda: xm.pair_table(r6, ax, ux, sc, sm, sx))
    assert not dz.any() and (q < (1 << 31) - 1).any() and (q == (1 << 31) - 1).any()
    each = np.arange(n, dtype=np.int32)
    for gid, G in ((None, 1), (each, n), ((each % 3).astype(np.int32), 3)):
        t, e = eng.fit_ext(*r6, ax, ux, sc, sm, sx, gid, G)
        mt, me = xm.totals_from_pairs(q, dz, gid, G)
        assert np.array_equal(e, me) and np.array_equal(t, mt), G
    # the first non-fast spec: x = 2^52 + 1 turns its wave exact; same semantics
    sx2 = sx.copy()
    sx2[0, 6] = (1 << 52) + 1
    sx2[1, 69] = (1 << 52) + 1
    assert not xm.spec_is_fast(1, 1, sx2[:, 6]) and not xm.spec_is_fast(1, 1, sx2[:, 69])
    q2, dz2 = cached("edge_pairs2", lambda: xm.pair_table(r6, ax, ux, sc, sm, sx2))
    t, e = eng.fit_ext(*r6, ax, ux, sc, sm, sx2, each, n)
    mt, me = xm.totals_from_pairs(q2, dz2, each, n)
    assert np.array_equal(e, me) and np.array_equal(t, mt)


# ---- identities on the device --------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_ext_identities(eng):
    n, S, R = 1025, 65, 2
    r6 = rows(n)
    ax, ux, sc, sm, sx = case_inputs(n, S, R)
    none_n, none_s = np.zeros((0, n), np.int64), np.zeros((0, S), np.int64)
    base = eng.total_possible_max_replicas(*r6, sc, sm)
    # R = 0 is kcc_fit
    t, e = eng.fit_ext(*r6, none_n, none_n, sc, sm, none_s)
    assert t.shape == (S,) and np.array_equal(t, base[0]) and np.array_equal(e, base[1])
    # R = 0 with groups is kcc_fit_grouped
    for G in (7, 1000):
        gid = group_ids(n, G, 3)
        t, e = eng.fit_ext(*r6, none_n, none_n, sc, sm, none_s, gid, G)
        gt, ge = eng.fit_grouped(*r6, gid, G, sc, sm)
        assert np.array_equal(t, gt) and np.array_equal(e, ge)
    # a resource nobody requests changes nothing
    t, e = eng.fit_ext(*r6, ax, ux, sc, sm, np.zeros_like(sx))
    assert np.array_equal(t, base[0]) and np.array_equal(e, base[1])
    one = sx.copy()
    one[0] = 0
    a = eng.fit_ext(*r6, ax, ux, sc, sm, one)
    b = eng.fit_ext(*r6, ax[1:], ux[1:], sc, sm, one[1:])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], base[0])
    # a copy of the memory column changes nothing, zero and negative requests included
    assert (sm == 0).any() and (sm < 0).any()
    t, e = eng.fit_ext(*r6, r6[1][None], r6[5][None], sc, sm, sm[None])
    assert np.array_equal(t, base[0]) and np.array_equal(e, base[1])
    gid = group_ids(n, 7, 3)
    t, e = eng.fit_ext(*r6, r6[1][None], r6[5][None], sc, sm, sm[None], gid, 7)
    gt, ge = eng.fit_grouped(*r6, gid, 7, sc, sm)
    assert np.array_equal(t, gt) and np.array_equal(e, ge)
    # a spec's unflagged cells sum (wrapping) to the ungrouped call on the rows not skipped
    for G in (2, 1000):
        gid = group_ids(n, G, 3)
        keep = (gid >= 0) & (gid < G)
        t, e = eng.fit_ext(*r6, ax, ux, sc, sm, sx, gid, G)
        wt, we = eng.fit_ext(*[a[keep] for a in r6], ax[:, keep], ux[:, keep], sc, sm, sx)
        ok = ~(e != 0).any(axis=0)
        assert ok.any() and (~ok).any() and np.array_equal(we != 0, ~ok)
        assert np.array_equal(t.view(np.uint64).sum(axis=0, dtype=np.uint64)[ok],
                              wt.view(np.uint64)[ok])


# ---- plumbing ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_ext_degenerate(eng):
    n, S, R = 257, 65, 2
    r6 = rows(n)
    ax, ux, sc, sm, sx = case_inputs(n, S, R)
    empty = [a[:0] for a in r6]
    t, e = eng.fit_ext(*empty, ax[:, :0], ux[:, :0], sc, sm, sx)
    assert t.shape == (S,) and not t.any() and not e.any()
    t, e = eng.fit_ext(*empty, ax[:, :0], ux[:, :0], sc, sm, sx, np.zeros(0, np.int32), 5)
    assert t.shape == (5, S) and not t.any() and not e.any()
    t, e = eng.fit_ext(*r6, ax, ux, sc[:0], sm[:0], sx[:, :0])
    assert t.shape == (0,) and e.shape == (0,)
    t, e = eng.fit_ext(*r6, ax, ux, sc[:0], sm[:0], sx[:, :0], np.zeros(n, np.int32), 5)
    assert t.shape == (5, 0) and e.shape == (5, 0)
    # empty groups, every id invalid
    q, dz = pairs(n, S, R)
    gid = (np.arange(n) % 2 * 4).astype(np.int32)  # groups 0 and 4 of 6
    t, e = eng.fit_ext(*r6, ax, ux, sc, sm, sx, gid, 6)
    mt, me = xm.totals_from_pairs(q, dz, gid, 6)
    assert np.array_equal(t, mt) and np.array_equal(e, me)
    assert not t[[1, 2, 3, 5]].any() and not e[[1, 2, 3, 5]].any()
    for bad in (-1, 3):
        t, e = eng.fit_ext(*r6, ax, ux, sc, sm, sx, np.full(n, bad, np.int32), 3)
        assert t.shape == (3, S) and not t.any() and not e.any()


@pytest.mark.gpu
def test_gpu_ext_argument_errors(eng):
    a = [np.zeros(4, t) for t in (np.uint64, np.int64, np.int64, np.int64, np.uint64, np.int64)]
    gid = np.zeros(4, np.int32)
    ax, ux = np.zeros(16, np.int64), np.zeros(16, np.int64)
    sc, sm, sx = np.ones(2, np.uint64), np.ones(2, np.int64), np.ones(8, np.int64)
    t, e = np.zeros(8, np.int64), np.zeros(8, np.int32)
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)  # noqa: E731

    def call(n=4, R=2, AX=ax, UX=ux, group=gid, G=4, S=2, SX=sx):
        rc = eng._lib.kcc_fit_ext(eng._h, n, *[p(x) for x in a], R, p(AX), p(UX), p(group), G, S,
                                  p(sc), p(sm), p(SX), p(t), p(e))
        return rc, eng._lib.kcc_last_error(eng._h).decode()

    bad = [dict(R=-1), dict(R=5), dict(R=1 << 40),               # n_ext outside [0, 4]
           dict(AX=None), dict(UX=None), dict(SX=None),           # NULL extra array, n_ext > 0
           dict(R=4, AX=None, UX=None, SX=None),
           dict(group=None, G=4), dict(group=None, G=0), dict(group=None, G=2),
           dict(G=0), dict(G=-1), dict(G=(1 << 27) + 1), dict(G=1 << 28),  # G x S > 2^28
           dict(G=1 << 62, S=1 << 62),
           dict(n=(1 << 31) - 4095), dict(n=-1), dict(S=-1)]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == _lib.KCC_EINVAL and msg, kw
    for kw in (dict(), dict(group=None, G=1), dict(R=0, AX=None, UX=None, SX=None),
               dict(R=4), dict(n=0, AX=None, UX=None, group=None, G=1)):
        rc, msg = call(**kw)  # the same buffers with valid arguments
        assert rc == 0, (kw, msg)
    from kubernetesclustercapacity_amd import KccError
    with pytest.raises(KccError):
        eng.fit_ext(*a, np.zeros((5, 4), np.int64), np.zeros((5, 4), np.int64), sc, sm,
                    np.zeros((5, 2), np.int64))
    with pytest.raises(KccError):
        eng.fit_ext(*a, ax.reshape(4, 4), ux.reshape(4, 4), sc, sm, sx.reshape(4, 2), None, 3)


@pytest.mark.gpu
def test_gpu_ext_workspace_reuse():
    """A small call after a call that grew every buffer, and the large call right after a
    small one on a fresh engine: the same answers as on the module's engine."""
    from kubernetesclustercapacity_amd import CapacityEngine
    small = (65, 65, 2)
    large = (1025, 65, 4)

    def run(e, n, S, R, G):
        ax, ux, sc, sm, sx = case_inputs(n, S, R)
        gid = None if G is None else group_ids(n, G, 3)
        return e.fit_ext(*rows(n), ax, ux, sc, sm, sx, gid, 1 if G is None else G)

    def want(n, S, R, G):
        q, dz = pairs(n, S, R)
        return xm.totals_from_pairs(q, dz, None if G is None else group_ids(n, G, 3),
                                    1 if G is None else G)

    for G_small, G_large in ((None, 1000), (7, None)):
        with CapacityEngine(0, 1) as a:
            first = run(a, *small, G_small)
            big = run(a, *large, G_large)      # large after small, fresh engine
            again = run(a, *small, G_small)    # small after large
        for got, exp in ((first, want(*small, G_small)), (big, want(*large, G_large)),
                         (again, want(*small, G_small))):
            assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


@pytest.mark.gpu
def test_gpu_ext_async_on_torch_tensors(eng):
    import torch
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.array(a).view(  # noqa: E731  (a copy: the cache is read-only)
        np.int64 if a.dtype == np.uint64 else a.dtype)).to(dev)
    cases = []
    for n, S, R, G in [(1025, 65, 2, None), (257, 64, 2, 1000), (1025, 65, 4, 7)]:
        ax, ux, sc, sm, sx = case_inputs(n, S, R)
        gid = None if G is None else group_ids(n, G, 3)
        g1 = 1 if G is None else G
        d = [T(a) for a in rows(n)] + [R, T(ax), T(ux), None if gid is None else T(gid), g1,
                                       T(sc), T(sm), T(sx)]
        out = (torch.full((g1 * S,), 77, dtype=torch.int64, device=dev),
               torch.full((g1 * S,), 77, dtype=torch.int32, device=dev))
        q, dz = pairs(n, S, R)
        exp = xm.totals_from_pairs(q, dz, gid, g1)
        cases.append((d, out, exp))
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        for d, out, _ in cases:
            eng.fit_ext_async(*d, out[0], out[1], stream=stream)
    stream.synchronize()
    for _, out, exp in cases:
        assert np.array_equal(out[0].cpu().numpy().reshape(exp[0].shape), exp[0])
        assert np.array_equal(out[1].cpu().numpy().reshape(exp[1].shape), exp[1])
    # R = 0 with NULL extra pointers, outputs pre-filled
    n, S = 257, 64
    _, _, sc, sm, _ = case_inputs(n, S, 2)
    out = (torch.full((S,), 77, dtype=torch.int64, device=dev),
           torch.full((S,), 77, dtype=torch.int32, device=dev))
    eng.fit_ext_async(*[T(a) for a in rows(n)], 0, None, None, None, 1, T(sc), T(sm), None,
                      out[0], out[1])
    torch.cuda.synchronize()
    bt, be = eng.total_possible_max_replicas(*rows(n), sc, sm)
    assert np.array_equal(out[0].cpu().numpy(), bt) and np.array_equal(out[1].cpu().numpy(), be)
