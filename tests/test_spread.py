"""Spread constraints on the GPU (kcc_fit_capped, kcc_spread_fold): every
cell of totals / err / cell_min and every group_rows entry against tests/spread_model.py
(the semantics in Python integers) over tests/test_ext.py's inputs and cached pair tables —
sizes around the 64-lane wave, the 256-record run and the 1024-row sort workgroup; R = 0, 2,
4; no groups and 2 to 1025 groups with skipped ids; caps that bind, caps that do not and
non-positive caps; the identities with kcc_fit_ext; the fold over device cells with and
without a domain map, an eligibility mask and a maxSkew; degenerate inputs, argument errors,
workspace reuse, the device forms and fit_spread.  All comparisons are integer equality."""
import ctypes as C

import numpy as np
import pytest

from kubernetesclustercapacity_amd import _lib
from kubernetesclustercapacity_amd.engine import select_groups
from tests import spread_model as sp
from tests.test_ext import ALL_N, ALL_S, cached, case_inputs, pairs, rows
from tests.test_groups import group_ids

I64 = np.iinfo(np.int64)
ALL_R = [0, 2, 4]
ALL_G = [None, 2, 7, 1000, 1025]
CAPS = [0, -3, 1, 2, 110, I64.max]
SKEWS = [0, 1, 2, 5, I64.max]


@pytest.fixture(scope="module")
def eng():
    from tests.conftest import init_torch_first
    init_torch_first()
    from kubernetesclustercapacity_amd import CapacityEngine
    with CapacityEngine(0, 1) as e:
        yield e


# ---- inputs (computed once, never modified) ------------------------------------------------
def node_caps(S):
    """One of CAPS per spec, every value present once S >= 6."""
    return cached(("caps", S), lambda: np.array([CAPS[(s * 5 + 1) % 6] for s in range(S)], np.int64))


def skews(S):
    return cached(("skews", S), lambda: np.array([SKEWS[(s * 3 + 1) % 5] for s in range(S)], np.int64))


def want_cells(n, S, R, G, ordinary=False, capped=True):
    """The model's (totals, err, cell_min, group_rows) of a case."""
    def make():
        q, dz = pairs(n, S, R, ordinary)
        gid = None if G is None else group_ids(n, G, 3)
        return sp.capped_cells(q, dz, gid, 1 if G is None else G, node_caps(S) if capped else None)
    return cached(("cells", n, S, R, G, ordinary, capped), make)


def domain_map(G, D):
    """Groups onto D domains, many to one, a few ids outside [0, D)."""
    def make():
        rng = np.random.default_rng([G, D, 0xD0])
        dom = rng.integers(0, D, G).astype(np.int32)
        k = rng.choice(G, min(G, 6), replace=False)
        dom[k[:3]] = -1
        dom[k[3:]] = D + 2
        return dom
    return cached(("dom", G, D), make)


def eligibility(G, S):
    """About 70 % of the cells, specs 3 and S - 2 eligible nowhere."""
    def make():
        el = np.random.default_rng([G, S, 0xE1]).random((G, S)) < 0.7
        el[:, 3 % S] = False
        el[:, (S - 2) % S] = False
        return el
    return cached(("el", G, S), make)


def check_case(eng, n, S, R, G=None, ordinary=False):
    """One device call against the model; G None: no group ids."""
    ax, ux, sc, sm, sx = case_inputs(n, S, R, ordinary)
    gid = None if G is None else group_ids(n, G, 3)
    got = eng.fit_capped(*rows(n), ax, ux, sc, sm, sx, gid, 1 if G is None else G, node_caps(S))
    exp = want_cells(n, S, R, G, ordinary)
    for name, g, w in zip(("totals", "err", "cell_min", "group_rows"), got, exp):
        assert g.shape == w.shape and g.dtype == w.dtype, (name, n, S, R, G)
        assert np.array_equal(g, w), (name, n, S, R, G)
    return got


# ---- the pair pass -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", ALL_N)
def test_gpu_capped_every_n(eng, n):
    check_case(eng, n, 65, 2)
    check_case(eng, n, 65, 2, G=7)
    check_case(eng, n, 65, 2, ordinary=True)


@pytest.mark.gpu
@pytest.mark.parametrize("S", ALL_S)
def test_gpu_capped_every_s(eng, S):
    check_case(eng, 257, S, 2)
    check_case(eng, 257, S, 2, G=7)
    check_case(eng, 257, S, 2, ordinary=True)


@pytest.mark.gpu
@pytest.mark.parametrize("R", ALL_R)
@pytest.mark.parametrize("G", ALL_G)
def test_gpu_capped_every_r_and_group_form(eng, R, G):
    n, S = 1025, 65
    t, e, m, r = check_case(eng, n, S, R, G)
    assert (e != 0).any() and (e == 0).any() and (t < 0).any() and (t > 0).any()
    assert (m < 0).any() and r.sum() == (n if G is None else
                                         ((group_ids(n, G, 3) >= 0) & (group_ids(n, G, 3) < G)).sum())
    if G is not None and G >= 1000:
        assert (r == 0).any() and (m[r == 0] == I64.max).all()  # empty groups: the identity
    t, e, m, r = check_case(eng, n, S, R, G, ordinary=True)
    assert not e.any() and (t > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("ordinary", [False, True])
def test_gpu_capped_identities(eng, ordinary):
    n, S, R = 1025, 65, 2
    ax, ux, sc, sm, sx = case_inputs(n, S, R, ordinary)
    for G in (None, 7, 1000):
        gid = None if G is None else group_ids(n, G, 3)
        g1 = 1 if G is None else G
        base = eng.fit_ext(*rows(n), ax, ux, sc, sm, sx, gid, g1)
        # every optional argument NULL is kcc_fit_ext
        t, e, m, r = eng.fit_capped(*rows(n), ax, ux, sc, sm, sx, gid, g1, None, want_min=False,
                                    want_rows=False)
        assert m is None and r is None
        assert np.array_equal(t, base[0]) and np.array_equal(e, base[1])
        # a cap nothing exceeds, and non-positive caps, are no cap; the minima do not change it
        for cap in (np.full(S, I64.max, np.int64), np.zeros(S, np.int64), np.full(S, -3, np.int64)):
            t, e, m, r = eng.fit_capped(*rows(n), ax, ux, sc, sm, sx, gid, g1, cap)
            assert np.array_equal(t, base[0]) and np.array_equal(e, base[1])
            w = want_cells(n, S, R, G, ordinary, capped=False)
            assert np.array_equal(m, w[2]) and np.array_equal(r, w[3])
        # group_rows alone rides on kcc_fit_ext's launches
        t, e, m, r = eng.fit_capped(*rows(n), ax, ux, sc, sm, sx, gid, g1, None, want_min=False)
        assert np.array_equal(t, base[0]) and np.array_equal(e, base[1])
        assert np.array_equal(r, want_cells(n, S, R, G, ordinary, capped=False)[3])


# ---- the fold on device cells --------------------------------------------------------------
def fold_variants(G, S):
    """(domain_of, D, eligible, max_skew) of every fold case over G x S cells."""
    out = [(None, G, None, None), (None, G, None, skews(S)), (None, G, eligibility(G, S), skews(S))]
    for D in (3, G):
        out += [(domain_map(G, D), D, None, skews(S)),
                (domain_map(G, D), D, eligibility(G, S), skews(S)),
                (domain_map(G, D), D, eligibility(G, S), None)]
    for k in SKEWS:
        out.append((domain_map(G, 3), 3, eligibility(G, S), np.full(S, k, np.int64)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ordinary", [False, True])
def test_gpu_fold_on_device_cells(eng, ordinary):
    n, S, R, G = 1025, 65, 2, 1000
    ax, ux, sc, sm, sx = case_inputs(n, S, R, ordinary)
    t, e, m, r = eng.fit_capped(*rows(n), ax, ux, sc, sm, sx, group_ids(n, G, 3), G, node_caps(S))
    w = want_cells(n, S, R, G, ordinary)
    assert np.array_equal(t, w[0]) and np.array_equal(e, w[1]) and np.array_equal(r, w[3])
    for dom, D, el, sk in fold_variants(G, S):
        for gr in (r, None):
            got = eng.spread_fold(t, e, gr, dom, D, el, sk)
            exp = sp.fold(t, e, gr, dom, D, el, sk)
            key = (D, dom is None, el is None, None if sk is None else int(sk[0]), gr is None)
            assert np.array_equal(got[1], exp[1]), key
            assert np.array_equal(got[0], exp[0]), key
    # unconstrained over each group as its own domain is select_groups on the same mask
    el = eligibility(G, S)
    got = eng.spread_fold(t, e, None, None, G, el, None)
    st, se = select_groups(t, e, el)
    assert np.array_equal(got[0], st) and np.array_equal(got[1], se)


@pytest.mark.gpu
def test_gpu_fold_small_shapes(eng):
    """One spec over many groups (the slices of fold_cells), one group, and sizes around the
    256-spec workgroup, on made-up cells."""
    rng = np.random.default_rng(11)
    for G, S, D in ((4096, 1, 3), (1, 65, 1), (5, 255, 2), (7, 256, 7), (3, 257, 2), (1025, 3, 40)):
        t = rng.integers(-50, 2000, (G, S), dtype=np.int64)
        t[rng.random((G, S)) < 0.02] = I64.max - 3
        e = (rng.random((G, S)) < 0.001).astype(np.int32)
        gr = rng.integers(0, 4, G).astype(np.int64)
        dom = rng.integers(-1, D + 1, G).astype(np.int32)
        el = rng.random((G, S)) < 0.7
        sk = rng.choice(np.array(SKEWS, np.int64), S)
        got = eng.spread_fold(t, e, gr, dom, D, el, sk)
        exp = sp.fold(t, e, gr, dom, D, el, sk)
        assert np.array_equal(got[1], exp[1]) and np.array_equal(got[0], exp[0]), (G, S, D)
    # the issue's example, and the saturating limit
    z = np.zeros((3, 1), np.int32)
    t, _ = eng.spread_fold(np.array([[10], [4], [7]]), z, max_skew=[1])
    assert t.tolist() == [14]
    t, _ = eng.spread_fold(np.array([[I64.max - 1], [I64.max]]), z[:2], max_skew=[5])
    assert t.tolist() == [sp.i64(2 * I64.max - 1)]  # lim = MaxInt64, not a wrapped m + 5


# ---- plumbing ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_spread_degenerate(eng):
    n, S, R = 257, 65, 2
    r6 = rows(n)
    ax, ux, sc, sm, sx = case_inputs(n, S, R)
    cap = node_caps(S)
    empty = [a[:0] for a in r6]
    t, e, m, r = eng.fit_capped(*empty, ax[:, :0], ux[:, :0], sc, sm, sx, None, 1, cap)
    assert t.shape == (S,) and not t.any() and not e.any() and (m == I64.max).all()
    assert r.tolist() == [0]
    t, e, m, r = eng.fit_capped(*empty, ax[:, :0], ux[:, :0], sc, sm, sx, np.zeros(0, np.int32), 5, cap)
    assert t.shape == (5, S) and not t.any() and not e.any() and (m == I64.max).all()
    assert r.tolist() == [0] * 5
    gid = group_ids(n, 5, 3)
    t, e, m, r = eng.fit_capped(*r6, ax, ux, sc[:0], sm[:0], sx[:, :0], gid, 5, cap[:0])
    assert t.shape == (5, 0) and m.shape == (5, 0)
    assert r.tolist() == np.bincount(gid[(gid >= 0) & (gid < 5)], minlength=5).tolist()
    t, e, m, r = eng.fit_capped(*r6, ax, ux, sc[:0], sm[:0], sx[:, :0], None, 1, cap[:0])
    assert t.shape == (0,) and r.tolist() == [n]
    # every id invalid: no rows anywhere
    t, e, m, r = eng.fit_capped(*r6, ax, ux, sc, sm, sx, np.full(n, -1, np.int32), 3, cap)
    assert not t.any() and not e.any() and (m == I64.max).all() and not r.any()
    # the fold: no groups, no specs, no live group
    t, e = eng.spread_fold(np.zeros((0, 4), np.int64), np.zeros((0, 4), np.int32), max_skew=[1] * 4)
    assert t.tolist() == [0] * 4 and e.tolist() == [0] * 4
    t, e = eng.spread_fold(np.zeros((4, 0), np.int64), np.zeros((4, 0), np.int32))
    assert t.shape == (0,) and e.shape == (0,)
    cells, flags = np.full((4, 2), 9, np.int64), np.ones((4, 2), np.int32)
    t, e = eng.spread_fold(cells, flags, np.zeros(4, np.int64), max_skew=[1, 0])
    assert t.tolist() == [0, 0] and e.tolist() == [0, 0]  # an empty group's flag does not count
    t, e = eng.spread_fold(cells, flags, None, np.full(4, 7, np.int32), 3, None, [1, 0])
    assert t.tolist() == [0, 0] and e.tolist() == [0, 0]


@pytest.mark.gpu
def test_gpu_spread_argument_errors(eng):
    a = [np.zeros(4, t) for t in (np.uint64, np.int64, np.int64, np.int64, np.uint64, np.int64)]
    gid = np.zeros(4, np.int32)
    ax, ux = np.zeros(16, np.int64), np.zeros(16, np.int64)
    sc, sm, sx = np.ones(2, np.uint64), np.ones(2, np.int64), np.ones(8, np.int64)
    t, e = np.zeros(8, np.int64), np.zeros(8, np.int32)
    cap, cm, gr = np.ones(2, np.int64), np.zeros(8, np.int64), np.zeros(4, np.int64)
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)  # noqa: E731

    def capped(n=4, R=2, AX=ax, UX=ux, group=gid, G=4, S=2, SX=sx, CAP=cap, CM=cm, GR=gr):
        rc = eng._lib.kcc_fit_capped(eng._h, n, *[p(x) for x in a], R, p(AX), p(UX), p(group), G,
                                     S, p(sc), p(sm), p(SX), p(t), p(e), p(CAP), p(CM), p(GR))
        return rc, eng._lib.kcc_last_error(eng._h).decode()

    bad = [dict(R=-1), dict(R=5), dict(R=1 << 40), dict(AX=None), dict(UX=None), dict(SX=None),
           dict(R=4, AX=None, UX=None, SX=None),
           dict(group=None, G=4), dict(group=None, G=0), dict(group=None, G=2),
           dict(G=0), dict(G=-1), dict(G=(1 << 27) + 1), dict(G=1 << 28),
           dict(G=1 << 62, S=1 << 62), dict(n=(1 << 31) - 4095), dict(n=-1), dict(S=-1)]
    for kw in bad:
        rc, msg = capped(**kw)
        assert rc == _lib.KCC_EINVAL and msg, kw
    for kw in (dict(), dict(group=None, G=1), dict(R=0, AX=None, UX=None, SX=None), dict(R=4),
               dict(CAP=None), dict(CM=None), dict(GR=None), dict(CAP=None, CM=None, GR=None),
               dict(n=0, AX=None, UX=None, group=None, G=1)):
        rc, msg = capped(**kw)  # the same buffers with valid arguments
        assert rc == 0, (kw, msg)

    ct, ce = np.zeros(8, np.int64), np.zeros(8, np.int32)
    dom, el, sk = np.zeros(4, np.int32), np.ones(8, np.uint8), np.ones(2, np.int64)
    ot, oe = np.zeros(2, np.int64), np.zeros(2, np.int32)

    def fold(G=4, S=2, CT=ct, CE=ce, GR=gr, DOM=dom, D=3, EL=el, SK=sk, OT=ot, OE=oe):
        rc = eng._lib.kcc_spread_fold(eng._h, G, S, p(CT), p(CE), p(GR), p(DOM), D, p(EL), p(SK),
                                      p(OT), p(OE))
        return rc, eng._lib.kcc_last_error(eng._h).decode()

    bad = [dict(D=0), dict(D=-1), dict(DOM=None, D=3), dict(DOM=None, D=5),
           dict(G=(1 << 27) + 1), dict(G=1 << 62, S=1 << 62),     # G x S > 2^28
           dict(D=(1 << 27) + 1), dict(D=1 << 62),                # D x S > 2^28
           dict(G=-1), dict(S=-1), dict(CT=None), dict(CE=None), dict(OT=None), dict(OE=None)]
    for kw in bad:
        rc, msg = fold(**kw)
        assert rc == _lib.KCC_EINVAL and msg, kw
    for kw in (dict(), dict(DOM=None, D=4), dict(GR=None), dict(EL=None), dict(SK=None),
               dict(G=0, D=0, DOM=None), dict(S=0, OT=None, OE=None), dict(D=1000)):
        rc, msg = fold(**kw)
        assert rc == 0, (kw, msg)


@pytest.mark.gpu
def test_gpu_spread_workspace_reuse():
    """A small call after a call that grew every buffer, and the large call right after a
    small one on a fresh engine: the same answers as the model's."""
    from kubernetesclustercapacity_amd import CapacityEngine
    small = (65, 65, 2)
    large = (1025, 65, 4)

    def run(e, n, S, R, G):
        ax, ux, sc, sm, sx = case_inputs(n, S, R)
        gid = None if G is None else group_ids(n, G, 3)
        g1 = 1 if G is None else G
        cells = e.fit_capped(*rows(n), ax, ux, sc, sm, sx, gid, g1, node_caps(S))
        dom = None if G is None else domain_map(G, 3)
        D = 1 if G is None else 3
        f = e.spread_fold(cells[0].reshape(g1, S), cells[1].reshape(g1, S), cells[3], dom, D, None,
                          skews(S))
        return cells, f

    def want(n, S, R, G):
        w = want_cells(n, S, R, G)
        g1 = 1 if G is None else G
        dom = None if G is None else domain_map(G, 3)
        return w, sp.fold(w[0].reshape(g1, S), w[1].reshape(g1, S), w[3], dom, 1 if G is None else 3,
                          None, skews(S))[:2]

    for G_small, G_large in ((None, 1000), (7, None)):
        with CapacityEngine(0, 1) as a:
            first = run(a, *small, G_small)
            big = run(a, *large, G_large)      # large after small, fresh engine
            again = run(a, *small, G_small)    # small after large
        for got, exp in ((first, want(*small, G_small)), (big, want(*large, G_large)),
                         (again, want(*small, G_small))):
            for g, w in zip(list(got[0]) + list(got[1]), list(exp[0]) + list(exp[1])):
                assert np.array_equal(g, w)


@pytest.mark.gpu
def test_gpu_spread_async_on_torch_tensors(eng):
    import torch
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.array(a).view(  # noqa: E731  (a copy: the cache is read-only)
        np.int64 if a.dtype == np.uint64 else a.dtype)).to(dev)
    cases = []
    for n, S, R, G in [(1025, 65, 2, None), (257, 64, 2, 1000), (1025, 65, 4, 7)]:
        ax, ux, sc, sm, sx = case_inputs(n, S, R)
        gid = None if G is None else group_ids(n, G, 3)
        g1 = 1 if G is None else G
        D = 1 if G is None else 3
        dom = None if G is None else domain_map(G, D)
        el = eligibility(g1, S)
        d = [T(a) for a in rows(n)] + [R, T(ax), T(ux), None if gid is None else T(gid), g1,
                                       T(sc), T(sm), T(sx)]
        full = lambda k, t: torch.full((k,), 77, dtype=t, device=dev)  # noqa: E731
        out = dict(t=full(g1 * S, torch.int64), e=full(g1 * S, torch.int32),
                   m=full(g1 * S, torch.int64), r=full(g1, torch.int64),
                   ft=full(S, torch.int64), fe=full(S, torch.int32))
        fold_in = (None if dom is None else T(dom), D, T(el.astype(np.uint8)), T(skews(S)))
        w = want_cells(n, S, R, G)
        wf = sp.fold(w[0].reshape(g1, S), w[1].reshape(g1, S), w[3], dom, D, el, skews(S))
        cases.append((d, T(node_caps(S)), out, fold_in, g1, S, w, wf))
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        for d, cap, out, (dom, D, el, sk), g1, S, _, _ in cases:
            eng.fit_capped_async(*d, out["t"], out["e"], cap, out["m"], out["r"], stream=stream)
            eng.spread_fold_async(g1, S, out["t"], out["e"], out["r"], dom, D, el, sk, out["ft"],
                                  out["fe"], stream=stream)
    stream.synchronize()
    for _, _, out, _, g1, S, w, wf in cases:
        for key, exp in zip(("t", "e", "m", "r"), w):
            assert np.array_equal(out[key].cpu().numpy().reshape(exp.shape), exp), key
        assert np.array_equal(out["fe"].cpu().numpy(), wf[1])
        assert np.array_equal(out["ft"].cpu().numpy(), wf[0])
    # every optional pointer NULL: kcc_fit_ext_async's outputs, pre-filled buffers
    d, _, out, _, g1, S, _, _ = cases[2]
    ref = (torch.full_like(out["t"], 55), torch.full_like(out["e"], 55))
    eng.fit_ext_async(*d, ref[0], ref[1])
    eng.fit_capped_async(*d, out["t"], out["e"])
    torch.cuda.synchronize()
    assert torch.equal(out["t"], ref[0]) and torch.equal(out["e"], ref[1])


@pytest.mark.gpu
@pytest.mark.parametrize("G", [None, 7])
def test_gpu_fit_spread_against_the_model(eng, G):
    n, S, R = 1025, 65, 2
    ax, ux, sc, sm, sx = case_inputs(n, S, R, ordinary=True)
    q, dz = pairs(n, S, R, True)
    gid = None if G is None else group_ids(n, G, 3)
    g1 = 1 if G is None else G
    zone = None if G is None else np.array([0, 1, 2, 0, 1, 2, 5], np.int32)  # group 6: no zone
    D = 1 if G is None else 3
    el = None if G is None else eligibility(G, S)
    cap = node_caps(S)
    hk = np.array([[0, 1, 3, I64.max][s % 4] for s in range(S)], np.int64)
    # zone spread and a per-node cap
    got = eng.fit_spread(*rows(n), ax, ux, sc, sm, sx, gid, g1, cap, zone, skews(S), el, n_zones=D)
    c = sp.capped_cells(q, dz, gid, g1, cap)
    exp = sp.fold(c[0].reshape(g1, S), c[1].reshape(g1, S), c[3], zone, D, el, skews(S))
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    # and a hostname-level spread on top: two pair passes
    got = eng.fit_spread(*rows(n), ax, ux, sc, sm, sx, gid, g1, cap, zone, skews(S), el, hk, n_zones=D)
    cap2 = sp.host_cap(c[2].reshape(g1, S), c[3], hk, cap, zone, D, el)
    assert (cap2 != cap).any() and (cap2 > 0).any()
    c2 = sp.capped_cells(q, dz, gid, g1, cap2)
    exp2 = sp.fold(c2[0].reshape(g1, S), c2[1].reshape(g1, S), c2[3], zone, D, el, skews(S))
    assert np.array_equal(got[0], exp2[0]) and np.array_equal(got[1], exp2[1])
    assert (exp2[0] < exp[0]).any()  # the hostname spread binds somewhere
