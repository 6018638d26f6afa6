"""kcc_fit_explain on the GPU, bit for bit against tests/explain_model.py:
which term binds each node (why_rows / why_pods) and what is left over (left), at the GRP_RUN,
wave and sblocks edges, R = 0..4, with and without group ids; the identities with
kcc_fit_capped; the nullable outputs; the degenerate and EINVAL cases; the async form in a
graph, alone and behind kcc_deploy_async; a small seeded fuzz.

The input generators are used by tests/test_explain_cpu.py too, which checks on the model that
they reach every slot on fast and on exact pairs and hit every tie."""
import ctypes as C

import numpy as np
import pytest

from kubernetesclustercapacity_amd import _lib
from tests import explain_model as em

I64 = np.iinfo(np.int64)
GIB = 1 << 30
RUN = 256  # kcc_internal.h GRP_RUN
ALL_N = [1, 64, RUN - 1, RUN, RUN + 1, 2 * RUN + 1]
ALL_S = [1, 63, 64, 65, 257]
S3 = 130  # three waves: one with the special specs (exact path), one without, one of two lanes
# the tie spec: a row with free amounts k x these has every quotient equal to k
TIE_C, TIE_M, TIE_X = 500, GIB, [1, 10 * GIB, 2, 5]
TIE_CAP = 7
BIG_K = 5_000_000  # 500 x BIG_K >= 2^31: a tie row off the fast path


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
        _CACHE[key] = fn()
    return _CACHE[key]


def make_rows(n, R, seed=7):
    """Six node columns and alloc_x / used_x [R, n].  Ordinary rows (a scarce resource each,
    a few full, pod counts up to and past the limit) and, at fixed positions (mod n), tie rows
    for the tie spec, rows off the fast path (free CPU >= 2^31, free memory >= 2^50, a negative
    free amount, a free extra amount >= 2^50), full rows and rows over their pod limit."""
    rng = np.random.default_rng([seed, n, R])
    ac = rng.choice([2000, 4000, 8000, 16000, 64000], n).astype(np.uint64)
    uc = (ac * rng.random(n) * 0.9).astype(np.uint64)
    am = rng.choice([4, 8, 16, 64, 256], n).astype(np.int64) * GIB
    um = (am * rng.random(n) * 0.9).astype(np.int64)
    ap = rng.choice([110, 30, 10, 4], n).astype(np.int64)
    pc = (ap * rng.random(n)).astype(np.int64)
    over = rng.random(n) < 0.08
    pc[over] = ap[over] + rng.integers(0, 4, int(over.sum()))
    ax = np.zeros((R, n), np.int64)
    ux = np.zeros((R, n), np.int64)
    for r in range(R):
        if r % 2 == 0:  # device counts
            ax[r] = rng.integers(0, 9, n)
            ux[r] = np.minimum(rng.integers(0, 9, n), ax[r] + 1)
        else:           # bytes
            ax[r] = rng.choice([50, 200, 2000], n) * GIB
            ux[r] = (ax[r] * rng.random(n)).astype(np.int64)
    scarce = rng.integers(0, 2 + R + 2, n)  # rows short of one resource
    for i in range(n):
        k = int(scarce[i])
        if k == 0:
            uc[i] = ac[i] - np.uint64(rng.integers(0, 700))
        elif k == 1:
            um[i] = am[i] - rng.integers(0, GIB)
        elif k < 2 + R:
            ux[k - 2, i] = ax[k - 2, i] - min(int(ax[k - 2, i]), int(rng.integers(0, 3)))

    def put(k, fc, fm, fx, pods, count):
        i = (3 + 5 * k) % n
        ac[i], uc[i] = np.uint64(fc + 77 if fc > 0 else 77), np.uint64(77 if fc > 0 else 77 - fc)
        am[i], um[i] = (fm + 5, 5) if fm > 0 else (5, 5 - fm)
        ap[i], pc[i] = pods, count
        for r in range(R):
            f = fx[r] if isinstance(fx, list) else fx
            ax[r, i], ux[r, i] = (f + 1, 1) if f > 0 else (1, 1 - f)
        return i

    tie = lambda k: (TIE_C * k, TIE_M * k, [x * k for x in TIE_X])  # noqa: E731
    put(0, *tie(3), 110, 0)                 # every quotient 3: CPU holds the tie
    put(1, *tie(7), 7, 2)                   # q == alloc_pods: the clamp fires
    put(2, *tie(7), 110, 0)                 # q == node_cap of the tie spec: the cap does not
    put(3, *tie(9), 110, 0)                 # q above that cap
    put(4, (1 << 31) + 12345, 1 << 40, 1 << 20, 110, 3)   # free CPU off the fast path
    put(5, 32000, (1 << 50) + GIB, 1 << 20, 110, 3)       # free memory off the fast path
    i = put(6, 32000, 1, 1 << 20, 110, 3)
    am[i], um[i] = I64.max, -(1 << 40)                    # the free memory wraps negative
    put(7, 0, 64 * GIB, 8, 110, 0)          # no CPU left
    put(8, 32000, -3, 8, 110, 0)            # memory over-used
    put(9, 64000, 256 * GIB, 1 << 40, 10, 17)   # over its pod limit: the clamp value is -7
    put(10, 64000, 256 * GIB, 1 << 40, -3, 2)   # a negative pod limit
    put(11, *tie(BIG_K), BIG_K, 0)          # the ties off the fast path, and q == alloc_pods
    put(12, *tie(BIG_K + 1), 1 << 40, 0)
    if R > 0:
        i = put(13, 32000, 64 * GIB, 1 << 20, 110, 0)
        ax[R - 1, i], ux[R - 1, i] = (1 << 50) + 9, 2     # a free extra amount off the fast path
        i = put(14, 32000, 64 * GIB, 1 << 20, 110, 0)
        ax[0, i], ux[0, i] = 4, 4                          # the first extra resource used up
    return [ac, am, ap, pc, uc, um], ax, ux


def make_specs(S, R, special=True, seed=7):
    """spec_cpu, spec_mem, spec_x [R, S], node_cap [S].  Index 0 (and 64: a wave without the
    specials) is the tie spec.  special: indices 1..6 hold c = 0, m = 0, m = -1, a cpu and a
    memory request above 2^52 and a negative extra request — their wave runs the exact path."""
    rng = np.random.default_rng([seed, S, R, int(special)])
    sc = rng.choice([100, 250, 500, 1000, 2000, 4000], S).astype(np.uint64)
    sm = rng.choice([64 << 20, 256 << 20, GIB, 4 * GIB, 16 * GIB], S).astype(np.int64)
    sx = np.zeros((R, S), np.int64)
    for r in range(R):
        sx[r] = rng.integers(1, 4, S) if r % 2 == 0 else rng.choice([GIB, 20 * GIB, 100 * GIB], S)
        sx[r, rng.random(S) < 0.3] = 0  # not requested
    cap = np.array([[0, 0, 1, 2, 5, I64.max][s % 6] for s in range(S)], np.int64)
    sp = [(0, GIB), (500, 0), (250, -1), ((1 << 52) + 5, 1 << 20), (100, (1 << 52) + 1),
          (100, 64 << 20)]
    if special:
        for k, (c, m) in enumerate(sp):
            if 1 + k < S:
                sc[1 + k], sm[1 + k] = c, m
        if R > 0 and 6 < S:
            sx[0, 6] = -2
    for s in (0, 64):
        if s < S:
            sc[s], sm[s], cap[s] = TIE_C, TIE_M, TIE_CAP
            sx[:, s] = TIE_X[:R]
    return sc, sm, sx, cap


def make_groups(n, G, seed=7):
    """Unsorted ids; group 1 stays empty; 6 % of the ids lie outside [0, G)."""
    rng = np.random.default_rng([seed, n, G])
    gid = rng.choice([g for g in range(G) if g != 1], n).astype(np.int32)
    bad = rng.random(n) < 0.06
    gid[bad] = np.where(rng.random(int(bad.sum())) < 0.5, -1, G + 5)
    return gid


def case(n, S, R, G=None, special=True, capped=True):
    """The inputs of one case and the model's table and cells."""
    def make():
        rows, ax, ux = cached(("rows", n, R), lambda: make_rows(n, R))
        sc, sm, sx, cap = make_specs(S, R, special)
        if not capped:
            cap = None
        gid = None if G is None else make_groups(n, G)
        tab = em.explain_table(rows, ax, ux, sc, sm, sx, cap)
        cells = em.explain_cells(tab, sc, sm, sx, gid, 1 if G is None else G)
        for a in rows + [ax, ux, sc, sm, sx, cap, gid, tab["q"], tab["b"], tab["dz"]] + list(cells):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        return dict(rows=rows, ax=ax, ux=ux, sc=sc, sm=sm, sx=sx, cap=cap, gid=gid,
                    G=1 if G is None else G, tab=tab, cells=cells)
    return cached(("case", n, S, R, G, special, capped), make)


def run(eng, c, **kw):
    return eng.fit_explain(*c["rows"], c["ax"], c["ux"], c["sc"], c["sm"], c["sx"], c["gid"],
                           c["G"], c["cap"], **kw)


def check(eng, n, S, R, G=None, special=True, capped=True):
    c = case(n, S, R, G, special, capped)
    res = run(eng, c)
    t, e, wr, wp, left = c["cells"]
    sq = (lambda a: a) if G is not None else (lambda a: a[..., 0, :])
    msg = str((n, S, R, G, special, capped))
    np.testing.assert_array_equal(res.err, sq(e), msg)
    np.testing.assert_array_equal(res.totals, sq(t), msg)
    np.testing.assert_array_equal(res.why_rows, sq(wr), msg)
    np.testing.assert_array_equal(res.why_pods, sq(wp), msg)
    np.testing.assert_array_equal(res.left, sq(left), msg)
    assert res.why_rows.shape == ((8, S) if G is None else (8, G, S))
    assert res.left.shape == ((2 + R, S) if G is None else (2 + R, G, S))
    return c, res


# ---- parity with the model -----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", ALL_N)
def test_gpu_explain_every_n(eng, n):
    check(eng, n, 96, 2)  # (a wave with the special specs, and half a wave without)


@pytest.mark.gpu
@pytest.mark.parametrize("S,special", [(S, True) for S in ALL_S] + [(63, False), (64, False)])
def test_gpu_explain_every_s(eng, S, special):
    check(eng, 129, S, 1, 3, special)


@pytest.mark.gpu
@pytest.mark.parametrize("R", range(_lib.KCC_EXT_MAX + 1))
@pytest.mark.parametrize("G", [None, 5])
def test_gpu_explain_every_r_and_group_form(eng, R, G):
    c, res = check(eng, RUN + 1, S3, R, G)
    if G is not None:  # the flagged cells are zero and their neighbours are not touched
        bad = res.err != 0
        assert bad.any() and (~bad).any()
        assert not res.why_rows[:, bad].any() and not res.left[:, bad].any()
        assert res.why_rows[:, ~bad].any()
        assert not res.why_rows[:, 1].any() and not res.left[:, 1].any()  # the empty group


# ---- identities pinned on the device ---------------------------------------------------------
@pytest.mark.gpu
def test_gpu_explain_identities(eng):
    n, S, R, G = RUN + 1, S3, 2, 5
    c = case(n, S, R, G)
    res = run(eng, c)
    ct, ce, _, grows = eng.fit_capped(*c["rows"], c["ax"], c["ux"], c["sc"], c["sm"], c["sx"],
                                      c["gid"], G, c["cap"], want_min=False)
    np.testing.assert_array_equal(res.totals, ct)
    np.testing.assert_array_equal(res.err, ce)
    ok = res.err == 0
    rows_sum = res.why_rows.sum(axis=0)
    assert np.array_equal(rows_sum[ok], np.broadcast_to(grows[:, None], (G, S))[ok])
    pods_sum = res.why_pods.view(np.uint64).sum(axis=0, dtype=np.uint64).view(np.int64)
    assert np.array_equal(pods_sum[ok], res.totals[ok])
    assert res.why_rows[_lib.KCC_WHY_CAP].any()
    assert not res.why_rows[_lib.KCC_WHY_EXT0 + R:_lib.KCC_WHY_PODS].any()
    assert not res.why_pods[_lib.KCC_WHY_EXT0 + R:_lib.KCC_WHY_PODS].any()
    # no cap: an empty CAP plane (NULL, zeros and negatives alike)
    for cap in (None, np.zeros(S, np.int64), np.full(S, -4, np.int64)):
        r0 = eng.fit_explain(*c["rows"], c["ax"], c["ux"], c["sc"], c["sm"], c["sx"], c["gid"], G,
                             cap)
        assert not r0.why_rows[_lib.KCC_WHY_CAP].any() and not r0.why_pods[_lib.KCC_WHY_CAP].any()
        assert r0.why_rows[_lib.KCC_WHY_PODS].any()
    # an unrequested resource holds no row and leaves its whole free amount
    sx0 = c["sx"].copy()
    sx0[1] = 0
    r1 = eng.fit_explain(*c["rows"], c["ax"], c["ux"], c["sc"], c["sm"], sx0, c["gid"], G, c["cap"])
    assert not r1.why_rows[_lib.KCC_WHY_EXT0 + 1].any()
    fx1 = np.array(c["tab"]["free"][2][1], dtype=object)
    for g in range(G):
        want = em.i64(int(sum(fx1[c["gid"] == g])))
        assert (r1.left[3, g][r1.err[g] == 0] == want).all()
    # an extra column that copies the memory column never takes a row: the tie goes to MEM
    ax2, ux2, sx2 = c["ax"].copy(), c["ux"].copy(), c["sx"].copy()
    ax2[0], ux2[0], sx2[0] = c["rows"][1], c["rows"][5], c["sm"]
    r2 = eng.fit_explain(*c["rows"], ax2, ux2, c["sc"], c["sm"], sx2, c["gid"], G, c["cap"])
    assert not r2.why_rows[_lib.KCC_WHY_EXT0].any() and r2.why_rows[_lib.KCC_WHY_MEM].any()
    np.testing.assert_array_equal(r2.left[2][r2.err == 0], r2.left[1][r2.err == 0])


@pytest.mark.gpu
@pytest.mark.parametrize("G", [None, 5])
def test_gpu_explain_nullable_outputs(eng, G):
    c = case(RUN + 1, S3, 2, G)
    full = run(eng, c)
    ct, ce, _, _ = eng.fit_capped(*c["rows"], c["ax"], c["ux"], c["sc"], c["sm"], c["sx"],
                                  c["gid"], c["G"], c["cap"], want_min=False, want_rows=False)
    none = run(eng, c, want_rows=False, want_pods=False, want_left=False)
    assert none.why_rows is None and none.why_pods is None and none.left is None
    np.testing.assert_array_equal(none.totals, ct)
    np.testing.assert_array_equal(none.err, ce)
    for name in ("why_rows", "why_pods", "left"):
        kw = {f"want_{k}": k == name.split("_")[-1] for k in ("rows", "pods", "left")}
        one = run(eng, c, **kw)
        np.testing.assert_array_equal(getattr(one, name), getattr(full, name), name)
        np.testing.assert_array_equal(one.totals, full.totals, name)
        np.testing.assert_array_equal(one.err, full.err, name)
        assert [getattr(one, k) is None for k in ("why_rows", "why_pods", "left")].count(True) == 2


@pytest.mark.gpu
def test_gpu_explain_degenerate_and_argument_errors(eng):
    from kubernetesclustercapacity_amd import KccError
    c = case(64, 65, 2)
    S, R = 65, 2
    empty = [a[:0] for a in c["rows"]]
    r = eng.fit_explain(*empty, c["ax"][:, :0], c["ux"][:, :0], c["sc"], c["sm"], c["sx"], None, 1,
                        c["cap"])
    for a in (r.totals, r.err, r.why_rows, r.why_pods, r.left):
        assert not a.any()
    assert r.why_rows.shape == (8, S) and r.left.shape == (2 + R, S)
    r = eng.fit_explain(*c["rows"], c["ax"], c["ux"], c["sc"][:0], c["sm"][:0], c["sx"][:, :0], None,
                        1, None)
    assert r.totals.shape == (0,) and r.why_rows.shape == (8, 0) and r.left.shape == (2 + R, 0)
    # grouped and empty: G x S zeros
    r = eng.fit_explain(*empty, None, None, c["sc"], c["sm"], None, np.zeros(0, np.int32), 3, None)
    assert r.why_pods.shape == (8, 3, S) and not r.why_pods.any() and not r.left.any()

    def code(fn):
        with pytest.raises(KccError) as ei:
            fn()
        return ei.value.code

    rows, ax, ux, sc, sm, sx = c["rows"], c["ax"], c["ux"], c["sc"], c["sm"], c["sx"]
    bad = [
        lambda: eng.fit_explain(*rows, ax, ux, sc, sm, sx, None, 2),            # no ids: G must be 1
        lambda: eng.fit_explain(*rows, ax, ux, sc, sm, sx, c["gid"], 0),
        lambda: eng.fit_explain(*rows, np.zeros((5, 64), np.int64), np.zeros((5, 64), np.int64),
                                sc, sm, np.zeros((5, S), np.int64)),              # n_ext > KCC_EXT_MAX
    ]
    for fn in bad:
        assert code(fn) == _lib.KCC_EINVAL
    # KCC_WHY_SLOTS x G x S <= 2^28 when a why_* output is asked for (G x S itself is in range)
    gid = np.zeros(64, np.int32)
    big_g = (1 << 28) // 8 // S + 1
    for kw in (dict(want_left=False), dict(want_pods=False, want_left=False)):
        lib, h = eng._lib, eng._h
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        one = np.zeros(1, np.int64)
        rc = lib.kcc_fit_explain(h, 64, *[p(a) for a in rows], R, p(ax), p(ux), p(gid), big_g, S,
                                 p(sc), p(sm), p(sx), None, p(one), p(one.view(np.int32)[:1]),
                                 p(one), p(one) if kw.get("want_pods", True) else None, None)
        assert rc == _lib.KCC_EINVAL and b"KCC_WHY_SLOTS" in lib.kcc_last_error(h)
    # NULL outputs / arrays
    rc = eng._lib.kcc_fit_explain(eng._h, 64, *[None] * 6, 0, None, None, None, 1, S,
                                  C.c_void_p(sc.ctypes.data), C.c_void_p(sm.ctypes.data), None, None,
                                  C.c_void_p(16), C.c_void_p(16), None, None, None)
    assert rc == _lib.KCC_EINVAL


# ---- the async form in a graph ---------------------------------------------------------------
def _dv(torch, dev, a):
    a = np.array(a, order="C", copy=True)  # (the cached inputs are read-only)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)


@pytest.mark.gpu
def test_gpu_explain_async_graph_replayed_on_changed_inputs():
    """fit_explain_async captured into one graph on one stream; replayed on the captured
    inputs, then on another case's written into the same tensors: each replay equals the
    model."""
    import torch

    from conftest import init_torch_first
    from kubernetesclustercapacity_amd import CapacityEngine
    init_torch_first()
    dev = torch.device("cuda", 0)
    n, S, R, G = RUN + 1, S3, 2, 5
    a = case(n, S, R, G)
    rows_b, ax_b, ux_b = make_rows(n, R, seed=11)
    tab_b = em.explain_table(rows_b, ax_b, ux_b, a["sc"], a["sm"], a["sx"], a["cap"])
    cells_b = em.explain_cells(tab_b, a["sc"], a["sm"], a["sx"], a["gid"], G)
    with CapacityEngine(0, 1) as eng:
        d_rows = [_dv(torch, dev, x) for x in a["rows"]]
        d_ax, d_ux = _dv(torch, dev, a["ax"]), _dv(torch, dev, a["ux"])
        d_gid = _dv(torch, dev, a["gid"])
        d_sc, d_sm, d_sx, d_cap = (_dv(torch, dev, a[k]) for k in ("sc", "sm", "sx", "cap"))
        full = lambda k, t: torch.empty(k, dtype=t, device=dev)  # noqa: E731
        out = dict(t=full(G * S, torch.int64), e=full(G * S, torch.int32),
                   wr=full(8 * G * S, torch.int64), wp=full(8 * G * S, torch.int64),
                   left=full((2 + R) * G * S, torch.int64))

        def enqueue(stream):
            eng.fit_explain_async(*d_rows, R, d_ax, d_ux, d_gid, G, d_sc, d_sm, d_sx, d_cap,
                                  out["t"], out["e"], out["wr"], out["wp"], out["left"],
                                  stream=stream)

        stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(stream):  # warm-up: every workspace allocated
            enqueue(stream)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            enqueue(stream)
        for cells, rows, ax, ux in ((a["cells"], None, None, None), (cells_b, rows_b, ax_b, ux_b)):
            with torch.cuda.stream(stream):
                if rows is not None:
                    for d, h in zip(d_rows + [d_ax, d_ux], rows + [ax, ux]):
                        d.copy_(_dv(torch, dev, h))
                for t in out.values():
                    t.fill_(77)
                g.replay()
            stream.synchronize()
            t, e, wr, wp, left = cells
            for name, want in (("t", t), ("e", e), ("wr", wr), ("wp", wp), ("left", left)):
                np.testing.assert_array_equal(out[name].cpu().numpy().reshape(want.shape), want, name)
        del g


@pytest.mark.gpu
def test_gpu_explain_graph_behind_deploy():
    """kcc_deploy_async and kcc_fit_explain_async in one capture: the explanation is of the
    state the plan leaves.  Each replay equals the host forms run one after the other (and the
    model on the state they return)."""
    import torch

    from conftest import init_torch_first
    from kubernetesclustercapacity_amd import KCC_DEPLOY_PACK, CapacityEngine
    init_torch_first()
    dev = torch.device("cuda", 0)
    n, S, R, K = RUN + 1, 65, 2, 3
    a = case(n, S, R, None, special=False)
    rows, ax, ux = a["rows"], a["ax"], a["ux"]
    p_sc = np.array([500, 1000, 250], np.uint64)
    p_sm = np.array([GIB, 2 * GIB, 256 << 20], np.int64)
    p_sx = np.array([[1, 0, 0], [0, 10 * GIB, 0]], np.int64)
    p_rep = np.array([40, 25, 300], np.int64)
    with CapacityEngine(0, 1) as eng:
        dep = eng.deploy(*rows, p_sc, p_sm, p_rep, KCC_DEPLOY_PACK, ax, ux, p_sx, want_rows=False)
        assert dep.placed.sum() > 0 and not dep.err.any()
        after = [rows[0], rows[1], rows[2], dep.pod_count, dep.used_cpu, dep.used_mem]
        eager = eng.fit_explain(*after, ax, dep.used_x, a["sc"], a["sm"], a["sx"], None, 1, a["cap"])
        tab = em.explain_table(after, ax, dep.used_x, a["sc"], a["sm"], a["sx"], a["cap"])
        model = em.explain_cells(tab, a["sc"], a["sm"], a["sx"])
        before = eng.fit_explain(*rows, ax, ux, a["sc"], a["sm"], a["sx"], None, 1, a["cap"])
        assert not np.array_equal(before.why_rows, eager.why_rows)
        d_ac, d_am, d_ap = (_dv(torch, dev, x) for x in rows[:3])
        pristine = [_dv(torch, dev, x) for x in (rows[3], rows[4], rows[5], ux)]
        work = [torch.empty_like(t) for t in pristine]
        d_ax = _dv(torch, dev, ax)
        d_p = [_dv(torch, dev, x) for x in (p_sc, p_sm, p_sx, p_rep)]
        d_sc, d_sm, d_sx, d_cap = (_dv(torch, dev, a[k]) for k in ("sc", "sm", "sx", "cap"))
        full = lambda k, t: torch.empty(k, dtype=t, device=dev)  # noqa: E731
        out = dict(placed=full(K, torch.int64), used=full(K, torch.int64), perr=full(K, torch.int32),
                   t=full(S, torch.int64), e=full(S, torch.int32), wr=full(8 * S, torch.int64),
                   wp=full(8 * S, torch.int64), left=full((2 + R) * S, torch.int64))

        def enqueue(stream):
            for w, p in zip(work, pristine):
                w.copy_(p)
            eng.deploy_async(d_ac, d_am, d_ap, R, d_ax, work[0], work[1], work[2], work[3], None, 1,
                             None, d_p[0], d_p[1], d_p[2], d_p[3], None, KCC_DEPLOY_PACK,
                             out["placed"], out["used"], out["perr"], None, stream=stream)
            eng.fit_explain_async(d_ac, d_am, d_ap, work[0], work[1], work[2], R, d_ax, work[3],
                                  None, 1, d_sc, d_sm, d_sx, d_cap, out["t"], out["e"], out["wr"],
                                  out["wp"], out["left"], stream=stream)

        stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(stream):
            enqueue(stream)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            enqueue(stream)
        for _ in range(2):
            with torch.cuda.stream(stream):
                for t in list(out.values()) + work:
                    t.fill_(77)
                g.replay()
            stream.synchronize()
            np.testing.assert_array_equal(out["placed"].cpu().numpy(), dep.placed)
            for name, field, k in (("t", "totals", 0), ("e", "err", 1), ("wr", "why_rows", 2),
                                   ("wp", "why_pods", 3), ("left", "left", 4)):
                got = out[name].cpu().numpy().reshape(getattr(eager, field).shape)
                np.testing.assert_array_equal(got, getattr(eager, field), field)
                np.testing.assert_array_equal(got, model[k][..., 0, :], field)
        del g


# ---- a small seeded fuzz ---------------------------------------------------------------------
def fuzz_params():
    out = []
    for seed in range(8):
        rng = np.random.default_rng([0xE8, seed])
        n = int(rng.choice([1, 2, 63, 65, 200, RUN, RUN + 3, 2 * RUN + 9]))
        S = int(rng.choice([1, 2, 64, 65, 66, 130]))
        while n * S > 40000:
            S //= 2
        out.append((seed, n, S, int(rng.integers(0, 5)), [None, 1, 2, 3, 9][int(rng.integers(0, 5))],
                    bool(rng.integers(0, 2)), bool(rng.integers(0, 2))))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n,S,R,G,special,capped", fuzz_params())
def test_gpu_explain_fuzz(eng, seed, n, S, R, G, special, capped):
    rows, ax, ux = make_rows(n, R, seed=100 + seed)
    sc, sm, sx, cap = make_specs(S, R, special, seed=100 + seed)
    cap = cap if capped else None
    gid = None if G is None else (make_groups(n, G, seed=100 + seed) if G > 1
                                  else np.zeros(n, np.int32))
    g1 = 1 if G is None else G
    tab = em.explain_table(rows, ax, ux, sc, sm, sx, cap)
    t, e, wr, wp, left = em.explain_cells(tab, sc, sm, sx, gid, g1)
    res = eng.fit_explain(*rows, ax, ux, sc, sm, sx, gid, g1, cap)
    sq = (lambda a: a) if G is not None else (lambda a: a[..., 0, :])
    msg = f"seed={seed} n={n} S={S} R={R} G={G} special={special} capped={capped}"
    for got, want in ((res.err, e), (res.totals, t), (res.why_rows, wr), (res.why_pods, wp),
                      (res.left, left)):
        np.testing.assert_array_equal(got, sq(want), msg)
