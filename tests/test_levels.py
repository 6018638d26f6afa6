"""kcc_reduce_requests_levels and kcc_fit_levels on the GPU, bit for bit
against tests/levels_model.py: the reduce at the wave, tile and workgroup edges, with empty nodes,
empty pods, wrapping values, levels past L and a node of 70,000 pods cut by tiles and
workgroups; the fit with S_l in {0, 1, 64, 65, 257} mixed over the levels, with and without
group ids, extra resources and node_cap; the identities (plane 0, L == 1, shuffled specs,
monotone totals); the EINVAL and zero-size cases; both async forms in one graph.

The input generators are used by tests/test_levels_cpu.py too, which checks on the model that
they reach what they are meant to reach."""
import ctypes as C

import numpy as np
import pytest

from kubernetesclustercapacity_amd import _lib
from tests import levels_model as lm
from tests import test_explain as tx

GIB = 1 << 30
TILE = 256       # kcc_internal.h LV_WG: pods per tile
MIN_GRID = 256   # kcc_internal.h LV_MIN_GRID: a workgroup takes k = tiles / MIN_GRID tiles (1..8)
LONG = 70_000
RED_N = [1, 63, 64, 65, 257]
RED_L = [1, 2, 8]
# (n_nodes, long node or None): one tile a workgroup; 4 tiles a workgroup; 8 (the most)
RED_BIG = [(257, 100), (20_000, 9_001), (48_000, 23_456)]
FIT_SIZES = [257, 0, 1, 64, 65, 0, 1, 64]  # S_l of the fit cases: L = 8
FIT_N = 129
FULL_LEVEL = 3   # the plane without a row that has CPU left


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


def make_pods(N, L, long_at=None, seed=11):
    """node_pod_ptr, pod_ptr, cpu_req, mem_req, pod_level: 0 / 1 / 3 / 40 pods a node, 0-3
    containers a pod, 2 % of the cpu values near 2^64 and of the memory values negative or near
    2^63 (the sums wrap), levels in [0, L + 2); node long_at holds LONG pods."""
    rng = np.random.default_rng([seed, N, L])
    per = rng.choice([0, 1, 3, 40], N)
    if long_at is not None:
        per[long_at] = LONG
    npp = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    P = int(npp[-1])
    pp = np.concatenate([[0], np.cumsum(rng.integers(0, 4, P))]).astype(np.int64)
    Cn = int(pp[-1])
    cpu = rng.choice([100, 250, 500, 1000, 4000], Cn).astype(np.uint64)
    mem = rng.choice([64 << 20, 256 << 20, GIB, 4 * GIB], Cn).astype(np.int64)
    odd = rng.random(Cn)
    cpu[odd < 0.02] = np.uint64((1 << 64) - 300)
    mem[(odd >= 0.02) & (odd < 0.03)] = -3 * GIB
    mem[(odd >= 0.03) & (odd < 0.04)] = (1 << 63) - 5
    lvl = rng.integers(0, L + 2, P).astype(np.uint8)
    return npp, pp, cpu, mem, lvl


def red_case(N, L, long_at=None):
    def make():
        inp = make_pods(N, L, long_at)
        out = lm.reduce_levels(*inp, L)
        for a in inp + out:
            a.setflags(write=False)
        return inp, out
    return cached(("red", N, L, long_at), make)


def make_fit(sizes=FIT_SIZES, n=FIT_N, R=2, G=None, capped=True):
    """One fit case: tests/test_explain.py's rows (its exact-path rows at fixed positions: free
    CPU >= 2^31 among them) with one used_* / pod_count plane per level, each from another seed;
    plane FULL_LEVEL has no CPU left on any row.  Per level tests/test_explain.py's specs (the
    zero requests at indices 1 and 2 of every level of 7 specs or more)."""
    L = len(sizes)
    rows0, ax, _ = tx.make_rows(n, R)
    planes = [tx.make_rows(n, R, seed=20 + l) for l in range(L)]
    pc = np.stack([p[0][3] for p in planes])
    uc = np.stack([p[0][4] for p in planes])
    um = np.stack([p[0][5] for p in planes])
    ux = np.stack([p[2] for p in planes]).reshape(L, R, n)
    if L > FULL_LEVEL:
        uc[FULL_LEVEL] = rows0[0]
    specs = [tx.make_specs(s, R, True, seed=30 + l) for l, s in enumerate(sizes)]
    sc = np.concatenate([s[0] for s in specs])
    sm = np.concatenate([s[1] for s in specs])
    sx = np.concatenate([s[2] for s in specs], axis=1)
    cap = np.concatenate([s[3] for s in specs]) if capped else None
    lp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    gid = None if G is None else tx.make_groups(n, G)
    return dict(alloc3=rows0[:3], pc=pc, uc=uc, um=um, ax=ax, ux=ux, sc=sc, sm=sm, sx=sx, cap=cap,
                lp=lp, gid=gid, G=1 if G is None else G, L=L, R=R)


def fit_case(R=2, G=None, capped=True, sizes=tuple(FIT_SIZES), n=FIT_N):
    def make():
        c = make_fit(list(sizes), n, R, G, capped)
        c["model"] = lm.fit_levels(c["alloc3"], c["pc"], c["uc"], c["um"], c["ax"], c["ux"],
                                   c["sc"], c["sm"], c["sx"], c["lp"], c["gid"], c["G"], c["cap"])
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        return c
    return cached(("fit", R, G, capped, sizes, n), make)


def run_fit(eng, c, **kw):
    t, e = eng.fit_levels(*c["alloc3"], c["pc"], c["uc"], c["um"], c["ax"], c["ux"], c["sc"],
                          c["sm"], c["sx"], group=c["gid"], n_groups=c["G"], node_cap=c["cap"],
                          **({"level_ptr": c["lp"]} if not kw else kw))
    return t.reshape(c["G"], -1), e.reshape(c["G"], -1)


def check_reduce(eng, N, L, long_at=None):
    inp, (uc, um, pc) = red_case(N, L, long_at)
    guc, gum, gpc = eng.reduce_requests_levels(*inp, L)
    msg = str((N, L, long_at))
    np.testing.assert_array_equal(gpc, pc, msg)
    np.testing.assert_array_equal(guc, uc, msg)
    np.testing.assert_array_equal(gum, um, msg)
    return inp, (guc, gum, gpc)


# ---- the reduce ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L", RED_L)
@pytest.mark.parametrize("N", RED_N)
def test_gpu_levels_reduce(eng, N, L):
    check_reduce(eng, N, L)


@pytest.mark.gpu
@pytest.mark.parametrize("N,long_at", RED_BIG)
def test_gpu_levels_reduce_long_node(eng, N, long_at):
    """A node of 70,000 pods that begins mid-tile and crosses hundreds of tile edges and (with
    1, 4 and 8 tiles a workgroup) every workgroup edge in between."""
    for L in (2, 8):
        check_reduce(eng, N, L, long_at)


@pytest.mark.gpu
def test_gpu_levels_plane0_is_the_plain_reduce(eng):
    (npp, pp, cpu, mem, lvl), (uc, um, pc) = check_reduce(eng, 257, 8, 100)
    r = eng.get_pod_cpu_memory_requests_limits(pp[npp], cpu, mem)
    np.testing.assert_array_equal(uc[0], r.cpu_requests)
    np.testing.assert_array_equal(um[0], r.memory_requests)
    np.testing.assert_array_equal(pc[0], np.diff(npp))


@pytest.mark.gpu
def test_gpu_levels_reduce_fresh_and_reused_engine(eng):
    from kubernetesclustercapacity_amd import CapacityEngine
    with CapacityEngine(0, 1) as fresh:
        small = check_reduce(fresh, 65, 8)[1]
    check_reduce(eng, 20_000, 8, 9_001)  # a larger call first
    again = check_reduce(eng, 65, 8)[1]
    for a, b in zip(small, again):
        np.testing.assert_array_equal(a, b)


# ---- the fit -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("capped", [True, False])
@pytest.mark.parametrize("G", [None, 3])
@pytest.mark.parametrize("R", [0, 2])
def test_gpu_levels_fit(eng, R, G, capped):
    c = fit_case(R, G, capped)
    t, e = run_fit(eng, c)
    np.testing.assert_array_equal(e, c["model"][1])
    np.testing.assert_array_equal(t, c["model"][0])


@pytest.mark.gpu
def test_gpu_levels_fit_two_runs_of_rows(eng):
    c = fit_case(1, 3, True, (65, 1, 0, 64), 257)
    t, e = run_fit(eng, c)
    np.testing.assert_array_equal(e, c["model"][1])
    np.testing.assert_array_equal(t, c["model"][0])


@pytest.mark.gpu
def test_gpu_levels_zero_request_by_plane(eng):
    """A zero cpu request (index 1 of a level's specs) is flagged on a plane with CPU left on
    some row and is not on the plane without."""
    c = fit_case(2, None, True)
    _, e = run_fit(eng, c)
    assert e[0, c["lp"][0] + 1] == _lib.KCC_SPEC_DIVZERO
    assert e[0, c["lp"][FULL_LEVEL] + 1] == _lib.KCC_SPEC_OK
    assert e[0, c["lp"][FULL_LEVEL] + 2] == _lib.KCC_SPEC_DIVZERO  # the zero memory request


@pytest.mark.gpu
@pytest.mark.parametrize("G", [None, 3])
def test_gpu_levels_one_level_is_fit_capped(eng, G):
    c = fit_case(2, G, True, (257,))
    t, e = run_fit(eng, c)
    ct, ce, _, _ = eng.fit_capped(*c["alloc3"], c["pc"][0], c["uc"][0], c["um"][0], c["ax"],
                                  c["ux"][0], c["sc"], c["sm"], c["sx"], c["gid"], c["G"], c["cap"],
                                  want_min=False, want_rows=False)
    np.testing.assert_array_equal(t, ct.reshape(c["G"], -1))
    np.testing.assert_array_equal(e, ce.reshape(c["G"], -1))
    np.testing.assert_array_equal(t, c["model"][0])


@pytest.mark.gpu
def test_gpu_levels_shuffled_specs(eng):
    c = fit_case(2, 3, True)
    t, e = run_fit(eng, c)
    level = np.repeat(np.arange(c["L"]), np.diff(c["lp"]))
    perm = np.random.default_rng(5).permutation(level.size)
    c2 = dict(c, sc=c["sc"][perm], sm=c["sm"][perm], sx=c["sx"][:, perm], cap=c["cap"][perm])
    t2, e2 = run_fit(eng, c2, spec_level=level[perm])
    np.testing.assert_array_equal(t2, t[:, perm])
    np.testing.assert_array_equal(e2, e[:, perm])
    # one [R, N] block of used_x stands for every level
    c3 = dict(c, ux=np.ascontiguousarray(np.broadcast_to(c["ux"][0], c["ux"].shape)))
    t3, _ = run_fit(eng, c3)
    t4, _ = run_fit(eng, dict(c, ux=c["ux"][0]))
    np.testing.assert_array_equal(t4, t3)


def sane_pipeline(N=300, L=4, seed=3):
    """Sane pods (no wrapping value) and generous nodes: the reduce's planes feed the fit.  The
    pod limit is out of every quotient's reach: the reference's clamp (CC:134-136) replaces a q
    that reaches the limit by the slots left, which can be fewer than a smaller q was."""
    rng = np.random.default_rng(seed)
    per = rng.choice([0, 1, 3, 40], N)
    npp = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    P = int(npp[-1])
    pp = np.concatenate([[0], np.cumsum(rng.integers(0, 4, P))]).astype(np.int64)
    cpu = rng.choice([100, 250, 500], int(pp[-1])).astype(np.uint64)
    mem = rng.choice([64 << 20, 256 << 20, GIB], int(pp[-1])).astype(np.int64)
    lvl = rng.integers(0, L, P).astype(np.uint8)
    alloc3 = [np.full(N, 32_000, np.uint64), np.full(N, 128 * GIB, np.int64), np.full(N, 1000, np.int64)]
    return (npp, pp, cpu, mem, lvl), alloc3


@pytest.mark.gpu
def test_gpu_levels_totals_grow_with_the_level(eng):
    """The intended use: the same spec at every level.  On sane inputs a higher level sees no
    more pods, so its total is no smaller (while no quotient reaches the pod limit: see
    sane_pipeline)."""
    L = 4
    pods, alloc3 = sane_pipeline(L=L)
    uc, um, pc = eng.reduce_requests_levels(*pods, L)
    sc = np.tile(np.array([250, 1000, 4000], np.uint64), L)
    sm = np.tile(np.array([GIB, 256 << 20, 8 * GIB], np.int64), L)
    level = np.repeat(np.arange(L), 3)
    t, e = eng.fit_levels(*alloc3, pc, uc, um, None, None, sc, sm, None, spec_level=level)
    assert not e.any()
    t = t.reshape(L, 3)
    assert (np.diff(t, axis=0) >= 0).all() and (t[-1] > t[0]).all()
    muc, mum, mpc = lm.reduce_levels(*pods, L)
    mt, _ = lm.fit_levels(alloc3, mpc, muc, mum, np.zeros((0, len(pc[0])), np.int64),
                          np.zeros((L, 0, len(pc[0])), np.int64), sc, sm, np.zeros((0, sc.size), np.int64),
                          np.arange(0, 3 * L + 1, 3))
    np.testing.assert_array_equal(t.reshape(-1), mt[0])


# ---- argument errors and zero sizes ----------------------------------------------------------
def _reduce_rc(eng, npp, pp, cpu, mem, lvl, L, N=None, P=None):
    npp, pp = np.asarray(npp, np.int64), np.asarray(pp, np.int64)
    cpu, mem = np.asarray(cpu, np.uint64), np.asarray(mem, np.int64)
    lvl = np.asarray(lvl, np.uint8)
    N = npp.size - 1 if N is None else N
    P = pp.size - 1 if P is None else P
    out = [np.full(max(L, 1) * max(N, 1), 77, t) for t in (np.uint64, np.int64, np.int64)]
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = eng._lib.kcc_reduce_requests_levels(eng._h, N, P, cpu.size, p(npp), p(pp), p(cpu), p(mem),
                                             p(lvl), L, *[p(o) for o in out])
    return rc, out


@pytest.mark.gpu
def test_gpu_levels_reduce_einval_and_zero_sizes(eng):
    ok = ([0, 2, 3], [0, 1, 1, 3], [5, 6, 7], [1, 2, 3], [0, 1, 9])
    assert _reduce_rc(eng, *ok, 2)[0] == _lib.KCC_OK
    for L in (0, 9, -1):
        assert _reduce_rc(eng, *ok, L)[0] == _lib.KCC_EINVAL
    bad = [([1, 2, 3], ok[1]), ([0, 3, 2], ok[1]), ([0, 2, 4], ok[1]), (ok[0], [1, 1, 1, 3]),
           (ok[0], [0, 2, 1, 3]), (ok[0], [0, 1, 1, 2])]
    for npp, pp in bad:
        assert _reduce_rc(eng, npp, pp, *ok[2:], 2)[0] == _lib.KCC_EINVAL, (npp, pp)
    rc, out = _reduce_rc(eng, [0], [0], [], [], [], 2, N=0, P=0)  # no nodes
    assert rc == _lib.KCC_OK and all((o == 77).all() for o in out)
    uc, um, pc = eng.reduce_requests_levels([0, 0, 0, 0], [0], [], [], [], 3)  # no pods
    assert uc.shape == (3, 3) and not uc.any() and not um.any() and not pc.any()


@pytest.mark.gpu
def test_gpu_levels_fit_einval_and_zero_sizes(eng):
    c = fit_case(2, None, True, (3, 0, 4), 5)
    S = c["sc"].size

    def rc_of(lp, **kw):
        try:
            run_fit(eng, dict(c, **kw), level_ptr=np.asarray(lp, np.int64))
        except Exception as ex:  # KccError carries the code
            return ex.code
        return 0
    assert rc_of([0, 3, 3, 7]) == 0
    for lp in ([1, 3, 3, 7], [0, 4, 3, 7], [0, 3, 3, 6], [0, 3, 3, 8]):
        assert rc_of(lp) == _lib.KCC_EINVAL, lp
    assert rc_of([0, 3, 3, 7], G=2) == _lib.KCC_EINVAL  # kcc_fit_capped's: NULL group, G != 1
    z = np.zeros(1, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    args = lambda L, lp: (eng._h, 1, p(z), p(z), p(z), L, p(z), p(z), p(z), 0, None, None, None,  # noqa: E731
                          1, 1, p(z), p(z), None, None, lp, p(z), p(z))
    for L, lp in ((0, p(z)), (9, p(z)), (1, None)):
        assert eng._lib.kcc_fit_levels(*args(L, lp)) == _lib.KCC_EINVAL
    # no specs / no nodes: KCC_OK, outputs 0
    e3 = [a[:0] for a in c["alloc3"]]
    t, e = eng.fit_levels(*e3, c["pc"][:, :0], c["uc"][:, :0], c["um"][:, :0], c["ax"][:, :0],
                          c["ux"][:, :, :0], c["sc"], c["sm"], c["sx"], level_ptr=c["lp"])
    assert t.shape == (S,) and not t.any() and not e.any()
    t, e = eng.fit_levels(*c["alloc3"], c["pc"], c["uc"], c["um"], c["ax"], c["ux"], [], [],
                          np.zeros((2, 0)), level_ptr=[0, 0, 0, 0])
    assert t.shape == (0,)


# ---- both async forms in one graph -----------------------------------------------------------
@pytest.mark.gpu
def test_gpu_levels_graph_replay():
    """kcc_reduce_requests_levels_async + kcc_fit_levels_async captured once (tests/
    test_faults_graphs.py's pattern), replayed after pod_level is overwritten in place: each
    replay gives the model's result for the levels it found."""
    import torch

    from kubernetesclustercapacity_amd import CapacityEngine
    from tests.conftest import init_torch_first
    from tests.test_faults_graphs import _to_dev
    init_torch_first()
    L, R, G = 4, 0, 1
    pods, alloc3 = sane_pipeline(N=1100, L=L, seed=9)
    npp, pp, cpu, mem, lvl = pods
    N = npp.size - 1
    sizes = [65, 0, 64, 1]
    lp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    specs = [tx.make_specs(s, R, True, seed=40 + l) for l, s in enumerate(sizes)]
    sc, sm = np.concatenate([s[0] for s in specs]), np.concatenate([s[1] for s in specs])
    cap = np.concatenate([s[3] for s in specs])
    S = sc.size
    rng = np.random.default_rng(2)
    variants = [lvl, rng.integers(0, L + 3, lvl.size).astype(np.uint8), np.zeros_like(lvl)]
    dev = torch.device("cuda", 0)
    d = {k: _to_dev(v, dev) for k, v in dict(npp=npp, pp=pp, cpu=cpu, mem=mem, lvl=lvl, ac=alloc3[0],
                                             am=alloc3[1], ap=alloc3[2], sc=sc, sm=sm, cap=cap).items()}
    planes = {k: torch.zeros(L * N, dtype=torch.int64, device=dev) for k in ("uc", "um", "pc")}
    tot = torch.zeros(G * S, dtype=torch.int64, device=dev)
    err = torch.zeros(G * S, dtype=torch.int32, device=dev)

    def capture(eng, stream):
        eng.reduce_requests_levels_async(d["npp"], d["pp"], d["cpu"], d["mem"], d["lvl"], L,
                                         planes["uc"], planes["um"], planes["pc"], stream=stream)
        eng.fit_levels_async(d["ac"], d["am"], d["ap"], L, planes["pc"], planes["uc"], planes["um"],
                             R, None, None, None, G, d["sc"], d["sm"], None, d["cap"], lp, tot, err,
                             stream=stream)

    with CapacityEngine(0, 1) as eng:
        stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(stream):  # warm-up: every workspace allocated
            capture(eng, stream)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            capture(eng, stream)
        for k in (1, 2, 0):
            with torch.cuda.stream(stream):
                d["lvl"].copy_(torch.from_numpy(variants[k]).to(dev))
                for t in list(planes.values()) + [tot, err]:
                    t.fill_(77)
                g.replay()
            stream.synchronize()
            muc, mum, mpc = lm.reduce_levels(npp, pp, cpu, mem, variants[k], L)
            mt, me = lm.fit_levels(alloc3, mpc, muc, mum, np.zeros((0, N), np.int64),
                                   np.zeros((L, 0, N), np.int64), sc, sm, np.zeros((0, S), np.int64),
                                   lp, None, 1, cap)
            np.testing.assert_array_equal(planes["pc"].cpu().numpy().reshape(L, N), mpc, f"variant {k}")
            np.testing.assert_array_equal(planes["uc"].cpu().numpy().view(np.uint64).reshape(L, N), muc)
            np.testing.assert_array_equal(err.cpu().numpy(), me[0], f"variant {k}")
            np.testing.assert_array_equal(tot.cpu().numpy(), mt[0], f"variant {k}")
        assert eng.reduce_faults() == 0
        del g
