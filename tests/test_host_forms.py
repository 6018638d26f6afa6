"""The host-array entry points against their device forms ("Host forms").

Every host form checks its arguments, stages its arrays into the context's slots (the k-th
array a call stages takes slot k), calls the device-level function its *_async twin calls, and
copies the outputs back.  Two things can go wrong there and no kernel test sees them:

  - the host form and the device form disagree, above all at the degenerate sizes (no rows, no
    specs, no steps, no groups), which only the device-level function states: every pair below
    gives bit-equal outputs on numpy arrays and on torch tensors, and the Python models' where
    there is one;
  - a slot holds another call's size or another call's data: one engine runs a sequence of
    different entry points, small and large, and every result equals the same call's on a fresh
    engine.
"""
import numpy as np
import pytest

from kubernetesclustercapacity_amd import _lib
from oracle import coracle
from tests import deploy_model as dm
from tests import explain_model as em
from tests import ext_model as xm
from tests import spread_model as spm
from tests import test_deploy as td
from tests import test_explain as tx
from tests import test_pods as tp

pytestmark = pytest.mark.gpu
I64 = np.iinfo(np.int64)
SENTINEL = 77
R2 = 2


@pytest.fixture(scope="module")
def eng():
    from tests.conftest import init_torch_first
    init_torch_first()
    from kubernetesclustercapacity_amd import CapacityEngine
    with CapacityEngine(0, 1) as e:
        yield e


def dev_of(a):
    """A numpy array as a torch tensor on the device (uint64 as its int64 bits; None: None)."""
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).to(torch.device("cuda", 0))


def dev_ids(gid):
    """Group ids on the device; no rows: one unused element, as an empty tensor has no address
    and NULL ids mean "one group"."""
    return dev_of(gid if gid is None or gid.size else np.zeros(1, np.int32))


def dev_out(shape, dtype):
    """A device output of the numpy dtype, filled with the sentinel."""
    return dev_of(np.full(shape, SENTINEL, np.int64 if dtype == np.uint64 else dtype))


def host_of(t, like):
    """A device output back on the host with `like`'s dtype and shape."""
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


def same(got, want, msg):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, msg
    np.testing.assert_array_equal(got.reshape(-1), want.reshape(-1), err_msg=msg)


# ---- the cell fits ---------------------------------------------------------------------------
_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def cell_case(n, S, R, G):
    """test_explain's rows, specs and ids, cut to n rows (none: the empty prefix)."""
    rows, ax, ux = cached(("rows", max(n, 1), R), lambda: tx.make_rows(max(n, 1), R))
    rows, ax, ux = [a[:n] for a in rows], ax[:, :n], ux[:, :n]
    sc, sm, sx, cap = cached(("specs", max(S, 1), R), lambda: tx.make_specs(max(S, 1), R))
    sc, sm, sx, cap = sc[:S], sm[:S], sx[:, :S], cap[:S]
    gid = None if G is None else tx.make_groups(n, G)
    return rows, ax, ux, sc, sm, sx, cap, gid


def cell_table(n, S, R, capped):
    def make():
        rows, ax, ux, sc, sm, sx, cap, _ = cell_case(n, S, R, None)
        return em.explain_table(rows, ax, ux, sc, sm, sx, cap if capped else None)
    return cached(("tab", n, S, R, capped), make)


def cells_device(eng, which, rows, R, ax, ux, gid, G, sc, sm, sx, cap, like):
    """The device form of `which` on copies of the inputs; the outputs shaped as `like`'s."""
    d = [dev_of(a) for a in rows]
    dax, dux, dsx = dev_of(ax.reshape(-1)), dev_of(ux.reshape(-1)), dev_of(sx.reshape(-1))
    dg, dsc, dsm, dcap = dev_ids(gid), dev_of(sc), dev_of(sm), dev_of(cap)
    outs = [dev_out(a.size, a.dtype) for a in like]
    if which == "grouped":
        eng.fit_grouped_async(*d, dg, G, dsc, dsm, *outs)
    elif which == "ext":
        eng.fit_ext_async(*d, R, dax, dux, dg, G, dsc, dsm, dsx, *outs)
    elif which == "capped":
        eng.fit_capped_async(*d, R, dax, dux, dg, G, dsc, dsm, dsx, outs[0], outs[1], dcap,
                             outs[2], outs[3])
    else:
        eng.fit_explain_async(*d, R, dax, dux, dg, G, dsc, dsm, dsx, dcap, *outs)
    return [host_of(t, a) for t, a in zip(outs, like)]


@pytest.mark.parametrize("G", [None, 3])
@pytest.mark.parametrize("S", [0, 1, 65])
@pytest.mark.parametrize("n", [0, 1, 257])
def test_cell_fits_host_equals_device(eng, n, S, G):
    """kcc_fit_grouped, _ext, _capped and _explain (all three outputs on), R = 2 (the grouped
    fit: none): host form == device form == the models; no rows: every cell 0, cell_min
    INT64_MAX, no group has a row; no specs: nothing but group_rows."""
    g1 = 1 if G is None else G
    msg = f"n={n} S={S} G={G}"
    rows, ax, ux, sc, sm, sx, cap, gid = cell_case(n, S, R2, G)
    live = n > 0 and S > 0

    # the grouped fit insists on ids: all in group 0 where the other three take none
    rows0, ax0, ux0, sc0, sm0, sx0, _, _ = cell_case(n, S, 0, G)
    gid0 = np.zeros(n, np.int32) if G is None else gid
    host = list(eng.fit_grouped(*rows0, gid0, g1, sc0, sm0))
    got = cells_device(eng, "grouped", rows0, 0, ax0, ux0, gid0, g1, sc0, sm0, sx0, None, host)
    for h, d, name in zip(host, got, ("totals", "err")):
        same(d, h, f"grouped {name}: {msg}")
    if live:
        tab = cell_table(n, S, 0, False)
        t, e = xm.totals_from_pairs(tab["q"], tab["dz"], gid0, g1)
        same(host[0], t, f"grouped totals, model: {msg}")
        same(host[1], e, f"grouped err, model: {msg}")

    host = list(eng.fit_ext(*rows, ax, ux, sc, sm, sx, gid, g1))
    got = cells_device(eng, "ext", rows, R2, ax, ux, gid, g1, sc, sm, sx, None, host)
    for h, d, name in zip(host, got, ("totals", "err")):
        same(d, h, f"ext {name}: {msg}")
    if live:
        tab = cell_table(n, S, R2, False)
        want = xm.totals_from_pairs(tab["q"], tab["dz"], gid, g1)
        for h, w, name in zip(host, want, ("totals", "err")):
            same(h, w, f"ext {name}, model: {msg}")

    names = ("totals", "err", "cell_min", "group_rows")
    host = list(eng.fit_capped(*rows, ax, ux, sc, sm, sx, gid, g1, cap))
    got = cells_device(eng, "capped", rows, R2, ax, ux, gid, g1, sc, sm, sx, cap, host)
    for h, d, name in zip(host, got, names):
        same(d, h, f"capped {name}: {msg}")
    if live:
        want = spm.capped_cells(tab["q"], tab["dz"], gid, g1, cap)
        for h, w, name in zip(host, want, names):
            same(h, w, f"capped {name}, model: {msg}")
    assert host[0].size == g1 * S and host[3].shape == (g1,)
    if n == 0:
        assert not host[0].any() and not host[1].any() and not host[3].any(), msg
        assert (host[2] == I64.max).all(), msg

    names = ("totals", "err", "why_rows", "why_pods", "left")
    res = eng.fit_explain(*rows, ax, ux, sc, sm, sx, gid, g1, cap)
    host = [res.totals, res.err, res.why_rows, res.why_pods, res.left]
    got = cells_device(eng, "explain", rows, R2, ax, ux, gid, g1, sc, sm, sx, cap, host)
    for h, d, name in zip(host, got, names):
        same(d, h, f"explain {name}: {msg}")
    if live:
        want = em.explain_cells(cell_table(n, S, R2, True), sc, sm, sx, gid, g1)
        for h, w, name in zip(host, want, names):
            same(h, w, f"explain {name}, model: {msg}")
    assert host[2].size == _lib.KCC_WHY_SLOTS * g1 * S and host[4].size == (2 + R2) * g1 * S
    if n == 0:
        assert not any(a.any() for a in host), msg


@pytest.mark.parametrize("S", [0, 65])
@pytest.mark.parametrize("G", [0, 3])
def test_spread_fold_host_equals_device(eng, G, S):
    rng = np.random.default_rng([G, S])
    ct = rng.integers(0, 1000, (G, S)).astype(np.int64)
    ce = (rng.random((G, S)) < 0.05).astype(np.int32)
    gr = rng.integers(0, 3, G).astype(np.int64)
    dom = np.array([1, 0, 1], np.int32)[:G]
    el = (rng.random((G, S)) < 0.8).astype(np.uint8)
    sk = rng.integers(0, 3, S).astype(np.int64)
    msg = f"G={G} S={S}"
    t, e = eng.spread_fold(ct, ce, gr, dom, 2, el, sk)
    dt, de = dev_out(S, np.int64), dev_out(S, np.int32)
    eng.spread_fold_async(G, S, dev_of(ct.reshape(-1)), dev_of(ce.reshape(-1)), dev_of(gr),
                          dev_of(dom), 2, dev_of(el.reshape(-1)), dev_of(sk), dt, de)
    same(host_of(dt, t), t, f"totals: {msg}")
    same(host_of(de, e), e, f"err: {msg}")
    assert t.shape == (S,) and e.shape == (S,)
    if G == 0:
        assert not t.any() and not e.any(), msg
    elif S:
        wt, we, _ = spm.fold(ct, ce, gr, dom, 2, el, sk)
        same(t, wt, f"totals, model: {msg}")
        same(e, we, f"err, model: {msg}")


# ---- deploy ----------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", td.POLICIES)
@pytest.mark.parametrize("R", [0, 2])
@pytest.mark.parametrize("K", [0, 1, 3])
@pytest.mark.parametrize("n", [0, 257])
def test_deploy_host_equals_device(eng, n, K, R, policy):
    """No rows: placed, nodes_used and err all zero, the state unchanged.  No steps: no output
    written (the device outputs keep their sentinel; the host form's have no element), the
    state unchanged."""
    msg = f"n={n} K={K} R={R} policy={policy}"
    case = td.plain_case(11, max(n, 1), max(K, 1), R)
    rows = [a[:n] for a in case["rows"]]
    ax, ux, sx = case["ax"][:, :n], case["ux"][:, :n], case["sx"][:, :K]
    sc, sm = case["sc"][:K], case["sm"][:K]
    G = 3
    gid = (np.arange(n) % 4 - 1).astype(np.int32)  # a quarter of the ids outside [0, G)
    el = np.random.default_rng(K).random((G, K)) < 0.8
    cap = np.array([0, 2, 1000], np.int64)[:K]
    cut = dict(rows=rows, ax=ax, ux=ux, sc=sc, sm=sm, sx=sx)
    rep = td.plan_replicas(cut, K, policy, 0, gid, G, el, cap) if n else np.full(K, 5, np.int64)
    got = eng.deploy(*rows, sc, sm, rep, policy, ax, ux, sx, cap, gid, G, el)
    if n and K:
        want = dm.deploy(rows, ax, ux, sc, sm, sx, rep, policy, cap, gid, G, el)
        for f in td.FIELDS:
            same(getattr(got, f), getattr(want, f), f"{f}, model: {msg}")
        assert got.placed.sum() > 0, msg
    else:
        assert not got.placed.any() and not got.nodes_used.any() and not got.err.any(), msg
        assert got.placed.shape == (K,) and got.rows.shape == (K, n)
        for a, b in zip((got.pod_count, got.used_cpu, got.used_mem, got.used_x),
                        (rows[3], rows[4], rows[5], ux)):
            same(a, b, f"state: {msg}")
    state = [dev_of(a) for a in (rows[3], rows[4], rows[5], ux.reshape(-1))]
    outs = [dev_out(K, np.int64), dev_out(K, np.int64), dev_out(K, np.int32),
            dev_out(K * n, np.int64)]
    eng.deploy_async(dev_of(rows[0]), dev_of(rows[1]), dev_of(rows[2]), R, dev_of(ax.reshape(-1)),
                     *state, dev_ids(gid), G, dev_of(el.astype(np.uint8).reshape(-1)), dev_of(sc),
                     dev_of(sm), dev_of(sx.reshape(-1)), dev_of(rep), dev_of(cap), policy, *outs)
    for t, f in zip(outs + state, ("placed", "nodes_used", "err", "rows", "pod_count", "used_cpu",
                                   "used_mem", "used_x")):
        h = getattr(got, f)
        same(host_of(t, h), h, f"{f}: {msg}")


def test_deploy_no_steps_writes_nothing(eng):
    """K = 0 through the C-ABI with outputs that have room: host and device forms leave the
    sentinel in every output and the state as it was."""
    import ctypes as C
    n = 257
    case = td.plain_case(12, n, 1, 0)
    rows = case["rows"]
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    state = [np.array(rows[k], copy=True) for k in (3, 4, 5)]
    outs = [np.full(4, SENTINEL, np.int64), np.full(4, SENTINEL, np.int64),
            np.full(4, SENTINEL, np.int32), np.full(4 * n, SENTINEL, np.int64)]
    rc = eng._lib.kcc_deploy(eng._h, n, p(rows[0]), p(rows[1]), p(rows[2]), 0, None,
                             *[p(a) for a in state], None, None, 1, None, 0, None, None, None,
                             None, None, _lib.KCC_DEPLOY_PACK, *[p(a) for a in outs])
    assert rc == 0, eng._lib.kcc_last_error(eng._h).decode()
    assert all((a == SENTINEL).all() for a in outs)
    for a, k in zip(state, (3, 4, 5)):
        same(a, rows[k], "state")
    dstate = [dev_of(a) for a in state]
    douts = [dev_out(a.size, a.dtype) for a in outs]
    eng.deploy_async(dev_of(rows[0]), dev_of(rows[1]), dev_of(rows[2]), 0, None, *dstate, None,
                     None, 1, None, None, None, None, None, None, _lib.KCC_DEPLOY_PACK, *douts)
    for t, a in zip(douts + dstate, outs + state):
        same(host_of(t, a), a, "device form")


# ---- the reduces, the pod model, the parsers -------------------------------------------------
def containers(seed, n_rows, n):
    rng = np.random.default_rng([seed, n_rows, n])
    per = rng.multinomial(n, np.ones(max(n_rows, 1)) / max(n_rows, 1))[:n_rows]
    ptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(per, out=ptr[1:])
    cpu = rng.integers(0, 1 << 20, n).astype(np.uint64)
    mem = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    cpu[rng.random(n) < 0.02] = np.uint64(2**64 - 9)  # the sums wrap
    return ptr, cpu, mem, cpu * np.uint64(3), mem * 2


@pytest.mark.parametrize("lim", [False, True])
@pytest.mark.parametrize("n", [0, 1, 257])
def test_reduce_requests_host_equals_device(eng, n, lim):
    ptr, cpu, mem, cl, ml = containers(1, n, 20 * n)
    L = (cl, ml) if lim else (None, None)
    r = eng.get_pod_cpu_memory_requests_limits(ptr, cpu, mem, *L)
    host = [r.cpu_requests, r.memory_requests] + ([r.cpu_limits, r.memory_limits] if lim else [])
    outs = [dev_out(n, a.dtype) for a in host]
    eng.reduce_requests_async(dev_of(ptr), dev_of(cpu), dev_of(mem), outs[0], outs[1],
                              dev_of(L[0]), dev_of(L[1]), *outs[2:])
    want = coracle.reduce_requests(ptr, cpu, mem, *L)
    want = [want[0], want[1]] + ([want[2], want[3]] if lim else [])
    for t, h, w, k in zip(outs, host, want, range(4)):
        same(host_of(t, h), h, f"output {k}: n={n} lim={lim}")
        same(h, w, f"output {k}, oracle: n={n} lim={lim}")
    if not lim:
        assert r.cpu_limits is None and r.memory_limits is None


@pytest.mark.parametrize("lim", [False, True])
@pytest.mark.parametrize("n", [0, 1000])
@pytest.mark.parametrize("nk", [0, 5, 300])
def test_keyed_host_equals_device(eng, nk, n, lim):
    """The keyed reduce and kcc_count_by_key; keys outside [0, n_keys) are skipped."""
    rng = np.random.default_rng([nk, n])
    _, cpu, mem, cl, ml = containers(2, 1, n)
    key = rng.integers(-2, nk + 2, n).astype(np.int32)
    ok = (key >= 0) & (key < nk)
    msg = f"nk={nk} n={n} lim={lim}"
    L = (cl, ml) if lim else (None, None)
    r = eng.get_pod_cpu_memory_requests_limits_keyed(nk, key, cpu, mem, *L)
    host = [r.cpu_requests, r.memory_requests] + ([r.cpu_limits, r.memory_limits] if lim else [])
    outs = [dev_out(nk, a.dtype) for a in host]
    # (no containers: one unused element each — an empty tensor has no address, and NULL
    # limit arrays mean "no limits")
    pad = lambda a: dev_of(a if a is None or a.size else np.zeros(4, a.dtype))  # noqa: E731
    eng.reduce_requests_keyed_async(nk, pad(key), pad(cpu), pad(mem), outs[0], outs[1], None,
                                    pad(L[0]), pad(L[1]), *outs[2:], n=n)
    for t, h, src, k in zip(outs, host, (cpu, mem, cl, ml), range(4)):
        same(host_of(t, h), h, f"output {k}: {msg}")
        w = np.zeros(nk, np.uint64)  # wrapping sums, in any order
        np.add.at(w, key[ok], src[ok].view(np.uint64))
        same(h, w.view(src.dtype), f"output {k}, model: {msg}")
    if lim:
        return
    cnt = eng.count_by_key(nk, key)
    dc = dev_out(nk, np.int64)
    eng.count_by_key_async(nk, dev_of(key), dc)
    same(host_of(dc, cnt), cnt, f"count: {msg}")
    same(cnt, np.bincount(key[ok], minlength=nk).astype(np.int64)[:nk], f"count, model: {msg}")


@pytest.mark.parametrize("init", [False, True])
@pytest.mark.parametrize("P", [0, 1, 257])
def test_pod_requests_host_equals_device(eng, P, init):
    c = tp.pods_case(13, n_pods=P, extremes=P > 1)
    kw = {k: v for k, v in c.items() if k != "node_pod_ptr"}
    if not init:
        kw = {k: v for k, v in kw.items() if not k.startswith("init") and k != "restartable"}
    pc, pm = eng.pod_requests(**kw)
    t = {k: dev_of(v) for k, v in kw.items()}
    dc, dm_ = dev_out(P, np.uint64), dev_out(P, np.int64)
    eng.pod_requests_async(t.pop("pod_ptr"), t.pop("cpu_req"), t.pop("mem_req"), dc, dm_, **t)
    same(host_of(dc, pc), pc, f"cpu: P={P} init={init}")
    same(host_of(dm_, pm), pm, f"mem: P={P} init={init}")
    if P:
        oc, om = coracle.pod_requests(**kw)
        same(pc, oc, f"cpu, oracle: P={P} init={init}")
        same(pm, om, f"mem, oracle: P={P} init={init}")
    assert pc.shape == (P,) and pm.shape == (P,)


@pytest.mark.parametrize("n", [0, 3])
def test_parsers_host_equals_device(eng, n):
    from kubernetesclustercapacity_amd.quantity import pack_strings
    strings = ["250m", "1.5Gi", "12e3"][:n]
    buf, off = pack_strings(strings)
    want = {"cpu": coracle.parse_cpu_millis(buf, off), "bytes": coracle.parse_bytes(buf, off)} if n else {}
    for name, host, dev, dt in (("cpu", eng.convert_cpu_to_milis, eng.parse_cpu_millis_async, np.uint64),
                                ("bytes", eng.to_bytes, eng.parse_bytes_async, np.int64),
                                ("quantity", eng.quantity_value, eng.parse_quantity_async, np.int64)):
        v, st = host((buf, off))
        dv, ds = dev_out(n, dt), dev_out(n, np.int8)
        dev(dev_of(np.asarray(buf, np.uint8)), dev_of(off), dv, ds)
        same(host_of(dv, v), v, f"{name} values: n={n}")
        same(host_of(ds, st), st, f"{name} status: n={n}")
        assert v.shape == (n,) and v.dtype == dt and st.shape == (n,)
        if name in want:
            same(v, want[name][0], f"{name} values, oracle: n={n}")
            same(st, want[name][1], f"{name} status, oracle: n={n}")


# ---- slot reuse across entry points ------------------------------------------------------------
SMALL, LARGE = (65, 65), (4097, 257)


def reuse_steps():
    """(name, call(engine) -> tuple of arrays): the sequence the one engine runs."""
    def cells(n, S):
        rows, ax, ux = tx.make_rows(n, R2)
        sc, sm, sx, cap = tx.make_specs(S, R2)
        return rows, ax, ux, sc, sm, sx, cap, tx.make_groups(n, 5)

    rs, axs, uxs, scs, sms, sxs, caps, gids = cells(*SMALL)
    rl, axl, uxl, scl, sml, sxl, capl, gidl = cells(*LARGE)
    _, cpu, mem, cl, ml = containers(3, 1, 40 * LARGE[0])
    key = np.random.default_rng(3).integers(-1, LARGE[0] + 1, cpu.size).astype(np.int32)
    plan = td.plain_case(14, SMALL[0], 3, R2)
    rep = np.array([40, 1 << 40, 7], np.int64)
    strings = [f"{k}m" for k in range(SMALL[0])]
    ct = np.arange(5 * SMALL[1], dtype=np.int64).reshape(5, SMALL[1])
    ce = (ct % 11 == 0).astype(np.int32)

    def explain(e):
        r = e.fit_explain(*rl, axl, uxl, scl, sml, sxl, gidl, 5, capl)
        return r.totals, r.err, r.why_rows, r.why_pods, r.left

    def deploy(e):
        r = e.deploy(*plan["rows"], plan["sc"], plan["sm"], rep, td.SPREAD, plan["ax"], plan["ux"],
                     plan["sx"])
        return tuple(getattr(r, f) for f in td.FIELDS)

    def keyed(e):
        r = e.get_pod_cpu_memory_requests_limits_keyed(LARGE[0], key, cpu, mem, cl, ml)
        return r.cpu_requests, r.memory_requests, r.cpu_limits, r.memory_limits

    def sharded(e):
        e.set_node_shards(3)
        try:
            return e.total_possible_max_replicas(*rs, scs, sms)
        finally:
            e.set_node_shards(0)

    ext = lambda e: e.fit_ext(*rs, axs, uxs, scs, sms, sxs, gids, 5)  # noqa: E731
    return [("fit_ext small", ext), ("keyed reduce large", keyed), ("deploy small", deploy),
            ("fit_explain large", explain), ("parse small", lambda e: e.convert_cpu_to_milis(strings)),
            ("spread_fold small", lambda e: e.spread_fold(ct, ce, max_skew=np.ones(SMALL[1], np.int64))),
            ("fit, 3 node shards, small", sharded), ("fit_ext small again", ext)]


def test_slots_reused_across_entry_points():
    """One engine, eight calls of seven entry points, small (65 rows x 65 specs) and large
    (4097 x 257) in turn: every slot is grown by one call and then handed, larger than needed
    and full of that call's data, to the next.  Each result == the same call on a fresh
    engine."""
    from tests.conftest import init_torch_first
    init_torch_first()
    from kubernetesclustercapacity_amd import CapacityEngine
    steps = reuse_steps()
    with CapacityEngine(0, 1) as e:
        got = [call(e) for _, call in steps]
    for (name, call), g in zip(steps, got):
        with CapacityEngine(0, 1) as fresh:
            want = call(fresh)
        assert len(g) == len(want), name
        for k, (a, b) in enumerate(zip(g, want)):
            same(a, b, f"{name}: output {k}")
    assert got[0][0].any() and got[3][2].any() and got[6][0].any()  # (not all-zero answers)
