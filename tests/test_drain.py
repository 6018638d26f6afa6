"""kcc_drain on the device against tests/drain_model.py (Python integers): exact equality of the
summary, all seven shape arrays and all four state arrays.

Sizes sit around the deploy row pass's tile (_lib.KCC_DEPLOY_TILE); the table cases fill the
shape table to max_shapes exactly and one past it; the key cases put cpu values on both sides
of 2^63 and negative words next to each other.  The generators are importable without a GPU
(tests/test_drain_cpu.py checks them on the model).
"""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from kubernetesclustercapacity_amd import _lib
from kubernetesclustercapacity_amd.engine import KccError
from tests import drain_model as drm
from tests import ext_model as xm
from tests import spread_model as spm
from tests import test_gpu_fuzz_cells as fz
from tests.test_deploy import plain_case

TILE = _lib.KCC_DEPLOY_TILE
PACK, SPREAD = _lib.KCC_DEPLOY_PACK, _lib.KCC_DEPLOY_SPREAD
POLICIES = [PACK, SPREAD]
SIZES = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17]
i64, u64 = np.int64, np.uint64
SHAPE_FIELDS = ("shape_cpu", "shape_mem", "shape_x", "shape_count", "shape_placed", "shape_nodes",
                "shape_err")
STATE_FIELDS = ("pod_count", "used_cpu", "used_mem", "used_x")
# (drained fraction, pod_movable given): at 0.3 the model places every evicted pod, at 0.9 it
# leaves pods unplaced (tests/test_drain_cpu.py asserts both on the model)
MIXES = [(0.3, True), (0.9, True), (0.3, False)]


# ---- generators (no GPU) -------------------------------------------------------------------
def palette(rng, k, R):
    """k distinct plain pod shapes: (cpu [k] uint64, memory [k], x [R, k])."""
    cpu = rng.choice(np.arange(50, 3000), k, replace=False).astype(u64)
    return cpu, rng.integers(1 << 26, 1 << 31, k), rng.integers(0, 3, (R, k))


def drain_case(seed, n, R, frac, n_palette=7, movable=True, per_row=6, cover=False):
    """tests/test_deploy.plain_case's rows, integers(0, per_row) pods a row with shapes from a
    palette, a drained fraction of the rows and (movable) pod_movable about 80 % set.
    cover: the evicted pods take the palette's shapes in rotation, so every shape occurs (when
    there are at least n_palette evicted pods)."""
    base = plain_case(seed, n, 1, R)
    rng = np.random.default_rng([seed, n, R, n_palette, 0xD7A1])
    per = rng.integers(0, per_row + 1, n)
    ptr = np.concatenate([[0], np.cumsum(per)]).astype(i64)
    P = int(ptr[-1])
    pal_c, pal_m, pal_x = palette(rng, n_palette, R)
    idx = rng.integers(0, n_palette, P)
    drain = (rng.random(n) < frac).astype(np.uint8)
    mv = (rng.random(P) < 0.8).astype(np.uint8) if movable else None
    if cover:
        ev = np.flatnonzero(np.repeat(drain, per).astype(bool) & (True if mv is None else mv != 0))
        idx[ev] = np.arange(ev.size) % n_palette
    return dict(rows=base["rows"], ax=base["ax"], ux=base["ux"], drain=drain, ptr=ptr,
                pc=pal_c[idx], pm=pal_m[idx], px=pal_x[:, idx], mv=mv)


def hand_case(n, R, drain, per_row, pods, rows=None):
    """n roomy rows (or `rows`), per_row[i] pods on row i, pods = a list of (cpu, mem, x...)."""
    if rows is None:
        rows = [np.full(n, 64000, u64), np.full(n, 1 << 40, i64), np.full(n, 1 << 30, i64),
                np.zeros(n, i64), np.zeros(n, u64), np.zeros(n, i64)]
    ptr = np.concatenate([[0], np.cumsum(np.asarray(per_row, i64))]).astype(i64)
    assert ptr[-1] == len(pods)
    P = len(pods)
    pc = np.array([p[0] for p in pods], u64) if P else np.zeros(0, u64)
    pm = np.array([p[1] for p in pods], i64) if P else np.zeros(0, i64)
    px = np.array([[p[2 + r] for p in pods] for r in range(R)], i64).reshape(R, P)
    return dict(rows=rows, ax=np.full((R, n), 1 << 20, i64), ux=np.zeros((R, n), i64),
                drain=np.asarray(drain, np.uint8), ptr=ptr, pc=pc, pm=pm, px=px, mv=None)


def model_of(case, policy, max_shapes=64, model=drm.drain):
    return model(case["rows"], case["ax"], case["ux"], case["drain"], case["ptr"], case["pc"],
                 case["pm"], case["px"], case["mv"], policy, max_shapes)


def compare(got, want, msg):
    assert (got.drained_rows, got.evicted, got.shapes, got.placed) == \
        (want.drained_rows, want.evicted, want.shapes, want.placed), f"summary: {msg}"
    for f in SHAPE_FIELDS + STATE_FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.shape == w.shape and g.dtype == w.dtype, f"{f}: {msg}"
        np.testing.assert_array_equal(g, w, err_msg=f"{f}: {msg}")


def run(engine, case, policy, max_shapes=64, model=drm.drain, msg=""):
    """The device call (host form) and the model on one input; everything compared."""
    keys = ("drain", "ptr", "pc", "pm", "px", "mv", "ax", "ux")
    before = [np.array(a, copy=True) for a in case["rows"]] + \
        [None if case[k] is None else np.array(case[k], copy=True) for k in keys]
    got = engine.drain(*case["rows"], case["drain"], case["ptr"], case["pc"], case["pm"], policy,
                       case["ax"], case["ux"], case["px"], case["mv"], max_shapes)
    for a, b in zip(list(case["rows"]) + [case[k] for k in keys], before):  # inputs not mutated
        if b is not None:
            np.testing.assert_array_equal(a, b, err_msg=f"input mutated: {msg}")
    want = model_of(case, policy, max_shapes, model)
    compare(got, want, msg)
    return got, want


def padded(res, M):
    """A host-form or model result as the async form writes it: the shape arrays [M], zeros
    behind the shapes."""
    D = max(res.shapes, 0)
    out = {"summary": np.array([res.drained_rows, res.evicted, res.shapes, res.placed], i64)}
    for f in SHAPE_FIELDS:
        a = getattr(res, f)
        full = np.zeros(a.shape[:-1] + (M,), a.dtype)
        full[..., :D] = a
        out[f] = full
    for f in STATE_FIELDS:
        out[f] = getattr(res, f)
    return out


# ---- the device form, through torch tensors -------------------------------------------------
def to_dev(a, dev):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)


class AsyncCall:
    """One case resident on the device: call(stream) resets the working state from the pristine
    copy and enqueues drain_async; read() brings every output back as padded() lays it out."""

    def __init__(self, eng, case, policy, M, dev):
        import torch
        self.eng, self.policy, self.M, self.R = eng, policy, M, case["ax"].shape[0]
        rows = case["rows"]
        self.n = rows[0].size
        self.alloc = [to_dev(rows[k], dev) for k in range(3)]
        self.ax = to_dev(case["ax"], dev)
        self.pristine = [to_dev(rows[3], dev), to_dev(rows[4], dev), to_dev(rows[5], dev),
                         to_dev(case["ux"], dev)]
        self.work = [torch.empty_like(t) for t in self.pristine]
        self.pods = [to_dev(case[k], dev) for k in ("drain", "ptr", "pc", "pm", "px")]
        self.mv = None if case["mv"] is None else to_dev(case["mv"], dev)
        full = lambda k, t: torch.empty(k, dtype=t, device=dev)  # noqa: E731
        self.outs = dict(summary=full(4, torch.int64), shape_cpu=full(M, torch.int64),
                         shape_mem=full(M, torch.int64), shape_x=full(self.R * M, torch.int64),
                         shape_count=full(M, torch.int64), shape_placed=full(M, torch.int64),
                         shape_nodes=full(M, torch.int64), shape_err=full(M, torch.int32))

    def call(self, stream):
        for w, p in zip(self.work, self.pristine):
            w.copy_(p)
        o = self.outs
        self.eng.drain_async(*self.alloc, self.R, self.ax, *self.work, *self.pods, self.mv,
                             self.policy, self.M, o["summary"], o["shape_cpu"], o["shape_mem"],
                             o["shape_x"], o["shape_count"], o["shape_placed"], o["shape_nodes"],
                             o["shape_err"], stream=stream)

    def poison(self):
        for t in list(self.outs.values()) + self.work:
            t.fill_(77)

    def read(self):
        got = {k: v.cpu().numpy() for k, v in self.outs.items()}
        got["shape_cpu"] = got["shape_cpu"].view(np.uint64)
        got["shape_x"] = got["shape_x"].reshape(self.R, self.M)
        st_ = [w.cpu().numpy() for w in self.work]
        got.update(pod_count=st_[0], used_cpu=st_[1].view(np.uint64), used_mem=st_[2],
                   used_x=st_[3].reshape(self.R, self.n))
        return got


def compare_padded(got, want, msg):
    for f in ("summary",) + SHAPE_FIELDS + STATE_FIELDS:
        assert got[f].shape == want[f].shape and got[f].dtype == want[f].dtype, f"{f}: {msg}"
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{f}: {msg}")


# ---- sizes x R x policy x mix ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("frac,movable", MIXES)
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("R", [0, 2])
@pytest.mark.parametrize("n", SIZES)
def test_sizes(engine, n, R, policy, frac, movable):
    case = drain_case(n, n, R, frac, movable=movable)
    got, _ = run(engine, case, policy, msg=f"n={n} R={R} policy={policy} frac={frac} mv={movable}")
    if n >= 63:
        assert got.evicted > 0
        assert got.placed == got.evicted if frac == 0.3 else got.placed < got.evicted


# ---- the table's edges ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("D", [1, 2, 3, 7])
def test_table_full_and_one_over(engine, D, policy):
    """max_shapes == D: every claim counts up to the limit and not past it.  max_shapes == D - 1:
    overflow — the drained rows are full, nothing else changes."""
    case = drain_case(40 + D, 65, 2, 0.5, n_palette=D, cover=True)
    got, want = run(engine, case, policy, max_shapes=D, msg=f"D={D} policy={policy}")
    assert want.shapes == D and got.placed > 0
    if D > 1:
        got, want = run(engine, case, policy, max_shapes=D - 1, msg=f"D={D} over policy={policy}")
        assert got.shapes == -1 and got.placed == 0 and got.shape_cpu.size == 0
        assert got.evicted == want.evicted > 0
        full = drm.fill_drained(case["rows"], case["ax"], case["ux"], case["drain"])
        for g, w in zip((got.pod_count, got.used_cpu, got.used_mem, got.used_x), full):
            np.testing.assert_array_equal(g, w)


@pytest.mark.gpu
def test_thousand_shapes(engine):
    """D = max_shapes = 1000 at N = 65: the rank pass over a table of 2048 slots, half full."""
    case = drain_case(5, 65, 1, 0.5, n_palette=1000, per_row=100, cover=True)
    got, want = run(engine, case, SPREAD, max_shapes=1000, msg="D=1000")
    assert want.shapes == 1000
    got, _ = run(engine, case, SPREAD, max_shapes=999, msg="D=1000 over")
    assert got.shapes == -1


@pytest.mark.gpu
@pytest.mark.parametrize("M", [0, _lib.KCC_DRAIN_MAX_SHAPES + 1, -3])
def test_max_shapes_out_of_range(engine, M):
    case = drain_case(1, 5, 0, 0.5)
    with pytest.raises(KccError) as e:
        engine.drain(*case["rows"], case["drain"], case["ptr"], case["pc"], case["pm"],
                     max_shapes=M)
    assert e.value.code == _lib.KCC_EINVAL


# ---- key equality and order -------------------------------------------------------------------
def key_case():
    """Every row drained (only the shape outputs matter): shapes that differ in the last extra
    word alone, cpu on both sides of 2^63 (unsigned order), negative memory and negative extra
    words (signed order), each shape on several pods spread over the rows."""
    big = 1 << 63
    shapes = [(7, 5, 1, 1), (7, 5, 1, 2), (7, 5, 1, -2), (7, 5, 0, 2),
              (big - 1, 1, 0, 0), (big, 1, 0, 0), (big + 1, 1, 0, 0), ((1 << 64) - 1, 9, 0, 0),
              (0, 3, 0, 0), (7, -5, 1, 1), (7, -(1 << 62), 0, 0), (7, (1 << 62), 0, 0),
              (7, 5, -(1 << 63), 0), (7, 5, (1 << 63) - 1, 0), (big, -1, -1, -1), (big, -1, -1, 0)]
    pods = [shapes[(3 * k) % len(shapes)] for k in range(5 * len(shapes))] + shapes[:5]
    per = [len(pods) - 40, 17, 0, 23]
    return hand_case(4, 2, [1, 1, 1, 1], per, pods), len(shapes)


@pytest.mark.gpu
@pytest.mark.parametrize("policy", POLICIES)
def test_key_equality_and_order(engine, policy):
    case, D = key_case()
    got, want = run(engine, case, policy, max_shapes=D, msg="keys")
    assert got.shapes == D and got.placed == 0 and got.evicted == case["pc"].size
    assert got.shape_cpu[0] == np.uint64((1 << 64) - 1) and got.shape_cpu[-1] == 0


# ---- degenerate cases -------------------------------------------------------------------------
def degenerate_cases():
    base = drain_case(9, 70, 2, 0.4)
    n, P = 70, base["pc"].size
    none = dict(base, drain=np.zeros(n, np.uint8))
    every = dict(base, drain=np.ones(n, np.uint8))
    empty = np.zeros(n, np.uint8)
    empty[np.flatnonzero(np.diff(base["ptr"]) == 0)] = 1  # only rows that run nothing
    unmovable = dict(base, mv=np.zeros(P, np.uint8))
    no_pods = dict(base, ptr=np.zeros(n + 1, i64), pc=np.zeros(0, u64), pm=np.zeros(0, i64),
                   px=np.zeros((2, 0), i64), mv=None)
    return dict(none=none, every=every, empty_rows=dict(base, drain=empty), unmovable=unmovable,
                no_pods=no_pods)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["none", "every", "empty_rows", "unmovable", "no_pods"])
def test_degenerate(engine, name):
    case = degenerate_cases()[name]
    got, _ = run(engine, case, SPREAD, msg=name)
    rows = case["rows"]
    if name == "none":
        assert (got.drained_rows, got.evicted, got.shapes, got.placed) == (0, 0, 0, 0)
        for g, w in zip((got.pod_count, got.used_cpu, got.used_mem, got.used_x),
                        (rows[3], rows[4], rows[5], case["ux"])):
            np.testing.assert_array_equal(g, w)
    elif name == "every":
        assert got.drained_rows == 70 and got.evicted > 0 and got.placed == 0
    else:
        assert got.drained_rows > 0 and (got.evicted, got.shapes, got.placed) == (0, 0, 0)


@pytest.mark.gpu
def test_no_nodes(engine):
    z = lambda t: np.zeros(0, t)  # noqa: E731
    got = engine.drain(z(u64), z(i64), z(i64), z(i64), z(u64), z(i64), z(np.uint8), z(i64),
                       z(u64), z(i64), max_shapes=8)
    assert (got.drained_rows, got.evicted, got.shapes, got.placed) == (0, 0, 0, 0)
    assert got.shape_cpu.size == 0 and got.pod_count.size == 0


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["first", "decreasing", "last"])
def test_bad_csr_is_einval(engine, bad):
    case = drain_case(2, 20, 0, 0.5)
    ptr = case["ptr"].copy()
    if bad == "first":
        ptr[0] = 1
    elif bad == "decreasing":
        k = int(np.flatnonzero(np.diff(ptr) > 0)[1])
        ptr[k] = ptr[k + 1] + 1
    else:
        ptr[-1] += 1
    with pytest.raises(KccError) as e:
        engine.drain(*case["rows"], case["drain"], ptr, case["pc"], case["pm"])
    assert e.value.code == _lib.KCC_EINVAL


# ---- a flagged shape --------------------------------------------------------------------------
def flagged_case():
    """Row 0 drained; its pods: a zero-memory shape with the largest cpu (the first step: it
    meets free memory and is flagged), two ordinary shapes behind it, and a zero-cpu shape (the
    last step: it meets free CPU and is flagged)."""
    pods = [(3000, 0), (1000, 1 << 26), (500, 1 << 27), (1000, 1 << 26), (0, 1 << 20), (3000, 0)]
    return hand_case(5, 0, [1, 0, 0, 0, 0], [6, 0, 0, 0, 0], pods)


@pytest.mark.gpu
@pytest.mark.parametrize("policy", POLICIES)
def test_flagged_shape(engine, policy):
    got, _ = run(engine, flagged_case(), policy, msg="flagged")
    assert got.shape_err.tolist() == [1, 0, 0, 1]
    assert got.shape_placed.tolist() == [0, 2, 1, 0] and got.placed == 3 and got.evicted == 6


# ---- skew -------------------------------------------------------------------------------------
def skew_case():
    """One drained row owns 5000 pods, its neighbours none."""
    case = drain_case(11, 65, 1, 0.0)
    rng = np.random.default_rng(11)
    per = np.zeros(65, i64)
    per[32] = 5000
    pal_c, pal_m, pal_x = palette(rng, 7, 1)
    idx = rng.integers(0, 7, 5000)
    drain = np.zeros(65, np.uint8)
    drain[31:34] = 1
    return dict(case, drain=drain, ptr=np.concatenate([[0], np.cumsum(per)]).astype(i64),
                pc=pal_c[idx], pm=pal_m[idx], px=pal_x[:, idx],
                mv=(rng.random(5000) < 0.8).astype(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("policy", POLICIES)
def test_skew(engine, policy):
    got, _ = run(engine, skew_case(), policy, msg="skew")
    assert got.drained_rows == 3 and 3500 < got.evicted < 4500 and got.shapes == 7


# ---- property test ----------------------------------------------------------------------------
@pytest.mark.gpu
@settings(max_examples=40, derandomize=True, deadline=None,
          suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])
@given(seed=st.integers(0, 2**32 - 1),
       n=st.one_of(st.sampled_from([2 * TILE, TILE + 1, 257, 65, 64, 1]), st.integers(1, 600)),
       n_palette=st.integers(1, 40), frac=st.sampled_from([0.0, 0.1, 0.3, 0.6, 0.9, 1.0]),
       R=st.integers(0, 2), policy=st.sampled_from(POLICIES), movable=st.booleans(),
       M=st.sampled_from([1, 5, 16, 64]))
def test_drain_property(engine, seed, n, n_palette, frac, R, policy, movable, M):
    case = drain_case(seed, n, R, frac, n_palette=n_palette, movable=movable)
    run(engine, case, policy, max_shapes=M,
        msg=f"seed={seed} n={n} palette={n_palette} frac={frac} R={R} policy={policy} "
            f"mv={movable} M={M}")


# ---- host form against async form -------------------------------------------------------------
ASYNC_CASES = {  # name: (case arguments, max_shapes)
    "padding": (dict(seed=21, n=TILE + 9, R=2, frac=0.3), 64),       # D = 7 of 64: padding steps
    "exact": (dict(seed=22, n=65, R=0, frac=0.5, cover=True), 7),    # D == max_shapes
    "overflow": (dict(seed=23, n=300, R=1, frac=0.5, cover=True), 4),
    "none_drained": (dict(seed=24, n=65, R=2, frac=0.0), 16),
}


@pytest.mark.gpu
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", list(ASYNC_CASES))
def test_host_form_equals_async_form(engine, name, policy):
    import torch
    dev = torch.device("cuda", 0)
    kw, M = ASYNC_CASES[name]
    case = drain_case(**kw)
    host, want = run(engine, case, policy, max_shapes=M, msg=name)
    ac = AsyncCall(engine, case, policy, M, dev)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        ac.poison()
        ac.call(stream)
    stream.synchronize()
    got = ac.read()
    compare_padded(got, padded(host, M), f"async vs host: {name}")
    compare_padded(got, padded(want, M), f"async vs model: {name}")
    if name == "overflow":
        assert got["summary"][2] == -1
    if name == "padding":
        assert 0 < got["summary"][2] < M and got["summary"][3] > 0


# ---- in a graph with the fit that follows -----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("policy", POLICIES)
def test_graph_drain_then_fit(policy):
    """One linear graph: the pristine state copied to the working state, drain_async with
    max_shapes = 16 (9 of the steps padding), fit_capped_async on the result.  Replayed twice
    with the outputs poisoned in between: both replays equal the eager run (the host forms)
    and the model."""
    import torch

    from conftest import init_torch_first
    from kubernetesclustercapacity_amd import CapacityEngine
    init_torch_first()
    dev = torch.device("cuda", 0)
    n, R, G, S, M = 2 * TILE + 77, 2, 4, 5, 16
    case = drain_case(31, n, R, 0.3)
    rows, ax = case["rows"], case["ax"]
    gid = fz.group_layout(31, n, G, "uniform")
    fit = plain_case(32, n, S, R)  # the specs of the fit that follows
    fcap = np.array([0, 1, 4, 0, 2], i64)
    want = model_of(case, policy, M)
    assert want.shapes == 7 and want.placed > 0
    q, dz = xm.pair_table([rows[0], rows[1], rows[2], want.pod_count, want.used_cpu, want.used_mem],
                          ax, want.used_x, fit["sc"], fit["sm"], fit["sx"])
    assert not q[case["drain"] != 0].any() and not dz[case["drain"] != 0].any()
    wt, we, _, _ = spm.capped_cells(q, dz, gid, G, fcap)

    with CapacityEngine(0, 1) as eng:
        eager = eng.drain(*rows, case["drain"], case["ptr"], case["pc"], case["pm"], policy, ax,
                          case["ux"], case["px"], case["mv"], M)
        compare(eager, want, "eager vs model")
        et, ee, _, _ = eng.fit_capped(rows[0], rows[1], rows[2], eager.pod_count, eager.used_cpu,
                                      eager.used_mem, ax, eager.used_x, fit["sc"], fit["sm"],
                                      fit["sx"], gid, G, fcap, want_min=False, want_rows=False)
        ac = AsyncCall(eng, case, policy, M, dev)
        d_gid = to_dev(gid, dev)
        f_sc, f_sm, f_sx, f_cap = (to_dev(a, dev) for a in (fit["sc"], fit["sm"], fit["sx"], fcap))
        t = torch.empty(G * S, dtype=torch.int64, device=dev)
        e = torch.empty(G * S, dtype=torch.int32, device=dev)

        def capture(stream):
            ac.call(stream)
            eng.fit_capped_async(*ac.alloc, ac.work[0], ac.work[1], ac.work[2], R, ac.ax,
                                 ac.work[3], d_gid, G, f_sc, f_sm, f_sx, t, e, f_cap,
                                 stream=stream)

        stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(stream):  # warm-up: every workspace allocated
            capture(stream)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            capture(stream)
        for rep_no in range(2):
            with torch.cuda.stream(stream):
                ac.poison()
                t.fill_(77)
                e.fill_(77)
                g.replay()
            stream.synchronize()
            got = ac.read()
            for ref, name in ((eager, "eager"), (want, "model")):
                compare_padded(got, padded(ref, M), f"vs {name}: replay {rep_no}")
            for ref_t, ref_e, name in ((et, ee, "eager"), (wt, we, "model")):
                np.testing.assert_array_equal(t.cpu().numpy().reshape(G, S), ref_t,
                                              err_msg=f"fit totals vs {name}: replay {rep_no}")
                np.testing.assert_array_equal(e.cpu().numpy().reshape(G, S), ref_e,
                                              err_msg=f"fit err vs {name}: replay {rep_no}")
        del g
