"""kcc_consolidate on the device against tests/consolidate_model.py: exact equality of the four
per-candidate outputs and of pod_target, and the state arrays unchanged.

Sizes sit around the walk's chunk (_lib.KCC_CONS_CHUNK) and the wavefront; the overlay cases
put KCC_CONS_MAX_PODS pods on as many rows, and on a handful; the run cases pin the shortcut for
equal shapes.  The generators are importable without a GPU (tests/test_consolidate_cpu.py checks
them on the model).
"""
import ctypes as C

import numpy as np
import pytest
from hypothesis import given, settings
from hypothesis import strategies as st

from kubernetesclustercapacity_amd import _lib
from kubernetesclustercapacity_amd.engine import KccError
from tests import consolidate_model as cm
from tests import test_gpu_fuzz_cells as fz
from tests.test_deploy import plain_case
from tests.test_drain import palette, to_dev

CHUNK = _lib.KCC_CONS_CHUNK
MAXP = _lib.KCC_CONS_MAX_PODS
SIZES = [1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17]
RS = [0, 2, 4]
i64, u64 = np.int64, np.uint64
FIELDS = ("evicted", "placed", "zero", "err", "pod_target")
GiB = 1 << 30


# ---- generators (no GPU) -------------------------------------------------------------------
def make(rows, ax, ux, per_row, pods, cand, mv=None, target=None):
    """per_row[i] pods on row i; pods = a list of (cpu, mem, x...) in row order."""
    R, n, P = ax.shape[0], rows[0].size, len(pods)
    ptr = np.concatenate([[0], np.cumsum(np.asarray(per_row, i64))]).astype(i64)
    assert ptr.size == n + 1 and ptr[-1] == P
    pc = np.array([p[0] for p in pods], u64) if P else np.zeros(0, u64)
    pm = np.array([p[1] for p in pods], i64) if P else np.zeros(0, i64)
    px = np.array([[p[2 + r] for p in pods] for r in range(R)], i64).reshape(R, P)
    return dict(rows=rows, ax=ax, ux=ux, ptr=ptr, pc=pc, pm=pm, px=px,
                mv=None if mv is None else np.asarray(mv, np.uint8),
                target=None if target is None else np.asarray(target, np.uint8),
                cand=np.asarray(cand, i64))


def slots_rows(n, R, per_row):
    """Row i holds exactly per_row[i] pods of 1000 millicores (memory, the pod limit and the
    extra resources never bind for the shapes of pod())."""
    a = np.broadcast_to(np.asarray(per_row, i64), (n,))
    rows = [(a * 1000 + 999).astype(u64), np.full(n, 1 << 50, i64), np.full(n, 1 << 40, i64),
            np.zeros(n, i64), np.zeros(n, u64), np.zeros(n, i64)]
    return rows, np.full((R, n), 1 << 40, i64), np.zeros((R, n), i64)


def pod(R, mem=1, cpu=1000):
    return (cpu, mem) + tuple(1 + r for r in range(R))


def size_case(n, R):
    """tests/test_deploy.plain_case's rows with less free CPU, 3 to 9 pods a row from a palette
    of 7 shapes, about 80 % of them movable; every third candidate runs one pod that fits
    nowhere in front of its others.  Candidates: the first and the last row, rows around the
    wavefront and the chunk, and a duplicate."""
    base = plain_case(n, n, 1, R)
    rng = np.random.default_rng([n, R, 0xC0D5])
    ac, uc = base["rows"][0].astype(i64), base["rows"][4].astype(i64)
    # little free CPU, so that a candidate's pods spread over rows: up to 5000m a row
    base["rows"][4] = np.where(uc < ac, ac - np.minimum(ac, rng.integers(0, 5000, n)), uc).astype(u64)
    per = rng.integers(3, 10, n)
    P = int(per.sum())
    pal_c, pal_m, pal_x = palette(rng, 7, R)
    idx = rng.integers(0, 7, P)
    pods = [(int(pal_c[k]), int(pal_m[k])) + tuple(int(pal_x[r, k]) for r in range(R)) for k in idx]
    mv = (rng.random(P) < 0.8).astype(np.uint8)
    cand = sorted({c for c in (0, 1, 62, 63, 64, 65, CHUNK - 1, CHUNK, n // 2, n - 2, n - 1)
                   if 0 <= c < n})
    ptr = np.concatenate([[0], np.cumsum(per)])
    for k, c in enumerate(cand):
        if k % 3 == 1:
            p = int(ptr[c])
            pods[p] = (10 ** 7,) + pods[p][1:]
            mv[p] = 1
    return make(base["rows"], base["ax"], base["ux"], per, pods, cand + cand[:1], mv)


def only_row_combos():
    """(n, candidate, the one row with room): the first, the last and the row just behind the
    candidate, the candidate being row 0 and row n - 1."""
    out = []
    for n in SIZES:
        for c in sorted({0, n - 1}):
            firsts = [i for i in (0, 1) if i != c and i < n][:1]
            lasts = [i for i in (n - 1, n - 2) if i != c and i >= 0][:1]
            after = [c + 1] if c + 1 < n else []
            for f in sorted(set(firsts + lasts + after)):
                out.append((n, c, f))
    return out


def only_row_case(n, c, f, R=2):
    """Every row is full but row f, which holds the candidate's five pods (three of one shape, a
    different one, the first again) and not a sixth."""
    per_row = np.zeros(n, i64)
    per_row[f] = 5
    rows, ax, ux = slots_rows(n, R, per_row)
    per = np.zeros(n, i64)
    per[c] = 6
    pods = [pod(R), pod(R), pod(R), pod(R, mem=2), pod(R), pod(R)]
    return make(rows, ax, ux, per, pods, [c])


def count_case(k, R=1, extra_unmovable=3):
    """65 roomy rows; row 3 runs k movable pods of two alternating shapes and some unmovable
    ones in between; row 5 runs two pods."""
    n = 65
    rows, ax, ux = slots_rows(n, R, 2000)
    pods, mv = [], []
    for q in range(k):
        pods.append(pod(R, mem=1 + (q // 3) % 2))
        mv.append(1)
        if q < extra_unmovable:
            pods.append(pod(R, mem=9))
            mv.append(0)
    per = np.zeros(n, i64)
    per[3] = len(pods)
    per[5] = 2
    pods += [pod(R), pod(R)]
    mv += [1, 1]
    return make(rows, ax, ux, per, pods, [3, 5], mv)


def overlay_case(per_row, alternate, R=4):
    """Row 0 runs KCC_CONS_MAX_PODS pods; the rows behind it hold per_row pods each (a few rows
    to spare).  alternate: two shapes in turn, so no pod takes the shortcut and every walk
    starts at row 0 and passes every row filled so far."""
    n = 1 + MAXP // per_row + 6
    per_rows = np.full(n, per_row, i64)
    per_rows[2] = 0  # a full row among them
    rows, ax, ux = slots_rows(n, R, per_rows)
    pods = [pod(R, mem=1 + (q % 2 if alternate else 0)) for q in range(MAXP)]
    per = np.zeros(n, i64)
    per[0] = MAXP
    return make(rows, ax, ux, per, pods, [0])


def runs_case(R=2):
    """Runs of equal shapes broken by another shape, placed and not placed.  Rows 1 .. 4 hold
    2, 1, 3, 2 pods of 1000m, row 5 holds 4; a pod of 9000m fits nowhere."""
    rows, ax, ux = slots_rows(8, R, [0, 2, 1, 3, 2, 4, 0, 0])
    A, B, big, z = pod(R), pod(R, mem=2), pod(R, cpu=9000), (0, 1) + (0,) * R
    pods = [A, A, A, B, A, z, A, big, big, A, big, B, B, big, big, pod(R, cpu=2000), A]
    per = [len(pods), 0, 0, 0, 0, 0, 0, 0]
    return make(rows, ax, ux, per, pods, [0])


def clamp_case():
    """Row 1: alloc_pods = 10, pod_count = 7, a resource quotient of 11 for one-core pods.  The
    clamp gives 3 while q >= 10, and stops firing once q drops below 10: the row takes more
    than 3 pods, as kcc_deploy steps would.  Row 2 is roomy."""
    rows = [np.array([4000, 11000, 64000], u64), np.full(3, 64 * GiB, i64),
            np.array([110, 10, 110], i64), np.array([0, 7, 0], i64), np.zeros(3, u64),
            np.zeros(3, i64)]
    e = np.zeros((0, 3), i64)
    return make(rows, e, e, [12, 0, 0], [(1000, GiB)] * 12, [0])


def misc_case(R=2):
    """Ten roomy rows of 4 slots; pods on rows 1, 4 and 7; zero-request and unmovable pods among
    them; rows 0 .. 2 are no targets."""
    rows, ax, ux = slots_rows(10, R, 4)
    A, B = pod(R), pod(R, mem=2)
    per = [0, 4, 0, 0, 6, 0, 0, 3, 0, 0]
    pods = [A, (0, 5) + (0,) * R, B, A,   B, B, A, (7, 0) + (1,) * R, A, B,   A, A, B]
    mv = [1, 1, 0, 1,   1, 0, 1, 1, 1, 1,   1, 1, 1]
    return make(rows, ax, ux, per, pods, [1, 4, 7, 9],
                mv, target=[0, 0, 0, 1, 1, 1, 1, 1, 1, 1])


def fuzz_case(seed, n, n_pods, R, n_cand):
    """Arbitrary 64-bit rows and pod shapes (tests/test_gpu_fuzz_cells.make_cell_case: negative
    requests, cpu above 2^63, wrapping sums), the pods dealt to the rows at random."""
    cell = fz.make_cell_case(seed, n, n_pods, R)
    rng = np.random.default_rng([seed, n, n_pods, R, 0xC0D6])
    owner = np.sort(rng.integers(0, n, n_pods))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n))]).astype(i64)
    return dict(rows=cell["rows"], ax=cell["ax"], ux=cell["ux"], ptr=ptr, pc=cell["sc"],
                pm=cell["sm"], px=cell["sx"], mv=(rng.random(n_pods) < 0.85).astype(np.uint8),
                target=(rng.random(n) < 0.8).astype(np.uint8) if seed % 2 else None,
                cand=rng.integers(-1, n + 1, n_cand).astype(i64))


def model_of(case, model=cm.consolidate):
    return model(case["rows"], case["ax"], case["ux"], case["cand"], case["ptr"], case["pc"],
                 case["pm"], case["px"], case["mv"], case["target"])


HAND = {"runs": runs_case, "clamp": clamp_case, "misc": misc_case,
        "only_last": lambda: only_row_case(CHUNK + 1, 0, CHUNK),
        "count_65": lambda: count_case(65), "toomany": lambda: count_case(MAXP + 1)}


def compare(got, want, msg):
    for f in FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.shape == w.shape and g.dtype == w.dtype, f"{f}: {msg}"
        np.testing.assert_array_equal(g, w, err_msg=f"{f}: {msg}")


def run(engine, case, model=cm.consolidate, msg=""):
    """The device call (host form) and the model on one input; everything compared, and
    nothing passed in modified."""
    keys = ("ax", "ux", "ptr", "pc", "pm", "px", "mv", "target", "cand")
    before = [np.array(a, copy=True) for a in case["rows"]] + \
        [None if case[k] is None else np.array(case[k], copy=True) for k in keys]
    got = engine.consolidate(*case["rows"], case["cand"], case["ptr"], case["pc"], case["pm"],
                             case["ax"], case["ux"], case["px"], case["mv"], case["target"])
    for a, b in zip(list(case["rows"]) + [case[k] for k in keys], before):
        if b is not None:
            np.testing.assert_array_equal(a, b, err_msg=f"input modified: {msg}")
    want = model_of(case, model)
    compare(got, want, msg)
    return got, want


# ---- the device form, through torch tensors -------------------------------------------------
class AsyncCall:
    """One case resident on the device: call(stream) enqueues consolidate_async, read() brings
    the outputs back, state() the four state arrays."""

    def __init__(self, eng, case, dev, targets=True):
        import torch
        self.eng, self.R = eng, case["ax"].shape[0]
        self.rows = [to_dev(a, dev) for a in case["rows"]]
        self.ax, self.ux = to_dev(case["ax"], dev), to_dev(case["ux"], dev)
        opt = lambda k: None if case[k] is None else to_dev(case[k], dev)  # noqa: E731
        self.target, self.mv = opt("target"), opt("mv")
        self.pods = [to_dev(case[k], dev) for k in ("ptr", "pc", "pm", "px")]
        self.cand = to_dev(case["cand"], dev)
        Cn, P = case["cand"].size, case["pc"].size
        full = lambda k, t: torch.empty(k, dtype=t, device=dev)  # noqa: E731
        self.outs = dict(evicted=full(Cn, torch.int64), placed=full(Cn, torch.int64),
                         zero=full(Cn, torch.int64), err=full(Cn, torch.int32))
        self.tgt = full(P, torch.int64) if targets else None

    def load(self, case):
        """Another case of the same sizes into the same tensors."""
        for t, a in zip(self.rows, case["rows"]):
            t.copy_(to_dev(a, t.device))
        self.ux.copy_(to_dev(case["ux"], self.ux.device))
        for t, k in zip(self.pods, ("ptr", "pc", "pm", "px")):
            t.copy_(to_dev(case[k], t.device))
        self.cand.copy_(to_dev(case["cand"], self.cand.device))
        self.ax.copy_(to_dev(case["ax"], self.ax.device))
        for t, k in ((self.target, "target"), (self.mv, "mv")):
            assert (t is None) == (case[k] is None)
            if t is not None:
                t.copy_(to_dev(case[k], t.device))

    def call(self, stream):
        r, o = self.rows, self.outs
        self.eng.consolidate_async(r[0], r[1], r[2], self.R, self.ax, r[3], r[4], r[5], self.ux,
                                   self.target, *self.pods, self.mv, self.cand, o["evicted"],
                                   o["placed"], o["zero"], o["err"], self.tgt, stream=stream)

    def poison(self):
        for t in list(self.outs.values()) + ([] if self.tgt is None else [self.tgt]):
            t.fill_(77)

    def read(self):
        o = {k: v.cpu().numpy() for k, v in self.outs.items()}
        return cm.Result(o["evicted"], o["placed"], o["zero"], o["err"],
                         None if self.tgt is None else self.tgt.cpu().numpy())


# ---- sizes x R ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes(engine, n, R):
    got, _ = run(engine, size_case(n, R), cm.consolidate_np, f"n={n} R={R}")
    if n >= 63:
        assert got.removable.any() and not got.removable.all()


@pytest.mark.gpu
@pytest.mark.parametrize("n,c,f", only_row_combos())
def test_only_fitting_row(engine, n, c, f):
    got, _ = run(engine, only_row_case(n, c, f), cm.consolidate_np, f"n={n} c={c} f={f}")
    assert got.placed.tolist() == [5] and got.pod_target.tolist() == [f] * 5 + [-1]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 64, 65, MAXP, MAXP + 1])
def test_pods_per_candidate(engine, k):
    got, _ = run(engine, count_case(k), cm.consolidate_np, f"k={k}")
    assert got.evicted.tolist() == [k, 2]
    if k > MAXP:
        assert got.err.tolist() == [_lib.KCC_CAND_TOOMANY, 0] and got.placed.tolist() == [0, 2]
        assert (got.pod_target[:-2] == -2).all() and (got.pod_target[-2:] >= 0).all()
    else:
        assert got.placed.tolist() == [k, 2] and got.removable.all()


# ---- the overlay ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("alternate", [False, True])
@pytest.mark.parametrize("per_row", [1, 100])
def test_overlay_stress(engine, per_row, alternate):
    """KCC_CONS_MAX_PODS pods that each land on a row of their own (per_row = 1: as many overlay
    slots as pods), and that fill one row after another (per_row = 100)."""
    got, _ = run(engine, overlay_case(per_row, alternate), cm.consolidate_np,
                 f"per_row={per_row} alternate={alternate}")
    assert got.placed.tolist() == [MAXP]
    assert np.unique(got.pod_target).size == (MAXP if per_row == 1 else 11)


# ---- hand cases: the shortcut, the clamp quirk, masks --------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HAND))
def test_hand_cases(engine, name):
    got, _ = run(engine, HAND[name](), msg=name)
    if name == "clamp":
        assert got.pod_target.tolist() == [1] * 11 + [2]
    if name == "runs":
        assert got.pod_target.tolist() == [1, 1, 2, 3, 3, -3, 3, -1, -1, 4, -1, 4, 5, -1, -1, 5, 5]


@pytest.mark.gpu
def test_duplicates_and_bad_rows(engine):
    case = dict(misc_case(), cand=np.array([4, 4, -1, 10, 7, 4, 1 << 40, -(1 << 62)], i64))
    got, _ = run(engine, case, msg="duplicates")
    assert got.err.tolist() == [0, 0, 1, 1, 0, 0, 1, 1]
    assert got.placed[0] == got.placed[1] == got.placed[5] > 0


@pytest.mark.gpu
def test_null_forms(engine):
    """pod_target NULL, target NULL, pod_movable NULL, pod_x NULL: the other outputs unchanged."""
    case = misc_case()
    want = model_of(case)
    got = engine.consolidate(*case["rows"], case["cand"], case["ptr"], case["pc"], case["pm"],
                             case["ax"], case["ux"], case["px"], case["mv"], case["target"],
                             want_targets=False)
    assert got.pod_target is None
    for f in FIELDS[:4]:
        np.testing.assert_array_equal(getattr(got, f), getattr(want, f), err_msg=f)
    bare = dict(case, mv=None, target=None, px=np.zeros_like(case["px"]))
    got = engine.consolidate(*bare["rows"], bare["cand"], bare["ptr"], bare["pc"], bare["pm"],
                             bare["ax"], bare["ux"])
    compare(got, model_of(bare), "NULL forms")


@pytest.mark.gpu
def test_no_candidates_and_no_nodes(engine):
    case = dict(misc_case(), cand=np.zeros(0, i64))
    got, _ = run(engine, case, msg="no candidates")
    assert got.evicted.size == 0 and (got.pod_target == -2).all()
    z = lambda t: np.zeros(0, t)  # noqa: E731
    got = engine.consolidate(z(u64), z(i64), z(i64), z(i64), z(u64), z(i64), [0, 5], z(i64),
                             z(u64), z(i64))
    assert got.evicted.tolist() == [0, 0] and got.placed.tolist() == [0, 0]
    assert got.err.tolist() == [0, 0] and got.pod_target.size == 0


# ---- property test -------------------------------------------------------------------------------
@pytest.mark.gpu
@settings(max_examples=60, **fz.FUZZ)
@given(seed=st.integers(0, 2**32 - 1), n=st.sampled_from([40, 17, 3, 2, 1]),
       n_pods=st.sampled_from([48, 20, 5]), R=st.integers(0, 4), n_cand=st.integers(1, 4))
def test_consolidate_property(engine, seed, n, n_pods, R, n_cand):
    run(engine, fuzz_case(seed, n, n_pods, R, n_cand),
        msg=f"seed={seed} n={n} pods={n_pods} R={R} cand={n_cand}")


# ---- host form against async form ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HAND))
def test_host_form_equals_async_form(engine, name):
    import torch
    dev = torch.device("cuda", 0)
    case = HAND[name]()
    host, want = run(engine, case, msg=name)
    ac = AsyncCall(engine, case, dev)
    state = [t.clone() for t in ac.rows[3:]] + [ac.ux.clone()]
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        ac.poison()
        ac.call(stream)
    stream.synchronize()
    got = ac.read()
    compare(got, host, f"async vs host: {name}")
    compare(got, want, f"async vs model: {name}")
    for a, b in zip(ac.rows[3:] + [ac.ux], state):
        assert torch.equal(a, b), "the state changed"


# ---- one graph -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_replays_on_changed_inputs():
    """consolidate_async captured once, replayed on two other inputs of the same sizes (other
    rows, other pods, other candidates): each replay equals the model."""
    import torch

    from conftest import init_torch_first
    from kubernetesclustercapacity_amd import CapacityEngine
    init_torch_first()
    dev = torch.device("cuda", 0)
    cases = [fuzz_case(seed, 40, 48, 2, 4) for seed in (101, 103, 105)]  # odd: a target mask
    with CapacityEngine(0, 1) as eng:
        ac = AsyncCall(eng, cases[0], dev)
        stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(stream):
            ac.call(stream)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            ac.call(stream)
        for case in cases[1:]:
            with torch.cuda.stream(stream):
                ac.load(case)
                ac.poison()
                g.replay()
            stream.synchronize()
            compare(ac.read(), model_of(case), "replay")
        del g


# ---- argument errors -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["first", "decreasing", "last"])
def test_bad_csr_is_einval(engine, bad):
    case = misc_case()
    ptr = case["ptr"].copy()
    if bad == "first":
        ptr[0] = 1
    elif bad == "decreasing":
        ptr[2] = ptr[3] + 1
    else:
        ptr[-1] += 1
    with pytest.raises(KccError) as e:
        engine.consolidate(*case["rows"], case["cand"], ptr, case["pc"], case["pm"], case["ax"],
                           case["ux"], case["px"])
    assert e.value.code == _lib.KCC_EINVAL


@pytest.mark.gpu
def test_argument_errors(engine):
    case = misc_case(0)
    n = 10
    with pytest.raises(KccError) as e:  # n_ext above KCC_EXT_MAX
        engine.consolidate(*case["rows"], case["cand"], case["ptr"], case["pc"], case["pm"],
                           np.zeros((5, n), i64), np.zeros((5, n), i64))
    assert e.value.code == _lib.KCC_EINVAL
    with pytest.raises(KccError) as e:  # pods without nodes
        z = lambda t: np.zeros(0, t)  # noqa: E731
        engine.consolidate(z(u64), z(i64), z(i64), z(i64), z(u64), z(i64), [0], z(i64),
                           np.ones(2, u64), np.ones(2, i64))
    assert e.value.code == _lib.KCC_EINVAL
    # through the binding: a negative n_cand, sizes past the limits, a NULL required array
    a = [np.ascontiguousarray(x) for x in case["rows"]]
    out = [np.zeros(4, i64) for _ in range(3)] + [np.zeros(4, np.int32)]
    vp = lambda x: None if x is None else C.c_void_p(x.ctypes.data)  # noqa: E731

    def call(n_nodes=n, n_pods=13, n_cand=4, alloc_cpu=a[0], cand=case["cand"], err=out[3],
             pod_cpu=case["pc"]):
        return engine._lib.kcc_consolidate(
            engine._h, n_nodes, vp(alloc_cpu), vp(a[1]), vp(a[2]), 0, None, vp(a[3]), vp(a[4]),
            vp(a[5]), None, None, n_pods, vp(case["ptr"]), vp(pod_cpu), vp(case["pm"]), None, None,
            n_cand, vp(cand), vp(out[0]), vp(out[1]), vp(out[2]), vp(err), None)

    assert call() == _lib.KCC_OK
    lim = (1 << 31) - 4096
    for kw in (dict(n_cand=-1), dict(n_cand=lim + 1), dict(n_nodes=-1), dict(n_pods=-1), dict(n_nodes=lim + 1),
               dict(n_pods=lim + 1), dict(alloc_cpu=None), dict(cand=None), dict(err=None),
               dict(pod_cpu=None)):
        assert call(**kw) == _lib.KCC_EINVAL, kw
