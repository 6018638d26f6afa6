"""kcc_deploy on the device against tests/deploy_model.py (Python integers): exact equality of
placed, nodes_used, err, the per-row placement and all four state arrays.

Sizes sit around the row pass's tile (_lib.KCC_DEPLOY_TILE) and the first N at which the scan
of the tile sums takes a second pass of its workgroup; the hand-built cases put PACK's boundary
and SPREAD's remainder rows on tile edges and drive the digit search's top and lowest rounds;
the adversarial rows are tests/test_gpu_fuzz_cells.make_cell_case's.  The generators are
importable without a GPU (tests/test_deploy_cpu.py checks them on the model).
"""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from kubernetesclustercapacity_amd import _lib
from tests import deploy_model as dm
from tests import ext_model as xm
from tests import spread_model as spm
from tests import test_gpu_fuzz_cells as fz

TILE = _lib.KCC_DEPLOY_TILE
SCAN_N = _lib.KCC_DEPLOY_SCAN_PASS * TILE + 1  # the scan's second pass holds one tile sum
PACK, SPREAD = _lib.KCC_DEPLOY_PACK, _lib.KCC_DEPLOY_SPREAD
POLICIES = [PACK, SPREAD]
SIZES = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17]
I64 = np.iinfo(np.int64)
i64, u64 = np.int64, np.uint64
FIELDS = ("err", "placed", "nodes_used", "rows", "pod_count", "used_cpu", "used_mem", "used_x")


# ---- generators (no GPU) -------------------------------------------------------------------
def plain_case(seed, n, K, R):
    """An ordinary cluster and plan: non-negative values, nothing wraps, nothing panics.  About
    a tenth of the rows are full on CPU, a tenth are over their pod limit (a negative clamp
    value) and a third have a pod limit no quotient reaches."""
    rng = np.random.default_rng([seed, n, K, R, 0xDE9])
    ac = rng.integers(1000, 64001, n)
    uc = (ac * rng.random(n) * 0.9).astype(i64)
    uc[rng.random(n) < 0.1] = ac.max() + 5
    am = rng.integers(1 << 32, 1 << 38, n)
    um = (am * rng.random(n) * 0.9).astype(i64)
    ap = rng.choice(np.array([3, 30, 110, 1 << 40], i64), n, p=[0.2, 0.2, 0.3, 0.3])
    pc = rng.integers(0, 100, n)
    over = rng.random(n) < 0.1
    pc[over] = ap[over] % 1000 + rng.integers(1, 9, int(over.sum()))
    ax = rng.integers(0, 65, (R, n))
    ux = (ax * rng.random((R, n))).astype(i64)
    sc = rng.integers(50, 3000, K).astype(u64)
    sm = rng.integers(1 << 26, 1 << 31, K)
    sx = rng.integers(0, 3, (R, K))
    rows = [ac.astype(u64), am, ap, pc, uc.astype(u64), um]
    return dict(rows=rows, ax=ax, ux=ux, sc=sc, sm=sm, sx=sx)


def uniform_case(n, per_row, R=0):
    """Every row holds exactly per_row[i] pods of the one spec (1000 millicores; memory and the
    pod limit never bind)."""
    a = np.broadcast_to(np.asarray(per_row, i64), (n,))
    rows = [(a * 1000 + 999).astype(u64), np.full(n, 1 << 50, i64), np.full(n, 1 << 62, i64),
            np.zeros(n, i64), np.zeros(n, u64), np.zeros(n, i64)]
    return dict(rows=rows, ax=np.full((R, n), 1 << 40, i64), ux=np.zeros((R, n), i64),
                sc=np.array([1000], u64), sm=np.array([1], i64), sx=np.ones((R, 1), i64))


def scan_case():
    """SCAN_N plain rows, one step, one extra resource; the last row (alone in the last tile,
    the one whose offset the scan's second pass writes) is empty, so it takes something."""
    case = plain_case(3, SCAN_N, 1, 1)
    rows = case["rows"]
    rows[2][-1] = 1 << 40
    rows[3][-1] = rows[4][-1] = rows[5][-1] = 0
    case["ax"][0, -1], case["ux"][0, -1] = 16, 0
    return case


def plan_replicas(case, K, policy, kind, gid=None, G=1, el=None, cap=None):
    """replicas [K] that bind: a share of what step k could take of the INITIAL state (later
    steps see less), in rotation a third, a half, everything and more, and nothing."""
    R = case["ax"].shape[0]
    ac, am, ap, pc, uc, um = [[int(v) for v in c] for c in case["rows"]]
    elig = dm._eligibility(len(ac), K, gid, G, el)
    rep = np.zeros(K, i64)
    for k in range(K):
        a = dm.counts((pc, uc, um, case["ux"].tolist()), (ac, am, ap, case["ax"].tolist()),
                      (int(case["sc"][k]), int(case["sm"][k]), [int(case["sx"][r][k]) for r in range(R)]),
                      dm.R_MAX, 0 if cap is None else int(cap[k]), elig[k])
        T = 0 if a is None else sum(a)
        rep[k] = [T // 3, T // 2 + 1, 1 << 40, 0, -7, T][(k + kind) % 6]
    return rep


def run(engine, case, rep, policy, cap=None, gid=None, G=1, el=None, model=dm.deploy, msg=""):
    """The device call and the model on one input; every output and state array compared."""
    rows, ax, ux, sc, sm, sx = (case[k] for k in ("rows", "ax", "ux", "sc", "sm", "sx"))
    before = [np.array(a, copy=True) for a in rows] + [ux.copy()]
    got = engine.deploy(*rows, sc, sm, rep, policy, ax, ux, sx, cap, gid, G, el)
    for a, b in zip(list(rows) + [ux], before):  # the inputs are not mutated
        np.testing.assert_array_equal(a, b, err_msg=f"input mutated: {msg}")
    want = model(rows, ax, ux, sc, sm, sx, rep, policy, cap, gid, G, el)
    for f in FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.shape == w.shape and g.dtype == w.dtype, f"{f}: {msg}"
        np.testing.assert_array_equal(g, w, err_msg=f"{f}: {msg}")
    return got, want


# ---- sizes x K x R x policy ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("R", [0, 2])
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("n", SIZES)
def test_sizes(engine, n, K, R, policy):
    """Groups (with ids outside [0, G)), eligibility, a cap that binds on some steps, and
    replicas that bind partially, fully and not at all."""
    G = 5
    case = plain_case(n + K, n, K, R)
    gid = fz.group_layout(n, n, G, "uniform" if n > 65 else "invalid40")
    el = np.random.default_rng(n + K).random((G, K)) < 0.8
    cap = np.array([0, 2, 1000, -1], i64)[:K]
    rep = plan_replicas(case, K, policy, n % 2, gid, G, el, cap)  # the first step binds partially
    got, _ = run(engine, case, rep, policy, cap, gid, G, el, msg=f"n={n} K={K} R={R} policy={policy}")
    if n >= 63:
        assert got.placed.sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("policy", POLICIES)
def test_scan_second_pass(engine, policy):
    """SCAN_N rows: the tile sums need a second pass of the scan's workgroup.  The numpy model
    on plain inputs; PACK's boundary lands in the last tile, SPREAD's remainder too."""
    n, K, R = SCAN_N, 1, 1
    case = scan_case()
    a0 = dm.deploy_np(case["rows"], case["ax"], case["ux"], case["sc"], case["sm"], case["sx"],
                      [1 << 40], PACK).rows[0]
    T = int(a0.sum())
    assert a0[-1] > 1 and a0[:-1].sum() > 0
    rep = np.array([T - 1], i64)  # PACK: the last row misses one; SPREAD: rem is one short
    got, _ = run(engine, case, rep, policy, model=dm.deploy_np, msg=f"n={n} policy={policy}")
    assert got.placed[0] == T - 1 and got.rows[0, -1] in (a0[-1], a0[-1] - 1)


# ---- hand-built cases ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_pack_boundary_on_tile_edges(engine, delta):
    """3 per row: R = 3 TILE fills tile 0 exactly (the boundary on its last row), + 1 puts one
    on the first row of tile 1 (mid-row), - 1 leaves tile 0's last row one short (mid-row)."""
    n = 2 * TILE + 5
    got, _ = run(engine, uniform_case(n, 3), np.array([3 * TILE + delta], i64), PACK, msg=f"delta={delta}")
    assert got.rows[0, TILE - 1] == 3 + min(delta, 0) and got.rows[0, TILE] == max(delta, 0)
    assert got.rows[0, TILE + 1:].sum() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["equal", "straddle", "exact", "one_short"])
def test_spread_equal_rows(engine, name):
    """Every a_i = 3 over two tiles and a bit: the remainder rows end inside tile 0, straddle
    the edge of tiles 0 / 1, vanish (sum min(a, t) == Rk exactly: every row takes t) and cover
    every row but the last."""
    n = 2 * TILE + 5
    rem = {"equal": 7, "straddle": TILE + 5, "exact": n, "one_short": n - 1}[name]
    got, _ = run(engine, uniform_case(n, 3), np.array([n + rem], i64), SPREAD, msg=name)
    assert (got.rows[0, :rem] == 2).all() and (got.rows[0, rem:] == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("policy", POLICIES)
def test_huge_row_and_top_round(engine, policy):
    """One row whose raw q is 2^40: its a is clipped at Rk = 2^31 - 1 (replicas above that are
    clamped), T exceeds Rk, and SPREAD's level t has a nonzero digit in the search's top round."""
    n = TILE + 9
    case = uniform_case(n, 5)
    case["rows"][0][17] = u64((1 << 40) * 1000)
    got, want = run(engine, case, np.array([1 << 45], i64), policy, msg=f"policy={policy}")
    assert got.placed[0] == dm.R_MAX
    assert got.rows[0, 17] == (dm.R_MAX - (5 * 17 if policy == PACK else 5 * (n - 1)))
    assert got.rows[0, 17] >> 24 == 127


@pytest.mark.gpu
def test_spread_low_round_digits(engine):
    """a_i = 0x010200 + (0 .. 255): the rows share every digit but the last round's."""
    n = TILE + 300
    a = 0x010200 + (np.arange(n) * 37) % 256
    case = uniform_case(n, a)
    T = int(a.sum())
    for rep in (T * 6 // 10, T - 200, 0x010200 * n + 3, 0x010200 * n, 5):
        got, _ = run(engine, case, np.array([rep], i64), SPREAD, msg=f"rep={rep}")
        assert got.placed[0] == rep


@pytest.mark.gpu
@pytest.mark.parametrize("policy", POLICIES)
def test_flagged_step_clamped_replicas_and_untouched_extra(engine, policy):
    """K = 5: step 1 asks for 0 millicores (Go panics on every row with free CPU: flagged, the
    state untouched, later steps still placed), step 2's eligible column is all zero, step 3
    has negative replicas, step 4 more than 2^31 - 1.  Resource 1 is never requested: its used
    column, full-range int64 noise, comes back bit for bit."""
    n, K, R, G = TILE + 65, 5, 2, 3
    case = plain_case(9, n, K, R)
    rng = np.random.default_rng(9)
    case["ux"][1] = rng.integers(I64.min, I64.max, n, dtype=i64)
    case["sx"][0] = [1, 1, 2, 1, 1]
    case["sx"][1] = 0
    case["sc"][1] = 0
    gid = fz.group_layout(9, n, G, "uniform")
    el = np.ones((G, K), bool)
    el[:, 2] = False
    rep = np.array([300, 50, 50, -3, 1 << 33], i64)
    got, _ = run(engine, case, rep, policy, None, gid, G, el, msg=f"policy={policy}")
    assert got.err.tolist() == [0, 1, 0, 0, 0]
    assert got.placed[0] == 300 and got.placed[1:4].tolist() == [0, 0, 0] and got.placed[4] > 300
    np.testing.assert_array_equal(got.used_x[1], case["ux"][1])
    # the panicking rows made ineligible: the step is not flagged
    el2 = el.copy()
    el2[:, 1] = False
    got, _ = run(engine, case, rep, policy, None, gid, G, el2, msg=f"policy={policy} ineligible")
    assert got.err.tolist() == [0] * K


@pytest.mark.gpu
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("seed,n,R", [(1, 1025, 2), (2, 257, 4), (3, 2049, 0), (4, 65, 1)])
def test_adversarial_rows(engine, seed, n, R, policy):
    """make_cell_case's rows and specs: wrapping differences, negative requests, MinInt64 / -1,
    zero requests (flagged steps between placed ones), with group ids and eligibility."""
    K, G = 4, 7
    flagged = 0
    for sub in range(3):
        case = fz.make_cell_case(seed * 10 + sub, n, K, R)
        gid = fz.group_layout(seed + sub, n, G, ["zipf", "invalid40", "none"][sub])
        g1 = 1 if gid is None else G
        el = None if sub == 1 else np.random.default_rng(seed).random((g1, K)) < 0.7
        cap = fz.node_caps(seed + sub, K)
        rep = plan_replicas(case, K, policy, sub, gid, g1, el, cap)
        got, _ = run(engine, case, rep, policy, cap, gid, g1, el, msg=f"seed={seed} sub={sub} n={n} R={R}")
        flagged += int(got.err.sum())
    print("flagged steps", flagged, "of", 3 * K)


# ---- against the existing entry points -----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("cap", [0, 2])
def test_cross_check_with_fit_capped(engine, policy, cap):
    """An ordinary cluster without a negative q: one step of Rk = 2^31 - 1 places fit_capped's
    total for that spec and cap, and a fit_capped of the same spec on the returned state gives 0
    on every row where the pod-slot clamp cannot fire."""
    n, R = 3 * TILE + 17, 2
    case = plain_case(21, n, 1, R)
    rows = case["rows"]
    rows[3] = np.minimum(rows[3], rows[2])  # pod_count <= alloc_pods: no negative clamp value
    rows[2] = np.where(rows[2] > 1000, rows[2], 1 << 40)  # ... and the clamp never fires
    capv = np.array([cap], i64)
    t, e, _, _ = engine.fit_capped(*rows, case["ax"], case["ux"], case["sc"], case["sm"], case["sx"],
                                   node_cap=capv, want_min=False, want_rows=False)
    got, _ = run(engine, case, np.array([dm.R_MAX], i64), policy, capv, msg=f"policy={policy} cap={cap}")
    assert e[0] == 0 and got.placed[0] == t[0] > 0
    t2, e2, _, _ = engine.fit_capped(rows[0], rows[1], rows[2], got.pod_count, got.used_cpu,
                                     got.used_mem, case["ax"], got.used_x, case["sc"], case["sm"],
                                     case["sx"], node_cap=capv, want_min=False, want_rows=False)
    if cap == 0:
        assert t2[0] == 0 and e2[0] == 0
    else:  # what the cap held back is still there
        q, dz = xm.pair_table(rows, case["ax"], case["ux"], case["sc"], case["sm"], case["sx"])
        left = np.minimum(np.maximum(q[:, 0] - cap, 0), cap).sum()
        assert t2[0] == left and e2[0] == 0


# ---- property test -------------------------------------------------------------------------
@pytest.mark.gpu
@settings(max_examples=60, derandomize=True, deadline=None,
          suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])
@given(seed=st.integers(0, 2**32 - 1),
       n=st.one_of(st.sampled_from([600, 513, 257, 65, 64, 1]), st.integers(1, 600)),
       K=st.integers(1, 4), R=st.integers(0, 2), policy=st.sampled_from(POLICIES),
       rkind=st.integers(0, 5), cap_on=st.booleans(),
       kind=st.sampled_from(["none", "uniform", "zipf", "sorted", "invalid60", "one", "all_invalid"]),
       el_on=st.booleans(), adversarial=st.booleans())
def test_deploy_property(engine, seed, n, K, R, policy, rkind, cap_on, kind, el_on, adversarial):
    G = 1 if kind == "none" else 6
    case = fz.make_cell_case(seed, n, K, R) if adversarial else plain_case(seed, n, K, R)
    gid = fz.group_layout(seed, n, G, kind)
    el = (np.random.default_rng(seed).random((G, K)) < 0.75) if el_on else None
    cap = fz.node_caps(seed, K) if cap_on else None
    rep = plan_replicas(case, K, policy, rkind, gid, G, el, cap)
    run(engine, case, rep, policy, cap, gid, G, el,
        msg=f"seed={seed} n={n} K={K} R={R} policy={policy} rkind={rkind} cap={cap_on} kind={kind} "
            f"el={el_on} adversarial={adversarial}")


# ---- in a graph with the fit that follows ---------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("policy", POLICIES)
def test_graph_deploy_then_fit(policy):
    """One linear graph: the pristine state copied to the working state, deploy_async with
    K = 3, fit_capped_async on the result.  Replayed twice: both replays equal the eager run
    (the host forms) and the model."""
    import torch

    from conftest import init_torch_first
    from kubernetesclustercapacity_amd import CapacityEngine
    init_torch_first()
    dev = torch.device("cuda", 0)
    n, K, R, G, S = 2 * TILE + 77, 3, 2, 4, 5
    case = plain_case(31, n, K, R)
    gid = fz.group_layout(31, n, G, "uniform")
    el = np.random.default_rng(31).random((G, K)) < 0.8
    cap = np.array([0, 3, 0], i64)
    rep = plan_replicas(case, K, policy, 0, gid, G, el, cap)
    rows, ax, ux, sc, sm, sx = (case[k] for k in ("rows", "ax", "ux", "sc", "sm", "sx"))
    fit = plain_case(32, n, S, R)  # the specs of the fit that follows
    fcap = np.array([0, 1, 4, 0, 2], i64)
    want = dm.deploy(rows, ax, ux, sc, sm, sx, rep, policy, cap, gid, G, el)
    q, dz = xm.pair_table([rows[0], rows[1], rows[2], want.pod_count, want.used_cpu, want.used_mem],
                          ax, want.used_x, fit["sc"], fit["sm"], fit["sx"])
    wt, we, _, _ = spm.capped_cells(q, dz, gid, G, fcap)

    def dv(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)

    with CapacityEngine(0, 1) as eng:
        eager = eng.deploy(*rows, sc, sm, rep, policy, ax, ux, sx, cap, gid, G, el)
        et, ee, _, _ = eng.fit_capped(rows[0], rows[1], rows[2], eager.pod_count, eager.used_cpu,
                                      eager.used_mem, ax, eager.used_x, fit["sc"], fit["sm"],
                                      fit["sx"], gid, G, fcap, want_min=False, want_rows=False)
        d_ac, d_am, d_ap = dv(rows[0]), dv(rows[1]), dv(rows[2])
        pristine = [dv(rows[3]), dv(rows[4]), dv(rows[5]), dv(ux)]
        work = [torch.empty_like(t) for t in pristine]
        d_ax, d_gid, d_el = dv(ax), dv(gid), dv(el.astype(np.uint8))
        d_sc, d_sm, d_sx, d_rep, d_cap = dv(sc), dv(sm), dv(sx), dv(rep), dv(cap)
        f_sc, f_sm, f_sx, f_cap = dv(fit["sc"]), dv(fit["sm"]), dv(fit["sx"]), dv(fcap)
        full = lambda k, t: torch.empty(k, dtype=t, device=dev)  # noqa: E731
        outs = dict(placed=full(K, torch.int64), nodes_used=full(K, torch.int64),
                    err=full(K, torch.int32), rows=full(K * n, torch.int64),
                    t=full(G * S, torch.int64), e=full(G * S, torch.int32))

        def capture(stream):
            for w, p in zip(work, pristine):
                w.copy_(p)
            eng.deploy_async(d_ac, d_am, d_ap, R, d_ax, work[0], work[1], work[2], work[3], d_gid,
                             G, d_el, d_sc, d_sm, d_sx, d_rep, d_cap, policy, outs["placed"],
                             outs["nodes_used"], outs["err"], outs["rows"], stream=stream)
            eng.fit_capped_async(d_ac, d_am, d_ap, work[0], work[1], work[2], R, d_ax, work[3],
                                 d_gid, G, f_sc, f_sm, f_sx, outs["t"], outs["e"], f_cap,
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
                for t in list(outs.values()) + work:
                    t.fill_(77)
                g.replay()
            stream.synchronize()
            state = [w.cpu().numpy() for w in work]
            got = dict(placed=outs["placed"], nodes_used=outs["nodes_used"], err=outs["err"],
                       rows=outs["rows"])
            got = {k: v.cpu().numpy() for k, v in got.items()}
            got.update(pod_count=state[0], used_cpu=state[1].view(np.uint64), used_mem=state[2],
                       used_x=state[3])
            for ref, name in ((eager, "eager"), (want, "model")):
                for f in FIELDS:
                    np.testing.assert_array_equal(got[f].reshape(getattr(ref, f).shape), getattr(ref, f),
                                                  err_msg=f"{f} vs {name}: replay {rep_no}")
            for ref_t, ref_e, name in ((et, ee, "eager"), (wt, we, "model")):
                np.testing.assert_array_equal(outs["t"].cpu().numpy().reshape(G, S), ref_t,
                                              err_msg=f"fit totals vs {name}: replay {rep_no}")
                np.testing.assert_array_equal(outs["e"].cpu().numpy().reshape(G, S), ref_e,
                                              err_msg=f"fit err vs {name}: replay {rep_no}")
        del g
