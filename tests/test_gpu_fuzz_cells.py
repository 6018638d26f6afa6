"""Property-based parity of the cell fits and the fold (kcc_fit_grouped, kcc_fit_ext,
kcc_fit_capped, kcc_spread_fold) against tests/ext_model.py and
tests/spread_model.py (Python integers), and with no extra resource also against the C oracle
on each group's rows.  The value mixtures aim at the pair loop's own bounds (kcc_internal.h
ext_pairs_body): free CPU around 2^31, free memory and free extras around 2^50 and negative,
requests around 2^52, whole 64-spec blocks of fast specs beside mixed ones (a wave is fast
only when its 64 specs in caller order all are), and free amounts that are k d + {-1, 0, 1}
for a request d of the same case, where the f64 estimate trunc(f (1/d)) is off by one for
about one pair in twenty and grp_div's remainder correction decides.  The group ids come in
every layout the sort (grp_hist, grp_scan, ext_scatter) and the pair loop's flush on a group
change can meet.  hypothesis draws shapes, seeds, layouts and entry points (derandomized);
numpy draws the values from the seed.  All comparisons are integer equality.

test_cell_inputs_cover_the_branches needs no GPU: it counts, from the models alone, that the
generated inputs reach the branches named above.
"""
import numpy as np
import pytest
from hypothesis import HealthCheck, example, given, settings
from hypothesis import strategies as st

from tests import ext_model as xm
from tests import spread_model as sp
from tests.test_gpu_fuzz import _mix, _near
from tests.test_groups import expected

I64 = np.iinfo(np.int64)
i64, u64 = np.int64, np.uint64
RUN = 256  # kcc_internal.h GRP_RUN

KINDS = ["zipf", "none", "blocks256", "uniform", "sorted", "invalid60", "one", "all_invalid"]
CAPS = [0, -3, 1, 2, 110, I64.max]
SKEWS = [0, -3, 1, 2, 5, I64.max]


# ---- generators ----------------------------------------------------------------------------
def group_layout(seed, n, G, kind):
    """int32 ids [n] of one layout (None for "none": the NULL group of the entry points that
    take one, G = 1).  Invalid ids are -1, G, G + 5, INT32_MIN and INT32_MAX.
      uniform      uniform over the groups, 3 % invalid
      zipf         one group holds about 70 % of the rows, the rest uniform, 3 % invalid
      sorted       uniform with 3 % invalid, ascending
      blocks256    contiguous groups of 256 or 512 rows (the last takes the rest): every
                   pair-loop run starts on a group boundary
      one          every row in group G // 2
      invalidNN    uniform, NN % invalid
      all_invalid  no valid id"""
    if kind == "none":
        return None
    rng = np.random.default_rng([seed, n, G, sum(kind.encode())])
    bad_ids = np.array([-1, G, G + 5, -(2**31), 2**31 - 1], i64)

    def spoil(gid, frac):
        bad = rng.random(n) < frac
        gid[bad] = rng.choice(bad_ids, int(bad.sum()))
        return gid

    if kind == "uniform":
        gid = spoil(rng.integers(0, G, n), 0.03)
    elif kind == "zipf":
        gid = rng.integers(0, G, n)
        gid[rng.random(n) < 0.7] = int(rng.integers(0, G))
        gid = spoil(gid, 0.03)
    elif kind == "sorted":
        gid = np.sort(spoil(rng.integers(0, G, n), 0.03))
    elif kind == "blocks256":
        gid = np.empty(n, i64)
        ids = np.sort(rng.choice(G, min(G, n // RUN + 1), replace=False))
        pos = 0
        for j, g in enumerate(ids):
            size = n - pos if j == ids.size - 1 else RUN * int(rng.integers(1, 3))
            gid[pos:pos + size] = g
            pos += size
            if pos >= n:
                break
    elif kind == "one":
        gid = np.full(n, G // 2, i64)
    elif kind.startswith("invalid"):
        gid = spoil(rng.integers(0, G, n), int(kind[len("invalid"):]) / 100.0)
    elif kind == "all_invalid":
        gid = rng.choice(bad_ids, n)
    else:
        raise ValueError(kind)
    return gid.astype(np.int32)


def _wrap_add(a, b):
    """a + b with 64-bit wrap, in a's dtype."""
    return (a.view(u64) + b.view(u64)).view(a.dtype)


def make_cell_case(seed, n, S, R, derived=0.15):
    """One cluster and spec set for the cell fits.  Returns a dict: rows (alloc_cpu, alloc_mem,
    alloc_pods, pod_count, used_cpu, used_mem), ax / ux int64 [R, n], sc uint64 [S], sm int64
    [S], sx int64 [R, S].  The used and the free amounts are drawn separately and alloc = used
    + free (wrapping), so the free-amount classes are hit by construction; the specs are drawn
    per block of 64 in caller order, about half the blocks all fast with each request from a
    pool of four values; on a `derived` share of the rows one free amount is k d + {-1, 0, 1}
    for a request d of a fast block, inside the fast bound."""
    rng = np.random.default_rng([seed, n, S, R, 0xCE11])
    zeros_i = lambda k: np.zeros(k, i64)  # noqa: E731
    full_u = lambda k: rng.integers(0, 2**64, k, dtype=u64)  # noqa: E731
    full_i = lambda k: rng.integers(-2**63, 2**63, k, dtype=i64)  # noqa: E731

    def free_signed(extra):
        parts = [(56, lambda k: rng.integers(0, 2**40, k)), (10, zeros_i),
                 (8, lambda k: _near(rng, 2**50, k, i64)),
                 (5, lambda k: -rng.integers(1, 2**40, k)),
                 (5, lambda k: I64.min + rng.integers(0, 2**40, k)),  # wraps under a negative used
                 (8, full_i)]
        if extra:
            parts.append((10, lambda k: rng.integers(0, 9, k)))  # device counts
        return _mix(rng, n, parts, i64)

    def used_signed():
        return _mix(rng, n, [(70, lambda k: rng.integers(0, 2**38, k)), (10, zeros_i),
                             (10, lambda k: -rng.integers(1, 2**62, k)), (10, full_i)], i64)

    fc = _mix(rng, n, [(58, lambda k: rng.integers(0, 2**17, k).astype(u64)),
                       (10, lambda k: np.zeros(k, u64)), (10, lambda k: _near(rng, 2**31, k, u64)),
                       (10, lambda k: rng.integers(2**31, 2**40, k).astype(u64)), (12, full_u)], u64)
    uc = _mix(rng, n, [(85, lambda k: rng.integers(0, 2**16, k).astype(u64)),
                       (10, lambda k: np.zeros(k, u64)), (5, full_u)], u64)
    fm, um = free_signed(False), used_signed()
    fx = np.stack([free_signed(True) for _ in range(R)]) if R else np.zeros((0, n), i64)
    ux = np.stack([used_signed() for _ in range(R)]) if R else np.zeros((0, n), i64)
    ap = _mix(rng, n, [(45, lambda k: rng.integers(0, 256, k)), (15, lambda k: -rng.integers(0, 50, k)),
                       (40, lambda k: np.full(k, 2**62, i64))], i64)  # 2^62: no clamp
    pc = _mix(rng, n, [(70, lambda k: rng.integers(0, 300, k)), (15, zeros_i), (15, full_i)], i64)

    # specs, per 64-spec block in caller order
    top = lambda k: (2**52 - rng.integers(0, 3, k))  # noqa: E731
    fast_c = [(60, lambda k: rng.integers(1, 8001, k)), (15, lambda k: rng.integers(1, 4, k)),
              (15, top), (10, lambda k: rng.integers(2**23, 2**40, k))]
    fast_m = [(60, lambda k: rng.integers(2**20, 2**35, k)), (15, lambda k: rng.integers(1, 4, k)),
              (15, top), (10, lambda k: rng.integers(1, 2**18, k))]
    fast_x = [(25, zeros_i), (30, lambda k: rng.integers(1, 2**34, k)),
              (20, lambda k: rng.integers(1, 9, k)), (10, lambda k: rng.integers(1, 4, k)), (15, top)]
    mixed_c = [(45, lambda k: rng.integers(1, 8001, k).astype(u64)), (10, lambda k: np.zeros(k, u64)),
               (9, lambda k: np.full(k, 2**64 - 1, u64)),
               (9, lambda k: ~rng.integers(1, 2**40, k, dtype=u64)),  # other negatives, wrapped
               (9, lambda k: _near(rng, 2**52, k, u64, 2)), (18, full_u)]
    mixed_m = [(45, lambda k: rng.integers(2**20, 2**35, k)), (10, zeros_i),
               (9, lambda k: np.full(k, -1, i64)), (9, lambda k: -rng.integers(2, 2**45, k)),
               (9, lambda k: _near(rng, 2**52, k, i64, 2)), (18, full_i)]
    mixed_x = [(20, zeros_i), (35, lambda k: rng.integers(1, 2**34, k)),
               (9, lambda k: np.full(k, -1, i64)), (9, lambda k: -rng.integers(2, 2**45, k)),
               (9, lambda k: _near(rng, 2**52, k, i64, 2)), (18, full_i)]
    sc, sm, sx = np.zeros(S, u64), np.zeros(S, i64), np.zeros((R, S), i64)
    pools = []  # per all-fast block: the request pools [c, m, x_0 ..]
    for lo in range(0, S, 64):
        k = min(S, lo + 64) - lo
        if rng.random() < 0.5:
            pool = [_mix(rng, 4, fast_c, i64), _mix(rng, 4, fast_m, i64)]
            pool += [_mix(rng, 4, fast_x, i64) for _ in range(R)]
            pools.append(pool)
            sc[lo:lo + k] = pool[0][rng.integers(0, 4, k)].astype(u64)
            sm[lo:lo + k] = pool[1][rng.integers(0, 4, k)]
            for r in range(R):
                sx[r, lo:lo + k] = pool[2 + r][rng.integers(0, 4, k)]
        else:
            sc[lo:lo + k] = _mix(rng, k, mixed_c, u64)
            sm[lo:lo + k] = _mix(rng, k, mixed_m, i64)
            for r in range(R):
                sx[r, lo:lo + k] = _mix(rng, k, mixed_x, i64)

    # derived multiples: one free amount of the row becomes k d + {-1, 0, 1} below the fast bound
    if pools:
        for i in np.flatnonzero(rng.random(n) < derived):
            pool = pools[int(rng.integers(0, len(pools)))]
            col = int(rng.integers(0, 2 + R))
            if not (pool[col] > 0).any():
                col = 1  # (an extra resource the block does not request: the memory column)
            bound = xm.FC_MAX if col == 0 else xm.FX_MAX
            ds = pool[col][(pool[col] > 3) & (pool[col] < bound // 2)]  # where a multiple fits
            if ds.size == 0:
                ds = pool[col][pool[col] > 0]
            d = int(ds[int(rng.integers(0, ds.size))])
            kmax = (bound - 2) // d
            kq = min(kmax, int(2.0 ** rng.uniform(0, np.log2(kmax)))) if kmax >= 1 else 0
            f = max(kq * d + int(rng.choice([-1, 0, 0, 1])), 0)
            small = int(rng.integers(0, 2**16))  # an ordinary used amount: alloc does not wrap
            if col == 0:
                fc[i], uc[i] = f, small
            elif col == 1:
                fm[i], um[i] = f, small
            else:
                fx[col - 2, i], ux[col - 2, i] = f, small
    rows = [_wrap_add(uc, fc), _wrap_add(um, fm), ap, pc, uc, um]
    ax = _wrap_add(ux, fx) if R else np.zeros((0, n), i64)
    return dict(rows=rows, ax=ax, ux=ux, sc=sc, sm=sm, sx=sx)


def node_caps(seed, S):
    return np.random.default_rng([seed, S, 0xCA9]).choice(np.array(CAPS, i64), S)


def pair_model(case):
    return xm.pair_table(case["rows"], case["ax"], case["ux"], case["sc"], case["sm"], case["sx"])


# ---- shapes --------------------------------------------------------------------------------
# (largest first: hypothesis starts from, and keeps returning to, a strategy's first element)
SIZES_N = st.one_of(st.sampled_from([3100, 2049, 1025, 1024, 1023, 513, 512, 511, 257, 256, 255,
                                     65, 64, 63, 1]), st.integers(1, 3100))
SIZES_S = st.one_of(st.sampled_from([257, 256, 255, 129, 128, 127, 65, 64, 63, 1]),
                    st.integers(1, 257))
SIZES_G = st.sampled_from([9000, 4097, 4096, 2049, 1025, 1024, 1023, 256, 255, 7, 2, 1])
MAX_PAIRS = 20_000   # n x S: caps on the Python models' cost, not on the kernels
MAX_CELLS = 100_000  # G x S
FUZZ = dict(derandomize=True, deadline=None,
            suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])


# ---- the cell fits -------------------------------------------------------------------------
def _cell_example(seed, n, S, R, G, kind, entry, cap_on=True, want_min=True, want_rows=True):
    return example(seed=seed, n=n, S=S, R=R, G=G, kind=kind, entry=entry, cap_on=cap_on,
                   want_min=want_min, want_rows=want_rows)


# (the examples hypothesis always runs, whatever it draws besides: four sort workgroups and
# thirteen runs under more than GRP_LDS_GROUPS groups and under 1025 to 4096; every layout at
# n = 1025 through another entry point; the NULL group)
@pytest.mark.gpu
@settings(max_examples=120, **FUZZ)
@_cell_example(1, 3100, 6, 2, 9000, "uniform", "fit_ext")
@_cell_example(2, 3100, 6, 0, 4097, "zipf", "fit_grouped")
@_cell_example(3, 3100, 6, 4, 9000, "sorted", "fit_capped")
@_cell_example(4, 3100, 6, 1, 2049, "blocks256", "fit_capped")
@_cell_example(5, 2049, 9, 0, 4096, "invalid60", "fit_grouped")
@_cell_example(6, 2049, 9, 3, 1025, "one", "fit_ext")
@_cell_example(7, 1025, 19, 2, 1024, "blocks256", "fit_ext")
@_cell_example(8, 1025, 19, 0, 7, "zipf", "fit_capped", cap_on=False, want_min=False)
@_cell_example(9, 1025, 19, 2, 255, "all_invalid", "fit_capped")
@_cell_example(10, 513, 38, 4, 1, "none", "fit_capped", want_rows=False)
@_cell_example(11, 257, 77, 3, 1, "none", "fit_ext")
@_cell_example(12, 77, 257, 0, 1, "none", "fit_ext")
@given(seed=st.integers(0, 2**32 - 1), n=SIZES_N, S=SIZES_S, R=st.integers(0, 4), G=SIZES_G,
       kind=st.sampled_from(KINDS), entry=st.sampled_from(["fit_capped", "fit_ext", "fit_grouped"]),
       cap_on=st.booleans(), want_min=st.booleans(), want_rows=st.booleans())
def test_cell_fit_fuzz(engine, seed, n, S, R, G, kind, entry, cap_on, want_min, want_rows):
    S = max(1, min(S, MAX_PAIRS // n))
    if entry == "fit_grouped":
        R = 0
        kind = "one" if kind == "none" else kind  # (the grouped call takes no NULL group)
    G = 1 if kind == "none" else max(1, min(G, MAX_CELLS // S))
    msg = f"seed={seed} n={n} S={S} R={R} G={G} kind={kind} entry={entry}"
    case = make_cell_case(seed, n, S, R)
    rows, ax, ux, sc, sm, sx = (case[k] for k in ("rows", "ax", "ux", "sc", "sm", "sx"))
    gid = group_layout(seed, n, G, kind)
    q, dz = pair_model(case)
    cap = None
    if entry == "fit_grouped":
        got = dict(zip(("totals", "err"), engine.fit_grouped(*rows, gid, G, sc, sm)))
        want = dict(zip(("totals", "err"), xm.totals_from_pairs(q, dz, gid, G)))
    elif entry == "fit_ext":
        got = dict(zip(("totals", "err"), engine.fit_ext(*rows, ax, ux, sc, sm, sx, gid, G)))
        want = dict(zip(("totals", "err"), xm.totals_from_pairs(q, dz, gid, G)))
    else:
        cap = node_caps(seed, S) if cap_on else None
        msg += f" cap={'on' if cap_on else 'NULL'} want_min={want_min} want_rows={want_rows}"
        names = ("totals", "err", "cell_min", "group_rows")
        got = dict(zip(names, engine.fit_capped(*rows, ax, ux, sc, sm, sx, gid, G, cap,
                                                want_min=want_min, want_rows=want_rows)))
        want = dict(zip(names, sp.capped_cells(q, dz, gid, G, cap)))
        for name, on in (("cell_min", want_min), ("group_rows", want_rows)):
            if not on:
                assert got.pop(name) is None, msg
                want.pop(name)
    for name in ("err", "totals", "cell_min", "group_rows"):
        if name in want:
            assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, \
                f"{name}: {msg}"
            np.testing.assert_array_equal(got[name], want[name], err_msg=f"{name}: {msg}")
    if R == 0:  # a second, independent reference: the C oracle on each group's rows
        ot, oe = expected(rows, np.zeros(n, np.int32) if gid is None else gid, G, sc, sm)
        if gid is None:
            ot, oe = ot[0], oe[0]
        np.testing.assert_array_equal(got["err"], oe, err_msg=f"err (C oracle): {msg}")
        if cap is None:
            np.testing.assert_array_equal(got["totals"], ot, err_msg=f"totals (C oracle): {msg}")


# ---- the fold ------------------------------------------------------------------------------
def domain_layout(rng, G, D, kind):
    """domain_of int32 [G] (None for "none": each group its own domain, D = G)."""
    if kind == "none":
        return None
    if kind == "interleaved":
        return (np.arange(G) % D).astype(np.int32)
    dom = rng.integers(0, D, G)
    k = rng.choice(G, min(G, 6), replace=False)
    dom[k[:3]] = -1
    dom[k[3:]] = D + 2
    return (np.sort(dom) if kind == "sorted" else dom).astype(np.int32)


def made_up_cells(rng, G, S):
    """Cells no fit produced: small counts, some near MaxInt64 and MinInt64 (the saturating
    limit, the wrapping sums), a few flags, and group_rows with zeros."""
    t = rng.integers(-50, 2000, (G, S), dtype=i64)
    pick = rng.random((G, S))
    t[pick < 0.03] = I64.max - rng.integers(0, 5, int((pick < 0.03).sum()))
    t[pick > 0.98] = I64.min + rng.integers(0, 5, int((pick > 0.98).sum()))
    e = (rng.random((G, S)) < 0.002).astype(np.int32)
    return t, e, rng.integers(0, 4, G).astype(i64)


def _fold_example(seed, G, S, source, D, dom_kind, n=257, R=1, kind="uniform"):
    return example(seed=seed, G=G, S=S, source=source, n=n, R=R, kind=kind, D=D,
                   dom_kind=dom_kind, el_on=True, gr_on=True, skew_on=True)


# (always run: more groups than fold_cells has slices, with several specs, both sources)
@pytest.mark.gpu
@settings(max_examples=60, **FUZZ)
@_fold_example(1, 9000, 11, "made", 40, "many")
@_fold_example(2, 9000, 11, "capped", 3, "sorted", n=1025, R=2, kind="zipf")
@_fold_example(3, 4097, 24, "made", 4097, "none")
@_fold_example(4, 257, 256, "made", 3, "interleaved")
@_fold_example(5, 255, 257, "made", 40, "sorted")
@_fold_example(6, 1025, 19, "capped", 1025, "none", n=1025, R=0, kind="invalid60")
@given(seed=st.integers(0, 2**32 - 1),
       G=st.sampled_from([1, 2, 7, 255, 256, 257, 1024, 1025, 4097, 9000]),
       S=st.one_of(st.sampled_from([1, 2, 3, 11, 64, 65, 255, 256, 257]), st.integers(1, 300)),
       source=st.sampled_from(["made", "capped"]), n=st.sampled_from([65, 257, 1025]),
       R=st.integers(0, 2), kind=st.sampled_from(["uniform", "zipf", "invalid60"]),
       D=st.sampled_from([1, 3, 40, 9000]),
       dom_kind=st.sampled_from(["none", "many", "sorted", "interleaved"]),
       el_on=st.booleans(), gr_on=st.booleans(), skew_on=st.booleans())
def test_fold_fuzz(engine, seed, G, S, source, n, R, kind, D, dom_kind, el_on, gr_on, skew_on):
    S = max(1, min(S, MAX_CELLS // G))
    rng = np.random.default_rng([seed, G, S, 0xF01D])
    msg = f"seed={seed} G={G} S={S} source={source} dom={dom_kind} el={el_on} gr={gr_on} skew={skew_on}"
    if source == "capped":  # the cells of a fit_capped call, themselves checked
        S = max(1, min(S, MAX_PAIRS // n))
        msg += f" n={n} S={S} R={R} kind={kind}"
        case = make_cell_case(seed, n, S, R)
        gid = group_layout(seed, n, G, kind)
        cap = node_caps(seed, S)
        t, e, m, gr = engine.fit_capped(*case["rows"], case["ax"], case["ux"], case["sc"],
                                        case["sm"], case["sx"], gid, G, cap)
        q, dz = pair_model(case)
        for name, g, w in zip(("totals", "err", "cell_min", "group_rows"), (t, e, m, gr),
                              sp.capped_cells(q, dz, gid, G, cap)):
            np.testing.assert_array_equal(g, w, err_msg=f"{name}: {msg}")
    else:
        t, e, gr = made_up_cells(rng, G, S)
    D = G if dom_kind == "none" else min(D, G)
    msg += f" D={D}"
    dom = domain_layout(rng, G, D, dom_kind)
    el = None
    if el_on:  # about 70 % of the cells, two specs eligible nowhere
        el = rng.random((G, S)) < 0.7
        el[:, 3 % S] = False
        el[:, (S - 2) % S] = False
    sk = rng.choice(np.array(SKEWS, i64), S) if skew_on else None
    gr = gr if gr_on else None
    got = engine.spread_fold(t, e, gr, dom, D, el, sk)
    want = sp.fold(t, e, gr, dom, D, el, sk)
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"err: {msg}")
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"totals: {msg}")


# ---- what the inputs reach (no GPU) --------------------------------------------------------
COVER = [(11, 1, 257, 2), (12, 63, 129, 1), (13, 64, 64, 0), (14, 65, 65, 4), (15, 255, 63, 3),
         (16, 256, 65, 2), (17, 257, 64, 1), (18, 511, 33, 4), (19, 512, 31, 0), (20, 513, 32, 2),
         (21, 1023, 16, 3), (22, 1024, 17, 1), (23, 1025, 15, 2), (24, 2049, 8, 4), (25, 3100, 6, 2),
         (26, 100, 128, 2), (27, 70, 256, 1), (28, 129, 127, 3), (29, 300, 65, 0), (30, 40, 255, 4)]


def _frees(case):
    """Per row: free CPU, [free memory, free extras ..], fast (the model's row class)."""
    ac, am, _, _, uc, um = case["rows"]
    n = ac.size
    fcs = [xm.free_cpu(int(ac[i]), int(uc[i])) for i in range(n)]
    fxs = [[xm.free_signed(int(am[i]), int(um[i]))] +
           [xm.free_signed(int(a), int(u)) for a, u in zip(case["ax"][:, i], case["ux"][:, i])]
           for i in range(n)]
    fast = np.array([xm.row_is_fast(int(ac[i]), int(am[i]), int(uc[i]), int(um[i]),
                                    case["ax"][:, i], case["ux"][:, i]) for i in range(n)], bool)
    return fcs, fxs, fast


def _estimate_off(f, d):
    """Per pair [len(f), len(d)], the f64 estimate of the pair loop's fast path minus the
    quotient: trunc(float(f) * (1.0 / float(d))) - f // d (f < 2^50, 1 <= d <= 2^52).  -1:
    grp_div's `r >= d` step corrects it; +1: its `r < 0` step would (two roundings of 2^-53
    each lift f / d by less than f 2^-52 / d, which reaches the next integer, at least 1 / d
    away, only for f >= 2^52: beyond the fast rows' 2^50, and the counts below find none)."""
    f, d = np.asarray(f, i64)[:, None], np.asarray(d, i64)[None, :]
    est = np.trunc(f.astype(np.float64) * (1.0 / d.astype(np.float64)))
    return (est - (f // d).astype(np.float64)).astype(i64)


def test_cell_inputs_cover_the_branches():
    """Conditions on the generated inputs, counted from the models alone over a fixed list of
    cases: both row classes and both wave classes well populated, flagged and unflagged
    cells, enough fast pairs whose f64 estimate is off by one (grp_div's correction decides
    them), pairs decided by an extra resource, by the pod-slot clamp and by the per-node cap,
    and every id layout with its defining property."""
    n_rows = n_fast = waves = fast_waves = cells = flagged = off = below = above = 0
    by_extra = by_clamp = by_cap = 0
    for j, (seed, n, S, R) in enumerate(COVER):
        case = make_cell_case(seed, n, S, R)
        sc, sm, sx = case["sc"], case["sm"], case["sx"]
        fcs, fxs, fast = _frees(case)
        n_rows += n
        n_fast += int(fast.sum())
        sfast = np.array([xm.spec_is_fast(int(sc[s]), int(sm[s]), sx[:, s]) for s in range(S)])
        wfast = np.array([sfast[lo:lo + 64].all() for lo in range(0, S, 64)])  # lanes past S are fast
        waves += wfast.size
        fast_waves += int(wfast.sum())
        # fast pairs: a fast row under an all-fast wave
        in_fast_wave = np.repeat(wfast, 64)[:S]
        fr, fs = np.flatnonzero(fast), np.flatnonzero(in_fast_wave)
        if fr.size and fs.size:
            diffs = [_estimate_off([fcs[i] for i in fr], sc[fs].astype(i64)),
                     _estimate_off([fxs[i][0] for i in fr], sm[fs])]
            for r in range(R):
                req = sx[r, fs] != 0
                x = np.where(req, sx[r, fs], 1)
                diffs.append(_estimate_off([fxs[i][1 + r] for i in fr], x) * req[None, :])
            diffs = np.stack(diffs)
            assert (np.abs(diffs) <= 1).all()  # within 1: what grp_div's two steps rely on
            off += int((diffs != 0).any(axis=0).sum())
            below += int((diffs < 0).sum())
            above += int((diffs > 0).sum())
        # what decides q: an extra resource, the clamp, the cap
        q, dz = pair_model(case)
        no_x = dict(case, sx=np.zeros_like(sx))
        q0, dz0 = pair_model(no_x)
        by_extra += int(((q != q0) & ~dz & ~dz0).sum())
        rows = list(case["rows"])
        rows[2] = np.full(n, 2**62, i64)
        q1, _ = pair_model(dict(case, rows=rows))
        by_clamp += int(((q != q1) & ~dz).sum())
        cap = node_caps(seed, S)
        by_cap += int(((cap[None, :] > 0) & (q > cap[None, :]) & ~dz).sum())
        # flagged cells under the case's id layout (the kinds in rotation, 7 groups)
        kind = KINDS[j % len(KINDS)]
        G = 1 if kind == "none" else 7
        _, err = xm.totals_from_pairs(q, dz, group_layout(seed, n, G, kind), G)
        cells += err.size
        flagged += int((err != 0).sum())
    print(f"rows {n_rows} fast {n_fast} ({100.0 * n_fast / n_rows:.1f} %); waves {waves} all-fast "
          f"{fast_waves} ({100.0 * fast_waves / waves:.1f} %); cells {cells} flagged {flagged} "
          f"({100.0 * flagged / cells:.1f} %); fast pairs with the f64 estimate off by one {off} "
          f"(quotients below {below}, above {above}); "
          f"pairs decided by an extra resource {by_extra}, the clamp {by_clamp}, the cap {by_cap}")
    assert 0.30 * n_rows <= n_fast <= 0.85 * n_rows
    assert 0.25 * waves <= fast_waves <= 0.75 * waves
    assert 0.02 * cells <= flagged <= 0.50 * cells
    assert off >= 50
    assert by_extra >= 1 and by_clamp >= 1 and by_cap >= 1

    # the id layouts
    n, G = 1300, 7
    valid = lambda g: (g >= 0) & (g < G)  # noqa: E731
    g = group_layout(5, n, G, "uniform")
    assert 0 < (~valid(g)).sum() < 0.08 * n and np.unique(g[valid(g)]).size == G
    assert {-1, G, G + 5, -(2**31), 2**31 - 1} >= set(g[~valid(g)].tolist())
    g = group_layout(5, n, 2049, "zipf")
    top = np.bincount(g[(g >= 0) & (g < 2049)]).max()
    assert top > 0.6 * n and np.unique(g).size > 100  # one giant group beside near-singletons
    g = group_layout(5, n, G, "sorted")
    assert (np.diff(g) >= 0).all() and (~valid(g)).any() and np.unique(g[valid(g)]).size == G
    g = group_layout(5, n, 2049, "blocks256")
    starts = np.flatnonzero(np.diff(g)) + 1
    assert starts.size >= 2 and (starts % RUN == 0).all() and ((g >= 0) & (g < 2049)).all()
    assert (np.diff(g) >= 0).all()
    g = group_layout(5, n, G, "one")
    assert (g == G // 2).all()
    g = group_layout(5, n, G, "invalid60")
    assert 0.5 * n < (~valid(g)).sum() < 0.7 * n
    g = group_layout(5, n, G, "invalid40")
    assert 0.3 * n < (~valid(g)).sum() < 0.5 * n
    g = group_layout(5, n, G, "all_invalid")
    assert not valid(g).any()
    assert group_layout(5, n, 1, "none") is None
    for kind in KINDS:  # n below one run, and more groups than rows
        g = group_layout(5, 40, 9000, kind)
        assert kind == "none" or (g.shape == (40,) and g.dtype == np.int32)
