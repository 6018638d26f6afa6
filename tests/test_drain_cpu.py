"""The drain what-if without a GPU: tests/drain_model.py on the worked example and on hand
cases, drain_np against it, the conditions tests/test_drain.py's generators promise, and the
claim that the drained state alone carries the drain into the fits."""
import os
import re

import numpy as np
import pytest

from kubernetesclustercapacity_amd import _lib
from tests import drain_model as drm
from tests import ext_model as xm
from tests import test_drain as td

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64, u64 = np.int64, np.uint64
GiB, MiB = 1 << 30, 1 << 20
PACK, SPREAD = drm.PACK, drm.SPREAD


def worked_example():
    """Three nodes A, B, C of 4 cores / 16 GiB / 110 pods.  A runs two pods of 1 core / 1 GiB
    and a daemon pod of 100m / 100 MiB, B one pod of 2 cores / 2 GiB, C nothing."""
    rows = [np.full(3, 4000, u64), np.full(3, 16 * GiB, i64), np.full(3, 110, i64),
            np.array([3, 1, 0], i64), np.array([2100, 2000, 0], u64),
            np.array([2 * GiB + 100 * MiB, 2 * GiB, 0], i64)]
    ptr = np.array([0, 3, 4, 4], i64)
    pc = np.array([1000, 1000, 100, 2000], u64)
    pm = np.array([GiB, GiB, 100 * MiB, 2 * GiB], i64)
    mv = np.array([1, 1, 0, 1], np.uint8)
    return rows, ptr, pc, pm, mv


def fit_total(rows, res, c, m):
    q, dz = xm.pair_table([rows[0], rows[1], rows[2], res.pod_count, res.used_cpu, res.used_mem],
                          res.used_x, res.used_x, [c], [m], np.zeros((0, 1), i64))
    assert not dz.any()
    return q[:, 0]


def test_constants_and_binding():
    assert _lib.KCC_DRAIN_MAX_SHAPES == 4096 and _lib.KCC_DRAIN_SUMMARY == 4
    hdr = open(os.path.join(ROOT, "include", "kcc.h")).read()
    assert re.search(r"#define KCC_DRAIN_MAX_SHAPES 4096\b", hdr)
    assert re.search(r"#define KCC_DRAIN_SUMMARY 4\b", hdr)
    assert "kcc_drain" in _lib.SIGNATURES and "kcc_drain_async" in _lib.SIGNATURES
    mk = open(os.path.join(ROOT, "kubernetesclustercapacity_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bkcc_drain\.hip\b", mk, re.M)


@pytest.mark.parametrize("policy,per_node", [(SPREAD, [0, 1, 1]), (PACK, [0, 2, 0])])
def test_worked_example(policy, per_node):
    rows, ptr, pc, pm, mv = worked_example()
    e = np.zeros((0, 3), i64)
    before = xm.pair_table(rows, e, e, [1000], [GiB], np.zeros((0, 1), i64))[0][:, 0]
    assert before.tolist() == [1, 2, 4]  # 7 as things stand
    res = drm.drain(rows, e, e, [1, 0, 0], ptr, pc, pm, None, mv, policy)
    assert res.summary.tolist() == [1, 2, 1, 2]
    assert res.shape_cpu.tolist() == [1000] and res.shape_mem.tolist() == [GiB]
    assert res.shape_count.tolist() == [2] and res.shape_placed.tolist() == [2]
    assert res.shape_nodes.tolist() == [sum(1 for v in per_node if v)]
    assert (res.pod_count - np.array([110, 1, 0])).tolist() == [0] + per_node[1:]
    assert res.used_cpu[0] == 4000 and res.used_mem[0] == 16 * GiB and res.pod_count[0] == 110
    after = fit_total(rows, res, 1000, GiB)
    assert after[0] == 0 and after.sum() == 4  # 4 either way


def test_hand_cases():
    # shapes are sorted descending with cpu unsigned and the other words signed; equal pods merge
    case, D = td.key_case()
    res = td.model_of(case, SPREAD, D)
    keys = list(zip(res.shape_cpu.tolist(), res.shape_mem.tolist(), *res.shape_x.tolist()))
    assert len(set(keys)) == D == res.shapes and keys == sorted(keys, reverse=True)
    assert keys[0][0] == (1 << 64) - 1 and keys[-1] == (0, 3, 0, 0)
    assert keys.index((1 << 63, 1, 0, 0)) < keys.index(((1 << 63) - 1, 1, 0, 0))
    assert keys.index((7, 5, 1, 2)) < keys.index((7, 5, 1, 1)) < keys.index((7, 5, 1, -2))
    assert res.shape_count.sum() == res.evicted == case["pc"].size and res.placed == 0
    # one more shape than max_shapes: nothing placed, the drained rows still full
    over = td.model_of(case, SPREAD, D - 1)
    assert over.summary.tolist() == [4, case["pc"].size, -1, 0] and over.shape_cpu.size == 0
    np.testing.assert_array_equal(over.used_cpu, case["rows"][0])
    np.testing.assert_array_equal(over.pod_count, case["rows"][2])
    np.testing.assert_array_equal(over.used_x, case["ax"])
    # a flagged shape places nothing; the later shapes are placed
    res = td.model_of(td.flagged_case(), PACK)
    assert res.shape_err.tolist() == [1, 0, 0, 1] and res.shape_placed.tolist() == [0, 2, 1, 0]
    assert res.pod_count.tolist() == [1 << 30, 3, 0, 0, 0]
    # an unmovable pod goes away with its node; no pods at all
    for name, case in td.degenerate_cases().items():
        res = td.model_of(case, SPREAD)
        assert res.drained_rows == int(case["drain"].sum())
        if name in ("empty_rows", "unmovable", "no_pods"):
            assert res.drained_rows > 0 and (res.evicted, res.shapes, res.placed) == (0, 0, 0)
    res = td.model_of(td.skew_case(), SPREAD)
    assert res.shapes == 7 and 3500 < res.evicted < 4500


@pytest.mark.parametrize("policy", [PACK, SPREAD])
@pytest.mark.parametrize("R", [0, 2])
@pytest.mark.parametrize("n,frac", [(1, 0.9), (65, 0.3), (65, 0.9), (300, 0.5)])
def test_drain_np_equals_drain(n, R, policy, frac):
    case = td.drain_case(n + 1, n, R, frac)
    a, b = td.model_of(case, policy), td.model_of(case, policy, model=drm.drain_np)
    td.compare(b, a, f"n={n} R={R} policy={policy} frac={frac}")


@pytest.mark.parametrize("policy", [PACK, SPREAD])
@pytest.mark.parametrize("R", [0, 2])
@pytest.mark.parametrize("n", [s for s in td.SIZES if s >= 63] + [65, 1025])
def test_generator_conditions(n, R, policy):
    """What test_drain.test_sizes relies on: with a drained fraction of 0.3 the model places
    every evicted pod, with 0.9 it leaves pods unplaced — a test cannot pass by placing
    nothing, nor by placing everything."""
    for frac, movable in td.MIXES:
        case = td.drain_case(n, n, R, frac, movable=movable)
        res = td.model_of(case, policy, model=drm.drain_np)
        assert res.evicted > 0 and 1 <= res.shapes <= 7
        assert 0 < int(case["drain"].sum()) < n
        if movable:
            assert 0 < int(case["mv"].sum()) < case["mv"].size
        if frac == 0.3:
            assert res.placed == res.evicted, (n, R, policy, frac, res.placed, res.evicted)
        else:
            assert 0 < res.placed < res.evicted, (n, R, policy, frac, res.placed, res.evicted)


def test_table_generators():
    for D in (1, 2, 3, 7):
        case = td.drain_case(40 + D, 65, 2, 0.5, n_palette=D, cover=True)
        res = td.model_of(case, SPREAD, D)
        assert res.shapes == D and res.placed > 0
    case = td.drain_case(5, 65, 1, 0.5, n_palette=1000, per_row=100, cover=True)
    _, evicted, shapes = drm.evicted_shapes(case["drain"], case["ptr"], case["pc"], case["pm"],
                                            case["px"], case["mv"], 1)
    assert len(shapes) == 1000 and evicted >= 1000
    for name, (kw, M) in td.ASYNC_CASES.items():
        res = td.model_of(td.drain_case(**kw), SPREAD, M)
        assert res.shapes == {"padding": 7, "exact": 7, "overflow": -1, "none_drained": 0}[name]


@pytest.mark.parametrize("R", [0, 2])
def test_drained_rows_fit_nothing_and_raise_no_flag(R):
    """On the model's output state every drained row gives 0 and no flag for every spec — a
    zero-request spec too: the state alone carries the drain into the fits."""
    case = td.drain_case(77, 200, R, 0.4)
    res = td.model_of(case, SPREAD, model=drm.drain_np)
    rows = case["rows"]
    sc = np.array([0, 1, 250, 0, 1 << 40], u64)
    sm = np.array([0, 1, 1 << 28, 1 << 20, 0], i64)
    sx = np.array([[0, 1, 2, 0, 0]] * R, i64).reshape(R, 5)
    q, dz = xm.pair_table([rows[0], rows[1], rows[2], res.pod_count, res.used_cpu, res.used_mem],
                          case["ax"], res.used_x, sc, sm, sx)
    d = case["drain"] != 0
    assert d.sum() > 20 and not q[d].any() and not dz[d].any()
    assert dz[~d].any() and q[~d].any()  # (the other rows do hold pods, and do flag)
