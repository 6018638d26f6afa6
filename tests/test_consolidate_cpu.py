"""The removal what-if without a GPU: the constants and the binding, tests/consolidate_model.py
on the README's worked example and on hand cases, consolidate_np against it, and the conditions
tests/test_consolidate.py's generators promise."""
import os
import re

import numpy as np
import pytest

from kubernetesclustercapacity_amd import _lib
from tests import consolidate_model as cm
from tests import test_consolidate as tc
from tests.test_drain_cpu import worked_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64, u64 = np.int64, np.uint64
GiB = 1 << 30
CHUNK = _lib.KCC_CONS_CHUNK


def test_constants_and_binding():
    assert _lib.KCC_CONS_MAX_PODS == cm.MAX_PODS == 1024
    assert (_lib.KCC_CAND_OK, _lib.KCC_CAND_BADROW, _lib.KCC_CAND_TOOMANY) == (0, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "kcc.h")).read()
    assert re.search(r"#define KCC_CONS_MAX_PODS 1024\b", hdr)
    assert re.search(r"KCC_CAND_OK = 0, KCC_CAND_BADROW = 1, KCC_CAND_TOOMANY = 2", hdr)
    internal = open(os.path.join(ROOT, "kubernetesclustercapacity_amd", "csrc", "kcc_internal.h")).read()
    m = re.search(r"CONS_THREADS = (\d+);.*?CONS_IPT = (\d+);", internal, re.S)
    assert int(m.group(1)) * int(m.group(2)) == CHUNK
    assert re.search(r"CONS_MAX_PODS = 1024;", internal)
    arity = _lib.header_arities()
    for name, n_args in (("kcc_consolidate", 25), ("kcc_consolidate_async", 26)):
        assert name in _lib.SIGNATURES and name in _lib.header_symbols()
        assert len(_lib.SIGNATURES[name][1]) == arity[name] == n_args
    mk = open(os.path.join(ROOT, "kubernetesclustercapacity_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bkcc_consolidate\.hip\b", mk, re.M)
    # the step arithmetic has one copy: the deploy row pass and the walk both call it
    src = os.path.join(ROOT, "kubernetesclustercapacity_amd", "csrc")
    for f in ("kcc_deploy.hip", "kcc_consolidate.hip"):
        text = open(os.path.join(src, f)).read()
        assert "deploy_row_q<R>(" in text and "CC:134-136, after all the mins" not in text, f


def readme_case(fourth=False):
    """The -drain example's cluster; fourth: a pod of 2500m / 1 GiB on C."""
    rows, ptr, pc, pm, mv = worked_example()
    if fourth:
        rows[3] = np.array([3, 1, 1], i64)
        rows[4] = np.array([2100, 2000, 2500], u64)
        rows[5] = rows[5] + np.array([0, 0, GiB], i64)
        ptr = np.array([0, 3, 4, 5], i64)
        pc, pm, mv = np.append(pc, u64(2500)), np.append(pm, i64(GiB)), np.append(mv, np.uint8(1))
    e = np.zeros((0, 3), i64)
    return dict(rows=rows, ax=e, ux=e, ptr=ptr, pc=pc, pm=pm, px=np.zeros((0, pc.size), i64), mv=mv,
                target=None, cand=np.arange(3))


def test_readme_example():
    res = tc.model_of(readme_case())
    assert res.evicted.tolist() == [2, 1, 0] and res.placed.tolist() == [2, 1, 0]
    assert res.zero.tolist() == [0, 0, 0] and res.err.tolist() == [0, 0, 0]
    assert res.pod_target.tolist() == [1, 1, -2, 2]  # A's pods on B, the daemon pod stays, B's on C
    assert res.removable.tolist() == [True, True, True]
    res = tc.model_of(readme_case(fourth=True))
    assert res.evicted.tolist() == [2, 1, 1] and res.placed.tolist() == [2, 0, 0]
    assert res.pod_target.tolist() == [1, 1, -2, -1, -1]
    assert res.removable.tolist() == res.removable_lenient.tolist() == [True, False, False]
    # the README's lines are these numbers
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name, e, p in (("A", 2, 2), ("B", 1, 1), ("C", 0, 0)):
        assert f"Node {name} : {e} pods evicted, {p} placed, 0 not placed, 0 without requests" in readme
    assert "Removable one at a time : 3 of 3 nodes (3 counting pods without requests as placed)" in readme
    assert "Node B : 1 pods evicted, 0 placed, 1 not placed, 0 without requests" in readme
    assert "Removable one at a time : 1 of 3 nodes (1 counting pods without requests as placed)" in readme


def test_hand_cases():
    # the clamp quirk: 3 slots by the clamp, but the clamp stops firing below q = 10
    res = tc.model_of(tc.clamp_case())
    assert res.pod_target.tolist() == [1] * 11 + [2] and res.removable.tolist() == [True]
    # runs of equal shapes, placed and not placed; a pod without requests is not tried
    res = tc.model_of(tc.runs_case())
    assert res.pod_target.tolist() == [1, 1, 2, 3, 3, -3, 3, -1, -1, 4, -1, 4, 5, -1, -1, 5, 5]
    assert (res.evicted[0], res.placed[0], res.zero[0]) == (17, 11, 1)
    assert not res.removable[0] and not res.removable_lenient[0]
    # masks: unmovable and zero-request pods, rows 0 .. 2 no targets, no pod on its own row
    case = tc.misc_case()
    res = tc.model_of(case)
    assert res.evicted.tolist() == [3, 5, 3, 0] and res.zero.tolist() == [1, 1, 0, 0]
    assert res.placed.tolist() == [2, 4, 3, 0] and res.removable.tolist() == [False, False, True, True]
    assert res.removable_lenient.all()
    assert res.pod_target.tolist() == [3, -3, -2, 3, 3, -2, 3, -3, 3, 3, 3, 3, 3]
    owner = np.repeat(np.arange(10), np.diff(case["ptr"]))
    placed = res.pod_target >= 0
    assert (res.pod_target[placed] != owner[placed]).all() and (res.pod_target[placed] >= 3).all()
    # candidate 4's pods skip row 4 itself once row 3 is full
    case = dict(case, cand=np.array([4], i64), mv=None)
    assert tc.model_of(case).pod_target[4:10].tolist() == [3, 3, 3, -3, 3, 5]
    # duplicates and rows out of range
    res = tc.model_of(dict(tc.misc_case(), cand=np.array([4, 4, -1, 10], i64)))
    assert res.err.tolist() == [0, 0, 1, 1] and res.placed.tolist() == [4, 4, 0, 0]
    # one pod too many: not evaluated, its pods keep -2
    res = tc.model_of(tc.count_case(cm.MAX_PODS + 1), cm.consolidate_np)
    assert res.err.tolist() == [2, 0] and res.evicted.tolist() == [cm.MAX_PODS + 1, 2]
    assert (res.pod_target[:-2] == -2).all()


@pytest.mark.parametrize("name", [k for k in tc.HAND if k not in ("toomany", "clamp")])
def test_consolidate_np_equals_consolidate(name):
    case = tc.HAND[name]()
    tc.compare(tc.model_of(case, cm.consolidate_np), tc.model_of(case), name)


@pytest.mark.parametrize("R", [0, 2])
def test_np_model_on_the_size_generator(R):
    case = tc.size_case(65, R)
    tc.compare(tc.model_of(case, cm.consolidate_np), tc.model_of(case), f"R={R}")


@pytest.mark.parametrize("R", tc.RS)
@pytest.mark.parametrize("n", [s for s in tc.SIZES if s >= 63])
def test_generator_conditions(n, R):
    """What test_consolidate.test_sizes relies on: some candidates are removable and some are
    not, some candidate puts two pods on one row (the overlay matters) and some spreads over two
    rows — a kernel cannot pass by placing nothing, everything, or everything on one row."""
    case = tc.size_case(n, R)
    res = tc.model_of(case, cm.consolidate_np)
    assert res.removable.any() and not res.removable.all() and (res.err == 0).all()
    assert 0 < int(case["mv"].sum()) < case["mv"].size
    two_on_one = two_rows = False
    for c in case["cand"]:
        t = res.pod_target[case["ptr"][c]:case["ptr"][c + 1]]
        t = t[t >= 0]
        two_on_one |= t.size > np.unique(t).size
        two_rows |= np.unique(t).size >= 2
    assert two_on_one and two_rows


def test_last_chunk_and_stress_generators():
    # some pod's hit lies in the last chunk, and the candidate is the first or the last row
    combos = tc.only_row_combos()
    assert {n for n, _, _ in combos} == set(tc.SIZES) - {1}
    big = 3 * CHUNK + 17
    assert (big, 0, big - 1) in combos and (big, big - 1, big - 2) in combos
    assert (CHUNK + 1, 0, CHUNK) in combos and (CHUNK, CHUNK - 1, 0) in combos
    for n, c, f in ((big, 0, big - 1), (CHUNK + 1, CHUNK, 0), (2, 1, 0), (65, 0, 1)):
        res = tc.model_of(tc.only_row_case(n, c, f), cm.consolidate_np)
        assert res.pod_target.tolist() == [f] * 5 + [-1] and res.placed.tolist() == [5]
    # KCC_CONS_MAX_PODS pods on as many rows; on eleven rows
    for per_row, alternate in ((1, False), (1, True), (100, True)):
        res = tc.model_of(tc.overlay_case(per_row, alternate), cm.consolidate_np)
        assert res.placed.tolist() == [cm.MAX_PODS]
        assert np.unique(res.pod_target).size == (cm.MAX_PODS if per_row == 1 else 11)
    for k in (0, 1, 64, 65, cm.MAX_PODS):
        res = tc.model_of(tc.count_case(k), cm.consolidate_np)
        assert res.evicted.tolist() == [k, 2] and res.removable.all()


def test_fuzz_generator_covers_the_branches():
    """The property test's inputs reach zero requests, unplaced pods, placed pods, rows out of
    range and both the masked and the unmasked form."""
    seen = dict(zero=0, unplaced=0, placed=0, bad=0, masked=0, unmasked=0, cpu_high=0, negative=0)
    for seed in range(40):
        case = tc.fuzz_case(seed, 17, 20, seed % 5, 3)
        res = tc.model_of(case)
        seen["zero"] += int(res.zero.sum())
        seen["placed"] += int(res.placed.sum())
        seen["unplaced"] += int((res.pod_target == -1).sum())
        seen["bad"] += int((res.err == cm.BADROW).sum())
        seen["masked" if case["target"] is not None else "unmasked"] += 1
        seen["cpu_high"] += int((case["pc"] >= u64(1 << 63)).sum())
        seen["negative"] += int((case["pm"] < 0).sum())
    assert all(v > 0 for v in seen.values()), seen
