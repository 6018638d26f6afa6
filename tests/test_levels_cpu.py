"""tests/levels_model.py against the oracle, and the generators of tests/test_levels.py against
what they are meant to reach (no GPU).

The hand example — 2 nodes, 3 priority classes (levels 0, 1, 2), the spec 1000m / 1 GiB, where
preemption changes which term binds:

    node X: 4000m, 8 GiB, 10 pod slots         node Y: 8000m, 4 GiB, 3 pod slots
      pod level 0: 3000m, 1 GiB                  pod level 0: 1000m, 1 GiB
      pod level 1:  500m, 5 GiB                  pod level 1: 1000m, 2 GiB
      pod level 2:  500m, 1 GiB                  (no pod of level 2)

    plane 0 (every pod):   X used 4000m 7 GiB 3 pods   Y used 2000m 3 GiB 2 pods
    plane 1 (level >= 1):  X used 1000m 6 GiB 2 pods   Y used 1000m 2 GiB 1 pod
    plane 2 (level >= 2):  X used  500m 1 GiB 1 pod    Y used    0m 0 GiB 0 pods

    level 0:  X min(0, 1) = 0: CPU binds           Y min(6, 1) = 1: memory binds       total 1
    level 1:  X min(3, 2) = 2: memory binds now    Y min(7, 2) = 2: memory             total 4
    level 2:  X min(3, 7) = 3: CPU again           Y min(8, 4) = 4 >= 3 slots: the
                                                     clamp, 3 - 0 pods = 3             total 6
"""
import numpy as np

from oracle import pyoracle
from tests import levels_model as lm
from tests import test_levels as tl

GIB = 1 << 30


def hand_example():
    npp = np.array([0, 3, 5])
    pp = np.arange(6)
    cpu = np.array([3000, 500, 500, 1000, 1000], np.uint64)
    mem = np.array([1, 5, 1, 1, 2], np.int64) * GIB
    lvl = np.array([0, 1, 2, 0, 1], np.uint8)
    alloc3 = [np.array([4000, 8000], np.uint64), np.array([8, 4], np.int64) * GIB,
              np.array([10, 3], np.int64)]
    return (npp, pp, cpu, mem, lvl), alloc3


def test_hand_example():
    pods, alloc3 = hand_example()
    uc, um, pc = lm.reduce_levels(*pods, 3)
    assert uc.tolist() == [[4000, 2000], [1000, 1000], [500, 0]]
    assert (um // GIB).tolist() == [[7, 3], [6, 2], [1, 0]]
    assert pc.tolist() == [[3, 2], [2, 1], [1, 0]]
    sc, sm = np.full(3, 1000, np.uint64), np.full(3, GIB, np.int64)
    t, e = lm.fit_levels(alloc3, pc, uc, um, np.zeros((0, 2), np.int64), np.zeros((3, 0, 2), np.int64),
                         sc, sm, np.zeros((0, 3), np.int64), [0, 1, 2, 3])
    assert t.tolist() == [[1, 4, 6]] and not e.any()
    # the binding terms the docstring names
    rows = lambda l: [int(a[0]) for a in alloc3] + [int(pc[l][0]), int(uc[l][0]), int(um[l][0])]  # noqa: E731
    assert [pyoracle.fit_one(*rows(l), 1000, GIB) for l in range(3)] == [0, 2, 3]


def drop_below(pods, l, L):
    """The flattened node CSR of the containers of the pods with min(level, L - 1) >= l."""
    npp, pp, cpu, mem, lvl = pods
    keep_pod = np.minimum(lvl.astype(np.int64), L - 1) >= l
    keep_c = np.repeat(keep_pod, np.diff(pp))
    node_of_c = np.repeat(np.repeat(np.arange(npp.size - 1), np.diff(npp)), np.diff(pp))
    counts = np.bincount(node_of_c[keep_c], minlength=npp.size - 1)
    ptr = np.concatenate([[0], np.cumsum(counts)])
    return ptr.tolist(), cpu[keep_c].tolist(), mem[keep_c].tolist(), keep_pod


def test_model_planes_are_the_oracle_reduce_without_the_lower_pods():
    for N, L in ((65, 1), (65, 2), (257, 8), (1, 8)):
        pods, (uc, um, pc) = tl.red_case(N, L)
        for l in range(L):
            ptr, c, m, keep = drop_below(pods, l, L)
            want = pyoracle.reduce_requests(ptr, c, m)
            assert [w[0] for w in want] == uc[l].tolist(), (N, L, l)
            assert [w[1] for w in want] == um[l].tolist(), (N, L, l)
            node_of_pod = np.repeat(np.arange(N), np.diff(pods[0]))
            assert np.bincount(node_of_pod[keep], minlength=N).tolist() == pc[l].tolist()
        assert pc[0].tolist() == np.diff(pods[0]).tolist()


def test_model_fit_columns_are_the_oracle_fit_per_plane():
    pods, alloc3 = tl.sane_pipeline(N=40, L=4)
    uc, um, pc = lm.reduce_levels(*pods, 4)
    sc = np.array([250, 0, 1000, 4000, 100, 500, 2000], np.uint64)
    sm = np.array([GIB, GIB, 0, 8 * GIB, 64 << 20, -1, GIB], np.int64)
    lp = [0, 3, 3, 5, 7]
    N = 40
    t, e = lm.fit_levels(alloc3, pc, uc, um, np.zeros((0, N), np.int64), np.zeros((4, 0, N), np.int64),
                         sc, sm, np.zeros((0, 7), np.int64), lp)
    for l in range(4):
        lo, hi = lp[l], lp[l + 1]
        wt, we = pyoracle.fit(*alloc3, pc[l], uc[l], um[l], sc[lo:hi], sm[lo:hi])
        assert t[0, lo:hi].tolist() == wt and e[0, lo:hi].tolist() == we
    assert e.any() and not e.all()


def test_generators_reach_what_they_are_meant_to():
    for N, long_at in tl.RED_BIG:
        (npp, pp, cpu, mem, lvl), (uc, um, pc) = tl.red_case(N, 8, long_at)
        P = int(npp[-1])
        per, cont = np.diff(npp), np.diff(pp)
        assert set(np.minimum(lvl, 7).tolist()) == set(range(8)) and (lvl >= 8).any()
        assert (per == 0).any() and (cont == 0).any() and cont.max() == 3
        assert per[long_at] == tl.LONG
        first, last = int(npp[long_at]), int(npp[long_at + 1]) - 1
        tiles = -(-P // tl.TILE)
        k = min(8, max(1, tiles // tl.MIN_GRID))  # tiles a workgroup (launch_levels_reduce)
        assert first % tl.TILE != 0 and last // tl.TILE - first // tl.TILE > 200  # cut by tiles
        assert last // (k * tl.TILE) - first // (k * tl.TILE) >= 30               # and workgroups
        assert (cpu > np.uint64(1 << 63)).any() and (mem < 0).any()
        assert (um[0] < 0).any() or (uc[0] < np.uint64(1 << 40)).any()  # sums that wrapped
    assert [min(8, max(1, -(-int(tl.red_case(N, 8, la)[0][0][-1]) // tl.TILE) // tl.MIN_GRID))
            for N, la in tl.RED_BIG] == [1, 4, 8]
    # every pod level appears at the small sizes too, and levels past L
    for L in tl.RED_L:
        lvl = tl.red_case(257, L)[0][4]
        assert set(np.minimum(lvl, L - 1).tolist()) == set(range(L)) and (lvl >= L).any()
    # the fit cases: every S_l of the issue, the exact-path rows and the zero requests
    c = tl.fit_case(2, 3, True)
    assert sorted(set(np.diff(c["lp"]).tolist())) == [0, 1, 64, 65, 257]
    free_cpu = c["alloc3"][0].astype(object) - c["uc"].astype(object)
    assert (free_cpu[0] >= 1 << 31).any()
    assert (free_cpu[tl.FULL_LEVEL] <= 0).all() and (free_cpu[0] > 0).any()
    for l in (0, tl.FULL_LEVEL):
        assert c["sc"][c["lp"][l] + 1] == 0 and c["sm"][c["lp"][l] + 2] == 0
    assert ((c["gid"] < 0) | (c["gid"] >= 3)).any()
    e = c["model"][1]
    assert e[:, c["lp"][0] + 1].any() and not e[:, c["lp"][tl.FULL_LEVEL] + 1].any()
