"""The fit explained (kcc_fit_explain), the checks that need no GPU:

  - the header declares both entry points and the KCC_WHY_* slots, _lib binds them with their
    arity, and KCC_ABI_VERSION is still 2;
  - tests/explain_model.py on the README's three-node example, by hand;
  - the model's q and totals are tests/ext_model.pair_table's and
    tests/spread_model.capped_cells'; `left` summed row by row is sum(free) - request x total
    modulo 2^64; explain_groups against the model;
  - the inputs tests/test_explain.py generates reach every slot 0-7 on fast pairs and on exact
    pairs alike, and hit each tie;
  - kcc_explain.hip compiles for gfx950, no kernel with a private segment or more than 64 KiB
    of LDS;
  - the CLI refuses -explain with -spreadBy zone before it opens anything.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from kubernetesclustercapacity_amd import _lib
from kubernetesclustercapacity_amd.engine import ExplainResult, explain_groups
from tests import explain_model as em
from tests import ext_model as xm
from tests import spread_model as sp
from tests import test_explain as te
from tests.test_host import _run, cli  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "kubernetesclustercapacity_amd", "csrc", "kcc_explain.hip")
GIB = 1 << 30


# ---- ABI ---------------------------------------------------------------------------------
def test_header_and_signatures():
    ar = _lib.header_arities()
    for name, k in {"kcc_fit_explain": 23, "kcc_fit_explain_async": 24}.items():
        assert name in _lib.header_symbols()
        assert ar.get(name) == k
        assert len(_lib.SIGNATURES[name][1]) == k
    # kcc_fit_capped's inputs in its order (its first 17 arguments), then node_cap
    assert _lib.SIGNATURES["kcc_fit_explain"][1][:17] == _lib.SIGNATURES["kcc_fit_capped"][1][:17]
    text = open(_lib.HEADER_PATH).read()
    want = {"KCC_WHY_SLOTS": 8, "KCC_WHY_CPU": 0, "KCC_WHY_MEM": 1, "KCC_WHY_EXT0": 2,
            "KCC_WHY_PODS": 6, "KCC_WHY_CAP": 7}
    for name, v in want.items():
        assert re.search(rf"#define\s+{name}\s+{v}\b", text), name
        assert getattr(_lib, name) == v
    assert (em.SLOTS, em.CPU, em.MEM, em.EXT0, em.PODS, em.CAP) == (8, 0, 1, 2, 6, 7)
    assert _lib.KCC_WHY_EXT0 + _lib.KCC_EXT_MAX <= _lib.KCC_WHY_PODS
    assert re.search(r"#define\s+KCC_ABI_VERSION\s+2\b", text)  # adding symbols: unchanged
    mk = open(os.path.join(os.path.dirname(SRC), "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bkcc_explain\.hip\b", mk, re.M)


# ---- the README example, by hand -----------------------------------------------------------
def example(cap=None):
    # node A: 4000m / 2Gi free; B: 1000m / 16Gi; C: 8000m / 64Gi, 10 pod slots, 7 running
    rows = [[4000, 1000, 8000], [2 * GIB, 16 * GIB, 64 * GIB], [110, 110, 10], [0, 0, 7],
            [0, 0, 0], [0, 0, 0]]
    tab = em.explain_table(rows, [], [], [500], [GIB], [], cap)
    return tab, em.explain_cells(tab, [500], [GIB], [])


def test_the_readme_example():
    tab, (t, e, wr, wp, left) = example()
    assert tab["q"][:, 0].tolist() == [2, 2, 3] and tab["b"][:, 0].tolist() == [em.MEM, em.CPU, em.PODS]
    assert t.tolist() == [[7]] and e.tolist() == [[0]]
    assert wr[:, 0, 0].tolist() == [1, 1, 0, 0, 0, 0, 1, 0]
    assert wp[:, 0, 0].tolist() == [2, 2, 0, 0, 0, 0, 3, 0]
    assert left[:, 0, 0].tolist() == [9500, 80530636800]
    tab, (t, e, wr, wp, left) = example([2])
    assert tab["b"][:, 0].tolist() == [em.MEM, em.CPU, em.CAP]  # q == node_cap on A and B: no cap
    assert t.tolist() == [[6]] and wp[:, 0, 0].tolist() == [2, 2, 0, 0, 0, 0, 0, 2]
    assert left[:, 0, 0].tolist() == [10000, 76 * GIB]


def test_tie_rules_by_hand():
    one = lambda *a: em.explain_one(*a)[:2]  # noqa: E731
    assert one(1000, 2 * GIB, [], 110, 0, 500, GIB, [], 0) == (2, em.CPU)       # qc == qm: CPU
    assert one(1000, 2 * GIB, [2], 110, 0, 500, GIB, [1], 0) == (2, em.CPU)     # q == qx: the earlier
    assert one(1500, 2 * GIB, [2], 110, 0, 500, GIB, [1], 0) == (2, em.MEM)
    assert one(1500, 3 * GIB, [2], 110, 0, 500, GIB, [1], 0) == (2, em.EXT0)
    assert one(1500, 3 * GIB, [2, 1], 110, 0, 500, GIB, [0, 1], 0) == (1, em.EXT0 + 1)
    assert one(1500, 3 * GIB, [], 3, 1, 500, GIB, [], 0) == (2, em.PODS)        # q == alloc_pods fires
    assert one(1500, 3 * GIB, [], 4, 1, 500, GIB, [], 3) == (3, em.CPU)         # q == node_cap does not
    assert one(1500, 3 * GIB, [], 4, 1, 500, GIB, [], 2) == (2, em.CAP)
    assert one(0, 3 * GIB, [], 4, 1, 500, GIB, [], 0) == (0, em.CPU)            # no CPU left: CPU-bound
    assert one(0, -5, [], 4, 1, 500, 2, [], 0) == (-2, em.MEM)                  # a negative quotient beats it
    assert one(1500, 3 * GIB, [], 2, 9, 500, GIB, [], 5) == (-7, em.PODS)       # a negative clamp value
    with pytest.raises(ZeroDivisionError):
        one(1500, 3 * GIB, [], 4, 1, 0, GIB, [], 0)
    assert one(0, 0, [5], 4, 1, 0, 0, [0], 0) == (0, em.CPU)                    # nothing free: no division


# ---- the model against the other models ------------------------------------------------------
@pytest.mark.parametrize("n,S,R,G", [(te.RUN + 1, te.S3, 2, 5), (te.RUN + 1, te.S3, 4, None),
                                     (129, 65, 0, 3)])
def test_model_is_the_capped_fit_and_left_is_the_identity(n, S, R, G):
    c = te.case(n, S, R, G)
    tab, (t, e, wr, wp, left) = c["tab"], c["cells"]
    g1 = c["G"]
    q, dz = xm.pair_table(c["rows"], c["ax"], c["ux"], c["sc"], c["sm"], c["sx"])
    assert np.array_equal(dz, tab["dz"])
    # q before the cap is the extended fit's; after it, the capped fit's
    capb = np.broadcast_to(c["cap"][None, :], q.shape)
    capped = np.where((capb > 0) & (q > capb), capb, q)
    assert np.array_equal(capped[~dz], tab["q"][~dz])
    ct, ce, _, grows = sp.capped_cells(q, dz, c["gid"], g1, c["cap"])
    assert np.array_equal(np.asarray(ct).reshape(g1, S), t)
    assert np.array_equal(np.asarray(ce).reshape(g1, S), e)
    ok = e == 0
    assert np.array_equal(wr.sum(axis=0)[ok], np.broadcast_to(grows[:, None], (g1, S))[ok])
    assert np.array_equal(wp.view(np.uint64).sum(axis=0, dtype=np.uint64).view(np.int64)[ok], t[ok])
    assert not wr[:, ~ok].any() and not wp[:, ~ok].any() and not left[:, ~ok].any()
    assert (~ok).any() and not wr[em.EXT0 + R:em.PODS].any()
    # left by rows == sum(free) - request x totals, modulo 2^64
    assert np.array_equal(em.left_by_identity(tab, t, e, c["sc"], c["sm"], c["sx"], c["gid"], g1),
                          left)
    assert (left < 0).any() and (left > 0).any()


def test_explain_groups_against_the_model():
    n, S, R, G = te.RUN + 1, te.S3, 2, 5
    c = te.case(n, S, R, G)
    t, e, wr, wp, left = c["cells"]
    res = ExplainResult(t, e, wr, wp, left)
    rng = np.random.default_rng(5)
    grows = np.array([(c["gid"] == g).sum() for g in range(G)], np.int64)
    assert grows[1] == 0
    for el in (rng.random((G, S)) < 0.7, np.array([True, True, False, True, True]),
               np.zeros(G, bool)):
        for gr in (None, grows):
            got = explain_groups(res, el, gr)
            want = em.fold_groups(c["cells"], el, gr)
            for a, b in zip((got.totals, got.err, got.why_rows, got.why_pods, got.left), want):
                assert np.array_equal(a, b)
            assert got.why_rows.shape == (8, S) and got.left.shape == (2 + R, S)
    full = explain_groups(res, np.ones(G, bool))
    assert (full.err != 0).any() and not full.why_rows[:, full.err != 0].any()
    ok = full.err == 0
    assert np.array_equal(full.why_rows.sum(axis=0)[ok], np.full(S, grows.sum())[ok])
    part = explain_groups(ExplainResult(t, e, None, wp, None), np.ones(G, bool))
    assert part.why_rows is None and part.left is None and np.array_equal(part.why_pods, full.why_pods)
    with pytest.raises(ValueError):
        explain_groups(res, np.ones(G + 1, bool))


# ---- the GPU tests' inputs carry what they are meant to ----------------------------------
def fast_pairs(c):
    """[N, S]: the pair runs on the fast path (a fast row under a wave of 64 fast specs)."""
    rows, ax, ux, sx = c["rows"], c["ax"], c["ux"], c["sx"]
    n, S = len(rows[0]), len(c["sc"])
    rf = np.array([xm.row_is_fast(int(rows[0][i]), int(rows[1][i]), int(rows[4][i]),
                                  int(rows[5][i]), ax[:, i].tolist(), ux[:, i].tolist())
                   for i in range(n)])
    sf = np.array([xm.spec_is_fast(int(c["sc"][s]), int(c["sm"][s]), sx[:, s].tolist())
                   for s in range(S)])
    wf = np.array([sf[s // 64 * 64:s // 64 * 64 + 64].all() for s in range(S)])
    return rf[:, None] & wf[None, :]


def test_generated_inputs_reach_every_slot_and_tie():
    c = te.case(te.RUN + 1, te.S3, 4, 5)
    tab = c["tab"]
    fast = fast_pairs(c)
    live = ~tab["dz"]
    on_fast = np.bincount(tab["b"][fast & live], minlength=8)
    on_exact = np.bincount(tab["b"][~fast & live], minlength=8)
    print("fast pairs by slot", on_fast.tolist(), "exact pairs by slot", on_exact.tolist(),
          "ties", tab["ties"])
    assert (on_fast > 0).all() and (on_exact > 0).all()
    assert fast.any(axis=1).sum() > 200 and (~fast.any(axis=1)).sum() >= 4  # rows off the fast path
    assert all(v > 0 for v in tab["ties"].values())
    # every other case of the GPU tests: each slot it can reach, each tie
    for n, S, R, G, special in [(n, 96, 2, None, True) for n in te.ALL_N[2:]] + \
            [(129, 257, 1, 3, True), (129, 64, 1, 3, False)] + \
            [(te.RUN + 1, te.S3, R, None, True) for R in range(5)]:
        k = te.case(n, S, R, G, special)
        slots = [b for b in range(8) if b < 2 + R or b >= em.PODS]
        f = fast_pairs(k)
        ok = ~k["tab"]["dz"]
        assert set(k["tab"]["b"][f & ok].tolist()) == set(slots), (n, S, R, G)
        if special:
            assert set(k["tab"]["b"][~f & ok].tolist()) == set(slots), (n, S, R, G)
            assert k["tab"]["dz"].any() and (k["cells"][1] != 0).any()
        ties = k["tab"]["ties"]
        assert ties["qc==qm"] and ties["q==alloc_pods"] and ties["q==node_cap"] and \
            (ties["q==qx"] or R == 0), (n, S, R, G)
    # the listed rows and specs are there
    c = te.case(te.RUN + 1, te.S3, 2, 5)
    fc, fm, fx = c["tab"]["free"]
    assert max(fc) >= 1 << 31 and max(fm) >= 1 << 50 and min(fm) < 0 and max(fx[1]) >= 1 << 50
    assert 0 in fc and 0 in fm and (c["rows"][3] > c["rows"][2]).any() and (c["rows"][2] < 0).any()
    sc, sm, sx = c["sc"], c["sm"], c["sx"]
    assert (sc == 0).any() and (sm == 0).any() and (sm == -1).any() and (sx == 0).any()
    assert (sc > 1 << 52).any() and (sm > 1 << 52).any() and (sx < 0).any()
    assert (c["tab"]["q"] < 0).any()
    gid = c["gid"]
    assert (gid < 0).any() and (gid >= 5).any() and not (gid == 1).any()
    assert (np.diff(gid) < 0).any()  # unsorted: a run of GRP_RUN records holds several groups


# ---- the kernels compile for gfx950 without spills ----------------------------------------
HIPCC = shutil.which("hipcc") or shutil.which(
    os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"))


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_kernels_compile_without_scratch(tmp_path):
    out = tmp_path / "kcc_explain.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                    "--cuda-device-only", "-I", os.path.join(ROOT, "include"), SRC, "-o",
                    str(out)], check=True, capture_output=True)
    asm = out.read_text()
    meta = {}
    for blk in asm.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                      for k in ("private_segment_fixed_size", "vgpr_count", "sgpr_count",
                                "group_segment_fixed_size")}
    want = ["why_finalize_kernel"]
    for r in range(_lib.KCC_EXT_MAX + 1):
        want += [f"why_pairs_kernelILi{r}E", f"why_free_kernelILi{r}E"]
    for k in want:
        hit = [v for name, v in meta.items() if k in name]
        assert len(hit) == 1, (k, sorted(meta))
        print(k, "vgpr", hit[0]["vgpr_count"], "sgpr", hit[0]["sgpr_count"], "lds",
              hit[0]["group_segment_fixed_size"])
        assert hit[0]["private_segment_fixed_size"] == 0, k
        assert hit[0]["group_segment_fixed_size"] <= 64 * 1024, k
    assert len(meta) == len(want)
    assert set(re.findall(r"; ScratchSize: (\d+)", asm)) == {"0"}


# ---- the CLI refuses what it cannot explain -----------------------------------------------
def test_cli_refuses_explain_with_zone_spread(cli):  # noqa: F811
    for args in (["-explain", "-spreadBy", "zone"], ["-spreadBy=zone", "-explain=true", "-maxSkew=2"]):
        r = _run(args + ["-cluster", "/nonexistent/cluster.txt"])  # (never opened)
        assert r.returncode == 2 and r.stdout == ""
        assert "-explain cannot be combined with -spreadBy zone" in r.stderr
        assert "cannot open" not in r.stderr
    r = _run(["-explain=false", "-spreadBy=zone", "-cluster", "/nonexistent/cluster.txt"])
    assert "cannot be combined" not in r.stderr and "cannot open" in r.stderr
