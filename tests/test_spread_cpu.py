"""Spread constraints in the fit (kcc_fit_capped, kcc_spread_fold), the
checks that need no GPU:

  - the header declares the four entry points and _lib.SIGNATURES binds them with its arity;
  - tests/spread_model.py (the semantics in Python integers) on hand cases — the 10 / 4 / 7
    example, a full zone, cap 1, the saturating limit, an ineligible domain, an empty group,
    two groups of one domain — and on its identities with tests/ext_model.py and
    select_groups;
  - the inputs tests/test_spread.py generates carry what they are meant to, on the model;
  - kcc_spread.hip compiles for gfx950 and no kernel of it has a private segment.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from kubernetesclustercapacity_amd import _lib
from kubernetesclustercapacity_amd.engine import select_groups
from tests import ext_model as xm
from tests import spread_model as sp
from tests import test_spread as ts
from tests.test_ext import gpu_storage_expected, pairs
from tests.test_groups import group_ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "kubernetesclustercapacity_amd", "csrc", "kcc_spread.hip")
I64 = np.iinfo(np.int64)


def fold1(caps, k, **kw):
    """One spec, one group per entry of caps."""
    t = np.array(caps, np.int64)[:, None]
    tot, err, _ = sp.fold(t, np.zeros_like(t, np.int32), max_skew=[k], **kw)
    return int(tot[0]), int(err[0])


# ---- ABI ---------------------------------------------------------------------------------
def test_header_and_signatures():
    ar = _lib.header_arities()
    want = {"kcc_fit_capped": 22, "kcc_fit_capped_async": 23, "kcc_spread_fold": 12,
            "kcc_spread_fold_async": 13}
    for name, k in want.items():
        assert name in _lib.header_symbols()
        assert ar.get(name) == k
        assert len(_lib.SIGNATURES[name][1]) == k
    # kcc_fit_capped is kcc_fit_ext's arguments, then three
    assert _lib.SIGNATURES["kcc_fit_capped"][1][:19] == _lib.SIGNATURES["kcc_fit_ext"][1]
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define\s+KCC_ABI_VERSION\s+2\b", text)  # adding symbols: unchanged


# ---- hand cases --------------------------------------------------------------------------
def test_the_issue_example_and_a_full_zone():
    assert fold1([10, 4, 7], 1) == (14, 0)       # 5 + 4 + 5
    assert fold1([10, 4, 7], 0) == (21, 0)       # unconstrained: the plain sum
    assert fold1([10, 4, 7], 3) == (18, 0)       # lim 7: 7 + 4 + 7
    assert fold1([10, 4, 7], 2) == (16, 0)
    assert fold1([10, 0, 7], 1) == (2, 0)        # a full zone: every zone at most maxSkew
    assert fold1([10, 0, 7], 2) == (4, 0)
    assert fold1([10, -3, 7], 2) == (-3 - 1 - 1, 0)  # signed min; the limit may be negative
    assert fold1([], 1) == (0, 0)


def test_limit_saturates():
    big = int(I64.max)
    assert fold1([big - 1, big], 5) == (sp.i64(2 * big - 1), 0)   # lim = MaxInt64: nothing clipped
    assert fold1([big - 2, big], 1) == (sp.i64(2 * big - 3), 0)   # lim = MaxInt64 - 1 clips one
    assert fold1([5, big], big) == (sp.i64(5 + big), 0)           # 5 + MaxInt64 saturates
    assert fold1([-5, big], big) == (sp.i64(-5 + big - 5), 0)     # -5 + MaxInt64 does not


def test_ineligible_domain_empty_group_and_shared_domain():
    t = np.array([[10], [4], [7]], np.int64)
    e = np.zeros((3, 1), np.int32)
    # the smallest zone is not eligible: neither the min nor the sum sees it
    tot, err, caps = sp.fold(t, e, eligible=[True, False, True], max_skew=[1])
    assert tot.tolist() == [8 + 7] and caps[0] == {0: 10, 2: 7}
    # ... even when its cell is flagged
    e2 = e.copy()
    e2[1] = 1
    assert sp.fold(t, e2, eligible=[True, False, True], max_skew=[1])[0].tolist() == [15]
    tot, err, _ = sp.fold(t, e2, max_skew=[1])      # eligible and flagged: select_groups' rule
    assert tot.tolist() == [0] and err.tolist() == [1]
    # an empty group is not a domain: its 0 would force every zone to maxSkew
    t0 = np.array([[10], [0], [7]], np.int64)
    assert sp.fold(t0, e, group_rows=[5, 0, 2], max_skew=[1])[0].tolist() == [8 + 7]
    assert sp.fold(t0, e, group_rows=[5, 3, 2], max_skew=[1])[0].tolist() == [1 + 0 + 1]
    # two groups of one domain add before the min: zones {10 + 4, 7} -> lim 8
    tot, _, caps = sp.fold(t, e, domain_of=[0, 0, 1], n_domains=2, max_skew=[1])
    assert caps[0] == {0: 14, 1: 7} and tot.tolist() == [8 + 7]
    # a domain id outside [0, D) is skipped
    assert sp.fold(t, e, domain_of=[0, 2, 1], n_domains=2, max_skew=[1])[0].tolist() == [8 + 7]


def test_cap_one_counts_the_rows_that_hold_a_replica():
    q, dz, _, _ = gpu_storage_expected()  # an ordinary accelerator cluster: no panic
    keep = ~(q < 0).any(axis=1)           # rows without a negative clamp value
    assert not dz.any() and keep.sum() > 900
    q, dz = q[keep], dz[keep]
    n, S = q.shape
    gid = group_ids(n, 7, 3)
    t, e, m, r = sp.capped_cells(q, dz, None, 1, np.ones(S, np.int64))
    assert np.array_equal(t, (q >= 1).sum(axis=0)) and (t > 0).any() and (t < n).any()
    t, e, m, r = sp.capped_cells(q, dz, gid, 7, np.ones(S, np.int64))
    for g in range(7):
        assert np.array_equal(t[g], (q[gid == g] >= 1).sum(axis=0))
        assert r[g] == (gid == g).sum()
    # the cap follows the clamp: q = 500 over a pod limit of 110 with 100 pods is 10, then 2
    q1 = np.array([[10], [1], [0], [-4]], np.int64)
    t, _, m, _ = sp.capped_cells(q1, np.zeros((4, 1), bool), None, 1, [2])
    assert t.tolist() == [2 + 1 + 0 - 4] and m.tolist() == [-4]


# ---- identities --------------------------------------------------------------------------
@pytest.mark.parametrize("G", [None, 7, 1000])
def test_no_cap_is_the_ext_model(G):
    n, S, R = 257, 65, 2
    q, dz = pairs(n, S, R)
    gid = None if G is None else group_ids(n, G, 3)
    g1 = 1 if G is None else G
    want = xm.totals_from_pairs(q, dz, gid, g1)
    for cap in (None, np.zeros(S, np.int64), np.full(S, -3, np.int64), np.full(S, I64.max, np.int64)):
        t, e, m, r = sp.capped_cells(q, dz, gid, g1, cap)
        assert np.array_equal(t, want[0]) and np.array_equal(e, want[1])
    ids = np.zeros(n, np.int64) if gid is None else gid
    assert r.tolist() == [int((ids == g).sum()) for g in range(g1)]
    assert ((m == I64.max).reshape(g1, S) == (r == 0)[:, None]).all()
    assert not m[e != 0].any()


def test_unconstrained_fold_is_select_groups():
    n, S, R, G = 257, 65, 2, 7
    t, e, m, r = ts.want_cells(n, S, R, G)
    el = ts.eligibility(G, S)
    for sk in (None, np.zeros(S, np.int64), np.full(S, -1, np.int64)):
        tot, err, _ = sp.fold(t, e, eligible=el, max_skew=sk)
        st, se = select_groups(t, e, el)
        assert np.array_equal(tot, st) and np.array_equal(err, se)
        assert (err != 0).any() and (err == 0).any()
    # many-to-one domains do not change an unconstrained total
    tot2, err2, _ = sp.fold(t, e, domain_of=np.arange(G) % 3, n_domains=3, eligible=el)
    assert np.array_equal(tot2, tot) and np.array_equal(err2, err)


# ---- the GPU tests' inputs carry what they are meant to ----------------------------------
def test_generated_inputs_cover_the_listed_cases():
    n, S, R, G = 1025, 65, 2, 1000
    assert sorted(set(ts.node_caps(S).tolist())) == sorted(ts.CAPS)
    assert sorted(set(ts.skews(S).tolist())) == sorted(ts.SKEWS)
    q, dz = pairs(n, S, R)
    cap = ts.node_caps(S)
    binds = (q > cap[None, :]) & (cap[None, :] > 0)
    assert binds.any() and ((cap[None, :] > 0) & ~binds).any()      # the cap binds on some pairs
    assert binds[:, cap == 1].any() and not binds[:, cap == I64.max].any()
    t, e, m, r = ts.want_cells(n, S, R, G)
    t0 = ts.want_cells(n, S, R, G, capped=False)[0]
    assert (t != t0).any() and (t < 0).any() and (e != 0).any() and (e == 0).any()
    assert (m < 0).any() and (r == 0).any() and (r > 1).any()
    for ordinary in (False, True):
        t, e, m, r = ts.want_cells(n, S, R, G, ordinary)
        dom, el, sk = ts.domain_map(G, 3), ts.eligibility(G, S), ts.skews(S)
        assert ((dom < 0) | (dom >= 3)).sum() >= 4 and len(set(dom.tolist()) & {0, 1, 2}) == 3
        assert 0.6 < el.mean() < 0.8 and (~el.any(axis=0)).sum() == 2
        tot, err, caps = sp.fold(t, e, r, dom, 3, el, sk)
        free, _, _ = sp.fold(t, e, r, dom, 3, el, None)
        ok = err == 0
        lowered = ok & (tot != free)
        print("ordinary" if ordinary else "adversarial", "specs flagged", int((~ok).sum()),
              "lowered by the skew", int(lowered.sum()), "left", int((ok & ~lowered).sum()))
        assert lowered.any() and (ok & ~lowered & (sk > 0)).any()  # the skew lowers some, leaves others
        assert not lowered[sk <= 0].any()
        assert any(not c for c, f in zip(caps, ok) if f)           # a spec with no present domain
        assert tot[~el.any(axis=0)].tolist() == [0, 0]
        if not ordinary:
            assert (~ok).any() and any(v < 0 for c in caps for v in c.values())
    # fit_spread's hostname pass: the second cap differs from the first
    q, dz = pairs(n, S, R, True)
    c = sp.capped_cells(q, dz, None, 1, cap)
    hk = np.array([[0, 1, 3, I64.max][s % 4] for s in range(S)], np.int64)
    cap2 = sp.host_cap(c[2].reshape(1, S), c[3], hk, cap)
    assert (cap2 != cap).any() and (cap2[hk == 0] == np.where(cap > 0, cap, 0)[hk == 0]).all()


# ---- the kernels compile for gfx950 without spills ----------------------------------------
HIPCC = shutil.which("hipcc") or shutil.which(
    os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"))

PLAIN = ["cap_finalize_kernel", "grp_rows_kernel", "fill_i64_kernel", "fold_cells_kernel",
         "fold_finish_kernel"]


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_kernels_compile_without_scratch(tmp_path):
    out = tmp_path / "kcc_spread.s"
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
    want = PLAIN + [f"cap_pairs_kernelILi{r}E" for r in range(_lib.KCC_EXT_MAX + 1)]
    for k in want:
        hit = [v for name, v in meta.items() if k in name]
        assert len(hit) == 1, (k, sorted(meta))
        print(k, "vgpr", hit[0]["vgpr_count"], "sgpr", hit[0]["sgpr_count"], "lds",
              hit[0]["group_segment_fixed_size"])
        assert hit[0]["private_segment_fixed_size"] == 0, k
        assert hit[0]["group_segment_fixed_size"] <= 64 * 1024, k
    assert len(meta) == len(want)
    assert set(re.findall(r"; ScratchSize: (\d+)", asm)) == {"0"}
