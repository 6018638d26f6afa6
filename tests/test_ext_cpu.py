"""Extended-resource fit (kcc_fit_ext), the checks that need no GPU:

  - the header declares both entry points and _lib.SIGNATURES binds them with its arity;
  - tests/ext_model.py (the semantics in Python integers) against oracle.pyoracle.fit where
    the two must agree: R = 0, every request zero, and an extra column that copies the
    memory column (for every spec, zero and negative memory requests included);
  - the fast path: grp_div's model (tests/test_groups_cpu.py model_div) on the extra
    resource's bounds (0 <= fx < 2^50, 1 <= x <= 2^52), and a numpy restatement of the fast
    pair in which a lane that does not request a resource divides by 1.0 and has that
    quotient selected away before the one conversion — every intermediate stays finite;
  - kcc_ext.hip compiles for gfx950 and no kernel of it has a private segment.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from kubernetesclustercapacity_amd import _lib, synth
from oracle import pyoracle
from tests import ext_model as xm
from tests.test_groups_cpu import _edge_values, model_div

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "kubernetesclustercapacity_amd", "csrc", "kcc_ext.hip")
I64 = np.iinfo(np.int64)


# ---- ABI ---------------------------------------------------------------------------------
def test_header_and_signatures():
    ar = _lib.header_arities()
    assert ar.get("kcc_fit_ext") == 19
    assert ar.get("kcc_fit_ext_async") == 20
    for name in ("kcc_fit_ext", "kcc_fit_ext_async"):
        assert name in _lib.header_symbols()
        assert len(_lib.SIGNATURES[name][1]) == ar[name]
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define\s+KCC_EXT_MAX\s+4\b", text) and _lib.KCC_EXT_MAX == 4
    assert re.search(r"#define\s+KCC_ABI_VERSION\s+2\b", text)  # adding symbols: unchanged


# ---- the model against the reference's restatement ---------------------------------------
@pytest.fixture(scope="module")
def adv():
    """A 160-row adversarial cluster, its request sums, 24 adversarial specs and the
    two-resource answer of oracle.pyoracle.fit."""
    n, S = 160, 24
    c = synth.make_cluster(n, 20 * n, seed=13, chunk=1024, adversarial=True)
    sums = pyoracle.reduce_requests(c.node_ptr, c.cpu_req, c.mem_req)
    uc = np.array([s[0] for s in sums], np.uint64)
    um = np.array([s[1] for s in sums], np.int64)
    rows = [c.alloc_cpu, c.alloc_mem, c.alloc_pods, c.pod_count, uc, um]
    sc, sm = synth.make_specs(S, seed=13, adversarial=True)
    assert (sc == 0).any() and (sm == 0).any() and (sm < 0).any() and (sm == -1).any()
    t, e = pyoracle.fit(*rows, sc, sm)
    assert any(e) and not all(e)
    return rows, sc, sm, np.array(t, np.int64), np.array(e, np.int32)


def test_model_equals_pyoracle_at_r0(adv):
    rows, sc, sm, t, e = adv
    n, S = rows[0].size, sc.size
    mt, me = xm.fit_ext(rows, np.zeros((0, n), np.int64), np.zeros((0, n), np.int64), sc, sm,
                        np.zeros((0, S), np.int64))
    assert np.array_equal(mt, t) and np.array_equal(me, e)
    # one group per row, a few ids skipped: every cell is fit_one of that row
    gid = np.arange(n)
    gid[::17] = -1
    gt, ge = xm.fit_ext(rows, np.zeros((0, n), np.int64), np.zeros((0, n), np.int64), sc, sm,
                        np.zeros((0, S), np.int64), gid, n)
    for i in (0, 1, 17, n - 1):
        for s in range(S):
            try:
                want = (pyoracle.fit_one(*[int(a[i]) for a in rows], int(sc[s]), int(sm[s])), 0)
            except ZeroDivisionError:
                want = (0, 1)
            if gid[i] < 0:
                want = (0, 0)
            assert (int(gt[i, s]), int(ge[i, s])) == want


def test_all_zero_requests_change_nothing(adv):
    rows, sc, sm, t, e = adv
    n, S = rows[0].size, sc.size
    rng = np.random.default_rng(13)
    ax = rng.integers(I64.min, I64.max, (3, n), dtype=np.int64)
    ux = rng.integers(I64.min, I64.max, (3, n), dtype=np.int64)
    mt, me = xm.fit_ext(rows, ax, ux, sc, sm, np.zeros((3, S), np.int64))
    assert np.array_equal(mt, t) and np.array_equal(me, e)
    # one resource requested by nobody beside one that is
    sx = np.zeros((2, S), np.int64)
    sx[1] = rng.integers(1, 1 << 40, S)
    a, _ = xm.fit_ext(rows, ax[:2], ux[:2], sc, sm, sx)
    b, _ = xm.fit_ext(rows, ax[1:2], ux[1:2], sc, sm, sx[1:])
    assert np.array_equal(a, b) and not np.array_equal(a, t)


def test_memory_copy_changes_nothing(adv):
    rows, sc, sm, t, e = adv
    mt, me = xm.fit_ext(rows, rows[1][None], rows[5][None], sc, sm, sm[None])
    assert np.array_equal(me, e)
    assert np.array_equal(mt, t)
    # a zero memory request with no free memory anywhere: no panic, and the copy (zero:
    # not requested) still changes nothing
    full = [a.copy() for a in rows]
    full[1] = full[5].copy()  # alloc_mem == used_mem on every row
    t0, e0 = pyoracle.fit(*full, sc, sm)
    z = int(np.flatnonzero((sm == 0) & (sc != 0))[0])
    assert e0[z] == 0
    mt, me = xm.fit_ext(full, full[1][None], full[5][None], sc, sm, sm[None])
    assert mt.tolist() == list(t0) and me.tolist() == list(e0)


def test_extra_resource_binds_and_never_panics():
    # free CPU 3000, free memory 6 GiB, 2 free GPUs of 8; 110 pod slots, 10 taken
    row = (4000, 8 << 30, 110, 10, 1000, 2 << 30)
    q = lambda x, c=100, m=1 << 28: xm.fit_one_ext(*row, [8], [6], c, m, [x])  # noqa: E731
    assert q(0) == 24 and q(1) == 2 and q(2) == 1 and q(3) == 0 and q(-1) == -2
    assert xm.fit_one_ext(4000, 8 << 30, 110, 10, 1000, 2 << 30, [6], [8], 100, 1 << 28, [1]) == 0
    # the clamp follows the mins: qc = 3000 >= 110 alone would clamp to 100
    assert q(1, c=1, m=1) == 2 and q(0, c=1, m=1) == 100
    # the difference wraps: alloc 0, used MinInt64 -> fx = MinInt64; MinInt64 / -1 wraps
    assert xm.ext_quotient(0, I64.min, -1) == I64.min
    assert xm.ext_quotient(0, I64.min, 1) == I64.min
    assert xm.ext_quotient(I64.max, -5, 3) == pyoracle.go_div_i64(pyoracle.i64(I64.max + 5), 3)
    with pytest.raises(ZeroDivisionError):
        q(1, c=0)
    with pytest.raises(ZeroDivisionError):
        q(1, m=0)


# ---- the fast path -----------------------------------------------------------------------
def test_fast_division_model_on_the_extra_bounds():
    rng = np.random.default_rng(17)
    f = _edge_values(0, xm.FX_MAX, rng, 500)
    d = _edge_values(1, xm.SPEC_MAX + 1, rng, 500)
    F, D = [v.ravel() for v in np.meshgrid(f, d)]
    k = rng.integers(0, 1 << 20, F.size)
    mult = np.clip((F // D) * D + (k % 3 - 1), 0, xm.FX_MAX - 1)
    for ff in (F, mult):
        for ulps in (0, 2, -2):
            assert np.array_equal(model_div(ff, D, ulps), ff // D)
    # the issue's edge divisors, fx = k x + {-1, 0, 1} up to 2^50 - 1
    for x in (1, 3, (1 << 26) - 1, (1 << 26) + 1, (1 << 52) - 1, 1 << 52):
        ks = np.unique(np.clip(np.array([0, 1, 2, 1000, (xm.FX_MAX - 1) // x]), 0, None))
        fx = (ks[:, None] * x + np.array([-1, 0, 1])).ravel()
        fx = np.unique(np.clip(fx, 0, xm.FX_MAX - 1))
        assert np.array_equal(model_div(fx, np.full(fx.size, x)), fx // x), x


def fast_pair_model(fc, fm, fx, P, cl, c, m, x):
    """ext_pairs' fast branch in numpy f64, every floating-point warning an error.  fx / x
    are [R, n].  A zero x divides by 1.0 and is selected away; only the selected minimum is
    converted.  Returns (q, the f64 values that reached the conversion)."""
    with np.errstate(all="raise"):
        t = np.minimum(model_div(fc, c), model_div(fm, m)).astype(np.float64)
        for r in range(len(x)):
            xd = np.where(x[r] == 0, 1, x[r])
            tx = model_div(fx[r], xd).astype(np.float64)
            assert np.isfinite(tx).all()
            t = np.where((x[r] != 0) & (tx < t), tx, t)
        assert np.isfinite(t).all() and (t < 2.0 ** 31).all() and (t >= 0).all()
        q = t.astype(np.int32).astype(np.int64)
    return np.where(q >= P, cl, q), t


def test_zero_request_lane_never_reaches_a_conversion():
    rng = np.random.default_rng(19)
    n, R = 20_000, 4
    fc = rng.integers(0, xm.FC_MAX, n)
    fm = rng.integers(0, xm.FX_MAX, n)
    fx = rng.integers(0, xm.FX_MAX, (R, n))
    fx[:, ::5] = 0
    c = rng.integers(1, 8000, n)
    m = rng.integers(1 << 20, 1 << 35, n)
    x = rng.integers(1, 1 << 36, (R, n))
    x[rng.random((R, n)) < 0.4] = 0
    x[0, :64] = 0  # a whole wave's worth of unrequested lanes
    P = rng.integers(-3, 300, n)
    cl = P - rng.integers(0, 300, n)
    got, t = fast_pair_model(fc, fm, fx, P, cl, c, m, x)
    want = np.minimum(fc // c, fm // m)
    for r in range(R):
        want = np.where(x[r] != 0, np.minimum(want, fx[r] // np.where(x[r] == 0, 1, x[r])), want)
    assert np.array_equal(t.astype(np.int64), want)
    assert np.array_equal(got, np.where(want >= P, cl, want))
    # what the finite divisor avoids: 1.0 / 0 is +inf and 0 * inf a NaN
    with np.errstate(all="ignore"):
        assert np.isinf(np.float64(1.0) / np.float64(0.0))
        assert np.isnan(np.float64(0.0) * (np.float64(1.0) / np.float64(0.0)))
    # and the model's answer is the integer model's on the same pairs
    for i in range(0, 400, 7):
        rowx = [int(v) for v in fx[:, i]]
        q = xm.fit_one_ext(int(fc[i]), int(fm[i]), int(P[i]), int(P[i] - cl[i]), 0, 0, rowx,
                           [0] * R, int(c[i]), int(m[i]), [int(v) for v in x[:, i]])
        assert q == int(got[i]), i


def test_fast_classes():
    assert xm.row_is_fast(xm.FC_MAX - 1, xm.FX_MAX - 1, 0, 0, [xm.FX_MAX - 1], [0])
    assert not xm.row_is_fast(xm.FC_MAX - 1, xm.FX_MAX - 1, 0, 0, [xm.FX_MAX], [0])
    assert not xm.row_is_fast(1, 1, 0, 0, [0], [I64.min])  # the difference wraps negative
    assert xm.row_is_fast(1, 1, 0, 0, [5], [9])            # alloc <= used: free 0
    assert xm.spec_is_fast(1, 1, [0, xm.SPEC_MAX])
    assert not xm.spec_is_fast(1, 1, [xm.SPEC_MAX + 1])
    assert not xm.spec_is_fast(1, 1, [-1]) and not xm.spec_is_fast(0, 1, [])


# ---- the kernels compile for gfx950 without spills ----------------------------------------
HIPCC = shutil.which("hipcc") or shutil.which(
    os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"))

KERNELS = ["ext_rows_kernel", "ext_scatter_kernel", "ext_pairs_kernel"]
LDS_STATIC_MAX = 64 * 1024


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_kernels_compile_without_scratch(tmp_path):
    out = tmp_path / "kcc_ext.s"
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
    # every kernel once per R = 0 .. KCC_EXT_MAX (R is the template argument, ILi<R>E)
    for k in KERNELS:
        for r in range(_lib.KCC_EXT_MAX + 1):
            hit = [v for name, v in meta.items() if k + f"ILi{r}E" in name]
            assert len(hit) == 1, (k, r, sorted(meta))
            print(k, r, "vgpr", hit[0]["vgpr_count"], "lds", hit[0]["group_segment_fixed_size"],
                  hit[0])
            assert hit[0]["private_segment_fixed_size"] == 0, (k, r)
            assert hit[0]["group_segment_fixed_size"] <= LDS_STATIC_MAX, (k, r)
    assert len(meta) == len(KERNELS) * (_lib.KCC_EXT_MAX + 1)
    assert set(re.findall(r"; ScratchSize: (\d+)", asm)) == {"0"}
    # the R = 0 instances are the grouped fit's kernels: the pair loop's 8
    # waves per SIMD (<= 64 VGPRs) and 256 x (48 + 4) B of staged records, the scatter's
    # GRP_LDS_GROUPS x 4 B of per-workgroup counts
    pairs0, = [v for name, v in meta.items() if "ext_pairs_kernelILi0E" in name]
    scatter0, = [v for name, v in meta.items() if "ext_scatter_kernelILi0E" in name]
    assert pairs0["group_segment_fixed_size"] == 13312 and pairs0["vgpr_count"] <= 64, pairs0
    assert scatter0["group_segment_fixed_size"] == 16384, scatter0
    assert pairs0["private_segment_fixed_size"] == 0 == scatter0["private_segment_fixed_size"]
