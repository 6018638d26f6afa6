"""kcc_deploy (a rollout plan placed on the nodes), the checks that need no
GPU:

  - the header declares the two entry points and _lib.SIGNATURES binds them with its arity;
  - tests/deploy_model.py (the semantics in Python integers) on hand cases and on its
    identities with tests/ext_model.py and tests/spread_model.py; its numpy form against its
    pure form;
  - the inputs tests/test_deploy.py generates carry what they are meant to, on the model;
  - kcc_deploy.hip compiles for gfx950, no kernel of it has a private segment, each at most
    64 KiB of LDS;
  - the CLI's -deploy argument errors that exit before a context exists.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from kubernetesclustercapacity_amd import _lib
from tests import deploy_model as dm
from tests import ext_model as xm
from tests import spread_model as spm
from tests import test_deploy as td

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "kubernetesclustercapacity_amd", "csrc", "kcc_deploy.hip")
PACK, SPREAD = dm.PACK, dm.SPREAD
i64, u64 = np.int64, np.uint64


def one_step(case, rep, policy, **kw):
    return dm.deploy(case["rows"], case["ax"], case["ux"], case["sc"], case["sm"], case["sx"],
                     [rep], policy, **kw)


# ---- ABI ---------------------------------------------------------------------------------
def test_header_and_signatures():
    ar = _lib.header_arities()
    for name, k in {"kcc_deploy": 25, "kcc_deploy_async": 26}.items():
        assert name in _lib.header_symbols()
        assert ar.get(name) == k
        assert len(_lib.SIGNATURES[name][1]) == k
    assert _lib.SIGNATURES["kcc_deploy_async"][1][:25] == _lib.SIGNATURES["kcc_deploy"][1]
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define\s+KCC_ABI_VERSION\s+2\b", text)  # adding symbols: unchanged
    assert re.search(r"#define\s+KCC_DEPLOY_PACK\s+0\b", text) and _lib.KCC_DEPLOY_PACK == 0
    assert re.search(r"#define\s+KCC_DEPLOY_SPREAD\s+1\b", text) and _lib.KCC_DEPLOY_SPREAD == 1
    internal = open(os.path.join(os.path.dirname(SRC), "kcc_internal.h")).read()
    ipt = int(re.search(r"DEPLOY_IPT\s*=\s*(\d+);", internal).group(1))
    assert re.search(r"DEPLOY_TILE\s*=\s*256 \* DEPLOY_IPT;", internal)
    assert 256 * ipt == _lib.KCC_DEPLOY_TILE  # the constants _lib restates
    assert int(re.search(r"DEPLOY_SCAN_PASS\s*=\s*(\d+);", internal).group(1)) == _lib.KCC_DEPLOY_SCAN_PASS


# ---- hand cases --------------------------------------------------------------------------
A = [3, 0, 5, 2]


@pytest.mark.parametrize("policy,rep,want", [
    (PACK, 4, [3, 0, 1, 0]), (PACK, 3, [3, 0, 0, 0]), (PACK, 99, A), (PACK, 0, [0] * 4),
    (SPREAD, 4, [2, 0, 1, 1]),   # t = 2, b = [1, 0, 1, 1], rem = 1: the first row with a >= 2
    (SPREAD, 6, [2, 0, 2, 2]),   # rem = 3: all three qualifying rows take one
    (SPREAD, 9, [3, 0, 4, 2]), (SPREAD, 10, A), (SPREAD, 0, [0] * 4), (SPREAD, 1, [1, 0, 0, 0])])
def test_hand_cases(policy, rep, want):
    assert dm.place(A, rep, policy) == want
    assert dm.place_np(np.array(A, i64), rep, policy).tolist() == want
    r = one_step(td.uniform_case(4, A), rep, policy)  # the same through the whole step
    assert r.rows[0].tolist() == want and r.placed[0] == sum(want) and r.err[0] == 0
    assert r.nodes_used[0] == sum(1 for v in want if v)
    assert r.pod_count.tolist() == want and r.used_cpu.tolist() == [1000 * v for v in want]
    assert r.used_mem.tolist() == want


def test_negative_clamp_row_holds_nothing():
    case = td.uniform_case(3, 10)
    case["rows"][2][:] = [5, 1 << 62, 5]   # allocatable pods
    case["rows"][3][:] = [9, 0, 2]         # pod count: row 0's clamp value is 5 - 9 = -4
    for policy in (PACK, SPREAD):
        r = one_step(case, 100, policy)
        assert r.rows[0].tolist() == [0, 10, 3]  # (row 2: q = 10 >= 5 -> 5 - 2)
        assert r.pod_count.tolist() == [9, 10, 5] and r.used_cpu[0] == 0 and r.used_mem[0] == 0


def test_panic_flags_the_step_unless_ineligible_and_steps_chain():
    n = 4
    case = td.uniform_case(n, A)
    case["sc"] = np.array([0, 1000], u64)     # step 0 asks for 0 millicores: Go panics
    case["sm"] = np.array([1, 1], i64)
    case["sx"] = np.ones((0, 2), i64)
    args = (case["rows"], case["ax"], case["ux"], case["sc"], case["sm"], case["sx"])
    r = dm.deploy(*args, [5, 4], PACK)
    assert r.err.tolist() == [1, 0] and r.placed.tolist() == [0, 4]
    assert r.rows.tolist() == [[0] * 4, [3, 0, 1, 0]]      # the state was untouched by step 0
    # row 1 is full (a = 0 but free CPU 999 > 0 panics too): only ineligibility silences a row
    gid = np.array([0, 0, 0, 0], np.int32)
    el = np.array([[False, True]])
    r = dm.deploy(*args, [5, 4], PACK, group=gid, n_groups=1, eligible=el)
    assert r.err.tolist() == [0, 0] and r.placed.tolist() == [0, 4]
    # step 2 sees step 1's commit
    case = td.uniform_case(n, A)
    case["sc"], case["sm"] = np.array([1000, 1000], u64), np.array([1, 1], i64)
    case["sx"] = np.ones((0, 2), i64)
    r = dm.deploy(case["rows"], case["ax"], case["ux"], case["sc"], case["sm"], case["sx"], [4, 4], PACK)
    assert r.rows.tolist() == [[3, 0, 1, 0], [0, 0, 4, 0]]
    r = dm.deploy(case["rows"], case["ax"], case["ux"], case["sc"], case["sm"], case["sx"], [4, 99], SPREAD)
    assert r.rows.tolist() == [[2, 0, 1, 1], [1, 0, 4, 1]] and r.placed.tolist() == [4, 6]
    # ids outside [0, G) take nothing; the cap follows the clamp
    r = one_step(td.uniform_case(n, A), 99, PACK, group=np.array([0, 1, 2, -1]), n_groups=2,
                 node_cap=[2])
    assert r.rows[0].tolist() == [2, 0, 0, 0]


# ---- identities --------------------------------------------------------------------------
@pytest.mark.parametrize("policy", [PACK, SPREAD])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_identities(seed, policy):
    n, K, R = 300, 4, 2
    case = td.plain_case(seed, n, K, R)
    cap = np.array([0, 2, 7, 0], i64)
    rep = td.plan_replicas(case, K, policy, 0, cap=cap)  # a third, a half, all and more, none
    ax, sc, sm, sx = case["ax"], case["sc"], case["sm"], case["sx"]
    r = dm.deploy(case["rows"], ax, case["ux"], sc, sm, sx, rep, policy, cap)
    alloc = [[int(v) for v in c] for c in case["rows"][:3]] + [ax.tolist()]
    rows, ux = list(case["rows"]), case["ux"]
    binding = 0
    for k in range(K):  # the plan one step a call: each step's a on the state it sees
        Rk = dm.clamp_replicas(rep[k])
        state = [[int(v) for v in c] for c in rows[3:]] + [ux.tolist()]
        a = dm.counts(state, alloc, (int(sc[k]), int(sm[k]), sx[:, k].tolist()), Rk, int(cap[k]),
                      [True] * n)
        p = r.rows[k].tolist()
        assert r.placed[k] == min(Rk, sum(a))
        assert all(0 <= x <= y for x, y in zip(p, a))
        binding += 1 <= Rk < sum(a)
        if policy == SPREAD:  # among the rows with room left the counts differ by at most 1
            short = [x for x, y in zip(p, a) if x < y]
            assert not short or max(short) - min(short) <= 1
            assert not short or all(x <= max(short) + 1 for x in p)  # nobody above the level
        one = dm.deploy(rows, ax, ux, sc[k:k + 1], sm[k:k + 1], sx[:, k:k + 1], [rep[k]], policy,
                        cap[k:k + 1])
        assert one.rows[0].tolist() == p
        rows, ux = rows[:3] + [one.pod_count, one.used_cpu, one.used_mem], one.used_x
    assert binding >= 1
    for got, f in zip(rows[3:] + [ux], ("pod_count", "used_cpu", "used_mem", "used_x")):
        assert np.array_equal(got, getattr(r, f))  # K calls of one step == one call of K steps


def test_two_half_steps_pack_equal_one():
    n, R = 257, 2
    case = td.plain_case(5, n, 1, R)
    case["rows"][2][:] = 1 << 62  # the clamp never fires
    args = (case["rows"], case["ax"], case["ux"])
    tail = (case["sx"], )
    T = int(one_step(case, 1 << 40, PACK).placed[0])
    for rep in (T // 2 * 2, 20, 2 * T + 2):
        one = dm.deploy(*args, case["sc"], case["sm"], *tail, [rep], PACK)
        two = dm.deploy(*args, np.repeat(case["sc"], 2), np.repeat(case["sm"], 2),
                        np.repeat(case["sx"], 2, axis=1), [rep // 2, rep // 2], PACK)
        assert two.placed.sum() == one.placed[0] and np.array_equal(two.rows.sum(axis=0), one.rows[0])
        for f in ("pod_count", "used_cpu", "used_mem", "used_x"):
            assert np.array_equal(getattr(one, f), getattr(two, f))


@pytest.mark.parametrize("policy", [PACK, SPREAD])
def test_unbounded_step_is_the_capped_total(policy):
    n, S, R = 300, 5, 2
    case = td.plain_case(6, n, S, R)
    case["rows"][3] = np.minimum(case["rows"][3], case["rows"][2])  # no negative clamp value
    q, dz = xm.pair_table(case["rows"], case["ax"], case["ux"], case["sc"], case["sm"], case["sx"])
    assert not dz.any() and (q >= 0).all()
    cap = np.array([0, 1, 3, -2, 1 << 40], i64)
    t, e, _, _ = spm.capped_cells(q, dz, None, 1, cap)
    for s in range(S):
        r = dm.deploy(case["rows"], case["ax"], case["ux"], case["sc"][s:s + 1], case["sm"][s:s + 1],
                      case["sx"][:, s:s + 1], [dm.R_MAX], policy, cap[s:s + 1])
        assert r.placed[0] == t[s] and r.err[0] == 0


# ---- the numpy form against the pure form ---------------------------------------------------
@pytest.mark.parametrize("policy", [PACK, SPREAD])
@pytest.mark.parametrize("n,K,R,G", [(1, 1, 0, 1), (65, 4, 2, 3), (300, 3, 1, 1), (1025, 2, 2, 5)])
def test_numpy_form_equals_pure_form(n, K, R, G, policy):
    case = td.plain_case(n, n, K, R)
    gid = None if G == 1 else td.fz.group_layout(n, n, G, "uniform")
    el = None if G == 1 else np.random.default_rng(n).random((G, K)) < 0.7
    cap = np.array([0, 2, 1000, -1], i64)[:K]
    rep = td.plan_replicas(case, K, policy, n, gid, G, el, cap)
    args = (case["rows"], case["ax"], case["ux"], case["sc"], case["sm"], case["sx"], rep, policy,
            cap, gid, G, el)
    a, b = dm.deploy(*args), dm.deploy_np(*args)
    for f in td.FIELDS:
        assert getattr(a, f).dtype == getattr(b, f).dtype, f
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
    assert n < 65 or a.placed.sum() > 0


# ---- the GPU tests' inputs carry what they are meant to ----------------------------------
def test_generated_inputs_cover_the_listed_cases():
    n, K, R, G = 1025, 4, 2, 5
    case = td.plain_case(7, n, K, R)
    q, dz = xm.pair_table(case["rows"], case["ax"], case["ux"], case["sc"], case["sm"], case["sx"])
    assert not dz.any() and (q < 0).any() and (q == 0).any() and (q > 2).any()
    q0, _ = xm.pair_table(case["rows"], case["ax"], case["ux"], case["sc"], case["sm"],
                          np.zeros_like(case["sx"]))
    assert (q != q0).any()                      # an extra resource decides some pairs
    gid = td.fz.group_layout(n, n, G, "uniform")
    assert ((gid < 0) | (gid >= G)).any()
    for policy in (PACK, SPREAD):
        rep = td.plan_replicas(case, K, policy, 0)
        r = dm.deploy(case["rows"], case["ax"], case["ux"], case["sc"], case["sm"], case["sx"], rep, policy)
        assert 0 < r.placed[0] == rep[0] and r.placed[2] < rep[2] and r.placed[3] == 0
        assert 0 < r.nodes_used[0] < n
        if policy == SPREAD:
            assert r.nodes_used[0] > dm.deploy(case["rows"], case["ax"], case["ux"], case["sc"],
                                               case["sm"], case["sx"], rep, PACK).nodes_used[0]
    # the adversarial plans hold flagged and unflagged steps
    flagged = steps = 0
    for seed in range(10, 40):
        c = td.fz.make_cell_case(seed, 65, 4, 1)
        r = dm.deploy(c["rows"], c["ax"], c["ux"], c["sc"], c["sm"], c["sx"],
                      td.plan_replicas(c, 4, PACK, seed), PACK)
        flagged += int(r.err.sum())
        steps += 4
    print("adversarial steps", steps, "flagged", flagged)
    assert 0 < flagged < steps
    assert td.SCAN_N <= 1 << 20 and td.SCAN_N > _lib.KCC_DEPLOY_SCAN_PASS * _lib.KCC_DEPLOY_TILE


# ---- the kernels compile for gfx950 without scratch ----------------------------------------
HIPCC = shutil.which("hipcc") or shutil.which(
    os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"))
PLAIN = ["dp_hist_kernel", "dp_ind_kernel", "dp_scan_kernel"]


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_kernels_compile_without_scratch(tmp_path):
    out = tmp_path / "kcc_deploy.s"
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
    want = PLAIN + [f"{k}ILi{r}ELb{b}E" for k in ("dp_rows_kernel", "dp_apply_kernel")
                    for r in range(_lib.KCC_EXT_MAX + 1) for b in (0, 1)]
    for k in want:
        hit = [v for name, v in meta.items() if k in name]
        assert len(hit) == 1, (k, sorted(meta))
        print(k, "vgpr", hit[0]["vgpr_count"], "sgpr", hit[0]["sgpr_count"], "lds",
              hit[0]["group_segment_fixed_size"])
        assert hit[0]["private_segment_fixed_size"] == 0, k
        assert hit[0]["group_segment_fixed_size"] <= 64 * 1024, k
    assert len(meta) == len(want)
    assert set(re.findall(r"; ScratchSize: (\d+)", asm)) == {"0"}


# ---- the CLI's argument errors that exit before a context exists ---------------------------
from tests.test_host import _run, cli  # noqa: E402, F401


def test_cli_deploy_argument_errors(cli, tmp_path):  # noqa: F811
    good = tmp_path / "plan.txt"
    good.write_text("100m 100mb 5 spread perNode:2 amd.com/gpu=1  # fine\n")
    for line in ("100m 100mb 5 sideways", "100m 100mb 5 Spread", "100m 100mb 5 perNode:x",
                 "100m 100mb 5 perNode:-1", "100m 100mb 5 pack =1"):
        bad = tmp_path / "bad.txt"
        bad.write_text("# a plan\n100m 100mb 5 pack\n" + line + "\n")
        r = _run(["-cluster", "/nonexistent", "-deploy", str(bad)])
        assert r.returncode == 2 and r.stdout == "" and "invalid token" in r.stderr, line
        assert line.split()[-1] in r.stderr
    r = _run(["-cluster", "/nonexistent", "-v", "-deploy", str(good)])
    assert r.returncode == 2 and r.stdout == "" and "-v cannot be combined with -deploy" in r.stderr
    r = _run(["-cluster", "/nonexistent", "-deploy", str(tmp_path / "missing.txt")])
    assert r.returncode == 1 and r.stdout == "" and "cannot open deploy file" in r.stderr
    r = _run(["-deploy"])
    assert r.returncode == 2 and "flag needs an argument: -deploy" in r.stderr
