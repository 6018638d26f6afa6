"""The CLI's -priority (host/cluster_capacity.cpp): `priority <int>` lines after a pod, and
under each spec's result "With preemption of pods below priority p : <total>, at most <V> pods
evicted" from kcc_reduce_requests_levels + kcc_fit_levels.  Checked against the existing models
over an independent reading of a copy of the cluster file from which the pods below p are cut
out — alone, with -extRequests, -maxPerNode, -byPool and -specs; the worked example of the
README; the refusals; and without -priority the output is byte for byte what it was."""
import numpy as np
import pytest

from tests import ext_model as xm
from tests import spread_model as sp
from tests.test_host import _run, cli, parse_expected  # noqa: F401
from tests.test_host_ext import DISK, GPU, read_ext, total_line, write_ext

MB = 1 << 20
# the README's example: three nodes of 4 cores, batch pods (priority 0) fill two of them
EXAMPLE = ("node A 4 16777216Ki 110 False False False False\n"
           "node B 4 16777216Ki 110 False False False False\n"
           "node C 4 16777216Ki 110 False False False False\n"
           + "".join(f"pod {n} batch b{n}{k} Running\ncontainer 900m 900m 1073741824 0\n"
                     for n in "AB" for k in range(4))
           + "pod A prod web Running\npriority 1000\ncontainer 300m 300m 1073741824 0\n"
           + "pod C prod db Running\npriority 1000\ncontainer 2 2 4294967296 0\n")


def write_prio(tmp_path):
    """tests/test_host_ext.py's 60-node file with a priority line after two pods in three
    (0, 100, 1000, -5; the others keep the default 0)."""
    _, ext, pools = write_ext(tmp_path)
    rng = np.random.default_rng(17)
    out = []
    for line in open(ext).read().splitlines():
        out.append(line)
        if line.startswith("pod ") and rng.random() < 0.67:
            out.append(f"priority {rng.choice([0, 100, 1000, -5])}")
    path = tmp_path / "prio.txt"
    path.write_text("\n".join(out) + "\n")
    return ext, str(path), pools


def cut_below(path, p, out_path):
    """A copy of the file without the pods of priority below p (and their lines); returns the
    number of counted pods cut out (on any row: a pod without a node sits on the zero rows)."""
    blocks, cur = [], None
    for line in open(path).read().splitlines():
        kind = line.split()[0]
        if kind == "pod":
            cur = {"lines": [line], "prio": 0}
            blocks.append(cur)
        elif kind == "node":
            cur = None
            blocks.append({"lines": [line], "prio": None})
        elif kind == "priority":
            cur["prio"] = int(line.split()[1])
        elif cur is not None and kind in ("container", "initcontainer", "request", "overhead"):
            cur["lines"].append(line)
        else:
            blocks[-1]["lines"].append(line)
    keep = [b for b in blocks if b["prio"] is None or b["prio"] >= p]
    open(out_path, "w").write("\n".join(ln for b in keep for ln in b["lines"]) + "\n")
    return str(out_path)


def preempt_lines(stdout):
    return [ln for ln in stdout.splitlines() if ln.startswith("With preemption ")]


def want(path, tmp_path, p, sc, sm, names=(), sx=(), cap=0, pools=None):
    """(total per spec, err per spec, pods evicted, pool cells) of -priority p."""
    cut = cut_below(path, p, tmp_path / f"cut{p}.txt")
    rows, rows0 = parse_expected(cut), parse_expected(path)
    ax, ux = read_ext(cut, list(names))
    q, dz = xm.pair_table(rows, ax, ux, sc, sm, [list(x) for x in sx])
    caps = None if cap == 0 else [cap] * len(sc)
    t, e, _, _ = sp.capped_cells(q, dz, None, 1, caps)
    cells = None
    if pools is not None:
        order = list(dict.fromkeys(pools))
        gid = [order.index(x) for x in pools]
        cells = sp.capped_cells(q, dz, gid, len(order), caps)[:2] + (order,)
    return t, e, sum(rows0[3]) - sum(rows[3]), cells


@pytest.mark.gpu
def test_cli_priority_readme_example(cli, tmp_path):  # noqa: F811
    path = tmp_path / "prio.txt"
    path.write_text(EXAMPLE)
    args = ["-cluster", str(path), "-cpuRequests=1", "-memRequests=1G", "-replicas=8"]
    r = _run(args + ["-priority", "1000"])
    assert r.returncode == 0, r.stderr
    # as things stand: A 4000 - 3900 -> 0, B 4000 - 3600 -> 0, C 4000 - 2000 -> 2
    assert total_line(r.stdout) == [2] and "Unfortunately" in r.stdout
    # the eight batch pods make way: A 3700 -> 3, B 4000 -> 4, C -> 2
    assert preempt_lines(r.stdout) == [
        "With preemption of pods below priority 1000 : 9, at most 8 pods evicted"]
    r = _run(args + ["-priority=1001"])  # everything yields: 4 + 4 + 4, ten pods
    assert preempt_lines(r.stdout) == [
        "With preemption of pods below priority 1001 : 12, at most 10 pods evicted"]
    r = _run(args + ["-priority=-7"])  # nothing is below: the plain total
    assert preempt_lines(r.stdout) == [
        "With preemption of pods below priority -7 : 2, at most 0 pods evicted"]


@pytest.mark.gpu
def test_cli_priority_against_the_model(cli, tmp_path):  # noqa: F811
    ext, path, pools = write_prio(tmp_path)
    args = ["-cluster", path, "-cpuRequests=200m", "-memRequests=250mb", "-replicas=10"]
    sc, sm = [200], [250 * MB]
    for extra, names, sx, cap in (
            ([], [], [], 0),
            (["-maxPerNode=3"], [], [], 3),
            ([f"-extRequests={GPU}=1,{DISK}=20Gi"], [GPU, DISK], [[1], [20 << 30]], 0),
            ([f"-extRequests={DISK}=20Gi,{GPU}=2", "-maxPerNode", "1"], [DISK, GPU],
             [[20 << 30], [2]], 1)):
        for p in ((100, 1000) if not extra else (100,)):
            r = _run(args + extra + [f"-priority={p}"])
            assert r.returncode == 0, r.stderr
            t, e, v, _ = want(path, tmp_path, p, sc, sm, names, sx, cap)
            assert e.tolist() == [0] and v > 0
            assert preempt_lines(r.stdout) == [
                f"With preemption of pods below priority {p} : {t[0]}, at most {v} pods evicted"], extra
            # the line follows the result; without the flag the same output less that line, and
            # the priority lines of the file change nothing
            out = r.stdout.splitlines()
            assert set(out[-2]) == {"="} and out[-1].startswith("With preemption ")
            plain = _run(args + extra)
            kept = "".join(ln for ln in r.stdout.splitlines(True) if not ln.startswith("With preemption "))
            assert plain.stdout.encode() == kept.encode() and plain.stderr == r.stderr
    assert _run(["-cluster", ext] + args[2:]).stdout.encode() == _run(args).stdout.encode()


@pytest.mark.gpu
def test_cli_priority_batch_and_pools(cli, tmp_path):  # noqa: F811
    _, path, pools = write_prio(tmp_path)
    specs = tmp_path / "specs.txt"
    specs.write_text(f"200m 250mb 10\n0 1G 3\n1 1G 3 {DISK}=1Gi\n50m 10mb 5000 {GPU}=1\n")
    sc, sm = [200, 0, 1000, 50], [250 * MB, 1 << 30, 1 << 30, 10 * MB]
    sx = [[0, 0, 1 << 30, 0], [0, 0, 0, 1]]  # names in first-appearance order: DISK, GPU
    r = _run(["-cluster", path, "-specs", str(specs), "-priority", "100", "-byPool"])
    assert r.returncode == 0, r.stderr
    t, e, v, (ct, ce, order) = want(path, tmp_path, 100, sc, sm, [DISK, GPU], sx, 0, pools)
    assert e.tolist() == [0, 1, 0, 0]
    got = preempt_lines(r.stdout)
    assert got == [f"With preemption of pods below priority 100 : panic: runtime error: integer divide by zero"
                   if e[s] else
                   f"With preemption of pods below priority 100 : {t[s]}, at most {v} pods evicted"
                   for s in range(4)]
    out = r.stdout.strip().splitlines()
    heads = [i for i, ln in enumerate(out) if ln.startswith(("200m 250mb", "0 1G", "1 1G", "50m 10mb"))]
    assert len(heads) == 4 and all(out[i + 1].startswith("With preemption ") for i in heads)
    for s, i in enumerate(heads):  # the pools' lines, then the pools with preemption
        blk = out[i + 2: i + 2 + 2 * len(order)]
        assert [ln.split(" : ")[0] for ln in blk] == \
            [f"Pool {g}" for g in order] + [f"Pool {g} with preemption" for g in order]
        wantp = ["panic: runtime error: integer divide by zero" if ce[g, s] else str(ct[g, s])
                 for g in range(len(order))]
        assert [ln.split(" : ")[1] for ln in blk[len(order):]] == wantp
    plain = _run(["-cluster", path, "-specs", str(specs), "-byPool"])
    kept = "".join(ln for ln in r.stdout.splitlines(True) if "ith preemption " not in ln)
    assert plain.stdout.encode() == kept.encode()


@pytest.mark.gpu
def test_cli_priority_refusals(cli, tmp_path):  # noqa: F811
    _, path, _ = write_prio(tmp_path)
    plan = tmp_path / "plan.txt"
    plan.write_text("100m 100mb 3\n")
    for extra, word in ((["-schedulerRequests"], "-schedulerRequests"),
                        (["-deploy", str(plan)], "-deploy"),
                        (["-spreadBy", "zone"], "-spreadBy zone")):
        r = _run(["-cluster", path, "-priority", "100"] + extra)
        assert r.returncode == 2 and r.stdout == ""
        assert r.stderr.startswith(f"-priority cannot be combined with {word}"), r.stderr
    r = _run(["-cluster", path, "-priority", "high"])
    assert r.returncode == 2 and "invalid value \"high\" for flag -priority" in r.stderr
    bad = tmp_path / "bad.txt"
    bad.write_text("node A 4 16777216Ki 110 False False False False\npriority 5\n")
    r = _run(["-cluster", str(bad), "-priority", "1"])
    assert r.returncode == 2 and "priority before any pod" in r.stderr
