"""The CLI's -explain (host/cluster_capacity.cpp): under each spec's result the "Limited by"
and "Left over" lines of one ungrouped kcc_fit_explain call, checked against
tests/explain_model.py over an independent reading of the cluster file — alone, with
-extRequests, -maxPerNode, -specs (a flagged spec prints nothing after its panic line) and
after a -deploy plan; the worked example of the README; and without -explain the output is
byte for byte what it was."""
import pytest

from tests import explain_model as em
from tests.test_host import _run, cli, parse_expected  # noqa: F401
from tests.test_host_deploy import after_plan, write_plan
from tests.test_host_ext import DISK, GPU, read_ext, total_line, write_ext
from tests.test_host_spread import write_healthy

MB = 1 << 20
SLOT_NAMES = {em.CPU: "cpu", em.MEM: "memory", em.PODS: "pods", em.CAP: "perNode"}
EXAMPLE = """node A 4 2097152Ki 110 False False False False
node B 1000m 16777216Ki 110 False False False False
node C 8 67108864Ki 10 False False False False
""" + "".join(f"pod C ns p{k} Running\ncontainer 0 0 0 0\n" for k in range(7))


def want_lines(rows, ax, ux, names, sc, sm, sx, cap):
    """The lines -explain prints under each spec ([] for a flagged one)."""
    S = len(sc)
    tab = em.explain_table(rows, ax, ux, sc, sm, sx, None if cap == 0 else [cap] * S)
    t, e, wr, wp, left = em.explain_cells(tab, sc, sm, sx)
    out = []
    for s in range(S):
        lines = []
        for b in range(em.SLOTS):
            if not e[0, s] and wr[b, 0, s]:
                name = SLOT_NAMES.get(b) or names[b - em.EXT0]
                lines.append(f"Limited by {name} : {wr[b, 0, s]} nodes, {wp[b, 0, s]} replicas")
        if not e[0, s]:
            lines.append(f"Left over cpu : {left[0, 0, s]}m")
            lines.append(f"Left over memory : {left[1, 0, s]}")
            lines += [f"Left over {nm} : {left[2 + r, 0, s]}" for r, nm in enumerate(names)]
        out.append(lines)
    return t[0], e[0], out


def explain_lines(stdout):
    return [ln for ln in stdout.splitlines() if ln.startswith(("Limited by ", "Left over "))]


@pytest.mark.gpu
def test_cli_explain_readme_example(cli, tmp_path):  # noqa: F811
    path = tmp_path / "abc.txt"
    path.write_text(EXAMPLE)
    args = ["-cluster", str(path), "-cpuRequests=500m", "-memRequests=1G", "-replicas=5"]
    r = _run(args + ["-explain"])
    assert r.returncode == 0, r.stderr
    assert total_line(r.stdout) == [7]
    assert r.stdout.splitlines()[-5:] == [
        "Limited by cpu : 1 nodes, 2 replicas", "Limited by memory : 1 nodes, 2 replicas",
        "Limited by pods : 1 nodes, 3 replicas", "Left over cpu : 9500m",
        "Left over memory : 80530636800"]
    r = _run(args + ["-explain", "-maxPerNode", "2"])
    assert r.returncode == 0, r.stderr
    assert total_line(r.stdout) == [6]
    assert r.stdout.splitlines()[-5:] == [
        "Limited by cpu : 1 nodes, 2 replicas", "Limited by memory : 1 nodes, 2 replicas",
        "Limited by perNode : 1 nodes, 2 replicas", "Left over cpu : 10000m",
        f"Left over memory : {76 << 30}"]


@pytest.mark.gpu
def test_cli_explain_against_the_model(cli, tmp_path):  # noqa: F811
    _, ext, _ = write_ext(tmp_path)  # (with unhealthy nodes: their zero rows are rows too)
    rows = parse_expected(ext)
    ax, ux = read_ext(ext, [GPU, DISK])
    args = ["-cluster", ext, "-cpuRequests=200m", "-memRequests=250mb", "-replicas=10"]
    sc, sm = [200], [250 * MB]
    # alone; with a per-node cap; with extended requests; with both
    for extra, names, mx, mu, sx, cap in (
            ([], [], [], [], [], 0),
            (["-maxPerNode=3"], [], [], [], [], 3),
            ([f"-extRequests={GPU}=1,{DISK}=20Gi"], [GPU, DISK], ax, ux, [[1], [20 << 30]], 0),
            ([f"-extRequests={DISK}=20Gi,{GPU}=2", "-maxPerNode", "1"], [DISK, GPU], ax[::-1],
             ux[::-1], [[20 << 30], [2]], 1)):
        r = _run(args + extra + ["-explain"])
        assert r.returncode == 0, r.stderr
        t, e, lines = want_lines(rows, mx, mu, names, sc, sm, sx, cap)
        assert e.tolist() == [0] and total_line(r.stdout) == [int(t[0])]
        tail = r.stdout.splitlines()[-len(lines[0]) - 1:]
        assert set(tail[0]) == {"="} and tail[1:] == lines[0], extra
        assert len(lines[0]) >= 2 + 2 + len(names)
        if cap:
            assert any(ln.startswith("Limited by perNode") for ln in lines[0])
        # without -explain: the same output less those lines, byte for byte
        plain = _run(args + extra)
        off = _run(args + extra + ["-explain=false"])
        kept = "".join(ln for ln in r.stdout.splitlines(True)
                       if not ln.startswith(("Limited by ", "Left over ")))
        assert plain.stdout.encode() == kept.encode() == off.stdout.encode()
        assert not explain_lines(plain.stdout) and plain.stderr == r.stderr
    # -byPool: the explanation comes between the result and the pools
    r = _run(args + ["-explain", "-byPool"])
    out = r.stdout.splitlines()
    first_pool = min(i for i, ln in enumerate(out) if ln.startswith("Pool "))
    assert max(i for i, ln in enumerate(out) if ln.startswith("Left over ")) == first_pool - 1


@pytest.mark.gpu
def test_cli_explain_batch_with_a_flagged_spec(cli, tmp_path):  # noqa: F811
    _, ext, _ = write_ext(tmp_path)
    rows = parse_expected(ext)
    ax, ux = read_ext(ext, [GPU, DISK])
    specs = tmp_path / "specs.txt"
    specs.write_text(f"200m 250mb 10\n0 1G 3\n1 1G 3 {DISK}=1Gi\n50m 10mb 5000 {GPU}=1\n")
    r = _run(["-cluster", ext, "-specs", str(specs), "-explain", "-maxPerNode=40"])
    assert r.returncode == 0, r.stderr
    sc, sm = [200, 0, 1000, 50], [250 * MB, 1 << 30, 1 << 30, 10 * MB]
    sx = [[0, 0, 1 << 30, 0], [0, 0, 0, 1]]  # names in first-appearance order: DISK, GPU
    t, e, lines = want_lines(rows, ax[::-1], ux[::-1], [DISK, GPU], sc, sm, sx, 40)
    assert e.tolist() == [0, 1, 0, 0]
    heads, reps = ["200m 250mb 10", "0 1G 3", "1 1G 3", "50m 10mb 5000"], [10, 3, 3, 5000]
    want = []
    for s, h in enumerate(heads):
        want.append(f"{h} panic: integer divide by zero" if e[s] else
                    f"{h} total={t[s]} {'yes' if t[s] >= reps[s] else 'no'}")
        want += lines[s]
    assert lines[1] == [] and all(len(lines[s]) >= 5 for s in (0, 2, 3))
    assert r.stdout.strip().splitlines()[-len(want):] == want
    plain = _run(["-cluster", ext, "-specs", str(specs), "-maxPerNode=40"])
    assert plain.stdout.strip().splitlines()[-4:] == [w for w in want if not w.startswith(("Li", "Le"))]


@pytest.mark.gpu
def test_cli_explain_after_a_plan(cli, tmp_path):  # noqa: F811
    path, _, _ = write_healthy(tmp_path)
    rows0 = parse_expected(path)
    ax, ux0 = read_ext(path, [GPU, DISK])
    plan = write_plan(tmp_path / "plan.txt")
    rows, ux, deployed = after_plan(rows0, ax, ux0)
    args = ["-cluster", path, "-cpuRequests=200m", "-memRequests=250mb", "-replicas=10",
            f"-extRequests={GPU}=1", "-maxPerNode=3", "-explain"]
    r = _run(args + ["-deploy", plan])
    assert r.returncode == 0, r.stderr
    # the plan names DISK too: the name list is the spec's, then the plan's
    t, e, lines = want_lines(rows, ax, ux, [GPU, DISK], [200], [250 * MB], [[1], [0]], 3)
    assert total_line(r.stdout) == [int(t[0])]
    assert explain_lines(r.stdout) == lines[0]
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("Deployed ")] == deployed
    r0 = _run(args)  # the same cluster without the plan: other numbers
    t0, _, lines0 = want_lines(rows0, ax[:1], ux0[:1], [GPU], [200], [250 * MB], [[1]], 3)
    assert total_line(r0.stdout) == [int(t0[0])] and explain_lines(r0.stdout) == lines0[0]
    assert lines0[0] != lines[0][:len(lines0[0])]
