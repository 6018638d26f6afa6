"""The CLI's drain what-if (host/cluster_capacity.cpp -drain pool=|zone=|node= with
-drainPolicy pack|spread): the README's worked example, line for line, under both policies; a
`daemon` pod that goes away with its node; -drain with -byPool, -explain, -extRequests and
-specs; a flagged shape; the refusals and an unknown name."""
import pytest

from tests.test_host import _run, cli  # noqa: F401
from tests.test_host_ext import total_line

GiB, MiB = 1 << 30, 1 << 20
OK4 = "False False False False"
DAEMON_POD = ["pod A kube-system agent Running", "daemon", f"container 100m 100m {100 * MiB} {100 * MiB}"]


def example(daemon=True, extra=()):
    """Three nodes A, B, C of 4 cores / 16 GiB / 110 pods in zones a, b, b (pools p1, p2, p2).  A
    runs two pods of 1 core / 1 GiB and a daemon pod of 100m / 100 MiB, B one pod of 2 cores /
    2 GiB, C nothing."""
    lines = [f"node A 4 16777216Ki 110 {OK4}", "zone a", "pool p1", "resource amd.com/gpu 8",
             f"node B 4 16777216Ki 110 {OK4}", "zone b", "pool p2", "resource amd.com/gpu 8",
             f"node C 4 16777216Ki 110 {OK4}", "zone b", "pool p2", "resource amd.com/gpu 1",
             "pod A default web-1 Running", f"container 1 2 {GiB} {GiB}", "request amd.com/gpu 1",
             "pod A default web-2 Running", f"container 500m 1 {GiB // 2} {GiB}",
             f"container 500m 1 {GiB // 2} {GiB}", "request amd.com/gpu 1"]
    lines += [ln for ln in DAEMON_POD if daemon or ln != "daemon"]
    lines += ["pod B default db-1 Running", f"container 2 2 {2 * GiB} {2 * GiB}"]
    return "\n".join(lines + list(extra)) + "\n"


@pytest.fixture
def files(tmp_path):
    def write(name, text):
        p = tmp_path / name
        p.write_text(text)
        return str(p)
    return write


SPEC = ["-cpuRequests=1", "-memRequests=1G", "-replicas=4"]
LINE = "Drained 1 nodes : 2 pods evicted, 2 placed, 0 not placed (1 shapes)"


def drained(out):
    return [ln for ln in out.splitlines() if ln.startswith(("Drained ", "Drain shape "))]


@pytest.mark.gpu
def test_cli_worked_example(cli, files):  # noqa: F811
    path = files("cluster.txt", example())
    r = _run(["-cluster", path] + SPEC)
    assert r.returncode == 0 and total_line(r.stdout) == [7] and not drained(r.stdout), r.stderr
    for policy in ([], ["-drainPolicy=spread"], ["-drainPolicy", "pack"]):
        r = _run(["-cluster", path, "-drain", "zone=a"] + policy + SPEC)
        assert r.returncode == 0, r.stderr
        out = r.stdout.splitlines()
        echo = [i for i, ln in enumerate(out) if ln.startswith("CPU limits, requests")]
        total = [i for i, ln in enumerate(out) if "Total possible replicas" in ln]
        assert drained(r.stdout) == [LINE] and echo[0] < out.index(LINE) < total[0]
        assert total_line(r.stdout) == [4]
        assert "So you can go ahead with deployment of 4 pod replicas" in r.stdout
        # where the two pods went: B holds one more replica under spread, none under pack
        r = _run(["-cluster", path, "-drain=zone=a", "-byPool", "-maxPerNode=1"] + policy + SPEC)
        assert total_line(r.stdout) == [2 if policy[-1:] != ["pack"] else 1], r.stdout
    # the same row by pool and by name
    for how in ("pool=p1", "node=A"):
        r = _run(["-cluster", path, "-drain", how] + SPEC)
        assert r.returncode == 0 and drained(r.stdout) == [LINE] and total_line(r.stdout) == [4]
    # two nodes: three pods of two shapes, all on C, which is then full
    r = _run(["-cluster", path, "-drain", "node=A,B"] + SPEC)
    assert drained(r.stdout) == ["Drained 2 nodes : 3 pods evicted, 3 placed, 0 not placed (2 shapes)"]
    assert total_line(r.stdout) == [0] and "Unfortunately" in r.stdout
    # every node: nowhere to go
    r = _run(["-cluster", path, "-drain", "zone=b", "-drain", "node=A,B,C"] + SPEC)
    assert drained(r.stdout) == ["Drained 3 nodes : 3 pods evicted, 0 placed, 3 not placed (2 shapes)"]
    assert total_line(r.stdout) == [0]


@pytest.mark.gpu
def test_cli_daemon_pod_is_not_counted(cli, files):  # noqa: F811
    # without its `daemon` line the agent pod is evicted and placed like any other
    path = files("nodaemon.txt", example(daemon=False))
    r = _run(["-cluster", path, "-drain", "zone=a"] + SPEC)
    assert r.returncode == 0, r.stderr
    assert drained(r.stdout) == ["Drained 1 nodes : 3 pods evicted, 3 placed, 0 not placed (2 shapes)"]
    assert total_line(r.stdout) == [3]  # (spread: the agent lands on B, which then has 900m free)
    path = files("cluster.txt", example())
    r = _run(["-cluster", path, "-drain", "zone=a"] + SPEC)
    assert drained(r.stdout) == [LINE]
    # the `daemon` line changes nothing without -drain
    a, b = _run(["-cluster", path] + SPEC), _run(["-cluster", files("n2.txt", example(False))] + SPEC)
    assert a.stdout == b.stdout and a.returncode == b.returncode == 0


@pytest.mark.gpu
def test_cli_drain_composes(cli, files):  # noqa: F811
    path = files("cluster.txt", example())
    r = _run(["-cluster", path, "-drain", "zone=a", "-byPool", "-explain"] + SPEC)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert drained(r.stdout) == [LINE] and total_line(r.stdout) == [4]
    assert [ln for ln in out if ln.startswith("Pool ")] == ["Pool p1 : 0", "Pool p2 : 4"]
    # the drained row counts under cpu with 0 replicas and 0 left over
    assert [ln for ln in out if ln.startswith("Limited by ")] == ["Limited by cpu : 3 nodes, 4 replicas"]
    assert [ln for ln in out if ln.startswith("Left over ")] == \
        ["Left over cpu : 0m", f"Left over memory : {(13 + 15 - 4) * GiB}"]
    # an extended resource: the evicted pods carry their gpu requests to B (C has one gpu: the
    # even fill gives it one pod, B the other), and the spec needs one gpu a replica
    r = _run(["-cluster", path, "-drain", "zone=a", "-extRequests=amd.com/gpu=1", "-spreadBy=zone"] + SPEC)
    assert r.returncode == 0, r.stderr
    assert drained(r.stdout) == [LINE] and total_line(r.stdout) == [1]  # B: 1000m free, 7 gpus; C: 0 gpus
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("Zone ")] == ["Zone a : 0 of 0", "Zone b : 1 of 1"]
    # a batch of specs on the drained state
    specs = files("specs.txt", "1 1G 4\n500m 100mb 9\n")
    r = _run(["-cluster", path, "-drain", "zone=a", "-drainPolicy=pack", "-specs", specs])
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-2:] == ["1 1G 4 total=4 yes", "500m 100mb 9 total=8 no"]


@pytest.mark.gpu
def test_cli_drain_flagged_shape(cli, files):  # noqa: F811
    """A pod without requests (0 cpu, 0 memory) meets free room: its shape is not placed, the
    CLI names it, and the other shapes are placed."""
    path = files("zero.txt", example(extra=["pod A default idle Running", "container 0 0 0 0"]))
    r = _run(["-cluster", path, "-drain", "zone=a"] + SPEC)
    assert r.returncode == 0, r.stderr
    got = drained(r.stdout)
    assert got[0] == "Drained 1 nodes : 3 pods evicted, 2 placed, 1 not placed (2 shapes)"
    assert len(got) == 2 and got[1].startswith("Drain shape 0m 0 : 1 pods not placed")
    assert "integer divide by zero" in got[1] and total_line(r.stdout) == [4]


@pytest.mark.gpu
def test_cli_unhealthy_node_is_not_drained(cli, files):  # noqa: F811
    """An unhealthy node keeps a zero row and the reference lists no pods for it: named by
    -drain it is known, but not drained, not counted, and its pods are not evicted."""
    extra = ["node D 4 16777216Ki 110 False True False False", "zone a", "pool p1",
             "pod D default lost Running", f"container 1 1 {GiB} {GiB}"]
    path = files("sick.txt", example(extra=extra))
    r = _run(["-cluster", path, "-drain", "zone=a"] + SPEC)
    assert r.returncode == 0 and drained(r.stdout) == [LINE] and total_line(r.stdout) == [4], r.stderr
    r = _run(["-cluster", path, "-drain", "node=D"] + SPEC)
    assert r.returncode == 0, r.stderr
    assert drained(r.stdout) == ["Drained 0 nodes : 0 pods evicted, 0 placed, 0 not placed (0 shapes)"]
    assert total_line(r.stdout) == [7]


@pytest.mark.gpu
def test_cli_drain_refusals_and_unknown_names(cli, files):  # noqa: F811
    path = files("cluster.txt", example())
    plan = files("plan.txt", "500m 1G 2\n")
    for extra in (["-deploy", plan], ["-priority=5"], ["-schedulerRequests"], ["-v"]):
        r = _run(["-cluster", path, "-drain", "zone=a"] + extra + SPEC)
        assert r.returncode == 2 and f"-drain cannot be combined with {extra[0].split('=')[0]}" in r.stderr
        assert "Drained" not in r.stdout and "Total possible" not in r.stdout
    for how, what in (("pool=nosuch", "pool nosuch"), ("zone=c", "zone c"), ("node=A,Z", "name Z")):
        r = _run(["-cluster", path, "-drain", how] + SPEC)
        assert r.returncode == 1 and f"-drain: no node with {what}" in r.stderr, (r.stdout, r.stderr)
        assert "Drained" not in r.stdout and "Total possible" not in r.stdout
    for bad in (["-drain", "rack=1"], ["-drain", "zone"], ["-drain", "zone="],
                ["-drain", "node=,"], ["-drain", "node=,,"],
                ["-drain", "zone=a", "-drainPolicy=evenly"]):
        r = _run(["-cluster", path] + bad + SPEC)
        assert r.returncode == 2 and "invalid value" in r.stderr
