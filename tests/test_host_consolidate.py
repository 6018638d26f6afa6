"""The CLI's removal what-if (host/cluster_capacity.cpp -consolidate all | below=<pct> |
node=<a,b,...>): the README's worked example, line for line, and its second run; below= and
node=; pods without requests and `daemon` pods; -consolidate with -specs, -byPool, -explain,
-extRequests, -maxPerNode and -spreadBy zone (the fits unchanged); the refusals and an unknown
name."""
import pytest

from tests.test_host import _run, cli  # noqa: F401
from tests.test_host_drain import SPEC, example, files  # noqa: F401
from tests.test_host_ext import total_line

GiB = 1 << 30
NODE = "Node {} : {} pods evicted, {} placed, {} not placed, {} without requests"
SUMMARY = "Removable one at a time : {} of {} nodes ({} counting pods without requests as placed)"
EXAMPLE = [NODE.format("A", 2, 2, 0, 0), NODE.format("B", 1, 1, 0, 0), NODE.format("C", 0, 0, 0, 0),
           SUMMARY.format(3, 3, 3)]
FOURTH = ["pod C default batch Running", f"container 2500m 3 {GiB} {GiB}"]


def report(out):
    return [ln for ln in out.splitlines() if ln.startswith(("Node ", "Removable "))]


def rest(out):
    return [ln for ln in out.splitlines() if not ln.startswith(("Node ", "Removable "))]


@pytest.mark.gpu
def test_cli_worked_example(cli, files):  # noqa: F811
    path = files("cluster.txt", example())
    plain = _run(["-cluster", path] + SPEC)
    assert plain.returncode == 0 and total_line(plain.stdout) == [7] and not report(plain.stdout)
    for flag in (["-consolidate", "all"], ["-consolidate=all"]):
        r = _run(["-cluster", path] + flag + SPEC)
        assert r.returncode == 0, r.stderr
        out = r.stdout.splitlines()
        echo = [i for i, ln in enumerate(out) if ln.startswith("CPU limits, requests")]
        total = [i for i, ln in enumerate(out) if "Total possible replicas" in ln]
        assert report(r.stdout) == EXAMPLE
        assert echo[0] < out.index(EXAMPLE[0]) and out.index(EXAMPLE[-1]) < total[0]
        # the call does not touch the state: every other line is what it is without the flag
        assert rest(r.stdout) == plain.stdout.splitlines() and total_line(r.stdout) == [7]
    # a fourth pod, 2500m on C: A's two pods still go to B, but B's 2-core pod fits neither A's
    # 1900m nor C's 1500m, and C's own pod fits nowhere
    path = files("fourth.txt", example(extra=FOURTH))
    r = _run(["-cluster", path, "-consolidate", "all"] + SPEC)
    assert r.returncode == 0, r.stderr
    assert report(r.stdout) == [NODE.format("A", 2, 2, 0, 0), NODE.format("B", 1, 0, 1, 0),
                                NODE.format("C", 1, 0, 1, 0), SUMMARY.format(1, 3, 1)]


@pytest.mark.gpu
def test_cli_below_and_node(cli, files):  # noqa: F811
    """cpu utilisation: A 52.5 %, B 50 %, C 0 %; memory: 13.1 %, 12.5 %, 0 %.  Both must be below
    the threshold, strictly, in integers."""
    path = files("cluster.txt", example())
    for pct, names in ((53, "ABC"), (51, "BC"), (50, "C"), (13, "C"), (1, "C"), (0, "")):
        r = _run(["-cluster", path, f"-consolidate=below={pct}"] + SPEC)
        assert r.returncode == 0, r.stderr
        want = [ln for ln in EXAMPLE[:3] if ln.split()[1] in names]
        assert report(r.stdout) == want + [SUMMARY.format(len(names), len(names), len(names))], pct
        assert total_line(r.stdout) == [7]
    # by name: listed in node order, once
    r = _run(["-cluster", path, "-consolidate", "node=C,A,C"] + SPEC)
    assert r.returncode == 0, r.stderr
    assert report(r.stdout) == [EXAMPLE[0], EXAMPLE[2], SUMMARY.format(2, 2, 2)]
    # an unhealthy node is never a candidate: known by name, not evaluated
    extra = ["node D 4 16777216Ki 110 False True False False", "zone a", "pool p1",
             "pod D default lost Running", f"container 1 1 {GiB} {GiB}"]
    path = files("sick.txt", example(extra=extra))
    r = _run(["-cluster", path, "-consolidate", "node=D,B"] + SPEC)
    assert r.returncode == 0 and report(r.stdout) == [EXAMPLE[1], SUMMARY.format(1, 1, 1)], r.stderr
    for how in ("all", "below=100"):
        r = _run(["-cluster", path, "-consolidate", how] + SPEC)
        assert r.returncode == 0 and report(r.stdout) == EXAMPLE, r.stderr


@pytest.mark.gpu
def test_cli_pods_without_requests_and_daemon_pods(cli, files):  # noqa: F811
    path = files("zero.txt", example(extra=["pod A default idle Running", "container 0 0 0 0"]))
    r = _run(["-cluster", path, "-consolidate", "all"] + SPEC)
    assert r.returncode == 0, r.stderr
    assert report(r.stdout) == [NODE.format("A", 3, 2, 0, 1)] + EXAMPLE[1:3] + [SUMMARY.format(2, 3, 3)]
    # without its `daemon` line the agent pod is evicted and placed like any other
    path = files("nodaemon.txt", example(daemon=False))
    r = _run(["-cluster", path, "-consolidate", "node=A"] + SPEC)
    assert report(r.stdout) == [NODE.format("A", 3, 3, 0, 0), SUMMARY.format(1, 1, 1)]


@pytest.mark.gpu
def test_cli_too_many_pods(cli, files):  # noqa: F811
    """A candidate with more than KCC_CONS_MAX_PODS evicted pods is not evaluated: it gets a line
    of its own, counts among the candidates and is not removable."""
    extra = []
    for k in range(1025):
        extra += [f"pod C default tiny-{k} Running", "container 1m 1m 1 1"]
    path = files("many.txt", example(extra=extra))
    r = _run(["-cluster", path, "-consolidate", "all"] + SPEC)
    assert r.returncode == 0, r.stderr
    assert report(r.stdout) == EXAMPLE[:2] + ["Node C : 1025 pods evicted, more than 1024: not evaluated",
                                              SUMMARY.format(2, 3, 2)]


@pytest.mark.gpu
def test_cli_consolidate_composes(cli, files):  # noqa: F811
    path = files("cluster.txt", example())
    specs = files("specs.txt", "1 1G 4\n500m 100mb 9\n")
    for extra in (["-byPool", "-explain"], ["-maxPerNode=1", "-byPool"], ["-specs", specs],
                  ["-extRequests=amd.com/gpu=1", "-spreadBy=zone"], ["-extRequests=amd.com/gpu=1"]):
        plain = _run(["-cluster", path] + extra + SPEC)
        r = _run(["-cluster", path, "-consolidate", "all"] + extra + SPEC)
        assert r.returncode == plain.returncode == 0, r.stderr
        assert report(r.stdout) == EXAMPLE and rest(r.stdout) == plain.stdout.splitlines(), extra
    # the pods' `request` lines become pod_x: with one gpu on B and none on C the second of A's
    # pods (one gpu each) has nowhere to go; without -extRequests the gpus are not read
    text = example().replace("resource amd.com/gpu 8", "resource amd.com/gpu 1")
    text = text.replace("resource amd.com/gpu 1", "resource amd.com/gpu 8", 1)
    head, _, tail = text.rpartition("resource amd.com/gpu 1")
    path = files("gpus.txt", head + "resource amd.com/gpu 0" + tail)
    r = _run(["-cluster", path, "-consolidate", "node=A", "-extRequests=amd.com/gpu=1"] + SPEC)
    assert r.returncode == 0, r.stderr
    assert report(r.stdout) == [NODE.format("A", 2, 1, 1, 0), SUMMARY.format(0, 1, 0)]
    r = _run(["-cluster", path, "-consolidate", "node=A"] + SPEC)
    assert report(r.stdout) == [EXAMPLE[0], SUMMARY.format(1, 1, 1)]


@pytest.mark.gpu
def test_cli_consolidate_refusals_and_unknown_names(cli, files):  # noqa: F811
    path = files("cluster.txt", example())
    plan = files("plan.txt", "500m 1G 2\n")
    for extra in (["-drain", "zone=a"], ["-deploy", plan], ["-priority=5"], ["-schedulerRequests"],
                  ["-v"]):
        r = _run(["-cluster", path, "-consolidate", "all"] + extra + SPEC)
        assert r.returncode == 2, (extra, r.stderr)
        assert f"-consolidate cannot be combined with {extra[0].split('=')[0]}" in r.stderr
        assert "Removable" not in r.stdout and "Total possible" not in r.stdout
    r = _run(["-cluster", path, "-consolidate", "node=A,Z"] + SPEC)
    assert r.returncode == 1 and "-consolidate: no node with name Z" in r.stderr
    assert "Removable" not in r.stdout and "Total possible" not in r.stdout
    for bad in ("some", "below", "below=", "below=x", "below=-3", "node=", "node=,", "all=1",
                "pool=p1"):
        r = _run(["-cluster", path, "-consolidate", bad] + SPEC)
        assert r.returncode == 2 and "invalid value" in r.stderr, bad
