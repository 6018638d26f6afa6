"""The CLI's -byPool (host/cluster_capacity.cpp): `pool <name>` lines of the cluster file,
"Pool <name> : <total>" per spec and pool in first-appearance order from kcc_fit_grouped,
checked against the Python oracle run on each pool's rows; without the flag a file with
pool lines prints byte for byte what the same file without them prints."""
import numpy as np
import pytest

from oracle import pyoracle
from tests.test_host import _run, cli, parse_expected, write_cluster  # noqa: F401

POOLS = ["gpu-a", "spot", "system"]
PANIC = "panic: runtime error: integer divide by zero"


def write_pooled(tmp_path):
    """The 60-node file of tests/test_host.py and a copy with pool lines: every fourth node
    unlabelled (pool "-", first to appear), the others in 3 named pools."""
    plain = write_cluster(str(tmp_path / "plain.txt"))
    rng = np.random.default_rng(21)
    out, pools = [], []
    for line in open(plain).read().splitlines():
        out.append(line)
        if line.startswith("node "):
            i = len(pools)
            name = "-" if i % 4 == 0 else POOLS[int(rng.integers(0, 3))]
            pools.append(name)
            if name != "-":
                out.append(f"pool {name}")
    pooled = tmp_path / "pooled.txt"
    pooled.write_text("\n".join(out) + "\n")
    return plain, str(pooled), pools


def pool_lines(stdout):
    return [ln for ln in stdout.splitlines() if ln.startswith("Pool ")]


@pytest.mark.gpu
def test_cli_by_pool_matches_oracle_per_pool(cli, tmp_path):  # noqa: F811
    plain, pooled, pools = write_pooled(tmp_path)
    arrays = parse_expected(plain)
    order = list(dict.fromkeys(pools))
    assert order[0] == "-" and sorted(order[1:]) == sorted(POOLS) and len(pools) == 60

    def want(sc, sm):
        lines = []
        for name in order:
            sel = [i for i, p in enumerate(pools) if p == name]
            t, e = pyoracle.fit(*[[a[i] for i in sel] for a in arrays], [sc], [sm])
            lines.append(f"Pool {name} : {PANIC if e[0] else t[0]}")
        return lines

    # one spec: the pool lines follow the closing rule line
    r = _run(["-cluster", pooled, "-cpuRequests=200m", "-memRequests=250mb", "-replicas=10",
              "-byPool"])
    assert r.returncode == 0, r.stderr
    tail = r.stdout.splitlines()[-len(order) - 1:]
    assert set(tail[0]) == {"="}
    assert tail[1:] == want(200, 262_144_000)
    # a batch with a zero cpu request (0.5 -> Atoi fails -> 0) and a zero memory request
    specs = tmp_path / "specs.txt"
    specs.write_text("200m 250mb 10\n0.5 1G 3\n1 0.5B 3\n")
    r = _run(["-cluster", pooled, "-specs", str(specs), "--byPool=true"])
    assert r.returncode == 0, r.stderr
    got = pool_lines(r.stdout)
    exp = want(200, 262_144_000) + want(0, 1 << 30) + want(1000, 0)
    assert got == exp
    assert any(PANIC in ln for ln in got) and any(PANIC not in ln for ln in got)


@pytest.mark.gpu
def test_cli_pool_lines_change_nothing_without_the_flag(cli, tmp_path):  # noqa: F811
    plain, pooled, _ = write_pooled(tmp_path)
    specs = tmp_path / "specs.txt"
    specs.write_text("200m 250mb 10\n0.5 1G 3\n")
    for args in (["-cpuRequests=200m", "-memRequests=250mb"], ["-v"], ["-specs", str(specs)],
                 ["-cpuRequests=0.5"]):
        a = _run(["-cluster", plain] + args)
        b = _run(["-cluster", pooled] + args)
        assert a.returncode == b.returncode
        assert a.stdout.encode() == b.stdout.encode() and "Pool " not in b.stdout
