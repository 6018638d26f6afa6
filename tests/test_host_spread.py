"""The CLI's spread constraints (host/cluster_capacity.cpp): `zone <name>` lines of the
cluster file, -maxPerNode, -spreadBy zone and -maxSkew.  The totals come from kcc_fit_capped
and kcc_spread_fold and are checked against tests/spread_model.py over an independent
reading of the file, alone and with -byPool / -extRequests; without the new flags a file
with zone lines prints byte for byte what the same file without them prints."""
import numpy as np
import pytest

from tests import ext_model as xm
from tests import spread_model as sp
from tests.test_host import _run, cli, parse_expected  # noqa: F401
from tests.test_host_ext import DISK, GPU, PANIC, read_ext, total_line, write_ext

ZONES = ["z-a", "z-b", "z-c"]


def write_zoned(tmp_path):
    """tests/test_host_ext.py's 60-node file (two named pools and "-") and a copy with zone
    lines: every fifth node unlabelled (zone "-", first to appear), the others in 3 zones."""
    _, ext, pools = write_ext(tmp_path)
    rng = np.random.default_rng(41)
    out, zones = [], []
    for line in open(ext).read().splitlines():
        out.append(line)
        if line.startswith("node "):
            name = "-" if len(zones) % 5 == 0 else ZONES[int(rng.integers(0, 3))]
            zones.append(name)
            if name != "-":
                out.append(f"zone {name}")
    zoned = tmp_path / "zoned.txt"
    zoned.write_text("\n".join(out) + "\n")
    return ext, str(zoned), pools, zones


def write_healthy(tmp_path):
    """write_zoned's file with every node healthy.  (An unhealthy node's zero row counts the
    pods without a node against 0 pod slots, CC:135: its zone's capacity goes negative and
    the skew then holds every zone below zero — tests/test_host_spread.py keeps one such
    run, the others use this file.)"""
    _, zoned, pools, zones = write_zoned(tmp_path)
    out = []
    for line in open(zoned).read().splitlines():
        f = line.split()
        if f and f[0] == "node":
            f[5:9] = ["False"] * 4
            line = " ".join(f)
        out.append(line)
    healthy = tmp_path / "healthy.txt"
    healthy.write_text("\n".join(out) + "\n")
    return str(healthy), pools, zones


def zone_lines(stdout):
    return [ln for ln in stdout.splitlines() if ln.startswith("Zone ")]


def model(rows, ax, ux, sc, sm, sx, gid, G, cap, skew):
    """(totals, err, the groups' capped cells) of one CLI run."""
    q, dz = xm.pair_table(rows, ax, ux, sc, sm, sx)
    S = len(sc)
    c = sp.capped_cells(q, dz, gid, G, [cap] * S)
    t, e, _ = sp.fold(c[0].reshape(G, S), c[1].reshape(G, S), c[3], None, G, None, [skew] * S)
    return t, e, c[0].reshape(G, S), c[1].reshape(G, S)


def want_zone_lines(order, cells, cerr, err, skew, s):
    lim = min(int(cells[:, s].min()) + skew, sp.I64_MAX)
    out = []
    for z, name in enumerate(order):
        cap = int(cells[z, s])
        used = PANIC if cerr[z, s] else ("-" if err[s] else min(cap, lim))
        out.append(f"Zone {name} : {used}" + ("" if cerr[z, s] else f" of {cap}"))
    return out


@pytest.mark.gpu
def test_cli_max_per_node_and_zone_spread(cli, tmp_path):  # noqa: F811
    zoned, pools, zones = write_healthy(tmp_path)
    rows = parse_expected(zoned)
    order = list(dict.fromkeys(zones))
    gid = [order.index(z) for z in zones]
    assert order[0] == "-" and sorted(order[1:]) == sorted(ZONES) and len(zones) == 60
    args = ["-cluster", zoned, "-cpuRequests=200m", "-memRequests=250mb", "-replicas=10"]
    sc, sm = [200], [262_144_000]
    base = _run(args)
    assert base.returncode == 0, base.stderr
    # at most k per node
    r = _run(args + ["-maxPerNode=3"])
    assert r.returncode == 0, r.stderr
    t, e, _, _ = model(rows, [], [], sc, sm, [], None, 1, 3, 0)
    assert e.tolist() == [0] and total_line(r.stdout) == [int(t[0])]
    assert 0 < int(t[0]) < total_line(base.stdout)[0] and not zone_lines(r.stdout)
    # zones with maxSkew 1 (the default), then with the per-node cap too
    for extra, k, skew in ((["-spreadBy", "zone"], 0, 1),
                           (["-spreadBy=zone", "-maxPerNode", "2"], 2, 1)):
        r = _run(args + extra)
        assert r.returncode == 0, r.stderr
        t, e, cells, cerr = model(rows, [], [], sc, sm, [], gid, len(order), k, skew)
        assert e.tolist() == [0] and total_line(r.stdout) == [int(t[0])]
        assert 0 < int(t[0]) < int(cells.sum())  # the skew binds
        assert ("So you can go ahead" if t[0] >= 10 else "Unfortunately") in r.stdout
        tail = r.stdout.splitlines()[-len(order) - 1:]
        assert set(tail[0]) == {"="}
        assert tail[1:] == want_zone_lines(order, cells, cerr, e, skew, 0)
    # a batch with a zero cpu request: its line and its zones panic
    specs = tmp_path / "specs.txt"
    specs.write_text("200m 250mb 10\n0.5 1G 3\n1 1G 3\n")
    r = _run(["-cluster", zoned, "-specs", str(specs), "-spreadBy=zone", "-maxSkew=2"])
    assert r.returncode == 0, r.stderr
    sc3, sm3 = [200, 0, 1000], [262_144_000, 1 << 30, 1 << 30]
    t, e, cells, cerr = model(rows, [], [], sc3, sm3, [], gid, len(order), 0, 2)
    assert e.tolist() == [0, 1, 0]
    heads, reps = ["200m 250mb 10", "0.5 1G 3", "1 1G 3"], [10, 3, 3]
    want = []
    for s, h in enumerate(heads):
        want.append(f"{h} panic: integer divide by zero" if e[s] else
                    f"{h} total={t[s]} {'yes' if t[s] >= reps[s] else 'no'}")
        want += want_zone_lines(order, cells, cerr, e, 2, s)
    assert r.stdout.strip().splitlines()[-len(want):] == want
    # unhealthy nodes: a zone's capacity is negative and the skew holds every zone below zero
    _, sick, _, _ = write_zoned(tmp_path)
    r = _run(["-cluster", sick, "-cpuRequests=200m", "-memRequests=250mb", "-spreadBy=zone"])
    assert r.returncode == 0, r.stderr
    t, e, cells, cerr = model(parse_expected(sick), [], [], sc, sm, [], gid, len(order), 0, 1)
    assert total_line(r.stdout) == [int(t[0])] and int(t[0]) < 0 < int(cells.max())
    assert zone_lines(r.stdout) == want_zone_lines(order, cells, cerr, e, 1, 0)


@pytest.mark.gpu
def test_cli_spread_with_pools_and_ext_requests(cli, tmp_path):  # noqa: F811
    zoned, pools, zones = write_healthy(tmp_path)
    rows = parse_expected(zoned)
    ax, ux = read_ext(zoned, [GPU, DISK])
    order = list(dict.fromkeys(zones))
    gid = [order.index(z) for z in zones]
    porder = list(dict.fromkeys(pools))
    pgid = [porder.index(p) for p in pools]
    sc, sm, sx = [200], [262_144_000], [[1], [20 << 30]]
    args = ["-cluster", zoned, "-cpuRequests=200m", "-memRequests=250mb", "-replicas=10"]
    extreq = f"-extRequests={GPU}=1,{DISK}=20Gi"
    # -extRequests and the zone spread
    r = _run(args + [extreq, "-spreadBy=zone", "-maxPerNode=2"])
    assert r.returncode == 0, r.stderr
    t, e, cells, cerr = model(rows, ax, ux, sc, sm, sx, gid, len(order), 2, 1)
    plain, _, _, _ = model(rows, [], [], sc, sm, [], gid, len(order), 2, 1)
    assert total_line(r.stdout) == [int(t[0])] and 0 < int(t[0]) < int(plain[0])
    assert zone_lines(r.stdout) == want_zone_lines(order, cells, cerr, e, 1, 0)
    # -byPool with -maxPerNode: the pools under the cap; with -spreadBy the zones come first
    for ext_args, (mx, mu, msx) in (([], ([], [], [])), ([extreq], (ax, ux, sx))):
        r = _run(args + ext_args + ["-byPool", "-maxPerNode=1", "-spreadBy=zone"])
        assert r.returncode == 0, r.stderr
        t, e, cells, cerr = model(rows, mx, mu, sc, sm, msx, gid, len(order), 1, 1)
        _, _, pcells, perr = model(rows, mx, mu, sc, sm, msx, pgid, len(porder), 1, 0)
        assert total_line(r.stdout) == [int(t[0])]
        tail = r.stdout.splitlines()[-len(order) - len(porder):]
        assert tail[:len(order)] == want_zone_lines(order, cells, cerr, e, 1, 0)
        assert tail[len(order):] == [f"Pool {p} : {pcells[g, 0]}" for g, p in enumerate(porder)]
        r0 = _run(args + ext_args + ["-byPool"])
        assert [ln for ln in r0.stdout.splitlines() if ln.startswith("Pool ")] != tail[len(order):]


@pytest.mark.gpu
def test_cli_zone_lines_change_nothing_without_the_flags(cli, tmp_path):  # noqa: F811
    ext, zoned, _, _ = write_zoned(tmp_path)
    specs = tmp_path / "specs.txt"
    specs.write_text("200m 250mb 10\n0.5 1G 3 trailing words\n")
    for args in (["-v"], ["-specs", str(specs)], ["-byPool", f"-extRequests={GPU}=1"],
                 ["-cpuRequests=0.5", "-maxPerNode=0", "-maxSkew=3"]):
        a = _run(["-cluster", ext] + [x for x in args if not x.startswith("-max")])
        b = _run(["-cluster", zoned] + args)
        assert a.returncode == b.returncode, args
        assert a.stdout.encode() == b.stdout.encode() and a.stderr == b.stderr, args
        assert "Zone " not in b.stdout
    for bad in (["-spreadBy=rack"], ["-maxSkew=0"], ["-maxPerNode=-1"], ["-maxPerNode=x"]):
        r = _run(["-cluster", zoned] + bad)
        assert r.returncode == 2 and r.stdout == "" and "invalid value" in r.stderr, bad
