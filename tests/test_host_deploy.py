"""The CLI's rollout plan (host/cluster_capacity.cpp -deploy <file>): the steps run through
kcc_deploy before every fit, in file order; the "Deployed" lines, the total after the plan,
-specs, -byPool and -spreadBy zone after the plan are checked against tests/deploy_model.py
and the fits' models over an independent reading of the cluster file.  A flagged step prints
the reference's panic line and exits with status 2; a plan without steps prints byte for byte
what no plan prints."""
import numpy as np
import pytest

from tests import deploy_model as dm
from tests import ext_model as xm
from tests.test_host import _run, cli, parse_expected  # noqa: F401
from tests.test_host_ext import DISK, GPU, PANIC, read_ext, total_line
from tests.test_host_spread import model, want_zone_lines, write_healthy, zone_lines

MB = 1 << 20
# (cpu string, millicores, memory string, bytes, replicas, policy, perNode, {name: (string, value)})
STEPS = [("500m", 500, "1G", 1 << 30, 40, dm.PACK, 0, {GPU: ("1", 1)}),
         ("200m", 200, "250mb", 250 * MB, 25, dm.SPREAD, 2, {}),
         ("100m", 100, "100mb", 100 * MB, 300, dm.SPREAD, 0, {}),
         ("1", 1000, "2G", 2 << 30, 100000, dm.PACK, 0, {DISK: ("5Gi", 5 << 30)})]


def write_plan(path, steps=STEPS):
    lines = ["# Friday's rollout"]
    for k, (cs, _, ms, _, rep, pol, per, ext) in enumerate(steps):
        toks = [cs, ms, str(rep)]
        if pol == dm.SPREAD:
            toks.append("spread")
        elif k > 0:
            toks.append("pack")  # (the default, spelled out on the later lines)
        if per:
            toks.append(f"perNode:{per}")
        toks += [f"{name}={s}" for name, (s, _) in ext.items()]
        lines.append(" ".join(toks) + "   # a comment")
    path.write_text("\n".join(lines) + "\n\n")
    return str(path)


def after_plan(rows, ax, ux, steps=STEPS):
    """The model's state after the plan, one step a call, and the "Deployed" lines."""
    rows, ux, lines = list(rows), np.array(ux, np.int64), []
    for cs, c, ms, m, rep, pol, per, ext in steps:
        sx = [[ext.get(GPU, (0, 0))[1]], [ext.get(DISK, (0, 0))[1]]]
        r = dm.deploy(rows, ax, ux, [c], [m], sx, [rep], pol, [per])
        assert r.err[0] == 0
        lines.append(f"Deployed {cs} {ms} {rep} : {r.placed[0]} on {r.nodes_used[0]} nodes")
        rows, ux = rows[:3] + [r.pod_count, r.used_cpu, r.used_mem], r.used_x
    return rows, ux, lines


@pytest.mark.gpu
def test_cli_deploy_then_every_fit(cli, tmp_path):  # noqa: F811
    path, pools, zones = write_healthy(tmp_path)
    rows0 = parse_expected(path)
    ax, ux0 = read_ext(path, [GPU, DISK])
    plan = write_plan(tmp_path / "plan.txt")
    rows, ux, deployed = after_plan(rows0, ax, ux0)
    placed = [int(ln.split(" : ")[1].split()[0]) for ln in deployed]
    assert placed[0] == 40 and placed[1] == 25 and placed[2] == 300 and 0 < placed[3] < 100000
    args = ["-cluster", path, "-cpuRequests=200m", "-memRequests=250mb", "-replicas=10"]
    sc, sm, none = [200], [250 * MB], [[0], [0]]
    # the Deployed lines follow the echo line; the total comes from the state after the plan
    r = _run(args + ["-deploy", plan])
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    echo = [i for i, ln in enumerate(out) if ln.startswith("CPU limits, requests")]
    first = out.index(deployed[0])  # (the node listing's own prints come in between, CC:99)
    total = [i for i, ln in enumerate(out) if "Total possible replicas" in ln]
    assert len(echo) == 1 and echo[0] < first and out[first:first + len(STEPS)] == deployed
    assert len(total) == 1 and first + len(STEPS) < total[0]
    t, e = xm.fit_ext(rows, ax, ux, sc, sm, none)
    assert e.tolist() == [0] and total_line(r.stdout) == [int(t[0])]
    t0, _ = xm.fit_ext(rows0, ax, ux0, sc, sm, none)
    assert int(t[0]) < int(t0[0])  # (what the same cluster holds without the plan)
    # -byPool and -spreadBy zone after the plan, under a per-node cap, with an extended request
    order, porder = list(dict.fromkeys(zones)), list(dict.fromkeys(pools))
    gid, pgid = [order.index(z) for z in zones], [porder.index(p) for p in pools]
    for extra, sx, cap in (([], none, 0), ([f"-extRequests={GPU}=1", "-maxPerNode=3"], [[1], [0]], 3)):
        r = _run(args + extra + ["-deploy=" + plan, "-byPool", "-spreadBy=zone"])
        assert r.returncode == 0, r.stderr
        t, e, cells, cerr = model(rows, ax, ux, sc, sm, sx, gid, len(order), cap, 1)
        _, _, pcells, _ = model(rows, ax, ux, sc, sm, sx, pgid, len(porder), cap, 0)
        assert total_line(r.stdout) == [int(t[0])]
        assert zone_lines(r.stdout) == want_zone_lines(order, cells, cerr, e, 1, 0)
        assert [ln for ln in r.stdout.splitlines() if ln.startswith("Pool ")] == \
            [f"Pool {p} : {pcells[g, 0]}" for g, p in enumerate(porder)]
        assert [ln for ln in r.stdout.splitlines() if ln.startswith("Deployed ")] == deployed
        t0, _, _, _ = model(rows0, ax, ux0, sc, sm, sx, gid, len(order), cap, 1)
        assert int(t0[0]) != int(t[0])  # the plan changed the numbers
    # a batch of specs after the plan
    specs = tmp_path / "specs.txt"
    specs.write_text(f"200m 250mb 10\n1 1G 3 {DISK}=1Gi\n50m 10mb 5000\n")
    r = _run(["-cluster", path, "-specs", str(specs), "-deploy", plan])
    assert r.returncode == 0, r.stderr
    t, e = xm.fit_ext(rows, ax, ux, [200, 1000, 50], [250 * MB, 1 << 30, 10 * MB],
                      [[0, 0, 0], [0, 1 << 30, 0]])
    heads, reps = ["200m 250mb 10", "1 1G 3", "50m 10mb 5000"], [10, 3, 5000]
    assert e.tolist() == [0, 0, 0]
    assert r.stdout.strip().splitlines()[-3:] == \
        [f"{h} total={t[s]} {'yes' if t[s] >= reps[s] else 'no'}" for s, h in enumerate(heads)]


@pytest.mark.gpu
def test_cli_deploy_flagged_step(cli, tmp_path):  # noqa: F811
    path, _, _ = write_healthy(tmp_path)
    rows0 = parse_expected(path)
    ax, ux0 = read_ext(path, [GPU, DISK])
    # the second step asks for 0 millicores: Go panics on a node with free CPU
    bad = tmp_path / "bad.txt"
    bad.write_text("500m 1G 40\n0 100mb 5 spread\n100m 100mb 7\n")
    r = _run(["-cluster", path, "-deploy", str(bad)])
    _, _, deployed = after_plan(rows0, ax, ux0, [("500m", 500, "1G", 1 << 30, 40, dm.PACK, 0, {})])
    assert r.returncode == 2 and r.stderr.strip().splitlines()[-1] == PANIC
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("Deployed ")] == deployed
    assert "Total possible replicas" not in r.stdout


@pytest.mark.gpu
def test_cli_plan_without_steps_changes_nothing(cli, tmp_path):  # noqa: F811
    """Every fit then reads explicit sums (kcc_fit / kcc_fit_ext instead of kcc_capacity) and
    prints byte for byte what no plan prints."""
    path, _, _ = write_healthy(tmp_path)
    empty = tmp_path / "empty.txt"
    empty.write_text("# nothing this week\n\n")
    specs = tmp_path / "specs.txt"
    specs.write_text("200m 250mb 10\n0.5 1G 3 trailing words\n")
    for args in (["-specs", str(specs)],
                 ["-byPool", f"-extRequests={GPU}=1", "-spreadBy=zone", "-maxPerNode=2"]):
        a = _run(["-cluster", path] + args)
        b = _run(["-cluster", path, "-deploy", str(empty)] + args)
        assert a.returncode == b.returncode, (args, a.stderr, b.stderr)
        assert a.stdout.encode() == b.stdout.encode() and a.stderr == b.stderr, args
        assert "Deployed" not in b.stdout
