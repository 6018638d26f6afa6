"""The CLI's extended resources (host/cluster_capacity.cpp): `resource <name> <allocatable>`
lines of a node, `request <name> <amount>` lines of a container, -extRequests and the
name=amount columns of a -specs file.  Totals, -byPool lines and -v's "Max replicas" come
from kcc_fit_ext and are checked against tests/ext_model.py over an independent reading of
the file; without a request for an extended resource the file prints byte for byte what
the same file without those lines prints."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import ext_model as xm
from tests import quantity_model as qm
from tests.test_host import _run, cli, parse_expected, write_cluster  # noqa: F401

GPU, DISK, HUGE = "amd.com/gpu", "ephemeral-storage", "hugepages-2Mi"
POOLS = ["gpu-a", "spot"]
PANIC = "panic: runtime error: integer divide by zero"


def write_ext(tmp_path):
    """The 60-node file of tests/test_host.py and a copy with pool, resource and request
    lines (and one init container whose request must not be read)."""
    plain = write_cluster(str(tmp_path / "plain.txt"))
    rng = np.random.default_rng(31)
    out, pools = [], []
    first_pod = True
    for line in open(plain).read().splitlines():
        out.append(line)
        if line.startswith("node "):
            pools.append(POOLS[len(pools) % 2] if len(pools) % 3 else "-")
            if pools[-1] != "-":
                out.append(f"pool {pools[-1]}")
            if rng.random() < 0.5:
                out.append(f"resource {GPU} {rng.choice(['8', '4', '8'])}")
            out.append(f"resource {DISK} {rng.choice(['500Gi', '1800G', '953869Mi', '100Gi'])}")
            if rng.random() < 0.3:
                out.append(f"resource {HUGE} {rng.choice(['1Gi', '512Mi'])}")
            out.append("resource example.com/unused 3")
        elif line.startswith("container "):
            if rng.random() < 0.15:
                out.append(f"request {GPU} {rng.choice(['1', '2'])}")
            if rng.random() < 0.6:
                out.append(f"request {DISK} {rng.choice(['2Gi', '500Mi', '10G', '1500M'])}")
            if rng.random() < 0.1:
                out.append(f"request {HUGE} 64Mi")
        elif line.startswith("pod ") and first_pod:
            first_pod = False
            out += ["initcontainer 100m 100m 0 0", f"request {GPU} 4", f"request {DISK} 700Gi"]
    ext = tmp_path / "ext.txt"
    ext.write_text("\n".join(out) + "\n")
    return plain, str(ext), pools


def read_ext(path, names):
    """alloc_x / used_x [R][N] from the file, read independently of the CLI: a node without
    a `resource` line has 0, an unhealthy node's zero row has 0 and sums the pods without a
    node; `request` lines count for app containers of pods the reference sums (CC:262-294)."""
    val = lambda s: qm.value(s)[0]  # noqa: E731
    nodes, pods, last = [], [], None
    for line in open(path):
        f = line.split()
        if not f:
            continue
        if f[0] == "node":
            nodes.append({"name": f[1], "healthy": all(c == "False" for c in f[5:9]), "res": {}})
        elif f[0] == "resource":
            nodes[-1]["res"][f[1]] = val(f[2])
        elif f[0] == "pod":
            pods.append({"node": "" if f[1] == "-" else f[1], "phase": f[4],
                         "missing": len(f) > 5 and f[5] == "missing", "c": []})
        elif f[0] in ("container", "initcontainer"):
            last = {"init": f[0] == "initcontainer", "req": {}}
            pods[-1]["c"].append(last)
        elif f[0] == "request":
            last["req"][f[1]] = val(f[2])
    ax = [[0] * len(nodes) for _ in names]
    ux = [[0] * len(nodes) for _ in names]
    for i, nd in enumerate(nodes):
        name = nd["name"] if nd["healthy"] else ""
        sel = [p for p in pods if p["node"] == name and p["phase"] not in
               ("Pending", "Succeeded", "Failed", "Unknown")]
        for r, res in enumerate(names):
            if nd["healthy"]:
                ax[r][i] = nd["res"].get(res, 0)
            for p in sel:
                if p["missing"]:
                    continue
                for c in p["c"]:
                    if not c["init"]:
                        ux[r][i] = pyoracle.i64(ux[r][i] + c["req"].get(res, 0))
    return ax, ux


def total_line(out):
    key = "Total possible replicas for the pod with required input specs : "
    return [int(ln.split(key)[1]) for ln in out.splitlines() if key in ln]


@pytest.mark.gpu
def test_cli_ext_one_spec_and_batch(cli, tmp_path):  # noqa: F811
    plain, ext, _ = write_ext(tmp_path)
    rows = parse_expected(ext)
    ax, ux = read_ext(ext, [GPU, DISK])
    assert any(ax[0]) and any(ux[0]) and any(ux[1]) and not all(ax[0])
    base, _ = pyoracle.fit(*rows, [200], [262_144_000])
    r = _run(["-cluster", ext, "-cpuRequests=200m", "-memRequests=250mb", "-replicas=10",
              f"-extRequests={GPU}=1,{DISK}=20Gi"])
    assert r.returncode == 0, r.stderr
    t, e = xm.fit_ext(rows, ax, ux, [200], [262_144_000], [[1], [20 << 30]])
    assert e.tolist() == [0] and total_line(r.stdout) == [int(t[0])] and int(t[0]) < base[0]
    assert ("So you can go ahead" if t[0] >= 10 else "Unfortunately") in r.stdout
    # separate-argument form, one resource; the resource nobody names is never read
    r = _run(["-cluster", ext, "-cpuRequests=200m", "-memRequests=250mb", "-extRequests",
              f"{DISK}=100Gi"])
    assert r.returncode == 0, r.stderr
    t, _ = xm.fit_ext(rows, ax[1:], ux[1:], [200], [262_144_000], [[100 << 30]])
    assert total_line(r.stdout) == [int(t[0])]
    # a batch: per-spec columns, resources in first-appearance order (disk, hugepages, gpu);
    # a spec that does not name a resource requests 0 of it; a zero cpu request still panics
    names = [DISK, HUGE, GPU]
    ax3, ux3 = read_ext(ext, names)
    specs = tmp_path / "specs.txt"
    specs.write_text(f"200m 250mb 10 {DISK}=20Gi\n"
                     "200m 250mb 10\n"
                     f"1 1G 3 {HUGE}=128Mi {GPU}=2  # two of them\n"
                     f"0.5 1G 3 {GPU}=1\n"
                     f"100m 100mb 1 {GPU}=8 {DISK}=1\n")
    r = _run(["-cluster", ext, "-specs", str(specs)])
    assert r.returncode == 0, r.stderr
    sc, sm = [200, 200, 1000, 0, 100], [262_144_000, 262_144_000, 1 << 30, 1 << 30, 104_857_600]
    sx = [[20 << 30, 0, 0, 0, 1], [0, 0, 128 << 20, 0, 0], [0, 0, 2, 1, 8]]
    t, e = xm.fit_ext(rows, ax3, ux3, sc, sm, sx)
    heads = ["200m 250mb 10", "200m 250mb 10", "1 1G 3", "0.5 1G 3", "100m 100mb 1"]
    reps = [10, 10, 3, 3, 1]
    want = [f"{h} panic: integer divide by zero" if e[s] else
            f"{h} total={t[s]} {'yes' if t[s] >= reps[s] else 'no'}" for s, h in enumerate(heads)]
    assert r.stdout.strip().splitlines()[-5:] == want
    assert e.tolist() == [0, 0, 0, 1, 0] and int(t[1]) == base[0] and len(set(t.tolist())) >= 4


@pytest.mark.gpu
def test_cli_ext_by_pool_and_verbose_rows(cli, tmp_path):  # noqa: F811
    plain, ext, pools = write_ext(tmp_path)
    rows = parse_expected(ext)
    ax, ux = read_ext(ext, [GPU, DISK])
    order = list(dict.fromkeys(pools))
    gid = [order.index(p) for p in pools]
    assert order[0] == "-" and sorted(order[1:]) == sorted(POOLS)
    specs = tmp_path / "specs.txt"
    specs.write_text(f"200m 250mb 10 {GPU}=1 {DISK}=20Gi\n0.5 1G 3 {GPU}=1\n1 1G 3 {DISK}=1Gi\n")
    r = _run(["-cluster", ext, "-specs", str(specs), "-byPool"])
    assert r.returncode == 0, r.stderr
    t, e = xm.fit_ext(rows, ax, ux, [200, 0, 1000], [262_144_000, 1 << 30, 1 << 30],
                      [[1, 1, 0], [20 << 30, 0, 1 << 30]], gid, len(order))
    want = [f"Pool {order[g]} : {PANIC if e[g, s] else t[g, s]}" for s in range(3)
            for g in range(len(order))]
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("Pool ")] == want
    assert e.any() and not e.all()
    # -v: one "Max replicas" per row, from one call with every row its own group
    r = _run(["-cluster", ext, "-cpuRequests=200m", "-memRequests=250mb", "-v",
              f"-extRequests={GPU}=1,{DISK}=20Gi"])
    assert r.returncode == 0, r.stderr
    q, dz = xm.pair_table(rows, ax, ux, [200], [262_144_000], [[1], [20 << 30]])
    assert not dz.any()
    got = [int(ln.split(":")[1]) for ln in r.stdout.splitlines() if ln.startswith("Max replicas :")]
    assert got == q[:, 0].tolist() and len(got) == 60
    q0, _ = xm.pair_table(rows, ax, ux, [200], [262_144_000], [[0], [0]])
    assert (q != q0).any()
    assert total_line(r.stdout) == [int(q[:, 0].sum())]


@pytest.mark.gpu
def test_cli_ext_lines_change_nothing_without_a_request(cli, tmp_path):  # noqa: F811
    plain, ext, _ = write_ext(tmp_path)
    nopool = tmp_path / "nopool.txt"  # (the pool lines alone are tests/test_host_pools.py's)
    nopool.write_text("".join(ln for ln in open(ext) if not ln.startswith(("resource ", "request "))))
    specs = tmp_path / "specs.txt"
    specs.write_text("200m 250mb 10\n0.5 1G 3 trailing words\n")
    for args in (["-cpuRequests=200m", "-memRequests=250mb"], ["-v"], ["-specs", str(specs)],
                 ["-cpuRequests=0.5"], ["-byPool"], ["-schedulerRequests"], ["-extRequests="]):
        a = _run(["-cluster", str(nopool)] + args)
        b = _run(["-cluster", ext] + args)
        assert a.returncode == b.returncode, args
        assert a.stdout.encode() == b.stdout.encode() and a.stderr == b.stderr, args


@pytest.mark.gpu
def test_cli_ext_load_errors(cli, tmp_path):  # noqa: F811
    plain, ext, _ = write_ext(tmp_path)
    # a string ParseQuantity rejects: in the flag, in a spec column, in the cluster file
    bad_spec = tmp_path / "bad_specs.txt"
    bad_spec.write_text(f"200m 250mb 10 {GPU}=1\n200m 250mb 10 {DISK}=10GiB\n")
    bad_file = tmp_path / "bad.txt"
    bad_file.write_text(open(ext).read().replace(f"resource {GPU} 8", f"resource {GPU} eight", 1))
    for args in (["-cluster", ext, f"-extRequests={GPU}=1x"],
                 ["-cluster", ext, "-specs", str(bad_spec)],
                 ["-cluster", str(bad_file), f"-extRequests={GPU}=1"],
                 # a fifth resource name
                 ["-cluster", ext, "-extRequests=a/a=1,b/b=1,c/c=1,d/d=1,e/e=1"]):
        r = _run(args)
        assert r.returncode == 1, (args, r.stdout, r.stderr)
        assert r.stdout == "" and r.stderr.strip(), args
    # the same bad cluster line is not read when nobody names the resource
    r = _run(["-cluster", str(bad_file), f"-extRequests={DISK}=1Gi"])
    assert r.returncode == 0, r.stderr
    # four names are fine
    r = _run(["-cluster", ext, f"-extRequests={GPU}=1,{DISK}=1Gi,{HUGE}=2Mi,example.com/unused=1"])
    assert r.returncode == 0, r.stderr
    rows = parse_expected(ext)
    names = [GPU, DISK, HUGE, "example.com/unused"]
    ax, ux = read_ext(ext, names)
    t, _ = xm.fit_ext(rows, ax, ux, [100], [104_857_600], [[1], [1 << 30], [2 << 20], [1]])
    assert total_line(r.stdout) == [int(t[0])]
