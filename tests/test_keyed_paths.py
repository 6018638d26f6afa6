"""The list-order (keyed) reduce's paths that tests/test_keyed.py reaches at one shape or not
at all (kcc_keyed.hip):

  - the gather's multi-part hand-off at every part count 1..4 and at the thresholds where the
    count changes, with empty, one-tile and uneven parts next to a skewed list;
  - the device-pointer entry points (kcc_reduce_requests_keyed_async, kcc_count_by_key_async)
    on a caller's stream, into caller-owned outputs of exactly n_keys elements, and their
    argument validation;
  - the atomic fallback with pod-like runs of equal keys and with limits
    (reduce_keyed_kernel<4>);
  - the workspace's exact fit: first calls on fresh engines (ensure() only grows buffers, so a
    long-lived engine hides a buffer sized one element short);
  - switches between the paths on one engine, workspace sizes going up and down.

Everything is checked bit for bit against the C oracle over the stably regrouped list
(tests/test_keyed.py oracle_keyed) and np.bincount for the counts."""
import numpy as np
import pytest

from kubernetesclustercapacity_amd import synth
from tests.test_keyed import list_order, oracle_keyed

pytestmark = pytest.mark.gpu

ROWS = 4096                 # rows per bucket (KB_ROWS)
TILE = 8192                 # containers per sweep tile (KB_SW_TILE)
NK_ATOMIC = 4096 * 4096 + 5  # more rows than the bucketed paths hold: device atomics
SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD = 512


def fresh_engine():
    from tests.conftest import init_torch_first
    init_torch_first()
    from kubernetesclustercapacity_amd import CapacityEngine
    return CapacityEngine(0, 1)


@pytest.fixture
def fresh():
    with fresh_engine() as e:
        yield e


def counts_of(nk, key):
    return np.bincount(key[(key >= 0) & (key < nk)], minlength=nk).astype(np.int64)


def quantities(rng, nc):
    """cpu: multiples of 50 m, 1 % at 2^40 (escapes); memory: MiB multiples, 1 % at 12345
    (escapes)."""
    cpu = (rng.integers(0, 41, nc) * 50).astype(np.uint64)
    cpu[rng.random(nc) < 0.01] = np.uint64(1 << 40)
    mem = rng.integers(0, 8192, nc).astype(np.int64) << 20
    mem[rng.random(nc) < 0.01] = 12345
    return cpu, mem


def full_range(rng, nc):
    """(cpu, mem, cpu_lim, mem_lim) over the whole uint64 / int64 range."""
    v = rng.integers(0, 1 << 64, (4, nc), dtype=np.uint64)
    return v[0], v[1].view(np.int64), v[2], v[3].view(np.int64)


def check_requests(eng, nk, key, cpu, mem, want, cl=None, ml=None):
    r = eng.get_pod_cpu_memory_requests_limits_keyed(nk, key, cpu, mem, cl, ml)
    assert np.array_equal(r.cpu_requests, want[0]) and np.array_equal(r.memory_requests, want[1])
    if cl is not None:
        assert np.array_equal(r.cpu_limits, want[2]) and np.array_equal(r.memory_limits, want[3])


# ---- B1: gather parts 1..4 at their thresholds ----------------------------------------------

def device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def parts_of(cus, ng):
    """keyed_sweep_parts restated: gather workgroups per bucket group."""
    return min(4, max(1, cus // ng))


# bucket-group counts on each side of every threshold of parts_of (256 CUs: 64, 65, 85, 86,
# 128, 129 -> 4, 3, 3, 2, 2, 1 parts)
NG_AT = {"cus//4": lambda c: c // 4, "cus//4+1": lambda c: c // 4 + 1,
         "cus//3": lambda c: c // 3, "cus//3+1": lambda c: c // 3 + 1,
         "cus//2": lambda c: c // 2, "cus//2+1": lambda c: c // 2 + 1}


@pytest.fixture(scope="module")
def parts_eng():
    """One fresh engine for the whole parts parametrization."""
    with fresh_engine() as e:
        yield e


def test_gather_parts_cover_1_to_4(parts_eng):
    """The thresholds below run every part count on this device (another CU count must not
    shift the coverage silently)."""
    cus = device_cus()
    got = {parts_of(cus, f(cus)) for f in NG_AT.values()}
    print(f"CUs: {cus}; bucket groups {[f(cus) for f in NG_AT.values()]} -> parts {sorted(got)}")
    assert got == {1, 2, 3, 4}, (cus, got)
    assert parts_eng.reduce_faults() == 0


def parts_keys(rng, nk, nc, hot):
    key = rng.integers(0, nk, nc).astype(np.int32)
    u = rng.random(nc)
    sel = u < 0.30
    key[sel] = rng.choice(np.array(hot, np.int32), int(sel.sum()))
    sel = (u >= 0.30) & (u < 0.32)
    key[sel] = rng.choice(np.array([-1, nk, -(2 ** 31)], np.int64), int(sel.sum())).astype(np.int32)
    return key


@pytest.mark.parametrize("odd", [0, 1], ids=["nb=2ng", "nb=2ng-1"])
@pytest.mark.parametrize("at", list(NG_AT))
def test_gather_parts_thresholds(parts_eng, at, odd):
    """Each part count at both sides of its threshold, the last group a pair of buckets or a
    single one, over tile counts G in {1, p - 1, p, p + 1, 2p + 1}: parts without a tile,
    with one tile, and uneven parts; hot rows on both sides of a group's split and at the
    last row, off-row keys, escapes.  A call with other data comes first (stale part_acc
    rows, arrive / ready counts left behind would show), then the checked call three times
    (which part arrives last is not controlled), then the counts (NA = 0)."""
    eng = parts_eng
    cus = device_cus()
    ng = NG_AT[at](cus)
    assert ng >= 2, cus
    p = parts_of(cus, ng)
    nb = 2 * ng - odd
    nk = (nb - 1) * ROWS + 1 + (37 * nb) % ROWS  # nb buckets, the last one partial
    assert (nk + ROWS - 1) // ROWS == nb and (nb + 1) // 2 == ng
    gi = (ng - 1) // 2  # a group of two buckets (never the last one)
    hot = [2 * gi * ROWS + 7, (2 * gi + 1) * ROWS + ROWS - 1, nk - 1]
    sizes = {5000: 1, TILE * p: p, TILE * p + 1: p + 1, TILE * (2 * p + 1) - 3: 2 * p + 1}
    if p > 1:
        sizes[TILE * (p - 2) + 17] = p - 1
    rng = np.random.default_rng([cus, ng, odd])
    nc0 = TILE * (p + 1) + 1  # the call before: every part holds rows
    k0 = parts_keys(rng, nk, nc0, hot)
    c0, m0 = quantities(rng, nc0)
    want0 = oracle_keyed(nk, k0, c0, m0)
    for nc, G in sorted(sizes.items()):
        assert (nc + TILE - 1) // TILE == G and nc <= TILE * cus
        key = parts_keys(rng, nk, nc, hot)
        cpu, mem = quantities(rng, nc)
        want = oracle_keyed(nk, key, cpu, mem)
        check_requests(eng, nk, k0, c0, m0, want0)
        for _ in range(3):
            check_requests(eng, nk, key, cpu, mem, want)
        assert np.array_equal(eng.count_by_key(nk, key), counts_of(nk, key))
    assert eng.reduce_faults() == 0


# ---- B2: the device-pointer entry points ----------------------------------------------------

def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to("cuda:0")


class Guarded:
    """An output of exactly nk int64 inside a sentinel-filled tensor of nk + 2 * GUARD."""

    def __init__(self, nk):
        import torch
        self.nk = nk
        self.whole = torch.full((nk + 2 * GUARD,), SENTINEL, dtype=torch.int64, device="cuda:0")
        self.out = self.whole[GUARD:GUARD + nk]

    def guards_intact(self):
        w = self.whole
        return bool((w[:GUARD] == SENTINEL).all()) and bool((w[GUARD + self.nk:] == SENTINEL).all())

    def untouched(self):
        return bool((self.whole == SENTINEL).all())

    def host(self, dtype=np.int64):
        return self.out.cpu().numpy().view(dtype)


def device_case(eng, nk, key, cpu, mem, cl=None, ml=None):
    """One list through the device entry points on a side stream == the oracle == the
    host-array entry points; guards intact."""
    import torch
    lim = cl is not None
    want = oracle_keyed(nk, key, cpu, mem, cl, ml)
    host = eng.get_pod_cpu_memory_requests_limits_keyed(nk, key, cpu, mem, cl, ml)
    host_count = eng.count_by_key(nk, key)
    d_key, d_cpu, d_mem = _dev(key), _dev(cpu), _dev(mem)
    d_cl, d_ml = (_dev(cl), _dev(ml)) if lim else (None, None)
    outs = [Guarded(nk) for _ in range(4 if lim else 2)]
    cnt = Guarded(nk)
    s = torch.cuda.Stream(device=0)
    s.wait_stream(torch.cuda.current_stream())  # (the uploads and fills above)
    eng.reduce_requests_keyed_async(nk, d_key, d_cpu, d_mem, outs[0].out, outs[1].out, stream=s,
                                    cpu_lim=d_cl, mem_lim=d_ml,
                                    lim_cpu=outs[2].out if lim else None,
                                    lim_mem=outs[3].out if lim else None)
    eng.count_by_key_async(nk, d_key, cnt.out, stream=s)
    s.synchronize()
    got = [outs[0].host(np.uint64), outs[1].host()]
    ref = [host.cpu_requests, host.memory_requests]
    if lim:
        got += [outs[2].host(np.uint64), outs[3].host()]
        ref += [host.cpu_limits, host.memory_limits]
    for g, w, h in zip(got, want, ref):
        assert np.array_equal(g, w) and np.array_equal(g, h)
    assert all(o.guards_intact() for o in outs) and cnt.guards_intact()
    c = counts_of(nk, key)
    assert np.array_equal(cnt.host(), c) and np.array_equal(host_count, c)
    assert eng.reduce_faults() == 0


def device_list(nk, nc, seed, lim):
    rng = np.random.default_rng([nk % 65521, nc, seed])
    key = rng.integers(-1, nk + 1, nc).astype(np.int32)  # off-row keys at both ends
    if nc:
        key[rng.random(nc) < 0.2] = nk - 1
    cpu, mem = quantities(rng, nc)
    cl, ml = full_range(rng, nc)[2:] if lim else (None, None)
    return key, cpu, mem, cl, ml


DEV_NK = [1, 4095, 4097, 3 * 4096 + 5]


@pytest.mark.parametrize("nc", [0, 3, 8191, 20_000])
@pytest.mark.parametrize("nk", DEV_NK)
def test_device_api_sweep(engine, nk, nc):
    """One sweep (requests without limits) and the counts: rows without containers come back
    0, not the outputs' fill."""
    device_case(engine, nk, *device_list(nk, nc, 1, False))


@pytest.mark.parametrize("nk", DEV_NK)
def test_device_api_bucketed_limits(engine, nk):
    device_case(engine, nk, *device_list(nk, 20_000, 2, True))


@pytest.mark.parametrize("lim", [False, True], ids=["requests", "limits"])
def test_device_api_atomic_fallback(engine, lim):
    nk = NK_ATOMIC
    key, _, _, cl, ml = device_list(nk, 50_001, 3, lim)
    key[:6] = [nk - 1, nk - 1, 0, 0, nk, -1]
    cpu, mem = full_range(np.random.default_rng(33), key.size)[:2]
    device_case(engine, nk, key, cpu, mem, cl, ml)


def test_device_api_validation(engine):
    """Every rejected call returns KCC_EINVAL and touches no output."""
    import torch
    from kubernetesclustercapacity_amd import _lib
    from kubernetesclustercapacity_amd.engine import KccError
    eng = engine
    nk, nc = 100, 64
    key, cpu, mem, cl, ml = device_list(nk, nc, 4, True)
    d_key, d_cpu, d_mem, d_cl, d_ml = (_dev(x) for x in (key, cpu, mem, cl, ml))
    uc, um, lc, lm, cnt = (Guarded(nk) for _ in range(5))
    s = torch.cuda.Stream(device=0)
    s.wait_stream(torch.cuda.current_stream())

    def reduce_(n_keys=nk, n=nc, k=d_key, c=d_cpu, m=d_mem, o0=uc.out, o1=um.out, **kw):
        eng.reduce_requests_keyed_async(n_keys, k, c, m, o0, o1, stream=s, n=n, **kw)

    def count_(n_keys=nk, n=nc, k=d_key, o=cnt.out):
        eng.count_by_key_async(n_keys, k, o, stream=s, n=n)

    lims = dict(cpu_lim=d_cl, mem_lim=d_ml, lim_cpu=lc.out, lim_mem=lm.out)
    bad = {
        "negative n_keys": lambda: reduce_(n_keys=-1),
        "negative n": lambda: reduce_(n=-1),
        "2^31 keys": lambda: reduce_(n_keys=2 ** 31, n=0),
        "NULL used_cpu": lambda: reduce_(o0=None),
        "NULL used_mem": lambda: reduce_(o1=None),
        "NULL key": lambda: reduce_(k=None),
        "cpu_lim alone": lambda: reduce_(**{**lims, "mem_lim": None}),
        "mem_lim alone": lambda: reduce_(**{**lims, "cpu_lim": None}),
        "limits without lim_cpu": lambda: reduce_(**{**lims, "lim_cpu": None}),
        "key off by one": lambda: reduce_(n=nc - 1, k=d_key[1:]),
        "cpu_req off by one": lambda: reduce_(n=nc - 1, c=d_cpu[1:]),
        "mem_req off by one": lambda: reduce_(n=nc - 1, m=d_mem[1:]),
        "cpu_lim off by one": lambda: reduce_(n=nc - 1, **{**lims, "cpu_lim": d_cl[1:]}),
        "count: negative n_keys": lambda: count_(n_keys=-1),
        "count: negative n": lambda: count_(n=-1),
        "count: 2^31 keys": lambda: count_(n_keys=2 ** 31, n=0),
        "count: NULL count": lambda: count_(o=None),
        "count: NULL key": lambda: count_(k=None),
        "count: key off by one": lambda: count_(n=nc - 1, k=d_key[1:]),
    }
    for what, call in bad.items():
        with pytest.raises(KccError) as ei:
            call()
        assert ei.value.code == _lib.KCC_EINVAL, what
    s.synchronize()
    torch.cuda.synchronize()
    assert all(g.untouched() for g in (uc, um, lc, lm, cnt))
    # the same arguments, valid: accepted and right
    reduce_(**lims)
    count_()
    s.synchronize()
    want = oracle_keyed(nk, key, cpu, mem, cl, ml)
    for g, w in zip((uc, um, lc, lm), want):
        assert np.array_equal(g.host(w.dtype), w) and g.guards_intact()
    assert np.array_equal(cnt.host(), counts_of(nk, key))
    assert eng.reduce_faults() == 0


# ---- B3: the atomic fallback with pod-like runs, with and without limits ----------------------

@pytest.fixture(scope="module")
def pod_runs():
    """40_003 containers in runs of 1-6 equal keys (a pod's containers are consecutive in a
    List; the run lengths are drawn per pod): 10 % of the runs off the rows (-1 or nk), 10 %
    each on rows 0 and nk - 1, the rest uniform; full-range values in all four arrays."""
    nk, nc = NK_ATOMIC, 40_003
    rng = np.random.default_rng(20)
    lens = rng.integers(1, 7, nc)  # (more runs than needed: cut below)
    rk = rng.integers(0, nk, nc).astype(np.int64)
    u = rng.random(nc)
    rk[u < 0.10] = rng.choice(np.array([-1, nk]), int((u < 0.10).sum()))
    rk[(u >= 0.10) & (u < 0.20)] = 0
    rk[(u >= 0.20) & (u < 0.30)] = nk - 1
    key = np.repeat(rk, lens)[:nc].astype(np.int32)
    assert key.size == nc
    runs = np.diff(np.flatnonzero(np.r_[True, key[1:] != key[:-1], True]))
    assert set(range(1, 7)) <= set(runs.tolist())  # every run length, some longer (merged)
    return (key,) + full_range(rng, nc)


@pytest.mark.parametrize("nc", [40_000, 40_001, 40_002, 40_003])
def test_atomic_fallback_pod_runs(engine, pod_runs, nc):
    """reduce_keyed_kernel<2> and count_keyed_kernel: runs of 1-6 equal keys (off-row runs
    included) crossing the lanes' quads, and every n % 4 (the last quad's scalar path)."""
    nk = NK_ATOMIC
    key, cpu, mem = (a[:nc] for a in pod_runs[:3])
    check_requests(engine, nk, key, cpu, mem, oracle_keyed(nk, key, cpu, mem))
    assert np.array_equal(engine.count_by_key(nk, key), counts_of(nk, key))
    assert engine.reduce_faults() == 0


def test_atomic_fallback_pod_runs_limits(engine, pod_runs):
    """reduce_keyed_kernel<4>: the same runs with limits, n % 4 == 3."""
    nk = NK_ATOMIC
    key, cpu, mem, cl, ml = pod_runs
    assert key.size % 4 == 3
    check_requests(engine, nk, key, cpu, mem, oracle_keyed(nk, key, cpu, mem, cl, ml), cl, ml)
    assert engine.reduce_faults() == 0


# ---- B4: the staging buffer's exact fit, first call on a fresh engine ---------------------------

@pytest.mark.parametrize("m,bucket", [(1, 0), (2, 0), (32, 0), (2, 2)])
def test_exact_fit_first_call(fresh, m, bucket):
    """n = 8192 m containers (full tiles, the last one too), every key valid and inside one
    of 3 buckets: the other groups' segments are empty, and the empty segments past the
    last tile's records start at the end of the staging buffer's last region — the slot the
    buffer's one-line pad holds (kcc_keyed.hip keyed_sr_slots).  The engine's first keyed
    call, so every workspace buffer has exactly this call's size (m = 32: a staging buffer
    of 2 MiB plus the pad)."""
    nk, n = 3 * ROWS, TILE * m
    rng = np.random.default_rng([m, bucket])
    key = (bucket * ROWS + rng.integers(0, ROWS, n)).astype(np.int32)
    cpu, mem = quantities(rng, n)
    check_requests(fresh, nk, key, cpu, mem, oracle_keyed(nk, key, cpu, mem))
    assert np.array_equal(fresh.count_by_key(nk, key), counts_of(nk, key))
    assert fresh.reduce_faults() == 0


def test_exact_fit_first_call_counts(fresh):
    """The same shape with the counts (NA = 0) as the engine's first keyed call."""
    nk, n = 3 * ROWS, TILE * 2
    key = np.random.default_rng(7).integers(0, ROWS, n).astype(np.int32)
    assert np.array_equal(fresh.count_by_key(nk, key), counts_of(nk, key))
    assert fresh.reduce_faults() == 0


# ---- B5: path switches on one fresh engine ----------------------------------------------------

def test_path_switching(fresh):
    """Sweep, counts, bucketed, sweep, atomics, sweep, sweep on one engine: the bucket count,
    the parts, the arrive / ready split and the workspace sizes change upwards and
    downwards between the calls."""
    eng = fresh
    rng = np.random.default_rng(50)
    # 1. a sweep with escapes (adversarial cluster in list order, off-row pods)
    nk1 = 300_000
    c = synth.make_cluster(nk1, 60_000, seed=5, chunk=4096, adversarial=True)
    k1, c1, m1, *_ = list_order(c, 6, 0.05)
    k1, c1, m1 = k1[:100_000].copy(), c1[:100_000].copy(), m1[:100_000].copy()
    assert (c1 >> np.uint64(20)).any() and (m1 % 64 != 0).any()  # escapes of both kinds
    w1 = oracle_keyed(nk1, k1, c1, m1)
    check_requests(eng, nk1, k1, c1, m1, w1)
    # 2. counts
    k = rng.integers(-1, 6, 70_001).astype(np.int32)
    assert np.array_equal(eng.count_by_key(5, k), counts_of(5, k))
    # 3. bucketed, with limits
    nk, nc = 40_000, 90_003
    k = rng.integers(-1, nk + 1, nc).astype(np.int32)
    cpu, mem, cl, ml = full_range(rng, nc)
    check_requests(eng, nk, k, cpu, mem, oracle_keyed(nk, k, cpu, mem, cl, ml), cl, ml)
    # 4. a sweep without any escape (171 buckets, 86 groups: two parts on 256 CUs)
    nk, nc = 700_000, 100_000
    k = rng.integers(0, nk, nc).astype(np.int32)
    k[rng.random(nc) < 0.3] = nk - 1
    cpu = (rng.integers(0, 41, nc) * 50).astype(np.uint64)
    mem = rng.integers(0, 8192, nc).astype(np.int64) << 20
    check_requests(eng, nk, k, cpu, mem, oracle_keyed(nk, k, cpu, mem))
    # 5. the atomic fallback
    nk, nc = NK_ATOMIC, 50_002
    k = rng.integers(-1, nk + 1, nc).astype(np.int32)
    k[:4] = [nk - 1, nk - 1, 0, 0]
    cpu, mem = full_range(rng, nc)[:2]
    check_requests(eng, nk, k, cpu, mem, oracle_keyed(nk, k, cpu, mem))
    # 6. the smallest sweep
    one = (np.zeros(1, np.int32), np.array([(1 << 40) + 3], np.uint64), np.array([77], np.int64))
    check_requests(eng, 1, *one, oracle_keyed(1, *one))
    # 7. call 1 again
    check_requests(eng, nk1, k1, c1, m1, w1)
    assert eng.reduce_faults() == 0
