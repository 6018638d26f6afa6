#!/usr/bin/env python3
"""The extended-resource fit against the grouped fit it is built on.

Arms in one process, alternating after a warm-up, each timed with device events around
work that ends in a synchronise:
  (a)   kcc_fit_grouped_async with G = 1 (every row in group 0): the pair loop the ext
        fit extends, with its three sort launches;
  (b_R) kcc_fit_ext_async without group ids at R = 0, 1, 2, 4 extra resources;
  (fit) kcc_fit_async, the two-resource engine the README row compares with.
Before timing, outputs are compared cell by cell: (b_0) against (a) and (fit), and every
(b_R) run once with all-zero requests against (a) (a resource nobody requests changes
nothing).  Rows are synth's C3 (100k nodes x 256 specs) and C4 (1M x 4096); the extra
columns are a device count (8 on a quarter of the nodes), storage, hugepages and a second
device count.  Prints one JSON line per case; --out appends them to a file.

  python scripts/bench_ext.py --cases C3,C4 --out profiles/ext_bench.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GIB = 1 << 30
RS = (0, 1, 2, 4)


def stats(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]),
                p25_ms=float(np.percentile(a, 25)), p75_ms=float(np.percentile(a, 75)),
                spread_ms=float(a[-1] - a[0]), reps=int(a.size))


def extra_columns(n, S, seed):
    """alloc_x / used_x [4, n] and spec_x [4, S]: every row and every spec stays fast."""
    rng = np.random.default_rng([seed, n, S])
    ax = np.zeros((4, n), np.int64)
    ux = np.zeros((4, n), np.int64)
    ax[0] = np.where(rng.random(n) < 0.25, 8, 0)
    ux[0] = rng.integers(0, 9, n)
    ax[1] = rng.integers(50, 2001, n) * GIB
    ux[1] = (ax[1] * rng.random(n)).astype(np.int64)
    ax[2] = rng.choice(np.array([0, 1, 4, 16]), n) * GIB
    ux[2] = (ax[2] * rng.random(n)).astype(np.int64)
    ax[3] = np.where(rng.random(n) < 0.5, 4, 0)
    ux[3] = rng.integers(0, 5, n)
    sx = np.zeros((4, S), np.int64)
    sx[0] = rng.choice(np.array([0, 0, 1, 2, 4, 8]), S)
    sx[1] = np.where(rng.random(S) < 0.3, 0, rng.integers(1, 50, S) * GIB)
    sx[2] = np.where(rng.random(S) < 0.7, 0, rng.integers(1, 9, S) * (GIB // 4))
    sx[3] = rng.choice(np.array([0, 0, 0, 1, 2]), S)
    return ax, ux, sx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="C3,C4")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["all", "b"], default="all",
                    help="b: the ext arms alone, no comparison (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    torch.cuda.init()
    from kubernetesclustercapacity_amd import CapacityEngine, synth
    dev = torch.device("cuda", 0)

    def T(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)

    eng = CapacityEngine(0, 1)
    for name in args.cases.split(","):
        t0 = time.time()
        c = synth.config_cluster(name, limits=False)
        r = eng.get_pod_cpu_memory_requests_limits(c.node_ptr, c.cpu_req, c.mem_req)
        sc, sm = synth.config_specs(name)
        rows = [c.alloc_cpu, c.alloc_mem, c.alloc_pods, c.pod_count, r.cpu_requests,
                r.memory_requests]
        n, S = rows[0].size, sc.size
        ax, ux, sx = extra_columns(n, S, 20261015)
        print(f"# {name}: {n} nodes, {S} specs generated in {time.time() - t0:.1f} s", flush=True)
        d_rows, d_sc, d_sm = [T(a) for a in rows], T(sc), T(sm)
        d_gid = torch.zeros(n, dtype=torch.int32, device=dev)
        d_x = {R: (T(ax[:R]), T(ux[:R]), T(sx[:R]), torch.zeros(max(R, 1) * S, dtype=torch.int64,
                                                               device=dev)) for R in RS}
        out = {k: (torch.empty(S, dtype=torch.int64, device=dev),
                   torch.empty(S, dtype=torch.int32, device=dev))
               for k in ["grouped_g1", "fit"] + [f"ext_r{R}" for R in RS]}
        stream = torch.cuda.Stream(dev)

        def arm_a():
            eng.fit_grouped_async(*d_rows, d_gid, 1, d_sc, d_sm, *out["grouped_g1"], stream=stream)

        def arm_fit():
            eng._check(eng._lib.kcc_fit_async(
                eng._h, n, *[x.data_ptr() for x in d_rows], S, d_sc.data_ptr(), d_sm.data_ptr(),
                out["fit"][0].data_ptr(), out["fit"][1].data_ptr(), stream.cuda_stream))

        def arm_b(R, zero=False):
            a_x, u_x, s_x, z_x = d_x[R]
            eng.fit_ext_async(*d_rows, R, a_x, u_x, None, 1, d_sc, d_sm, z_x if zero else s_x,
                              *out[f"ext_r{R}"], stream=stream)

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b)

        arms = [(f"ext_r{R}", (lambda R=R: arm_b(R))) for R in RS]
        if args.only == "all":
            arms = [("grouped_g1", arm_a)] + arms + [("fit", arm_fit)]
        host = lambda k: (out[k][0].cpu().numpy().copy(), out[k][1].cpu().numpy().copy())  # noqa: E731
        equal = None
        if args.only == "all":
            timed(arm_a)
            timed(arm_fit)
            ref, fit = host("grouped_g1"), host("fit")
            equal = bool(np.array_equal(ref[0], fit[0]) and np.array_equal(ref[1], fit[1]))
            for R in RS:
                timed(lambda R=R: arm_b(R, zero=True))
                got = host(f"ext_r{R}")
                equal = equal and bool(np.array_equal(got[0], ref[0]) and
                                       np.array_equal(got[1], ref[1]))
            if not equal:
                print(json.dumps(dict(case=name, error="the arms' outputs differ")))
                sys.exit(1)
        for _ in range(args.warmup):
            for _, fn in arms:
                timed(fn)
        changed = None
        if args.only == "all":
            ref = host("grouped_g1")
            changed = {f"ext_r{R}": int((host(f"ext_r{R}")[0] != ref[0]).sum()) for R in RS}
        ms = {k: [] for k, _ in arms}
        for _ in range(args.reps):
            for k, fn in arms:
                ms[k].append(timed(fn))
        res = dict(case=name, n_nodes=int(n), n_specs=int(S), outputs_equal=equal,
                   specs_changed_by_requests=changed, device=torch.cuda.get_device_name(0),
                   **{k: stats(v) for k, v in ms.items()})
        med = {k: res[k]["median_ms"] for k in ms}
        res["ms_per_added_resource"] = {
            f"r{a}_to_r{b}": (med[f"ext_r{b}"] - med[f"ext_r{a}"]) / (b - a)
            for a, b in ((0, 1), (1, 2), (2, 4))}
        if args.only == "all":
            a = res["grouped_g1"]
            res["r0_minus_grouped_ms"] = med["ext_r0"] - a["median_ms"]
            res["r0_slower_beyond_grouped_spread"] = bool(
                med["ext_r0"] - a["median_ms"] > a["spread_ms"])
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
