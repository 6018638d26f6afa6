#!/usr/bin/env python3
"""Grouped fit against what a user did before it.

Two arms in one process, alternating after a warm-up, each timed with device events
around work that ends in a synchronise:
  (a) kcc_fit_grouped_async: one call, G x S cells;
  (b) kcc_fit_async once per group on device arrays already sorted and split by group
      (the sort is not charged to it).
Before timing, the two arms' outputs are compared cell by cell.  Shapes are seeded from
synth: C3 (100k nodes x 256 specs) and C4 (1M x 4096) with uniform group ids, plus one
Zipf-sized assignment at C3.  Prints one JSON line per case; --out appends them to a file.

  python scripts/bench_groups.py --cases C3:16,C3:1024,C3:1024:zipf,C4:16,C4:1024
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def group_ids(n, G, kind, seed):
    rng = np.random.default_rng([seed, G])
    if kind == "zipf":  # group sizes ~ Zipf(1.2): a few huge pools and a long tail
        return np.minimum(rng.zipf(1.2, n) - 1, G - 1).astype(np.int32)
    return rng.integers(0, G, n).astype(np.int32)


def stats(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]),
                p25_ms=float(np.percentile(a, 25)), p75_ms=float(np.percentile(a, 75)),
                spread_ms=float(a[-1] - a[0]), reps=int(a.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="C3:16,C3:1024,C3:1024:zipf,C4:16,C4:1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["both", "a"], default="both",
                    help="a: the grouped arm alone (for a kernel trace)")
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
    clusters = {}
    for case in args.cases.split(","):
        f = case.split(":")
        name, G, kind = f[0], int(f[1]), (f[2] if len(f) > 2 else "uniform")
        if name not in clusters:
            t0 = time.time()
            c = synth.config_cluster(name, limits=False)
            r = eng.get_pod_cpu_memory_requests_limits(c.node_ptr, c.cpu_req, c.mem_req)
            sc, sm = synth.config_specs(name)
            clusters[name] = ([c.alloc_cpu, c.alloc_mem, c.alloc_pods, c.pod_count,
                               r.cpu_requests, r.memory_requests], sc, sm)
            print(f"# {name}: {c.n_nodes} nodes, {sc.size} specs generated in "
                  f"{time.time() - t0:.1f} s", flush=True)
        rows, sc, sm = clusters[name]
        n, S = rows[0].size, sc.size
        gid = group_ids(n, G, kind, 20261015)
        d_rows, d_gid, d_sc, d_sm = [T(a) for a in rows], T(gid), T(sc), T(sm)
        tot_a = torch.empty(G * S, dtype=torch.int64, device=dev)
        err_a = torch.empty(G * S, dtype=torch.int32, device=dev)
        # arm (b)'s inputs: rows sorted by group, one slice per group
        order = np.argsort(gid, kind="stable")
        bounds = np.searchsorted(gid[order], np.arange(G + 1), "left")
        s_rows = [T(a[order]) for a in rows]
        tot_b = torch.zeros(G, S, dtype=torch.int64, device=dev)
        err_b = torch.zeros(G, S, dtype=torch.int32, device=dev)
        stream = torch.cuda.Stream(dev)

        def arm_a():
            eng.fit_grouped_async(*d_rows, d_gid, G, d_sc, d_sm, tot_a, err_a, stream=stream)

        def arm_b():
            for g in range(G):
                lo, hi = int(bounds[g]), int(bounds[g + 1])
                if hi == lo:
                    continue  # (an empty pool: zeros, set once above)
                eng._check(eng._lib.kcc_fit_async(
                    eng._h, hi - lo, *[x[lo:hi].data_ptr() for x in s_rows], S,
                    d_sc.data_ptr(), d_sm.data_ptr(), tot_b[g].data_ptr(), err_b[g].data_ptr(),
                    stream.cuda_stream))

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b)

        arms = [("grouped", arm_a)] + ([("per_group", arm_b)] if args.only == "both" else [])
        for _ in range(args.warmup):
            for _, fn in arms:
                timed(fn)
        equal = None
        if args.only == "both":
            ta, ea = tot_a.view(G, S).cpu().numpy(), err_a.view(G, S).cpu().numpy()
            tb, eb = tot_b.cpu().numpy(), err_b.cpu().numpy()
            equal = bool(np.array_equal(ta, tb) and np.array_equal(ea, eb))
            if not equal:
                print(json.dumps(dict(case=case, error="the two arms' outputs differ",
                                      cells_differ=int((ta != tb).sum() + (ea != eb).sum()))))
                sys.exit(1)
        ms = {k: [] for k, _ in arms}
        for _ in range(args.reps):
            for k, fn in arms:
                ms[k].append(timed(fn))
        res = dict(case=case, n_nodes=int(n), n_specs=int(S), n_groups=G, ids=kind,
                   outputs_equal=equal, device=torch.cuda.get_device_name(0),
                   **{k: stats(v) for k, v in ms.items()})
        if args.only == "both":
            a, b = res["grouped"], res["per_group"]
            res["speedup_median"] = b["median_ms"] / a["median_ms"]
            res["grouped_wins_beyond_spread"] = bool(
                b["median_ms"] - a["median_ms"] > max(a["spread_ms"], b["spread_ms"]))
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
