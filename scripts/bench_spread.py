#!/usr/bin/env python3
"""The capped fit and the spread fold against the extended-resource fit.

Arms in one process, alternating after a warm-up, each timed with device events around
work that ends in a synchronise:
  (a) kcc_fit_ext_async: the path the capped fit extends;
  (b) kcc_fit_capped_async with every optional pointer NULL: the same kernel instantiations
      as (a);
  (c) (b) with a per-node cap;
  (d) (c) with cell_min (and group_rows).
Before timing, outputs are compared cell by cell: (b) against (a); (c) and (d) against each
other, and run once with a cap nothing exceeds against (a).  Rows are synth's C3 (100k nodes
x 256 specs) and C4 (1M x 4096) with R = 0 and 2 extra resources, without group ids and with
1024 uniform groups.  Then the fold alone (kcc_spread_fold_async) at G x S = 1024 x 4096 and
4096 x 1 onto D = 3 domains with maxSkew 1, checked against numpy first.  Prints one JSON
line per case; --out appends them to a file.

  python scripts/bench_spread.py --cases C3,C4 --out profiles/spread_bench.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_ext import extra_columns, stats  # noqa: E402

I64_MAX = np.iinfo(np.int64).max
FOLD_SHAPES = ((1024, 4096, 3), (4096, 1, 3))


def fold_numpy(t, e, dom, D, k):
    """kcc_spread_fold with every group live, in numpy (no wrap on these inputs)."""
    G, S = t.shape
    cap = np.zeros((D, S), np.int64)
    np.add.at(cap, dom, t)
    present = np.zeros(D, bool)
    present[dom] = True
    cap = cap[present]
    lim = cap.min(axis=0) + k
    tot = np.minimum(cap, lim[None, :]).sum(axis=0)
    flagged = (e != 0).any(axis=0)
    return np.where(flagged, 0, tot), flagged.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="C3,C4")
    ap.add_argument("--ext", default="0,2")
    ap.add_argument("--groups", default="0,1024", help="0: no group ids")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    torch.cuda.init()
    from kubernetesclustercapacity_amd import CapacityEngine, synth
    dev = torch.device("cuda", 0)

    def T(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)

    stream = torch.cuda.Stream(dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    def measure(arms):
        for _ in range(args.warmup):
            for _, fn in arms:
                timed(fn)
        ms = {k: [] for k, _ in arms}
        for _ in range(args.reps):
            for k, fn in arms:
                ms[k].append(timed(fn))
        return {k: stats(v) for k, v in ms.items()}

    eng = CapacityEngine(0, 1)
    for name in [c for c in args.cases.split(",") if c]:
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
        rng = np.random.default_rng([20261021, n, S])
        d_cap = T(rng.choice(np.array([0, 1, 2, 4, 110], np.int64), S))
        d_nocap = T(np.full(S, I64_MAX, np.int64))
        for R in [int(x) for x in args.ext.split(",")]:
            d_ax, d_ux, d_sx = T(ax[:R]), T(ux[:R]), T(sx[:R])
            for G in [int(x) for x in args.groups.split(",")]:
                g1 = max(G, 1)
                d_gid = T(rng.integers(0, G, n).astype(np.int32)) if G else None
                cells = g1 * S
                out = {k: (torch.empty(cells, dtype=torch.int64, device=dev),
                           torch.empty(cells, dtype=torch.int32, device=dev)) for k in "abcd"}
                d_min = torch.empty(cells, dtype=torch.int64, device=dev)
                d_gr = torch.empty(g1, dtype=torch.int64, device=dev)
                head = (*d_rows, R, d_ax, d_ux, d_gid, g1, d_sc, d_sm, d_sx)

                def arm_a():
                    eng.fit_ext_async(*head, *out["a"], stream=stream)

                def arm_b():
                    eng.fit_capped_async(*head, *out["b"], stream=stream)

                def arm_c(cap=d_cap):
                    eng.fit_capped_async(*head, *out["c"], cap, stream=stream)

                def arm_d(cap=d_cap):
                    eng.fit_capped_async(*head, *out["d"], cap, d_min, d_gr, stream=stream)

                host = lambda k: (out[k][0].cpu().numpy().copy(), out[k][1].cpu().numpy().copy())  # noqa: E731
                same = lambda x, y: bool(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]))  # noqa: E731
                timed(arm_a)
                timed(arm_b)
                timed(lambda: arm_c(d_nocap))
                timed(lambda: arm_d(d_nocap))
                ref = host("a")
                equal = same(host("b"), ref) and same(host("c"), ref) and same(host("d"), ref)
                timed(arm_c)
                timed(arm_d)
                equal = equal and same(host("c"), host("d"))
                rows_ok = int(d_gr.sum().item()) == n
                if not (equal and rows_ok):
                    emit(dict(case=name, n_ext=R, n_groups=G, error="the arms' outputs differ"))
                    sys.exit(1)
                changed = int((host("c")[0] != ref[0]).sum())
                res = dict(case=name, n_nodes=int(n), n_specs=int(S), n_ext=R, n_groups=G,
                           outputs_equal=equal, cells_changed_by_cap=changed, cells=int(cells),
                           device=torch.cuda.get_device_name(0),
                           **measure([("ext", arm_a), ("capped_null", arm_b),
                                      ("capped_cap", arm_c), ("capped_cap_min", arm_d)]))
                a = res["ext"]
                for k in ("capped_null", "capped_cap", "capped_cap_min"):
                    res[f"{k}_minus_ext_ms"] = res[k]["median_ms"] - a["median_ms"]
                    res[f"{k}_over_ext"] = res[k]["median_ms"] / a["median_ms"]
                res["null_inside_ext_spread"] = bool(
                    a["min_ms"] <= res["capped_null"]["median_ms"] <= a["max_ms"])
                emit(res)
        del d_rows

    # the fold alone
    for G, S, D in FOLD_SHAPES:
        rng = np.random.default_rng([20261021, G, S])
        t = rng.integers(0, 5000, (G, S)).astype(np.int64)
        e = (rng.random((G, S)) < 1e-5).astype(np.int32)
        dom = rng.integers(0, D, G).astype(np.int32)
        d_t, d_e, d_dom = T(t.ravel()), T(e.ravel()), T(dom)
        d_gr = torch.ones(G, dtype=torch.int64, device=dev)
        d_k = torch.ones(S, dtype=torch.int64, device=dev)
        o = (torch.empty(S, dtype=torch.int64, device=dev), torch.empty(S, dtype=torch.int32, device=dev))

        def arm_fold():
            eng.spread_fold_async(G, S, d_t, d_e, d_gr, d_dom, D, None, d_k, *o, stream=stream)

        timed(arm_fold)
        wt, we = fold_numpy(t, e, dom, D, 1)
        equal = bool(np.array_equal(o[0].cpu().numpy(), wt) and np.array_equal(o[1].cpu().numpy(), we))
        if not equal:
            emit(dict(case=f"fold:{G}x{S}", error="the fold differs from numpy"))
            sys.exit(1)
        emit(dict(case=f"fold:{G}x{S}", n_groups=G, n_specs=S, n_domains=D, outputs_equal=equal,
                  device=torch.cuda.get_device_name(0), **measure([("fold", arm_fold)])))
    eng.close()


if __name__ == "__main__":
    main()
