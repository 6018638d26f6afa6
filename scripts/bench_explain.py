#!/usr/bin/env python3
"""The fit explained against the capped fit it extends.

Arms in one process, alternating after a warm-up, each timed with device events around work
that ends in a synchronise:
  (a) kcc_fit_capped_async with a per-node cap: the parent path;
  (b) kcc_fit_explain_async with all three outputs NULL: (a)'s kernels;
  (c) why_rows + why_pods;
  (d) left alone;
  (e) all three.
Before timing, outputs are compared cell by cell: the totals and flags of (b) - (e) against
(a); the planes of (c) and (d) against (e); and on (e) the sum of why_rows over the slots
against the groups' row counts, the wrapping sum of why_pods against the totals, and left
against sum(free) - request x total recomputed in numpy from the same rows.  Rows are synth's
C3 (100k nodes x 256 specs) and C4 (1M x 4096) with R = 0 and 2 extra resources, without group
ids and with 1024 uniform groups.  Prints one JSON line per case; --out appends them to a file.

  python scripts/bench_explain.py --cases C3,C4 --out profiles/explain_bench.jsonl
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


def left_numpy(rows, ax, ux, sc, sm, sx, gid, G, totals, err):
    """left [2 + R, G, S] by the identity, in wrapping uint64 numpy."""
    ac, am, _, _, uc, um = rows
    u = lambda a: np.ascontiguousarray(a).astype(np.int64, copy=False).view(np.uint64)  # noqa: E731
    free = [np.where(ac > uc, ac - uc, np.uint64(0)), np.where(am > um, u(am) - u(um), np.uint64(0))]
    free += [np.where(a > b, u(a) - u(b), np.uint64(0)) for a, b in zip(ax, ux)]
    req = [sc.astype(np.uint64), u(sm)] + [u(x) for x in sx]
    ids = np.zeros(ac.size, np.int64) if gid is None else gid.astype(np.int64)
    t = u(totals).reshape(G, -1)
    out = np.zeros((len(free), G, t.shape[1]), np.uint64)
    for k, (f, r) in enumerate(zip(free, req)):
        fsum = np.zeros(G, np.uint64)
        np.add.at(fsum, ids, f)
        out[k] = fsum[:, None] - r[None, :] * t
    out[:, err.reshape(G, -1) != 0] = 0
    return out.view(np.int64)


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
    from kubernetesclustercapacity_amd import KCC_WHY_SLOTS, CapacityEngine, synth
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
        for R in [int(x) for x in args.ext.split(",")]:
            d_ax, d_ux, d_sx = T(ax[:R]), T(ux[:R]), T(sx[:R])
            for G in [int(x) for x in args.groups.split(",")]:
                g1 = max(G, 1)
                gid = rng.integers(0, G, n).astype(np.int32) if G else None
                d_gid = T(gid) if G else None
                cells = g1 * S
                full = lambda k, t=torch.int64: torch.empty(k, dtype=t, device=dev)  # noqa: E731
                out = {k: (full(cells), full(cells, torch.int32)) for k in "abcde"}
                d_gr = full(g1)
                wr = {k: full(KCC_WHY_SLOTS * cells) for k in "ce"}
                wp = {k: full(KCC_WHY_SLOTS * cells) for k in "ce"}
                lf = {k: full((2 + R) * cells) for k in "de"}
                head = (*d_rows, R, d_ax, d_ux, d_gid, g1, d_sc, d_sm, d_sx)

                def arm_a():
                    eng.fit_capped_async(*head, *out["a"], d_cap, stream=stream)

                def arm_b():
                    eng.fit_explain_async(*head, d_cap, *out["b"], stream=stream)

                def arm_c():
                    eng.fit_explain_async(*head, d_cap, *out["c"], wr["c"], wp["c"], stream=stream)

                def arm_d():
                    eng.fit_explain_async(*head, d_cap, *out["d"], None, None, lf["d"], stream=stream)

                def arm_e():
                    eng.fit_explain_async(*head, d_cap, *out["e"], wr["e"], wp["e"], lf["e"],
                                          stream=stream)

                H = lambda t: t.cpu().numpy()  # noqa: E731
                timed(lambda: eng.fit_capped_async(*head, *out["a"], d_cap, None, d_gr, stream=stream))
                for fn in (arm_b, arm_c, arm_d, arm_e):
                    timed(fn)
                ta, ea = H(out["a"][0]), H(out["a"][1])
                equal = all(np.array_equal(H(out[k][0]), ta) and np.array_equal(H(out[k][1]), ea)
                            for k in "bcde")
                equal = equal and np.array_equal(H(wr["c"]), H(wr["e"])) and \
                    np.array_equal(H(wp["c"]), H(wp["e"])) and np.array_equal(H(lf["d"]), H(lf["e"]))
                ok = ea == 0
                wre = H(wr["e"]).reshape(KCC_WHY_SLOTS, cells)
                wpe = H(wp["e"]).reshape(KCC_WHY_SLOTS, cells)
                grows = np.repeat(H(d_gr), S)
                sums_ok = bool(np.array_equal(wre.sum(axis=0)[ok], grows[ok]) and np.array_equal(
                    wpe.view(np.uint64).sum(axis=0, dtype=np.uint64).view(np.int64)[ok], ta[ok]) and
                    not wre[:, ~ok].any() and not wpe[:, ~ok].any())
                want_left = left_numpy(rows, ax[:R], ux[:R], sc, sm, sx[:R], gid, g1, ta, ea)
                left_ok = bool(np.array_equal(H(lf["e"]).reshape(want_left.shape), want_left))
                if not (equal and sums_ok and left_ok):
                    emit(dict(case=name, n_ext=R, n_groups=G, error="the arms' outputs differ",
                              equal=bool(equal), sums_ok=sums_ok, left_ok=left_ok))
                    sys.exit(1)
                res = dict(case=name, n_nodes=int(n), n_specs=int(S), n_ext=R, n_groups=G,
                           outputs_equal=True, cells=int(cells), flagged_cells=int((~ok).sum()),
                           rows_by_slot=[int(v) for v in wre.sum(axis=1)],
                           device=torch.cuda.get_device_name(0),
                           **measure([("capped", arm_a), ("explain_null", arm_b),
                                      ("explain_why", arm_c), ("explain_left", arm_d),
                                      ("explain_all", arm_e)]))
                a = res["capped"]
                for k in ("explain_null", "explain_why", "explain_left", "explain_all"):
                    res[f"{k}_minus_capped_ms"] = res[k]["median_ms"] - a["median_ms"]
                    res[f"{k}_over_capped"] = res[k]["median_ms"] / a["median_ms"]
                res["null_inside_capped_spread"] = bool(
                    a["min_ms"] <= res["explain_null"]["median_ms"] <= a["max_ms"])
                emit(res)
                del out, wr, wp, lf
        del d_rows
    eng.close()


if __name__ == "__main__":
    main()
