#!/usr/bin/env python3
"""kcc_consolidate against the loop a caller runs today.

Arms in one process, alternating after a warm-up:
  (loop)   per candidate one host-form kcc_deploy: one step per movable pod with requests,
           KCC_DEPLOY_PACK, the candidate's row ineligible (group id -1).  Timed on 16 candidates,
           reported per candidate.  Host clock.
  (host)   kcc_consolidate, host form: one upload, one launch, the outputs back.  Host clock.
  (device) kcc_consolidate_async on device-resident arrays, device events around the call.
Before timing, the arms' outputs are compared on those 16 candidates: evicted / placed / zero of
all three, pod_target of host and device.
Rows are synth's C3 (100k nodes, 2M pods) and C4 (1M nodes, 20M pods), built as
scripts/bench_drain.py builds them (a row runs as many pods as the config counts on it, shapes
from a palette of 200, a tenth of the pods unmovable).  The candidates are the 1024 and the 16384
rows of lowest cpu utilisation that run at least one pod.  --front-full f repeats every shape
with the first f of the rows left without free CPU (a packed cluster: as the configs generate
them the very first rows have room, and every first fit lies there).  Beside the times: the
mean row index a placed pod went to — the walk's cost is how far down the rows the first fit
lies.  Prints one JSON line per case, front and candidate count; --out appends them to a file.

  python scripts/bench_consolidate.py --cases C3,C4 --out profiles/consolidate_bench.jsonl
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

from bench_ext import stats  # noqa: E402

PACK = 0
LOOP_CANDS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="C3,C4")
    ap.add_argument("--cands", default="1024,16384")
    ap.add_argument("--front-full", default="0,0.9",
                    help="fractions of the rows, from the front, left without free CPU")
    ap.add_argument("--palette", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    torch.cuda.init()
    from kubernetesclustercapacity_amd import CapacityEngine, synth
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)

    def dv(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    eng = CapacityEngine(0, 1)
    for name in [c for c in args.cases.split(",") if c]:
        t0 = time.time()
        c = synth.config_cluster(name, limits=False)
        r = eng.get_pod_cpu_memory_requests_limits(c.node_ptr, c.cpu_req, c.mem_req)
        ac, am, ap = c.alloc_cpu, c.alloc_mem, c.alloc_pods
        pc0, uc0, um0 = c.pod_count, r.cpu_requests, r.memory_requests
        n = ac.size
        rng = np.random.default_rng([20261021, n])
        per = np.maximum(pc0, 0)
        ptr = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
        P = int(ptr[-1])
        pal_c = rng.choice(np.arange(50, 4000), args.palette, replace=False).astype(np.uint64)
        pal_m = rng.integers(1 << 26, 1 << 32, args.palette)
        idx = rng.integers(0, args.palette, P)
        pcpu, pmem = pal_c[idx], pal_m[idx]
        mv = (rng.random(P) < 0.9).astype(np.uint8)  # a tenth of the pods are DaemonSet pods
        print(f"# {name}: {n} nodes, {P} pods generated in {time.time() - t0:.1f} s", flush=True)
        d_nodes = [dv(ac), dv(am), dv(ap)]
        d_pods = [dv(ptr), dv(pcpu), dv(pmem)]
        d_mv = dv(mv)
        d_tgt = torch.empty(P, dtype=torch.int64, device=dev)
        uc_listed = uc0

        for front, Cn in [(float(f), int(v)) for f in args.front_full.split(",") if f
                          for v in args.cands.split(",") if v]:
            # a packed cluster: the first `front` of the rows have no free CPU, so a first fit
            # lies behind them (0: the rows as the config generates them)
            uc0 = uc_listed.copy()
            k_full = int(front * n)
            uc0[:k_full] = np.maximum(uc0[:k_full], ac[:k_full])
            d_state = [dv(pc0), dv(uc0), dv(um0)]
            # cpu utilisation, lowest first, among the rows that run a pod (a full or
            # overcommitted row sorts last)
            util = np.where(ac > 0, uc0.astype(np.float64) / np.maximum(ac, 1).astype(np.float64), np.inf)
            order = np.argsort(np.where(per > 0, util, np.inf), kind="stable")[:int((per > 0).sum())]
            cand = np.sort(order[:Cn]).astype(np.int64)
            Cn = cand.size
            d_cand = dv(cand)
            i64 = lambda k: torch.empty(k, dtype=torch.int64, device=dev)  # noqa: E731
            outs = [i64(Cn), i64(Cn), i64(Cn), torch.empty(Cn, dtype=torch.int32, device=dev)]
            # the loop arm's 16: spread over the candidates
            few = cand[np.linspace(0, Cn - 1, min(LOOP_CANDS, Cn)).astype(np.int64)]

            def arm_loop(rows=few):
                out = []
                for row in rows:
                    p = np.arange(ptr[row], ptr[row + 1])
                    p = p[mv[p] != 0]
                    zero = (pcpu[p] == 0) | (pmem[p] == 0)
                    t = p[~zero]
                    group = np.zeros(n, np.int32)
                    group[row] = -1
                    placed = 0
                    if t.size:
                        res = eng.deploy(ac, am, ap, pc0, uc0, um0, pcpu[t], pmem[t],
                                         np.ones(t.size, np.int64), PACK, group=group, n_groups=1,
                                         want_rows=False)
                        placed = int(res.placed.sum())
                    out.append((p.size, placed, int(zero.sum())))
                return out

            def arm_host(rows=cand, targets=False):
                return eng.consolidate(ac, am, ap, pc0, uc0, um0, rows, ptr, pcpu, pmem,
                                       pod_movable=mv, want_targets=targets)

            def arm_device(c_t=d_cand, o=outs):
                eng.consolidate_async(*d_nodes, 0, None, *d_state, None, None, *d_pods, None, d_mv,
                                      c_t, *o, d_tgt, stream=stream)

            def timed_device():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                arm_device()
                b.record(stream)
                b.synchronize()
                return a.elapsed_time(b)

            def timed_host(fn):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                return (time.perf_counter() - t) * 1e3

            # outputs first, on the loop arm's candidates
            h = arm_host(few, targets=True)
            o_few = [i64(few.size), i64(few.size), i64(few.size),
                     torch.empty(few.size, dtype=torch.int32, device=dev)]
            arm_device(dv(few), o_few)
            stream.synchronize()
            g = [t.cpu().numpy() for t in o_few] + [d_tgt.cpu().numpy()]
            lp = arm_loop()
            equal = all(np.array_equal(a, b) for a, b in
                        zip(g, (h.evicted, h.placed, h.zero, h.err, h.pod_target)))
            equal = equal and [tuple(v) for v in zip(h.evicted.tolist(), h.placed.tolist(),
                                                     h.zero.tolist())] == lp
            if not equal or h.err.any():
                emit(dict(case=name, front_full=front, n_cand=Cn, error="the arms' outputs differ"))
                sys.exit(1)

            arms = [("device", timed_device), ("host", lambda: timed_host(arm_host)),
                    ("loop", lambda: timed_host(arm_loop))]
            for _ in range(args.warmup):
                for _, fn in arms:
                    fn()
            ms = {k: [] for k, _ in arms}
            for _ in range(args.reps):
                for k, fn in arms:
                    ms[k].append(fn())
            stream.synchronize()
            ev, pl = outs[0].cpu().numpy(), outs[1].cpu().numpy()
            tgt = d_tgt.cpu().numpy()
            res = dict(case=name, n_nodes=int(n), n_pods=P, front_full=front, n_cand=int(Cn),
                       loop_cands=int(few.size),
                       outputs_equal=bool(equal), evicted=int(ev.sum()), placed=int(pl.sum()),
                       removable=int((ev == pl).sum()), max_evicted=int(ev.max()),
                       mean_target_row=float(tgt[tgt >= 0].mean()) if (tgt >= 0).any() else None,
                       max_target_row=int(tgt.max()), gpu=torch.cuda.get_device_name(0),
                       **{k: stats(v) for k, v in ms.items()})
            per_cand = dict(device=res["device"]["median_ms"] / Cn, host=res["host"]["median_ms"] / Cn,
                            loop=res["loop"]["median_ms"] / few.size)
            res.update(per_candidate_ms=per_cand, loop_over_host=per_cand["loop"] / per_cand["host"],
                       loop_over_device=per_cand["loop"] / per_cand["device"])
            emit(res)
    eng.close()


if __name__ == "__main__":
    main()
