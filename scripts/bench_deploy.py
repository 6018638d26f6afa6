#!/usr/bin/env python3
"""kcc_deploy against the host loop it replaces.

Arms in one process, alternating after a warm-up:
  (loop)   the only route without kcc_deploy, per step: max_replicas_per_row (kcc_fit_rows, host
           form: the node table goes up, q comes back), a numpy prefix sum (PACK) or water
           level (SPREAD) decides the placement, numpy patches used_cpu / used_mem / pod_count,
           and the next call uploads everything again.  Host clock around the loop: every
           call in it ends in a synchronise.  It knows no extended resources: R = 0 only.
  (host)   kcc_deploy, host form: one upload, K steps, the state back.  Host clock.
  (device) kcc_deploy_async on device-resident state, device events around the call; the copy
           of the pristine state into the working state is outside the timed window.
Before timing, at R = 0, the three arms' outputs are compared for equality (placed, the
per-row placement summed over the steps through pod_count, and the three state arrays).
Rows are synth's C3 (100k nodes) and C4 (1M nodes); the plan is K = 8 of the config's specs,
each asking for a sixteenth of what the untouched cluster would hold of it, so every step
binds and none exhausts the cluster.  Beside the times: the bytes the step's launches move,
counted from the kernels (kcc_deploy.hip), and the time those bytes take at 8 TB/s.  Prints
one JSON line per case; --out appends them to a file.

  python scripts/bench_deploy.py --cases C3,C4 --out profiles/deploy_bench.jsonl
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

PACK, SPREAD = 0, 1
R_MAX = (1 << 31) - 1
HBM_BYTES_PER_S = 8e12


def place_numpy(a, Rk, policy):
    """The placement of one step from the rows' counts (include/kcc.h kcc_deploy)."""
    T = int(a.sum())
    if Rk >= T:
        return a.copy()
    if Rk == 0:
        return np.zeros_like(a)
    if policy == PACK:
        before = np.cumsum(a) - a
        return np.minimum(a, np.maximum(0, Rk - before))
    lo, hi = 1, int(a.max())  # the smallest level t with sum(min(a, t)) >= Rk
    while lo < hi:
        mid = (lo + hi) // 2
        if int(np.minimum(a, mid).sum()) >= Rk:
            hi = mid
        else:
            lo = mid + 1
    p = np.minimum(a, lo - 1)
    top = np.flatnonzero(a >= lo)
    p[top[:Rk - int(p.sum())]] += 1
    return p


def step_bytes(n, r_req, policy, placed_rows, tiles):
    """Bytes one step's launches move (kcc_deploy.hip, no group ids, no placed_rows):
    dp_rows reads six 8-B columns and two per requested extra resource and writes a (4 B);
    dp_hist x 3 and dp_ind (SPREAD) read a; dp_scan reads and writes the tile sums; dp_apply
    reads a and, on the rows that take pods, reads and writes used_cpu, used_mem, pod_count and
    each requested extra column."""
    rows = n * (48 + 16 * r_req + 4)
    search = 4 * n * 4 if policy == SPREAD else 0
    scan = 16 * tiles
    apply_ = 4 * n + placed_rows * 16 * (3 + r_req)
    return rows + search + scan + apply_


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="C3,C4")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--ext", default="0,2")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    torch.cuda.init()
    from kubernetesclustercapacity_amd import CapacityEngine, _lib, synth
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    K = args.steps

    def T(a):
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
        sc_all, sm_all = synth.config_specs(name)
        ac, am, ap = c.alloc_cpu, c.alloc_mem, c.alloc_pods
        pc0, uc0, um0 = c.pod_count, r.cpu_requests, r.memory_requests
        n = ac.size
        tiles = (n + _lib.KCC_DEPLOY_TILE - 1) // _lib.KCC_DEPLOY_TILE
        ax, ux0, sx_all = extra_columns(n, max(sc_all.size, K), 20261021)
        # K specs with ordinary requests, each asking for 1/16 of what the cluster holds of it
        pick = np.flatnonzero((sc_all > 0) & (sm_all > 0))[:K]
        sc, sm, sx2 = sc_all[pick], sm_all[pick], sx_all[:, pick]
        rep = np.zeros(K, np.int64)
        for k in range(K):
            q, e = eng.max_replicas_per_row(ac, am, ap, pc0, uc0, um0, sc[k], sm[k])
            assert not e.any()
            rep[k] = max(int(np.maximum(q, 0).sum()) // 16, 1)
        print(f"# {name}: {n} nodes generated in {time.time() - t0:.1f} s; replicas {rep.tolist()}",
              flush=True)
        d_alloc = [T(ac), T(am), T(ap)]
        pristine = [T(pc0), T(uc0), T(um0)]
        work = [torch.empty_like(t) for t in pristine]
        d_sc, d_sm, d_rep = T(sc), T(sm), T(rep)
        outs = (torch.empty(K, dtype=torch.int64, device=dev), torch.empty(K, dtype=torch.int64, device=dev),
                torch.empty(K, dtype=torch.int32, device=dev))

        for policy in (PACK, SPREAD):
            def arm_loop():
                pc, uc, um = pc0.copy(), uc0.copy(), um0.copy()
                placed = np.zeros(K, np.int64)
                for k in range(K):
                    q, _ = eng.max_replicas_per_row(ac, am, ap, pc, uc, um, sc[k], sm[k])
                    Rk = min(max(int(rep[k]), 0), R_MAX)
                    a = np.minimum(np.maximum(q, 0), Rk)
                    p = place_numpy(a, Rk, policy)
                    uc += p.astype(np.uint64) * sc[k]
                    um += p * sm[k]
                    pc += p
                    placed[k] = p.sum()
                return placed, pc, uc, um

            def arm_host(R=0):
                return eng.deploy(ac, am, ap, pc0, uc0, um0, sc, sm, rep, policy, ax[:R], ux0[:R],
                                  sx2[:R], want_rows=False)

            for R in [int(x) for x in args.ext.split(",")]:
                d_ax, d_ux0, d_sx = T(ax[:R]), T(ux0[:R]), T(sx2[:R])
                d_ux = torch.empty_like(d_ux0)

                def reset():
                    with torch.cuda.stream(stream):
                        for w, p in zip(work, pristine):
                            w.copy_(p)
                        d_ux.copy_(d_ux0)

                def arm_device():
                    eng.deploy_async(*d_alloc, R, d_ax, work[0], work[1], work[2], d_ux, None, 1, None,
                                     d_sc, d_sm, d_sx, d_rep, None, policy, *outs, stream=stream)

                def timed_device():
                    reset()
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

                # outputs first
                timed_device()
                got = dict(placed=outs[0].cpu().numpy(), nodes_used=outs[1].cpu().numpy(),
                           err=outs[2].cpu().numpy(), pod_count=work[0].cpu().numpy(),
                           used_cpu=work[1].cpu().numpy().view(np.uint64), used_mem=work[2].cpu().numpy())
                h = arm_host(R)
                equal = all(np.array_equal(got[f], getattr(h, f)) for f in got)
                equal = equal and np.array_equal(d_ux.cpu().numpy().reshape(R, n), h.used_x)
                if R == 0:
                    lp, lpc, luc, lum = arm_loop()
                    equal = equal and bool(np.array_equal(lp, h.placed) and np.array_equal(lpc, h.pod_count)
                                           and np.array_equal(luc, h.used_cpu) and np.array_equal(lum, h.used_mem))
                if not equal or h.err.any():
                    emit(dict(case=name, policy=policy, n_ext=R, error="the arms' outputs differ"))
                    sys.exit(1)
                arms = [("device", timed_device), ("host", lambda: timed_host(lambda: arm_host(R)))]
                if R == 0:
                    arms.append(("loop", lambda: timed_host(arm_loop)))
                for _ in range(args.warmup):
                    for _, fn in arms:
                        fn()
                ms = {k: [] for k, _ in arms}
                for _ in range(args.reps):
                    for k, fn in arms:
                        ms[k].append(fn())
                res = dict(case=name, n_nodes=int(n), steps=K, n_ext=R,
                           policy="spread" if policy else "pack", outputs_equal=bool(equal),
                           placed=[int(v) for v in h.placed], nodes_used=[int(v) for v in h.nodes_used],
                           gpu=torch.cuda.get_device_name(0), **{k: stats(v) for k, v in ms.items()})
                r_req = [int((sx2[:R, k] != 0).sum()) for k in range(K)]
                nbytes = sum(step_bytes(n, r_req[k], policy, int(h.nodes_used[k]), tiles) for k in range(K))
                floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
                res.update(kernel_launches=K * (7 if policy else 3), memsets=5 if policy else 4,
                           bytes_moved=int(nbytes),
                           floor_ms_at_8TBps=floor_ms,
                           device_ms_per_step=res["device"]["median_ms"] / K,
                           floor_over_device=floor_ms / res["device"]["median_ms"])
                if R == 0:
                    res["loop_over_device"] = res["loop"]["median_ms"] / res["device"]["median_ms"]
                    res["loop_over_host"] = res["loop"]["median_ms"] / res["host"]["median_ms"]
                emit(res)
    eng.close()


if __name__ == "__main__":
    main()
