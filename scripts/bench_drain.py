#!/usr/bin/env python3
"""kcc_drain against the host route it replaces.

Arms in one process, alternating after a warm-up:
  (loop)   the route without kcc_drain: the drained rows' pods gathered on the host, np.unique
           over the shape columns (descending), the drained rows filled in numpy, then the host
           form of kcc_deploy with one step per shape.  Host clock.
  (host)   kcc_drain, host form: one upload, the pod pass, D steps, the state back.  Host clock.
  (device) kcc_drain_async on device-resident state and pods, device events around the call;
           the copy of the pristine state into the working state is outside the timed window.
           It runs max_shapes steps: the ones behind D are padding.
Before timing the three arms' outputs are compared for equality (the summary, the shapes and
their counts, what each shape placed, and the four state arrays).
Rows are synth's C3 (100k nodes, 2M pods) and C4 (1M nodes, 20M pods); a row runs as many pods
as the config counts on it, their shapes drawn from a palette of 200; one zone of eight (the
rows with i % 8 == 0) is drained; max_shapes 256.  Beside the times: the bytes the new kernels
move (not the deploy steps'), counted from kcc_drain.hip, and the time those bytes take at
8 TB/s.  Prints one JSON line per case and policy; --out appends them to a file.

  python scripts/bench_drain.py --cases C3,C4 --out profiles/drain_bench.jsonl
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

PACK, SPREAD = 0, 1
HBM_BYTES_PER_S = 8e12


def drain_bytes(n, P, n_drained, evicted, D, M, T):
    """Bytes the new launches move at R = 0 (kcc_drain.hip): the table's reset; dr_rows reads
    drain and copies three 8-B columns on the drained rows; dr_pods reads the CSR offsets, the
    drain bytes and pod_movable once (the search's repeats hit in cache), an evicted pod's 16-B
    key and its slot's representative's, and adds 4 B to the slot's count; dr_plan's T / 256
    workgroups each read the T slots and the D representatives' keys, and write the plan and
    the four key outputs; dr_finish reads and writes the three step outputs."""
    reset = 8 * T + 64
    rows = n + n_drained * 48
    pods = 8 * (n + 1) + n + P + evicted * (16 + 16 + 4 + 4)
    plan = (T // 256) * (4 * T + 16 * D) + M * (4 * 8 + 3 * 8)
    finish = M * 2 * (8 + 8 + 4) + 32
    return reset + rows + pods + plan + finish


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="C3,C4")
    ap.add_argument("--palette", type=int, default=200)
    ap.add_argument("--max-shapes", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    torch.cuda.init()
    from kubernetesclustercapacity_amd import CapacityEngine, synth
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    M = args.max_shapes
    T = 256
    while T < 2 * M:
        T *= 2

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
        drain = (np.arange(n) % 8 == 0).astype(np.uint8)
        print(f"# {name}: {n} nodes, {P} pods generated in {time.time() - t0:.1f} s", flush=True)

        d_alloc = [dv(ac), dv(am), dv(ap)]
        pristine = [dv(pc0), dv(uc0), dv(um0)]
        work = [torch.empty_like(t) for t in pristine]
        d_pods = [dv(drain), dv(ptr), dv(pcpu), dv(pmem)]
        d_mv = dv(mv)
        i64 = lambda k: torch.empty(k, dtype=torch.int64, device=dev)  # noqa: E731
        outs = [i64(4), i64(M), i64(M), None, i64(M), i64(M), i64(M),
                torch.empty(M, dtype=torch.int32, device=dev)]

        for policy in (PACK, SPREAD):
            def arm_loop():
                on = np.repeat(drain, per).astype(bool) & (mv != 0)
                keys = np.stack([pcpu[on].astype(np.int64), pmem[on]], axis=1)
                u, cnt = np.unique(keys, axis=0, return_counts=True)
                u, cnt = u[::-1], cnt[::-1]  # descending (plain values: signed order is unsigned order)
                d = drain != 0
                pc, uc, um = np.where(d, ap, pc0), np.where(d, ac, uc0), np.where(d, am, um0)
                res = eng.deploy(ac, am, ap, pc, uc, um, u[:, 0].astype(np.uint64), u[:, 1], cnt,
                                 policy, want_rows=False)
                return u, cnt, res

            def arm_host():
                return eng.drain(ac, am, ap, pc0, uc0, um0, drain, ptr, pcpu, pmem, policy,
                                 pod_movable=mv, max_shapes=M)

            def reset():
                with torch.cuda.stream(stream):
                    for w, p in zip(work, pristine):
                        w.copy_(p)

            def arm_device(m):
                eng.drain_async(*d_alloc, 0, None, *work, None, *d_pods, None, d_mv, policy, m,
                                *outs, stream=stream)

            def timed_device(m=M):
                reset()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                arm_device(m)
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
            h = arm_host()
            D = h.shapes
            summary = outs[0].cpu().numpy()
            equal = D >= 0 and summary.tolist() == [h.drained_rows, h.evicted, h.shapes, h.placed]
            for t, f in ((outs[1], "shape_cpu"), (outs[2], "shape_mem"), (outs[4], "shape_count"),
                         (outs[5], "shape_placed"), (outs[6], "shape_nodes"), (outs[7], "shape_err")):
                g = t.cpu().numpy()
                g = g.view(np.uint64) if f == "shape_cpu" else g
                equal = equal and np.array_equal(g[:D], getattr(h, f)) and not g[D:].any()
            for t, f in zip(work, ("pod_count", "used_cpu", "used_mem")):
                g = t.cpu().numpy()
                equal = equal and np.array_equal(g.view(np.uint64) if f == "used_cpu" else g, getattr(h, f))
            u, cnt, lp = arm_loop()
            equal = equal and bool(
                np.array_equal(u[:, 0].astype(np.uint64), h.shape_cpu) and np.array_equal(u[:, 1], h.shape_mem)
                and np.array_equal(cnt, h.shape_count) and np.array_equal(lp.placed, h.shape_placed)
                and np.array_equal(lp.nodes_used, h.shape_nodes) and np.array_equal(lp.pod_count, h.pod_count)
                and np.array_equal(lp.used_cpu, h.used_cpu) and np.array_equal(lp.used_mem, h.used_mem))
            if not equal or h.shape_err.any():
                emit(dict(case=name, policy=policy, error="the arms' outputs differ"))
                sys.exit(1)
            # device_exact: max_shapes = D, no padding steps (the difference is what they cost)
            arms = [("device", timed_device), ("device_exact", lambda: timed_device(max(D, 1))),
                    ("host", lambda: timed_host(arm_host)), ("loop", lambda: timed_host(arm_loop))]
            for _ in range(args.warmup):
                for _, fn in arms:
                    fn()
            ms = {k: [] for k, _ in arms}
            for _ in range(args.reps):
                for k, fn in arms:
                    ms[k].append(fn())
            res = dict(case=name, n_nodes=int(n), n_pods=P, palette=args.palette, max_shapes=M,
                       policy="spread" if policy else "pack", outputs_equal=bool(equal),
                       drained_rows=h.drained_rows, evicted=h.evicted, shapes=D, placed=h.placed,
                       padding_steps=M - D, gpu=torch.cuda.get_device_name(0),
                       **{k: stats(v) for k, v in ms.items()})
            nbytes = drain_bytes(n, P, h.drained_rows, h.evicted, D, M, T)
            res.update(drain_kernel_bytes=int(nbytes),
                       drain_kernel_floor_ms_at_8TBps=nbytes / HBM_BYTES_PER_S * 1e3,
                       padding_ms=res["device"]["median_ms"] - res["device_exact"]["median_ms"],
                       loop_over_host=res["loop"]["median_ms"] / res["host"]["median_ms"],
                       loop_over_device=res["loop"]["median_ms"] / res["device"]["median_ms"])
            emit(res)
    eng.close()


if __name__ == "__main__":
    main()
