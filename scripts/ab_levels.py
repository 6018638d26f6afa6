"""Timing of the preemption what-if against what a caller had to compose before
it, in ONE process on resident inputs.

  python scripts/ab_levels.py [--out profiles/levels_bench.jsonl] [--shapes C4,C3]   (GPU)

Reduce: kcc_reduce_requests_levels_async (L = 4, levels uniform) against L x
(kcc_pod_requests_async on request arrays with the pods below the level zeroed +
kcc_reduce_requests_async over the pods of each node); the masking itself is not timed, and
the composition yields no pod counts.  Every plane of the levelled reduce is checked against
the composition's sums.  Fit: kcc_fit_levels_async (S = 4096 and 256 split evenly over the
levels, G = 1 and 16) against L kcc_fit_capped_async calls on the planes; outputs compared.

Shapes: synth C4 (1M nodes, 39.6M containers cut into ~20M pods) and C3 (100k nodes, ~2M pods).
Each figure: warm-up calls, then events around REPS back-to-back calls, ROUNDS times; the median
and the spread (min, max) over the rounds.  One JSON line per measurement is appended to --out.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L = 4
HBM_BYTES_PER_S = 8e12


def timed(fn, torch, rounds, reps, warm):
    out = []
    for _ in range(rounds):
        for _ in range(warm):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "levels_bench.jsonl"))
    ap.add_argument("--shapes", default="C4,C3")
    args = ap.parse_args()
    import torch

    from kubernetesclustercapacity_amd import CapacityEngine, synth

    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    for shape in args.shapes.split(","):
        cl = synth.config_cluster(shape, limits=False)
        N = cl.node_ptr.size - 1
        ptr = torch.from_numpy(cl.node_ptr).to(dev)
        cpu = torch.from_numpy(cl.cpu_req.view(np.int64)).to(dev)
        mem = torch.from_numpy(cl.mem_req).to(dev)
        Cn = cpu.numel()
        g = torch.Generator(device=dev)
        g.manual_seed(20261021)
        start = torch.rand(Cn, device=dev, generator=g) < 0.5
        start[ptr[:-1][torch.diff(ptr) > 0]] = True  # a pod never spans two nodes
        starts = torch.nonzero(start).flatten()
        pod_ptr = torch.cat([starts, torch.tensor([Cn], device=dev)])
        P = pod_ptr.numel() - 1
        node_pod_ptr = torch.searchsorted(starts, ptr)  # pods that begin before each node
        level = torch.randint(0, L, (P,), device=dev, generator=g, dtype=torch.int64)
        lvl8 = level.to(torch.uint8)
        level_of_c = torch.repeat_interleave(level, torch.diff(pod_ptr))
        masked = [(torch.where(level_of_c >= l, cpu, 0), torch.where(level_of_c >= l, mem, 0))
                  for l in range(L)]
        del level_of_c
        uc, um, pc = (torch.empty(L * N, dtype=torch.int64, device=dev) for _ in range(3))
        b_pc, b_pm = (torch.empty(P, dtype=torch.int64, device=dev) for _ in range(2))
        b_uc, b_um = (torch.empty(L * N, dtype=torch.int64, device=dev) for _ in range(2))
        with CapacityEngine(0, 1) as eng:
            def levelled():
                eng.reduce_requests_levels_async(node_pod_ptr, pod_ptr, cpu, mem, lvl8, L, uc, um, pc)

            def composed():
                for l in range(L):
                    eng.pod_requests_async(pod_ptr, masked[l][0], masked[l][1], b_pc, b_pm)
                    eng.reduce_requests_async(node_pod_ptr, b_pc, b_pm, b_uc[l * N:(l + 1) * N],
                                              b_um[l * N:(l + 1) * N])

            t_new = timed(levelled, torch, 7, 10, 3)
            t_old = timed(composed, torch, 7, 10, 3)
            same = bool(torch.equal(uc, b_uc) and torch.equal(um, b_um)
                        and torch.equal(pc[:N], torch.diff(node_pod_ptr)))
            alg = 16 * Cn + 9 * P + 8 * N + 24 * L * N
            emit(what="reduce_levels", shape=shape, n_nodes=N, n_pods=P, n_containers=Cn, L=L,
                 ms=t_new[0], ms_min=t_new[1], ms_max=t_new[2], alg_bytes=alg,
                 hbm_frac=alg / (t_new[0] * 1e-3) / HBM_BYTES_PER_S, baseline="L x (pod_requests + reduce_requests)",
                 baseline_ms=t_old[0], baseline_ms_min=t_old[1], baseline_ms_max=t_old[2],
                 ratio=t_old[0] / t_new[0], faster_beyond_spread=bool(t_new[2] < t_old[1]),
                 planes_equal_baseline=same)
            del masked, b_pc, b_pm
            ac = torch.from_numpy(cl.alloc_cpu.view(np.int64)).to(dev)
            am = torch.from_numpy(cl.alloc_mem).to(dev)
            apods = torch.from_numpy(cl.alloc_pods).to(dev)
            for S in (4096, 256):
                sc_h, sm_h = synth.make_specs(S)
                sc = torch.from_numpy(sc_h.view(np.int64)).to(dev)
                sm = torch.from_numpy(sm_h).to(dev)
                lp = [S * l // L for l in range(L + 1)]
                for G in (1, 16):
                    grp = None if G == 1 else (torch.arange(N, device=dev, dtype=torch.int32) % G)
                    tot = torch.empty(G * S, dtype=torch.int64, device=dev)
                    err = torch.empty(G * S, dtype=torch.int32, device=dev)
                    parts = [(torch.empty(G * (lp[l + 1] - lp[l]), dtype=torch.int64, device=dev),
                              torch.empty(G * (lp[l + 1] - lp[l]), dtype=torch.int32, device=dev))
                             for l in range(L)]

                    def fit_levels():
                        eng.fit_levels_async(ac, am, apods, L, pc, uc, um, 0, None, None, grp, G, sc,
                                             sm, None, None, lp, tot, err)

                    def fit_calls():
                        for l in range(L):
                            pl = slice(l * N, (l + 1) * N)
                            eng.fit_capped_async(ac, am, apods, pc[pl], uc[pl], um[pl], 0, None, None,
                                                 grp, G, sc[lp[l]:lp[l + 1]], sm[lp[l]:lp[l + 1]], None,
                                                 parts[l][0], parts[l][1])

                    f_new = timed(fit_levels, torch, 5, 4, 1)
                    f_old = timed(fit_calls, torch, 5, 4, 1)
                    want_t = torch.cat([p[0].view(G, -1) for p in parts], 1).reshape(-1)
                    want_e = torch.cat([p[1].view(G, -1) for p in parts], 1).reshape(-1)
                    emit(what="fit_levels", shape=shape, n_nodes=N, S=S, G=G, L=L, ms=f_new[0],
                         ms_min=f_new[1], ms_max=f_new[2], baseline="L x fit_capped on the planes",
                         baseline_ms=f_old[0], baseline_ms_min=f_old[1], baseline_ms_max=f_old[2],
                         overhead_ms=f_new[0] - f_old[0], overhead_frac=f_new[0] / f_old[0] - 1.0,
                         cells_equal_baseline=bool(torch.equal(tot, want_t) and torch.equal(err, want_e)))
        del cpu, mem, uc, um, pc, b_uc, b_um
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("".join(ln + "\n" for ln in lines))


if __name__ == "__main__":
    main()
