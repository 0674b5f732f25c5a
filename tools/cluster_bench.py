"""Outcome clustering on the device against what a caller does without it, by the
method of §4.13: device buffers, every call synchronised, a host clock.

Shapes: cfg1 (SE(2)) at 64 groups x 32 configurations, cfg4 (SE(3), the expensive distance) at
64 x 32, cfg3's arm at 16 x 256.  The outcomes are resident in HBM (clumped draws of
tests/cluster_cases.py: six clumps per call, one configuration in eight a duplicate; the threshold
lies between the clumps' diameter and their separation).  Two rows each:
  (a) what a caller does today: the positions come down, fks_cluster_configs clusters them on one
      host thread (labels and counts);
  (b) one fks_cluster_configs_device call on the resident outcomes; only labels and counts come down.
Per repetition the rows alternate (a, b, a, b, ...), 2 warm-up repetitions and 10 timed ones; a
row's figure is the median, its spread (max - min) / median.  The two rows' labels and counts must
be identical bytes.

    python tools/cluster_bench.py [--out profiles/cluster_bench.json] [--reps 10] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("cluster_bench.py measures on the GPU: no HIP device")
    torch.zeros(1, device="cuda:0")
    import cluster_cases as CC
    from fast_kinematic_simulator_amd import cluster_outcomes_host, make_linked_simulator

    dev = "cuda:0"
    rows = []
    for name, G, n in (("cfg1", 64, 32), ("cfg4", 64, 32), ("cfg3", 16, 256)):
        wl = CC.workload(name)
        robot, Wd = wl.robot, wl.robot.config_width
        configs, centres = CC.draw_clumped(robot, np.random.default_rng(11), G * n)
        D = cluster_outcomes_host(robot, [centres], 0.0, distances=True, labels=False)["distances"][0]
        threshold = 0.5 * float(D[np.triu_indices(len(centres), 1)].min())
        begin = np.arange(0, G * n + 1, n, dtype=np.uint64)
        d_q = torch.tensor(configs, dtype=torch.float64, device=dev).contiguous()
        d_labels = torch.zeros(G * n, dtype=torch.int32, device=dev)
        d_counts = torch.zeros(G, dtype=torch.int32, device=dev)
        sim = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
        sim.set_robot(robot)
        torch.cuda.synchronize()
        result = {}

        def host():
            q = d_q.cpu().numpy()  # positions down
            r = cluster_outcomes_host(robot, [q[g * n:(g + 1) * n] for g in range(G)], threshold)
            result["a"] = (np.concatenate(r["labels"]), r["counts"])

        def device():
            sim.cluster_outcomes_device(robot, d_q.data_ptr(), begin, threshold, 0, d_labels.data_ptr(), d_counts.data_ptr(),
                                        synchronize=True)
            result["b"] = (d_labels.cpu().numpy().view(np.uint32), d_counts.cpu().numpy().view(np.uint32))  # labels and counts down

        run = {"a": host, "b": device}
        times = {r: [] for r in "ab"}
        for rep in range(args.warmup + args.reps):
            for r in "ab":
                t0 = time.perf_counter()
                run[r]()
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= args.warmup:
                    times[r].append(dt)
        sim.close()
        same = bool(np.array_equal(result["a"][0], result["b"][0]) and np.array_equal(result["a"][1], result["b"][1]))
        clusters = [int(result["a"][1].min()), int(result["a"][1].max())]
        for r in "ab":
            t = times[r]
            med = statistics.median(t)
            rows.append({"shape": name, "groups": G, "group_size": n, "row": r, "threshold": threshold, "clusters_per_group": clusters,
                         "median_ms": med, "min_ms": min(t), "max_ms": max(t), "spread": (max(t) - min(t)) / med, "reps": len(t),
                         "outputs_identical": same})
            print(json.dumps(rows[-1]), flush=True)
    out = {"tool": "tools/cluster_bench.py", "warmup": args.warmup, "reps": args.reps, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("| shape | groups x size | (a) host ms (min-max) | (b) device ms (min-max) | (a) spread | (b) spread | b / a | ranges apart |")
    print("|---|---|---|---|---|---|---|---|")
    for a in [r for r in rows if r["row"] == "a"]:
        b = next(r for r in rows if r["row"] == "b" and r["shape"] == a["shape"])
        apart = b["max_ms"] < a["min_ms"] or a["max_ms"] < b["min_ms"]
        print(f"| {a['shape']} | {a['groups']} x {a['group_size']} | {a['median_ms']:.3f} ({a['min_ms']:.3f}-{a['max_ms']:.3f}) | "
              f"{b['median_ms']:.3f} ({b['min_ms']:.3f}-{b['max_ms']:.3f}) | {a['spread']:.3f} | {b['spread']:.3f} | "
              f"{b['median_ms'] / a['median_ms']:.3f} | {'yes' if apart else 'no'} |")
    if not all(r["outputs_identical"] for r in rows):
        raise SystemExit("the rows' outputs differ")


if __name__ == "__main__":
    main()
