"""Cluster summaries on the device against what a caller does without them, by the
method of §4.13 and tools/cluster_bench.py: device buffers, every call synchronised, a host clock.

Shapes: cfg1 (SE(2)) at 64 groups x 32 configurations, cfg4 (SE(3), the rotation mean) at 64 x 32,
cfg3's arm at 16 x 256.  The outcomes and their labels are resident in HBM (clumped draws of
tests/cluster_cases.py: six clumps per call, one configuration in eight a duplicate; the labels are
the clustering call's at a threshold between the clumps' diameter and their separation).  Two rows each:
  (a) what a caller does today: labels and positions come down, fks_summarize_clusters makes the
      child states on one host thread, the regrouped members go up as the next batch's starts;
  (b) one fks_summarize_clusters_device call on the resident arrays (every output but reached);
      only count and begin come down.
Per repetition the rows alternate (a, b, a, b, ...), 2 warm-up repetitions and 10 timed ones; a
row's figure is the median, with its min and max.  The two rows' members, counts, begins,
expectations and variances must be identical bytes.

    python tools/summary_bench.py [--out profiles/summary_bench.json] [--reps 10] [--warmup 2]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("summary_bench.py measures on the GPU: no HIP device")
    torch.zeros(1, device="cuda:0")
    import cluster_cases as CC
    from fast_kinematic_simulator_amd import SUMMARY_OUTPUTS, _capi, cluster_outcomes_host, make_linked_simulator, summarize_clusters_host

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
        N = G * n
        Wv = Wd if robot.robot_type == _capi.ROBOT_LINKED else (3 if robot.robot_type == _capi.ROBOT_SE2 else 6)
        names = [k for k in SUMMARY_OUTPUTS if k != "reached"]
        labels = np.concatenate(cluster_outcomes_host(robot, [configs[g * n:(g + 1) * n] for g in range(G)], threshold)["labels"])
        d_labels = torch.from_numpy(labels.astype(np.uint32).view(np.int32)).to(dev)
        widths = {"order": 1, "members": Wd, "count": 1, "begin": 1, "expectation": Wd, "variances": Wv, "variance": 1}
        d_out = {k: torch.zeros(N * widths[k], dtype=torch.int32 if k in ("order", "count", "begin") else torch.float64, device=dev)
                 for k in names}
        ptrs = {k: t.data_ptr() for k, t in d_out.items()}
        d_next = torch.zeros((N, Wd), dtype=torch.float64, device=dev)  # route (a)'s regrouped members, uploaded
        sim = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
        sim.set_robot(robot)
        torch.cuda.synchronize()
        result = {}

        def host():
            q = d_q.cpu().numpy()  # positions and labels down
            lab = d_labels.cpu().numpy().view(np.uint32)
            r = summarize_clusters_host(robot, [q[g * n:(g + 1) * n] for g in range(G)], [lab[g * n:(g + 1) * n] for g in range(G)],
                                        outputs=names)
            d_next.copy_(torch.from_numpy(r["members"]))  # members up
            torch.cuda.synchronize()
            result["a"] = r

        def device():
            sim.summarize_clusters_device(robot, d_q.data_ptr(), begin, d_labels.data_ptr(), d_out=ptrs, synchronize=True)
            result["b"] = (d_out["count"].cpu().numpy().view(np.uint32), d_out["begin"].cpu().numpy().view(np.uint32))  # count and begin down

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
        got = {k: (t.cpu().numpy().view(np.uint32) if t.dtype == torch.int32 else t.cpu().numpy()) for k, t in d_out.items()}
        same = all(got[k].tobytes() == np.ascontiguousarray(result["a"][k]).tobytes() for k in names)
        same = bool(same and result["b"][0].tobytes() == result["a"]["count"].tobytes() and d_next.cpu().numpy().tobytes() == got["members"].tobytes())
        per_group = (result["a"]["count"].reshape(G, n) > 0).sum(axis=1)
        clusters = [int(per_group.min()), int(per_group.max())]
        for r in "ab":
            t = times[r]
            med = statistics.median(t)
            rows.append({"shape": name, "groups": G, "group_size": n, "row": r, "threshold": threshold, "clusters_per_group": clusters,
                         "median_ms": med, "min_ms": min(t), "max_ms": max(t), "spread": (max(t) - min(t)) / med, "reps": len(t),
                         "outputs_identical": same})
            print(json.dumps(rows[-1]), flush=True)
    out = {"tool": "tools/summary_bench.py", "warmup": args.warmup, "reps": args.reps, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("| shape | groups x size | (a) host route ms (min-max) | (b) device call ms (min-max) | (a) spread | (b) spread | b / a | ranges apart |")
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
