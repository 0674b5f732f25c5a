"""Waypoint paths against the chained calls they replace, device buffers.

Three shapes: cfg1 at 32 particles x 8 legs, cfg2 at 4,096 x 4, cfg3 at 8,192 x 3.  Three rows each:
  (a) K chained fks_forward_simulate_device calls on the generic kernels (specialisation off),
  (b) the same chain at the library's defaults (the shape-specialised kernel where it applies),
  (c) one fks_forward_simulate_path_device call.
Every call synchronises, so a row's time is a host clock around work that ends in a device
synchronise.  Per repetition the three rows run one after the other (a, b, c, a, b, c, ...), 2
warm-up repetitions (code objects, the shaped module's build) and 10 timed ones; a row's figure
is the median, its spread (max - min) / median.  (a) is the yardstick: the same kernel family as
(c).  The final positions of the three rows must be identical bytes.

    python tools/path_bench.py [--out profiles/path_bench.json] [--reps 10] [--warmup 2]
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


def shapes():
    from fast_kinematic_simulator_amd import workloads as W

    c1, c2, c3 = W.cfg1(1.0), W.cfg2(1.0), W.cfg3(8192 / 65536)
    there_and_back = lambda wl, k: [wl.targets if i % 2 == 0 else wl.starts[:1] for i in range(k)]
    c1_legs = [c1.targets, [[0.6, 3.4, -1.0]], [[3.4, 0.6, 2.0]], [[0.6, 0.6, 0.0]]] * 2
    return [("cfg1", c1, [np.asarray(t, dtype=np.float64) for t in c1_legs]), ("cfg2", c2, there_and_back(c2, 4)),
            ("cfg3", c3, there_and_back(c3, 3))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("path_bench.py measures on the GPU: no HIP device")
    torch.zeros(1, device="cuda:0")
    from fast_kinematic_simulator_amd import make_linked_simulator

    dev = "cuda:0"
    rows = []
    for name, wl, legs in shapes():
        n, K, Wd = len(wl.starts), len(legs), wl.robot.config_width
        d_starts = torch.tensor(wl.starts, dtype=torch.float64, device=dev).contiguous()
        d_way = torch.tensor(np.stack(legs), dtype=torch.float64, device=dev).contiguous()  # [K, 1, W]
        out = {r: torch.zeros((K, n, Wd), dtype=torch.float64, device=dev) for r in "abc"}
        sims = {}
        for r in "abc":
            sims[r] = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
            sims[r].set_robot(wl.robot)
            if r != "b":
                sims[r].set_specialization(False)
        torch.cuda.synchronize()

        def chain(r):
            sim, o = sims[r], out[r]
            sim.set_call_index(0)
            for k in range(K):
                src = d_starts if k == 0 else o[k - 1]
                sim.forward_simulate_device(wl.robot, src.data_ptr(), n, d_way[k].data_ptr(), 1, 0, True, o[k].data_ptr(),
                                            synchronize=True)

        def path():
            sims["c"].set_call_index(0)
            sims["c"].forward_simulate_path_device(wl.robot, d_starts.data_ptr(), n, d_way.data_ptr(), K, 1, 0, True,
                                                   out["c"].data_ptr(), synchronize=True)

        run = {"a": lambda: chain("a"), "b": lambda: chain("b"), "c": path}
        times = {r: [] for r in "abc"}
        for rep in range(args.warmup + args.reps):
            for r in "abc":
                t0 = time.perf_counter()
                run[r]()
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= args.warmup:
                    times[r].append(dt)
        kernels = {r: sims[r].launch_info()["last_kernel"] for r in "abc"}
        same = bool(torch.equal(out["a"], out["c"]) and torch.equal(out["a"], out["b"]))
        for r in "abc":
            sims[r].close()
            t = times[r]
            med = statistics.median(t)
            rows.append({"shape": name, "particles": n, "legs": K, "row": r, "kernel": kernels[r], "median_ms": med,
                         "min_ms": min(t), "max_ms": max(t), "spread": (max(t) - min(t)) / med, "reps": len(t),
                         "outputs_identical": same})
            print(json.dumps(rows[-1]), flush=True)
    result = {"tool": "tools/path_bench.py", "warmup": args.warmup, "reps": args.reps, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("| shape | particles x legs | (a) chain, generic ms | (b) chain, defaults ms | (c) path ms | (a) spread | c / a |")
    print("|---|---|---|---|---|---|---|")
    for name in dict.fromkeys(r["shape"] for r in rows):
        a, b, c = (next(r for r in rows if r["shape"] == name and r["row"] == x) for x in "abc")
        print(f"| {name} | {a['particles']} x {a['legs']} | {a['median_ms']:.2f} | {b['median_ms']:.2f} | {c['median_ms']:.2f} | "
              f"{a['spread']:.3f} | {c['median_ms'] / a['median_ms']:.3f} |")
    if not all(r["outputs_identical"] for r in rows):
        raise SystemExit("the rows' outputs differ")


if __name__ == "__main__":
    main()
