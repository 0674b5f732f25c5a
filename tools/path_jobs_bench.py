"""Path-job batches against what a caller can do without them, device buffers.

Three shapes: cfg1 at 32 particles x 64 jobs x 2 legs, cfg3 at 32 x 64 x 2, cfg2 at 4,096 x 4 x 2.
Every job is the planner's edge: the workload's own batch forward to its target, then back to
each particle's own start, at its own call indices.  Three rows each:
  (a) J fks_forward_simulate_path_device calls one after the other (specialisation off): the
      sequence the batch's bytes are defined by,
  (b) K fks_forward_simulate_jobs_device calls, leg by leg, the previous leg's outputs as the
      next leg's starts: the other thing a caller can do; its call indices differ from (a)'s, so
      it is timed only,
  (c) one fks_forward_simulate_path_jobs_device call.
Every call synchronises, so a row's time is a host clock around work that ends in a device
synchronise.  Per repetition the three rows run one after the other (a, b, c, a, b, c, ...), 2
warm-up repetitions and 10 timed ones; a row's figure is the median, its spread
(max - min) / median.  The final bytes of (a) and (c) must be identical.

    python tools/path_jobs_bench.py [--out profiles/path_jobs_bench.json] [--reps 10] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = 2


def shapes():
    from fast_kinematic_simulator_amd import workloads as W

    return [("cfg1", W.cfg1(1.0), 64), ("cfg3", W.cfg3(32 / 65536), 64), ("cfg2", W.cfg2(1.0), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_jobs_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("path_jobs_bench.py measures on the GPU: no HIP device")
    torch.zeros(1, device="cuda:0")
    from fast_kinematic_simulator_amd import make_linked_simulator

    dev = "cuda:0"
    rows = []
    for name, wl, J in shapes():
        n, Wd = len(wl.starts), wl.robot.config_width
        starts = np.asarray(wl.starts, dtype=np.float64).reshape(n, Wd)
        forward = np.tile(np.asarray(wl.targets, dtype=np.float64).reshape(-1, Wd)[:1], (n, 1))
        d_starts = torch.tensor(starts, device=dev).contiguous()
        d_way = torch.tensor(np.stack([forward, starts]), device=dev).contiguous()  # [LEGS][n][W]: forward, then back
        out = {r: torch.zeros((J, LEGS, n, Wd), dtype=torch.float64, device=dev) for r in "abc"}
        sims = {}
        for r in "abc":
            sims[r] = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
            sims[r].set_robot(wl.robot)
            sims[r].set_specialization(False)
        torch.cuda.synchronize()

        def paths():
            sim, o = sims["a"], out["a"]
            sim.set_call_index(0)
            for j in range(J):
                sim.forward_simulate_path_device(wl.robot, d_starts.data_ptr(), n, d_way.data_ptr(), LEGS, n, 0, True, o[j].data_ptr(),
                                                 synchronize=True)

        leg_jobs = [[{"d_starts": d_starts.data_ptr() if k == 0 else out["b"][j, k - 1].data_ptr(), "n": n,
                      "d_targets": d_way[k].data_ptr(), "num_targets": n, "allow_contacts": True,
                      "d_out_positions": out["b"][j, k].data_ptr()} for j in range(J)] for k in range(LEGS)]

        def legs():
            sims["b"].set_call_index(0)
            for k in range(LEGS):
                sims["b"].forward_simulate_jobs_device(wl.robot, leg_jobs[k], synchronize=True)

        path_jobs = [{"d_starts": d_starts.data_ptr(), "n": n, "d_waypoints": d_way.data_ptr(), "num_legs": LEGS, "num_targets": n,
                      "allow_contacts": True, "d_out_positions": out["c"][j].data_ptr()} for j in range(J)]

        def batch():
            sims["c"].set_call_index(0)
            sims["c"].forward_simulate_path_jobs_device(wl.robot, path_jobs, synchronize=True)

        run = {"a": paths, "b": legs, "c": batch}
        times = {r: [] for r in "abc"}
        for rep in range(args.warmup + args.reps):
            for r in "abc":
                t0 = time.perf_counter()
                run[r]()
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= args.warmup:
                    times[r].append(dt)
        kernels = {r: sims[r].launch_info()["last_kernel"] for r in "abc"}
        kernel_ms = {r: sims[r].last_call_counters()["kernel_ms"] for r in "abc"}  # (a), (b): the last call's alone
        same = bool(torch.equal(out["a"], out["c"]))
        for r in "abc":
            sims[r].close()
            t = times[r]
            med = statistics.median(t)
            rows.append({"shape": name, "particles": n, "jobs": J, "legs": LEGS, "row": r, "kernel": kernels[r], "median_ms": med,
                         "min_ms": min(t), "max_ms": max(t), "spread": (max(t) - min(t)) / med, "reps": len(t),
                         "last_kernel_ms": kernel_ms[r], "a_and_c_identical": same})
            print(json.dumps(rows[-1]), flush=True)
    result = {"tool": "tools/path_jobs_bench.py", "warmup": args.warmup, "reps": args.reps, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("| shape | particles x jobs x legs | (a) path calls ms | (b) jobs calls per leg ms | (c) path jobs ms | (a) spread | (b) spread | "
          "(c) spread | c / a | c / b |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for name in dict.fromkeys(r["shape"] for r in rows):
        a, b, c = (next(r for r in rows if r["shape"] == name and r["row"] == x) for x in "abc")
        print(f"| {name} | {a['particles']} x {a['jobs']} x {a['legs']} | {a['median_ms']:.2f} | {b['median_ms']:.2f} | "
              f"{c['median_ms']:.2f} | {a['spread']:.3f} | {b['spread']:.3f} | {c['spread']:.3f} | "
              f"{c['median_ms'] / a['median_ms']:.3f} | {c['median_ms'] / b['median_ms']:.3f} |")
    if not all(r["a_and_c_identical"] for r in rows):
        raise SystemExit("the outputs of (a) and (c) differ")


if __name__ == "__main__":
    main()
