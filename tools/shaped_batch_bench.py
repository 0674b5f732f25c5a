"""Path, job and path-job batches on the generic kernels against the robot's batched shaped module
(DESIGN.md §4.15), device buffers.

The shapes are §4.14's three path-job batches, cfg1 at 32 particles x 64 jobs x 2 legs, cfg3 at
32 x 64 x 2 and cfg2 at 4,096 x 4 x 2 (every job the planner's edge: forward to the target, then
back to each particle's own start), and cfg3 at 8,192 particles x 3 legs through the path entry.
Two rows each:
  (a) the call with set_batched_specialization(False): the generic batched kernels,
  (b) the same call on the shaped kernels, the module built before anything is timed.
Every call synchronises, so a row's time is a host clock around work that ends in a device
synchronise.  Per repetition the rows run one after the other (a, b, a, b, ...), 2 warm-up
repetitions and 10 timed ones; a row's figure is the median, its spread (max - min) / median.
The bytes of (a) and (b) must be identical.

    python tools/shaped_batch_bench.py [--out profiles/shaped_batch_bench.json] [--reps 10] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes():
    from fast_kinematic_simulator_amd import workloads as W

    # name, workload, entry, jobs, legs
    return [("cfg1", W.cfg1(1.0), "path_jobs", 64, 2), ("cfg3", W.cfg3(32 / 65536), "path_jobs", 64, 2),
            ("cfg2", W.cfg2(1.0), "path_jobs", 4, 2), ("cfg3_path", W.cfg3(8192 / 65536), "path", 1, 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shaped_batch_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shape", action="append", default=[], help="only these shapes (default: all)")
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("shaped_batch_bench.py measures on the GPU: no HIP device")
    torch.zeros(1, device="cuda:0")
    from fast_kinematic_simulator_amd import make_linked_simulator

    dev = "cuda:0"
    rows = []
    for name, wl, entry, J, legs in shapes():
        if args.shape and name not in args.shape:
            continue
        n, Wd = len(wl.starts), wl.robot.config_width
        starts = np.asarray(wl.starts, dtype=np.float64).reshape(n, Wd)
        forward = np.tile(np.asarray(wl.targets, dtype=np.float64).reshape(-1, Wd)[:1], (n, 1))
        way = [forward, starts, forward][:legs]  # forward, back to the particle's own start, forward again
        d_starts = torch.tensor(starts, device=dev).contiguous()
        d_way = torch.tensor(np.stack(way), device=dev).contiguous()  # [legs][n][W]
        out = {r: torch.zeros((J, legs, n, Wd), dtype=torch.float64, device=dev) for r in "ab"}
        sims = {}
        for r in "ab":
            sims[r] = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
            sims[r].set_robot(wl.robot)
        sims["a"].set_batched_specialization(False)
        sims["b"].prepare_batched_specialization()  # the compile, or the cache, before anything is timed
        info = sims["b"].batched_specialization()
        torch.cuda.synchronize()

        def call(r):
            sim, o = sims[r], out[r]
            sim.set_call_index(0)
            if entry == "path":
                sim.forward_simulate_path_device(wl.robot, d_starts.data_ptr(), n, d_way.data_ptr(), legs, n, 0, True, o[0].data_ptr(),
                                                 synchronize=True)
            else:
                jobs = [{"d_starts": d_starts.data_ptr(), "n": n, "d_waypoints": d_way.data_ptr(), "num_legs": legs, "num_targets": n,
                         "allow_contacts": True, "d_out_positions": o[j].data_ptr()} for j in range(J)]
                sim.forward_simulate_path_jobs_device(wl.robot, jobs, synchronize=True)

        times = {r: [] for r in "ab"}
        for rep in range(args.warmup + args.reps):
            for r in "ab":
                t0 = time.perf_counter()
                call(r)
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= args.warmup:
                    times[r].append(dt)
        kernels = {r: sims[r].launch_info()["last_kernel"] for r in "ab"}
        kernel_ms = {r: sims[r].last_call_counters()["kernel_ms"] for r in "ab"}
        same = bool(torch.equal(out["a"], out["b"]))
        for r in "ab":
            sims[r].close()
            t = times[r]
            med = statistics.median(t)
            rows.append({"shape": name, "entry": entry, "particles": n, "jobs": J, "legs": legs, "row": r, "kernel": kernels[r],
                         "median_ms": med, "min_ms": min(t), "max_ms": max(t), "spread": (max(t) - min(t)) / med, "reps": len(t),
                         "last_kernel_ms": kernel_ms[r], "module": info["shape"], "module_from_cache": bool(info["from_cache"]),
                         "a_and_b_identical": same})
            print(json.dumps(rows[-1]), flush=True)
    result = {"tool": "tools/shaped_batch_bench.py", "warmup": args.warmup, "reps": args.reps, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("| shape | entry | particles x jobs x legs | (a) generic ms | (b) shaped ms | (a) spread | (b) spread | b / a | (b) kernel |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name in dict.fromkeys(r["shape"] for r in rows):
        a, b = (next(r for r in rows if r["shape"] == name and r["row"] == x) for x in "ab")
        print(f"| {name} | {a['entry']} | {a['particles']} x {a['jobs']} x {a['legs']} | {a['median_ms']:.2f} | {b['median_ms']:.2f} | "
              f"{a['spread']:.3f} | {b['spread']:.3f} | {b['median_ms'] / a['median_ms']:.3f} | {b['kernel']} |")
    if not all(r["a_and_b_identical"] for r in rows):
        raise SystemExit("the outputs of (a) and (b) differ")


if __name__ == "__main__":
    main()
