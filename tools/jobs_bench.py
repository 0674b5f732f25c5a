"""Job batches against the independent calls they replace, device buffers.

Three shapes: cfg1 at 32 particles x 64 jobs, cfg3 at 32 particles x 64 jobs, cfg2 at 4,096 x 4.
Every job is the workload's own batch toward its own targets, at its own call index.  Three rows
each:
  (a) J fks_forward_simulate_device calls on the generic kernels (specialisation off),
  (b) the same calls at the library's defaults (the shape-specialised kernel where it applies),
  (c) one fks_forward_simulate_jobs_device call.
Every call synchronises, so a row's time is a host clock around work that ends in a device
synchronise.  Per repetition the three rows run one after the other (a, b, c, a, b, c, ...), 2
warm-up repetitions (code objects, the shaped module's build) and 10 timed ones; a row's figure
is the median, its spread (max - min) / median.  (a) and (b) use only the plain entries: they
are the yardstick.  The final positions of the three rows must be identical bytes.

    python tools/jobs_bench.py [--out profiles/jobs_bench.json] [--reps 10] [--warmup 2]
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

    return [("cfg1", W.cfg1(1.0), 64), ("cfg3", W.cfg3(32 / 65536), 64), ("cfg2", W.cfg2(1.0), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jobs_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("jobs_bench.py measures on the GPU: no HIP device")
    torch.zeros(1, device="cuda:0")
    from fast_kinematic_simulator_amd import make_linked_simulator

    dev = "cuda:0"
    rows = []
    for name, wl, J in shapes():
        n, Wd = len(wl.starts), wl.robot.config_width
        d_starts = torch.tensor(wl.starts, dtype=torch.float64, device=dev).contiguous()
        d_targets = torch.tensor(wl.targets, dtype=torch.float64, device=dev).reshape(-1, Wd).contiguous()
        nt = d_targets.shape[0]
        out = {r: torch.zeros((J, n, Wd), dtype=torch.float64, device=dev) for r in "abc"}
        sims = {}
        for r in "abc":
            sims[r] = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
            sims[r].set_robot(wl.robot)
            if r != "b":
                sims[r].set_specialization(False)
        torch.cuda.synchronize()

        def calls(r):
            sim, o = sims[r], out[r]
            sim.set_call_index(0)
            for j in range(J):
                sim.forward_simulate_device(wl.robot, d_starts.data_ptr(), n, d_targets.data_ptr(), nt, 0, True, o[j].data_ptr(),
                                            synchronize=True)

        jobs = [{"d_starts": d_starts.data_ptr(), "n": n, "d_targets": d_targets.data_ptr(), "num_targets": nt, "allow_contacts": True,
                 "d_out_positions": out["c"][j].data_ptr()} for j in range(J)]

        def batch():
            sims["c"].set_call_index(0)
            sims["c"].forward_simulate_jobs_device(wl.robot, jobs, synchronize=True)

        run = {"a": lambda: calls("a"), "b": lambda: calls("b"), "c": batch}
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
        same = bool(torch.equal(out["a"], out["c"]) and torch.equal(out["a"], out["b"]))
        for r in "abc":
            sims[r].close()
            t = times[r]
            med = statistics.median(t)
            rows.append({"shape": name, "particles": n, "jobs": J, "row": r, "kernel": kernels[r], "median_ms": med,
                         "min_ms": min(t), "max_ms": max(t), "spread": (max(t) - min(t)) / med, "reps": len(t),
                         "last_kernel_ms": kernel_ms[r], "outputs_identical": same})
            print(json.dumps(rows[-1]), flush=True)
    result = {"tool": "tools/jobs_bench.py", "warmup": args.warmup, "reps": args.reps, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("| shape | particles x jobs | (a) calls, generic ms | (b) calls, defaults ms | (c) jobs ms | (a) spread | (c) spread | c / a |")
    print("|---|---|---|---|---|---|---|---|")
    for name in dict.fromkeys(r["shape"] for r in rows):
        a, b, c = (next(r for r in rows if r["shape"] == name and r["row"] == x) for x in "abc")
        print(f"| {name} | {a['particles']} x {a['jobs']} | {a['median_ms']:.2f} | {b['median_ms']:.2f} | {c['median_ms']:.2f} | "
              f"{a['spread']:.3f} | {c['spread']:.3f} | {c['median_ms'] / a['median_ms']:.3f} |")
    if not all(r["outputs_identical"] for r in rows):
        raise SystemExit("the rows' outputs differ")


if __name__ == "__main__":
    main()
