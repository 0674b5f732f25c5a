"""Policy roll-outs against the sequence a caller writes without them, device buffers.

Shapes: cfg1 at 32 particles x 8 legs, cfg3 at 32 x 4, cfg2 at 4,096 x 4, each with a table of M = 70
and of M = 4,096 entries (no terminal entry, max_distance +inf: every particle runs every leg, so
row (a) is one whole-batch call per leg).  Two rows each:
  (a) the K-leg sequence: per leg the positions come down, fks_policy_select chooses on the host, the
      chosen targets go up, and one fks_forward_simulate_device call with per-particle targets runs;
  (b) one fks_forward_simulate_policy_device call.
Both on the generic kernels (specialisation off).  Every call synchronises, so a row's time is a host
clock around work that ends in a device synchronise.  Per repetition the rows alternate (a, b, a, b,
...), 2 warm-up repetitions and 10 timed ones; a row's figure is the median, its spread
(max - min) / median.  The final positions of the two rows must be identical bytes.

    python tools/policy_bench.py [--out profiles/policy_bench.json] [--reps 10] [--warmup 2]
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


def table_for(wl, M, seed):
    """M states scattered over the box of the workload's starts and target (SE(3): a start's pose with
    its translation moved towards the target's), each state's action part of the way to the target"""
    from fast_kinematic_simulator_amd import PolicyTable

    rng = np.random.default_rng(seed)
    Wd = wl.robot.config_width
    starts = np.asarray(wl.starts, dtype=np.float64).reshape(-1, Wd)
    goal = np.asarray(wl.targets, dtype=np.float64).reshape(-1, Wd)[0]
    base = starts[rng.integers(0, len(starts), M)]
    keys = base + rng.uniform(0.0, 0.8, (M, 1)) * (goal - base) + rng.uniform(-0.05, 0.05, (M, Wd))
    targets = keys + rng.uniform(0.3, 0.8, (M, 1)) * (goal - keys)
    return PolicyTable(keys, targets, None, 0.0, float("inf"))


def shapes():
    from fast_kinematic_simulator_amd import workloads as W

    return [("cfg1", W.cfg1(1.0), 8), ("cfg3", W.cfg3(32 / 65536), 4), ("cfg2", W.cfg2(1.0), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("policy_bench.py measures on the GPU: no HIP device")
    torch.zeros(1, device="cuda:0")
    from fast_kinematic_simulator_amd import make_linked_simulator, policy_select

    dev = "cuda:0"
    rows = []
    for name, wl, K in shapes():
        for M in (70, 4096):
            table = table_for(wl, M, 7)
            n, Wd = len(wl.starts), wl.robot.config_width
            h_starts = np.ascontiguousarray(wl.starts, dtype=np.float64).reshape(n, Wd)
            h_targets = np.ascontiguousarray(table.targets)
            d_starts = torch.tensor(h_starts, dtype=torch.float64, device=dev).contiguous()
            d_keys = torch.tensor(np.ascontiguousarray(table.keys), dtype=torch.float64, device=dev).contiguous()
            d_targets = torch.tensor(h_targets, dtype=torch.float64, device=dev).contiguous()
            out = {r: torch.zeros((K, n, Wd), dtype=torch.float64, device=dev) for r in "ab"}
            d_choice = torch.zeros((K + 1, n), dtype=torch.int32, device=dev)
            sims = {}
            for r in "ab":
                sims[r] = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
                sims[r].set_robot(wl.robot)
                sims[r].set_specialization(False)
            torch.cuda.synchronize()

            def sequence():
                sim, o = sims["a"], out["a"]
                sim.set_call_index(0)
                q = h_starts
                for k in range(K):
                    if k > 0:
                        q = o[k - 1].cpu().numpy()  # positions down
                    choice = policy_select(wl.robot, table, q)["choice"]
                    d_t = torch.from_numpy(h_targets[choice]).to(dev)  # targets up
                    src = d_starts if k == 0 else o[k - 1]
                    sim.forward_simulate_device(wl.robot, src.data_ptr(), n, d_t.data_ptr(), n, 0, True, o[k].data_ptr(),
                                                synchronize=True)

            def roll_out():
                sims["b"].set_call_index(0)
                sims["b"].forward_simulate_policy_device(wl.robot, d_starts.data_ptr(), n, d_keys.data_ptr(), d_targets.data_ptr(), 0, M,
                                                         0.0, float("inf"), K, 0, True, out["b"].data_ptr(), d_choice.data_ptr(),
                                                         synchronize=True)

            run = {"a": sequence, "b": roll_out}
            times = {r: [] for r in "ab"}
            for rep in range(args.warmup + args.reps):
                for r in "ab":
                    t0 = time.perf_counter()
                    run[r]()
                    dt = (time.perf_counter() - t0) * 1e3
                    if rep >= args.warmup:
                        times[r].append(dt)
            kernels = {r: sims[r].launch_info()["last_kernel"] for r in "ab"}
            same = bool(torch.equal(out["a"], out["b"]))
            for r in "ab":
                sims[r].close()
                t = times[r]
                med = statistics.median(t)
                rows.append({"shape": name, "particles": n, "legs": K, "entries": M, "row": r, "kernel": kernels[r], "median_ms": med,
                             "min_ms": min(t), "max_ms": max(t), "spread": (max(t) - min(t)) / med, "reps": len(t),
                             "outputs_identical": same})
                print(json.dumps(rows[-1]), flush=True)
    result = {"tool": "tools/policy_bench.py", "warmup": args.warmup, "reps": args.reps, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("| shape | particles x legs | M | (a) sequence ms (min-max) | (b) roll-out ms (min-max) | (a) spread | (b) spread | b / a | ranges apart |")
    print("|---|---|---|---|---|---|---|---|---|")
    for a in [r for r in rows if r["row"] == "a"]:
        b = next(r for r in rows if r["row"] == "b" and r["shape"] == a["shape"] and r["entries"] == a["entries"])
        apart = b["max_ms"] < a["min_ms"] or a["max_ms"] < b["min_ms"]
        print(f"| {a['shape']} | {a['particles']} x {a['legs']} | {a['entries']} | {a['median_ms']:.2f} ({a['min_ms']:.2f}-{a['max_ms']:.2f}) | "
              f"{b['median_ms']:.2f} ({b['min_ms']:.2f}-{b['max_ms']:.2f}) | {a['spread']:.3f} | {b['spread']:.3f} | "
              f"{b['median_ms'] / a['median_ms']:.3f} | {'yes' if apart else 'no'} |")
    if not all(r["outputs_identical"] for r in rows):
        raise SystemExit("the rows' outputs differ")


if __name__ == "__main__":
    main()
