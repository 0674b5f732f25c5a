"""State selection on the device against what a caller does without it, by the method
of §4.13 and tools/summary_bench.py: device buffers, every call synchronised, a host clock.

Shapes: cfg1 (SE(2)), cfg4 (SE(3)) and cfg3's arm at J = 64 queries and P = 32 particles, against
S = 1,000 and S = 50,000 states each.  The table (keys, weights, counts 0 .. 48, begins, a pool of
S x 8 member rows) is resident in HBM and, for route (a), also on the host.  Two rows each:
  (a) what a caller does today: the table is already on the host, fks_select_states runs on one host
      thread (called through ctypes on preallocated arrays), the gathered starts [J][P][W] go up;
  (b) one fks_select_states_device call on the resident table (choice and starts); only choice comes
      down.
Per repetition the rows alternate (a, b, a, b, ...), 2 warm-up repetitions and 10 timed ones; a row's
figure is the median, with its min and max.  The two rows' choices and starts must be identical bytes.

--tile-lib PATH adds the tile comparison: the device call at S = 50,000 on this library and on the
build variant at PATH (FKS_SELECT_TILE=1: one query per workgroup of the search), each in a fresh child
process, alternating (this, variant, this, variant).

    python tools/select_bench.py [--out profiles/select_bench.json] [--reps 10] [--warmup 2] [--tile-lib build/libfks_tile1.so]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

J, P = 64, 32
SHAPES = [(name, S) for name in ("cfg1", "cfg4", "cfg3") for S in (1000, 50000)]


def measure(args, shapes, device_only):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("select_bench.py measures on the GPU: no HIP device")
    torch.zeros(1, device="cuda:0")
    import cluster_cases as CC
    from fast_kinematic_simulator_amd import _capi, make_linked_simulator, select_states_plan

    dev = "cuda:0"
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    lib = _capi.lib()
    rows = []
    for name, S in shapes:
        wl = CC.workload(name)
        robot, Wd = wl.robot, wl.robot.config_width
        rng = np.random.default_rng(21)
        base = CC.draw(robot, rng, 512)

        def spread(count):
            out = base[rng.integers(0, base.shape[0], count)].copy()
            cols = [3, 7, 11] if robot.robot_type == _capi.ROBOT_SE3 else list(range(Wd))
            out[:, cols] += rng.uniform(-0.05, 0.05, (count, len(cols)))
            return np.ascontiguousarray(out)

        keys, queries = spread(S), spread(J)
        weights = rng.uniform(0.5, 2.0, S)
        count = rng.integers(0, 49, S).astype(np.uint32)
        pool = 8 * S
        begin = rng.integers(0, pool - 48, S).astype(np.uint32)
        members = spread(pool)
        h = {"keys": keys, "weights": weights, "count": count, "begin": begin, "members": members}
        d = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).to(dev) for k, v in h.items()}
        d_q = torch.from_numpy(queries).to(dev)
        d_choice = torch.zeros(J, dtype=torch.int32, device=dev)
        d_starts = torch.zeros((J, P, Wd), dtype=torch.float64, device=dev)
        d_up = torch.zeros((J, P, Wd), dtype=torch.float64, device=dev)  # route (a)'s gathered starts, uploaded
        h_choice = np.zeros(J, dtype=np.uint32)
        h_starts = np.zeros((J, P, Wd))
        table = _capi.StateTable(num_states=S, num_member_rows=pool, **{k: v.ctypes.data for k, v in h.items()})
        sel = _capi.StateSelection(choice=h_choice.ctypes.data, starts=h_starts.ctypes.data)
        desc, keep = robot.to_c()
        sim = make_linked_simulator(wl.environment(), wl.solver, wl.controller_frequency, wl.seed)
        sim.set_robot(robot)
        torch.cuda.synchronize()
        result = {}

        def host():
            st = lib.fks_select_states(ctypes.byref(desc), ctypes.byref(table), _capi.as_ptr(queries, ctypes.c_double), J, P, 7,
                                       ctypes.byref(sel))
            assert st == 0
            d_up.copy_(torch.from_numpy(h_starts))  # the starts up
            torch.cuda.synchronize()

        def device():
            sim.select_states_device(robot, {k: t.data_ptr() for k, t in d.items()}, S, d_q.data_ptr(), J, P, 7,
                                     {"choice": d_choice.data_ptr(), "starts": d_starts.data_ptr()}, num_member_rows=pool, synchronize=True)
            result["b"] = d_choice.cpu().numpy().view(np.uint32)  # choice down

        run = {"a": host, "b": device}
        order = "b" if device_only else "ab"
        times = {r: [] for r in order}
        for rep in range(args.warmup + args.reps):
            for r in order:
                t0 = time.perf_counter()
                run[r]()
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= args.warmup:
                    times[r].append(dt)
        sim.close()
        same = None
        if not device_only:
            same = bool(result["b"].tobytes() == h_choice.tobytes() and d_starts.cpu().numpy().tobytes() == h_starts.tobytes()
                        and d_up.cpu().numpy().tobytes() == h_starts.tobytes())
        plan = select_states_plan(J, S, cus)
        for r in order:
            t = times[r]
            med = statistics.median(t)
            rows.append({"shape": name, "states": S, "queries": J, "particles": P, "row": r, "plan": plan, "median_ms": med, "min_ms": min(t),
                         "max_ms": max(t), "spread": (max(t) - min(t)) / med, "reps": len(t), "outputs_identical": same})
            print(json.dumps(rows[-1]), flush=True)
        del keep
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tile-lib", default=None, help="a build variant with FKS_SELECT_TILE=1 to time the device call against")
    ap.add_argument("--device-only", action="store_true", help="(the tile comparison's child) the S = 50,000 device rows alone, as JSON lines")
    args = ap.parse_args()
    if args.device_only:
        measure(args, [s for s in SHAPES if s[1] == 50000], True)
        return
    rows = measure(args, SHAPES, False)
    tile_rows = []
    if args.tile_lib:
        for turn in range(4):
            env = dict(os.environ)
            if turn % 2:
                env.update(FKS_LIB_PATH=os.path.abspath(args.tile_lib), FKS_VARIANT_LIB="1")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-only", "--reps", str(args.reps), "--warmup", str(args.warmup)],
                               env=env, stdout=subprocess.PIPE, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("the tile comparison's child failed")
            for line in p.stdout.splitlines():
                if line.startswith("{"):
                    tile_rows.append(dict(json.loads(line), turn=turn, library="tile 1" if turn % 2 else "product"))
                    print(json.dumps(tile_rows[-1]), flush=True)
    out = {"tool": "tools/select_bench.py", "warmup": args.warmup, "reps": args.reps, "rows": rows, "tile_rows": tile_rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("| shape | S | (a) host route ms (min-max) | (b) device call ms (min-max) | (a) spread | (b) spread | b / a | ranges apart |")
    print("|---|---|---|---|---|---|---|---|")
    for a in [r for r in rows if r["row"] == "a"]:
        b = next(r for r in rows if r["row"] == "b" and r["shape"] == a["shape"] and r["states"] == a["states"])
        apart = b["max_ms"] < a["min_ms"] or a["max_ms"] < b["min_ms"]
        print(f"| {a['shape']} | {a['states']} | {a['median_ms']:.3f} ({a['min_ms']:.3f}-{a['max_ms']:.3f}) | "
              f"{b['median_ms']:.3f} ({b['min_ms']:.3f}-{b['max_ms']:.3f}) | {a['spread']:.3f} | {b['spread']:.3f} | "
              f"{b['median_ms'] / a['median_ms']:.3f} | {'yes' if apart else 'no'} |")
    for r in tile_rows:
        print(f"| tile: {r['library']} (turn {r['turn']}) | {r['shape']} S={r['states']} tile {r['plan']['tile']} | "
              f"{r['median_ms']:.3f} ({r['min_ms']:.3f}-{r['max_ms']:.3f}) |")
    if not all(r["outputs_identical"] for r in rows):
        raise SystemExit("the rows' outputs differ")


if __name__ == "__main__":
    main()
