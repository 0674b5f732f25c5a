"""Build robot-shape-specialised kernels into the disk cache before a planner needs them.

    FKS_KERNEL_CACHE=<dir> python tools/precompile_kernels.py --workload cfg3 [--workload cfg5 ...] [--device 0] [--batched]

For each named BASELINE workload (or, from Python, any RobotDescription passed to
precompile()), a context is made on the device, the robot set and its shaped kernel built
(fks_set_specialization: the same module also carries the shaped configuration check).  The
code object lands in the disk cache (FKS_KERNEL_CACHE, default ~/.cache/fast_kinematic_simulator_amd),
where every later process on this machine finds it.  The launch layout that fixes a shape
depends on the device, so this runs on the GPU host the planner runs on.  Prints one JSON line
per robot: shape key, whether it was compiled now or found cached, and the failure log if any.
--batched also builds the robot's batched module (fks_prepare_batched_specialization: the kernels
of path, job and path-job batches, shape key ending in "-b") and adds its record under "batched".
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def precompile(robot, environment, solver, controller_frequency, seed=0, device=0, batched=False) -> dict:
    """Build `robot`'s shaped kernel on `device` into the caches; returns fks_get_specialization.
    batched: the batched module as well, its fks_get_batched_specialization under "batched"."""
    from fast_kinematic_simulator_amd import FksError, make_linked_simulator

    sim = make_linked_simulator(environment, solver, controller_frequency, seed, device=device)
    try:
        sim.set_robot(robot)
        try:
            sim.set_specialization(True)
        except FksError:
            pass  # reported through specialization()["failed"] / ["message"]
        info = sim.specialization()
        if batched:
            try:
                sim.prepare_batched_specialization()
            except FksError:
                pass  # reported through batched_specialization()["failed"] / ["message"]
            info["batched"] = sim.batched_specialization()
        return info
    finally:
        sim.close()


def main() -> int:
    from fast_kinematic_simulator_amd import workloads as W

    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="append", default=[], choices=sorted({**W.WORKLOADS, **W.COVERAGE}))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--batched", action="store_true", help="also build the module of path, job and path-job batches")
    a = ap.parse_args()
    rc = 0
    for name in a.workload or ["cfg3"]:
        wl = {**W.WORKLOADS, **W.COVERAGE}[name](8 / 65536 if name in W.WORKLOADS else 1.0)
        env = W.SCENES[name](device=a.device) if name in W.SCENES else wl.environment()
        info = precompile(wl.robot, env, wl.solver, wl.controller_frequency, wl.seed, a.device, batched=a.batched)

        def record(i):
            return {"shape": i["shape"], "active": bool(i["active"]), "from_cache": bool(i["from_cache"]),
                    "compile_seconds": i["compile_seconds"], "failed": bool(i["failed"]), "message": i["message"]}

        line = {"workload": name, **record(info)}
        if a.batched:
            line["batched"] = record(info["batched"])
        print(json.dumps(line), flush=True)
        rc = rc or (1 if info["failed"] or (a.batched and info["batched"]["failed"]) else 0)
    return rc


if __name__ == "__main__":
    sys.exit(main())
