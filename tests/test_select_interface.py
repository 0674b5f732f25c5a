"""The C++ layers of the state selection: tests/cpp/select_interface_test.cpp runs SelectStates of the
plain class and of the planner drop-in, and both static SelectStatesHost, against fks_select_states_ctx
and fks_select_states on a table of cfg1 states written out behind the planner program's SE(2) scene,
stand-alone and with the mock workspace on the include path."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cluster_cases as CC
from fast_kinematic_simulator_amd import select_states_host
from fast_kinematic_simulator_amd import workloads as W
from fast_kinematic_simulator_amd.build import build_select_test
from test_planner_interface import _fmt, _write_scene

S, ROWS, P, J = 300, 500, 6, 21


def _run_select_program(workspace):
    exe = build_select_test(workspace=workspace)
    wl = CC.workload("cfg1")
    rng = np.random.default_rng(47)
    keys = CC.draw(wl.robot, rng, S)
    weights = rng.uniform(0.5, 2.0, S)
    count = rng.choice([0, 1, P, P, P - 2, P + 5], S)
    begin = rng.integers(0, ROWS - P - 5, S)
    begin[::9] = ROWS - count[::9]  # these end exactly at the pool's end
    begin[4::9] = ROWS - count[4::9] + 1  # these one row past it
    members = CC.draw(wl.robot, rng, ROWS)
    queries = CC.draw(wl.robot, rng, J)
    # the case decides something: states of exactly P members (copied in order), of other counts (drawn), past the pool's end
    ref = select_states_host(wl.robot, keys, queries, P, 1, weights=weights, count=count, begin=begin, members=members)
    chosen = count[ref["choice"]]
    assert np.any(chosen == P) and np.any(chosen != P) and np.any(np.all(ref["source"] == 0xFFFFFFFF, axis=1))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "scene.txt")
        _write_scene(path, "se2", wl, W.cfg1_obstacles(), (wl.resolution, W.grid_origin([0.0, 0.0, -2.0]), (wl.grid_cells,) * 3))
        with open(path, "a") as f:
            f.write(f"table {S} {ROWS} {P} {J}\n")
            for i in range(S):
                f.write(f"{_fmt(keys[i:i + 1])} {float(weights[i])!r} {int(count[i])} {int(begin[i])}\n")
            f.write(_fmt(members) + "\n" + _fmt(queries) + "\n")
        return subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)


def test_select_program_builds_and_reports_a_missing_device():
    """g++ over the public headers; without a GPU the factory reports FKS_ERR_NO_DEVICE (exit 3)
    after the scene was read and its environment built"""
    p = _run_select_program(False)
    assert p.returncode in (0, 3), (p.stdout, p.stderr)
    if p.returncode == 3:
        assert "no HIP device" in p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("workspace", [False, True], ids=["standalone", "workspace"])
def test_select_interface(fks_lib, workspace):
    p = _run_select_program(workspace)
    assert p.returncode == 0, (p.stdout, p.stderr)
    assert "selections compared, 0 differences" in p.stdout, p.stdout
