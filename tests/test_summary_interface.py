"""The C++ layers of the cluster summaries: tests/cpp/summary_interface_test.cpp runs SummarizeClusters
of the plain class and of the planner drop-in, and both static SummarizeClustersHost, against
fks_summarize_clusters_ctx and fks_summarize_clusters on groups of cfg1 configurations written out
behind the planner program's SE(2) scene, stand-alone and with the mock workspace on the include path."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cluster_cases as CC
from fast_kinematic_simulator_amd import workloads as W
from fast_kinematic_simulator_amd.build import build_summary_test
from test_planner_interface import _fmt, _write_scene

SIZES = (0, 1, 2, 40, 64, 65, 130)


def _run_summary_program(workspace):
    exe = build_summary_test(workspace=workspace)
    wl = CC.workload("cfg1")
    rng = np.random.default_rng(43)
    configs, centres = CC.draw_clumped(wl.robot, rng, sum(SIZES))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "scene.txt")
        _write_scene(path, "se2", wl, W.cfg1_obstacles(), (wl.resolution, W.grid_origin([0.0, 0.0, -2.0]), (wl.grid_cells,) * 3))
        with open(path, "a") as f:
            f.write(f"groups {len(SIZES)} 3 0.0 0.1 {np.inf!r}\n")
            at = 0
            for n in SIZES:
                f.write(f"{n}\n" + (_fmt(configs[at:at + n]) + "\n" if n else ""))
                at += n
        return subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)


def test_summary_program_builds_and_reports_a_missing_device():
    """g++ over the public headers; without a GPU the factory reports FKS_ERR_NO_DEVICE (exit 3)
    after the scene was read and its environment built"""
    p = _run_summary_program(False)
    assert p.returncode in (0, 3), (p.stdout, p.stderr)
    if p.returncode == 3:
        assert "no HIP device" in p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("workspace", [False, True], ids=["standalone", "workspace"])
def test_summary_interface(fks_lib, workspace):
    p = _run_summary_program(workspace)
    assert p.returncode == 0, (p.stdout, p.stderr)
    assert "summaries compared, 0 differences" in p.stdout, p.stdout
