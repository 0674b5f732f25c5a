"""The launch decisions (csrc/fks_launch.h) on the CPU: tests/cpp/launch_plan_test.cpp links only that
unit, is built with AddressSanitizer and UndefinedBehaviorSanitizer, and checks a robot's layout
(workgroup halving, pairing, lean blocks, the HBM cap, the small-batch and cooperative geometries and
the refusal) against a fake occupancy query, the kernel and the module build of every kind of call, the
grid of a launch, the register gates and the kernel list's identities against values worked out by hand."""
import os
import subprocess


def test_launch_plan_program():
    from fast_kinematic_simulator_amd.build import build_launch_plan_test

    exe = build_launch_plan_test()
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout, p.stderr[-6000:])
    assert "launch plan test ok" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
