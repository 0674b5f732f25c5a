"""The host half of a robot (csrc/fks_robot.h) on the CPU: tests/cpp/robot_flatten_test.cpp links only
that unit, is built with AddressSanitizer and UndefinedBehaviorSanitizer, and checks the dof numbering,
every table fks_set_robot uploads, the levers, radii and links the skip proofs rest on against values
worked out by hand, every refusal's status and text, and the SDF analysis."""
import os
import subprocess


def test_robot_flatten_program():
    from fast_kinematic_simulator_amd.build import build_robot_flatten_test

    exe = build_robot_flatten_test()
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout, p.stderr[-6000:])
    assert "robot flatten test ok" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
