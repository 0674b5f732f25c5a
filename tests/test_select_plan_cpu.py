"""The host-side plan of a state selection and the host twin on the CPU: tests/cpp/select_plan_test.cpp
links only the HIP-free units (csrc/fks_batch.cpp, csrc/fks_state_select.cpp, csrc/fks_policy_select.cpp,
csrc/fks_robot.cpp), is built with AddressSanitizer and UndefinedBehaviorSanitizer, and checks every
refusal's status and text, the invariants of the decomposition over a sweep of queries, states and
compute-unit counts, and fks_select_states on hand cases with exactly-sized heap buffers (the guard case
at the pool's last row)."""
import os
import subprocess


def test_select_plan_program():
    from fast_kinematic_simulator_amd.build import build_select_plan_test

    exe = build_select_plan_test()
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout, p.stderr[-6000:])
    assert "select plan test ok" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
