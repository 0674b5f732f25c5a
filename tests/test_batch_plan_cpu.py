"""The host-side plan of batched calls (csrc/fks_batch.h) on the CPU: tests/cpp/batch_plan_test.cpp
links only that unit, is built with AddressSanitizer and UndefinedBehaviorSanitizer, and checks
the normal form of a path, a job batch and a path-job batch, every refusal's status and text, the
segment plan and the kernel-argument records."""
import os
import subprocess


def test_batch_plan_program():
    from fast_kinematic_simulator_amd.build import build_batch_plan_test

    exe = build_batch_plan_test()
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout, p.stderr[-6000:])
    assert "batch plan test ok" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
