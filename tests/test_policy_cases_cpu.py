"""The roll-out cases of tests/test_policy.py on the CPU oracle: the sequence of the contract
(tests/policy_cases.py: reference_chain) with the oracle simulating every run of active particles
(call index c + k, first_particle_id = the run's first particle).  It checks, on a machine without
a GPU, that each case makes the decisions its GPU test asserts before it compares: stops at several
legs, many entries chosen per leg, an index >= 64, the tie of entries 10 and 66 met and resolved
to 10, contacts, arrivals.  The GPU tests keep the same asserts on the GPU's own reference."""
import numpy as np
import pytest

import policy_cases as PC

BASE_CALL = 5


def _oracle_chain(wl, starts, table, K):
    import oracle

    def simulate(k, a, q, targets):
        return oracle.forward_simulate(wl.environment(), wl.robot, wl.solver, wl.controller_frequency, wl.seed, q, targets, True,
                                       call_index=BASE_CALL + k, first_particle_id=a)

    return PC.reference_chain(simulate, wl.robot, starts, table, K)


def _assert_rows_are_defined(ref, starts, K):
    """rows a particle does not run: the configuration handed over, zeros, NONE and +inf"""
    from fast_kinematic_simulator_amd import _capi

    for p, legs in enumerate(ref["legs_run"]):
        held = starts[p] if legs == 0 else ref["positions"][legs - 1, p]
        for k in range(legs, K):
            assert np.array_equal(ref["positions"][k, p], held)
            assert not ref["collided"][k, p] and ref["microsteps"][k, p] == 0 and ref["error_flags"][k, p] == 0
        assert np.all(ref["choice"][legs + 1:, p] == _capi.POLICY_NONE) and np.all(ref["distance"][legs + 1:, p] == np.inf)
        assert ref["choice"][legs, p] != _capi.POLICY_NONE


@pytest.mark.parametrize("max_distance", [1.2, np.inf], ids=["max_1.2", "max_inf"])
def test_cfg1_case_decides_what_its_test_asserts(fks_lib, oracle_lib, max_distance):
    wl, starts, table, K = PC.cfg1_case(max_distance)
    ref = _oracle_chain(wl, starts, table, K)
    PC.check_cfg1(ref, K)
    _assert_rows_are_defined(ref, starts, K)
    if max_distance == 1.2:
        from fast_kinematic_simulator_amd import _capi

        assert (ref["choice"] == _capi.POLICY_LOST).any()


def test_linked_cases_decide_what_their_tests_assert(fks_lib, oracle_lib):
    for case in (PC.folding_case, PC.cfg3_case):
        wl, starts, table, K = case()
        ref = _oracle_chain(wl, starts, table, K)
        PC.check_arm(ref, K)
        _assert_rows_are_defined(ref, starts, K)


def test_se3_case_decides_what_its_test_asserts(fks_lib, oracle_lib):
    wl, starts, table, K = PC.cfg4_case()
    ref = _oracle_chain(wl, starts, table, K)
    PC.check_cfg4(ref, K)
    _assert_rows_are_defined(ref, starts, K)
