"""The CPU oracle's contact resolution held to the definitions, iteration by iteration.

Bit parity between the HIP kernels and the oracle cannot see a misreading both share: a wrong
gradient axis, a normal chosen by the wrong maximum, a mass that is not the suffix sum, a scaling
decay one iteration off.  Here each scene is traced once on the oracle, and up to 128 of its resolver
iterations (a fixed stride over the whole trace) are recomputed from their recorded predecessor by
tests/hp_contact.py, a high-precision reference written from the reference header and the restated
library behaviour of DESIGN.md §2.2, and compared with the record: the next configuration within the
bound of tests/contact_replay.py, the collision verdict with what the trace does next, the stacked
system (J, b) the oracle solved with the reference's, row for row.  64 post-action configurations the
resolver did not run after must be free, and every controller step's microstep count must be the
reference's.  An iteration with a near decision (hp_contact's docstring) is not compared; at most 3 %
of a scene's replayed iterations may be skipped and at least 90 % must move the configuration.

Three kinds of near decision are compared before they count as skipped, and count only if that
comparison fails: a near rank decision at the structural rank; an extended self-collision key within
1e-9 of an integer at the key the header's own double arithmetic gives (the static base links of the
folding arm and of the telescope sit on cell faces: 75 % and 100 % of their iterations); a near pivot
tie that leads to other pivot columns at either pivot (every system of `wide_mixed`, whose prismatic
columns all have norm 1).  An all-zero system (only points no dof moves are corrected) is 0 / 0 by
the stated threshold and always skipped.

CheckConfigCollision is compared on 256 configurations of cfg3, of `mixed_tree` and of the telescope at
inflation 0 and 0.5; half of them are placed where the inflation ratio decides, and at least 10 % must
change their verdict between the two ratios (contact_replay.check_workload).  DESIGN.md §3 records the
measured ratios and the mutations of the oracle these tests catch."""
import numpy as np
import pytest

import contact_replay as R
import hp_contact as C
import hp_reference as H
from fast_kinematic_simulator_amd.trace import TRACE_RESOLVER_STEP


def oracle_traced(wl, individual):
    """(trace buffers, the stacked systems in trace order) of a one-thread oracle run"""
    import oracle

    with oracle.captured_systems(10 ** 7, 1, 10 ** 6) as systems:
        _, buf = oracle.forward_simulate_traced(wl.environment(), wl.robot, wl.solver, wl.controller_frequency, wl.seed, wl.starts,
                                                wl.targets, True, call_index=0, config_capacity=R.CONFIG_CAPACITY, threads=1,
                                                individual_jacobians=individual)
    return buf, systems


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_oracle_iterations_match_reference(oracle_lib, name):
    wl, individual = R.scene(name)
    buf, systems = oracle_traced(wl, individual)
    stats = R.replay_scene(name, wl, buf, individual, None if individual else systems)
    assert stats["compared"] > 0
    if not individual:
        assert stats["systems"] == stats["compared"]
    if name in ("folding_arm", "telescope", "resolver_params"):
        assert stats["self_corrected"] > 0


@pytest.mark.parametrize("name", R.CHECK_SCENES)
def test_oracle_config_checks_match_reference(oracle_lib, name):
    import oracle

    wl, configs = R.check_workload(name)
    results = [oracle.check_config_collision(wl.environment(), wl.robot, wl.solver, configs, inflation)
               for inflation in R.CHECK_INFLATIONS]
    assert not any(np.any(o["error_flags"]) for o in results)
    R.compare_config_checks(name, [o["collided"] for o in results])


def test_reference_backends_agree_on_iterations(oracle_lib):
    """The long-double and the 40-digit backends run the same code: on iterations of the telescope
    (self-collision corrections, a prismatic column, the rank decision) they take the same decisions
    and agree to long-double rounding."""
    wl, individual = R.scene("telescope")
    buf, _ = oracle_traced(wl, individual)
    mp = H.Backend("mpmath")
    refs = [C.ContactReference(wl.environment(), wl.robot, wl.solver, 1.0 / wl.controller_frequency, individual, B)
            for B in (H.DEFAULT, mp)]
    rp = R.Replay(wl, buf, refs[0])
    compared = 0
    for i, k in R.strided(rp.records(TRACE_RESOLVER_STEP), 3):
        post = rp.microstep_start(i, k)
        a, b = (R.with_double_keys(ref, lambda: ref.iterate(rp.previous(i, post), buf.configs[i, k - 1], k - post - 1))
                for ref in refs)
        assert a["corrected"] == b["corrected"] and a["in_collision"] == b["in_collision"]
        assert [s[:2] for s in a["solves"]] == [s[:2] for s in b["solves"]]
        for key, tol in (("next", 1e-16), ("J", 1e-17), ("b", 1e-17)):
            assert np.max(np.abs(H.to_float(a[key]) - H.to_float(b[key]))) <= tol, key
        assert H.max_abs_diff(b["next"], H.to_float(a["next"]), mp) < 1e-15
        compared += 1
    assert compared == 3
    # the module's one-call form is the same computation (exact-arithmetic keys)
    strict = refs[0].iterate(rp.previous(i, post), buf.configs[i, k - 1], k - post - 1)
    nxt, verdict, J, b, M = C.resolver_iteration(wl.environment(), wl.robot, wl.solver, rp.previous(i, post), buf.configs[i, k - 1],
                                                 k - post - 1, 1.0 / wl.controller_frequency)
    assert verdict == strict["in_collision"] and np.array_equal(H.to_float(J), H.to_float(strict["J"]))
    assert np.array_equal(H.to_float(b), H.to_float(strict["b"])) and M.near == strict["margins"].near
    assert (nxt is None and strict["next"] is None) or np.array_equal(H.to_float(nxt), H.to_float(strict["next"]))


def test_reference_scaling_schedule():
    """SPCS:1624, 1747-1761 by hand: the default schedule halves every 5 iterations from 1 and turns
    into -1/32 once below it; |scaling| is what the step is multiplied with."""
    wl, _ = R.scene("telescope")
    ref = C.ContactReference(wl.environment(), wl.robot, wl.solver, 1.0 / wl.controller_frequency)
    got = [float(ref.scaling(i)) for i in range(32)]
    expected = [1.0] * 5 + [0.5] * 5 + [0.25] * 5 + [0.125] * 5 + [0.0625] * 5 + [0.03125] * 5 + [-0.03125] * 2
    assert got == expected
