"""The HIP kernels' actuation half held to its definition.

The replay of tests/test_actuation_replay_cpu.py on traces the traced kernels wrote (the same scenes, bounds
and caps): the traced linked, SE(2) and SE(3) kernels, the lean traced kernel (cfg5), the individual-Jacobian
variant, the sampled actuator, a second call index, and a mutable-robot call that passes a non-zero PID state
in (fks_forward_simulate_traced_mutable).  The kernels draw the noise of floor(64 / D) microsteps at a time;
every linked scene, cfg1 (SE(2)) and cfg4 (SE(3)) have steps with more microsteps than that and steps whose
count is no multiple of it, so a draw taken from the wrong slot shows as a post-action record off by a whole
noise value.  The traced entry
takes no first particle id: ids above 2^32 are replayed on the oracle, which the untraced kernels equal bit
for bit.  tests/test_trace.py and the parity tests hold the untraced, shaped, small-batch and segmented kernels
bit-equal to the traced results, so they inherit the check."""
import pytest

import actuation_replay as AR


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted({**AR.SCENES, **AR.GPU_ONLY}))
def test_gpu_actuation_matches_reference(fks_lib, name):
    sc = AR.scene(name, device=0)
    stats = AR.replay_scene(sc, AR.gpu_traced(sc))
    assert max(stats["worst_input"], stats["worst_step"], stats["worst_post"]) <= 1.0
