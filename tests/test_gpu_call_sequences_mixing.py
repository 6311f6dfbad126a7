"""Seeded call sequences of machines E and F on the device against the host models (tests/call_sequences_mixing.py), bit for bit: one case
per frozen (config, seed) of tests/test_call_sequences_mixing.py, each run once.  Arrays compare with np.array_equal, the viscosity
field (NaN in its never-read rows) on its bit patterns, scalars with ==, status codes exactly -- the refusals include/moka_hip.h
states are host-side argument checks that return before any launch, and what follows them shows that the state is unchanged.  A last
case per config asserts from the runner's counters that the sequences reached the paths they exist for."""
import pytest

import call_sequences_mixing as cm
import moka_hip as mk
from test_call_sequences_mixing import CASES, SEEDS

pytestmark = pytest.mark.gpu
_DEVICES = {}


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)          # raises MokaError if the HIP extension or the GPU is missing
    yield b
    for d in _DEVICES.values():
        d.close()
    _DEVICES.clear()
    b.close()


def device_of(backend, name):
    """One device mesh per config, shared by its seeds.  After a HIP error in any config nothing more is launched in any other."""
    dead = [d.dead for d in _DEVICES.values() if d.dead]
    if dead:
        pytest.fail("an earlier sequence ended in a HIP error, nothing more is launched: " + dead[0])
    if name not in _DEVICES:
        _DEVICES[name] = cm.device_of(backend, cm.ALL_CONFIGS[name])
    return _DEVICES[name]


@pytest.mark.parametrize("name,seed", CASES)
def test_sequence_matches_the_model_bit_for_bit(backend, name, seed):
    cfg = cm.ALL_CONFIGS[name]
    ops = cm.sequence_of(cfg, seed)
    expect = cm.model_of(cfg, seed).run(ops)
    got = device_of(backend, name).run(ops, seed)
    message = cm.first_mismatch(cfg, seed, ops, expect, got)
    assert message is None, message


@pytest.mark.parametrize("name", list(SEEDS))
def test_sequences_reached_what_they_exist_for(backend, name):
    """From the counters the runner keeps: RK4 and Forward-Euler steps; mixed steps with Cd in every config and with a field that is
    on wherever a field has an active interface (not E4); a moka_run of nine steps with each of them on; sweeps with D_cd flagged in
    every config and with DF flagged (E4 too: the flag is legal, DF stays zero); the forward and the reverse forms the config's table
    names -- both reverse forms in E1 (a step recorded with a field beside one without) and E3, both forward forms in E3 --; and single
    RK4 steps that took the stage 1 -> 2 hand-off beside single steps that did not, inside the same config, where the shape is one
    the default stage kernel carries (E1, E2: include/moka_hip.h, key 12); in E3 and E4 key 12 is toggled all the same and no step
    takes the hand-off.  Runs behind the config's sequences (a config whose sequences did not run has nothing to show and fails)."""
    cfg = cm.ALL_CONFIGS[name]
    cnt = device_of(backend, name).counters
    print(name, cnt)
    assert cnt["sequences"] == len(SEEDS[name]), "the sequences of this config come first"
    if name in cm.F_CONFIGS:
        # machine F: steps and a moka_run of nine steps with the closure on; the 16-stream form under it whatever key 7 says (and
        # key 7 was 1 in some of those steps); single steps under the closure that took the hand-off and that did not in F1, none in
        # F2 and F3, whose shapes the default stage kernel does not carry; the
        # tracers' vertical pass in the forms the config names, and the momentum pass launched, where the closure launches (K >= 2)
        assert cnt["rk4_steps"] > 0 and cnt["closure_steps"] > 0 and cnt["run9_closure"] > 0, "no step, or no run of nine, with the closure on"
        assert cnt["streams"] == {16}, cnt["streams"]
        assert cnt["key7_closure_steps"] > 0, "no step with the closure on ran while key 7 asked for the 13-stream form"
        assert cnt["no_handoff"] > 0 and (cnt["handoff"] > 0) == ("handoff" in cfg.reach), \
            "the single RK4 steps under the closure all took, or all missed, the hand-off (or took it on a shape that cannot)"
        for what in cfg.reach:
            if what != "handoff":
                assert int(what[-1]) in cnt["vpaths"], (what, cnt["vpaths"])
        if cfg.K > 1:
            assert cnt["paths"] - {0}, "the momentum pass never ran under the closure"
        return
    assert cnt["rk4_steps"] > 0 and cnt["fe_steps"] > 0 and cnt["sweeps"] > 0
    assert cnt["mixed_cd"] > 0 and cnt["run9_cd"] > 0, "no mixed step, or no moka_run of nine steps, with Cd != 0"
    if cfg.K > 1:
        assert cnt["mixed_field"] > 0 and cnt["run9_field"] > 0, "no mixed step, or no moka_run of nine steps, with a field that is on"
    assert cnt["sweeps_df"] > 0 and cnt["sweeps_dcd"] > 0, "no sweep of recorded steps with DF, or with D_cd, flagged"
    assert cnt["no_handoff"] > 0 and (cnt["handoff"] > 0) == ("handoff" in cfg.reach), \
        "the single RK4 steps all took, or all missed, the stage 1 -> 2 hand-off (or took it on a shape that cannot)"
    for what in cfg.reach:
        if what == "handoff":
            continue
        if what.startswith("ft_path_"):
            assert int(what[-1]) in cnt["ft_paths"], (what, cnt["ft_paths"])
        else:
            assert int(what[-1]) in cnt["paths"], (what, cnt["paths"])
