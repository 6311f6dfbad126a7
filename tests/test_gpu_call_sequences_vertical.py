"""Seeded call sequences of machines C and D on the device against the host models (tests/call_sequences_vertical.py), bit for
bit: one case per frozen (config, seed) of tests/test_call_sequences_vertical.py, each run once.  Arrays compare with
np.array_equal, scalars with ==, status codes exactly -- the refusals include/moka_hip.h states are host-side argument checks that
return before any launch, and what follows them shows that the state is unchanged.  A last case per config asserts from the
runner's counters that the sequences reached the paths they exist for."""
import pytest

import call_sequences_vertical as cv
import moka_hip as mk
from test_call_sequences_vertical import CASES, SEEDS

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
    """One device mesh per config, shared by its seeds."""
    if name not in _DEVICES:
        _DEVICES[name] = cv.device_of(backend, cv.ALL_CONFIGS[name])
    return _DEVICES[name]


@pytest.mark.parametrize("name,seed", CASES)
def test_sequence_matches_the_model_bit_for_bit(backend, name, seed):
    cfg = cv.ALL_CONFIGS[name]
    ops = cv.sequence_of(cfg, seed)
    expect = cv.model_of(cfg, seed).run(ops)
    got = device_of(backend, name).run(ops, seed)
    message = cv.first_mismatch(cfg, seed, ops, expect, got)
    assert message is None, message


@pytest.mark.parametrize("name", list(SEEDS))
def test_sequences_reached_what_they_exist_for(backend, name):
    """From the counters the runners keep.  Machine C: the momentum pass in the tile form (path 1) in C1, C2 and C3 and in the
    column form (path 2) in C3 and C4; the transposed pass likewise, both forms in C3; RK4 steps in the 13-stream form in C1; a
    moka_run of nine steps in that form (the captured graph's 6-step period) with the pass on in C1 and C2; a moka_run of nine steps
    accepted with the pass on in every C config.  Machine D: the tracers' vertical pass in the tile form in D1 and in both forms in
    D2, and at least one sweep with a vertical gradient flagged in each.  Runs behind the config's sequences (a config whose
    sequences did not run has nothing to show and fails)."""
    cfg = cv.ALL_CONFIGS[name]
    cnt = device_of(backend, name).counters
    print(name, cnt)
    assert cnt["sequences"] == len(SEEDS[name]), "the sequences of this config come first"
    if name in cv.D_CONFIGS:
        assert cnt["rk4_steps"] > 0 and cfg.tracer_path in cnt["tracer_paths"], cnt["tracer_paths"]
        assert cnt["vgrad_sweeps"] > 0, "no sweep with a vertical gradient flagged"
        for what in cfg.reach:
            assert int(what[-1]) in cnt["vpaths"], (what, cnt["vpaths"])
        return
    assert cnt["rk4_steps"] > 0 and cnt["fe_steps"] > 0 and cnt["mixed_steps"] > 0 and cnt["sweeps"] > 0
    assert cnt["run9_on"] > 0, "no moka_run of nine steps with the pass on"
    for what in cfg.reach:
        if what == "s13":
            assert cnt["s13"] > 0, "no RK4 step ran in the 13-stream form"
        elif what == "s13_run9":
            assert cnt["run9_s13_on"] > 0, "no moka_run of nine steps in the 13-stream form (the graph's 6-step period) with the pass on"
        elif what.startswith("ft_path_"):
            assert int(what[-1]) in cnt["ft_paths"], (what, cnt["ft_paths"])
        else:
            assert int(what[-1]) in cnt["paths"], (what, cnt["paths"])
