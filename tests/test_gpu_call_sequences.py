"""Seeded call sequences on the device against the host model (tests/call_sequences.py), bit for bit: one case per frozen
(config, seed) of tests/test_call_sequences.py, each run once.  Arrays compare with np.array_equal (both time levels included),
scalars with ==, status codes exactly -- the refusals include/moka_hip.h states are observations too, and what follows them shows
that the state is unchanged.  A last case per config asserts from the runner's counters that the sequences reached the paths they
exist for."""
import pytest

import call_sequences as cs
import moka_hip as mk
from test_call_sequences import CASES, SEEDS

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
        _DEVICES[name] = cs.device_of(backend, cs.CONFIGS[name])
    return _DEVICES[name]


@pytest.mark.parametrize("name,seed", CASES)
def test_sequence_matches_the_model_bit_for_bit(backend, name, seed):
    cfg = cs.CONFIGS[name]
    ops = cs.sequence(cfg, seed)
    expect = cs.model_of(cfg, seed).run(ops)
    got = device_of(backend, name).run(ops, seed)
    message = cs.first_mismatch(cfg, seed, ops, expect, got)
    assert message is None, message


@pytest.mark.parametrize("name", list(SEEDS))
def test_sequences_reached_what_they_exist_for(backend, name):
    """From the counters Device.run keeps: lean Forward-Euler steps pending at least once and both stage-kernel paths where the
    config's table says so, the generic path elsewhere, RK4 steps in the 13-stream form in A1 and A2, tracer path 1 in B1 and 2 in B2, forwards and backwards.  Runs behind the config's
    sequences (a config whose sequences did not run has nothing to show and fails)."""
    cfg = cs.CONFIGS[name]
    cnt = device_of(backend, name).counters
    print(name, cnt)
    assert cnt["sequences"] == len(SEEDS[name]), "the sequences of this config come first"
    if isinstance(cfg, cs.TracerConfig):
        assert cnt["rk4_steps"] > 0
        assert cfg.tracer_path in cnt["tracer_paths"], (cfg.tracer_path, cnt["tracer_paths"])
        assert cfg.tracer_path in cnt["adjoint_paths"], (cfg.tracer_path, cnt["adjoint_paths"])
        return
    assert cnt["fe_steps"] > 0 and cnt["rk4_steps"] > 0
    for what in cfg.reach:
        if what == "lean":
            assert cnt["lean"] > 0, "no Forward-Euler step left its arrays pending"
        elif what == "s13":
            assert cnt["s13"] > 0, "no RK4 step ran in the 13-stream form"
        else:
            assert int(what[-1]) in cnt["fe_paths"], (what, cnt["fe_paths"])
    if "lean" not in cfg.reach and not cfg.f32:
        assert cnt["lean"] == 0 and cnt["s13"] == 0
