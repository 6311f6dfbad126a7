"""CPU checks of the frozen call sequences (tests/call_sequences.py): conditions on the sequences, checked on the host model alone,
that keep tests/test_gpu_call_sequences.py from passing by not looking.

Seeds.  The generator's weights and the lists below were tuned until every condition holds (a greedy cover over the first few
hundred seeds of each config), then frozen; tests/test_gpu_call_sequences.py runs exactly these.  Changing the generator means tuning them again.

| Config | Shape | ops per sequence | slowest model run of a frozen sequence on the CPU |
|---|---|---|---|
| A1 | fp64, icosahedral m = 4 (162 cells, pentagons), K = 34, full columns | 30 | 0.05 s |
| A2 | fp64, periodic planar 6 x 4, K = 60, basin mask | 30 | 0.01 s |
| A3 | fp64, icosahedral m = 4 with two flipped edges (four heptagons, maxEdges 7), K = 5 | 30 | 0.02 s |
| A4 | fp64, periodic planar 4 x 4, K = 1 | 30 | 0.01 s |
| A5 | fp32 storage, icosahedral m = 4, K = 40 | 30 | 0.04 s |
| A6 | fp32 storage, periodic planar 4 x 6, K = 4 | 30 | 0.01 s |
| B1 | tracers, planar 20 x 18, K = 34, three tracers (the first is the unit tracer), 72-cell patches | 32 | 0.7 s |
| B2 | tracers, icosahedral m = 6 with three flipped edges (362 cells, heptagons), K = 6, five tracers | 34 | 0.7 s |

Which config cannot express which hazard (HAZARDS below): machine B cannot express stale_from_prev (no Forward Euler with tracers);
machine A has no tracer coefficients (coeff_late).  Every A config has Forward Euler with MOKA_FE_STALE_HEDGE (stale_from_prev),
uploads of ssh / layerThickness ahead of moka_tendencies (ssh_stored; the RK4 half of that mutant is Float64 only), steps followed by
reads of the previous level (prev_level_lost) and steps followed by an upload or advanceTimeLevels! and a read of Diag / Tend (late).
"""
import numpy as np
import pytest

import call_sequences as cs

SEEDS = {
    "A1": (18, 46, 107, 114, 139, 168, 197, 236, 308, 335, 379, 415, 482, 510),
    "A2": (0, 1, 2, 6, 14, 18, 23, 76, 87, 127, 146, 159, 171, 210),
    "A3": (1, 8, 11, 12, 24, 32, 35, 52, 68, 76, 99, 155, 181, 196),
    "A4": (5, 10, 13, 19, 32, 39, 40, 60, 74, 84, 123, 125, 137, 145, 152, 161, 181),
    "A5": (19, 27, 49, 59, 88, 125, 141, 195),
    "A6": (14, 16, 37, 39, 43, 89, 106, 143, 197),
    "B1": (4, 5, 18, 29, 30, 31, 56, 69, 71, 76, 85),
    "B2": (2, 8, 13, 15, 17, 22, 40, 45, 58, 67),
}
CASES = [(c, s) for c in SEEDS for s in SEEDS[c]]
# Which config can express which hazard.  Machine A has no tracer coefficients (coeff_late).  Machine B has no Forward Euler
# (stale_from_prev needs MOKA_FE_STALE_HEDGE); late shows there in TendencyVars read behind a toggle of the nonlinear terms.
HAZARDS = {name: (cs.B_MUTANTS if isinstance(cs.CONFIGS[name], cs.TracerConfig) else cs.MUTANTS) for name in SEEDS}
_RUNS = {}


def run_of(name, seed, mutant=None):
    """(ops, observations) of the model, computed once per (config, seed, mutant) and shared; no test modifies one."""
    key = (name, seed, mutant)
    if key not in _RUNS:
        cfg = cs.CONFIGS[name]
        ops = cs.sequence(cfg, seed)
        _RUNS[key] = (ops, cs.model_of(cfg, seed, mutant).run(ops))
    return _RUNS[key]


def same(a, b):
    if a.rc != b.rc:
        return False
    if isinstance(a.value, np.ndarray):
        return np.array_equal(a.value, b.value)
    return a.value == b.value


def is_read(op):
    return op.kind in cs.READ_KINDS + ("adj_download",) + cs.B_READS


def is_b(name):
    return isinstance(cs.CONFIGS[name], cs.TracerConfig)


A_NAMES = [n for n in SEEDS if not is_b(n)]


def test_every_config_has_at_least_eight_seeds():
    assert set(SEEDS) == set(cs.CONFIGS)
    for name, seeds in SEEDS.items():
        assert len(seeds) >= 8 and len(set(seeds)) == len(seeds), name


@pytest.mark.parametrize("name", list(SEEDS))
def test_sequences_and_model_are_deterministic(name):
    cfg = cs.CONFIGS[name]
    for seed in SEEDS[name][:3]:
        ops, obs = run_of(name, seed)
        assert ops == cs.sequence(cfg, seed) and len(ops) == cfg.nops
        again = cs.model_of(cfg, seed).run(ops)
        assert all(same(a, b) for a, b in zip(obs, again)) and len(obs) == len(again) == len(ops)
    assert cs.sequence(cfg, SEEDS[name][0]) != cs.sequence(cfg, SEEDS[name][1])


@pytest.mark.parametrize("name", list(SEEDS))
def test_every_admitted_op_kind_and_argument_class_occurs(name):
    """Every op kind the config admits occurs, and every argument class of it is ACCEPTED at least once (status MOKA_OK; a refused
    call shows nothing of the kind): each uploadable field and level, each kernel variant, each tuning key and value, placement with
    0, 1 and 2 tries, moka_run with each integrator, each set of Forward-Euler flags, Del4 off / on / on with a mesh scaling, each
    tracer count (0 included), each coefficient pattern and source mode."""
    cfg = cs.CONFIGS[name]
    kinds, classes = set(), set()
    for seed in SEEDS[name]:
        ops, obs = run_of(name, seed)
        kinds |= {op.kind for op in ops}
        classes |= {cs.arg_class(op) for op, o in zip(ops, obs) if o.rc == cs.OK}
    want = set((cs.b_vocabulary if is_b(name) else cs.vocabulary)(cfg))
    assert kinds == want, sorted(want ^ kinds)
    assert set(cs.arg_classes(cfg)) <= classes, sorted(set(cs.arg_classes(cfg)) - classes, key=str)


@pytest.mark.parametrize("name", list(SEEDS))
def test_every_writer_is_followed_by_a_first_read_of_every_kind(name):
    """Every admitted ordered pair (state-changing op kind, observing op kind) occurs with the observation being the FIRST read of
    that array since the op.  The op returned MOKA_OK, and either changed that array, or is one of call_sequences.NON_ARRAY_OPS
    (a tuning key, a variant, a placement search, a toggle, a coefficient, a tape op) that came while a change of the array was
    still unread.  Machine A: every writer with download, rows and sum_sq.  Machine B: what changes tracers, and what falls between,
    with moka_tracer_download; what changes the dycore with the three reads of it (call_sequences.pairs_wanted)."""
    seen = set()
    for seed in SEEDS[name]:
        ops, obs = run_of(name, seed)
        seen |= {(w, op.kind) for op, o in zip(ops, obs) if is_read(op) and o.rc == cs.OK for w in o.after}
    want = cs.pairs_wanted(cs.CONFIGS[name])
    assert want <= seen, sorted(want - seen)


@pytest.mark.parametrize("name", list(SEEDS))
def test_the_named_orders_of_calls_occur(name):
    """Orders the plan names and luck must not decide (call_sequences.cases_wanted): moka_tape_destroy while the last taped step's
    tendencies are pending, then a read of them; TendencyVars read behind a sweep; kappa, kappa4 and a source changed between two
    taped tracer steps; moka_set_tracers(st, 0) followed by a step of the dycore alone and a read."""
    cfg = cs.CONFIGS[name]
    seen = set()
    for seed in SEEDS[name]:
        seen |= cs.cases_seen(cfg, *run_of(name, seed))
    assert set(cs.cases_wanted(cfg)) <= seen, sorted(set(cs.cases_wanted(cfg)) - seen)


@pytest.mark.parametrize("name", list(SEEDS))
def test_every_stated_refusal_is_predicted(name):
    seen = {o.refusal for seed in SEEDS[name] for o in run_of(name, seed)[1] if o.refusal}
    want = set((cs.b_refusals if is_b(name) else cs.refusals)(cs.CONFIGS[name]))
    assert seen >= want, sorted(want - seen)
    for seed in SEEDS[name]:
        assert all(o.rc != cs.OK for o in run_of(name, seed)[1] if o.refusal)


@pytest.mark.parametrize("name", list(SEEDS))
@pytest.mark.parametrize("mutant", cs.MUTANTS + ("coeff_late",))
def test_every_mutant_is_killed(name, mutant):
    """Teeth: each mutant of the model -- the bug one flag of the library's state machine exists to prevent -- differs from the true
    model in at least one observation of at least one frozen sequence of every config that can express the hazard."""
    cfg = cs.CONFIGS[name]
    if mutant not in HAZARDS[name]:
        return
    killed = [seed for seed in SEEDS[name]
              if not all(same(a, b) for a, b in zip(run_of(name, seed)[1], run_of(name, seed, mutant)[1]))]
    assert killed, f"mutant {mutant} survives every sequence of {name}: the generator is at fault"


@pytest.mark.parametrize("name", list(SEEDS))
def test_no_observation_counts_the_same_bits_twice(name):
    """Every array or scalar a sequence reads has changed since the sequence last read it (the uploads before the first op are
    never read back on their own): the device comparison never counts the same bits twice."""
    reads = 0
    for seed in SEEDS[name]:
        ops, obs = run_of(name, seed)
        for i, (op, o) in enumerate(zip(ops, obs)):
            if is_read(op) and o.rc == cs.OK:
                if o.key[0] in ("X", "G", "W"):
                    continue                            # tape outputs: each is read once behind its sweep
                assert o.fresh and o.after, f"{name} seed {seed}: op {i} ({op}) reads an array that has not changed since its last read"
                reads += 1
    assert reads >= 5 * len(SEEDS[name])


def test_the_triage_entry_point_prints_a_sequence(capsys):
    assert cs.main(["A4", str(SEEDS["A4"][0]), "--upto", "5"]) == 0
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 6 and out[0].startswith(" 0 ")
    assert cs.main(["nope"]) == 2
