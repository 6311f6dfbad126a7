"""CPU checks of the frozen call sequences of machines C and D (tests/call_sequences_vertical.py): conditions on the sequences,
checked on the host model alone, that keep tests/test_gpu_call_sequences_vertical.py from passing by not looking.

Seeds.  The generator's weights and the lists below were tuned until every condition holds (a greedy cover of `tokens_wanted` over
the first 150 to 300 seeds of each config, keeping only seeds whose every read is a first read), then frozen;
tests/test_gpu_call_sequences_vertical.py runs exactly these.  Changing a generator means tuning them again.

| Config | Shape | ops per sequence | slowest model run of a frozen sequence on the CPU |
|---|---|---|---|
| C1 | fp64, icosahedral m = 4 (162 cells, 480 edges), K = 34, full columns | 36 | 0.08 s |
| C2 | fp64, periodic planar 6 x 4 (72 edges), K = 60, edges of depth 0, 1 and 7 .. 60 | 36 | 0.12 s |
| C3 | fp64, icosahedral m = 4 with two flipped edges (heptagons), K = 5, variants 0 and 3 | 36 | 0.03 s |
| C4 | fp64, periodic planar 4 x 4 (48 edges), K = 1 | 36 | 0.01 s |
| D1 | tracers, planar 20 x 18, K = 34 over a sea floor (tracer_vmix_twin.column_mlt), three tracers, 72-cell patches | 36 | 0.7 s |
| D2 | tracers, icosahedral m = 6 with three flipped edges (362 cells), K = 6, five tracers, variants 0 and 3 | 36 | 0.4 s |

Which config cannot express which hazard (HAZARDS below): n1_always needs wet columns of one level, which only C2 (a band of
edges with n == 1) and C4 (K = 1) have; every other mutant of machine C is killed in every C config, every mutant of machine D in
both D configs.
"""
import numpy as np
import pytest

import call_sequences as cs
import call_sequences_vertical as cv
from test_call_sequences import same

SEEDS = {
    "C1": (1, 13, 22, 48, 54, 65, 70, 124, 129, 175, 177, 183, 217, 240, 281),
    "C2": (15, 27, 33, 50, 67, 91, 104, 112, 126, 144, 156, 176, 185, 202, 248, 265),
    "C3": (1, 6, 7, 31, 35, 44, 72, 78, 127, 128, 276, 286),
    "C4": (3, 7, 14, 23, 27, 35, 65, 70, 74, 95, 106, 110, 119, 121, 165, 241, 277),
    "D1": (5, 10, 15, 16, 18, 19, 71, 80, 97, 135, 138),
    "D2": (3, 6, 7, 15, 16, 20, 26, 100, 102, 148),
}
CASES = [(c, s) for c in SEEDS for s in SEEDS[c]]
HAZARDS = {name: cv.D_MUTANTS if name in cv.D_CONFIGS else tuple(m for m in cv.C_MUTANTS if m != "n1_always" or name in ("C2", "C4"))
           for name in SEEDS}
READS = cs.READ_KINDS + ("adj_download", "tr_download")
TAPE_READS = cv.FT_READS + cv.D_TAPE_READS
C_NAMES = [n for n in SEEDS if n in cv.V_CONFIGS]
_RUNS = {}


def is_d(name):
    return name in cv.D_CONFIGS


def run_of(name, seed, mutant=None):
    """(ops, observations) of the model, computed once per (config, seed, mutant) and shared; no test modifies one."""
    key = (name, seed, mutant)
    if key not in _RUNS:
        cfg = cv.ALL_CONFIGS[name]
        ops = cv.sequence_of(cfg, seed)
        _RUNS[key] = (ops, cv.model_of(cfg, seed, mutant).run(ops))
    return _RUNS[key]


def stale_reads(name, seed):
    """The reads of a sequence that count the same bits twice: (index, op) of every accepted read of an array that has not changed
    since its last read."""
    ops, obs = run_of(name, seed)
    return [(i, op) for i, (op, o) in enumerate(zip(ops, obs)) if op.kind in READS and o.rc == cs.OK and not (o.fresh and o.after)]


def tokens_of(name, seed, mutants=True):
    """Everything one sequence contributes to the conditions below, as a set of tokens."""
    cfg = cv.ALL_CONFIGS[name]
    ops, obs = run_of(name, seed)
    t = {("kind", op.kind) for op in ops}
    t |= {("class", (cv.d_arg_class if is_d(name) else cv.arg_class)(op)) for op, o in zip(ops, obs) if o.rc == cs.OK}
    for op, o in zip(ops, obs):
        if op.kind in READS and o.rc == cs.OK:
            t |= {("pair", w, op.kind) for w in o.after} | {("any", w) for w in o.after}
    t |= {("case", c) for c in (cv.d_cases_seen if is_d(name) else cv.cases_seen)(cfg, ops, obs)}
    later_read = False
    for op, o in reversed(list(zip(ops, obs))):
        if o.refusal:
            t.add(("refusal", o.refusal))
            if later_read:
                t.add(("refusal_then_read", o.refusal))
        later_read = later_read or (op.kind in READS + TAPE_READS and o.rc == cs.OK)
    if mutants:
        for m in HAZARDS[name]:
            if not all(same(a, b) for a, b in zip(obs, run_of(name, seed, m)[1])):
                t.add(("kill", m))
    return t


def tokens_wanted(name):
    cfg = cv.ALL_CONFIGS[name]
    if is_d(name):
        pairs, writers, voc, classes = cv.d_pairs_wanted(cfg), (), cv.d_vocabulary(cfg), cv.d_arg_classes(cfg)
        cases, refused = cv.d_cases_wanted(cfg), cv.d_refusals(cfg)
    else:
        (pairs, writers), voc, classes = cv.pairs_wanted(cfg), cv.vocabulary(cfg), cv.arg_classes(cfg)
        cases, refused = cv.cases_wanted(cfg), cv.refusals(cfg)
    t = {("kind", k) for k in voc} | {("class", c) for c in classes}
    t |= {("pair",) + p for p in pairs} | {("any", w) for w in writers} | {("case", c) for c in cases}
    t |= {(k, r) for r in refused for k in ("refusal", "refusal_then_read")} | {("kill", m) for m in HAZARDS[name]}
    return t


def seen(name, what):
    return {t[1:] for seed in SEEDS[name] for t in tokens_of(name, seed, mutants=what == "kill") if t[0] == what}


def wanted(name, what):
    return {t[1:] for t in tokens_wanted(name) if t[0] == what}


def test_every_config_has_at_least_eight_seeds():
    assert set(SEEDS) == set(cv.ALL_CONFIGS) and not set(SEEDS) & set(cs.CONFIGS)
    for name, seeds in SEEDS.items():
        assert len(seeds) >= 8 and len(set(seeds)) == len(seeds), name


FROZEN_CRC = {"C1": 0x60d9ec68, "C2": 0x2505400b, "C3": 0x52738ccc, "C4": 0xbd8ae4fd, "D1": 0x0634678a, "D2": 0x703ac9e3}


@pytest.mark.parametrize("name", list(SEEDS))
def test_the_frozen_sequences_are_the_ones_the_seeds_were_tuned_for(name):
    """crc32 over str(op) of every op of every frozen sequence of a config: a change of a generator that moves a sequence shows here
    first (tune the seeds again, then update the value)."""
    crc = 0
    for seed in SEEDS[name]:
        for op in run_of(name, seed)[0]:
            crc = cs.zlib.crc32(str(op).encode(), crc)
    assert crc == FROZEN_CRC[name], f"{name}: {crc:#010x}"


@pytest.mark.parametrize("name", C_NAMES)
def test_each_config_has_the_edge_depths_it_states(name):
    """From the masks: C1, C3, C4 full columns, C2 land, a band of one level and deeper columns; and the forms the K's take: the
    forward tile form for 2 <= K <= 105, reverse tiles of 64 columns for K <= 19 and of 32 for K <= 79, the column form for K = 1 and
    under variant 3."""
    import momentum_vmix_twin as mv
    from tracer_vgrad_twin import tile_columns_grad
    cfg = cv.V_CONFIGS[name]
    n = cv.depths_of(cfg)
    assert n.shape == (cs.get_mesh(cfg.meshname).nEdges,)
    if name == "C2":
        assert (n == 0).any() and (n == 1).any() and ((n > 1) & (n < cfg.K)).any() and (n == cfg.K).any()
        tau = cv.stress_values(cfg, "n0")
        assert np.any(tau != 0.0) and not mv.stress_on(tau, n)
    else:
        assert np.all(n == cfg.K) and cv.mask_of(cfg) is None
    assert mv.stress_on(cv.stress_values(cfg, "field"), n) and not mv.stress_on(cv.stress_values(cfg, "zero"), n)
    assert (cfg.K, mv.form_of(cfg.K), mv.form_of(cfg.K, True), tile_columns_grad(cfg.K), tile_columns_grad(cfg.K, True)) == \
        {"C1": (34, 1, 2, 32, 0), "C2": (60, 1, 2, 32, 0), "C3": (5, 1, 2, 64, 0), "C4": (1, 2, 2, 0, 0)}[name]
    assert cs.get_mesh(cfg.meshname).nCells <= 400


@pytest.mark.parametrize("name", list(SEEDS))
def test_sequences_and_model_are_deterministic(name):
    cfg = cv.ALL_CONFIGS[name]
    for seed in SEEDS[name][:3]:
        ops, obs = run_of(name, seed)
        assert ops == cv.sequence_of(cfg, seed) and len(ops) == cfg.nops
        again = cv.model_of(cfg, seed).run(ops)
        assert all(same(a, b) for a, b in zip(obs, again)) and len(obs) == len(again) == len(ops)
    assert cv.sequence_of(cfg, SEEDS[name][0]) != cv.sequence_of(cfg, SEEDS[name][1])


@pytest.mark.parametrize("name", list(SEEDS))
def test_every_admitted_op_kind_and_argument_class_occurs(name):
    """Every op kind occurs, and every argument class is ACCEPTED at least once: each visc and stress pattern, each step with dt and
    with 0.0, moka_run with three and with nine steps and with Forward Euler, each variant, both values of key 8, placement with 0 and
    1 tries, each uploadable field and level, each of the three reads of each of the twelve arrays, each gradient bit flagged and
    unflagged, both adjoint fields, each density and each scalar gradient."""
    assert seen(name, "kind") == wanted(name, "kind"), sorted(seen(name, "kind") ^ wanted(name, "kind"))
    assert wanted(name, "class") <= seen(name, "class"), sorted(wanted(name, "class") - seen(name, "class"), key=str)


@pytest.mark.parametrize("name", list(SEEDS))
def test_every_writer_is_followed_by_a_first_read_of_every_kind(name):
    """Every pair (op of call_sequences_vertical.WRITERS_EVERY_READ, read kind) occurs with the observation being the FIRST read of
    that array since the op, which returned MOKA_OK and either changed the array or (visc, stress, a variant) came while a change of
    it was still unread; every op of WRITERS_ANY_READ occurs so with at least one kind of read."""
    assert wanted(name, "pair") <= seen(name, "pair"), sorted(wanted(name, "pair") - seen(name, "pair"))
    assert wanted(name, "any") <= seen(name, "any"), sorted(wanted(name, "any") - seen(name, "any"))


@pytest.mark.parametrize("name", list(SEEDS))
def test_the_named_orders_of_calls_occur(name):
    """call_sequences_vertical.cases_wanted: the first read of each Diag and Tend array behind a step in which the pass ran, through
    each read kind; visc or stress changed between such a step and those reads; visc changed, and a stress uploaded and removed,
    between two runs of nine steps; the forced tape destroyed, or swept, while its last step's tendencies are pending, then a read of
    them; values changed between two forced taped steps, one of them with the pass off, then a sweep with all three gradients
    flagged; a variant switch between a forced taped step and its sweep; the pass switched off, a Forward-Euler step, both levels
    read; a dt == 0.0 step with the pass on, then a read."""
    assert wanted(name, "case") <= seen(name, "case"), sorted(wanted(name, "case") - seen(name, "case"), key=str)


@pytest.mark.parametrize("name", list(SEEDS))
def test_every_stated_refusal_is_predicted_and_followed_by_a_read(name):
    assert wanted(name, "refusal") <= seen(name, "refusal"), sorted(wanted(name, "refusal") - seen(name, "refusal"))
    assert wanted(name, "refusal_then_read") <= seen(name, "refusal_then_read")
    for seed in SEEDS[name]:
        assert all(o.rc != cs.OK for o in run_of(name, seed)[1] if o.refusal)


@pytest.mark.parametrize("name", list(SEEDS))
def test_every_mutant_is_killed(name):
    """Teeth: each mutant of the model differs from the true model in at least one observation of at least one frozen sequence of
    every config that can express it."""
    assert wanted(name, "kill") <= seen(name, "kill"), sorted(wanted(name, "kill") - seen(name, "kill"))


@pytest.mark.parametrize("name", list(SEEDS))
def test_no_observation_counts_the_same_bits_twice(name):
    reads = 0
    for seed in SEEDS[name]:
        assert not stale_reads(name, seed), (name, seed, stale_reads(name, seed))
        reads += sum(op.kind in READS and o.rc == cs.OK for op, o in zip(*run_of(name, seed)))
    assert reads >= 5 * len(SEEDS[name])


def test_the_triage_entry_point_prints_a_sequence(capsys):
    assert cv.main(["C2", str(SEEDS["C2"][0]), "--upto", "5"]) == 0
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 6 and out[0].startswith(" 0 ")
    assert cv.main(["nope"]) == 2
