"""CPU checks of the frozen call sequences of machines E and F (tests/call_sequences_mixing.py): conditions on the sequences, checked on the
host model alone, that keep tests/test_gpu_call_sequences_mixing.py from passing by not looking.

Seeds.  The generator's weights and the lists below were tuned until every condition holds (a greedy cover of `tokens_wanted` over
the first 240 seeds of each config, keeping only seeds whose every read is a first read), then frozen;
tests/test_gpu_call_sequences_mixing.py runs exactly these.  Changing the generator means tuning them again.

| Config | Shape | ops per sequence | slowest model run of a frozen sequence on the CPU |
|---|---|---|---|
| E1 | fp64, icosahedral m = 4 (162 cells, 480 edges), K = 64, full columns | 36 | 0.22 s |
| E2 | fp64, periodic planar 6 x 4 (72 edges), K = 60, edges of depth 0, 1 and 7 .. 60 | 36 | 0.32 s |
| E3 | fp64, icosahedral m = 4 with two flipped edges (heptagons), K = 5, variants 0 and 3 | 36 | 0.04 s |
| E4 | fp64, periodic planar 4 x 4 (48 edges), K = 1 | 36 | 0.02 s |
| F1 | tracers, periodic planar 6 x 4, K = 60, edges of depth 0, 1 and 7 .. 60, three tracers | 44 | 0.85 s |
| F2 | tracers, icosahedral m = 6 with three flipped edges (362 cells), K = 6, five tracers, variants 0 and 3 | 44 | 1.0 s |
| F3 | tracers, periodic planar 4 x 4, K = 1, two tracers | 44 | 0.11 s |

Which config cannot express which hazard: the table CANNOT below names, per mutant, the configs and the reason; HAZARDS is derived
from it, and every other mutant is killed in every config of its machine.
"""
import numpy as np
import pytest

import call_sequences as cs
import call_sequences_mixing as cm
import call_sequences_vertical as cv
from test_call_sequences import same

SEEDS = {
    "E1": (2, 15, 21, 39, 61, 84, 98, 107, 138, 147, 148, 152, 174, 182, 230),
    "E2": (0, 2, 4, 21, 22, 28, 31, 47, 71, 86, 90, 92, 95, 166, 182, 206),
    "E3": (5, 6, 19, 20, 26, 27, 31, 42, 60, 65, 85, 126, 169, 170, 182, 229),
    "E4": (11, 42, 52, 53, 56, 79, 92, 111, 131, 181, 217, 226, 228, 229),
    "F1": (25, 40, 48, 49, 61, 105, 133, 186, 193),
    "F2": (0, 21, 37, 51, 58, 60, 76, 124, 184),
    "F3": (16, 22, 28, 36, 70, 93, 102, 105, 136, 159),
}
CASES = [(c, s) for c in SEEDS for s in SEEDS[c]]
KINK_CONFIGS = ("E4",)
FIELD_MUTANTS = ("scalar_lost", "zero_field_transparent", "field_late", "tape_field_newest")
# mutant -> (the configs that cannot express it, why)
CANNOT = {
    "cd_skips_n1": (("E1", "E3"), "needs wet columns of one level: a band of edges with n == 1 (E2) or K = 1 (E4)"),
    "scalar_lost": (("E4",), "needs a field with an active interface; at K = 1 a field is present and counts as zero"),
    "zero_field_transparent": (("E4",), "at K = 1 nuV alone launches nothing, under a field or not"),
    "field_late": (("E4",), "at K = 1 no entry of a field is ever read"),
    "tape_field_newest": (("E4",), "at K = 1 no field is ever on, so no copy is taken"),
    "kink_divides": (("E1", "E2", "E3"), "needs u* == 0 exactly behind stage 4: only where the column sum has one term (KINK_CONFIGS, asserted below)"),
    # machine F.  F3 (K = 1): the closure is on and launches nothing, so nothing of F, G or the masks reaches an observation
    "rich_late": (("F3",), "K = 1: the closure launches nothing whatever its parameters"),
    "rich_from_mixed": (("F3",), "K = 1: F and G read zero"),
    "fields_stale": (("F3",), "K = 1: F and G read zero, always"),
    "mask_ignored": (("F3",), "K = 1: no tracer takes G"),
    "levels_swapped": (("F3",), "K = 1: moka_richardson_diagnose answers zeros for both levels"),
    "aside_lost": (("F3",), "K = 1: the set-aside viscosity and diffusivities launch nothing either"),
    "setter_dropped": (("F3",), "K = 1: as aside_lost; the getters are not part of the mutant"),
    "coeff_late": (("F3",), "K = 1: no vertical coefficient reaches the arithmetic"),
    # (mixed_flow_early is expressible in all of F1-F3: at K = 1 drag, Cd or a stress still mix the flow the tracers' stage 4 would read)
}
MUTANTS_OF = {"E": cm.E_MUTANTS, "F": cm.F_MUTANTS}
HAZARDS = {name: tuple(m for m in MUTANTS_OF[name[0]] if name not in CANNOT.get(m, ((),))[0]) for name in SEEDS}
READS = cs.READ_KINDS + ("tr_download",)
TAPE_READS = cm.FT_READS + ("rich_fields", "rich_diag", "rich_read")
E_NAMES = [n for n in SEEDS if n in cm.E_CONFIGS]


def is_f(name):
    return name in cm.F_CONFIGS
_RUNS = {}


def run_of(name, seed, mutant=None):
    """(ops, observations) of the model, computed once per (config, seed, mutant) and shared; no test modifies one."""
    key = (name, seed, mutant)
    if key not in _RUNS:
        cfg = cm.ALL_CONFIGS[name]
        ops = cm.sequence_of(cfg, seed)
        _RUNS[key] = (ops, cm.model_of(cfg, seed, mutant).run(ops))
    return _RUNS[key]


def stale_reads(name, seed):
    """The reads of a sequence that count the same bits twice: (index, op) of every accepted read of an array that has not changed
    since its last read."""
    ops, obs = run_of(name, seed)
    return [(i, op) for i, (op, o) in enumerate(zip(ops, obs)) if op.kind in READS and o.rc == cs.OK and not (o.fresh and o.after)]


def tokens_of(name, seed, mutants=True):
    """Everything one sequence contributes to the conditions below, as a set of tokens."""
    cfg = cm.ALL_CONFIGS[name]
    ops, obs = run_of(name, seed)
    t = {("kind", op.kind) for op in ops}
    t |= {("class", (cm.f_arg_class if is_f(name) else cm.arg_class)(op)) for op, o in zip(ops, obs) if o.rc == cs.OK}
    for op, o in zip(ops, obs):
        if op.kind in READS and o.rc == cs.OK:
            t |= {("pair", w, op.kind) for w in o.after} | {("any", w) for w in o.after}
    t |= {("case", c) for c in (cm.f_cases_seen if is_f(name) else cm.cases_seen)(cfg, ops, obs)}
    later_read = False
    for op, o in reversed(list(zip(ops, obs))):
        if o.refusal:
            for r in {o.refusal} | {b for b in cm.CAUSE_REFUSALS if o.refusal.startswith(b + "_") and o.refusal[len(b) + 1:] in ("cd", "field")}:
                t.add(("refusal", r))
                if later_read:
                    t.add(("refusal_then_read", r))
        later_read = later_read or (op.kind in READS + TAPE_READS and o.rc == cs.OK)
    if mutants:
        for m in HAZARDS[name]:
            if not all(same(a, b) for a, b in zip(obs, run_of(name, seed, m)[1])):
                t.add(("kill", m))
    return t


def tokens_wanted(name):
    cfg = cm.ALL_CONFIGS[name]
    if is_f(name):
        (pairs, writers), voc, classes = cm.f_pairs_wanted(cfg), cm.f_vocabulary(cfg), cm.f_arg_classes(cfg)
        cases, refused = cm.f_cases_wanted(cfg), cm.f_refusals(cfg)
    else:
        (pairs, writers), voc, classes = cm.pairs_wanted(cfg), cm.vocabulary(cfg), cm.arg_classes(cfg)
        cases, refused = cm.cases_wanted(cfg), cm.refusals(cfg)
    t = {("kind", k) for k in voc} | {("class", c) for c in classes}
    t |= {("pair",) + p for p in pairs} | {("any", w) for w in writers} | {("case", c) for c in cases}
    t |= {(k, r) for r in refused for k in ("refusal", "refusal_then_read")} | {("kill", m) for m in HAZARDS[name]}
    return t


def seen(name, what):
    return {t[1:] for seed in SEEDS[name] for t in tokens_of(name, seed, mutants=what == "kill") if t[0] == what}


def wanted(name, what):
    return {t[1:] for t in tokens_wanted(name) if t[0] == what}


def test_every_config_has_at_least_eight_seeds():
    assert set(SEEDS) == set(cm.ALL_CONFIGS) and not set(SEEDS) & (set(cs.CONFIGS) | set(cv.ALL_CONFIGS))
    for name, seeds in SEEDS.items():
        assert len(seeds) >= 8 and len(set(seeds)) == len(seeds), name


FROZEN_CRC = {"E1": 0xce7b7467, "E2": 0x01105cee, "E3": 0x5407dfb6, "E4": 0xded04285, "F1": 0xad4ba95d, "F2": 0xff722878, "F3": 0x7e69af31}


@pytest.mark.parametrize("name", list(SEEDS))
def test_the_frozen_sequences_are_the_ones_the_seeds_were_tuned_for(name):
    """crc32 over str(op) of every op of every frozen sequence of a config: a change of the generator that moves a sequence shows here
    first (tune the seeds again, then update the value)."""
    crc = 0
    for seed in SEEDS[name]:
        for op in run_of(name, seed)[0]:
            crc = cs.zlib.crc32(str(op).encode(), crc)
    assert crc == FROZEN_CRC[name], f"{name}: {crc:#010x}"


@pytest.mark.parametrize("name", E_NAMES)
def test_each_config_has_the_shape_it_states(name):
    """From the masks and the twins' restatement of the kernel selection: E1, E3, E4 full columns, E2 land, a band of one level and
    deeper columns next to each other; the forward tile form for 2 <= K <= 105 and the column form for K = 1 and under variant 3; in
    reverse E1 takes 32-column tiles for a step recorded without a field and the column form for one recorded with a field, E3 tiles
    of 64 columns either way, E2 tiles of 32; the fields' never-read rows hold NaN and the invalid patterns are invalid at an active
    row only."""
    import momentum_vfield_twin as mf
    import momentum_vmix_twin as mv
    cfg = cm.E_CONFIGS[name]
    n = cv.depths_of(cfg)
    mesh = cs.get_mesh(cfg.meshname)
    assert n.shape == (mesh.nEdges,) and mesh.nCells <= 400
    if name == "E2":
        assert (n == 0).any() and (n == 1).any() and ((n > 1) & (n < cfg.K)).any() and (n == cfg.K).any()
        c1, c2 = mv.edge_cells(mesh)
        eoc = np.asarray(mesh.edgesOnCell, dtype=np.int64) - 1
        depths = [{int(n[e]) for c in (c1[i], c2[i]) for e in eoc[c, :mesh.nEdgesOnCell[c]]} for i in range(mesh.nEdges)]
        assert any(len(d - {0}) > 1 for d in depths), "no stencil of the bottom speed sees two bottom levels"
    else:
        assert np.all(n == cfg.K) and cv.mask_of(cfg) is None
    assert (cfg.K, mv.form_of(cfg.K), mv.form_of(cfg.K, True), mf.adjoint_form(cfg.K, False), mf.adjoint_form(cfg.K, True),
            mf.adjoint_form(cfg.K, True, True)[0]) == \
        {"E1": (64, 1, 2, (1, 32), (2, 0), 2), "E2": (60, 1, 2, (1, 32), (1, 32), 2), "E3": (5, 1, 2, (1, 64), (1, 64), 2),
         "E4": (1, 2, 2, (2, 0), (2, 0), 2)}[name]
    assert int(np.asarray(mesh.edgesOnCell).shape[1]) == (7 if name == "E3" else 6)
    live = mf.live_of(n, cfg.K)
    for p in ("A", "B", "eqnu"):
        f = cm.field_values(cfg, p)
        assert np.all(np.isnan(f[~live])) and mf.check_field(f, n) and mf.field_on(f, n) == (cfg.K > 1)
    assert not mf.field_on(cm.field_values(cfg, "zero"), n) and live.any() == (cfg.K > 1)
    if cfg.K > 1:
        a = cm.field_values(cfg, "A")
        assert np.any(a[live] == 0.0) and not np.array_equal(a[live], cm.field_values(cfg, "B")[live])
        assert np.all(cm.field_values(cfg, "eqnu")[live] == cv.visc_values(cfg, "nu")[0])
        for p in cm.FIELD_BAD:
            assert not mf.check_field(cm.field_values(cfg, p), n)
    c = [cm.cd_values(cfg, p) for p in cm.CD_OK]
    assert c[0] == 0.0 and 0.0 < c[2] < c[1]


@pytest.mark.parametrize("name", E_NAMES)
def test_the_kink_is_reachable_exactly_where_hazards_says(name):
    """Zero normalVelocity over the resting thickness: u* == 0 exactly behind an RK4 step (and with it sp == 0 at every edge) in the
    configs of KINK_CONFIGS and only there."""
    cfg = cm.E_CONFIGS[name]
    m = cm.model_of(cfg, 0)
    m.run([cm.Op("upload_rest_h"), cm.Op("upload_zero_u"), cm.Op("rk4", (1.0,))])
    assert (not np.any(m.st.u[1])) == (name in KINK_CONFIGS)


@pytest.mark.parametrize("name", list(SEEDS))
def test_sequences_and_model_are_deterministic(name):
    cfg = cm.ALL_CONFIGS[name]
    for seed in SEEDS[name][:3]:
        ops, obs = run_of(name, seed)
        assert ops == cm.sequence_of(cfg, seed) and len(ops) == cfg.nops
        again = cm.model_of(cfg, seed).run(ops)
        assert all(same(a, b) for a, b in zip(obs, again)) and len(obs) == len(again) == len(ops)
    assert cm.sequence_of(cfg, SEEDS[name][0]) != cm.sequence_of(cfg, SEEDS[name][1])


@pytest.mark.parametrize("name", list(SEEDS))
def test_every_admitted_op_kind_and_argument_class_occurs(name):
    """Every op kind occurs, and every argument class is ACCEPTED at least once: each visc, stress, field and Cd pattern, a step with dt
    and with 0.0, moka_run with three and with nine steps and with Forward Euler, each variant, both values of keys 8 and 12, each of
    the three reads of a Prog, a Diag and a Tend array, moka_bottom_speed of both levels, both adjoint fields, the DF and the D_cd
    flag set and cleared."""
    assert seen(name, "kind") == wanted(name, "kind"), sorted(seen(name, "kind") ^ wanted(name, "kind"))
    assert wanted(name, "class") <= seen(name, "class"), sorted(wanted(name, "class") - seen(name, "class"), key=str)


@pytest.mark.parametrize("name", list(SEEDS))
def test_every_writer_is_followed_by_a_first_read_of_every_kind(name):
    """Every pair (op of call_sequences_mixing.WRITERS_EVERY_READ, read kind) occurs with the observation being the FIRST read of that
    array since the op, which returned MOKA_OK and changed the array; every op of WRITERS_ANY_READ occurs so with at least one kind of
    read, having changed the array or (a coefficient, a variant, a tape call) come while a change of it was still unread."""
    assert wanted(name, "pair") <= seen(name, "pair"), sorted(wanted(name, "pair") - seen(name, "pair"))
    assert wanted(name, "any") <= seen(name, "any"), sorted(wanted(name, "any") - seen(name, "any"))


@pytest.mark.parametrize("name", list(SEEDS))
def test_the_named_orders_of_calls_occur(name):
    """call_sequences_mixing.cases_wanted: a field uploaded, a mixed step, the field removed, a mixed step with nuV acting again, a
    read of normalVelocity; an all-zero field over nuV != 0, a step, a read; the field equal to nuV, a mixed step, a read; a field or
    Cd changed between two runs of nine steps; Cd set, a launched step, moka_bottom_speed_download, a launched step without Cd, the
    download returning zeros; moka_bottom_speed of level 0 and of level 1 behind one step; on a quadratic tape with D_cd flagged steps
    recorded with Cd == 0 and with two other Cd's, a sweep, the density; on a tape with DF flagged a step with a field, one after its
    removal, one after another upload, a sweep, DF; a field upload accepted and a stress upload refused while steps are recorded; a
    sweep, a recorded step, a seed, a sweep, a density; moka_forced_tape_device_arrays growing across a recorded step, and 0 on a
    quadratic tape whose recorded step saw no Cd, no flag and no pass; zeros uploaded to normalVelocity, a recorded step with Cd != 0,
    a sweep; key 12 toggled between two single RK4 steps with a read behind each; in E3 launched steps, and sweeps of a launched
    record, under variant 0 and under variant 3.  call_sequences_mixing.f_cases_wanted: the closure on, a step, off, a step with a
    set-aside coefficient acting again, on again, a step; a setter of a set-aside coefficient accepted while the closure is on, the
    closure off, a step; the parameters switched between two runs of nine steps; the fields download behind a step without the
    closure (zeros) and behind a dt == 0.0 step; moka_richardson_diagnose of level 0 and of level 1 behind one step, differing;
    moka_set_tracers while on, the diagnosis refused, the closure on again; a mask that leaves one tracer on its scalar and one on
    its field; the unit tracer as buoyancy; the closure refused beside a tracer tape, the tape destroyed, the closure accepted; key
    7 or 12 toggled between two steps with the closure on; drag, Cd or a stress in force under the closure."""
    assert wanted(name, "case") <= seen(name, "case"), sorted(wanted(name, "case") - seen(name, "case"), key=str)


@pytest.mark.parametrize("name", list(SEEDS))
def test_every_stated_refusal_is_predicted_and_followed_by_a_read(name):
    assert wanted(name, "refusal") <= seen(name, "refusal"), sorted(wanted(name, "refusal") - seen(name, "refusal"))
    assert wanted(name, "refusal_then_read") <= seen(name, "refusal_then_read"), \
        sorted(wanted(name, "refusal_then_read") - seen(name, "refusal_then_read"))
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


def test_the_closure_meets_all_three_branches():
    """richardson_twin.census over the steps of the frozen sequences of F1 and F2 that launch the closure (the edge recipe on u*, h_new
    and phi*_jb, from the twin alone): live interfaces with Ri > 0, with db == 0, and with db < 0."""
    shares = []
    for name in ("F1", "F2"):
        cfg = cm.ALL_CONFIGS[name]
        for seed in SEEDS[name]:
            m = cm.model_of(cfg, seed)
            m.census = []
            m.run(cm.sequence_of(cfg, seed))
            shares += m.census
    assert shares, "no step launched the closure"
    pos, zero, neg = (max(s[i] for s in shares) for i in range(3))
    print(f"largest shares over {len(shares)} steps: Ri > 0 {pos:.3f}, db == 0 {zero:.3f}, db < 0 {neg:.3f}")
    assert pos > 0.0 and zero > 0.0 and neg > 0.0


@pytest.mark.parametrize("name", list(SEEDS))
def test_the_hand_off_is_expected_where_the_default_stage_kernel_carries_the_shape(name):
    """`reach` names "handoff" exactly for the shapes call_sequences.Config.s13 documents for the default stage kernel (an even
    34 <= nVertLevels <= 64), which is what moka_set_tuning key 12 needs (include/moka_hip.h); the GPU file asserts the rest."""
    cfg = cm.ALL_CONFIGS[name]
    carried = cfg.K % 2 == 0 and 34 <= cfg.K <= 64
    assert ("handoff" in cfg.reach) == carried
    assert all(c.s13 == (c.K % 2 == 0 and 34 <= c.K <= 64) for c in cs.CONFIGS.values() if not c.f32 and not hasattr(c, "nT"))


def test_the_triage_entry_point_prints_a_sequence(capsys):
    assert cm.main(["E2", str(SEEDS["E2"][0]), "--upto", "5"]) == 0
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 6 and out[0].startswith(" 0 ")
    assert cm.main(["nope"]) == 2
