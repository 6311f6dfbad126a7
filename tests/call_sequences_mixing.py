"""Seeded call sequences through the C ABI for the viscosity field, the quadratic bottom drag, both kinds of forced tape and the
Richardson closure: machines E and F of the scheme of tests/call_sequences.py and tests/call_sequences_vertical.py (machines A-D,
which this file leaves alone and builds on).

Machine E, the forced dycore (configs E1-E4): the vocabulary of machine C that bears on the vertical pass -- moka_set_vertical_viscosity,
moka_surface_stress_upload, RK4 steps with dt, 0.0 and a negative dt, moka_run (three steps eagerly, nine through the captured graph),
Forward Euler, kernel variants, uploads, the three reads of every Prog / Diag / Tend array, moka_tape_create as something the pass
refuses, moka_forced_tape with its flags, seeds, sweep, densities and scalar gradients -- plus what the last features added:
moka_vertical_viscosity_field_upload (NULL, all zero, two fields with zero interfaces and NaN in every never-read row, a field equal
to nuV, a negative and a NaN entry at an active row) with its download and moka_has_vertical_viscosity_field,
moka_set_quadratic_bottom_drag and its getter, moka_bottom_speed_download, moka_bottom_speed of level 0, 1 and a bad level,
moka_forced_tape_create_quadratic beside moka_forced_tape_create, the DF and D_cd flags with their downloads,
moka_forced_tape_device_arrays, exact zeros uploaded to normalVelocity (with the resting thickness: sp == 0 where the column sum is
exact, see HAZARDS in tests/test_call_sequences_mixing.py), and tuning keys 8 and 12.  Key 12 (the stage 1 -> 2 hand-off) is ignored by
the model, because the hand-off is bit for bit; the device runner counts from moka_state_rk_handoff_escapes' status the single RK4
steps that took it and those that did not (only E1 and E2 have a shape the default stage kernel carries, which the hand-off needs:
in E3 and E4 the key is accepted and no step takes it).

The model is call_sequences_vertical.ForcedModel with the pass of quadratic_drag_twin.apply (which takes momentum_vfield_twin's field)
behind every RK4 step, quadratic_drag_twin.bottom_speed behind the two speed getters and quadratic_adjoint_twin.transposed_pass in
front of every reversed step; no arithmetic is restated here.  Every observation is compared bit for bit (the field download on its
bit patterns: its never-read rows hold NaN), a refusal is an observation.

What the header words and the model therefore does (include/moka_hip.h): while a field is present nuV is not read and acts again once
the field is removed; an all-zero field counts as nuV == 0 yet is present; "drag on" is r != 0 or Cd != 0 and decides the n == 1
columns; a change takes effect with the next RK4 step or moka_run; moka_bottom_speed_download gives the sp of the last pass that was
launched, zeros when that pass ran without Cd; a forced tape copies the field only when it was uploaded or removed since the tape's
newest copy and releases the copies when a sweep has emptied it, records Cd per step, records sp for steps with Cd != 0 or the D_cd
flag and u* for steps with Cd != 0, allocates each array with the first step that needs it, and every seed zeroes every density;
moka_forced_tape_device_arrays is modelled as the header lists the allocations: un, hn, hbar and the scratch with the first step that
records the new level, one array per density first flagged, sp, then u* and M, and one per field copy.

Refusals: those of call_sequences_vertical.refusals that this vocabulary reaches, and the new ones -- Cd != 0 beside a plain forced
tape, the plain create call while Cd != 0, the D_cd flag on a plain tape (MOKA_ERR_UNSUPPORTED) and with recorded steps
(MOKA_ERR_ARG), the DF flag with recorded steps, a D_cd or DF download without its flag, an invalid field, an invalid Cd, a field and
Cd != 0 beside a moka_tape, the removal of an all-zero field beside a moka_tape while nuV != 0 (the field stays), Forward Euler,
moka_run(FE), moka_tape_create and dt < 0 while only a field or only Cd turned the pass on, a second forced tape of either kind, a bad
time level of moka_bottom_speed.  A taped step on a plain tape while Cd != 0 cannot be reached through the ABI (the setter refuses
beside a plain tape and the plain create refuses while Cd != 0): the library keeps the check, no sequence can show it.

Mutants (E_MUTANTS), each the bug one sentence of the header exists to prevent: field_late, cd_late (a step runs with the values of
the step before), scalar_lost (nuV does not act again after a removal), zero_field_transparent (nuV acts under an all-zero field),
cd_skips_n1 (n == 1 columns are not computed with only Cd on), sp_stale (the download keeps the last nonzero sp), sp_from_mixed (sp
from u_new, not u*), tape_field_newest (every reversed step uses the newest field), tape_cd_current (the reverse uses the state's
Cd), dens_not_zeroed (a seed leaves DF / D_cd and the other densities as they were), kink_divides (M is formed where sp == 0), late
and prev_level_lost as in machine A.

Machine F, tracers under the Richardson closure (configs F1-F3): the vocabulary of machine D that bears on the vertical passes --
moka_set_tracers with a changing count (0 included), tracer uploads and downloads, kappaV and the per-tracer fields with their getters,
nuV / r, the stress, RK4 steps with dt, 0.0 and a negative dt, moka_run of three and nine steps, Forward Euler, variants, the three
reads -- plus moka_set_richardson_mixing (off, the defaults, other parameters, a mask with the buoyancy inside, one with it outside,
the unit tracer as buoyancy, a negative and a NaN parameter, a buoyancy tracer out of range), moka_richardson_mixing with the mask
through moka_tracer_count (and with a NULL `on` or `out`: MOKA_ERR_ARG), moka_richardson_fields_download (both, F alone, G alone), moka_richardson_diagnose (level 0, 1, a bad
level, all four outputs and a single one), machine E's viscosity field and Cd, every create call the closure refuses, and tuning keys
7, 8 and 12 each toggled between steps with the closure on (the step stays the 16-stream one: moka_state_rk4_streams is an
observation; the device runner counts the single steps under the closure that took the stage 1 -> 2 hand-off: only F1 has a shape
that carries it).  The
model is call_sequences_vertical.VTracerModel whose step is richardson_twin.RichardsonTwin.step_rk4; the header's rules it follows:
while the closure is on the caller's nuV, field, kappaV_j and per-tracer fields are set aside, their setters keep working and they
act again when it is switched off; drag, Cd and stress are untouched; tracers outside the mask keep their own coefficient; a change of
parameters takes effect with the next step or moka_run; the fields download gives zeros when the last step ran without the closure
or launched nothing (dt == 0.0, K == 1) and after the closure was switched off or on again; moka_set_tracers switches the closure
off; the validation order is parameters, tapes, no tracers, buoyancy range.  Mutants (F_MUTANTS): rich_late, aside_lost,
setter_dropped, rich_from_mixed, fields_stale, mask_ignored, drag_set_aside, levels_swapped, set_tracers_keeps, coeff_late,
mixed_flow_early (the tracers' stage 4, and with it G's tracer pass, over the flow the momentum pass has already mixed) and
prev_level_lost.  The named orders are counted per coefficient: a setter of nuV, of the field, of kappaV and of a per-tracer field,
each with a value that is on, accepted while the closure is on, then off, then a step in which that coefficient acts (at K = 1 no
field has an active interface: F3 shows nuV and kappaV only, by their values); each of the four acting again in a step behind a
closure step; "on, off, on" needs other parameters the second time; each of keys 7, 8 and 12 changed between two closure steps.
Refusals: a NULL out-pointer of moka_richardson_mixing, invalid parameters, a buoyancy tracer out of range, no tracers, the closure beside a tracer tape and a
tracer tape beside the closure, moka_tape_create and both forced create calls, moka_step_fe, moka_run(FE), dt < 0, a bad time level
and moka_richardson_diagnose while the closure is off.

Stay uncovered by machines E and F: the closure beside a moka_tape or a forced tape that already exists (neither can exist on a state
with tracers, and the closure needs one), the tracer tape's sweeps under changing coefficients (machine D has them), NULL
out-pointers other than moka_richardson_mixing's (moka_richardson_fields_download and moka_richardson_diagnose take NULL for any
output), the nonlinear / Del2 / Del4 toggles, placement, the 13-stream form and the moka_tape sweeps
(machine C has them), halos, partitions and fp32 (their refusals stay where tests/test_gpu_richardson.py has
them), the three moka_rk4_dist_* guards, a tracer count changing under a live tracer tape, and the K >= 106 column forms of the
closure's lane groups, which tests/test_gpu_richardson.py runs once by hand.

Replay a sequence on the CPU:   python tests/call_sequences_mixing.py E2 3 [--upto N]   (or F1 21)

This module imports no GPU code when it is imported (moka_hip.lib is loaded by the device runner only)."""
import ctypes as C
import os
import sys
import zlib
from dataclasses import dataclass

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import call_sequences as cs  # noqa: E402
import call_sequences_vertical as cv  # noqa: E402
from call_sequences import (DIAG, ERR_ARG, ERR_UNSUPPORTED, F_H, F_SSH, F_U, OK, PROG, READ_KINDS, STATE_KEYS, TEND, Obs, Op,  # noqa: E402
                            first_mismatch, get_mesh, initial_state, resting_thickness, shape_of, values, zlib_crc)
from call_sequences_vertical import GRAD_BITS, STRESS_OK, VISC_BAD, VISC_OK, depths_of, dt_of, free_seed, mask_of, stress_values, visc_values  # noqa: E402
import forced_adjoint_twin as fa  # noqa: E402
import momentum_vfield_twin as mf  # noqa: E402
import momentum_vmix_twin as mv  # noqa: E402
import quadratic_adjoint_twin as qa  # noqa: E402
import quadratic_drag_twin as qd  # noqa: E402

ERR_HIP = -2
E_MUTANTS = ("field_late", "cd_late", "scalar_lost", "zero_field_transparent", "cd_skips_n1", "sp_stale", "sp_from_mixed",
             "tape_field_newest", "tape_cd_current", "dens_not_zeroed", "kink_divides", "late", "prev_level_lost")
FIELD_OK = ("none", "zero", "A", "B", "eqnu")
FIELD_BAD = ("neg", "nan")
FIELD_ON = ("A", "B", "eqnu")
CD_OK = ("zero", "cd", "other")
CD_BAD = ("neg", "nan")
STEP_KINDS = ("fe", "rk4", "run", "ft_taped")
FT_READS = ("ft_download", "ft_density", "ft_gradient", "ft_df_download", "ft_cd_density", "ft_cd_gradient")
GETTERS = ("visc_read", "stress_download", "has_stress", "vmix_path", "ft_path", "field_download", "has_field", "cd_read", "sp_download",
           "sp_diag", "ft_arrays")
FT_OWN = ("ft_taped", "ft_want_df", "ft_want_cd", "ft_df_download", "ft_cd_density", "ft_cd_gradient")
# ops that change no array of the state but may fall between a change of one and its first read
NON_ARRAY_OPS = ("tuning", "variant", "tape_create", "tape_destroy", "visc", "stress", "field", "cd", "ft_create", "ftq_create", "ft_want",
                 "ft_want_df", "ft_want_cd", "ft_seed_ssh", "ft_seed_free", "ft_sweep", "ft_destroy")
CAUSE_REFUSALS = ("fe_vmix", "run_fe_vmix", "tape_vmix", "dt_negative_rk4")


# ---------------------------------------------------------------------------------------------------------------------------------
# configs
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class EConfig(cv.VConfig):
    machine = "E"


E_CONFIGS = {c.name: c for c in (
    # the forward tile form; reverse steps recorded with a field take the column form (five column sets: from K = 64), steps recorded
    # without one keep the four-set tiles of 32 columns: one tape holds both
    EConfig("E1", "ico4", 64, nops=36, variants=(0, 11), reach=("path_1", "ft_path_1", "ft_path_2", "handoff")),
    # neighbouring edges with different bottom levels: the depth test of the speed gather, the grouping by level of its transpose, "drag
    # on decides the n == 1 columns", field rows k >= n_e - 1 that hold NaN
    EConfig("E2", "hex6x4", 60, dt=2.0, depths="shelf", nops=36, variants=(0, 4), reach=("path_1", "ft_path_1", "handoff")),
    # heptagons: seven slots in the slot loops; FIELD reverse tiles of 64 columns; the tile and the column form inside one history
    EConfig("E3", "ico4f", 5, variants=(0, 3), nops=36, reach=("path_1", "path_2", "ft_path_1", "ft_path_2")),
    # K = 1: a field has no active row (present, counts as zero), every wet column has n == 1: Cd alone decides whether anything is launched
    EConfig("E4", "hex4x4", 1, dt=2.0, nops=36, variants=(0, 3), reach=("path_2", "ft_path_2")),
)}
ALL_CONFIGS = dict(E_CONFIGS)


def field_patterns(cfg, ok=True):
    """K == 1 has no active interface: no entry of a field is ever inspected, so no field is invalid there."""
    return FIELD_OK if ok else (FIELD_BAD if cfg.K > 1 else ())


def field_values(cfg, pattern):
    """The (nEdges, K) doubles of a field op: None (NULL), all zero, two random fields in [0, 2] x nuV with exact zeros at interface 1 of
    every fifth edge and below the first interface of edge 3 and NaN in every never-read row, the uniform field equal to visc_values'
    nuV (NaN in the never-read rows), and field A with a negative or a NaN entry at an active row."""
    if pattern == "none":
        return None
    nE, K = shape_of(cfg, F_U)
    mlt = depths_of(cfg)
    if pattern == "zero":
        return np.zeros((nE, K))
    nu = visc_values(cfg, "nu")[0]
    if pattern == "eqnu":
        return mf.uniform_field(nE, K, mlt, nu)
    f = np.random.default_rng([cfg.K, 81 if pattern == "B" else 80]).uniform(0.0, 2.0, (nE, K)) * nu
    if K > 1:
        f[::5, 1] = 0.0
    f[3, 1:] = 0.0
    live = mf.live_of(mlt, K)
    f[~live] = np.nan
    if pattern in FIELD_BAD:
        e, k = np.argwhere(live)[len(np.argwhere(live)) // 2]
        f[e, k] = -nu if pattern == "neg" else np.nan
    return np.ascontiguousarray(f)


def cd_values(cfg, pattern):
    c = qd.cd_of(cfg.K, cfg.dt)
    return {"zero": 0.0, "cd": c, "other": 0.375 * c, "neg": -c, "nan": float("nan")}[pattern]


def bits(a):
    """The bit patterns of a double array: what a field that may hold NaN is compared on."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).copy()


# ---------------------------------------------------------------------------------------------------------------------------------
# vocabulary
# ---------------------------------------------------------------------------------------------------------------------------------
def vocabulary(cfg):
    return ("visc", "stress", "field", "cd", "rk4", "run", "fe", "variant", "tuning", "upload", "upload_zero_u", "upload_rest_h",
            "download", "rows", "sumsq", "visc_read", "has_stress", "vmix_path", "field_download", "has_field", "cd_read",
            "sp_download", "sp_diag", "tape_create", "tape_destroy", "ft_create", "ftq_create", "ft_want", "ft_want_df", "ft_want_cd",
            "ft_taped", "ft_seed_ssh", "ft_seed_free", "ft_sweep", "ft_download", "ft_density", "ft_gradient", "ft_df_download",
            "ft_cd_density", "ft_cd_gradient", "ft_arrays", "ft_path", "ft_destroy")


def arg_class(op):
    k, a = op.kind, op.args
    if k in ("visc", "stress", "field", "cd", "variant", "ft_download", "ft_taped", "rk4", "sp_diag", "ft_want_df", "ft_want_cd"):
        return (k, a[0])
    if k in READ_KINDS:
        return (k, a[0] in PROG, a[0] in TEND)
    if k in ("tuning", "run"):
        return (k, a[0], a[1])
    return None


def arg_classes(cfg):
    """Every (kind, argument class) the config admits with status MOKA_OK."""
    c = [("visc", p) for p in VISC_OK] + [("stress", p) for p in ("none", "zero", "field")] + [("field", p) for p in FIELD_OK]
    c += [("cd", p) for p in CD_OK] + [("rk4", f) for f in (1.0, 0.0)] + [("run", 1, 3), ("run", 1, 9), ("run", 0, 3)]
    c += [("variant", v) for v in cfg.variants] + [("tuning", 8, v) for v in cs.TUNING_VALUES[8]] + [("tuning", 12, v) for v in (0, 1)]
    c += [(r, p, t) for r in READ_KINDS for p, t in ((True, False), (False, True), (False, False))]
    c += [("sp_diag", l) for l in (0, 1)] + [("ft_taped", f) for f in (1.0, 0.0)] + [("ft_download", f) for f in (F_U, F_H)]
    c += [(k, on) for k in ("ft_want_df", "ft_want_cd") for on in (0, 1)]
    return tuple(c)


def refusals(cfg):
    r = ["fe_vmix", "run_fe_vmix", "tape_vmix", "visc_tape", "stress_tape", "dt_negative_rk4", "dt_negative_run", "dt_negative_ft",
         "visc_invalid", "stress_nan", "ft_tape", "tape_forced", "stress_recorded", "ft_want_recorded", "ft_full", "ft_sweep_unseeded",
         "ft_density_unflagged",
         "cd_plain_tape", "ft_create_cd", "ft_want_cd_plain", "ft_want_cd_recorded", "ft_want_df_recorded", "ft_cd_unflagged",
         "ft_df_unflagged", "cd_invalid", "field_tape", "cd_tape", "field_removal_tape", "ft_second", "sp_diag_level"]
    r += [b + "_cd" for b in CAUSE_REFUSALS]
    if cfg.K > 1:
        r += ["field_invalid"] + [b + "_field" for b in CAUSE_REFUSALS]
    return tuple(r)


WRITERS_EVERY_READ = ("rk4", "run", "upload", "ft_taped")
WRITERS_ANY_READ = ("visc", "stress", "field", "cd", "fe", "variant", "tuning", "upload_zero_u", "upload_rest_h", "ft_create", "ftq_create",
                    "ft_seed_ssh", "ft_seed_free", "ft_sweep", "ft_destroy")


def pairs_wanted(cfg):
    return {(k, r) for k in WRITERS_EVERY_READ for r in READ_KINDS}, WRITERS_ANY_READ


def cases_wanted(cfg):
    c = ["zero_field_over_nu", "field_eq_scalar", "change_between_runs", "sp_cycle", "sp_diag_levels", "ftq_three_cd", "field_while_recorded",
         "second_seed", "arrays_lazy", "arrays_as_plain", "zero_u_sweep", "handoff_toggle"]
    if cfg.K > 1:                  # a field that is on needs an active interface
        c += ["field_cycle", "ft_three_fields"]
    if cfg.K > 1 and 3 in cfg.variants:      # both forms of both passes inside the config's histories
        c += ["forms_forward", "forms_reverse"]
    return tuple(c)


def cases_seen(cfg, ops, obs):
    """The named orders a sequence shows, from the ops and what the model says each accepted step did (Obs.info)."""
    seen = set()
    fc = 0        # field_cycle: 1 a mixed step under a field that is on with nuV != 0, 2 the field removed, 3 a mixed step with the scalar
    zf = 0        # zero_field_over_nu: 1 a step under an all-zero field with nuV != 0
    eq = 0        # field_eq_scalar: 1 a mixed step under the field equal to nuV
    runs = 0      # change_between_runs: 1 a run of nine with the pass on, 2 a field or Cd op accepted behind it
    sp = 0        # sp_cycle: 1 a launched step with Cd, 2 sp_download, 3 a launched step without Cd
    sd = None     # sp_diag_levels: the levels read since the last step
    q3 = None     # ftq_three_cd: the Cd's of the steps recorded on a quadratic tape with D_cd flagged; "swept" behind the sweep
    f3 = None     # ft_three_fields: progress on a tape with DF flagged
    fr = set()    # field_while_recorded: what happened while steps were recorded
    ss = 0        # second_seed: 1 a sweep of recorded steps with a density flagged, 2 a recorded step behind it, 3 a seed, 4 a sweep
    al = None     # arrays_lazy: the last ft_arrays value since the tape was made
    zu = 0        # zero_u_sweep: 1 upload_zero_u, 2 a recorded step with Cd != 0
    ho = [None, None]     # handoff_toggle: [key-12 value, read behind it] of the last two single RK4 steps with nothing else between
    key12 = 1
    variant, fwd, rev, rec_on = 0, set(), set(), False      # the forms that ran: launched steps / sweeps of a launched record by variant == 3
    quad = flagged = False
    nrec = 0
    for op, o in zip(ops, obs):
        if o.rc != OK:
            if op.kind == "stress" and o.refusal == "stress_recorded":
                fr.add("stress")
                if fr == {"stress", "field"}:
                    seen.add("field_while_recorded")
            continue
        k, a, info = op.kind, op.args, getattr(o, "info", {})
        if k in STEP_KINDS:
            mixed, fld, cd = bool(info.get("mixed")), info.get("field"), info.get("cd", 0.0)
            fc = 1 if (mixed and fld == "on" and info.get("nuV")) else 3 if (fc == 2 and mixed and fld is None and info.get("nuV")) else 0
            zf = 1 if (fld == "zero" and info.get("nuV")) else 0
            eq = 1 if (mixed and info.get("pattern") == "eqnu" and info.get("nu_set") == visc_values(cfg, "nu")[0]) else 0
            nine = k == "run" and a[0] == 1 and a[1] == 9 and info.get("on") and mixed
            if nine and runs == 2:
                seen.add("change_between_runs")
            runs = 1 if nine else 0
            launched = bool(info.get("launched"))
            if launched:
                sp = 1 if cd != 0.0 else 3 if sp == 2 else 0
            sd = set()
            if launched:
                fwd.add(variant == 3)
                if fwd == {False, True}:
                    seen.add("forms_forward")
            if k == "ft_taped":
                nrec += 1
                rec_on = rec_on or launched
                if q3 is not None and isinstance(q3, list) and info.get("dt") != 0.0:
                    q3.append(cd)
                if f3 == 0 and fld == "on" and mixed:
                    f3 = 1
                elif f3 == 1 and fld is None:
                    f3 = 2
                elif f3 == 2 and fld == "on" and mixed:
                    f3 = 3
                ss = 2 if ss in (1, 2) else 0
                zu = 2 if (zu == 1 and cd != 0.0 and info.get("dt") != 0.0) else 0
            else:
                zu = 0
            if k == "rk4":
                ho = [ho[1] if (ho[1] and ho[1][1]) else None, [key12, False]]
            else:
                ho = [None, None]
        elif k == "tuning" and a[0] == 12:
            key12 = a[1]
        elif k == "variant":
            variant = a[0]
        elif k == "field":
            fc = 2 if (fc == 1 and a[0] == "none") else 0
            runs = 2 if runs in (1, 2) else 0
            if nrec > 0:
                fr.add("field")
                if fr == {"stress", "field"}:
                    seen.add("field_while_recorded")
        elif k == "cd":
            runs = 2 if runs in (1, 2) else 0
        elif k == "upload_zero_u":
            zu = 1
        elif k == "upload" and a[0] == F_U and a[1] == 1:
            zu = 0
        elif k in ("ft_create", "ftq_create"):
            quad, flagged, nrec, al, fr, rec_on = k == "ftq_create", False, 0, None, set(), False
            q3 = f3 = None
            ss = 0
        elif k == "ft_destroy":
            q3 = f3 = al = None
            nrec, ss, fr, rec_on = 0, 0, set(), False
        elif k == "ft_want":
            flagged = flagged or bool(a[1])
        elif k == "ft_want_cd":
            flagged = flagged or bool(a[0])
            q3 = [] if (a[0] and quad) else None
        elif k == "ft_want_df":
            flagged = flagged or bool(a[0])
            f3 = 0 if a[0] else None
        elif k in ("ft_seed_ssh", "ft_seed_free"):
            ss = 3 if ss in (2, 3) else ss
        elif k == "ft_sweep":
            if isinstance(q3, list):
                q3 = "swept" if (0.0 in q3 and len({c for c in q3 if c != 0.0}) >= 2) else []
            if f3 == 3:
                f3 = 4
            elif f3 is not None:
                f3 = 0
            if zu == 2:
                seen.add("zero_u_sweep")
            zu = 0
            ss = 4 if ss == 3 else 1 if (nrec > 0 and flagged) else 0
            if rec_on:
                rev.add(variant == 3)
                if rev == {False, True}:
                    seen.add("forms_reverse")
            nrec, fr, rec_on = 0, set(), False
        elif k == "ft_cd_density" or k == "ft_cd_gradient":
            if q3 == "swept":
                seen.add("ftq_three_cd")
            if ss == 4:
                seen.add("second_seed")
        elif k == "ft_df_download":
            if f3 == 4:
                seen.add("ft_three_fields")
            if ss == 4:
                seen.add("second_seed")
        elif k in ("ft_density", "ft_gradient"):
            if ss == 4:
                seen.add("second_seed")
        elif k == "ft_arrays":
            if al is not None and o.value > al and nrec > 0:
                seen.add("arrays_lazy")
            if quad and nrec > 0 and o.value == 0:
                seen.add("arrays_as_plain")
            al = o.value
        elif k == "sp_download":
            if sp == 3 and not np.any(o.value):
                seen.add("sp_cycle")
            sp = 2 if (sp == 1 and np.any(o.value)) else 0
        elif k == "sp_diag":
            if sd is not None:
                sd.add((a[0], zlib.crc32(np.ascontiguousarray(o.value).tobytes())))
                if {l for l, _ in sd} >= {0, 1} and len({c for _, c in sd}) > 1:      # both levels, and they differ
                    seen.add("sp_diag_levels")
        elif k in READ_KINDS:
            if a[0] == F_U and a[1] == 1:
                if fc == 3:
                    seen.add("field_cycle")
                if zf == 1:
                    seen.add("zero_field_over_nu")
                if eq == 1:
                    seen.add("field_eq_scalar")
            if ho[1]:
                ho[1][1] = True
                if ho[0] and ho[0][0] != ho[1][0]:
                    seen.add("handoff_toggle")
        if k in ("upload", "upload_zero_u", "upload_rest_h"):
            ho = [None, None]          # something else moved the state: the pair of single steps is broken
    return seen


# ---------------------------------------------------------------------------------------------------------------------------------
# generator: a pure function of (config, seed)
# ---------------------------------------------------------------------------------------------------------------------------------
class _Abstract:
    """What the generator has to know to aim: which values are in force, which handles live, which arrays changed since their last read."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.visc, self.stress, self.field, self.cd = "zero", "none", "none", "zero"
        self.variant = 0
        self.tape = False
        self.ft = None                 # dict(cap, n, seeded, want, wantF, wantCd, quad)
        self.dirty = []                # keys, the most recently changed last

    def nu_on(self):
        if self.field != "none":
            return self.field in FIELD_ON and self.cfg.K > 1
        return self.visc in ("nu", "both", "other")

    def causes(self):
        c = set()
        if self.nu_on():
            c.add("field" if self.field != "none" else "nu")
        if self.visc in ("drag", "both", "other"):
            c.add("drag")
        if self.stress in ("field", "other"):
            c.add("stress")
        if self.cd != "zero":
            c.add("cd")
        return c

    def on(self):
        return bool(self.causes())

    def touch(self, keys):
        for k in keys:
            if k in self.dirty:
                self.dirty.remove(k)
            self.dirty.append(k)

    def stepped(self, dtf=1.0):
        if dtf == 0.0:
            self.touch([(f, 0) for f in PROG] + [(f, 1) for f in TEND])
        else:
            self.touch([(f, l) for l in (0, 1) for f in PROG] + [(f, 1) for f in DIAG + TEND])

    def accept(self, op):
        """Advance as include/moka_hip.h says the call behaves; a refusal changes nothing."""
        k, a, t, ft = op.kind, op.args, self.tape, self.ft
        if k == "visc":
            if a[0] in VISC_BAD or (a[0] != "zero" and t):
                return
            self.visc = a[0]
        elif k == "stress":
            if a[0] == "nan" or (a[0] != "none" and t) or (ft and ft["n"] > 0):
                return
            self.stress = a[0]
        elif k == "field":
            if (a[0] in FIELD_BAD and self.cfg.K > 1) or (a[0] != "none" and t):
                return
            if a[0] == "none" and t and self.field != "none" and self.visc in ("nu", "both", "other"):
                return
            self.field = "A" if a[0] in FIELD_BAD else a[0]
        elif k == "cd":
            if a[0] in CD_BAD or (a[0] != "zero" and (t or (ft and not ft["quad"]))):
                return
            self.cd = a[0]
        elif k == "rk4":
            if not (a[0] < 0 and self.on()):
                self.stepped(a[0])
        elif k == "run":
            if a[0] == 0 and self.on():
                return
            if a[0] == 1 and a[3] < 0 and self.on():
                return
            self.stepped(a[3] if a[0] == 1 else 1.0)
        elif k == "fe":
            if not self.on():
                self.stepped()
        elif k == "variant":
            if a[0] in cs.VARIANTS:
                self.variant = a[0]
        elif k == "upload":
            self.touch([(a[0], a[1])])
        elif k == "upload_zero_u":
            self.touch([(F_U, 1)])
        elif k == "upload_rest_h":
            self.touch([(F_H, 1)])
        elif k in READ_KINDS:
            if (a[0], a[1]) in self.dirty:
                self.dirty.remove((a[0], a[1]))
        elif k == "tape_create":
            if not (self.on() or ft or t):
                self.tape = True
        elif k == "tape_destroy":
            self.tape = False
        elif k in ("ft_create", "ftq_create"):
            if not (t or ft or (k == "ft_create" and self.cd != "zero")):
                self.ft = dict(cap=a[0], n=0, seeded=False, want=0, wantF=False, wantCd=False, quad=k == "ftq_create")
        elif k == "ft_destroy":
            self.ft = None
        elif ft is None:
            return
        elif k == "ft_want":
            if ft["n"] == 0:
                ft["want"] = (ft["want"] | a[0]) if a[1] else (ft["want"] & ~a[0])
        elif k == "ft_want_df":
            if ft["n"] == 0:
                ft["wantF"] = bool(a[0])
        elif k == "ft_want_cd":
            if ft["n"] == 0 and ft["quad"]:
                ft["wantCd"] = bool(a[0])
        elif k == "ft_taped":
            if ft["n"] < ft["cap"] and not (a[0] < 0 and self.on()):
                ft["n"] += 1
                ft["seeded"] = False
                self.stepped(a[0])
        elif k in ("ft_seed_ssh", "ft_seed_free"):
            ft["seeded"] = True
        elif k == "ft_sweep":
            if ft["seeded"]:
                ft["n"] = 0


def sequence(cfg, seed):
    """About cfg.nops ops, a pure function of (cfg, seed): scenes -- short scripts that aim at one named order or one refusal from
    whatever state the history has reached -- between random single ops and reads of what changed."""
    rng = np.random.default_rng([zlib_crc(cfg.name), seed])
    ab = _Abstract(cfg)
    ops = []
    vs = [0]
    pending = [(f, 1) for f in DIAG + TEND]
    NU = ("nu", "both", "other")

    def draw(items, weights=None):
        if weights is None:
            return items[int(rng.integers(len(items)))]
        w = np.asarray(weights, dtype=np.float64)
        return items[int(rng.choice(len(items), p=w / w.sum()))]

    def vseed():
        vs[0] += 1
        return 15485863 * (seed + 1) + vs[0]

    def a_read(keys=None, kind=None):
        cand = [k for k in ab.dirty if keys is None or k in keys]
        if not cand:
            return None
        w = [2.0 ** min(i - len(cand), 0) for i in range(1, len(cand) + 1)]
        key = draw(cand, w)
        kind = kind or draw(READ_KINDS)
        if kind == "rows":
            n = shape_of(cfg, key[0])[0]
            rows = tuple(int(r) for r in rng.integers(0, n, int(rng.integers(1, 5))))
            return Op("rows", (key[0], key[1], rows))
        return Op(kind, key)

    def a_seed():
        return Op("ft_seed_ssh") if rng.random() < 0.5 else Op("ft_seed_free", (vseed(),))

    def a_plain_step():
        name = draw(("rk4", "run3", "run9"), (4, 1.5, 1.0))
        if name == "rk4":
            return Op("rk4", (0.0 if rng.random() < 0.1 else 1.0,))
        return Op("run", (1, 3 if name == "run3" else 9, 0, 1.0))

    def a_tuning():
        return Op("tuning", (8, draw(cs.TUNING_VALUES[8]))) if rng.random() < 0.5 else Op("tuning", (12, int(rng.integers(2))))

    def a_step():
        if ab.ft and ab.ft["n"] < ab.ft["cap"] and rng.random() < 0.3:
            return Op("ft_taped", (1.0,))
        return a_plain_step()

    def stress_free():
        return not ab.tape and not (ab.ft and ab.ft["n"] > 0)

    def cd_free():
        return not ab.tape and not (ab.ft and not ab.ft["quad"])

    # ---- what a scene needs first ----
    def ensure_no_tape():
        if ab.tape:
            yield Op("tape_destroy")

    def ensure_cd_free():
        yield from ensure_no_tape()
        if ab.ft and not ab.ft["quad"]:
            yield Op("ft_destroy")

    def ensure_on():
        yield from ensure_no_tape()
        if not ab.on():
            r = rng.random()
            if r < 0.3 and cd_free():
                yield Op("cd", (draw(CD_OK[1:]),))
            elif r < 0.55 and cfg.K > 1:
                yield Op("field", (draw(("A", "B")),))
            elif r < 0.7 and stress_free():
                yield Op("stress", ("field",))
            else:
                yield Op("visc", (draw(VISC_OK[1:]),))

    def ensure_off():
        """The pass off, as far as the handles allow (a stress cannot go while steps are recorded: that tape is destroyed)."""
        if ab.visc != "zero":
            yield Op("visc", ("zero",))
        if ab.cd != "zero":
            yield Op("cd", ("zero",))
        if ab.field in FIELD_ON and cfg.K > 1:
            yield Op("field", (draw(("none", "zero")),))
        if ab.stress in ("field", "other"):
            if ab.ft and ab.ft["n"] > 0:
                yield Op("ft_destroy")
            yield Op("stress", (draw(("none", "zero")),))

    def ensure_ft(quad=None, cap=None, room=1, empty=False):
        yield from ensure_no_tape()
        ft = ab.ft
        if ft and ((quad is not None and ft["quad"] != quad) or ft["cap"] - ft["n"] < room or (empty and ft["n"] > 0) or (cap and ft["cap"] < cap)):
            yield Op("ft_destroy")
        if not ab.ft:
            q = quad if quad is not None else (ab.cd != "zero" or rng.random() < 0.5)
            if not q and ab.cd != "zero":
                yield Op("cd", ("zero",))
            yield Op("ftq_create" if q else "ft_create", (cap or int(rng.integers(max(room, 1), 4)),))

    # ---- scenes ----
    def scene_mixed_read():
        yield from ensure_on()
        yield a_step()
        for _ in range(int(rng.integers(1, 3))):
            yield a_read(pending)
        yield a_read()

    def scene_change_then_read():
        yield from ensure_on()
        yield a_step()
        c = [Op("visc", (draw([p for p in VISC_OK if p != ab.visc]),))] if not ab.tape else []
        c += [Op("field", (draw([p for p in FIELD_OK if p != ab.field]),))] * 2
        if cd_free():
            c += [Op("cd", (draw([p for p in CD_OK if p != ab.cd]),))] * 2
        if stress_free():
            c += [Op("stress", (draw([p for p in ("none", "zero", "field") if p != ab.stress]),))]
        c += [Op("variant", (draw([v for v in cfg.variants if v != ab.variant]),)), a_tuning()]
        yield draw(c)
        yield a_read([(f, 1) for f in TEND])
        yield a_read([(f, 1) for f in DIAG])
        yield a_read()

    def scene_field_cycle():
        yield from ensure_no_tape()
        eq = rng.random() < 0.4
        if ab.visc not in (("nu", "both") if eq else NU):
            yield Op("visc", (draw(("nu", "both")),))
        yield Op("field", ("eqnu" if eq else draw(("A", "B")),))
        yield Op("field_download") if rng.random() < 0.4 else None
        yield a_plain_step() if rng.random() < 0.7 else Op("rk4", (1.0,))
        yield a_read([(F_U, 1)])
        yield Op("field", ("none",))
        yield Op("has_field") if rng.random() < 0.4 else None
        yield Op("rk4", (1.0,)) if rng.random() < 0.7 else a_plain_step()
        yield a_read([(F_U, 1)])
        yield a_read(pending)

    def scene_zero_field():
        yield from ensure_no_tape()
        if ab.visc not in NU:
            yield Op("visc", ("nu",))
        yield Op("field", ("zero",))
        yield Op("rk4", (1.0,)) if rng.random() < 0.6 else a_plain_step()
        yield a_read([(F_U, 1)])
        if not ab.on() and not ab.ft and rng.random() < 0.7:
            yield Op("tape_create", (2,))
            yield Op("field", ("none",))                   # refused: nuV != 0 would act again beside the moka_tape; the field stays
            yield Op("has_field")
            yield draw((Op("field", (draw(("zero", "A")),)), Op("cd", ("cd",)), Op("visc", ("nu",)), Op("stress", ("zero",))))   # refused
            yield a_read()
            yield Op("tape_destroy")
            yield Op("field", ("none",))
        yield draw((Op("has_field"), Op("field_download"), Op("visc_read")))

    def scene_runs():
        yield from ensure_on()
        yield Op("run", (1, 9, 0, 1.0))
        if cd_free() and rng.random() < 0.5:
            yield Op("cd", (draw([p for p in CD_OK[1:] if p != ab.cd]),))
        else:
            yield Op("field", (draw([p for p in (FIELD_ON if cfg.K > 1 else FIELD_OK) if p != ab.field]),))
        yield Op("run", (1, 9, 0, 1.0))
        yield a_read([(F_U, 1)])
        yield a_read(pending)

    def scene_sp():
        yield from ensure_cd_free()
        if ab.visc not in ("drag", "both", "other"):
            yield Op("visc", (draw(("drag", "both")),))
        yield Op("cd", (draw([p for p in CD_OK[1:] if p != ab.cd] or ["cd"]),))
        yield Op("rk4", (1.0,)) if rng.random() < 0.7 else Op("run", (1, 3, 0, 1.0))
        yield Op("sp_download")
        for l in rng.permutation(2):
            yield Op("sp_diag", (int(l),))
        yield Op("cd", ("zero",))
        yield Op("cd_read") if rng.random() < 0.5 else None
        yield Op("rk4", (1.0,))
        yield Op("sp_download")
        yield a_read([(F_U, 1)])

    def scene_ftq_cd():
        yield from ensure_ft(quad=True, cap=3, empty=True)
        if ab.ft["wantCd"] or rng.random() < 0.3:
            yield Op("ft_want_cd", (0,))
        yield Op("ft_want_cd", (1,))
        if ab.cd != "zero":
            yield Op("cd", ("zero",))
        yield Op("ft_arrays")
        order = [("zero", "cd", "other"), ("zero", "other", "cd"), ("cd", "zero", "other")][int(rng.integers(3))]
        for i, p in enumerate(order):
            if ab.cd != p:
                yield Op("cd", (p,))
            yield Op("ft_taped", (1.0,))
            if i < 2 or rng.random() < 0.5:
                yield Op("ft_arrays")
        if rng.random() < 0.4:
            yield draw((Op("ft_want_cd", (0,)), Op("ft_want_df", (1,)), Op("ft_want", (draw(GRAD_BITS), 1))))     # refused: recorded steps
        yield a_seed()
        yield Op("ft_sweep")
        yield Op(draw(("ft_cd_density", "ft_cd_gradient")))
        yield Op("ft_download", (draw((F_U, F_H)),))
        yield Op("ft_path")

    def scene_ft_fields():
        yield from ensure_ft(cap=3, empty=True)
        if ab.ft["wantF"] or rng.random() < 0.3:
            yield Op("ft_want_df", (0,))
        yield Op("ft_want_df", (1,))
        first, third = ("A", "B") if rng.random() < 0.5 else ("B", "A")
        yield Op("field", (first,))
        yield Op("ft_arrays")
        yield Op("ft_taped", (1.0,))
        yield Op("ft_arrays")
        yield Op("field", ("none",))
        if ab.visc == "zero" and rng.random() < 0.5:
            yield Op("visc", (draw(VISC_OK[1:]),))
        yield Op("ft_taped", (1.0,))
        yield Op("stress", (draw(("none", "zero", "field")),))      # refused: recorded steps
        yield Op("field", (third,))
        yield Op("ft_taped", (1.0,))
        yield Op("ft_arrays")
        yield a_seed()
        yield Op("ft_sweep")
        yield Op("ft_df_download")
        yield Op("ft_arrays")
        yield Op("ft_download", (draw((F_U, F_H)),))
        yield Op("ft_path")

    def scene_second_seed():
        yield from ensure_ft(room=2, empty=True)
        ft = ab.ft
        flag = draw(["df", "bit"] + (["cd"] if ft["quad"] else []))
        yield Op("ft_want_df", (1,)) if flag == "df" else Op("ft_want_cd", (1,)) if flag == "cd" else Op("ft_want", (draw(GRAD_BITS), 1))
        yield from ensure_on()
        yield Op("ft_taped", (1.0,))
        yield a_seed()
        yield Op("ft_sweep")
        yield Op("ft_taped", (0.0 if rng.random() < 0.2 else 1.0,))
        yield a_read(pending)
        yield a_seed()
        if rng.random() < 0.4:
            yield a_seed()
        yield Op("ft_sweep")
        ft = ab.ft
        c = [Op("ft_df_download")] if ft["wantF"] else []
        c += [Op(draw(("ft_cd_density", "ft_cd_gradient")))] if ft["wantCd"] else []
        c += [Op(draw(("ft_density", "ft_gradient")), (b,)) for b in GRAD_BITS if ft["want"] & b]
        yield draw(c)
        yield Op("ft_download", (draw((F_U, F_H)),))

    def scene_zero_u():
        yield from ensure_ft(quad=True, room=1)
        if ab.cd == "zero":
            yield Op("cd", (draw(CD_OK[1:]),))
        yield Op("upload_rest_h")
        yield Op("upload_zero_u")
        yield Op("ft_taped", (1.0,))
        yield Op("sp_download")
        yield Op("ft_seed_free", (vseed(),))
        yield Op("ft_sweep")
        yield Op("ft_download", (F_U,))
        yield a_read([(F_H, 1)])
        yield a_read([(F_U, 1)])

    def scene_step_upload_read():
        """A step, then an upload into the level the step left its diagnostics and tendencies for, then a read of them."""
        if rng.random() < 0.7:
            yield from ensure_on()
        yield a_step()
        yield Op("upload", (draw((F_U, F_H)), 1, vseed()))
        yield a_read([(f, 1) for f in DIAG + TEND])
        yield a_read([(f, 1) for f in DIAG + TEND])
        yield a_read([(f, 1) for f in PROG])

    def scene_plain_quiet():
        """A quadratic tape that saw no Cd and no flag owns what a plain one does; a plain tape refuses Cd and the D_cd flag."""
        yield from ensure_off()
        if ab.ft:
            yield Op("ft_destroy")
        yield from ensure_no_tape()
        quad = rng.random() < 0.6
        yield Op("ftq_create" if quad else "ft_create", (2,))
        yield Op("ft_create" if rng.random() < 0.5 else "ftq_create", (2,))        # refused: a forced tape exists
        if not quad:
            yield Op("cd", (draw(CD_OK[1:]),))             # refused beside a plain tape
            yield Op("ft_want_cd", (1,))                   # refused: UNSUPPORTED
        yield Op("ft_taped", (1.0,))
        yield Op("ft_arrays")
        yield draw((Op("ft_cd_density"), Op("ft_cd_gradient"), Op("ft_df_download"), Op("ft_density", (draw(GRAD_BITS),))))   # refused: no flag
        yield Op("tape_create", (2,))                      # refused: a forced tape exists
        yield a_read(pending)
        yield a_seed()
        yield Op("ft_sweep")
        yield Op("ft_download", (draw((F_U, F_H)),))

    def scene_ft_variant():
        """A recorded step, a switch between the tile and the column form, the sweep."""
        yield from ensure_ft()
        yield from ensure_on()
        yield Op("ft_taped", (1.0,))
        yield Op("variant", (3 if ab.variant != 3 else 0,))
        yield a_seed()
        yield Op("ft_sweep")
        yield Op("ft_path")
        yield Op("ft_download", (draw((F_U, F_H)),))
        yield Op("rk4", (1.0,))
        yield Op("vmix_path")
        yield a_read([(F_U, 1)])

    def scene_handoff():
        v = int(rng.integers(2))
        yield Op("tuning", (12, v))
        yield Op("rk4", (1.0,))
        yield a_read([(f, 1) for f in PROG])
        yield Op("tuning", (12, 1 - v))
        yield Op("rk4", (1.0,))
        yield a_read([(f, 1) for f in PROG])
        yield a_read(pending)

    def scene_only_cause():
        """Only a field, or only Cd, turns the pass on; then what the pass refuses."""
        yield from ensure_no_tape()
        cause = "cd" if (cfg.K == 1 or rng.random() < 0.5) else "field"
        if cause == "cd":
            yield from ensure_cd_free()
        if ab.visc in ("drag", "both", "other") or (cause == "cd" and ab.visc != "zero"):
            yield Op("visc", ("zero" if cause == "cd" or rng.random() < 0.5 else "nu",))
        if ab.stress in ("field", "other"):
            if ab.ft and ab.ft["n"] > 0:
                yield Op("ft_destroy")
            yield Op("stress", ("none",))
        if cause == "cd":
            if ab.field in FIELD_ON and cfg.K > 1:
                yield Op("field", (draw(("none", "zero")),))
            if ab.cd == "zero":
                yield Op("cd", (draw(CD_OK[1:]),))
        else:
            if ab.cd != "zero":
                yield Op("cd", ("zero",))
            if ab.field not in FIELD_ON:
                yield Op("field", (draw(("A", "B")),))
        c = [Op("fe", (int(rng.integers(4)),)), Op("run", (0, 3, int(rng.integers(4)), 1.0)), Op("rk4", (-1.0,)), Op("run", (1, 3, 0, -1.0))]
        if not ab.ft:
            c += [Op("tape_create", (2,))] * 2
        elif ab.ft["n"] < ab.ft["cap"]:
            c += [Op("ft_taped", (-1.0,))]
        for i in rng.permutation(len(c))[:2]:
            yield c[int(i)]
        yield a_read() or Op("download", (F_U, 1))
        if rng.random() < 0.5:
            yield Op("rk4", (1.0,))
            yield Op("vmix_path")
            yield a_read(pending)

    def scene_off_then_fe():
        yield from ensure_on()
        yield a_plain_step()
        yield from ensure_off()
        yield Op("fe", (int(rng.integers(4)),)) if rng.random() < 0.6 else Op("run", (0, 3, int(rng.integers(4)), 1.0))
        f = draw(PROG)
        yield a_read([(f, 1)])
        yield a_read(pending)

    def scene_plain_tape():
        if ab.ft:
            yield Op("ft_destroy")
        yield from ensure_off()
        yield from ensure_no_tape()
        yield Op("tape_create", (2,))
        for _ in range(2):
            yield draw((Op("visc", (draw(VISC_OK[1:]),)), Op("stress", (draw(("zero", "field")),)), Op("field", (draw(FIELD_OK[1:]),)),
                        Op("cd", (draw(CD_OK[1:]),)), Op("ft_create", (2,)), Op("ftq_create", (2,)), Op("cd", ("zero",)), Op("field", ("none",))))
        yield a_read() or Op("sumsq", (F_H, 1))
        yield Op("tape_destroy")

    def scene_ft_full():
        yield from ensure_ft()
        while ab.ft["n"] < ab.ft["cap"]:
            yield Op("ft_taped", (0.0 if rng.random() < 0.2 else 1.0,))
        yield Op("ft_taped", (1.0,))                        # refused: the tape is full
        yield a_read(pending)
        yield Op("ft_sweep") if not ab.ft["seeded"] else None     # refused: no seed
        yield a_seed()
        yield Op("ft_sweep")
        yield Op("ft_download", (draw((F_U, F_H)),))

    def a_refusal():
        c = [Op("visc", (draw(VISC_BAD),)), Op("stress", ("nan",)), Op("cd", (draw(CD_BAD),)), Op("sp_diag", (draw((2, -1)),))]
        c += [Op("field", (draw(FIELD_BAD),))] * 2 if cfg.K > 1 else []
        ft = ab.ft
        if ab.on():
            c += [Op("fe", (int(rng.integers(4)),)), Op("run", (0, 3, 0, 1.0)), Op("rk4", (-1.0,)), Op("run", (1, 3, 0, -1.0))]
            if not ft and not ab.tape:
                c += [Op("tape_create", (2,))] * 2
        if ab.cd != "zero" and not ft and not ab.tape:
            c += [Op("ft_create", (2,))] * 4
        if ft:
            c += [Op("tape_create", (2,)), Op("ft_create", (2,)), Op("ftq_create", (2,))]
            if not ft["quad"]:
                c += [Op("cd", (draw(CD_OK[1:]),)), Op("ft_want_cd", (int(rng.integers(2)),))] * 2
            if ft["n"] > 0:
                c += [Op("stress", (draw(("none", "zero", "field")),)), Op("ft_want", (draw(GRAD_BITS), int(rng.integers(2)))),
                      Op("ft_want_df", (int(rng.integers(2)),))] * 2
                if ft["quad"]:
                    c += [Op("ft_want_cd", (int(rng.integers(2)),))] * 2
                if not ft["seeded"]:
                    c += [Op("ft_sweep")] * 2
            if not ft["wantF"]:
                c += [Op("ft_df_download")]
            if not ft["wantCd"]:
                c += [Op("ft_cd_density"), Op("ft_cd_gradient")]
            if ft["want"] != 7:
                c += [Op("ft_density", (draw([b for b in GRAD_BITS if not ft["want"] & b]),))]
            if ft["n"] < ft["cap"] and ab.on():
                c += [Op("ft_taped", (-1.0,))] * 3
        return draw(c)

    def scene_refusal_read():
        yield a_refusal()
        yield a_read() or Op(draw(READ_KINDS[::2]), (draw(PROG), int(rng.integers(2))))

    def a_single():
        ft = ab.ft
        c = [("step", 4), ("field", 3), ("upload", 3), ("variant", 2.5), ("tuning", 2.5), ("getter", 3), ("refusal", 4)]
        if not ab.tape:
            c += [("visc", 2)]
        if stress_free():
            c += [("stress", 1.5)]
        if cd_free():
            c += [("cd", 3)]
        if not ab.on():
            c += [("fe", 2), ("run_fe", 1)]
        if ft:
            c += [("ft", 5)]
        name = draw([x[0] for x in c], [x[1] for x in c])
        if name == "step":
            return a_plain_step()
        if name == "visc":
            return Op("visc", (draw([p for p in VISC_OK if p != ab.visc]),))
        if name == "stress":
            return Op("stress", (draw([p for p in STRESS_OK[:3] if p != ab.stress]),))
        if name == "field":
            return Op("field", (draw([p for p in FIELD_OK if p != ab.field]),)) if not ab.tape else Op("field_download")
        if name == "cd":
            return Op("cd", (draw([p for p in CD_OK if p != ab.cd]),))
        if name == "upload":
            return Op("upload", (draw(PROG), int(rng.integers(2)), vseed()))
        if name == "variant":
            return Op("variant", (draw([v for v in cfg.variants if v != ab.variant]),))
        if name == "tuning":
            return a_tuning()
        if name == "getter":
            return draw((Op("visc_read"), Op("has_stress"), Op("vmix_path"), Op("field_download"), Op("has_field"), Op("cd_read"),
                         Op("sp_download"), Op("sp_diag", (int(rng.integers(2)),)), Op("ft_arrays"), Op("ft_path")))
        if name == "refusal":
            return a_refusal()
        if name == "fe":
            return Op("fe", (int(rng.integers(4)),))
        if name == "run_fe":
            return Op("run", (0, 3, int(rng.integers(4)), 1.0))
        if ft["n"] > 0 and ft["seeded"]:
            return Op("ft_sweep")
        if ft["n"] > 0 and rng.random() < 0.5:
            return a_seed()
        if ft["n"] < ft["cap"]:
            return Op("ft_taped", (0.0 if rng.random() < 0.15 else 1.0,))
        return Op("ft_destroy") if rng.random() < 0.4 else a_seed()

    scenes = [(scene_mixed_read, 4), (scene_change_then_read, 4), (scene_field_cycle, 3), (scene_zero_field, 2.5), (scene_runs, 2),
              (scene_sp, 2.5), (scene_ftq_cd, 2.5), (scene_ft_fields, 2.5 if cfg.K > 1 else 0.5), (scene_second_seed, 2.5), (scene_zero_u, 2),
              (scene_plain_quiet, 2.5), (scene_handoff, 2), (scene_only_cause, 3.5), (scene_off_then_fe, 2), (scene_plain_tape, 2.5),
              (scene_ft_full, 1.5), (scene_refusal_read, 4), (scene_step_upload_read, 3)]
    if cfg.K > 1 and 3 in cfg.variants:
        scenes += [(scene_ft_variant, 3)]
    scene = None
    while len(ops) < cfg.nops:
        if scene is not None:
            try:
                op = next(scene)
            except StopIteration:
                scene = None
                continue
            if op is not None:
                ops.append(op)
                ab.accept(op)
            continue
        r = rng.random()
        if ab.dirty and r < 0.25:
            op = a_read()
        elif r < 0.7:
            scene = draw([s[0] for s in scenes], [s[1] for s in scenes])()
            continue
        else:
            op = a_single()
        ops.append(op)
        ab.accept(op)
    return ops[:cfg.nops]


# ---------------------------------------------------------------------------------------------------------------------------------
# host model
# ---------------------------------------------------------------------------------------------------------------------------------
class MixingModel(cv.ForcedModel):
    """Machine E on the CPU oracle and the twins, eagerly, as include/moka_hip.h words each call.  mutant: one of E_MUTANTS."""

    def __init__(self, cfg, seed, mutant=None):
        assert mutant is None or mutant in E_MUTANTS
        super().__init__(cfg, seed, mutant if mutant in cs.MUTANTS else None)
        self.mutant = mutant
        self.c1, self.c2 = mv.edge_cells(self.mesh)
        self.fld = None                # the field as uploaded (None: no field), and the pattern it came from
        self.pattern = "none"
        self.fld_gen = 0               # a new value with every accepted upload and removal
        self.cd = 0.0
        self.sp_last = np.zeros(self.mesh.nEdges)       # what moka_bottom_speed_download answers
        self.nu_dead = False           # mutant scalar_lost
        self.lag = None                # mutants field_late, cd_late: what the previous step ran with

    # ---- the pass ----
    def _effective(self, nu, fld):
        if self.mutant == "zero_field_transparent" and fld is not None and not mf.field_on(fld, self.mlt):
            fld = None
        if self.mutant == "scalar_lost" and self.nu_dead and fld is None:
            nu = 0.0
        return nu, fld

    def on(self):
        return mf.pass_on(self.mix.nu, self.mix.drag, self.mix.tau, self.mlt, self.fld) or self.cd != 0.0

    def why(self):
        """"_field" / "_cd" when a field alone / Cd alone turns the pass on, else ""."""
        mx = self.mix
        if mx.drag != 0.0 or mv.stress_on(mx.tau, self.mlt):
            return ""
        f = mf.pass_on(mx.nu, 0.0, None, self.mlt, self.fld)
        if self.cd != 0.0:
            return "" if f else "_cd"
        return "_field" if (f and self.fld is not None) else ""

    def _step_rk4(self, dt, s13=False):
        st, mx, K = self.st, self.mix, self.cfg.K
        fld, pattern, cd = self.fld, self.pattern, self.cd
        if self.mutant in ("field_late", "cd_late"):
            lag, self.lag = self.lag, (fld, pattern, cd)
            if lag is not None:
                fld, pattern = lag[:2] if self.mutant == "field_late" else (fld, pattern)
                cd = lag[2] if self.mutant == "cd_late" else cd
        cs.Model._step_rk4(self, dt, s13)
        nu, fld = self._effective(mx.nu, fld)
        drag, tau = mx.drag, mx.tau
        st_on = mv.stress_on(tau, self.mlt)
        on = mf.pass_on(nu, drag, tau, self.mlt, fld) or cd != 0.0
        nu_t, fld_t = mf.taken(nu, fld, self.mlt)
        us = st.u[1].copy()
        self.last = dict(on=on, mixed=False, launched=False, dt=dt, nu=nu_t, drag=drag, tau=tau if st_on else None,
                         fld=None if fld_t is None else fld_t.copy(), cd=cd, us=us, sp=np.zeros(self.mesh.nEdges), nuV=mx.nu != 0.0, nu_set=mx.nu,
                         field=None if fld is None else ("on" if fld_t is not None else "zero"), pattern=pattern)
        if not on or dt == 0.0:
            return
        self.last["mixed"] = True
        new, sp = qd.apply(us, st.h[1], self.mlt, self.c1, self.c2, dt, nu, drag, tau, cd, self.mesh, qd.bottom_speed, fld)
        if self.mutant == "cd_skips_n1" and cd != 0.0 and drag == 0.0 and not st_on:
            n1 = np.minimum(self.mlt, K) == 1
            new[n1] = us[n1]
        st.u[1][...] = new
        if not (K < 2 and drag == 0.0 and cd == 0.0 and not st_on):      # a pass was launched
            self.last["launched"] = True
            self.path = mv.form_of(K, self.variant == 3)
            if cd != 0.0:
                self.sp_last = qd.bottom_speed(new, self.mlt, self.mesh) if self.mutant == "sp_from_mixed" else sp
            elif self.mutant != "sp_stale":
                self.sp_last = np.zeros(self.mesh.nEdges)
            self.last["sp"] = sp
        self._clean_diag()             # the diagnostics of the new level come from the mixed u

    # ---- the forced tape ----
    def _arrays(self):
        ft = self.ft
        return len(ft["dens"]) + (4 if ft["unrec"] else 0) + (1 if ft["sprec"] else 0) + (2 if ft["usrec"] else 0) + ft["copies"]

    def _ft_sweep(self):
        ft, K = self.ft, self.cfg.K
        XU, XH = ft["X"]
        dens = {b: ft["dens"][b] for b in GRAD_BITS if ft["want"] & b}
        if ft["wantCd"]:
            dens[qa.QUADRATIC] = ft["dens"][qa.QUADRATIC]
        DF = ft["dens"]["F"] if ft["wantF"] else None
        generic = self.variant == 3
        newest = next((r["fld"] for r in reversed(ft["recs"]) if r["fld"] is not None), None)
        for r in reversed(ft["recs"]):
            if r["rec"] and r["dt"] != 0.0:
                fld, cd = r["fld"], r["cd"]
                if self.mutant == "tape_field_newest" and fld is not None:
                    fld = newest
                if self.mutant == "tape_cd_current" and cd != 0.0:      # the state's Cd, zero included: the recorded drag then vanishes
                    cd = self.cd
                chain = qa.speed_transpose
                if self.mutant == "kink_divides" and cd != 0.0:
                    bad = (r["sp"] == 0.0) & (np.minimum(self.mlt, K) >= 1)
                    chain = lambda mesh, mlt, X, us, M: qa.speed_transpose(mesh, mlt, X, us, np.where(bad, np.inf, M))     # noqa: E731
                XU, XH = qa.transposed_pass(self.mesh, self.mlt, XU, XH, r["un"], r["hn"], r["dt"], r["nu"], r["drag"], r["tau"], fld, dens, DF,
                                            cd, r["sp"], r["us"], chain)
                if ft["want"] or ft["wantF"] or (r["sp"] is not None and ft["wantCd"]) or \
                        (r["on"] and not (K < 2 and r["drag"] == 0.0 and r["cd"] == 0.0 and r["tau"] is None)):
                    ft["path"] = mf.adjoint_form(K, r["fld"] is not None, generic)[0]
            XU, XH = self._reverse_rk4(r["P"], r["dt"], XU, XH)
        ft["X"] = (XU, XH)
        ft["recs"] = []
        ft["copies"] = 0               # the tape is empty: the field copies are released

    # ---- one op ----
    def apply(self, op):
        o = self._apply(op)
        if op.kind in STEP_KINDS and o.rc == OK:
            o.info = {k: v for k, v in self.last.items() if k not in ("us", "sp", "fld", "tau")}
        if o.refusal in CAUSE_REFUSALS:
            o.refusal += self.why()
        return o

    def _apply(self, op):
        cfg, st, k, a, mx, ft = self.cfg, self.st, op.kind, op.args, self.mix, self.ft
        K, nE = cfg.K, self.mesh.nEdges
        R = lambda code, name: Obs(k, code, refusal=name)       # noqa: E731
        if k in FT_OWN and ft is None:
            return R(ERR_ARG, "null_handle")
        if k == "field":
            f = field_values(cfg, a[0])
            if f is not None and not mf.check_field(f, self.mlt):
                return R(ERR_ARG, "field_invalid")
            if f is None and self.fld is None:
                return Obs(k, OK)                              # nothing to remove: the call does nothing at all
            if self.tape is not None and (f is not None or mx.nu != 0.0):
                return R(ERR_UNSUPPORTED, "field_tape" if f is not None else "field_removal_tape")
            if f is None:
                self.nu_dead = True
            self.fld, self.pattern = f, a[0]
            self.fld_gen += 1
            return Obs(k, OK)
        if k == "visc":
            o = super()._apply(op)
            if o.rc == OK:
                self.nu_dead = False
            return o
        if k == "field_download":
            return Obs(k, OK, value=bits(np.zeros((nE, K)) if self.fld is None else self.fld))
        if k == "has_field":
            return Obs(k, OK, value=int(self.fld is not None))
        if k == "cd":
            c = cd_values(cfg, a[0])
            if not (c >= 0.0 and np.isfinite(c)):
                return R(ERR_ARG, "cd_invalid")
            if c != 0.0 and self.tape is not None:
                return R(ERR_UNSUPPORTED, "cd_tape")
            if c != 0.0 and ft is not None and not ft["quad"]:
                return R(ERR_UNSUPPORTED, "cd_plain_tape")
            self.cd = c
            return Obs(k, OK)
        if k == "cd_read":
            return Obs(k, OK, value=self.cd)
        if k == "sp_download":
            return Obs(k, OK, value=self.sp_last.copy())
        if k == "sp_diag":
            if a[0] not in (0, 1):
                return R(ERR_ARG, "sp_diag_level")
            return Obs(k, OK, value=qd.bottom_speed(st.u[a[0]], self.mlt, self.mesh))
        if k == "upload_zero_u":
            st.u[1][...] = 0.0
            return Obs(k, OK, key=(F_U, 1))
        if k == "upload_rest_h":
            st.h[1][...] = resting_thickness(cfg)
            self.ssh_loose = True
            return Obs(k, OK, key=(F_H, 1))
        if k == "tape_create" and self.tape is not None:
            raise ValueError("the generator never asks for a second moka_tape")
        if k in ("ft_create", "ftq_create"):
            if self.tape is not None:
                return R(ERR_UNSUPPORTED, "ft_tape")
            if k == "ft_create" and self.cd != 0.0:
                return R(ERR_UNSUPPORTED, "ft_create_cd")
            if ft is not None:
                return R(ERR_UNSUPPORTED, "ft_second")
            z = lambda f: np.zeros(shape_of(cfg, f))           # noqa: E731
            self.ft = dict(cap=a[0], recs=[], seeded=False, want=0, dens={}, X=(z(F_U), z(F_H)), path=0, quad=k == "ftq_create",
                           wantF=False, wantCd=False, unrec=False, sprec=False, usrec=False, copies=0, vfgen=None)
            return Obs(k, OK)
        if k == "ft_arrays":
            return Obs(k, OK, value=0 if ft is None else self._arrays())
        if k == "ft_want_df":
            if ft["recs"]:
                return R(ERR_ARG, "ft_want_df_recorded")
            if a[0] and "F" not in ft["dens"]:
                ft["dens"]["F"] = np.zeros((nE, K))
            ft["wantF"] = bool(a[0])
            return Obs(k, OK)
        if k == "ft_want_cd":
            if not ft["quad"]:
                return R(ERR_UNSUPPORTED, "ft_want_cd_plain")
            if ft["recs"]:
                return R(ERR_ARG, "ft_want_cd_recorded")
            if a[0] and qa.QUADRATIC not in ft["dens"]:
                ft["dens"][qa.QUADRATIC] = np.zeros(nE)
            ft["wantCd"] = bool(a[0])
            return Obs(k, OK)
        if k == "ft_df_download":
            if not ft["wantF"]:
                return R(ERR_ARG, "ft_df_unflagged")
            return Obs(k, OK, value=ft["dens"]["F"].copy())
        if k in ("ft_cd_density", "ft_cd_gradient"):
            if not ft["wantCd"]:
                return R(ERR_ARG, "ft_cd_unflagged")
            d = ft["dens"][qa.QUADRATIC]
            return Obs(k, OK, value=d.copy() if k == "ft_cd_density" else fa.host_sum(d))
        if k in ("ft_seed_ssh", "ft_seed_free") and ft is not None and self.mutant == "dens_not_zeroed":
            kept = {b: d.copy() for b, d in ft["dens"].items()}
            o = super()._apply(op)
            for b, d in kept.items():
                ft["dens"][b][...] = d
            return o
        if k == "ft_taped":
            dt = dt_of(cfg, a[0])
            if len(ft["recs"]) >= ft["cap"]:
                return R(ERR_ARG, "ft_full")
            if not ft["quad"] and self.cd != 0.0:
                return R(ERR_UNSUPPORTED, "ft_taped_cd")
            if dt < 0.0 and self.on():
                return R(ERR_ARG, "dt_negative_ft")
            on = self.on()
            rec = on or ft["want"] != 0 or ft["wantF"] or ft["wantCd"]
            qdr = ft["quad"] and self.cd != 0.0 and dt != 0.0
            wsp = qdr or (ft["wantCd"] and dt != 0.0)
            ft["unrec"] = ft["unrec"] or rec
            ft["sprec"] = ft["sprec"] or wsp
            ft["usrec"] = ft["usrec"] or qdr
            if on and self.fld is not None and mf.field_on(self.fld, self.mlt) and (ft["copies"] == 0 or ft["vfgen"] != self.fld_gen):
                ft["copies"] += 1
                ft["vfgen"] = self.fld_gen
            u0, h0 = st.u[1].copy(), st.h[1].copy()
            P, pu, ph = [(u0, h0)], u0, h0
            for s in (dt / 2., dt / 2., dt):
                tu, th, _ = self.om.tendencies_clean(pu, ph)
                pu, ph = u0 + s * tu, h0 + s * th
                P.append((pu, ph))
            self._step_rk4(dt)
            L = self.last
            cd = L["cd"] if qdr else 0.0
            sp = L["sp"] if cd != 0.0 else qd.bottom_speed(L["us"], self.mlt, self.mesh) if wsp else None
            ft["recs"].append(dict(P=P, dt=float(dt), rec=rec, on=L["on"], un=st.u[1].copy(), hn=st.h[1].copy(), nu=L["nu"], drag=L["drag"],
                                   tau=L["tau"], fld=L["fld"], cd=cd, sp=sp, us=L["us"] if cd != 0.0 else None))
            ft["seeded"] = False
            return Obs(k, OK)
        return super()._apply(op)

    def run(self, ops):
        """As call_sequences_vertical.ForcedModel.run, with this machine's ops that fall between a change and its read."""
        out = []
        keys = STATE_KEYS + cs.ADJ_KEYS
        before = self._snapshot()
        for op in ops:
            o = self.apply(op)
            if op.kind in READ_KINDS:
                if o.rc == OK:
                    cur = self.array(o.key)
                    o.fresh = not np.array_equal(self._last_read.get(o.key), cur)
                    o.after = frozenset(self._changed[o.key])
                    self._changed[o.key] = set()
                    self._last_read[o.key] = cur.copy()
            elif op.kind not in FT_READS + GETTERS:
                now = self._snapshot()
                for key in keys:
                    if not np.array_equal(before[key], now[key]):
                        self._changed[key].add(op.kind)
                    elif o.rc == OK and op.kind in NON_ARRAY_OPS and self._changed[key]:
                        self._changed[key].add(op.kind)
                before = now
            out.append(o)
        return out


def model_of(cfg, seed, mutant=None):
    return (ClosureModel if isinstance(cfg, FConfig) else MixingModel)(cfg, seed, mutant)


def sequence_of(cfg, seed):
    return f_sequence(cfg, seed) if isinstance(cfg, FConfig) else sequence(cfg, seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# device runner
# ---------------------------------------------------------------------------------------------------------------------------------
class MixingDevice:
    """Machine E through moka_hip.lib: one device mesh per config, shared by its seeds; run() gives each sequence a fresh state.  Every
    status code is an observation; a HIP error ends the sequence there (RuntimeError with moka_last_error) and every later sequence
    of the config before it launches anything (`dead`)."""

    def __init__(self, backend, cfg):
        import moka_hip as mk
        from moka_hip import lib as L
        self.L, self.lib, self.backend, self.cfg = L, L.lib(), backend, cfg
        hm = mk.HorzMesh(get_mesh(cfg.meshname))
        vm = mk.VerticalMesh(hm, nVertLevels=cfg.K, restingThickness=resting_thickness(cfg), multilayer=True)
        mlt = mask_of(cfg)
        if mlt is not None:
            vm.maxLevelEdge.Top[:] = mlt
        self.M = mk.Mesh(hm, vm, backend=backend)
        self.counters = {"sequences": 0, "rk4_steps": 0, "fe_steps": 0, "paths": set(), "ft_paths": set(), "mixed_field": 0, "mixed_cd": 0,
                         "run9_field": 0, "run9_cd": 0, "sweeps": 0, "sweeps_df": 0, "sweeps_dcd": 0, "handoff": 0, "no_handoff": 0}
        self.dead = None               # the message of a HIP error: no later sequence of this config launches anything

    def close(self):
        self.M.close()

    def run(self, ops, seed):
        if self.dead:
            raise RuntimeError("an earlier sequence of this config ended in a HIP error, nothing more is launched: " + self.dead)
        L, lib, cfg, ctx = self.L, self.lib, self.cfg, self.backend._h
        cnt = self.counters
        hS, hT, hF = C.c_void_p(), C.c_void_p(), C.c_void_p()
        saved = {}
        out = []
        nE = get_mesh(cfg.meshname).nEdges
        mlt = depths_of(cfg)
        vp = lambda arr: arr.ctypes.data_as(C.c_void_p)        # noqa: E731

        def tune(key, value):
            if key not in saved:
                v = C.c_int()
                L.check(lib.moka_get_tuning(key, C.byref(v)))
                saved[key] = v.value
            return lib.moka_set_tuning(key, value)

        # what the last accepted ops carried, and what the open tape has flagged and recorded (for the counters only)
        force = {"fld": None, "cd": 0.0, "wantF": False, "wantCd": False, "n": 0}

        def stepped(n, dt, nine=False):
            cnt["rk4_steps"] += n
            if dt != 0.0:
                f = force["fld"] is not None and mf.field_on(force["fld"], mlt)
                cnt["mixed_field"] += n * f
                cnt["mixed_cd"] += n * (force["cd"] != 0.0)
                cnt["run9_field"] += nine and f
                cnt["run9_cd"] += nine and force["cd"] != 0.0
                p = lib.moka_state_momentum_vmix_path(hS)
                if p:
                    cnt["paths"].add(p)

        try:
            L.check(lib.moka_state_create(ctx, self.M._h, C.byref(hS)), ctx)
            for (f, l), arr in initial_state(cfg, seed).items():
                L.check(lib.moka_state_upload(hS, f, l, L.f64(arr)), ctx)
            for op in ops:
                k, a = op.kind, op.args
                value = None
                if k == "visc":
                    rc = lib.moka_set_vertical_viscosity(hS, *visc_values(cfg, a[0]))
                elif k == "stress":
                    tau = stress_values(cfg, a[0])
                    rc = lib.moka_surface_stress_upload(hS, None if tau is None else vp(tau))
                elif k == "field":
                    f = field_values(cfg, a[0])
                    rc = lib.moka_vertical_viscosity_field_upload(hS, None if f is None else vp(f))
                    if rc == OK:
                        force["fld"] = f
                elif k == "field_download":
                    v = np.full((nE, cfg.K), 7.0)
                    rc = lib.moka_vertical_viscosity_field_download(hS, vp(v))
                    value = bits(v)
                elif k == "has_field":
                    v = C.c_int(-1)
                    rc = lib.moka_has_vertical_viscosity_field(hS, C.byref(v))
                    value = v.value
                elif k == "cd":
                    rc = lib.moka_set_quadratic_bottom_drag(hS, cd_values(cfg, a[0]))
                    if rc == OK:
                        force["cd"] = cd_values(cfg, a[0])
                elif k == "cd_read":
                    v = C.c_double(np.nan)
                    rc = lib.moka_quadratic_bottom_drag(hS, C.byref(v))
                    value = v.value
                elif k == "sp_download":
                    value = np.full(nE, np.nan)
                    rc = lib.moka_bottom_speed_download(hS, vp(value))
                elif k == "sp_diag":
                    value = np.full(nE, np.nan)
                    rc = lib.moka_bottom_speed(hS, a[0], vp(value))
                elif k == "visc_read":
                    nu, r = C.c_double(np.nan), C.c_double(np.nan)
                    rc = lib.moka_vertical_viscosity(hS, C.byref(nu), C.byref(r))
                    value = (nu.value, r.value)
                elif k == "stress_download":
                    value = np.full(nE, np.nan)
                    rc = lib.moka_surface_stress_download(hS, vp(value))
                elif k == "has_stress":
                    v = C.c_int(-1)
                    rc = lib.moka_has_surface_stress(hS, C.byref(v))
                    value = v.value
                elif k == "vmix_path":
                    rc, value = OK, lib.moka_state_momentum_vmix_path(hS)
                elif k == "rk4":
                    value = lib.moka_state_rk4_streams(hS)
                    rc = lib.moka_step_rk4(hS, dt_of(cfg, a[0]))
                    if rc == OK:
                        stepped(1, a[0])
                        nc, ne = C.c_int64(), C.c_int64()
                        took = lib.moka_state_rk_handoff_escapes(hS, C.byref(nc), C.byref(ne))
                        if took not in (OK, ERR_UNSUPPORTED):
                            rc = took
                        cnt["handoff" if took == OK else "no_handoff"] += 1
                elif k == "run":
                    rc = lib.moka_run(hS, a[0], dt_of(cfg, a[3]) if a[0] == 1 else cfg.dt, a[1], a[2])
                    if rc == OK and a[0] == 1:
                        stepped(a[1], a[3], nine=a[1] == 9)
                    elif rc == OK:
                        cnt["fe_steps"] += a[1]
                elif k == "fe":
                    rc = lib.moka_step_fe(hS, cfg.dt, a[0])
                    cnt["fe_steps"] += rc == OK
                elif k == "variant":
                    rc = lib.moka_set_kernel_variant(ctx, a[0])
                elif k == "tuning":
                    rc = tune(a[0], a[1])
                elif k == "upload":
                    rc = lib.moka_state_upload(hS, a[0], a[1], L.f64(values(cfg, a[0], a[2])))
                elif k == "upload_zero_u":
                    rc = lib.moka_state_upload(hS, F_U, 1, L.f64(np.zeros(shape_of(cfg, F_U))))
                elif k == "upload_rest_h":
                    rc = lib.moka_state_upload(hS, F_H, 1, L.f64(np.ascontiguousarray(resting_thickness(cfg))))
                elif k == "download":
                    value = np.full(shape_of(cfg, a[0]), np.nan)
                    rc = lib.moka_state_download(hS, a[0], a[1], L.f64(value))
                elif k == "rows":
                    rows = np.asarray(a[2], dtype=np.int32)
                    value = np.full((rows.size, 1 if a[0] == F_SSH else cfg.K), np.nan)
                    rc = lib.moka_state_download_rows(hS, a[0], a[1], rows.size, L.i32(rows), L.f64(value))
                elif k == "sumsq":
                    s = C.c_double(np.nan)
                    rc = lib.moka_sum_sq(hS, a[0], a[1], C.byref(s))
                    value = s.value
                elif k == "tape_create":
                    h = C.c_void_p()
                    rc = lib.moka_tape_create(hS, a[0], C.byref(h))
                    if rc == OK:
                        hT = h
                elif k == "tape_destroy":
                    lib.moka_tape_destroy(hT)
                    hT, rc = C.c_void_p(), OK
                elif k in ("ft_create", "ftq_create"):
                    h = C.c_void_p()
                    rc = (lib.moka_forced_tape_create if k == "ft_create" else lib.moka_forced_tape_create_quadratic)(hS, a[0], C.byref(h))
                    if rc == OK:
                        hF = h
                        force.update(wantF=False, wantCd=False, n=0)
                elif k == "ft_destroy":
                    lib.moka_forced_tape_destroy(hF)
                    hF, rc = C.c_void_p(), OK
                elif k == "ft_want":
                    rc = lib.moka_forced_adjoint_want_gradient(hF, a[0], a[1])
                elif k == "ft_want_df":
                    rc = lib.moka_forced_adjoint_want_viscosity_field_gradient(hF, a[0])
                    if rc == OK:
                        force["wantF"] = bool(a[0])
                elif k == "ft_want_cd":
                    rc = lib.moka_forced_adjoint_want_quadratic_drag_gradient(hF, a[0])
                    if rc == OK:
                        force["wantCd"] = bool(a[0])
                elif k == "ft_taped":
                    rc = lib.moka_step_rk4_forced_taped(hF, dt_of(cfg, a[0]))
                    if rc == OK:
                        stepped(1, a[0])
                        force["n"] += 1
                elif k == "ft_seed_ssh":
                    rc = lib.moka_forced_adjoint_seed_sum_sq_ssh(hF)
                elif k == "ft_seed_free":
                    XU, XH = free_seed(cfg, a[0])
                    rc = lib.moka_forced_adjoint_seed(hF, vp(XU), vp(XH))
                elif k == "ft_sweep":
                    rc = lib.moka_forced_adjoint_sweep(hF)
                    if rc == OK:
                        cnt["sweeps"] += 1
                        cnt["sweeps_df"] += force["wantF"] and force["n"] > 0
                        cnt["sweeps_dcd"] += force["wantCd"] and force["n"] > 0
                        force["n"] = 0
                        p = lib.moka_forced_tape_vmix_path(hF)
                        if p:
                            cnt["ft_paths"].add(p)
                elif k == "ft_download":
                    value = np.full(shape_of(cfg, a[0]), np.nan)
                    rc = lib.moka_forced_adjoint_download(hF, a[0], vp(value))
                elif k == "ft_density":
                    value = np.full(nE, np.nan)
                    rc = lib.moka_forced_adjoint_density_download(hF, a[0], vp(value))
                elif k == "ft_gradient":
                    s = C.c_double(np.nan)
                    rc = lib.moka_forced_adjoint_gradient(hF, a[0], C.byref(s))
                    value = s.value
                elif k == "ft_df_download":
                    value = np.full((nE, cfg.K), np.nan)
                    rc = lib.moka_forced_adjoint_viscosity_field_density_download(hF, vp(value))
                elif k == "ft_cd_density":
                    value = np.full(nE, np.nan)
                    rc = lib.moka_forced_adjoint_quadratic_drag_density_download(hF, vp(value))
                elif k == "ft_cd_gradient":
                    s = C.c_double(np.nan)
                    rc = lib.moka_forced_adjoint_quadratic_drag_gradient(hF, C.byref(s))
                    value = s.value
                elif k == "ft_arrays":
                    rc, value = OK, int(lib.moka_forced_tape_device_arrays(hF))
                elif k == "ft_path":
                    rc, value = OK, (lib.moka_forced_tape_vmix_path(hF) if hF else 0)
                else:
                    raise ValueError(f"unknown op {op}")
                if rc == ERR_HIP:
                    self.dead = f"config {cfg.name} seed {seed}: HIP error at op {len(out)} ({op}): {lib.moka_last_error(ctx)}"
                    raise RuntimeError(self.dead)
                out.append(Obs(k, int(rc), value=value if rc == OK else None))
            cnt["sequences"] += 1
        finally:
            if not self.dead:              # after a HIP error nothing more is sent to the device, the destroy calls included
                if hF:
                    lib.moka_forced_tape_destroy(hF)
                if hT:
                    lib.moka_tape_destroy(hT)
                if hS:
                    lib.moka_state_destroy(hS)
            lib.moka_set_kernel_variant(ctx, 0)
            for key, v in saved.items():
                lib.moka_set_tuning(key, v)
        return out


def device_of(backend, cfg):
    return (ClosureDevice if isinstance(cfg, FConfig) else MixingDevice)(backend, cfg)


# ---------------------------------------------------------------------------------------------------------------------------------
# machine F: tracers under the Richardson closure.  Model: call_sequences_vertical.VTracerModel whose step is
# richardson_twin.RichardsonTwin.step_rk4 (the closure on: F and G from u*, h_new and phi*_jb, the field forms of both passes; off: the
# chain's step with the set-aside coefficients), and richardson_twin.edge_field / cell_field behind moka_richardson_diagnose.
# ---------------------------------------------------------------------------------------------------------------------------------
F_MUTANTS = ("rich_late", "aside_lost", "setter_dropped", "rich_from_mixed", "fields_stale", "mask_ignored", "drag_set_aside",
             "levels_swapped", "set_tracers_keeps", "coeff_late", "mixed_flow_early", "prev_level_lost")
RICH_ON = ("P0", "P1", "mask_in", "mask_out", "unit")
RICH_BAD = ("neg", "nan", "range")
F_READS = READ_KINDS + ("tr_download",)
F_GETTERS = ("rich_read", "rich_read_null", "rich_fields", "rich_diag", "kappaV_read", "has_vfield", "visc_read", "has_field", "cd_read")
F_STEPS = ("rk4", "run")
F_SETTERS = ("kappaV", "vfield", "visc", "field")
F_NON_ARRAY = ("tuning", "variant", "rich", "kappaV", "vfield", "visc", "field", "cd", "stress", "tr_tape_create", "tr_tape_destroy")


@dataclass(frozen=True)
class FConfig(cv.VTracerConfig):
    depths: str = "full"

    machine = "F"


F_CONFIGS = {c.name: c for c in (
    # cells with nLev < 2 and edges with n < 2 have no interface; the cell sum omits slots too shallow for k+1; 60 of 64 lanes
    FConfig("F1", "hex6x4", 60, dt=2.0, nT=3, nops=44, depths="shelf", reach=("vpath_1", "handoff")),
    # heptagon slot lists, narrow lane groups, both forms of both passes
    FConfig("F2", "ico6f", 6, dt=20.0, nT=5, tracer_path=2, nops=44, variants=(0, 3), reach=("vpath_1", "vpath_2")),
    # the closure is on and launches nothing: F and G read zero, the momentum pass is the one it was
    FConfig("F3", "hex4x4", 1, dt=2.0, nT=2, nops=44, reach=()),
)}
ALL_CONFIGS.update(F_CONFIGS)


def buoyancy_values(cfg, level):
    """richardson_twin.buoyancy over this config's mesh: a stable profile with exact copies (db == 0) and inversions (db < 0)."""
    import richardson_twin as rt
    import tracer_cases as tc
    tc._MESHES.setdefault(cfg.meshname, get_mesh(cfg.meshname))        # the one mesh, under the one name, for richardson_twin's helper
    return np.ascontiguousarray(rt.buoyancy(cfg.meshname, cfg.K, seed=5 + level))


def rich_params(cfg, pattern, nT):
    """(richardson_twin.Params or None, valid): the parameter patterns of a `rich` op for a state with nT tracers."""
    import richardson_twin as rt
    if pattern == "off":
        return None
    kw = {"P0": {}, "P1": dict(nu0=0.01, alpha=3.0, nuB=2e-4, kB=2e-5, conv=0.5), "mask_in": dict(tracers=[0, 1]),
          "mask_out": dict(tracers=[0]), "unit": dict(buoyancy=0, nu0=0.008), "neg": dict(nu0=-0.005), "nan": dict(alpha=float("nan")),
          "range": dict(buoyancy=nT)}[pattern]
    return rt.Params(**{"buoyancy": 1, **kw})


def f_vocabulary(cfg):
    v = ("set_tracers", "tr_upload", "tr_buoy", "tr_download", "kappaV", "vfield", "kappaV_read", "has_vfield", "visc", "visc_read", "field",
         "has_field", "cd", "cd_read", "stress", "rich", "rich_read", "rich_read_null", "rich_fields", "rich_diag", "rk4", "run", "fe", "upload", "download", "rows", "sumsq",
         "tuning", "tr_tape_create", "tr_tape_destroy", "tape_create", "ft_create", "ftq_create")
    return v + (("variant",) if len(cfg.variants) > 1 else ())


def f_arg_class(op):
    k, a = op.kind, op.args
    if k in ("set_tracers", "kappaV", "visc", "field", "cd", "stress", "rich", "variant", "rk4", "rich_fields"):
        return (k, a[0])
    if k == "vfield":
        return (k, a[1])
    if k in ("rich_diag", "tuning"):
        return (k, a[0], a[1])
    if k == "run":
        return (k, a[0], a[1])
    return None


def f_arg_classes(cfg):
    c = [("set_tracers", n) for n in (2, cfg.nT)] + [("kappaV", p) for p in cv.KV_PATTERNS] + [("vfield", p) for p in ("none", "zero", "A")]
    c += [("visc", p) for p in ("zero", "nu", "drag", "both")] + [("field", p) for p in ("none", "zero", "A")] + [("cd", p) for p in ("zero", "cd")]
    c += [("stress", p) for p in ("none", "field")] + [("rich", p) for p in ("off",) + RICH_ON] + [("rk4", f) for f in (1.0, 0.0)]
    c += [("run", 1, 3), ("run", 1, 9)] + [("rich_fields", w) for w in ("both", "F", "G")] + [("rich_diag", l, w) for l in (0, 1) for w in ("all",)]
    c += [("rich_diag", 1, "F")] + [("tuning", k, v) for k in (7, 12) for v in (0, 1)] + [("tuning", 8, v) for v in cs.TUNING_VALUES[8]] + [("variant", v) for v in cfg.variants if len(cfg.variants) > 1]
    return tuple(c)


def f_refusals(cfg):
    return ("rich_null", "rich_invalid", "rich_range", "rich_no_tracers", "rich_tracer_tape", "rich_diag_level", "rich_diag_off", "tr_tape_rich", "tape_rich",
            "ft_rich", "ftq_rich", "fe_rich", "run_fe_rich", "dt_negative_rk4", "dt_negative_run")


def f_pairs_wanted(cfg):
    w = ("set_tracers", "tr_upload", "tr_buoy", "rk4", "run", "rich", "kappaV", "vfield", "visc", "field", "cd")
    return {(k, "tr_download") for k in w} | {(k, r) for k in ("rk4", "run") for r in READ_KINDS}, ()


def f_cases_wanted(cfg):
    c = ("on_off_on", "params_between_runs", "fields_zero_without", "fields_dt0", "set_tracers_off",
         "mask_split", "unit_buoyancy", "tape_blocks", "toggle_on_7", "toggle_on_8", "toggle_on_12", "drag_under_closure")
    # (K = 1: no field has an active interface, so neither kind of field can be "on"; nuV and kappaV count by their values)
    c += tuple(x + s for x in ("setter_then_off_", "acts_again_") for s in (F_SETTERS if cfg.K > 1 else ("kappaV", "visc")))
    return c + (("diag_levels",) if cfg.K > 1 else ())      # K = 1: both levels diagnose to zeros


def f_cases_seen(cfg, ops, obs):
    """The named orders of machine F a sequence shows (Obs.info of a step: rich = the pattern it ran with or None, dt)."""
    seen = set()
    ooo = 0       # on_off_on: 1 a step with the closure, 2 a step without, with a set-aside coefficient acting;  ooo_first: the first pattern
    ooo_first = None
    sto = {}      # setter_then_off_<setter>: 1 the setter accepted with a value that is on while the closure is on, 2 the closure switched off
    keys = {7: 0, 8: cs.PAIR_DEFAULT, 12: 1}       # the tuning keys as they stand (the library's defaults)
    tog = {}      # toggle_on_<key>: 1 a step with the closure, 2 the key changed behind it
    runs = None   # params_between_runs: the pattern of the last run of nine with the closure on
    last = None   # what the last step ran with
    dl = set()    # diag_levels: levels diagnosed (all outputs) behind the last step
    sto_set = False
    cur = None    # the closure as it stands (pattern)
    st_off = 0    # set_tracers_off: 1 set_tracers while on, 2 rich_diag refused, 3 rich on again
    tb = 0        # tape_blocks: 1 rich refused beside a tracer tape, 2 the tape destroyed
    have_kv = have_vf = False
    for op, o in zip(ops, obs):
        k, a, info = op.kind, op.args, getattr(o, "info", {})
        if o.rc != OK:
            if k == "rich_diag" and o.refusal == "rich_diag_off":
                st_off = 2 if st_off == 1 else st_off
            if k == "rich" and o.refusal == "rich_tracer_tape":
                tb = 1
            continue
        if k in F_STEPS:
            r, dt = info.get("rich"), info.get("dt")
            if r is not None and dt != 0.0:
                if ooo == 2 and r != ooo_first:            # on again with other parameters
                    seen.add("on_off_on")
                if ooo != 2:
                    ooo_first = r
                ooo = 1
                for key in (7, 8, 12):
                    if tog.get(key) == 2:
                        seen.add(f"toggle_on_{key}")
                    tog[key] = 1
                if info.get("drag"):
                    seen.add("drag_under_closure")
                if r == "mask_out" and have_kv and have_vf:
                    seen.add("mask_split")
                if r == "unit":
                    seen.add("unit_buoyancy")
            else:
                acts = info.get("acts", ()) if (r is None and dt != 0.0) else ()
                if ooo in (1, 2) and acts:
                    seen.update("acts_again_" + x for x in acts)
                ooo = 2 if (ooo in (1, 2) and acts) else 0
                tog = {}
            for x in list(sto):
                if sto[x] == 2:
                    if r is None and dt != 0.0 and x in info.get("acts", ()):      # the step used the value set under the closure
                        seen.add("setter_then_off_" + x)
                    del sto[x]
            nine = k == "run" and a[1] == 9 and r is not None and dt != 0.0
            if nine and runs is not None and runs != r:
                seen.add("params_between_runs")
            runs = r if nine else None
            last, dl = (r, dt), set()
        elif k == "rich":
            if a[0] == "off":
                sto = {x: 2 for x in sto}
            else:
                sto = {x: v for x, v in sto.items() if v == 1}
                if st_off == 2:
                    seen.add("set_tracers_off")
                if tb == 2:
                    seen.add("tape_blocks")
            st_off, tb = 0, 0
            cur = None if a[0] == "off" else a[0]
        elif k in F_SETTERS and cur is not None:
            if (a[1] if k == "vfield" else a[0]) in ("some", "other", "A", "nu", "both"):
                sto[k] = 1
            else:
                sto.pop(k, None)
        elif k == "set_tracers":
            st_off = 1 if cur is not None else st_off
            cur, have_kv, have_vf, runs, sto = None, False, False, None, {}
        elif k == "tr_tape_destroy":
            tb = 2 if tb == 1 else 0
        elif k == "tuning":
            if a[1] != keys[a[0]] and tog.get(a[0]) in (1, 2):
                tog[a[0]] = 2
            keys[a[0]] = a[1]
        elif k == "rich_fields" and last is not None:
            if last[0] is None and not np.any(o.value):
                seen.add("fields_zero_without")
            if last[0] is not None and last[1] == 0.0 and not np.any(o.value):
                seen.add("fields_dt0")
        elif k == "rich_diag" and a[1] == "all" and last is not None:
            dl.add((a[0], zlib.crc32(np.ascontiguousarray(o.value).tobytes())))
            if {l for l, _ in dl} == {0, 1} and len({c for _, c in dl}) > 1:
                seen.add("diag_levels")
        if k == "kappaV":
            have_kv = a[0] != "none"
        if k == "vfield":
            have_vf = a[1] == "A" or (have_vf and a[1] != "none")
    return seen


def f_sequence(cfg, seed):
    """About cfg.nops ops, a pure function of (cfg, seed): the tracers set up (the unit tracer, the buoyancy in both levels, a third), then
    scenes that aim at one named order or refusal each, between single ops and reads."""
    rng = np.random.default_rng([zlib_crc(cfg.name), seed])
    ops = []
    vs = [0]
    ab = dict(nT=0, rich=None, tape=False, dirty=[], variant=0)

    def draw(items, weights=None):
        if weights is None:
            return items[int(rng.integers(len(items)))]
        w = np.asarray(weights, dtype=np.float64)
        return items[int(rng.choice(len(items), p=w / w.sum()))]

    def vseed():
        vs[0] += 1
        return 32452843 * (seed + 1) + vs[0]

    def touch(keys):
        for key in keys:
            if key in ab["dirty"]:
                ab["dirty"].remove(key)
            ab["dirty"].append(key)

    def accept(op):
        k, a = op.kind, op.args
        if k == "set_tracers":
            if not ab["tape"] or a[0] == 0:
                ab["nT"], ab["rich"] = a[0], None
                ab["dirty"] = [x for x in ab["dirty"] if x[0] != "tr"]
        elif k in ("tr_upload", "tr_buoy"):
            touch([("tr", a[0], a[1])])
        elif k == "rich":
            if a[0] == "off":
                ab["rich"] = None
            elif a[0] in RICH_ON and not ab["tape"] and ab["nT"] > 0:
                ab["rich"] = a[0]
        elif k in F_STEPS:
            f = a[0] if k == "rk4" else a[3]
            if k == "run" and a[0] == 0:
                return
            if f < 0:
                return
            lv = (1,) if f == 0.0 else (0, 1)
            touch([("tr", j, 0) for j in range(ab["nT"])] + [(x, 0) for x in PROG])
            if f != 0.0:
                touch([("tr", j, 1) for j in range(ab["nT"])] + [(x, 1) for x in PROG])
            touch([(x, 1) for x in TEND])
        elif k == "upload":
            touch([(a[0], a[1])])
        elif k == "tr_download":
            if ("tr", a[0], a[1]) in ab["dirty"]:
                ab["dirty"].remove(("tr", a[0], a[1]))
        elif k in READ_KINDS:
            if (a[0], a[1]) in ab["dirty"]:
                ab["dirty"].remove((a[0], a[1]))
        elif k == "tr_tape_create":
            if ab["rich"] is None:
                ab["tape"] = True
        elif k == "tr_tape_destroy":
            ab["tape"] = False
        elif k == "variant":
            ab["variant"] = a[0]

    def a_read(tracer=None):
        cand = [x for x in ab["dirty"] if tracer is None or (x[0] == "tr") == tracer]
        if not cand:
            return None
        w = [2.0 ** min(i - len(cand), 0) for i in range(1, len(cand) + 1)]
        key = draw(cand, w)
        if key[0] == "tr":
            return Op("tr_download", (key[1], key[2]))
        kind = draw(READ_KINDS)
        if kind == "rows":
            n = shape_of(cfg, key[0])[0]
            return Op("rows", (key[0], key[1], tuple(int(r) for r in rng.integers(0, n, int(rng.integers(1, 4))))))
        return Op(kind, key)

    def a_step():
        name = draw(("rk4", "run3", "run9"), (4, 1.5, 0.7))
        return Op("rk4", (1.0,)) if name == "rk4" else Op("run", (1, 3 if name == "run3" else 9, 0, 1.0))

    def setup(n):
        yield Op("set_tracers", (n,))
        yield Op("tr_upload", (0, 1, "unit", 0))
        yield Op("tr_buoy", (1, 1))
        yield Op("tr_buoy", (1, 0))
        for j in range(2, n):
            yield Op("tr_upload", (j, 1, "phi", vseed()))

    def ensure_tracers():
        if ab["nT"] < 2:
            yield from setup(cfg.nT)

    def ensure_no_tape():
        if ab["tape"]:
            yield Op("tr_tape_destroy")

    def ensure_rich(pats=RICH_ON[:3]):
        yield from ensure_no_tape()
        yield from ensure_tracers()
        if ab["rich"] is None:
            yield Op("rich", (draw(pats),))

    def a_setter():
        j = int(rng.integers(ab["nT"]))
        return draw((Op("kappaV", (draw(cv.KV_PATTERNS[1:]),)), Op("vfield", (j, draw(("zero", "A")))), Op("visc", (draw(("nu", "both")),)),
                     Op("field", (draw(("zero", "A")),))))

    def scene_on_off_on():
        yield from ensure_rich()
        first = ab["rich"]
        yield a_setter()
        yield a_step()
        yield a_read(True)
        yield Op("rich", ("off",))
        yield a_step()
        yield a_read(True)
        yield a_read(False)
        yield Op("rich", (draw([p for p in RICH_ON[:4] if p != first]),))
        yield a_step()
        yield a_read(True)
        yield a_read(False)

    def scene_runs():
        yield from ensure_rich()
        yield Op("run", (1, 9, 0, 1.0))
        yield Op("rich", (draw([p for p in RICH_ON[:3] if p != ab["rich"]]),))
        yield Op("rich_read")
        yield Op("run", (1, 9, 0, 1.0))
        yield a_read(True)
        yield a_read(False)

    def scene_fields():
        yield from ensure_rich()
        yield a_step()
        yield Op("rich_fields", (draw(("both", "F", "G")),))
        if rng.random() < 0.5:
            yield Op("rk4", (0.0,))
            yield Op("rich_fields", ("both",))
            yield a_read()
        yield Op("rich", ("off",))
        yield Op("rk4", (1.0,))
        yield Op("rich_fields", (draw(("both", "F", "G")),))
        yield a_read(True)

    def scene_diag():
        yield from ensure_rich()
        yield a_step()
        for l in rng.permutation(2):
            yield Op("rich_diag", (int(l), "all"))
        yield draw((Op("rich_diag", (1, "F")), Op("rich_diag", (2, "all")), Op("rich_diag", (-1, "F"))))
        yield a_read()

    def scene_set_tracers():
        yield from ensure_rich()
        n = draw((0, 2, cfg.nT))
        yield Op("set_tracers", (n,))
        yield Op("rich_diag", (1, "all"))                  # refused: the closure went with the tracers
        if n == 0:
            yield Op("rich", ("P0",))                      # refused: no tracers
            yield a_read(False)
        yield from setup(cfg.nT if n != cfg.nT or rng.random() < 0.5 else 2)
        yield Op("rich", (draw(RICH_ON[:3]),))
        yield a_step()
        yield a_read(True)

    def scene_mask():
        yield from ensure_no_tape()
        yield from ensure_tracers()
        if ab["nT"] < 3:
            yield from setup(cfg.nT)
        if ab["nT"] >= 3:
            yield Op("kappaV", (draw(cv.KV_PATTERNS[1:]),))
            yield Op("vfield", (2, "A"))
        yield Op("rich", ("mask_out",))
        yield Op("rich_read")
        yield a_step()
        for j in rng.permutation(min(ab["nT"], 3)):
            yield Op("tr_download", (int(j), 1))

    def scene_unit():
        yield from ensure_no_tape()
        yield from ensure_tracers()
        yield Op("tr_upload", (0, 1, "unit", 0))
        yield Op("rich", ("unit",))
        yield a_step()
        yield Op("rich_fields", ("both",))
        yield a_read(True)
        yield a_read(False)

    def scene_tape():
        yield from ensure_tracers()
        if ab["rich"] is not None:
            yield Op("tr_tape_create", (2, (), ()))        # refused: the closure is on
            yield Op("rich", ("off",))
        if not ab["tape"]:
            yield Op("tr_tape_create", (2, (), ()))
        yield Op("rich", (draw(RICH_ON[:3]),))             # refused: a tracer tape exists
        yield a_read() or Op("tr_download", (0, 1))
        yield Op("tr_tape_destroy")
        yield Op("rich", (draw(RICH_ON[:3]),))
        yield a_step()
        yield a_read(True)

    def scene_toggle():
        yield from ensure_rich()
        yield Op("rk4", (1.0,))
        yield a_read()
        key = draw((7, 8, 12))
        yield a_key(key)
        yield Op("rk4", (1.0,))
        yield a_read(True)
        yield a_key(draw((7, 8, 12)))
        yield Op("variant", (draw([v for v in cfg.variants if v != ab["variant"]]),)) if len(cfg.variants) > 1 else None
        yield a_step()
        yield a_read(False)

    def a_key(key):
        """The key set to the value it does not have."""
        cur = ab.setdefault("keys", {7: 0, 8: cs.PAIR_DEFAULT, 12: 1})
        v = (0 if cur[8] else cs.PAIR_DEFAULT) if key == 8 else 1 - cur[key]
        cur[key] = v
        return Op("tuning", (key, v))

    def scene_drag():
        yield from ensure_rich()
        yield draw((Op("visc", (draw(("drag", "both")),)), Op("cd", ("cd",)), Op("stress", ("field",))))
        yield a_step()
        yield a_read(False)
        yield a_read(True)
        yield draw((Op("visc", ("zero",)), Op("cd", ("zero",)), Op("stress", ("none",))))

    def scene_refusals():
        yield from ensure_rich()
        c = [Op("fe", (0,)), Op("run", (0, 3, 0, 1.0)), Op("rk4", (-1.0,)), Op("run", (1, 3, 0, -1.0)), Op("tape_create", (2,)), Op("ft_create", (2,)),
             Op("ftq_create", (2,)), Op("tr_tape_create", (2, (), ())), Op("rich", (draw(RICH_BAD),)), Op("rich", (draw(RICH_BAD),)), Op("rich_read_null", (draw(("on", "out")),)),
             Op("rich_read_null", (draw(("on", "out")),))]
        for i in rng.permutation(len(c))[:3]:
            yield c[int(i)]
        yield a_read() or Op("tr_download", (1, 1))

    def a_single():
        if ab["nT"] < 2:
            return Op("set_tracers", (cfg.nT,))
        name = draw(("step", "setter", "getter", "upload", "tr_upload", "coef"), (4, 3, 3, 2, 2, 2))
        j = int(rng.integers(ab["nT"]))
        if name == "step":
            return a_step() if rng.random() < 0.85 else Op("rk4", (0.0,))
        if name == "setter":
            return a_setter()
        if name == "getter":
            return draw((Op("rich_read"), Op("rich_fields", (draw(("both", "F", "G")),)), Op("kappaV_read", (j,)), Op("has_vfield", (j,)), Op("visc_read"),
                         Op("has_field"), Op("cd_read")))
        if name == "upload":
            return Op("upload", (draw(PROG), int(rng.integers(2)), vseed()))
        if name == "tr_upload":
            return Op("tr_upload", (j, int(rng.integers(2)), "phi", vseed())) if j != 1 else Op("tr_buoy", (1, int(rng.integers(2))))
        return draw((Op("kappaV", ("none",)), Op("vfield", (j, "none")), Op("visc", ("zero",)), Op("field", ("none",)), Op("cd", (draw(("zero", "cd")),)),
                     Op("stress", (draw(("none", "field")),))))

    scenes = [(scene_on_off_on, 4), (scene_runs, 2), (scene_fields, 3), (scene_diag, 3), (scene_set_tracers, 3), (scene_mask, 2.5), (scene_unit, 2),
              (scene_tape, 2.5), (scene_toggle, 3), (scene_drag, 2.5), (scene_refusals, 4)]
    scene = setup(cfg.nT)
    while len(ops) < cfg.nops:
        if scene is not None:
            try:
                op = next(scene)
            except StopIteration:
                scene = None
                continue
            if op is not None:
                ops.append(op)
                accept(op)
            continue
        r = rng.random()
        if ab["dirty"] and r < 0.25:
            op = a_read()
        elif r < 0.75:
            scene = draw([x[0] for x in scenes], [x[1] for x in scenes])()
            continue
        else:
            op = a_single()
        ops.append(op)
        accept(op)
    return ops[:cfg.nops]


class ClosureModel(cv.VTracerModel):
    """Machine F on the twin stack, eagerly, as include/moka_hip.h words each call.  mutant: one of F_MUTANTS."""

    def __init__(self, cfg, seed, mutant=None):
        from types import SimpleNamespace
        import richardson_twin as rt
        import tracer_vfield_twin as tf
        assert mutant is None or mutant in F_MUTANTS
        super().__init__(cfg, seed, mutant if mutant in cv.D_MUTANTS else None)
        self.mutant, self.rt = mutant, rt
        if cfg.depths != "full":
            self.mlt = mask_of(cfg)
            self.om = cv.orc.OracleMesh(self.mesh, cfg.K, resting_thickness_sum=resting_thickness(cfg).sum(1), max_level_edge_top=self.mlt)
            self.twin = tf.VfieldTwin(self.om, self.om, [])
            self.nlev = self.twin.nlev(cfg.K)
            self.mix = mv.MomentumVmixTwin(SimpleNamespace(om=self.om))
        self.fld, self.cd = None, 0.0
        self.rich, self.pattern = None, None       # richardson_twin.Params while the closure is on, and the pattern it came from
        self.FG = None                 # what moka_richardson_fields_download answers (None: zeros)
        self.lag_rich = None           # mutant rich_late
        self.census = None             # a list: richardson_twin.census of every step that launches the closure is appended (edge recipe)

    def vert_on(self):
        return self.rich is not None or super().vert_on()

    def mom_on(self):
        return mf.pass_on(self.mix.nu, self.mix.drag, self.mix.tau, self.mlt, self.fld) or self.cd != 0.0

    def _aside(self):
        kv, fv = self._vcoeffs()
        return self.mix.nu != 0.0 or self.fld is not None or any(k != 0.0 for k in kv) or any(f is not None for f in fv)

    def _step(self, dt, taped=False):
        st, tw, K, rt = self.st, self.twin, self.cfg.K, self.rt
        cur = self._coeffs() + self._vcoeffs()
        use = cur
        if self.mutant == "coeff_late":
            use = self.lag if self.lag is not None and len(self.lag[0]) == self.nT else cur
            self.lag = cur
        tw.kappa, tw.kappa4, tw.source, tw.kappaV, tw.fieldV = (list(x) for x in use)
        tw.base = self._base()
        P, pattern = self.rich, self.pattern
        if self.mutant == "rich_late":
            lag, self.lag_rich = self.lag_rich, (P, pattern)
            if lag is not None and (lag[0] is None or lag[0].buoyancy < self.nT):
                P, pattern = lag
        if self.mutant == "mask_ignored" and P is not None:
            P = rt.Params(P.buoyancy, P.nu0, P.alpha, P.nuB, P.kB, P.conv, None)
        drag, tau, cd = self.mix.drag, self.mix.tau, self.cd
        if self.mutant == "drag_set_aside" and P is not None:
            drag, tau, cd = 0.0, None, 0.0
        kept = [[a.copy() for a in (st.ssh[0], st.u[0], st.h[0])], [p.copy() for p in self.phis[0]]] if self.mutant == "prev_level_lost" else None
        phi0 = [p.copy() for p in self.phis[1]]
        r = rt.RichardsonTwin(tw, self.mix.nu, drag, tau, cd, self.fld, P)
        launched = P is not None and K >= 2 and dt != 0.0
        if launched and self.census is not None:           # the three branches the step is about to meet, from the twin alone
            tw.kappaV, tw.fieldV = [], []
            probe = [[p.copy() for p in lv] for lv in self.phis]
            ps = type(st)(st.ssh[1].copy(), st.u[1].copy(), st.h[1].copy())
            tw.step_rk4(ps, probe, dt)
            tw.tape.pop()
            tw.kappaV, tw.fieldV = list(use[3]), list(use[4])
            m = r.mq.mt
            live, _, db, _ = rt.edge_parts(ps.u[1], ps.h[1], probe[1][P.buoyancy], m.mlt, m.c1, m.c2)
            ri = rt.edge_field(ps.u[1], ps.h[1], probe[1][P.buoyancy], m.mlt, m.c1, m.c2, P)[1]
            self.census.append(rt.census(ri[:, :-1], db, live))
        r.step_rk4(st, self.phis, dt)
        rec = tw.tape.pop()
        self.pending = None
        if self.mutant == "mixed_flow_early" and dt != 0.0 and (P is not None or self.mom_on()):
            # the tracers' stage 4 reads the flow the momentum pass has already mixed: the transport replayed over it, then the vertical pass
            early = dict(rec, P=rec["P"][:3] + [(st.u[1].copy(), rec["P"][3][1])])
            kv, fv = use[3], use[4]
            for j in range(self.nT):
                new = tw.replay(early, j, phi0[j])[1]
                if K >= 2 and P is not None and P.in_set(j):
                    new = self.tf.apply_field(st.h[1], new, self.nlev, dt, r.G)
                elif K >= 2 and fv[j] is not None:
                    if self.tf.field_on(fv[j], self.nlev):
                        new = self.tf.apply_field(st.h[1], new, self.nlev, dt, fv[j])
                elif K >= 2 and kv[j] != 0.0:
                    new = self.tv.apply(st.h[1], new, self.nlev, np.float64(dt) * np.float64(kv[j]))
                self.phis[1][j] = new
        if launched:
            self.FG = r.fields(st.u[1], st.h[1], self.phis[1][P.buoyancy]) if self.mutant == "rich_from_mixed" else (r.F, r.G)
        elif self.mutant != "fields_stale":
            self.FG = None
        if kept is not None:
            st.ssh[0], st.u[0], st.h[0] = kept[0]
            if len(kept[1]) == self.nT:
                self.phis[0] = kept[1]
        self.ssh_loose = False
        kvs, fvs = self._vcoeffs()
        acts = [x for x, yes in (("visc", self.mix.nu != 0.0 and self.fld is None), ("field", self.fld is not None and mf.field_on(self.fld, self.mlt)),
                                 ("kappaV", any(kk != 0.0 and f is None for kk, f in zip(kvs, fvs))),
                                 ("vfield", any(f is not None and self.tf.field_on(f, self.nlev) for f in fvs))) if yes]
        self.last = dict(rich=pattern if P is not None else None, dt=dt, aside=self._aside(), acts=tuple(acts),
                         drag=self.mix.drag != 0.0 or self.cd != 0.0 or mv.stress_on(self.mix.tau, self.mlt))
        if taped:
            self.tape["rec"].append(rec)

    def apply(self, op):
        cfg, k, a, st = self.cfg, op.kind, op.args, self.st
        nT, K, rt = self.nT, cfg.K, self.rt
        nE, nC = self.mesh.nEdges, self.mesh.nCells
        R = lambda code, name: Obs(k, code, refusal=name)       # noqa: E731
        on = self.rich is not None
        if k in F_SETTERS and on and self.mutant == "setter_dropped":
            return Obs(k, OK)
        if k == "rich_read_null":
            return R(ERR_ARG, "rich_null")
        if k == "set_tracers":
            keep = self.rich if (self.mutant == "set_tracers_keeps" and on and self.rich.buoyancy < a[0]
                                 and (self.rich.tracers is None or max(self.rich.tracers) < a[0])) else None
            o = super().apply(op)
            if o.rc == OK:
                self.rich, self.FG = keep, None
                self.pattern = self.pattern if keep is not None else None
            return o
        if k == "tr_buoy":
            self.phis[a[1]][a[0]] = buoyancy_values(cfg, a[1])
            return Obs(k, OK)
        if k == "rich":
            if a[0] == "off":
                if on and self.mutant == "aside_lost":
                    self.kappaV, self.fieldV, self.fld = [], [], None
                    self.mix.nu = 0.0
                self.rich, self.pattern, self.FG = None, None, None
                return Obs(k, OK)
            P = rich_params(cfg, a[0], nT)
            if not all(v >= 0.0 and np.isfinite(v) for v in (P.nu0, P.alpha, P.nuB, P.kB, P.conv)):
                return R(ERR_ARG, "rich_invalid")
            if self.tape is not None:
                return R(ERR_UNSUPPORTED, "rich_tracer_tape")
            if nT == 0:
                return R(ERR_ARG, "rich_no_tracers")
            if not 0 <= P.buoyancy < nT:
                return R(ERR_ARG, "rich_range")
            if not on:
                self.FG = None
            self.rich, self.pattern = P, a[0]
            return Obs(k, OK)
        if k == "rich_read":
            P = self.rich
            if P is None:
                return Obs(k, OK, value=(0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, (0,) * nT))
            return Obs(k, OK, value=(1, P.buoyancy) + tuple(float(v) for v in (P.nu0, P.alpha, P.nuB, P.kB, P.conv)) +
                       (tuple(int(P.in_set(j)) for j in range(nT)),))
        if k == "rich_fields":
            F, G = self.FG if (self.FG is not None and (on or self.mutant == "fields_stale")) else (np.zeros((nE, K)), np.zeros((nC, K)))
            return Obs(k, OK, value=np.concatenate([x.ravel() for x, w in ((F, "F"), (G, "G")) if a[0] in ("both", w)]))
        if k == "rich_diag":
            if a[0] not in (0, 1):
                return R(ERR_ARG, "rich_diag_level")
            if not on:
                return R(ERR_UNSUPPORTED, "rich_diag_off")
            l = 1 if self.mutant == "levels_swapped" else a[0]
            m = self.mix
            b = self.phis[l][self.rich.buoyancy]
            F, riE = rt.edge_field(st.u[l], st.h[l], b, self.mlt, m.c1, m.c2, self.rich)
            if a[1] == "F":
                return Obs(k, OK, value=F)
            G, riC = rt.cell_field(st.u[l], st.h[l], b, self.mlt, self.mesh, self.rich)
            return Obs(k, OK, value=np.concatenate([x.ravel() for x in (riE, riC, F, G)]))
        if k == "field":
            f = field_values(cfg, a[0])
            if f is not None and not mf.check_field(f, self.mlt):
                return R(ERR_ARG, "field_invalid")
            self.fld = f
            return Obs(k, OK)
        if k == "has_field":
            return Obs(k, OK, value=int(self.fld is not None))
        if k == "cd":
            self.cd = cd_values(cfg, a[0])
            return Obs(k, OK)
        if k == "cd_read":
            return Obs(k, OK, value=self.cd)
        if k == "tuning":
            return Obs(k, OK)
        if on and k in ("tr_tape_create", "tape_create", "ft_create", "ftq_create", "fe") or (on and k == "run" and a[0] == 0):
            return R(ERR_UNSUPPORTED, {"tr_tape_create": "tr_tape_rich", "tape_create": "tape_rich", "ft_create": "ft_rich", "ftq_create": "ftq_rich",
                                       "fe": "fe_rich", "run": "run_fe_rich"}[k])
        if k in ("ft_create", "ftq_create"):
            return R(ERR_UNSUPPORTED, "ft_tracers")
        o = super().apply(op)
        if k in F_STEPS and o.rc == OK:
            o.info = dict(self.last)
        return o

    def run(self, ops):
        out = []
        before = {key: self.array(key).copy() for key in self.keys()}
        self._last = dict(before)
        for op in ops:
            o = self.apply(op)
            if op.kind in F_READS:
                if o.rc == OK:
                    o.fresh = o.key not in self._last or not np.array_equal(self._last[o.key], self.array(o.key))
                    o.after = frozenset(self._changed.get(o.key, ()))
                    self._changed[o.key] = set()
                    self._last[o.key] = self.array(o.key).copy()
            elif op.kind not in F_GETTERS:
                now = {key: self.array(key).copy() for key in self.keys()}
                for key, v in now.items():
                    if key not in before or not np.array_equal(before[key], v) or \
                            (o.rc == OK and op.kind in F_NON_ARRAY and self._changed.get(key)):
                        self._changed.setdefault(key, set()).add(op.kind)
                before = now
            out.append(o)
        return out


class ClosureDevice:
    """Machine F through moka_hip.lib, in the form of call_sequences_vertical.VTracerDevice: one mesh per config, a fresh state per
    sequence.  A HIP error ends the sequence and every later one of the config (`dead`)."""

    def __init__(self, backend, cfg):
        import moka_hip as mk
        from moka_hip import lib as L
        self.L, self.lib, self.backend, self.cfg = L, L.lib(), backend, cfg
        hm = mk.HorzMesh(get_mesh(cfg.meshname))
        vm = mk.VerticalMesh(hm, nVertLevels=cfg.K, restingThickness=resting_thickness(cfg), multilayer=True)
        mlt = mask_of(cfg)
        if mlt is not None:
            vm.maxLevelEdge.Top[:] = mlt
        self.M = mk.Mesh(hm, vm, backend=backend, patch_cells=cfg.patch_cells)
        self.counters = {"sequences": 0, "rk4_steps": 0, "closure_steps": 0, "run9_closure": 0, "vpaths": set(), "paths": set(), "streams": set(),
                         "handoff": 0, "no_handoff": 0, "key7_closure_steps": 0}
        self.dead = None

    def close(self):
        self.M.close()

    def run(self, ops, seed):
        if self.dead:
            raise RuntimeError("an earlier sequence of this config ended in a HIP error, nothing more is launched: " + self.dead)
        L, lib, cfg, ctx = self.L, self.lib, self.cfg, self.backend._h
        cnt = self.counters
        hS, hT = C.c_void_p(), C.c_void_p()
        out, nT, rich = [], 0, False
        saved = {}
        key7 = [0]
        nE, nC, K = get_mesh(cfg.meshname).nEdges, get_mesh(cfg.meshname).nCells, cfg.K
        vp = lambda arr: arr.ctypes.data_as(C.c_void_p)        # noqa: E731
        hfield = lambda: np.full(shape_of(cfg, F_H), np.nan)   # noqa: E731

        def tune(key, value):
            if key not in saved:
                v = C.c_int()
                L.check(lib.moka_get_tuning(key, C.byref(v)))
                saved[key] = v.value
            return lib.moka_set_tuning(key, value)

        try:
            L.check(lib.moka_state_create(ctx, self.M._h, C.byref(hS)), ctx)
            for (f, l), arr in initial_state(cfg, seed).items():
                L.check(lib.moka_state_upload(hS, f, l, L.f64(arr)), ctx)
            for op in ops:
                k, a = op.kind, op.args
                value = None
                if k == "set_tracers":
                    rc = lib.moka_set_tracers(hS, a[0])
                    if rc == OK:
                        nT, rich = a[0], False
                elif k == "tr_upload":
                    rc = lib.moka_tracer_upload(hS, a[0], a[1], vp(cs.tracer_values(cfg, a[2], a[3])))
                elif k == "tr_buoy":
                    rc = lib.moka_tracer_upload(hS, a[0], a[1], vp(buoyancy_values(cfg, a[1])))
                elif k == "tr_download":
                    value = hfield()
                    rc = lib.moka_tracer_download(hS, a[0], a[1], vp(value))
                elif k == "kappaV":
                    v = cv.kappav_values(cfg, a[0], nT)
                    rc = lib.moka_set_tracer_vertical_diffusion(hS, None if v is None else vp(np.asarray(v, dtype=np.float64)))
                elif k == "vfield":
                    f = cv.vfield_values(cfg, a[1], a[0])
                    rc = lib.moka_tracer_vertical_field_upload(hS, a[0], None if f is None else vp(f))
                elif k == "has_vfield":
                    v = C.c_int(-1)
                    rc = lib.moka_tracer_has_vertical_field(hS, a[0], C.byref(v))
                    value = v.value
                elif k == "kappaV_read":
                    s = C.c_double(np.nan)
                    rc = lib.moka_tracer_vertical_diffusion(hS, a[0], C.byref(s))
                    value = s.value
                elif k == "visc":
                    rc = lib.moka_set_vertical_viscosity(hS, *visc_values(cfg, a[0]))
                elif k == "visc_read":
                    nu, r = C.c_double(np.nan), C.c_double(np.nan)
                    rc = lib.moka_vertical_viscosity(hS, C.byref(nu), C.byref(r))
                    value = (nu.value, r.value)
                elif k == "field":
                    f = field_values(cfg, a[0])
                    rc = lib.moka_vertical_viscosity_field_upload(hS, None if f is None else vp(f))
                elif k == "has_field":
                    v = C.c_int(-1)
                    rc = lib.moka_has_vertical_viscosity_field(hS, C.byref(v))
                    value = v.value
                elif k == "cd":
                    rc = lib.moka_set_quadratic_bottom_drag(hS, cd_values(cfg, a[0]))
                elif k == "cd_read":
                    v = C.c_double(np.nan)
                    rc = lib.moka_quadratic_bottom_drag(hS, C.byref(v))
                    value = v.value
                elif k == "stress":
                    tau = stress_values(cfg, a[0])
                    rc = lib.moka_surface_stress_upload(hS, None if tau is None else vp(tau))
                elif k == "rich":
                    if a[0] == "off":
                        rc = lib.moka_set_richardson_mixing(hS, None)
                    else:
                        P = rich_params(cfg, a[0], nT)
                        mask = None if P.tracers is None else np.asarray([int(P.in_set(j)) for j in range(max(nT, 1))], dtype=np.int32)
                        rp = L.RichardsonParams(P.buoyancy, float(P.nu0), float(P.alpha), float(P.nuB), float(P.kB), float(P.conv),
                                                None if mask is None else mask.ctypes.data)
                        rc = lib.moka_set_richardson_mixing(hS, C.byref(rp))
                    if rc == OK:
                        rich = a[0] != "off"
                elif k == "rich_read":
                    on, rp = C.c_int(-1), L.RichardsonParams()
                    mask = np.full(max(nT, 1), -1, dtype=np.int32)
                    rc = lib.moka_richardson_mixing(hS, C.byref(on), C.byref(rp), vp(mask))
                    n32 = C.c_int32(-1)
                    L.check(lib.moka_tracer_count(hS, C.byref(n32)))
                    value = (on.value, rp.buoyancyTracer, rp.nu0, rp.alpha, rp.nuBackground, rp.kappaBackground, rp.convective,
                             tuple(int(x) for x in mask[:n32.value]))
                elif k == "rich_read_null":
                    on, rp = C.c_int(-1), L.RichardsonParams()
                    rc = lib.moka_richardson_mixing(hS, None if a[0] == "on" else C.byref(on), None if a[0] == "out" else C.byref(rp), None)
                elif k == "rich_fields":
                    F, G = np.full((nE, K), np.nan), np.full((nC, K), np.nan)
                    rc = lib.moka_richardson_fields_download(hS, vp(F) if a[0] in ("both", "F") else None, vp(G) if a[0] in ("both", "G") else None)
                    value = np.concatenate([x.ravel() for x, w in ((F, "F"), (G, "G")) if a[0] in ("both", w)])
                elif k == "rich_diag":
                    riE, riC, F, G = (np.full(s, np.nan) for s in ((nE, K), (nC, K), (nE, K), (nC, K)))
                    if a[1] == "F":
                        rc = lib.moka_richardson_diagnose(hS, a[0], None, None, vp(F), None)
                        value = F
                    else:
                        rc = lib.moka_richardson_diagnose(hS, a[0], vp(riE), vp(riC), vp(F), vp(G))
                        value = np.concatenate([x.ravel() for x in (riE, riC, F, G)])
                elif k == "variant":
                    rc = lib.moka_set_kernel_variant(ctx, a[0])
                elif k == "tuning":
                    rc = tune(a[0], a[1])
                    if rc == OK and a[0] == 7:
                        key7[0] = a[1]
                elif k == "rk4":
                    value = lib.moka_state_rk4_streams(hS)
                    rc = lib.moka_step_rk4(hS, dt_of(cfg, a[0]))
                elif k == "run":
                    rc = lib.moka_run(hS, a[0], dt_of(cfg, a[3]), a[1], a[2])
                elif k == "fe":
                    rc = lib.moka_step_fe(hS, cfg.dt, a[0])
                elif k == "upload":
                    rc = lib.moka_state_upload(hS, a[0], a[1], L.f64(values(cfg, a[0], a[2])))
                elif k == "download":
                    value = np.full(shape_of(cfg, a[0]), np.nan)
                    rc = lib.moka_state_download(hS, a[0], a[1], L.f64(value))
                elif k == "rows":
                    rows = np.asarray(a[2], dtype=np.int32)
                    value = np.full((rows.size, 1 if a[0] == F_SSH else cfg.K), np.nan)
                    rc = lib.moka_state_download_rows(hS, a[0], a[1], rows.size, L.i32(rows), L.f64(value))
                elif k == "sumsq":
                    s = C.c_double(np.nan)
                    rc = lib.moka_sum_sq(hS, a[0], a[1], C.byref(s))
                    value = s.value
                elif k == "tr_tape_create":
                    h = C.c_void_p()
                    rc = lib.moka_tracer_tape_create(hS, a[0], C.byref(h))
                    if rc == OK:
                        hT = h
                elif k == "tr_tape_destroy":
                    lib.moka_tracer_tape_destroy(hT)
                    hT, rc = C.c_void_p(), OK
                elif k in ("tape_create", "ft_create", "ftq_create"):
                    h = C.c_void_p()
                    rc = {"tape_create": lib.moka_tape_create, "ft_create": lib.moka_forced_tape_create,
                          "ftq_create": lib.moka_forced_tape_create_quadratic}[k](hS, a[0], C.byref(h))
                    if rc == OK:
                        raise RuntimeError(f"{op}: a state with tracers was given a dycore tape")
                else:
                    raise ValueError(f"unknown op {op}")
                if rc == ERR_HIP:
                    self.dead = f"config {cfg.name} seed {seed}: HIP error at op {len(out)} ({op}): {lib.moka_last_error(ctx)}"
                    raise RuntimeError(self.dead)
                if rc == OK and k in F_STEPS:
                    n = a[1] if k == "run" else 1
                    f = a[0] if k == "rk4" else a[3]
                    cnt["rk4_steps"] += n
                    if rich and f != 0.0:
                        cnt["closure_steps"] += n
                        cnt["run9_closure"] += n == 9
                        cnt["vpaths"].add(lib.moka_state_tracer_vmix_path(hS))
                        cnt["paths"].add(lib.moka_state_momentum_vmix_path(hS))
                        cnt["streams"].add(lib.moka_state_rk4_streams(hS))
                        cnt["key7_closure_steps"] += n * (saved.get(7) is not None and key7[0] == 1)
                        if k == "rk4":     # a single step with the closure on: did it hand New over as codes?
                            nc, ne = C.c_int64(), C.c_int64()
                            took = lib.moka_state_rk_handoff_escapes(hS, C.byref(nc), C.byref(ne))
                            if took not in (OK, ERR_UNSUPPORTED):
                                rc = took
                            cnt["handoff" if took == OK else "no_handoff"] += 1
                out.append(Obs(k, int(rc), value=value if rc == OK else None))
            cnt["sequences"] += 1
        finally:
            if not self.dead:
                if hT:
                    lib.moka_tracer_tape_destroy(hT)
                if hS:
                    lib.moka_state_destroy(hS)
            lib.moka_set_kernel_variant(ctx, 0)
            for key, v in saved.items():
                lib.moka_set_tuning(key, v)
        return out


# ---------------------------------------------------------------------------------------------------------------------------------
# triage on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def describe(o):
    if o.rc == OK and o.key is None and isinstance(o.value, np.ndarray):
        return f"shape {o.value.shape} crc32 {zlib.crc32(np.ascontiguousarray(o.value).tobytes()):08x}"
    return cs.describe(o)


def main(argv):
    if len(argv) < 2 or argv[0] not in ALL_CONFIGS:
        print(f"usage: call_sequences_mixing.py CONFIG SEED [--upto N]   (CONFIG: {' '.join(ALL_CONFIGS)})")
        return 2
    cfg, seed = ALL_CONFIGS[argv[0]], int(argv[1])
    ops = sequence_of(cfg, seed)
    if "--upto" in argv:
        ops = ops[:int(argv[argv.index("--upto") + 1]) + 1]
    for i, (op, o) in enumerate(zip(ops, model_of(cfg, seed).run(ops))):
        print(f"{i:2d} {str(op):44s} -> {describe(o)}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
