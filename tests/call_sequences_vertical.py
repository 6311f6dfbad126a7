"""Seeded call sequences through the C ABI for the vertical passes and the forced tape: machines C and D of tests/call_sequences.py's scheme.

Machine C, the forced dycore (configs C1-C4): moka_set_vertical_viscosity, moka_surface_stress_upload and their getters, RK4 in both
forms and moka_run (three steps eagerly, nine through the captured graph in its 2- and its 6-step period) with the pass on and off,
Forward Euler behind a mixed step, the nonlinear / Del2 / Del4 toggles, kernel variants (the pass and its transpose move between the
tile and the column form inside one history), tuning key 8 (and 7 around single RK4 steps), placement, uploads, the three kinds of
reads of every Prog / Diag / Tend array, moka_tape (which refuses the pass and which the pass setters refuse) and moka_forced_tape
with its seeds, sweep, densities and scalar gradients.  The model is call_sequences.Model with the pass of
momentum_vmix_twin.MomentumVmixTwin behind every RK4 step and forced_adjoint_twin's transposed pass in front of every reversed one;
every observation is compared bit for bit, a refusal is an observation.

What the header words and the model therefore does (include/moka_hip.h, moka_set_vertical_viscosity and moka_forced_tape):
values take effect with the next RK4 step or moka_run; the stage-4 tendencies are those of the provisional state, the diagnostics of
the new level come from the mixed u; "the pass is on" is nuV != 0, r != 0 or a stress with a nonzero entry at an edge with n >= 1, a
present all-zero stress answers moka_has_surface_stress with 1 and keeps the pass off; dt == 0.0 skips the pass, dt < 0 with the pass
on is MOKA_ERR_ARG.

Mutants (C_MUTANTS), each the bug one rule exists to prevent: values_late (a step runs with the scalars and the stress of the step
before: a stale captured graph or a cached argument block), diag_unmixed (new-level diagnostics from u*), tend_mixed (the stage-4
tendencies from the new level), stress_sticky (a removed or zeroed stress stays in force), n1_always (columns with n == 1 computed
with only nuV on), late and prev_level_lost as in machine A.
n1_always in the FORWARD pass cannot be told from the true model: for n == 1 with neither drag nor stress the recipe gives
R[0] = 0.0, y[0] = 0.0 / d[0] = 0.0 and u_new = x + 0.0, which has the bits of x for every x but -0.0 (no state here holds one).
The mutant is therefore placed where the bits do differ, in the transposed pass: a computed n == 1 column replaces XU[0] by
h[0] * (XU[0] / h[0]), two roundings away from XU[0].  Only C2 (edges with n == 1) and C4 (K = 1) can express it.

Machine D, tracers with the vertical passes (configs D1, D2): moka_set_tracer_vertical_diffusion and the per-tracer fields of
moka_tracer_vertical_field_upload with their getters, beside moka_set_tracers with a changing count (which resets every kappaV,
frees every field and puts moka_state_tracer_vmix_path back to 0: the header says so, the model does so; D2 seed 148 op 26 is the
sequence that made the header say the last), the horizontal diffusivity, the momentum pass of machine C (tracers see
the mixed flow from the next step on), RK4, moka_run and taped steps each with dt and with 0.0, dt < 0 refused while a vertical
coefficient is on, kernel variants (D2: the tracers' vertical pass in the tile and in the column form), and the tracer tape with
moka_tracer_adjoint_want_vertical_gradient on and off, kappaV and fields changing between taped steps, X, the three views of D and
the scalar gradient behind a sweep.  The model is call_sequences.TracerModel over tracer_vfield_twin.VfieldTwin /
VfieldAdjointTwin.  Mutants (D_MUTANTS): coeff_late extended to kappaV and the fields, mixed_flow_early (the tracers' stage 4 sees
the mixed flow of the same step), prev_level_lost.  Machine B's biharmonic coefficients, sources, Del2 / Del4, placement and
advanceTimeLevels! are not repeated here; a tracer count that changes under a live tracer tape, halos and partitions stay uncovered.

Replay a sequence on the CPU:   python tests/call_sequences_vertical.py C2 3 [--upto N]

This module imports no GPU code when it is imported (moka_hip.lib is loaded by the device runners only)."""
import ctypes as C
import os
import sys
import zlib
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import call_sequences as cs  # noqa: E402
from call_sequences import (DIAG, ERR_ARG, ERR_UNSUPPORTED, F_H, F_SSH, F_U, OK, PROG, READ_KINDS, STATE_KEYS, TEND, Obs, Op,  # noqa: E402
                            first_mismatch, get_mesh, initial_state, resting_thickness, shape_of, values, zlib_crc)
import forced_adjoint_twin as fa  # noqa: E402
import momentum_vmix_twin as mv  # noqa: E402
import oracle as orc  # noqa: E402
from masks import basin  # noqa: E402
from tracer_vgrad_twin import tile_columns_grad  # noqa: E402

ERR_HIP = -2
C_MUTANTS = ("values_late", "diag_unmixed", "tend_mixed", "stress_sticky", "n1_always", "late", "prev_level_lost")
VISC_OK = ("zero", "nu", "drag", "both", "other")
VISC_BAD = ("neg", "nan")
STRESS_OK = ("none", "zero", "field", "other", "n0")
GRAD_BITS = (fa.STRESS, fa.VISCOSITY, fa.DRAG)
STEP_KINDS = ("fe", "rk4", "rk4_s13", "run", "run_s13", "rk4_taped", "ft_taped")
FT_READS = ("ft_download", "ft_density", "ft_gradient")
GETTERS = ("visc_read", "stress_download", "has_stress", "vmix_path", "ft_path")
# ops that change no array of the state but may fall between a change of one and its first read
NON_ARRAY_OPS = cs.NON_ARRAY_OPS + ("visc", "stress", "ft_create", "ft_want", "ft_seed_ssh", "ft_seed_free", "ft_sweep", "ft_destroy")


# ---------------------------------------------------------------------------------------------------------------------------------
# configs
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class VConfig(cs.Config):
    variants: tuple = (0, 3, 4, 11)
    depths: str = "full"           # "full": every edge has n == K;  "shelf": n == 0, n == 1 and n > 1 side by side

    machine = "C"


V_CONFIGS = {c.name: c for c in (
    # forward tile form (path 1), reverse tiles of 32 columns, the 13-stream form under key 7
    VConfig("C1", "ico4", 34, s13=True, nops=36, reach=("path_1", "s13", "s13_run9", "ft_path_1")),
    # the only config where the differing column rules show: n == 1 is skipped with only nuV on, computed with drag or stress
    VConfig("C2", "hex6x4", 60, dt=2.0, s13=True, depths="shelf", nops=36, reach=("path_1", "s13_run9", "ft_path_1")),
    # reverse tiles of 64 columns; the variant toggles between 0 and 3: tile and column form, forwards and backwards
    VConfig("C3", "ico4f", 5, variants=(0, 3), nops=36, reach=("path_1", "path_2", "ft_path_1", "ft_path_2")),
    # K = 1: the column form; with only nuV on no launch at all, with drag or stress every column
    VConfig("C4", "hex4x4", 1, dt=2.0, nops=36, reach=("path_2", "ft_path_2")),
)}


def mask_of(cfg):
    """maxLevelEdgeTop of a config, None for full columns.  "shelf": masks.basin, whose shallowest wet band on this mesh is 3 levels
    deep, with that band made one level deep: land (0), n == 1, and every depth up to K."""
    if cfg.depths == "full":
        return None
    mlt = basin(get_mesh(cfg.meshname), cfg.K).copy()
    mlt[mlt == mlt[mlt > 0].min()] = 1
    return mlt


def depths_of(cfg):
    mlt = mask_of(cfg)
    return np.full(get_mesh(cfg.meshname).nEdges, cfg.K, dtype=np.int32) if mlt is None else mlt


def visc_values(cfg, pattern):
    """(nuV, r) of a visc op, scaled by momentum_vmix_twin.coefficients (dt nuV / hm^2 = 4, dt r / hm = 1/2)."""
    nu, r = mv.coefficients(cfg.meshname, cfg.K)
    return {"zero": (0.0, 0.0), "nu": (nu, 0.0), "drag": (0.0, r), "both": (nu, r), "other": (0.5 * nu, 2.0 * r),
            "neg": (-nu, r), "nan": (float("nan"), 0.0)}[pattern]


def stress_values(cfg, pattern):
    """The nEdges doubles of a stress op: None (NULL), all zero, a field with every third edge exactly 0.0, another field, a field
    that is nonzero only on land ("n0": absent for "on", present for moka_has_surface_stress), a field with one NaN."""
    mesh = get_mesh(cfg.meshname)
    if pattern == "none":
        return None
    if pattern == "zero":
        return np.zeros(mesh.nEdges)
    if pattern == "other":
        return mv.stress_field(mesh, cfg.K, seed=32)
    tau = mv.stress_field(mesh, cfg.K, seed=31, zeros=True)
    if pattern == "n0":
        tau = np.where(depths_of(cfg) == 0, mv.stress_field(mesh, cfg.K, seed=33), 0.0)
    elif pattern == "nan":
        tau[mesh.nEdges // 2] = np.nan
    return np.ascontiguousarray(tau)


def free_seed(cfg, vseed):
    rng = np.random.default_rng([cfg.K, 555, vseed])
    return rng.uniform(-1, 1, shape_of(cfg, F_U)), rng.uniform(-1, 1, shape_of(cfg, F_H))


def dt_of(cfg, f):
    return cfg.dt * f


# ---------------------------------------------------------------------------------------------------------------------------------
# vocabulary
# ---------------------------------------------------------------------------------------------------------------------------------
def vocabulary(cfg):
    v = ["visc", "stress", "rk4", "run", "fe", "nonlinear", "del2", "del4", "variant", "tuning", "placement", "upload",
         "download", "rows", "sumsq", "visc_read", "stress_download", "has_stress", "vmix_path",
         "tape_create", "rk4_taped", "seed", "sweep", "adj_download", "tape_destroy",
         "ft_create", "ft_want", "ft_taped", "ft_seed_ssh", "ft_seed_free", "ft_sweep", "ft_download", "ft_density", "ft_gradient",
         "ft_path", "ft_destroy"]
    return tuple(v + (["rk4_s13", "run_s13"] if cfg.s13 else []))


def stress_patterns(cfg):
    return STRESS_OK if cfg.depths == "shelf" else STRESS_OK[:-1]


def arg_class(op):
    k, a = op.kind, op.args
    if k in ("visc", "stress", "variant", "placement", "ft_download", "ft_density", "ft_gradient", "ft_taped", "rk4", "rk4_s13", "nonlinear"):
        return (k, a[0])
    if k in READ_KINDS or k == "upload" or k == "tuning" or k == "ft_want":
        return (k, a[0], a[1])
    if k == "run":
        return (k, a[0], a[1])
    if k == "run_s13":
        return (k, a[0])
    return None


def arg_classes(cfg):
    """Every (kind, argument class) the config admits with status MOKA_OK."""
    c = [("visc", p) for p in VISC_OK] + [("stress", p) for p in stress_patterns(cfg)]
    c += [("rk4", f) for f in (1.0, 0.0)] + ([("rk4_s13", f) for f in (1.0, 0.0)] + [("run_s13", 9)] if cfg.s13 else [])
    c += [("run", 1, 3), ("run", 1, 9), ("run", 0, 3)] + [("variant", v) for v in cfg.variants]
    c += [("tuning", 8, v) for v in cs.TUNING_VALUES[8]] + [("placement", n) for n in (0, 1)] + [("nonlinear", n) for n in (0, 1)]
    c += [("upload", f, l) for f in PROG for l in (0, 1)] + [(r,) + k for r in READ_KINDS for k in STATE_KEYS]
    c += [("ft_want", b, on) for b in GRAD_BITS for on in (0, 1)] + [("ft_taped", f) for f in (1.0, 0.0)]
    c += [("ft_download", f) for f in (F_U, F_H)] + [(k, b) for k in ("ft_density", "ft_gradient") for b in GRAD_BITS]
    return tuple(c)


def refusals(cfg):
    return ("fe_vmix", "run_fe_vmix", "tape_vmix", "visc_tape", "stress_tape", "dt_negative_rk4", "dt_negative_run", "dt_negative_ft",
            "visc_invalid", "stress_nan", "ft_nonlinear", "ft_tape", "tape_forced", "nonlinear_forced", "placement_forced",
            "stress_recorded", "ft_want_recorded", "ft_full", "ft_sweep_unseeded", "ft_density_unflagged")


WRITERS_EVERY_READ = ("visc", "stress", "rk4", "run", "fe", "upload", "ft_taped", "variant")
WRITERS_ANY_READ = ("nonlinear", "del2", "del4", "tuning", "placement", "tape_create", "rk4_taped", "seed", "sweep", "tape_destroy",
                    "ft_create", "ft_want", "ft_seed_ssh", "ft_seed_free", "ft_sweep", "ft_destroy")


def pairs_wanted(cfg):
    """(pairs, writers): every pair (writer, read kind) of the first, and every writer of the second with at least one read kind, must
    occur with the read being the first of its array since the writer."""
    w = WRITERS_EVERY_READ + (("rk4_s13",) if cfg.s13 else ())
    return {(k, r) for k in w for r in READ_KINDS}, WRITERS_ANY_READ + (("run_s13",) if cfg.s13 else ())


def cases_wanted(cfg):
    c = [("first", f, r) for f in DIAG + TEND for r in READ_KINDS]
    c += ["s13_between_runs"] if cfg.s13 else []
    c += ["change_then_tend", "change_then_diag", "visc_between_runs", "stress_between_runs", "ft_destroy_pending", "ft_tend_after_sweep",
          "ft_values_between", "ft_variant_between", "off_then_fe", "dt0_on"]
    return tuple(c)


def cases_seen(cfg, ops, obs):
    """The named orders a sequence shows.  The model's observations say in which steps the pass ran (Obs.info)."""
    seen = set()
    unread = set()                 # Diag / Tend arrays not read since the last step in which the pass ran ...
    changed = False                # ... and a visc / stress op was accepted since that step
    rv = rs = 0                    # visc_between_runs: 1 a run of nine, 2 a visc op behind it;  stress_between_runs: 1, 2 uploaded, 3 removed
    ftp = 0                        # 1: a forced taped step's tendencies pending, 2: and the tape destroyed, 3: and the tape swept
    ftv = None                     # ft_values_between: dict(on: the first step's, changed, done)
    ftvar = 0                      # 1 a forced taped step, 2 a variant switch behind it
    fe, fe_levels = 0, set()       # off_then_fe: 1 a mixed step, 2 a Forward-Euler step behind it; the levels read since
    dt0 = False
    for op, o in zip(ops, obs):
        if o.rc != OK:
            continue
        k, a, info = op.kind, op.args, getattr(o, "info", {})
        if k in STEP_KINDS:
            on = bool(info.get("on"))
            unread = set(DIAG + TEND) if info.get("mixed") else set()
            changed = False
            ftp = 1 if k == "ft_taped" else 0
            if ((k == "run" and a[0] == 1 and a[1] == 9) or (k == "run_s13" and a[0] == 9)) and on and info.get("mixed"):
                if rv == 2:
                    seen.add("visc_between_runs")
                    if k == "run_s13" and info.get("streams") == 13:
                        seen.add("s13_between_runs")
                if rs == 3:
                    seen.add("stress_between_runs")
                rv, rs = 1, (2 if rs == 2 else 1)
            else:
                rv = rs = 0
            fe, fe_levels = ((2 if fe == 1 else 0) if k == "fe" else (1 if info.get("mixed") else 0)), set()
            dt0 = on and info.get("dt") == 0.0
            if k == "ft_taped":
                ftvar = 1
                if ftv is not None and ftv["changed"] and ftv["on"] != on:
                    ftv["done"] = True
                elif ftv is None or not ftv["done"]:
                    ftv = dict(on=on, changed=False, done=False)
        elif k in ("visc", "stress"):
            changed = True
            if k == "visc":
                rv = 2 if rv in (1, 2) else 0
            else:
                rs = 2 if (rs in (1, 2) and a[0] in ("field", "other")) else 3 if (rs == 2 and a[0] == "none") else 0
            if ftv is not None and not ftv["done"]:
                ftv["changed"] = True
        elif k == "variant":
            ftvar = 2 if ftvar in (1, 2) else 0
        elif k == "ft_destroy":
            ftp = 2 if ftp == 1 else 0
            ftv, ftvar = None, 0
        elif k == "ft_sweep":
            if info.get("steps"):
                ftp = 3 if ftp in (1, 3) else ftp
                if ftv is not None and ftv["done"] and info.get("want") == 7:
                    seen.add("ft_values_between")
                if ftvar == 2:
                    seen.add("ft_variant_between")
            ftv, ftvar = None, 0
        elif k in READ_KINDS:
            f, l = a[0], a[1]
            if f in unread:
                unread.discard(f)
                seen.add(("first", f, k))
                if changed:
                    seen.add("change_then_tend" if f in TEND else "change_then_diag")
            if f in TEND:
                if ftp == 2:
                    seen.add("ft_destroy_pending")
                if ftp == 3:
                    seen.add("ft_tend_after_sweep")
                ftp = 0
            if fe == 2 and f in PROG:
                fe_levels.add(l)
                if fe_levels == {0, 1}:
                    seen.add("off_then_fe")
            if dt0:
                seen.add("dt0_on")
    return seen


# ---------------------------------------------------------------------------------------------------------------------------------
# generator: a pure function of (config, seed)
# ---------------------------------------------------------------------------------------------------------------------------------
class _Abstract:
    """What the generator has to know to aim: which values are in force, which handles live, which arrays changed since their last read."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.visc, self.stress = "zero", "none"
        self.nonlinear, self.visc2, self.visc4, self.variant = False, 0, 0, 0
        self.tape = None               # dict(cap, n, seeded)
        self.ft = None                 # dict(cap, n, seeded, want)
        self.dirty = []                # keys, the most recently changed last

    def on(self):
        return self.visc != "zero" or self.stress in ("field", "other")

    def touch(self, keys):
        for k in keys:
            if k in self.dirty:
                self.dirty.remove(k)
            self.dirty.append(k)

    def stepped(self, dtf=1.0):
        if dtf == 0.0:                 # the new level has the bits of the old one: only the previous level and the tendencies move
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
        elif k in ("rk4", "rk4_s13"):
            if not (a[0] < 0 and self.on()):
                self.stepped(a[0])
        elif k == "run":
            if a[0] == 0 and (self.on() or self.nonlinear):
                return
            if a[0] == 1 and a[3] < 0 and self.on():
                return
            self.stepped(a[3] if a[0] == 1 else 1.0)
        elif k == "run_s13":
            if not (a[1] < 0 and self.on()):
                self.stepped(a[1])
        elif k == "fe":
            if not (self.on() or self.nonlinear):
                self.stepped()
        elif k == "nonlinear":
            if not (a[0] and (t or ft)):
                self.nonlinear = bool(a[0])
        elif k == "del2":
            if self.nonlinear or not a[0]:
                self.visc2 = a[0]
        elif k == "del4":
            if self.nonlinear or not a[0]:
                self.visc4 = a[0]
        elif k == "variant":
            if a[0] in cs.VARIANTS:
                self.variant = a[0]
        elif k == "upload":
            self.touch([(a[0], a[1])])
        elif k in READ_KINDS:
            if (a[0], a[1]) in self.dirty:
                self.dirty.remove((a[0], a[1]))
        elif k == "tape_create":
            if not (self.on() or self.nonlinear or ft):
                self.tape = dict(cap=a[0], n=0, seeded=False)
        elif k == "tape_destroy":
            self.tape = None
        elif k == "rk4_taped":
            if t["n"] < t["cap"]:
                t["n"] += 1
                t["seeded"] = False
                self.stepped()
        elif k == "seed":
            t["seeded"] = True
        elif k == "sweep":
            t["n"] = 0
        elif k == "ft_create":
            if not (t or self.nonlinear):
                self.ft = dict(cap=a[0], n=0, seeded=False, want=0)
        elif k == "ft_destroy":
            self.ft = None
        elif k == "ft_want":
            if ft["n"] == 0:
                ft["want"] = (ft["want"] | a[0]) if a[1] else (ft["want"] & ~a[0])
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
    K = cfg.K
    ops = []
    vs = [0]

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
            if len(rows) > 1 and rng.random() < 0.5:
                rows = rows + (rows[0],)
            return Op("rows", (key[0], key[1], rows))
        return Op(kind, key)

    pending = [(f, 1) for f in DIAG + TEND]

    def fe_flags():
        return int(rng.integers(0, 4))

    def a_visc(on=None):
        pats = [p for p in VISC_OK if p != ab.visc and (on is None or (p != "zero") == on)]
        return Op("visc", (draw(pats),))

    def a_stress(on=None):
        pats = [p for p in stress_patterns(cfg) if p != ab.stress and (on is None or (p in ("field", "other")) == on)]
        return Op("stress", (draw(pats),))

    def stress_free():
        return not ab.tape and not (ab.ft and ab.ft["n"] > 0)

    def a_plain_step():
        c = [("rk4", 4), ("run3", 1.5), ("run9", 0.7)] + ([("rk4_s13", 2.5), ("run9_s13", 0.7)] if cfg.s13 and not ab.nonlinear else [])
        name = draw([x[0] for x in c], [x[1] for x in c])
        if name == "run9_s13":
            return Op("run_s13", (9, 1.0))
        if name in ("rk4", "rk4_s13"):
            return Op(name, (0.0 if rng.random() < 0.12 else 1.0,))
        return Op("run", (1, 3 if name == "run3" else 9, 0, 1.0))

    # ---- what a scene needs first ----
    def ensure_no_tape():
        if ab.tape:
            yield Op("tape_destroy")

    def ensure_on():
        yield from ensure_no_tape()
        if not ab.on():
            yield a_stress(True) if (stress_free() and rng.random() < 0.4) else a_visc(True)

    def ensure_off():
        if ab.visc != "zero":
            yield Op("visc", ("zero",))
        if ab.stress in ("field", "other"):
            if ab.ft and ab.ft["n"] > 0:
                yield Op("ft_destroy")
            yield Op("stress", (draw([p for p in stress_patterns(cfg) if p not in ("field", "other")]),))

    def ensure_linear():
        if ab.nonlinear:
            yield Op("nonlinear", (0,))

    def ensure_ft(cap=None, room=1):
        yield from ensure_no_tape()
        yield from ensure_linear()
        if ab.ft and ab.ft["cap"] - ab.ft["n"] < room:
            yield Op("ft_destroy")
        if not ab.ft:
            yield Op("ft_create", (cap or int(rng.integers(max(room, 1), 4)),))

    def recorded_refusal(p=0.35):
        """Now and then what a forced tape with recorded steps refuses: a sweep without a seed, a flag, a stress upload."""
        if rng.random() < p and ab.ft and ab.ft["n"] > 0 and not ab.ft["seeded"]:
            return draw((Op("ft_sweep"), Op("ft_want", (draw(GRAD_BITS), int(rng.integers(2)))), Op("stress", (draw(stress_patterns(cfg)),))))
        return None

    # ---- scenes ----
    def scene_mixed_read():
        yield from ensure_on()
        yield a_plain_step()
        for _ in range(int(rng.integers(1, 3))):
            yield a_read(pending)

    def scene_change_then_read():
        yield from ensure_on()
        yield a_plain_step() if not (ab.ft and ab.ft["n"] < ab.ft["cap"] and rng.random() < 0.4) else Op("ft_taped", (1.0,))
        yield a_stress() if (stress_free() and rng.random() < 0.5) else a_visc()
        yield a_read([(f, 1) for f in TEND])
        yield a_read([(f, 1) for f in DIAG])

    def scene_runs():
        yield from ensure_on()
        if cfg.s13 and not ab.nonlinear and rng.random() < 0.4:      # the 13-stream form: the graph's 6-step period
            yield Op("run_s13", (9, 1.0))
            yield a_visc(True)
            yield Op("run_s13", (9, 1.0))
            yield a_read()
            yield a_read(pending)
            return
        yield Op("run", (1, 9, 0, 1.0))
        if stress_free() and rng.random() < 0.5:
            if ab.visc == "zero":
                yield a_visc(True)                         # the pass stays on when the stress goes
            yield a_stress(True)
            if rng.random() < 0.5:
                yield Op("run", (1, 9, 0, 1.0))
            yield Op("stress", ("none",))
        else:
            yield a_visc(True)
        yield Op("run", (1, 9, 0, 1.0))
        yield a_read()
        yield a_read(pending)

    def scene_ft_pending():
        yield from ensure_ft()
        if rng.random() < 0.7:
            yield from ensure_on()
        elif not ab.on():
            yield Op("tape_create", (2,))                   # refused: a forced tape exists
        yield Op("ft_taped", (1.0,))
        if rng.random() < 0.5:
            yield Op("ft_destroy")
        else:
            yield Op("ft_seed_ssh") if rng.random() < 0.5 else Op("ft_seed_free", (vseed(),))
            yield Op("ft_sweep")
        yield a_read([(f, 1) for f in TEND])
        if ab.ft:
            yield Op("ft_download", (draw((F_U, F_H)),))

    def scene_ft_values():
        yield from ensure_ft(cap=int(rng.integers(2, 4)), room=2)
        if ab.ft["n"] > 0 or ab.ft["cap"] < 2:
            yield Op("ft_destroy")
            yield Op("ft_create", (int(rng.integers(2, 4)),))
        yield Op("ft_want", (7 & ~ab.ft["want"] or 7, 1)) if ab.ft["want"] != 7 else None
        first_on = rng.random() < 0.5
        if first_on and ab.visc == "zero":
            yield a_visc(True)
        if not first_on:
            yield from ensure_off()
        yield Op("ft_taped", (1.0,))
        if first_on:                                       # (a stress cannot go while a step is recorded: the pass then stays on)
            yield a_visc() if ab.stress in ("field", "other") else Op("visc", ("zero",))
        else:
            yield a_visc(True)
        yield Op("ft_taped", (1.0,))
        yield recorded_refusal()
        yield Op("ft_seed_ssh") if rng.random() < 0.5 else Op("ft_seed_free", (vseed(),))
        yield Op("ft_sweep")
        for b in rng.permutation(3):
            yield Op(draw(("ft_density", "ft_gradient")), (GRAD_BITS[int(b)],))
        yield Op("ft_download", (draw((F_U, F_H)),))

    def scene_ft_variant():
        yield from ensure_ft()
        yield from ensure_on()
        yield Op("ft_taped", (0.0 if rng.random() < 0.15 else 1.0,))
        yield Op("variant", (draw([v for v in cfg.variants if v != ab.variant and (3 in (v, ab.variant) or rng.random() < 0.3)] or [3]),))
        yield recorded_refusal()
        yield Op("ft_seed_ssh") if rng.random() < 0.5 else Op("ft_seed_free", (vseed(),))
        yield Op("ft_sweep")
        yield Op("ft_path")
        yield Op("ft_download", (F_U,))
        yield Op("ft_download", (F_H,))

    def scene_ft_flags():
        yield from ensure_ft()
        if ab.ft["n"] > 0:
            yield Op("ft_destroy")
            yield Op("ft_create", (int(rng.integers(1, 4)),))
        b = draw(GRAD_BITS)
        yield Op("ft_want", (b, 1))
        if rng.random() < 0.5:
            yield Op("ft_want", (b, 0))
            yield Op("ft_want", (draw(GRAD_BITS), 1))
        if rng.random() < 0.7:
            yield from ensure_on()
        yield Op("ft_taped", (1.0,))
        yield recorded_refusal()
        yield Op("ft_seed_free", (vseed(),))
        yield Op("ft_sweep")
        for b in GRAD_BITS:
            if ab.ft["want"] & b:
                yield Op(draw(("ft_density", "ft_gradient")), (b,))
        yield Op("ft_density", (draw([b for b in GRAD_BITS if not ab.ft["want"] & b] or [8]),))      # refused: not flagged

    def scene_n1():
        """Only nuV on, a recorded step, a sweep, XU: the columns with n == 1 keep their bits."""
        yield from ensure_ft()
        if ab.stress in ("field", "other") and ab.ft["n"] > 0:
            yield Op("ft_destroy")
            yield Op("ft_create", (2,))
        if ab.stress in ("field", "other"):
            yield Op("stress", ("none",))
        if ab.visc != "nu":
            yield Op("visc", ("nu",))
        yield Op("ft_taped", (1.0,))
        yield Op("ft_seed_free", (vseed(),))
        yield Op("ft_sweep")
        yield Op("ft_download", (F_U,))

    def scene_off_then_fe():
        yield from ensure_linear()
        yield from ensure_on()
        yield a_plain_step()
        yield from ensure_off()
        yield Op("fe", (fe_flags(),))
        f = draw(PROG)
        yield a_read([(f, 1)])
        yield a_read([(f, 0)])
        yield a_read(pending)

    def scene_dt0():
        yield from ensure_on()
        yield Op("rk4", (0.0,)) if not (cfg.s13 and not ab.nonlinear and rng.random() < 0.4) else Op("rk4_s13", (0.0,))
        yield a_read()
        yield a_read()

    def scene_plain_tape():
        if ab.ft:
            yield Op("ft_destroy")
        yield from ensure_off()
        yield from ensure_linear()
        yield from ensure_no_tape()
        yield Op("tape_create", (int(rng.integers(1, 3)),))
        yield Op("rk4_taped")
        yield draw((Op("visc", (draw(VISC_OK[1:]),)), Op("stress", (draw(stress_patterns(cfg)[1:]),)), Op("ft_create", (2,)),
                    Op("visc", ("zero",)), Op("stress", ("none",))))
        yield a_read(pending)
        yield Op("seed")
        yield Op("sweep")
        yield Op("adj_download", (draw((F_U, F_H)),))
        yield a_read()
        if rng.random() < 0.5:
            yield Op("tape_destroy")

    def scene_ft_full():
        yield from ensure_ft()
        if rng.random() < 0.5:
            yield from ensure_on()
        while ab.ft["n"] < ab.ft["cap"]:
            yield Op("ft_taped", (1.0,))
        yield Op("ft_taped", (1.0,))                        # refused: the tape is full
        yield a_read(pending)
        yield Op("ft_seed_ssh")
        yield Op("ft_sweep")
        yield Op("ft_download", (draw((F_U, F_H)),))

    def scene_step_mutate_read():
        """A step, then something that changes an input of what the step left pending, then a read of it."""
        if rng.random() < 0.6:
            yield from ensure_on()
        yield a_plain_step() if not (ab.ft and ab.ft["n"] < ab.ft["cap"] and rng.random() < 0.3) else Op("ft_taped", (1.0,))
        c = [Op("upload", (draw((F_U, F_H)), 1, vseed())), Op("upload", (draw(PROG), int(rng.integers(2)), vseed()))]
        if not ab.tape and not ab.ft:
            c += [Op("nonlinear", (0 if ab.nonlinear else 1,))] * 2
        if ab.nonlinear:
            c += [Op("del2", (0 if ab.visc2 else 1,)), Op("del4", (0 if ab.visc4 else int(rng.integers(1, 3)),))]
        yield draw(c)
        yield a_read([(f, 1) for f in DIAG + TEND])
        yield a_read([(f, 1) for f in DIAG + TEND])

    def scene_nonlinear():
        """The nonlinear dycore under the pass, and what refuses it."""
        if ab.ft or ab.tape:
            yield Op("ft_destroy") if ab.ft else Op("tape_destroy")
        if not ab.nonlinear:
            yield Op("nonlinear", (1,))
        yield draw((Op("del2", (0 if ab.visc2 else 1,)), Op("del4", (0 if ab.visc4 else int(rng.integers(1, 3)),)), Op("ft_create", (2,))))
        if rng.random() < 0.7:
            yield from ensure_on()
        yield Op("rk4", (1.0,)) if rng.random() < 0.7 else Op("run", (1, 3, 0, 1.0))
        yield a_read(pending)
        yield draw((Op("ft_create", (2,)), Op("del4", (0 if ab.visc4 else int(rng.integers(1, 3)),)), Op("nonlinear", (0,))))
        yield a_read(pending)

    def a_refusal():
        c = [Op("visc", (draw(VISC_BAD),)), Op("stress", ("nan",)), Op("variant", (draw((1, 2, 5, 9)),))]
        t, ft = ab.tape, ab.ft
        if ab.on():
            c += [Op("fe", (fe_flags(),)), Op("run", (0, 3, fe_flags(), 1.0)), Op("rk4", (-1.0,)), Op("run", (1, 3, 0, -1.0))] * 2
            if not t and not ft:
                c += [Op("tape_create", (2,))] * 3
            if ft and ft["n"] < ft["cap"]:
                c += [Op("ft_taped", (-1.0,))] * 4
        if t:
            c += [Op("visc", (draw(VISC_OK[1:]),)), Op("stress", (draw(stress_patterns(cfg)[1:]),)), Op("ft_create", (2,))] * 2
        if ab.nonlinear and not ft:
            c += [Op("ft_create", (2,))] * 4
        if not ab.nonlinear:
            c += [Op("del2", (1,))]
        if ft:
            c += [Op("tape_create", (2,)), Op("nonlinear", (1,)), Op("placement", (1,))] * 2
            if not ab.on():
                c += [Op("tape_create", (2,))] * 4
            if ft["n"] > 0:
                c += [Op("stress", (draw(stress_patterns(cfg)),)), Op("ft_want", (draw(GRAD_BITS), int(rng.integers(2))))] * 3
                if not ft["seeded"]:
                    c += [Op("ft_sweep")] * 3
            if ft["n"] >= ft["cap"]:
                c += [Op("ft_taped", (1.0,))] * 5
            if ft["want"] != 7:
                c += [Op("ft_density", (draw([b for b in GRAD_BITS if not ft["want"] & b]),))]
        return draw(c)

    def a_single():
        t, ft = ab.tape, ab.ft
        c = [("step", 4), ("visc", 3), ("upload", 3), ("variant", 2), ("tuning", 1), ("getter", 2), ("refusal", 5)]
        if stress_free():
            c += [("stress", 3)]
        if not t and not ft:
            c += [("placement", 1), ("nonlinear", 1.5)]
        if ab.nonlinear:
            c += [("mixing", 2), ("nonlinear", 1)]
        if not ab.on() and not ab.nonlinear:
            c += [("fe", 2), ("run_fe", 1)]
        if ft:
            c += [("ft", 5)]
        name = draw([x[0] for x in c], [x[1] for x in c])
        if name == "step":
            return a_plain_step()
        if name == "visc":
            return a_visc() if not t else Op("visc", ("zero",))
        if name == "stress":
            return a_stress()
        if name == "upload":
            return Op("upload", (draw(PROG), int(rng.integers(2)), vseed()))
        if name == "variant":
            return Op("variant", (draw([v for v in cfg.variants if v != ab.variant]),))
        if name == "tuning":
            return Op("tuning", (8, draw(cs.TUNING_VALUES[8])))
        if name == "getter":
            return Op(draw(("visc_read", "stress_download", "has_stress", "vmix_path")))
        if name == "refusal":
            return a_refusal()
        if name == "placement":
            return Op("placement", (int(rng.integers(2)),))
        if name == "nonlinear":
            return Op("nonlinear", (0 if ab.nonlinear else 1,))
        if name == "mixing":
            return Op("del4", (0 if ab.visc4 else int(rng.integers(1, 3)),)) if rng.random() < 0.5 else Op("del2", (0 if ab.visc2 else 1,))
        if name == "fe":
            return Op("fe", (fe_flags(),))
        if name == "run_fe":
            return Op("run", (0, 3, fe_flags(), 1.0))
        # a forced tape is open
        if ft["n"] > 0 and ft["seeded"]:
            return Op("ft_sweep")
        if ft["n"] > 0 and rng.random() < 0.5:
            return Op("ft_seed_ssh") if rng.random() < 0.5 else Op("ft_seed_free", (vseed(),))
        if ft["n"] < ft["cap"]:
            return Op("ft_taped", (0.0 if rng.random() < 0.15 else 1.0,))
        return Op("ft_destroy") if rng.random() < 0.4 else Op("ft_seed_ssh")

    scenes = [(scene_mixed_read, 5), (scene_change_then_read, 4), (scene_runs, 2), (scene_ft_pending, 3.5), (scene_ft_values, 2.5),
              (scene_ft_variant, 2.5), (scene_ft_flags, 2.5), (scene_off_then_fe, 2.5), (scene_dt0, 1.5), (scene_plain_tape, 2.5),
              (scene_ft_full, 1.5), (scene_step_mutate_read, 4),
              (scene_nonlinear, 2.5)]
    if cfg.depths == "shelf" or K == 1:
        scenes += [(scene_n1, 2)]
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
        if ab.dirty and r < 0.3:
            op = a_read()
        elif r < 0.65:
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
def _n1_depth(mlt, K, q, st, on):
    """Mutant n1_always: forced_adjoint_twin.computed_depth with every wet column computed."""
    nn = np.clip(np.asarray(mlt, dtype=np.int64), 0, K)
    return np.where((nn >= 1) & bool(on), nn, 0)


class ForcedModel(cs.Model):
    """Machine C on the CPU oracle and the twins, eagerly, as include/moka_hip.h words each call.  mutant: one of C_MUTANTS."""

    def __init__(self, cfg, seed, mutant=None):
        assert mutant is None or mutant in C_MUTANTS
        super().__init__(cfg, seed, mutant if mutant in cs.MUTANTS else None)
        self.mutant = mutant
        self.mlt = depths_of(cfg)
        if mask_of(cfg) is not None:       # the base knows masks.basin only: the same state over this config's own depths
            self.om = orc.OracleMesh(self.mesh, cfg.K, resting_thickness_sum=resting_thickness(cfg).sum(1), max_level_edge_top=self.mlt)
            self.st = orc.OracleState(self.om, *(np.zeros(shape_of(cfg, f)) for f in (F_SSH, F_U, F_H)))
            for (f, l), arr in initial_state(cfg, seed).items():
                self.array((f, l))[...] = arr
            self._last_read = self._snapshot()
        self.mix = mv.MomentumVmixTwin(SimpleNamespace(om=self.om))      # nu, drag, tau: the values in force
        self.stress = None             # what moka_surface_stress_download answers (None: no stress)
        self.lagged = None             # mutant values_late: what the previous step ran with
        self.path = 0                  # moka_state_momentum_vmix_path
        self.ft = None                 # dict(cap, recs, seeded, want, dens, X, path)
        self.last = {}                 # what the last step did (Obs.info)
        self._rk = None

    # ---- the pass ----
    def on(self):
        return mv.pass_on(self.mix.nu, self.mix.drag, self.mix.tau, self.mlt)

    def _step_rk4(self, dt, s13=False):
        st, mx = self.st, self.mix
        cur = (mx.nu, mx.drag, mx.tau)
        use = cur
        if self.mutant == "values_late":
            use = self.lagged if self.lagged is not None else cur
            self.lagged = cur
        super()._step_rk4(dt, s13)
        nu, drag, tau = use
        on = mv.pass_on(nu, drag, tau, self.mlt)
        self.last = dict(on=on, mixed=False, dt=dt, nu=nu, drag=drag, tau=tau if mv.stress_on(tau, self.mlt) else None)
        if not on or dt == 0.0:
            return
        if not (self.cfg.K < 2 and drag == 0.0 and self.last["tau"] is None):
            self.path = mv.form_of(self.cfg.K, self.variant == 3)
        self.last["mixed"] = True
        mx.nu, mx.drag, mx.tau = nu, drag, tau
        st.u[1][...] = mx.mix(st.u[1], st.h[1], dt)
        mx.nu, mx.drag, mx.tau = cur
        if self.mutant != "diag_unmixed":
            self._clean_diag()             # the diagnostics of the new level come from the mixed u
        if self.mutant == "tend_mixed":
            tu, th, _ = self._tendencies(st.u[1], st.h[1])
            st.tendU[...] = tu; st.tendH[...] = th

    # ---- the forced tape ----
    def _reverse_rk4(self, P, dt, XU, XH):
        if self._rk is None:
            self._rk = orc.OracleAdjointRK4(self.st)
        return fa.ForcedTwin.reverse_rk4(SimpleNamespace(rk=self._rk), P, dt, XU, XH)

    def _ft_sweep(self):
        ft = self.ft
        XU, XH = ft["X"]
        dens = {b: ft["dens"][b] for b in GRAD_BITS if ft["want"] & b}
        generic = self.variant == 3
        depth = _n1_depth if self.mutant == "n1_always" else None
        for r in reversed(ft["recs"]):
            if r["rec"] and r["dt"] != 0.0:
                XU, XH = fa.transposed_pass(self.mesh, self.mlt, XU, XH, r["un"], r["hn"], r["dt"], r["nu"], r["drag"], r["tau"], dens,
                                            depth_of=depth)
                if ft["want"] or (r["on"] and not (self.cfg.K < 2 and r["drag"] == 0.0 and r["tau"] is None)):
                    ft["path"] = 1 if tile_columns_grad(self.cfg.K, generic) else 2
            XU, XH = self._reverse_rk4(r["P"], r["dt"], XU, XH)
        ft["X"] = (XU, XH)
        ft["recs"] = []

    # ---- one op ----
    def apply(self, op):
        o = self._apply(op)
        if op.kind in STEP_KINDS and o.rc == OK:
            o.info = dict(self.last)
        return o

    def _apply(self, op):
        cfg, st, k, a, mx, ft = self.cfg, self.st, op.kind, op.args, self.mix, self.ft
        K = cfg.K
        R = lambda code, name: Obs(k, code, refusal=name)
        # a NULL handle (only a mutant, which was refused the create, gets here): MOKA_ERR_ARG, and the destroy calls do nothing
        if (k in ("rk4_taped", "seed", "sweep", "adj_download") and self.tape is None) or (k.startswith("ft_") and ft is None and
                                                                                           k not in ("ft_create", "ft_destroy", "ft_path")):
            return R(ERR_ARG, "null_handle")
        if k == "visc":
            nu, r = visc_values(cfg, a[0])
            if not (nu >= 0.0 and r >= 0.0 and np.isfinite(nu) and np.isfinite(r)):
                return R(ERR_ARG, "visc_invalid")
            if (nu != 0.0 or r != 0.0) and self.tape is not None:
                return R(ERR_UNSUPPORTED, "visc_tape")
            mx.nu, mx.drag = nu, r
            return Obs(k, OK)
        if k == "stress":
            tau = stress_values(cfg, a[0])
            if tau is not None and not np.all(np.isfinite(tau)):
                return R(ERR_ARG, "stress_nan")
            if tau is not None and self.tape is not None:
                return R(ERR_UNSUPPORTED, "stress_tape")
            if ft is not None and ft["recs"]:
                return R(ERR_UNSUPPORTED, "stress_recorded")
            self.stress = tau
            if not (self.mutant == "stress_sticky" and not mv.stress_on(tau, self.mlt)):
                mx.tau = tau
            return Obs(k, OK)
        if k == "visc_read":
            return Obs(k, OK, value=(mx.nu, mx.drag))
        if k == "stress_download":
            return Obs(k, OK, value=np.zeros(self.mesh.nEdges) if self.stress is None else self.stress.copy())
        if k == "has_stress":
            return Obs(k, OK, value=int(self.stress is not None))
        if k == "vmix_path":
            return Obs(k, OK, value=self.path)
        if k in ("rk4", "rk4_s13"):
            dt = dt_of(cfg, a[0])
            n = self.streams(k == "rk4_s13")
            if dt < 0.0 and self.on():
                return R(ERR_ARG, "dt_negative_rk4")
            self._step_rk4(dt, s13=n == 13)
            return Obs(k, OK, value=n)
        if k == "run":
            integ, n, flags, f = a
            if integ == 0:
                if self.on():
                    return R(ERR_UNSUPPORTED, "run_fe_vmix")
                r = self._fe_refusal(k, flags)
                if r:
                    return r
            elif dt_of(cfg, f) < 0.0 and self.on():
                return R(ERR_ARG, "dt_negative_run")
            for _ in range(n):
                self._step_fe(cfg.dt, flags) if integ == 0 else self._step_rk4(dt_of(cfg, f))
            if integ == 0:
                self.last = dict(on=False, mixed=False, dt=cfg.dt)
            return Obs(k, OK)
        if k == "run_s13":
            n13, dt = self.streams(True), dt_of(cfg, a[1])
            if dt < 0.0 and self.on():
                return R(ERR_ARG, "dt_negative_run")
            for _ in range(a[0]):
                self._step_rk4(dt, s13=n13 == 13)
            self.last["streams"] = n13
            return Obs(k, OK, value=n13)
        if k == "fe":
            if self.on():
                return R(ERR_UNSUPPORTED, "fe_vmix")
            self.last = dict(on=False, mixed=False, dt=cfg.dt)
        if k == "tape_create":
            if self.on():
                return R(ERR_UNSUPPORTED, "tape_vmix")
            if ft is not None:
                return R(ERR_UNSUPPORTED, "tape_forced")
        if k == "nonlinear" and a[0] and ft is not None:
            return R(ERR_UNSUPPORTED, "nonlinear_forced")
        if k == "placement" and ft is not None:
            return R(ERR_UNSUPPORTED, "placement_forced")
        if k == "ft_create":
            if self.tape is not None:
                return R(ERR_UNSUPPORTED, "ft_tape")
            if self.nonlinear:
                return R(ERR_UNSUPPORTED, "ft_nonlinear")
            z = lambda f: np.zeros(shape_of(cfg, f))
            self.ft = dict(cap=a[0], recs=[], seeded=False, want=0, dens={}, X=(z(F_U), z(F_H)), path=0)
            return Obs(k, OK)
        if k == "ft_destroy":
            self.ft = None
            return Obs(k, OK)
        if k == "ft_want":
            if ft["recs"]:
                return R(ERR_ARG, "ft_want_recorded")
            if a[1]:
                for b in GRAD_BITS:
                    if a[0] & b and b not in ft["dens"]:
                        ft["dens"][b] = np.zeros(self.mesh.nEdges)
                ft["want"] |= a[0]
            else:
                ft["want"] &= ~a[0]
            return Obs(k, OK)
        if k == "ft_taped":
            dt = dt_of(cfg, a[0])
            if len(ft["recs"]) >= ft["cap"]:
                return R(ERR_ARG, "ft_full")
            if dt < 0.0 and self.on():
                return R(ERR_ARG, "dt_negative_ft")
            u0, h0 = st.u[1].copy(), st.h[1].copy()
            P, pu, ph = [(u0, h0)], u0, h0
            for s in (dt / 2., dt / 2., dt):
                tu, th, _ = self.om.tendencies_clean(pu, ph)
                pu, ph = u0 + s * tu, h0 + s * th
                P.append((pu, ph))
            self._step_rk4(dt)
            L = self.last
            ft["recs"].append(dict(P=P, dt=float(dt), rec=L["on"] or ft["want"] != 0, on=L["on"], un=st.u[1].copy(), hn=st.h[1].copy(),
                                   nu=L["nu"], drag=L["drag"], tau=L["tau"]))
            ft["seeded"] = False
            return Obs(k, OK)
        if k in ("ft_seed_ssh", "ft_seed_free"):
            if k == "ft_seed_ssh":
                ft["X"] = (np.zeros(shape_of(cfg, F_U)), np.repeat((2.0 * st.ssh[1])[:, None], K, axis=1))
            else:
                ft["X"] = free_seed(cfg, a[0])
            for d in ft["dens"].values():
                d[...] = 0.0
            ft["seeded"] = True
            return Obs(k, OK)
        if k == "ft_sweep":
            if not ft["seeded"]:
                return R(ERR_ARG, "ft_sweep_unseeded")
            o = Obs(k, OK)
            o.info = dict(steps=len(ft["recs"]), want=ft["want"])
            self._ft_sweep()
            return o
        if k == "ft_download":
            return Obs(k, OK, value=ft["X"][0 if a[0] == F_U else 1].copy())
        if k in ("ft_density", "ft_gradient"):
            if a[0] not in GRAD_BITS or not ft["want"] & a[0]:
                return R(ERR_ARG, "ft_density_unflagged")
            d = ft["dens"][a[0]]
            return Obs(k, OK, value=d.copy() if k == "ft_density" else fa.host_sum(d))
        if k == "ft_path":
            return Obs(k, OK, value=ft["path"] if ft is not None else 0)
        return super().apply(op)

    def run(self, ops):
        """As call_sequences.Model.run, with this machine's ops that fall between a change and its read (NON_ARRAY_OPS)."""
        out = []
        keys = STATE_KEYS + cs.ADJ_KEYS
        reads = READ_KINDS + ("adj_download",)
        before = self._snapshot()
        for op in ops:
            o = self.apply(op)
            if op.kind in reads:
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
    return (VTracerModel if isinstance(cfg, VTracerConfig) else ForcedModel)(cfg, seed, mutant)


def sequence_of(cfg, seed):
    return sequence_d(cfg, seed) if isinstance(cfg, VTracerConfig) else sequence(cfg, seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# device runner
# ---------------------------------------------------------------------------------------------------------------------------------
class ForcedDevice:
    """Machine C through moka_hip.lib: one device mesh per config, shared by its seeds; run() gives each sequence a fresh state.  Every
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
        self.counters = {"sequences": 0, "rk4_steps": 0, "fe_steps": 0, "s13": 0, "paths": set(), "ft_paths": set(), "run9_on": 0,
                         "mixed_steps": 0, "sweeps": 0, "run9_s13_on": 0}
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
        vp = lambda arr: arr.ctypes.data_as(C.c_void_p)

        def tune(key, value):
            if key not in saved:
                v = C.c_int()
                L.check(lib.moka_get_tuning(key, C.byref(v)))
                saved[key] = v.value
            return lib.moka_set_tuning(key, value)

        force = {"visc": (0.0, 0.0), "tau": None}      # what the last accepted visc and stress ops carried (for the counters only)

        def pass_on():
            """From the runner's own bookkeeping, so that no device call is added to the sequence."""
            return force["visc"] != (0.0, 0.0) or mv.stress_on(force["tau"], depths_of(cfg))

        def stepped(n, on, dt):
            cnt["rk4_steps"] += n
            if on and dt != 0.0:
                cnt["mixed_steps"] += n
                cnt["paths"].add(lib.moka_state_momentum_vmix_path(hS))

        try:
            L.check(lib.moka_state_create(ctx, self.M._h, C.byref(hS)), ctx)
            for (f, l), arr in initial_state(cfg, seed).items():
                L.check(lib.moka_state_upload(hS, f, l, L.f64(arr)), ctx)
            for op in ops:
                k, a = op.kind, op.args
                value = None
                if k == "visc":
                    rc = lib.moka_set_vertical_viscosity(hS, *visc_values(cfg, a[0]))
                    if rc == OK:
                        force["visc"] = visc_values(cfg, a[0])
                elif k == "stress":
                    tau = stress_values(cfg, a[0])
                    rc = lib.moka_surface_stress_upload(hS, None if tau is None else vp(tau))
                    if rc == OK:
                        force["tau"] = tau
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
                elif k in ("rk4", "rk4_s13"):
                    on = pass_on()
                    if k == "rk4_s13":
                        L.check(tune(7, 1))
                    try:
                        value = lib.moka_state_rk4_streams(hS)
                        rc = lib.moka_step_rk4(hS, dt_of(cfg, a[0]))
                    finally:
                        if k == "rk4_s13":
                            L.check(tune(7, 0))
                    if rc == OK:
                        stepped(1, on, a[0])
                        cnt["s13"] += value == 13
                elif k == "run":
                    on = pass_on()
                    rc = lib.moka_run(hS, a[0], dt_of(cfg, a[3]) if a[0] == 1 else cfg.dt, a[1], a[2])
                    if rc == OK and a[0] == 1:
                        stepped(a[1], on, a[3])
                        cnt["run9_on"] += a[1] == 9 and on
                    elif rc == OK:
                        cnt["fe_steps"] += a[1]
                elif k == "run_s13":
                    on = pass_on()
                    L.check(tune(7, 1))
                    try:
                        value = lib.moka_state_rk4_streams(hS)
                        rc = lib.moka_run(hS, 1, dt_of(cfg, a[1]), a[0], 0)
                    finally:
                        L.check(tune(7, 0))
                    if rc == OK:
                        stepped(a[0], on, a[1])
                        cnt["run9_on"] += a[0] == 9 and on
                        cnt["run9_s13_on"] += a[0] == 9 and on and value == 13
                elif k == "fe":
                    rc = lib.moka_step_fe(hS, cfg.dt, a[0])
                    cnt["fe_steps"] += rc == OK
                elif k == "nonlinear":
                    rc = lib.moka_set_nonlinear(hS, a[0])
                elif k == "del2":
                    rc = lib.moka_set_viscosity_del2(hS, cs.visc_del2(cfg) if a[0] else 0.0)
                elif k == "del4":
                    sc = cs.del4_scaling(cfg) if a[0] == 2 else None
                    rc = lib.moka_set_viscosity_del4(hS, cs.visc_del4(cfg) if a[0] else 0.0, None if sc is None else vp(sc))
                elif k == "variant":
                    rc = lib.moka_set_kernel_variant(ctx, a[0])
                elif k == "tuning":
                    rc = tune(a[0], a[1])
                elif k == "placement":
                    rc = lib.moka_state_optimize_placement(hS, a[0], None, None)
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
                elif k == "tape_create":
                    h = C.c_void_p()
                    rc = lib.moka_tape_create(hS, a[0], C.byref(h))
                    if rc == OK:
                        hT = h
                elif k == "tape_destroy":
                    lib.moka_tape_destroy(hT)
                    hT, rc = C.c_void_p(), OK
                elif k == "rk4_taped":
                    rc = lib.moka_step_rk4_taped(hT, cfg.dt)
                    if rc == OK:
                        stepped(1, False, 1.0)
                elif k == "seed":
                    rc = lib.moka_adjoint_seed_sum_sq_ssh(hT)
                elif k == "sweep":
                    rc = lib.moka_adjoint_sweep(hT)
                elif k == "adj_download":
                    value = np.full(shape_of(cfg, a[0]), np.nan)
                    rc = lib.moka_adjoint_download(hT, a[0], L.f64(value))
                elif k == "ft_create":
                    h = C.c_void_p()
                    rc = lib.moka_forced_tape_create(hS, a[0], C.byref(h))
                    if rc == OK:
                        hF = h
                elif k == "ft_destroy":
                    lib.moka_forced_tape_destroy(hF)
                    hF, rc = C.c_void_p(), OK
                elif k == "ft_want":
                    rc = lib.moka_forced_adjoint_want_gradient(hF, a[0], a[1])
                elif k == "ft_taped":
                    on = pass_on()
                    rc = lib.moka_step_rk4_forced_taped(hF, dt_of(cfg, a[0]))
                    if rc == OK:
                        stepped(1, on, a[0])
                elif k == "ft_seed_ssh":
                    rc = lib.moka_forced_adjoint_seed_sum_sq_ssh(hF)
                elif k == "ft_seed_free":
                    XU, XH = free_seed(cfg, a[0])
                    rc = lib.moka_forced_adjoint_seed(hF, vp(XU), vp(XH))
                elif k == "ft_sweep":
                    rc = lib.moka_forced_adjoint_sweep(hF)
                    if rc == OK:
                        cnt["sweeps"] += 1
                        cnt["ft_paths"].add(lib.moka_forced_tape_vmix_path(hF))
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
    return (VTracerDevice if isinstance(cfg, VTracerConfig) else ForcedDevice)(backend, cfg)


# ---------------------------------------------------------------------------------------------------------------------------------
# machine D: passive tracers with the vertical passes.  Model: call_sequences.TracerModel with tracer_vfield_twin.VfieldTwin /
# VfieldAdjointTwin (the top of the twin stack) in the place of its KgradTwin, and the momentum pass behind every step.
# ---------------------------------------------------------------------------------------------------------------------------------
D_MUTANTS = ("coeff_late", "mixed_flow_early", "prev_level_lost")
KV_PATTERNS = ("none", "some", "other")
VF_PATTERNS = ("none", "zero", "A", "B")
D_READS = READ_KINDS + ("tr_download",)
D_TAPE_READS = ("x_download", "v_density", "v_gradient")
D_GETTERS = ("vfield_download", "has_vfield", "kappaV_read", "tr_vmix_path", "visc_read")
D_STEPS = ("rk4", "run", "tr_taped")


@dataclass(frozen=True)
class VTracerConfig(cs.TracerConfig):
    variants: tuple = (0,)
    floor: bool = False            # a sea floor: tracer_vmix_twin.column_mlt (cells of depth 0, 1, 2, 3 and up to K)

    machine = "D"


D_CONFIGS = {c.name: c for c in (
    # 72-cell patches at K = 34 over a sea floor: the tile form of the vertical pass, columns of every depth
    VTracerConfig("D1", "planar", 34, dt=2.0, nT=3, patch_cells=72, tracer_path=1, nops=36, floor=True, reach=("vpath_1",)),
    # the variant toggles between 0 and 3: the tile and the column form of the vertical pass inside one history
    VTracerConfig("D2", "ico6f", 6, dt=20.0, nT=5, tracer_path=2, nops=36, variants=(0, 3), reach=("vpath_1", "vpath_2")),
)}
ALL_CONFIGS = {**V_CONFIGS, **D_CONFIGS}


def d_mask_of(cfg):
    import tracer_vmix_twin as tv
    return tv.column_mlt(get_mesh(cfg.meshname), cfg.K) if cfg.floor else None


def kappav_values(cfg, pattern, n):
    """The vector of a kappaV op: None (NULL), tracer_vmix_twin.kappavs (one exact zero), or the same values reversed."""
    import tracer_vmix_twin as tv
    if pattern == "none" or n == 0:
        return None
    k = tv.kappavs(cfg.meshname, cfg.K, n)
    return k if pattern == "some" else k[::-1]


def vfield_values(cfg, pattern, j):
    """The (nCells, K) doubles of a vfield op for tracer j: None (NULL), all zero, or uniform in [0, 2] x the largest kappaV with exact
    zeros at tracer_vfield_twin.ZEROS and below the first interface of cell 3 (no NaN: the field is read back whole)."""
    import tracer_vfield_twin as tf
    import tracer_vmix_twin as tv
    if pattern == "none":
        return None
    shp = shape_of(cfg, F_H)
    if pattern == "zero":
        return np.zeros(shp)
    f = np.random.default_rng([cfg.K, 77 if pattern == "A" else 78, j]).uniform(0.0, 2.0, shp) * tv.kappavs(cfg.meshname, cfg.K, 3)[0]
    for c, k in tf.ZEROS:
        if k < cfg.K:
            f[c, k] = 0.0
    f[3, 1:] = 0.0
    return f


def d_vocabulary(cfg):
    v = ("set_tracers", "tr_upload", "tr_download", "kappa", "kappaV", "vfield", "vfield_download", "has_vfield", "kappaV_read",
         "tr_vmix_path", "visc", "visc_read", "stress", "rk4", "run", "upload", "download", "rows", "sumsq", "fe",
         "tr_tape_create", "want_vgrad", "tr_taped", "tr_seed", "tr_sweep", "x_download", "v_density", "v_gradient", "tr_tape_destroy")
    return v + (("variant",) if len(cfg.variants) > 1 else ())


def d_arg_class(op):
    k, a = op.kind, op.args
    if k in ("set_tracers", "kappa", "kappaV", "visc", "stress", "variant", "rk4", "tr_taped"):
        return (k, a[0])
    if k in ("vfield", "want_vgrad"):
        return (k, a[1])
    if k == "v_density":
        return (k, a[1])
    if k == "run":
        return (k, a[1], a[3])
    if k in D_READS and k != "tr_download":
        return (k, a[0] in TEND)
    return None


def d_arg_classes(cfg):
    c = [("set_tracers", n) for n in (2, cfg.nT)] + [("kappa", p) for p in ("zero", "some")] + [("kappaV", p) for p in KV_PATTERNS]
    c += [("vfield", p) for p in VF_PATTERNS] + [("visc", p) for p in VISC_OK] + [("stress", p) for p in ("none", "zero", "field")]
    c += [("variant", v) for v in cfg.variants if len(cfg.variants) > 1] + [("rk4", f) for f in (1.0, 0.0)] + [("tr_taped", f) for f in (1.0, 0.0)]
    c += [("run", 3, 1.0), ("run", 3, 0.0), ("want_vgrad", 0), ("want_vgrad", 1)] + [("v_density", v) for v in (0, 1, 2)]
    return tuple(c + [(r, t) for r in READ_KINDS for t in (False, True)])


def d_refusals(cfg):
    return ("dt_negative_rk4", "dt_negative_run", "dt_negative_taped", "want_vgrad_recorded", "set_tracers_tape", "tape_full",
            "sweep_unseeded", "fe_tracers", "kappaV_invalid", "vfield_invalid", "v_density_unflagged")


def d_pairs_wanted(cfg):
    w = ("set_tracers", "tr_upload", "rk4", "run", "tr_taped", "kappa", "kappaV", "vfield", "visc", "stress", "tr_tape_create", "want_vgrad",
         "tr_seed", "tr_sweep") + (("variant",) if len(cfg.variants) > 1 else ())
    return {(k, "tr_download") for k in w} | {(k, r) for k in ("rk4", "run", "tr_taped", "upload") for r in READ_KINDS}


def d_cases_wanted(cfg):
    return ("count_change", "field_cycle", "kappaV_between", "visc_between", "run_dt0_on")


def d_cases_seen(cfg, ops, obs):
    seen = set()
    have = set()                   # "kappaV", "vfield": set and in force since the last moka_set_tracers
    fields = set()                 # the tracers that carry a field with nonzero entries
    cc = 0                         # count_change: 1 smaller, 2 larger again, 3 a step
    fc = None                      # field_cycle: [tracer, progress] behind a taped step
    kb = 0                         # kappaV_between: 1 a taped step with a flag, 2 a kappaV op behind it
    vb = 0                         # visc_between: 1 a step, 2 a tracer read, 3 a visc op, 4 a step
    flagged = False
    count = 0
    r0 = False                     # run_dt0_on: a moka_run with dt == 0.0 accepted while a vertical coefficient or the momentum pass is on
    for op, o in zip(ops, obs):
        if o.rc != OK:
            continue
        k, a = op.kind, op.args
        if k in D_STEPS:
            r0 = k == "run" and a[3] == 0.0 and bool(getattr(o, "info", {}).get("on"))
        elif k == "tr_download" and r0:
            seen.add("run_dt0_on")
        if k == "set_tracers":
            cc = 1 if (a[0] < count and have == {"kappaV", "vfield"}) else 2 if (cc == 1 and a[0] > count) else 0
            count, have, fields = a[0], set(), set()
        elif k == "kappaV":
            have = (have | {"kappaV"}) if a[0] != "none" else have - {"kappaV"}
            kb = 2 if kb in (1, 2) else 0
        elif k == "vfield":
            (fields.add if a[1] in ("A", "B") else fields.discard)(a[0])
            have = (have | {"vfield"}) if fields else have - {"vfield"}
            if fc is not None:
                j, n = fc
                if a[0] == j or n == 0:
                    on = a[1] in ("A", "B")
                    fc = [a[0], 1] if (n == 0 and on) else [j, 2] if (n == 1 and a[1] == "none") else [j, 3] if (n == 2 and on) else fc
        elif k == "tr_tape_create":
            flagged = False
        elif k == "want_vgrad":
            flagged = flagged or bool(a[1])
        elif k in D_STEPS:
            cc = 3 if cc == 2 else 0
            vb = 4 if vb == 3 else 1
            if k == "tr_taped":
                if fc is not None and fc[1] == 3:
                    seen.add("field_cycle")
                if kb == 2:
                    seen.add("kappaV_between")
                fc, kb = [None, 0], (1 if flagged else 0)
            else:
                fc, kb = None, 0
        elif k == "tr_sweep":
            fc, kb = None, 0
        elif k == "tr_download":
            if cc == 3:
                seen.add("count_change")
            if vb == 4:
                seen.add("visc_between")
            vb = 2 if vb == 1 else vb
        elif k == "visc":
            vb = 3 if vb in (2, 3) else 0
    return seen


def sequence_d(cfg, seed):
    """About cfg.nops ops of machine D, a pure function of (cfg, seed); scenes as in `sequence`."""
    rng = np.random.default_rng([zlib_crc(cfg.name), seed])
    ops, vs = [], [0]
    S = SimpleNamespace(nT=0, tape=None, kv="none", vf={}, visc="zero", stress="none", variant=0, dirty_tr=[], dirty_prog=[])

    def draw(items, weights=None):
        if weights is None:
            return items[int(rng.integers(len(items)))]
        w = np.asarray(weights, dtype=np.float64)
        return items[int(rng.choice(len(items), p=w / w.sum()))]

    def vseed():
        vs[0] += 1
        return 32452843 * (seed + 1) + vs[0]

    def vert_on():
        some = S.kv != "none"
        return any(p in ("A", "B") for p in S.vf.values()) or (some and any(j not in S.vf or S.vf[j] == "none" for j in range(S.nT)))

    def mom_on():
        return S.visc != "zero" or S.stress == "field"

    def touch(lst, keys):
        for k in keys:
            if k in lst:
                lst.remove(k)
            lst.append(k)

    def stepped():
        touch(S.dirty_tr, [(j, l) for l in (0, 1) for j in range(S.nT)])
        touch(S.dirty_prog, [(f, l) for l in (0, 1) for f in PROG] + [(f, 1) for f in TEND])

    def accept(op):
        k, a, t = op.kind, op.args, S.tape
        if k == "set_tracers":
            if t is None:
                S.nT, S.kv, S.vf, S.dirty_tr = a[0], "none", {}, []
        elif k == "tr_upload":
            touch(S.dirty_tr, [(a[0], a[1])])
        elif k == "tr_download":
            if (a[0], a[1]) in S.dirty_tr:
                S.dirty_tr.remove((a[0], a[1]))
        elif k == "kappaV":
            if a[0] != "bad":
                S.kv = a[0]
        elif k == "vfield":
            if a[1] != "bad":
                S.vf[a[0]] = a[1]
        elif k == "visc":
            if a[0] not in VISC_BAD:
                S.visc = a[0]
        elif k == "stress":
            S.stress = a[0]
        elif k == "variant":
            S.variant = a[0]
        elif k == "rk4":
            if not (a[0] < 0 and (vert_on() or mom_on())):
                stepped()
        elif k == "run":
            if not (a[3] < 0 and (vert_on() or mom_on())):
                stepped()
        elif k == "upload":
            touch(S.dirty_prog, [(a[0], a[1])])
        elif k in READ_KINDS:
            if (a[0], a[1]) in S.dirty_prog:
                S.dirty_prog.remove((a[0], a[1]))
        elif k == "tr_tape_create":
            S.tape = dict(cap=a[0], n=0, seeded=False, between=False, vfl=set(), nT=S.nT)
        elif k == "tr_tape_destroy":
            S.tape = None
        elif k == "want_vgrad":
            if t["n"] == 0 and not t["between"]:
                (t["vfl"].add if a[1] else t["vfl"].discard)(a[0])
        elif k == "tr_taped":
            if t["n"] < t["cap"] and not (a[0] < 0 and (vert_on() or mom_on())):
                t["n"] += 1
                t["seeded"] = t["between"] = False
                stepped()
        elif k == "tr_seed":
            t["seeded"] = t["between"] = True
        elif k == "tr_sweep":
            if t["seeded"]:
                t["n"], t["between"] = 0, False

    def a_read(tr=None, latest=False):
        if latest and S.dirty_prog:
            key = S.dirty_prog[-1]
            kind = draw(READ_KINDS)
            return Op("rows", key + (tuple(int(r) for r in rng.integers(0, shape_of(cfg, key[0])[0], 3)),)) if kind == "rows" else Op(kind, key)
        if S.dirty_tr and (tr or (tr is None and (not S.dirty_prog or rng.random() < 0.6))):
            return Op("tr_download", S.dirty_tr[-1 - int(rng.integers(min(3, len(S.dirty_tr))))])
        if S.dirty_prog and not tr:
            key = S.dirty_prog[-1 - int(rng.integers(min(4, len(S.dirty_prog))))]
            kind = draw(READ_KINDS)
            if kind == "rows":
                return Op("rows", key + (tuple(int(r) for r in rng.integers(0, shape_of(cfg, key[0])[0], 3)),))
            return Op(kind, key)
        return None

    def a_kappav(on=None):
        return Op("kappaV", (draw([p for p in KV_PATTERNS if p != S.kv and (on is None or (p != "none") == on)]),))

    def a_vfield(j=None, on=None):
        j = int(rng.integers(S.nT)) if j is None else j
        cur = S.vf.get(j, "none")
        return Op("vfield", (j, draw([p for p in VF_PATTERNS if p != cur and (on is None or (p in ("A", "B")) == on)])))

    def a_step():
        t = S.tape
        if t and t["n"] < t["cap"] and rng.random() < 0.6:
            return Op("tr_taped", (0.0 if rng.random() < 0.1 else 1.0,))
        if rng.random() < 0.25:
            return Op("run", (1, 3, 0, 0.0 if rng.random() < 0.2 else 1.0))
        return Op("rk4", (0.0 if rng.random() < 0.1 else 1.0,))

    def set_up(n):
        yield Op("set_tracers", (n,))
        for j in range(n):
            yield Op("tr_upload", (j, 1, "phi", vseed()))

    def ensure_tracers():
        if S.nT == 0:
            yield from set_up(cfg.nT)

    def ensure_tape(room=1, flags=None):
        t = S.tape
        if t and (t["cap"] - t["n"] < room or (flags is not None and (t["n"] > 0 or t["between"]))):
            yield Op("tr_tape_destroy")
        yield from ensure_tracers()
        if not S.tape:
            yield Op("tr_tape_create", (int(rng.integers(max(room, 1), 4)), (), ()))
        for j in (flags or ()):
            yield Op("want_vgrad", (j, 1))

    def finish_tape():
        yield Op("tr_seed", (vseed(),))
        yield Op("tr_sweep")
        t = S.tape
        rd = [Op("x_download", (j,)) for j in range(t["nT"])]
        for j in sorted(t["vfl"]):
            rd += [Op("v_density", (j, int(rng.integers(3)))), Op("v_gradient", (j,))]
        for i in rng.permutation(len(rd))[:4]:
            yield rd[int(i)]
        yield Op("v_density", (draw([j for j in range(t["nT"]) if j not in t["vfl"]] or [t["nT"]]), 0)) if rng.random() < 0.4 else None

    def scene_count_change():
        if S.tape:
            yield Op("tr_tape_destroy")
        if S.nT != cfg.nT:
            yield from set_up(cfg.nT)
        yield Op("kappaV", (draw(KV_PATTERNS[1:]),))
        yield a_vfield(on=True)
        if rng.random() < 0.5:
            yield a_step()
        yield from set_up(2)
        yield Op(draw(("kappaV_read", "has_vfield", "vfield_download")), (int(rng.integers(2)),))
        if rng.random() < 0.5:
            yield a_step()
            yield a_read(tr=True)
        yield from set_up(cfg.nT)
        yield Op(draw(("kappaV_read", "has_vfield")), (int(rng.integers(cfg.nT)),))
        yield Op("rk4", (1.0,))
        yield a_read(tr=True)
        yield a_read(tr=True)

    def scene_field_cycle():
        yield from ensure_tape(room=2, flags=[int(rng.integers(cfg.nT))] if rng.random() < 0.6 else None)
        yield Op("tr_taped", (1.0,))
        j = int(rng.integers(S.nT))
        if S.vf.get(j, "none") in ("A", "B"):
            yield Op("vfield", (j, "none"))
        yield a_vfield(j, on=True)
        yield Op("vfield", (j, "none"))
        yield a_vfield(j, on=True)
        yield Op("tr_taped", (1.0,))
        yield Op("tr_download", (j, 1))
        yield from finish_tape()

    def scene_kappav_between():
        yield from ensure_tape(room=2, flags=sorted({int(rng.integers(cfg.nT)) for _ in range(2)}))
        if rng.random() < 0.5:
            yield a_kappav()
        yield Op("tr_taped", (1.0,))
        yield Op("want_vgrad", (int(rng.integers(S.nT)), int(rng.integers(2)))) if rng.random() < 0.4 else None      # refused: a step is recorded
        yield a_kappav()
        yield Op("tr_taped", (0.0 if rng.random() < 0.15 else 1.0,))
        yield a_read(tr=True)
        yield from finish_tape()

    def scene_visc_between():
        yield from ensure_tracers()
        yield a_step()
        yield a_read(tr=True)
        if rng.random() < 0.8 or S.tape:
            yield Op("visc", (draw([p for p in VISC_OK if p != S.visc]),))
        else:
            yield Op("stress", (draw(("field", "zero", "none")),))
        if rng.random() < 0.3:
            yield Op("visc", (draw([p for p in VISC_OK if p != S.visc]),))
        yield a_step()
        yield a_read(tr=True)
        yield a_read(tr=False)

    def scene_run_dt0():
        """moka_run with dt == 0.0 while a vertical coefficient or the momentum pass is on: both passes are skipped."""
        yield from ensure_tracers()
        if not vert_on() or rng.random() < 0.3:
            yield a_kappav(True) if rng.random() < 0.5 else a_vfield(on=True)
        if not mom_on() and rng.random() < 0.5:
            yield Op("visc", (draw(VISC_OK[1:]),))
        yield Op("run", (1, 3, 0, 0.0))
        yield a_read(tr=True)
        yield a_read()

    def scene_upload():
        yield Op("upload", (draw(PROG), int(rng.integers(2)), vseed()))
        yield a_read(latest=True)
        if S.tape and rng.random() < 0.5:
            yield Op("set_tracers", (draw((2, cfg.nT)),))     # refused: the tape lives
            yield a_read()

    def scene_vertical():
        yield from ensure_tracers()
        yield a_kappav() if rng.random() < 0.5 else a_vfield()
        if len(cfg.variants) > 1 and rng.random() < 0.5:
            yield Op("variant", (draw([v for v in cfg.variants if v != S.variant]),))
        yield a_step()
        yield Op("tr_vmix_path") if rng.random() < 0.5 else None
        yield a_read(tr=True)
        yield a_read()

    def scene_tape():
        fl = sorted({int(rng.integers(cfg.nT)) for _ in range(int(rng.integers(0, 3)))})
        yield from ensure_tape(room=1, flags=fl)
        if fl and rng.random() < 0.4:
            yield Op("want_vgrad", (fl[0], 0))
        while S.tape["n"] < S.tape["cap"] and rng.random() < 0.75:
            yield Op("tr_taped", (1.0,))
            if rng.random() < 0.4:
                yield draw((a_kappav(), a_vfield(), Op("kappa", (draw(("zero", "some")),))))
        if S.tape["n"] >= S.tape["cap"] and rng.random() < 0.5:
            yield Op("tr_taped", (1.0,))                       # refused: full
        if S.tape["n"] == 0:
            yield Op("tr_taped", (1.0,))
        if rng.random() < 0.3:
            yield Op("tr_sweep")                               # refused: not seeded
        yield a_read()
        yield from finish_tape()
        if rng.random() < 0.5:
            yield Op("tr_tape_destroy")

    def a_refusal():
        c = [Op("kappaV", ("bad",)), Op("vfield", (int(rng.integers(S.nT)), "bad")), Op("fe", (0,))]
        if vert_on() or mom_on():
            c += [Op("rk4", (-1.0,)), Op("run", (1, 3, 0, -1.0))] * 2
            if S.tape and S.tape["n"] < S.tape["cap"]:
                c += [Op("tr_taped", (-1.0,))] * 4
        if S.tape:
            c += [Op("set_tracers", (draw((2, cfg.nT)),))] * 2
        return draw(c)

    def a_single():
        c = [("step", 4), ("kappaV", 2), ("vfield", 2), ("kappa", 1), ("visc", 2), ("tr_upload", 2), ("upload", 1.5), ("getter", 2),
             ("refusal", 3)]
        if not S.tape:
            c += [("stress", 1.5)]
        if len(cfg.variants) > 1:
            c += [("variant", 1.5)]
        name = draw([x[0] for x in c], [x[1] for x in c])
        if name == "step":
            return a_step()
        if name == "kappaV":
            return a_kappav()
        if name == "vfield":
            return a_vfield()
        if name == "kappa":
            return Op("kappa", (draw(("zero", "some")),))
        if name == "visc":
            return Op("visc", (draw([p for p in VISC_OK if p != S.visc]),))
        if name == "stress":
            return Op("stress", (draw([p for p in ("none", "zero", "field") if p != S.stress]),))
        if name == "tr_upload":
            return Op("tr_upload", (int(rng.integers(S.nT)), int(rng.integers(2)), "phi", vseed()))
        if name == "upload":
            return Op("upload", (draw(PROG), int(rng.integers(2)), vseed()))
        if name == "getter":
            g = draw(("vfield_download", "has_vfield", "kappaV_read", "tr_vmix_path", "visc_read"))
            return Op(g, (int(rng.integers(S.nT)),)) if g in ("vfield_download", "has_vfield", "kappaV_read") else Op(g)
        if name == "variant":
            return Op("variant", (draw([v for v in cfg.variants if v != S.variant]),))
        return a_refusal()

    scenes = [(scene_count_change, 2.5), (scene_field_cycle, 2.5), (scene_kappav_between, 2.5), (scene_visc_between, 3), (scene_vertical, 4),
              (scene_tape, 3), (scene_upload, 1.5), (scene_run_dt0, 1.2)]
    scene = set_up(cfg.nT)
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
        op = a_read() if r < 0.3 else None
        if op is None and r < 0.7:
            scene = draw([x[0] for x in scenes], [x[1] for x in scenes])()
            continue
        op = op or a_single()
        ops.append(op)
        accept(op)
    return ops[:cfg.nops]


class VTracerModel(cs.TracerModel):
    """Machine D on the twin stack, eagerly.  Mutants: D_MUTANTS."""

    def __init__(self, cfg, seed, mutant=None):
        import tracer_vfield_twin as tf
        import tracer_vmix_twin as tv
        assert mutant is None or mutant in D_MUTANTS
        super().__init__(cfg, seed, mutant if mutant in cs.B_MUTANTS else None)
        self.mutant, self.tf, self.tv = mutant, tf, tv
        mlt = d_mask_of(cfg)
        self.mlt = np.full(self.mesh.nEdges, cfg.K, dtype=np.int32) if mlt is None else mlt
        self.om = orc.OracleMesh(self.mesh, cfg.K, resting_thickness_sum=resting_thickness(cfg).sum(1), max_level_edge_top=self.mlt)
        self.twin = tf.VfieldTwin(self.om, self.om, [])
        self.nlev = self.twin.nlev(cfg.K)
        self.kappaV, self.fieldV = [], []
        self.mix = mv.MomentumVmixTwin(SimpleNamespace(om=self.om))
        self.stress = None
        self.vpath = 0
        self.variant = 0

    def _vcoeffs(self):
        n = self.nT
        return (list(self.kappaV) + [0.0] * n)[:n], (list(self.fieldV) + [None] * n)[:n]

    def vert_on(self):
        kv, fv = self._vcoeffs()
        return any((f is None and k != 0.0) or (f is not None and self.tf.field_on(f, self.nlev)) for k, f in zip(kv, fv))

    def mom_on(self):
        return mv.pass_on(self.mix.nu, self.mix.drag, self.mix.tau, self.mlt)

    def _step(self, dt, taped=False):
        st, tw, K = self.st, self.twin, self.cfg.K
        cur = self._coeffs() + self._vcoeffs()
        use = cur
        if self.mutant == "coeff_late":
            use = self.lag if self.lag is not None and len(self.lag[0]) == self.nT else cur
            self.lag = cur
        tw.kappa, tw.kappa4, tw.source, tw.kappaV, tw.fieldV = (list(x) for x in use)
        tw.base = self._base()
        kept = [[a.copy() for a in (st.ssh[0], st.u[0], st.h[0])], [p.copy() for p in self.phis[0]]] if self.mutant == "prev_level_lost" else None
        phi0 = [p.copy() for p in self.phis[1]]
        tw.step_rk4(st, self.phis, dt)
        rec = tw.tape.pop()
        self.pending = None
        kv, fv = use[3], use[4]
        if K >= 2 and dt != 0.0 and any((f is None and k != 0.0) or (f is not None and self.tf.field_on(f, self.nlev)) for k, f in zip(kv, fv)):
            self.vpath = 1 if self.tv.tile_columns(K, self.variant == 3) else 2
        if self.mom_on() and dt != 0.0:                    # tracers never see the pass inside a step: their stage 4 read the provisional flow
            st.u[1] = self.mix.mix(st.u[1], st.h[1], dt)
            if self.mutant == "mixed_flow_early":
                early = dict(rec, P=rec["P"][:3] + [(st.u[1].copy(), rec["P"][3][1])])
                for j in range(self.nT):
                    new = tw.replay(early, j, phi0[j])[1]
                    if K >= 2 and rec["fieldV"][j] is not None:
                        new = self.tf.apply_field(st.h[1], new, self.nlev, dt, rec["fieldV"][j])
                    elif K >= 2 and rec["kappaV"][j] != 0.0:
                        new = self.tv.apply(st.h[1], new, self.nlev, np.float64(dt) * np.float64(rec["kappaV"][j]))
                    self.phis[1][j] = new
        if kept is not None:
            st.ssh[0], st.u[0], st.h[0] = kept[0]
            if len(kept[1]) == self.nT:
                self.phis[0] = kept[1]
        self.ssh_loose = False
        if taped:
            self.tape["rec"].append(rec)

    def apply(self, op):
        cfg, k, a, t = self.cfg, op.kind, op.args, self.tape
        nT = self.nT
        R = lambda code, name: Obs(k, code, refusal=name)
        if k == "set_tracers":
            o = super().apply(op)
            if o.rc == OK:
                self.kappaV, self.fieldV = [], []          # moka_set_tracers resets every kappaV and frees every field
                self.vpath = 0                             # ... and puts moka_state_tracer_vmix_path back to 0
            return o
        if k == "kappaV":
            if a[0] == "bad":
                return R(ERR_ARG, "kappaV_invalid")
            v = kappav_values(cfg, a[0], nT)
            self.kappaV = [] if v is None else list(v)
            return Obs(k, OK)
        if k == "vfield":
            if a[1] == "bad":
                return R(ERR_ARG, "vfield_invalid")
            self.fieldV = (list(self.fieldV) + [None] * nT)[:nT]
            self.fieldV[a[0]] = vfield_values(cfg, a[1], a[0])
            return Obs(k, OK)
        if k == "vfield_download":
            f = self._vcoeffs()[1][a[0]]
            return Obs(k, OK, value=np.zeros(shape_of(cfg, F_H)) if f is None else f.copy())
        if k == "has_vfield":
            return Obs(k, OK, value=int(self._vcoeffs()[1][a[0]] is not None))
        if k == "kappaV_read":
            return Obs(k, OK, value=float(self._vcoeffs()[0][a[0]]))
        if k == "tr_vmix_path":
            return Obs(k, OK, value=self.vpath)
        if k == "visc":
            nu, r = visc_values(cfg, a[0])
            if not (nu >= 0.0 and r >= 0.0 and np.isfinite(nu) and np.isfinite(r)):
                return R(ERR_ARG, "visc_invalid")
            self.mix.nu, self.mix.drag = nu, r
            return Obs(k, OK)
        if k == "visc_read":
            return Obs(k, OK, value=(self.mix.nu, self.mix.drag))
        if k == "stress":
            self.stress = self.mix.tau = stress_values(cfg, a[0])
            return Obs(k, OK)
        if k == "variant":
            self.variant = a[0]
            return Obs(k, OK)
        if k in ("rk4", "run", "tr_taped"):
            dt = dt_of(cfg, a[3] if k == "run" else a[0])
            if k == "tr_taped":
                if len(t["rec"]) >= t["cap"]:
                    return R(ERR_ARG, "tape_full")
                if nT != t["nT"]:
                    return R(ERR_ARG, "taped_count_changed")
            if dt < 0.0 and (self.vert_on() or self.mom_on()):
                return R(ERR_ARG, "dt_negative_" + ("taped" if k == "tr_taped" else k))
            on = self.vert_on() or self.mom_on()
            for _ in range(a[1] if k == "run" else 1):
                self._step(dt, taped=k == "tr_taped")
            if k == "tr_taped":
                t["seeded"] = t["between"] = False
            o = Obs(k, OK, value=16 if k == "rk4" else None)
            o.info = dict(on=on, dt=dt)
            return o
        if k == "tr_tape_create":
            o = super().apply(op)
            self.tape.update(vfl=set(), D={}, between=False)
            return o
        if k == "want_vgrad":
            if t["rec"] or t["between"]:
                return R(ERR_ARG, "want_vgrad_recorded")
            before = set(t["vfl"])
            (t["vfl"].add if a[1] else t["vfl"].discard)(a[0])
            if t["vfl"] != before:
                t["D"] = {}                                # a changed set drops what earlier sweeps accumulated
            return Obs(k, OK)
        if k == "tr_seed":
            t["between"] = True
            return super().apply(op)
        if k == "tr_sweep":
            if not t["seeded"]:
                return R(ERR_ARG, "sweep_unseeded")
            recs = t["rec"]
            if self.mutant == "coeff_late":                # the coefficients in force now, not those recorded
                c = self._coeffs() + self._vcoeffs()
                on = [f is not None and self.tf.field_on(f, self.nlev) for f in c[4]]
                recs = [dict(r, kappa=list(c[0]), kappa4=list(c[1]), kappaV=[0.0 if f is not None else kk for kk, f in zip(c[3], c[4])],
                             fieldV=[f if o else None for f, o in zip(c[4], on)]) for r in recs]
            adj = self.tf.VfieldAdjointTwin(self.twin)
            t["X"], t["G"], t["W"], D = adj.sweep_vgrad(recs, [x.copy() for x in t["X"]], tuple(sorted(t["vfl"])), dict(t["kfl"]), tuple(t["want"]))
            t["D"] = D
            t["rec"], t["between"] = [], False
            return Obs(k, OK)
        if k in ("v_density", "v_gradient"):
            if a[0] >= t["nT"] or a[0] not in t["vfl"]:
                return R(ERR_ARG, "v_density_unflagged")
            import tracer_vgrad_twin as tg
            D = t["D"].get(a[0], np.zeros(shape_of(cfg, F_H)))
            cell, prof, scalar = tg.views(D)
            return Obs(k, OK, value=scalar if k == "v_gradient" else (D.copy(), cell, prof)[a[1]])
        return super().apply(op)

    def run(self, ops):
        out = []
        before = {key: self.array(key).copy() for key in self.keys()}
        self._last = dict(before)
        non_array = NON_ARRAY_OPS + ("kappaV", "vfield", "want_vgrad", "variant")
        for op in ops:
            o = self.apply(op)
            if op.kind in D_READS:
                if o.rc == OK:
                    o.fresh = o.key not in self._last or not np.array_equal(self._last[o.key], self.array(o.key))
                    o.after = frozenset(self._changed.get(o.key, ()))
                    self._changed[o.key] = set()
                    self._last[o.key] = self.array(o.key).copy()
            elif op.kind not in D_TAPE_READS + D_GETTERS:
                now = {key: self.array(key).copy() for key in self.keys()}
                for key, v in now.items():
                    if key not in before or not np.array_equal(before[key], v) or \
                            (o.rc == OK and op.kind in non_array and self._changed.get(key)):
                        self._changed.setdefault(key, set()).add(op.kind)
                before = now
            out.append(o)
        return out


class VTracerDevice:
    """Machine D through moka_hip.lib, in the form of call_sequences.TracerDevice: one mesh per config (here over the config's sea
    floor), a fresh state per sequence.  A HIP error ends the sequence and every later one of the config (`dead`)."""

    def __init__(self, backend, cfg):
        import moka_hip as mk
        from moka_hip import lib as L
        self.L, self.lib, self.backend, self.cfg = L, L.lib(), backend, cfg
        hm = mk.HorzMesh(get_mesh(cfg.meshname))
        vm = mk.VerticalMesh(hm, nVertLevels=cfg.K, restingThickness=resting_thickness(cfg), multilayer=True)
        mlt = d_mask_of(cfg)
        if mlt is not None:
            vm.maxLevelEdge.Top[:] = mlt
        self.M = mk.Mesh(hm, vm, backend=backend, patch_cells=cfg.patch_cells)
        self.counters = {"sequences": 0, "rk4_steps": 0, "tracer_paths": set(), "vpaths": set(), "adjoint_vpaths": set(), "vgrad_sweeps": 0}
        self.dead = None

    def close(self):
        self.M.close()

    def run(self, ops, seed):
        if self.dead:
            raise RuntimeError("an earlier sequence of this config ended in a HIP error, nothing more is launched: " + self.dead)
        L, lib, cfg, ctx = self.L, self.lib, self.cfg, self.backend._h
        cnt = self.counters
        hS, hT = C.c_void_p(), C.c_void_p()
        out, nT, tapeNT, flagged = [], 0, 0, set()
        vp = lambda arr: arr.ctypes.data_as(C.c_void_p)
        hfield = lambda: np.full(shape_of(cfg, F_H), np.nan)
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
                        nT = a[0]
                elif k == "tr_upload":
                    rc = lib.moka_tracer_upload(hS, a[0], a[1], vp(cs.tracer_values(cfg, a[2], a[3])))
                elif k == "tr_download":
                    value = hfield()
                    rc = lib.moka_tracer_download(hS, a[0], a[1], vp(value))
                elif k == "kappa":
                    v = cs.coefficients(cfg, "kappa", a[0], nT)
                    rc = lib.moka_set_tracer_diffusion(hS, None if v is None else vp(np.asarray(v, dtype=np.float64)))
                elif k == "kappaV":
                    v = [-1.0] * nT if a[0] == "bad" else kappav_values(cfg, a[0], nT)
                    rc = lib.moka_set_tracer_vertical_diffusion(hS, None if v is None else vp(np.asarray(v, dtype=np.float64)))
                elif k == "vfield":
                    f = -np.ones(shape_of(cfg, F_H)) if a[1] == "bad" else vfield_values(cfg, a[1], a[0])
                    rc = lib.moka_tracer_vertical_field_upload(hS, a[0], None if f is None else vp(f))
                elif k == "vfield_download":
                    value = hfield()
                    rc = lib.moka_tracer_vertical_field_download(hS, a[0], vp(value))
                elif k == "has_vfield":
                    v = C.c_int(-1)
                    rc = lib.moka_tracer_has_vertical_field(hS, a[0], C.byref(v))
                    value = v.value
                elif k == "kappaV_read":
                    s = C.c_double(np.nan)
                    rc = lib.moka_tracer_vertical_diffusion(hS, a[0], C.byref(s))
                    value = s.value
                elif k == "tr_vmix_path":
                    rc, value = OK, lib.moka_state_tracer_vmix_path(hS)
                elif k == "visc":
                    rc = lib.moka_set_vertical_viscosity(hS, *visc_values(cfg, a[0]))
                elif k == "visc_read":
                    nu, r = C.c_double(np.nan), C.c_double(np.nan)
                    rc = lib.moka_vertical_viscosity(hS, C.byref(nu), C.byref(r))
                    value = (nu.value, r.value)
                elif k == "stress":
                    tau = stress_values(cfg, a[0])
                    rc = lib.moka_surface_stress_upload(hS, None if tau is None else vp(tau))
                elif k == "variant":
                    rc = lib.moka_set_kernel_variant(ctx, a[0])
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
                    rc = lib.moka_tracer_tape_create(hS, a[0], C.byref(hT))
                    tapeNT, flagged = nT, set()
                elif k == "tr_tape_destroy":
                    lib.moka_tracer_tape_destroy(hT)
                    hT, rc = C.c_void_p(), OK
                elif k == "want_vgrad":
                    rc = lib.moka_tracer_adjoint_want_vertical_gradient(hT, a[0], a[1])
                    if rc == OK:
                        (flagged.add if a[1] else flagged.discard)(a[0])
                elif k == "tr_taped":
                    rc = lib.moka_step_rk4_tracer_taped(hT, dt_of(cfg, a[0]))
                elif k == "tr_seed":
                    rc = OK
                    for j in range(tapeNT):
                        rc = rc or lib.moka_tracer_adjoint_seed(hT, j, vp(cs.tracer_values(cfg, "seed", a[0] + 31 * j)))
                elif k == "tr_sweep":
                    rc = lib.moka_tracer_adjoint_sweep(hT)
                    if rc == OK:
                        cnt["adjoint_vpaths"].add(lib.moka_tracer_adjoint_vmix_path(hT))
                        cnt["vgrad_sweeps"] += bool(flagged)
                elif k == "x_download":
                    value = hfield()
                    rc = lib.moka_tracer_adjoint_download(hT, a[0], vp(value))
                elif k == "v_density":
                    value = np.full({0: shape_of(cfg, F_H), 1: shape_of(cfg, F_SSH), 2: (cfg.K,)}[a[1]], np.nan)
                    rc = lib.moka_tracer_adjoint_vertical_density_download(hT, a[0], a[1], vp(value))
                elif k == "v_gradient":
                    s = C.c_double(np.nan)
                    rc = lib.moka_tracer_adjoint_vertical_gradient(hT, a[0], C.byref(s))
                    value = s.value
                else:
                    raise ValueError(f"unknown op {op}")
                if rc == ERR_HIP:
                    self.dead = f"config {cfg.name} seed {seed}: HIP error at op {len(out)} ({op}): {lib.moka_last_error(ctx)}"
                    raise RuntimeError(self.dead)
                if rc == OK and k in D_STEPS and nT > 0:
                    cnt["rk4_steps"] += a[1] if k == "run" else 1
                    cnt["tracer_paths"].add(lib.moka_state_tracer_path(hS))
                    cnt["vpaths"].add(lib.moka_state_tracer_vmix_path(hS))
                out.append(Obs(k, int(rc), value=value if rc == OK else None))
            cnt["sequences"] += 1
        finally:
            first, second = ((hT, lib.moka_tracer_tape_destroy), (hS, lib.moka_state_destroy))[::1 if seed % 2 else -1]
            for h, fn in (first, second):
                if h and not self.dead:    # after a HIP error nothing more is sent to the device, the destroy calls included
                    fn(h)
            lib.moka_set_kernel_variant(ctx, 0)
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
        print(f"usage: call_sequences_vertical.py CONFIG SEED [--upto N]   (CONFIG: {' '.join(ALL_CONFIGS)})")
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
