"""Seeded call sequences through the C ABI: vocabulary, generator, host model, device runner.

Every kernel is pinned bit for bit elsewhere; what this module pins is the ORDER of calls.  Between the caller and the kernels sits a
state machine (csrc/api.hip, csrc/state.hpp: lazily pending DiagnosticVars / TendencyVars of lean Forward-Euler and of RK4 steps, the
stale-thickness shortcut, the ssh consistency flag, three or four rotating buffer sets, tapes that own rows of pending tendencies).
The header's contract is that every array reads as if each step had stored everything at once.  `sequence(config, seed)` draws about
thirty public calls; `Model.run` executes them on the CPU oracle EAGERLY, exactly as include/moka_hip.h words each call; `Device.run`
executes them through moka_hip.lib.  An observation is an array, a scalar or a status code -- a refusal the header states is one too --
and every observation is compared bit for bit (tests/test_gpu_call_sequences.py).  tests/test_call_sequences.py checks on the model
alone that the frozen sequences look where they should (vocabulary, first reads after writes, refusals, mutants).

Machine A, the dycore (configs A1-A6): Forward Euler, RK4 in both forms, moka_run, the fused and the piecewise tendencies, uploads
and the three kinds of reads, placement, kernel variants, tuning keys 4 / 8 / 9 (and 7 around single RK4 steps), the nonlinear / Del2
/ Del4 toggles (Del4 with and without meshScalingDel4) and the Forward-Euler / RK4 tapes.  Machine B, passive tracers (configs B1,
B2): moka_set_tracers with a changing count, 0 included (the dycore then steps alone, also under key 7), tracer and dycore uploads,
diffusivities, biharmonic coefficients and sources that come and go, RK4 / moka_run / advanceTimeLevels!, the nonlinear / Del2 /
Del4 toggles, placement, reads of TendencyVars, and the tracer tape with its source and diffusivity gradients, coefficients and
sources changing between taped steps.  Machines C and D live in tests/call_sequences_vertical.py, on this module's Op, Obs, Model,
TracerModel and TracerDevice: C, the forced dycore (configs C1-C4: moka_set_vertical_viscosity, moka_surface_stress_upload and
their getters, the pass in RK4 steps and in moka_run's captured graph, Forward Euler behind a mixed step, moka_tape against the
pass, every call of moka_forced_tape); D, tracers with the vertical passes (D1, D2: moka_set_tracer_vertical_diffusion, the
moka_tracer_vertical_field_* calls and moka_tracer_adjoint_want_vertical_gradient with its views, beside a changing tracer count
and the momentum pass).  Not covered by any machine: a tracer count that changes under a live tracer tape, halos and partitions
(several processes) -- their call order stays with test_partition_gloo.py; level masks and poisoned levels on a partition have a
file of their own, test_gpu_partition_masks.py (cases and CPU emulation: partition_cases.py, test_partition_masks.py).

Replay a sequence on the CPU:   python tests/call_sequences.py A1 3 [--upto N]

This module imports no GPU code when it is imported (moka_hip.lib is loaded by Device only)."""
import ctypes as C
import os
import sys
import zlib
from dataclasses import dataclass

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(_ROOT, "mpas-ocean.jl_amd"), os.path.join(_ROOT, "oracle"), os.path.join(_ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import oracle as orc  # noqa: E402
from masks import basin  # noqa: E402
from moka_hip import lib as _L  # noqa: E402  (constants only: the shared library is loaded by Device)
from moka_hip import meshgen as mg  # noqa: E402

OK, ERR_ARG, ERR_UNSUPPORTED = _L.OK, _L.ERR_ARG, _L.ERR_UNSUPPORTED
FIELD_NAMES = ("ssh", "normalVelocity", "layerThickness", "layerThicknessEdge", "thicknessFlux", "velocityDivCell",
               "relativeVorticity", "tendNormalVelocity", "tendLayerThickness")
(F_SSH, F_U, F_H, F_HEDGE, F_FLUX, F_DIV, F_VORT, F_TENDU, F_TENDH) = (
    _L.F_SSH, _L.F_NORMAL_VELOCITY, _L.F_LAYER_THICKNESS, _L.F_LAYER_THICKNESS_EDGE, _L.F_THICKNESS_FLUX, _L.F_VELOCITY_DIV_CELL,
    _L.F_RELATIVE_VORTICITY, _L.F_TEND_NORMAL_VELOCITY, _L.F_TEND_LAYER_THICKNESS)      # moka_field, from the binding's table
PROG, DIAG, TEND = (F_SSH, F_U, F_H), (F_HEDGE, F_FLUX, F_DIV, F_VORT), (F_TENDU, F_TENDH)
STATE_KEYS = tuple((f, l) for f in PROG for l in (0, 1)) + tuple((f, 1) for f in DIAG + TEND)
ADJ_KEYS = tuple(("adj", f) for f in (F_SSH, F_U, F_H, F_HEDGE))
FE_STALE, FE_ACCUM, FE_LEVEL1 = 1, 2, 4
PAIR_DEFAULT = 0b10000011           # moka_set_tuning key 8: the documented default mask (modes 0, 1, 7); 0 is the other documented one
TUNING_VALUES = {4: (0, 1), 9: (0, 1), 8: (0, PAIR_DEFAULT)}
VARIANTS = (0, 3, 4, 11)
MUTANTS = ("late", "stale_from_prev", "ssh_stored", "prev_level_lost")


def key_name(key):
    if key[0] in ("tr", "X", "G", "W"):
        return {"tr": "tracer", "X": "tracer adjoint", "G": "source gradient of tracer", "W": "diffusivity gradient of tracer"}[key[0]] + \
            " " + " ".join(str(x) for x in key[1:])
    if key[0] == "adj":
        return "adjoint of " + FIELD_NAMES[key[1]]
    f, l = key
    return FIELD_NAMES[f] + (f"[level {l}]" if f in PROG else "")


# ---------------------------------------------------------------------------------------------------------------------------------
# configs: the smallest shapes at which the dispatch still differs
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Config:
    name: str
    meshname: str
    K: int
    sbytes: int = 8
    mask: str = ""                 # "basin": poison_cases.basin
    dt: float = 20.0
    s13: bool = False              # moka_state_rk4_streams answers 13 under key 7 with the default kernel choice (even 34 <= K <= 64)
    reach: tuple = ()              # what the device counters must show (tests/test_gpu_call_sequences.py)
    nops: int = 30

    @property
    def f32(self):
        return self.sbytes == 4


CONFIGS = {c.name: c for c in (
    Config("A1", "ico4", 34, s13=True, reach=("lean", "fe_path_1", "fe_path_2", "s13")),
    Config("A2", "hex6x4", 60, mask="basin", dt=2.0, s13=True, reach=("lean", "fe_path_1", "fe_path_2", "s13")),
    Config("A3", "ico4f", 5, reach=("fe_path_0",)),
    Config("A4", "hex4x4", 1, dt=2.0, reach=("fe_path_0",)),
    Config("A5", "ico4", 40, sbytes=4, reach=("lean", "fe_path_1", "fe_path_2")),
    Config("A6", "hex4x6", 4, sbytes=4, dt=2.0, reach=("fe_path_1",)),
)}
_MESHES = {}


def get_mesh(name):
    if name not in _MESHES:
        if name == "planar":                                 # the tracer files' mesh, from where they keep it
            import tracer_cases
            _MESHES[name] = tracer_cases.get_mesh("planar")
            return _MESHES[name]
        _MESHES[name] = {
"ico6f": lambda: mg.icosahedral_mesh(6, flips=3, seed=4),        # 362 cells, heptagons
                         "ico4": lambda: mg.icosahedral_mesh(4),
                         "ico4f": lambda: mg.icosahedral_mesh(4, flips=2, seed=4),      # four heptagons: maxEdges 7
                         "hex6x4": lambda: mg.planar_hex_mesh(6, 4, 1000.0, f0=1e-4),
                         "hex4x4": lambda: mg.planar_hex_mesh(4, 4, 1000.0, f0=1e-4),
                         "hex4x6": lambda: mg.planar_hex_mesh(4, 6, 1000.0, f0=1e-4)}[name]()
    return _MESHES[name]


def mask_of(cfg):
    return basin(get_mesh(cfg.meshname), cfg.K) if cfg.mask == "basin" else None


def resting_thickness(cfg):
    """Belongs to the mesh (restingThicknessSum), so it is the config's, not the sequence's."""
    mesh = get_mesh(cfg.meshname)
    rng = np.random.default_rng([77, cfg.K, mesh.nCells])
    return np.full((mesh.nCells, cfg.K), 1000.0 / cfg.K) + rng.uniform(0, 0.1, (mesh.nCells, cfg.K))


def shape_of(cfg, f):
    mesh = get_mesh(cfg.meshname)
    n = {F_SSH: mesh.nCells, F_U: mesh.nEdges, F_H: mesh.nCells, F_HEDGE: mesh.nEdges, F_FLUX: mesh.nEdges, F_DIV: mesh.nCells,
         F_VORT: mesh.nVertices, F_TENDU: mesh.nEdges, F_TENDH: mesh.nCells}[f]
    return (n,) if f == F_SSH else (n, cfg.K)


def values(cfg, f, vseed):
    """What an upload of field f carries: drawn fresh from vseed, fp32-representable for an fp32-storage state (the way the existing
    tests round).  ssh is NOT the column sum of any layerThickness; layerThickness stays positive."""
    rng = np.random.default_rng([cfg.K, f, vseed])
    shp = shape_of(cfg, f)
    if f == F_H:
        a = resting_thickness(cfg) + rng.uniform(-1, 1, shp)
    elif f == F_HEDGE:
        a = 1000.0 / cfg.K + rng.uniform(-1, 1, shp)
    elif f in (F_DIV, F_VORT, F_TENDH):
        a = rng.uniform(-1e-3, 1e-3, shp)
    else:
        a = rng.uniform(-1, 1, shp)
    if cfg.f32:
        a = a.astype(np.float32).astype(np.float64)
    return np.ascontiguousarray(a)


def visc_del2(cfg):
    """The Del2 viscosity the toggle switches on: 0.01 dcEdge_min^2 / dt, as the other files choose it."""
    return 0.01 * float(get_mesh(cfg.meshname).dcEdge.min()) ** 2 / cfg.dt


def initial_state(cfg, seed):
    """Both time levels of the three prognostic fields, uploaded before the first op (level 0 differs from level 1)."""
    return {(f, l): values(cfg, f, 1000003 * (seed + 1) + 10 * f + l) for f in PROG for l in (0, 1)}


# ---------------------------------------------------------------------------------------------------------------------------------
# ops
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Op:
    kind: str
    args: tuple = ()

    def __str__(self):
        return self.kind + (str(self.args) if self.args else "")


# kinds that observe an array or a scalar of the state / the kinds that may change what a later read sees
READ_KINDS = ("download", "rows", "sumsq")
STEP_KINDS = ("fe", "rk4", "rk4_s13", "run", "fe_taped", "rk4_taped")


def vocabulary(cfg):
    """Every op kind the config admits."""
    v = ["fe", "rk4", "run", "tend", "advance", "upload", "download", "rows", "sumsq", "placement", "variant", "tuning"]
    if cfg.f32:
        return tuple(v + list(REFUSED_F32))
    v += ["rk4_s13", "diag", "tendU", "tendH", "nonlinear", "del2", "del4",
          "tape_create", "fe_taped", "rk4_taped", "seed", "sweep", "adj_download", "tape_destroy"]
    return tuple(v)


REFUSED_F32 = ("diag", "tendU", "tendH", "nonlinear", "tape_create")       # an fp32-storage state admits these only to refuse them


def writers(cfg):
    """The kinds that count as state-changing for the read-after-write table: everything but the reads (and what is only refused)."""
    return tuple(k for k in vocabulary(cfg) if k not in READ_KINDS + ("adj_download",) and not (cfg.f32 and k in REFUSED_F32))


def refusals(cfg):
    """The refusals include/moka_hip.h states that this config's vocabulary can provoke."""
    if cfg.f32:
        r = ["piecewise_f32", "diag_after_rk4", "fe_carry_after_rk4", "fe_level1_f32", "tape_f32", "nonlinear_f32", "variant_gone"]
        return tuple(r + (["advance_level1"] if cfg.K > 1 else []))
    r = ["fe_nonlinear", "piecewise_nonlinear", "tape_nonlinear", "nonlinear_tape", "placement_tape", "mix_integrators", "tape_full",
         "del2_without_nonlinear", "del4_without_nonlinear", "variant_gone"]
    return tuple(r + (["advance_level1", "taped_level1"] if cfg.K > 1 else []))


# ops that change no array but may fall between a change of one and its first read: they count for the read-after-write table
NON_ARRAY_OPS = ("tuning", "variant", "placement", "nonlinear", "del2", "del4", "tape_create", "tape_destroy", "seed", "sweep",
                 "kappa", "kappa4", "source", "tr_tape_create", "tr_seed", "tr_sweep")


def arg_class(op):
    """The argument class of an op for the vocabulary table (None: the kind alone)."""
    k, a = op.kind, op.args
    if k in ("upload", "tr_upload"):
        return (k, a[0], a[1]) if k == "upload" else (k, a[1])
    if k in ("variant", "placement", "fe", "set_tracers", "del4", "kappa", "kappa4"):
        return (k, a[0])
    if k == "tuning":
        return (k, a[0], a[1])
    if k == "run":
        return (k, a[0])
    if k == "source":
        return (k, a[1])
    return None


def arg_classes(cfg):
    """Every (kind, argument class) the config admits with status MOKA_OK."""
    if isinstance(cfg, TracerConfig):
        c = [("upload", f, l) for f in PROG for l in (0, 1)] + [("tr_upload", l) for l in (0, 1)]
        c += [("set_tracers", n) for n in (0, 2, cfg.nT)] + [(k, p) for k in ("kappa", "kappa4") for p in ("zero", "some", "other")]
        c += [("source", m) for m in ("source", "zero", "none")] + [("del4", m) for m in (0, 1, 2)] + [("placement", n) for n in (0, 1, 2)]
        return tuple(c + [("run", 1)])
    c = [("upload",) + k for k in STATE_KEYS] + [("variant", v) for v in VARIANTS]
    c += [("tuning", k, v) for k in TUNING_VALUES for v in TUNING_VALUES[k]] + [("placement", n) for n in (0, 1, 2)]
    c += [("run", 0), ("run", 1)] + [("fe", fl) for fl in range(8 if cfg.K == 1 else 4)]
    if not cfg.f32:
        c += [("del4", m) for m in (0, 1, 2)]
    return tuple(c)


def visc_del4(cfg):
    """The Del4 viscosity the toggle switches on: 0.002 dcEdge_min^4 / dt, as the other files choose it."""
    return 0.002 * float(get_mesh(cfg.meshname).dcEdge.min()) ** 4 / cfg.dt


def del4_scaling(cfg):
    """meshScalingDel4 of mode 2: one factor per edge in [0.5, 1.5]."""
    return np.random.default_rng([cfg.K, 4444]).uniform(0.5, 1.5, get_mesh(cfg.meshname).nEdges)


def destroys_tape_with_tendencies_pending(ops, obs):
    """A taped RK4 step, then nothing that reads or overwrites TendencyVars, then moka_tape_destroy, then a read of TendencyVars."""
    state = 0
    for op, o in zip(ops, obs):
        if o.rc != OK:
            continue
        k = op.kind
        if k == "rk4_taped":
            state = 1
        elif state == 1 and k == "tape_destroy":
            state = 2
        elif k in READ_KINDS and op.args[0] in TEND:
            if state == 2:
                return True
            state = 0
        elif k in READ_KINDS or k in ("adj_download", "seed", "sweep", "variant", "tuning"):
            pass
        else:
            state = 0
    return False


def reads_tendencies_behind_a_sweep(ops, obs):
    """moka_adjoint_sweep, then (with no step in between) a read of TendencyVars."""
    swept = False
    for op, o in zip(ops, obs):
        if o.rc != OK:
            continue
        if op.kind == "sweep":
            swept = True
        elif op.kind in STEP_KINDS + ("tend", "tendU", "tendH"):
            swept = False
        elif swept and op.kind in READ_KINDS and op.args[0] in TEND:
            return True
    return False


def steps_the_dycore_without_tracers(ops, obs):
    """moka_set_tracers(st, 0), then a step, then a read, all accepted, before tracers come back."""
    state = 0
    for op, o in zip(ops, obs):
        if o.rc != OK:
            continue
        if op.kind == "set_tracers":
            state = 1 if op.args[0] == 0 else 0
        elif state >= 1 and op.kind in ("rk4", "rk4_s13", "run"):
            state = 2
        elif state == 2 and op.kind in READ_KINDS:
            return True
    return False


def pairs_wanted(cfg):
    """The ordered pairs (state-changing op kind, observing op kind) the frozen sequences of a config must show."""
    if isinstance(cfg, TracerConfig):
        p = {(w, "tr_download") for w in ("set_tracers", "tr_upload", "rk4", "rk4_s13", "run", "advance", "tr_taped", "kappa", "kappa4",
                                          "source", "nonlinear", "del2", "del4", "placement", "tr_tape_create", "tr_seed", "tr_sweep")}
        return p | {(w, r) for w in ("upload", "rk4", "run", "advance", "tr_taped") for r in READ_KINDS}
    p = {(w, r) for w in writers(cfg) for r in READ_KINDS}
    return p if cfg.f32 else p | {("seed", "adj_download"), ("sweep", "adj_download")}


def cases_wanted(cfg):
    """Orders of calls that must not depend on luck: named predicates over a sequence."""
    if isinstance(cfg, TracerConfig):
        return ("tracers_zero", "kappa_between", "kappa4_between", "source_between")
    return () if cfg.f32 else ("destroy_pending", "tend_after_sweep")


def cases_seen(cfg, ops, obs):
    if isinstance(cfg, TracerConfig):
        seen = {k + "_between" for k in ("kappa", "kappa4", "source") if changes_between_taped_tracer_steps(ops, obs, k)}
        return seen | ({"tracers_zero"} if steps_the_dycore_without_tracers(ops, obs) else set())
    seen = {"destroy_pending"} if destroys_tape_with_tendencies_pending(ops, obs) else set()
    return seen | ({"tend_after_sweep"} if reads_tendencies_behind_a_sweep(ops, obs) else set())


def changes_between_taped_tracer_steps(ops, obs, kind):
    """Two recorded tracer steps with an accepted `kind` op (kappa, kappa4, source) between them and no sweep."""
    state = 0
    for op, o in zip(ops, obs):
        if o.rc != OK:
            continue
        if op.kind == "tr_taped":
            if state == 2:
                return True
            state = 1
        elif op.kind == kind and state >= 1:
            state = 2
        elif op.kind in ("tr_sweep", "tr_tape_destroy", "tr_tape_create"):
            state = 0
    return False


# ---------------------------------------------------------------------------------------------------------------------------------
# generator: a pure function of (config, seed)
# ---------------------------------------------------------------------------------------------------------------------------------
class _Abstract:
    """Just enough abstract state to weight useful choices: a symbolic identity per array (so that the generator reads what has
    changed since its last read), whether a tape is open, whether the state is nonlinear."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.n = 0
        self.ids = {k: ("init", k) for k in STATE_KEYS + ADJ_KEYS}
        self.read = {k: ("init", k) for k in STATE_KEYS + ADJ_KEYS}     # (the uploads before the first op are not worth a read)
        self.recent = []               # keys in the order they last changed
        self.nonlinear, self.visc, self.visc4 = False, 0.0, 0
        self.tape = None               # dict(cap, n, kind, seeded)
        self.diag_gone = False         # fp32 storage after an RK4 step
        self.variant = 0

    def fresh(self):
        self.n += 1
        return ("v", self.n)

    def set(self, key, ident):
        if self.ids[key] != ident:
            self.ids[key] = ident
            if key in self.recent:
                self.recent.remove(key)
            self.recent.append(key)

    def readable(self):
        out = [k for k in self.recent if k[0] != "adj" and self.read.get(k) != self.ids[k]]
        if self.diag_gone:
            out = [k for k in out if k[0] not in DIAG]
        return out

    def rotate(self):
        for f in PROG:
            self.set((f, 0), self.ids[(f, 1)])

    def step_fe(self, flags):
        u, h = self.ids[(F_U, 1)], self.ids[(F_H, 1)]
        hE_used = self.ids[(F_HEDGE, 1)] if flags & FE_STALE else ("interp", h)
        self.rotate()
        self.set((F_HEDGE, 1), ("interp", h))
        self.set((F_FLUX, 1), ("F", u, hE_used))
        self.set((F_DIV, 1), ("div", u))
        self.set((F_VORT, 1), self.fresh() if flags & FE_ACCUM else ("curl", u))
        # the step's tendencies are those of the level it started from: the bits a fused or piecewise evaluation there left
        self.set((F_TENDU, 1), ("tendU", self.ids[(F_SSH, 0)], u, None, (False, 0.0)))
        self.set((F_TENDH, 1), ("tendH", ("F", u, hE_used)))
        for f in (F_U, F_H):
            self.set((f, 1), self.fresh())
        self.set((F_SSH, 1), ("ssh", self.ids[(F_H, 1)]))
        self.diag_gone = False

    def step_rk4(self):
        self.rotate()
        for f in (F_U, F_H, F_TENDU, F_TENDH):
            self.set((f, 1), self.fresh())
        u, h = self.ids[(F_U, 1)], self.ids[(F_H, 1)]
        self.set((F_SSH, 1), ("ssh", h))
        if self.cfg.f32:
            self.diag_gone = True
            return
        self.set((F_HEDGE, 1), ("interp", h))
        self.set((F_FLUX, 1), ("F", u, ("interp", h)))
        self.set((F_DIV, 1), ("div", u))
        self.set((F_VORT, 1), ("curl", u))

    def tend(self):
        u, h = self.ids[(F_U, 1)], self.ids[(F_H, 1)]
        mode = (self.nonlinear, self.visc, self.visc4)
        self.set((F_SSH, 1), ("ssh", h))
        self.set((F_TENDU, 1), ("tendU", ("ssh", h), u, h if self.nonlinear else None, mode))
        self.set((F_TENDH, 1), ("tendH", ("F", u, ("interp", h))))

    def diag(self, flags):
        u, h = self.ids[(F_U, 1)], self.ids[(F_H, 1)]
        hE_used = self.ids[(F_HEDGE, 1)] if flags & FE_STALE else ("interp", h)
        self.set((F_FLUX, 1), ("F", u, hE_used))
        self.set((F_HEDGE, 1), ("interp", h))
        self.set((F_DIV, 1), ("div", u))
        self.set((F_VORT, 1), self.fresh() if flags & FE_ACCUM else ("curl", u))


def sequence(cfg, seed):
    """The ops of (cfg, seed): machine A below, machine B in sequence_b."""
    return sequence_b(cfg, seed) if isinstance(cfg, TracerConfig) else sequence_a(cfg, seed)


def model_of(cfg, seed, mutant=None):
    return (TracerModel if isinstance(cfg, TracerConfig) else Model)(cfg, seed, mutant)


def device_of(backend, cfg):
    return (TracerDevice if isinstance(cfg, TracerConfig) else Device)(backend, cfg)


def sequence_a(cfg, seed):
    """About cfg.nops ops, a pure function of (cfg, seed).  The weights favour the wanted pattern: a step, then something that
    mutates an input of what the step left pending (or moves the state machine), then a read of it."""
    rng = np.random.default_rng([zlib_crc(cfg.name), seed])
    ab = _Abstract(cfg)
    K, f32 = cfg.K, cfg.f32
    ops, plan = [], []
    vseed = [0]

    def draw(items, weights=None):
        if weights is None:
            return items[int(rng.integers(len(items)))]
        w = np.asarray(weights, dtype=np.float64)
        return items[int(rng.choice(len(items), p=w / w.sum()))]

    def fe_flags():
        return int(rng.integers(0, 8 if K == 1 else 4))

    def emit(op):
        """Append op and advance the abstract state as the header says the call behaves (refusals change nothing)."""
        ops.append(op)
        k, a = op.kind, op.args
        t = ab.tape
        if k == "fe" or k == "fe_taped":
            flags = a[0]
            if ab.nonlinear or (f32 and (flags & FE_LEVEL1 or (ab.diag_gone and flags & 3))):
                return
            if k == "fe_taped":
                if t["n"] >= t["cap"] or (flags & FE_LEVEL1 and K != 1) or (t["n"] > 0 and t["kind"] != 0):
                    return
                t["n"] += 1; t["kind"] = 0; t["seeded"] = False
            ab.step_fe(flags)
        elif k in ("rk4", "rk4_s13", "rk4_taped"):
            if k == "rk4_taped":
                if t["n"] >= t["cap"] or (t["n"] > 0 and t["kind"] != 1):
                    return
                t["n"] += 1; t["kind"] = 1; t["seeded"] = False
            ab.step_rk4()
        elif k == "run":
            integ, n, flags = a
            if integ == 0 and (ab.nonlinear or (f32 and (flags & FE_LEVEL1 or (ab.diag_gone and flags & 3)))):
                return
            for _ in range(n):
                ab.step_fe(flags) if integ == 0 else ab.step_rk4()
        elif k == "tend":
            ab.tend()
        elif k == "advance":
            if not (a[0] & FE_LEVEL1 and K > 1):
                ab.rotate()
        elif k == "diag":
            if not ab.nonlinear and not f32:
                ab.diag(a[0])
        elif k == "tendU":
            if not ab.nonlinear and not f32:
                ab.set((F_TENDU, 1), ("tendU", ab.ids[(F_SSH, 1)], ab.ids[(F_U, 1)], None, (False, 0.0)))
        elif k == "tendH":
            if not ab.nonlinear and not f32:
                ab.set((F_TENDH, 1), ("tendH", ab.ids[(F_FLUX, 1)]))
        elif k == "upload":
            if not (ab.diag_gone and a[0] in DIAG):
                ab.set((a[0], a[1]), ab.fresh())
        elif k in READ_KINDS:
            if not (ab.diag_gone and a[0] in DIAG):
                ab.read[(a[0], a[1])] = ab.ids[(a[0], a[1])]
        elif k == "variant":
            if a[0] in VARIANTS:
                ab.variant = a[0]
        elif k == "nonlinear":
            if not (a[0] and (f32 or ab.tape)):
                ab.nonlinear = bool(a[0])
        elif k == "del2":
            if ab.nonlinear or not a[0]:
                ab.visc = a[0]
        elif k == "del4":
            if ab.nonlinear or not a[0]:
                ab.visc4 = a[0]
        elif k == "tape_create":
            if not f32 and not ab.nonlinear:
                ab.tape = dict(cap=a[0], n=0, kind=None, seeded=False)
        elif k == "tape_destroy":
            ab.tape = None
            for key in ADJ_KEYS:
                ab.ids[key] = ab.read[key] = ("init", key)
        elif k == "seed":
            t["seeded"] = True
            for key in ADJ_KEYS:
                ab.set(key, ab.fresh() if key[1] == (F_SSH if t["kind"] == 0 else F_H) else ("zero",))
        elif k == "sweep":
            if t["n"] > 0:
                for key in ADJ_KEYS:
                    live = key[1] in (F_U, F_H) or t["kind"] == 0
                    ab.set(key, ab.fresh() if live else ("zero",))
            t["n"] = 0
        elif k == "adj_download":
            ab.read[("adj", a[0])] = ab.ids[("adj", a[0])]

    def a_read(key=None):
        cand = ab.readable()
        if key is None:
            if not cand:
                return None
            # the most recent changes first: read soon after writing
            w = [2.0 ** min(i - len(cand), 0) for i in range(1, len(cand) + 1)]
            key = draw(cand, w)
        kind = draw(READ_KINDS)
        if kind == "rows":
            n = shape_of(cfg, key[0])[0]
            rows = tuple(int(r) for r in rng.integers(0, n, int(rng.integers(1, 6))))
            if len(rows) > 1 and rng.random() < 0.5:
                rows = rows + (rows[0],)                       # a repeat
            return Op("rows", (key[0], key[1], rows))
        return Op(kind, key)

    def an_upload(keys):
        f, l = draw(keys)
        vseed[0] += 1
        return Op("upload", (f, l, 7919 * (seed + 1) + vseed[0]))

    def a_mutator():
        """Something between a step and the read of what it left pending."""
        c = [("upload_prog", 5), ("advance", 2), ("variant", 2), ("tuning", 2), ("placement", 1.5), ("tend", 1)]
        if not f32:
            c += [("nonlinear", 1.5), ("del2", 1), ("del4", 1.2)]
            if ab.tape:
                c += [("tape_destroy", 1.5)]
        name = draw([x[0] for x in c], [x[1] for x in c])
        if name == "upload_prog":
            return an_upload([(f, l) for f in PROG for l in (0, 1)])
        if name == "advance":
            return Op("advance", (0,))
        if name == "variant":
            return Op("variant", (draw([v for v in VARIANTS if v != ab.variant]),))
        if name == "tuning":
            key = draw((4, 9, 8))
            return Op("tuning", (key, draw(TUNING_VALUES[key])))
        if name == "placement":
            return Op("placement", (int(rng.integers(0, 3)),))
        if name == "tend":
            return Op("tend")
        if name == "nonlinear":
            return Op("nonlinear", (0 if ab.nonlinear else 1,)) if not ab.tape else Op("tend")
        if name == "del2":
            return Op("del2", (0 if ab.visc else 1,)) if ab.nonlinear else Op("tend")
        if name == "del4":
            return Op("del4", (0 if ab.visc4 else int(rng.integers(1, 3)),)) if ab.nonlinear else Op("tend")
        return Op("tape_destroy")

    def a_refusal(tape_only=False):
        """A call the header refuses in the present state (tape_only: one of an open tape's, None when none applies)."""
        c = []
        t = ab.tape
        if tape_only:
            if t["n"] >= t["cap"]:
                c += [Op("fe_taped", (0,)) if t["kind"] == 0 else Op("rk4_taped")]
            elif t["n"] > 0:
                c += [Op("rk4_taped") if t["kind"] == 0 else Op("fe_taped", (0,))]
            if K > 1 and t["n"] < t["cap"] and (t["n"] == 0 or t["kind"] == 0):
                c += [Op("fe_taped", (4 + int(rng.integers(0, 4)),))]
            return draw(c) if c else None
        if f32:
            c += [Op(draw(("diag", "tendU", "tendH")), (0,)), Op("fe", (4 + int(rng.integers(0, 4)),)), Op("tape_create", (2,)),
                  Op("nonlinear", (1,))]
            if ab.diag_gone:
                c += [Op(draw(READ_KINDS[::2]), (draw(DIAG), 1)), Op("fe", (int(rng.integers(1, 4)),))] * 2
        else:
            if ab.nonlinear:
                c += [Op("fe", (fe_flags(),)), Op(draw(("diag", "tendU", "tendH")), (0,))] * 2
                if not t:
                    c += [Op("tape_create", (2,))] * 2
            else:
                c += [Op("del2", (1,)), Op("del4", (int(rng.integers(1, 3)),))]
            if t:
                c += [Op("placement", (1,))] * 2
                if not ab.nonlinear:
                    c += [Op("nonlinear", (1,))] * 2
                if t["n"] >= t["cap"]:
                    c += [Op("fe_taped" if t["kind"] == 0 else "rk4_taped", (0,) if t["kind"] == 0 else ())] * 3
                elif t["n"] > 0:
                    c += [Op("rk4_taped") if t["kind"] == 0 else Op("fe_taped", (0,))] * 3
                if K > 1 and t["n"] < t["cap"] and (t["n"] == 0 or t["kind"] == 0):
                    c += [Op("fe_taped", (4 + int(rng.integers(0, 4)),))] * 2
        if K > 1:
            c += [Op("advance", (4,))]
        c += [Op("variant", (draw((1, 2, 5, 9, 12)),))]
        return draw(c)

    def a_writer():
        t = ab.tape
        c = [("fe", 5), ("rk4", 4), ("run", 2), ("tend", 1.5), ("advance", 1), ("upload", 5), ("mutator", 4), ("refusal", 2.5)]
        if not f32:
            c += [("rk4_s13", 2), ("diag", 1.2), ("tendU", 1), ("tendH", 1)]
            c += [("tape", 14)] if t else [("tape_create", 2.5)]
        name = draw([x[0] for x in c], [x[1] for x in c])
        if ab.nonlinear and name in ("fe", "diag", "tendU", "tendH", "rk4_s13", "tape_create", "tape"):
            name = draw(("rk4", "tend", "mutator", "run", "refusal", "mixing"))
        if name == "mixing":
            if rng.random() < 0.6:
                return Op("del4", (0 if ab.visc4 else int(rng.integers(1, 3)),))
            return Op("del2", (0 if ab.visc else 1,))
        if f32 and ab.diag_gone and name == "fe":
            return Op("fe", (0,))
        if name == "fe":
            return Op("fe", (fe_flags(),))
        if name in ("rk4", "rk4_s13", "tend"):
            return Op(name)
        if name == "run":
            integ = 1 if ab.nonlinear else int(rng.integers(0, 2))
            flags = 0 if (integ == 1 or (f32 and ab.diag_gone)) else fe_flags()
            return Op("run", (integ, int(rng.integers(2, 4)), flags))
        if name == "advance":
            return Op("advance", (0,))
        if name == "upload":
            keys = [k for k in STATE_KEYS if not (ab.diag_gone and k[0] in DIAG)]
            return an_upload(keys)
        if name in ("diag", "tendU", "tendH"):
            return Op(name, (fe_flags(),))
        if name == "mutator":
            return a_mutator()
        if name == "refusal":
            return a_refusal()
        if name == "tape_create":
            return Op("tape_create", (int(rng.integers(1, 4)),))
        # a tape is open: record, seed, sweep, read, destroy -- and now and then what it refuses
        if rng.random() < 0.3:
            r = a_refusal(tape_only=True)
            if r is not None:
                return r
        if t["seeded"] and t["n"] > 0:
            return Op("sweep")
        if t["n"] > 0 and rng.random() < 0.45:
            return Op("seed")
        if t["n"] < t["cap"]:
            if t["n"] > 0:
                return Op("fe_taped", (fe_flags(),)) if t["kind"] == 0 else Op("rk4_taped")
            return Op("fe_taped", (fe_flags(),)) if rng.random() < 0.5 else Op("rk4_taped")
        return Op("seed") if t["n"] > 0 else Op("tape_destroy")

    while len(ops) < cfg.nops:
        if plan:
            nxt = plan.pop(0)
            op = nxt() if callable(nxt) else nxt
            if op is None:
                continue
            emit(op)
            continue
        adj = [k for k in ADJ_KEYS if ab.tape and ab.read.get(k) != ab.ids[k] and ab.ids[k] != ("zero",)]
        if adj and rng.random() < 0.7:
            emit(Op("adj_download", (draw(adj)[1],)))
            continue
        rd = a_read() if rng.random() < 0.5 else None
        if rd is not None:
            emit(rd)
            continue
        op = a_writer()
        emit(op)
        if op.kind == "rk4_taped" and rng.random() < 0.3:
            # the tape goes while the stage-4 tendencies of its last step are still pending, then they are read
            plan = [Op("tape_destroy"), lambda: a_read((draw(TEND), 1))]
        elif op.kind in STEP_KINDS and rng.random() < 0.6:
            # the wanted pattern: a mutator, then a read of what the step left in Diag / Tend
            def pending_read():
                cand = [k for k in ab.readable() if k[0] in DIAG + TEND]
                return a_read(draw(cand)) if cand else a_read()
            plan = [a_mutator, pending_read]
        elif op.kind == "sweep" and rng.random() < 0.6 and any(k[0] in TEND for k in ab.readable()):
            plan = [lambda: a_read(draw([k for k in ab.readable() if k[0] in TEND]))]       # TendencyVars behind a sweep
        elif op.kind in ("seed", "sweep") and rng.random() < 0.7:
            plan = [a_read]                                      # a read of the state with the tape's work in between
        elif op.kind not in READ_KINDS and rng.random() < 0.5:
            plan = [a_read]
    return ops[:cfg.nops]


def zlib_crc(s):
    return zlib.crc32(s.encode())


# ---------------------------------------------------------------------------------------------------------------------------------
# host model
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Obs:
    kind: str
    rc: int
    key: tuple = None              # the array the observation reads (a STATE_KEYS / ADJ_KEYS entry)
    value: object = None           # np.ndarray, float, int or None
    refusal: str = None            # the name of the predicted refusal (model only)
    fresh: bool = True             # model only: the array changed since its last read (or was never read)
    after: frozenset = frozenset()  # model only: the writer kinds since that array's last read


def _rnd32(a):
    return a.astype(np.float32).astype(np.float64)


class Model:
    """The sequence on the CPU oracle, computed eagerly, exactly as include/moka_hip.h words each call.  mutant: one of MUTANTS,
    wrong on purpose -- each is the bug one flag of the library's state machine exists to prevent."""

    def __init__(self, cfg, seed, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.cfg, self.seed, self.mutant = cfg, seed, mutant
        self.mesh = get_mesh(cfg.meshname)
        mlt = mask_of(cfg)
        self.om = orc.OracleMesh(self.mesh, cfg.K, resting_thickness_sum=resting_thickness(cfg).sum(1),
                                 max_level_edge_top=cfg.K if mlt is None else mlt)
        z = lambda f: np.zeros(shape_of(cfg, f))
        self.st = orc.OracleState(self.om, z(F_SSH), z(F_U), z(F_H), mixed=cfg.f32)
        for (f, l), a in initial_state(cfg, seed).items():
            self.array((f, l))[...] = a
        self.nonlinear, self.visc, self.visc4 = False, 0.0, 0      # visc4: 0 off, 1 on, 2 on with meshScalingDel4
        self.variant = 0
        self.tape = None               # dict(cap, kind, rec=[...], seeded)
        self.lam = None                # {field: array}: the tape's adjoint state as it stands
        self.diag_gone = False         # fp32 storage: DiagnosticVars unavailable after an RK4 step
        self.ssh_loose = True          # ssh[1] was uploaded (or layerThickness[1] was) since something last made it the column sum
        self.pending = None            # mutant "late": what the last step left to be formed at read time
        self._last_read = self._snapshot()      # what the sequence starts from counts as read: zeros and the uploads before the first op
        self._changed = {k: set() for k in STATE_KEYS + ADJ_KEYS}

    # ---- arrays ----
    def array(self, key):
        st = self.st
        if key[0] == "adj":
            return self.lam[key[1]] if self.lam is not None else np.zeros(shape_of(self.cfg, key[1]))
        f, l = key
        return {F_SSH: st.ssh, F_U: st.u, F_H: st.h}[f][l] if f in PROG else \
            {F_HEDGE: st.hEdge, F_FLUX: st.F, F_DIV: st.div, F_VORT: st.vort, F_TENDU: st.tendU, F_TENDH: st.tendH}[f]

    def _snapshot(self):
        return {k: self.array(k).copy() for k in STATE_KEYS + ADJ_KEYS}

    def _rnd(self, a):
        return _rnd32(a) if self.cfg.f32 else a

    # ---- pieces of the oracle ----
    def _interp(self, h):
        return self.om.interpolate_cell2edge(h)

    def _clean_diag(self):
        """diagnostic_compute! of the current level as an RK4 step leaves it: vorticity from zero, fresh layerThicknessEdge."""
        st, om = self.st, self.om
        st.hEdge[...] = self._interp(st.h[1])
        st.F[...] = st.u[1] * st.hEdge
        st.div[...] = om.divergence_on_cell(st.u[1])
        st.vort[...] = om.curl_on_vertex(st.u[1])

    def _nl(self):
        return orc.OracleNonlinear(self.om, visc_del2=self.visc)

    def _del4(self):
        from del4_twin import Del4Twin
        return Del4Twin(self.om, visc_del2=self.visc, visc_del4=visc_del4(self.cfg),
                        scaling=del4_scaling(self.cfg) if self.visc4 == 2 else None)

    def _tendencies(self, u, h):
        """(tendU, tendH, ssh) of the fused evaluation under the terms that are switched on, stored in the state's type."""
        if self.nonlinear and self.visc4:
            return self._del4().tendencies(u, h)
        if self.nonlinear:
            return self._nl().tendencies(u, h)[:3]
        return self.om.tendencies_clean(u, h, mixed=self.cfg.f32)

    def _provisional4(self, dt):
        """P4 = Curr + dt k3 of an RK4 step from the current level (Float64)."""
        u0, h0 = self.st.u[1].copy(), self.st.h[1].copy()
        pu, ph = u0, h0
        for a in (dt / 2., dt / 2., dt):
            tu, th, _ = self._tendencies(pu, ph)
            pu, ph = u0 + a * tu, h0 + a * th
        return pu, ph

    # ---- mutant "late" ----
    def _materialize(self):
        """True model: nothing is ever pending.  Mutant "late": Diag and Tend of the last step are formed now, from whatever the
        arrays hold now (a flush that an upload, advanceTimeLevels!, a toggle or a coefficient change should have forced earlier)."""
        p, self.pending = self.pending, None
        if p is None:
            return
        st = self.st
        if p[0] == "fe":
            _, dt, flags, pre = p
            s = orc.OracleState(self.om, st.ssh[0], st.u[0], st.h[0], mixed=self.cfg.f32)
            for n in ("hEdge", "F", "div", "vort", "tendU", "tendH"):
                getattr(s, n)[...] = pre[n]
            s.step_fe(dt, flags)
            for n in ("hEdge", "F", "div", "tendU", "tendH"):
                getattr(st, n)[...] = getattr(s, n)
        else:
            _, pu, ph = p
            if not self.cfg.f32:
                self._clean_diag()
                if pu is not None:
                    tu, th, _ = self._tendencies(pu, ph)
                    st.tendU[...] = tu; st.tendH[...] = th

    # ---- steps ----
    def _keep_prev(self):
        return [a.copy() for a in (self.st.ssh[0], self.st.u[0], self.st.h[0])] if self.mutant == "prev_level_lost" else None

    def _lose_prev(self, kept):
        if kept is not None:           # mutant: a rotation off by one set hands back the level before the previous one
            for a, b in zip((self.st.ssh[0], self.st.u[0], self.st.h[0]), kept):
                a[...] = b

    def _step_fe(self, dt, flags):
        st = self.st
        self._materialize()
        kept = self._keep_prev()
        if self.mutant == "stale_from_prev" and flags & FE_STALE:
            st.hEdge[...] = self._rnd(self._interp(st.h[0]))     # hEdgePrev not cleared: the previous level, whatever Diag holds
        pre = {n: getattr(st, n).copy() for n in ("hEdge", "F", "div", "vort", "tendU", "tendH")} if self.mutant == "late" else None
        st.step_fe(dt, flags)
        self.diag_gone = False
        self.ssh_loose = bool(flags & FE_LEVEL1) and self.cfg.K > 1
        self._lose_prev(kept)
        if self.mutant == "late":
            self.pending = ("fe", dt, flags, pre)

    def _step_rk4(self, dt, s13=False):
        st = self.st
        self.pending = None                                      # superseded
        kept = self._keep_prev()
        p4 = (None, None)
        if self.mutant == "late" and not self.cfg.f32:
            p4 = self._provisional4(dt)
        if self.mutant == "ssh_stored" and self.ssh_loose and not self.cfg.f32 and not self.nonlinear:
            self._rk4_stored_ssh(dt)
        elif self.nonlinear and self.visc4:                      # Del4: the reference's running sum (no 13-stream form)
            from del4_twin import TwinState
            ts = TwinState(st.ssh[1], st.u[1], st.h[1])
            self._del4().step_rk4(ts, dt)
            for l in (0, 1):
                st.ssh[l][...] = ts.ssh[l]; st.u[l][...] = ts.u[l]; st.h[l][...] = ts.h[l]
            st.tendU[...] = ts.tendU; st.tendH[...] = ts.tendH
            self._clean_diag()
        elif self.nonlinear:
            nl = self._nl()
            (nl.step_rk4_s13 if s13 else nl.step_rk4)(st, dt)
            self._clean_diag()
        else:
            (st.step_rk4_s13 if s13 else st.step_rk4)(dt)
        self.diag_gone = self.cfg.f32
        self.ssh_loose = False
        self._lose_prev(kept)
        if self.mutant == "late":
            self.pending = ("rk4",) + p4

    def _rk4_stored_ssh(self, dt):
        """Mutant "ssh_stored": stage 1 takes the stored ssh although layerThickness or ssh of the current level was uploaded."""
        st, om, K = self.st, self.om, self.cfg.K
        for a in (st.ssh, st.u, st.h):
            a[0][...] = a[1]
        cu, ch = st.u[0], st.h[0]
        nu, nh = cu.copy(), ch.copy()
        a = (dt / 2., dt / 2., dt)
        b = (dt / 6., dt / 3., dt / 3., dt / 6.)
        pu, ph = cu.copy(), ch.copy()
        for s in range(4):
            tu, th, _ = om.tendencies_clean(pu, ph)
            if s == 0:
                tu = np.zeros_like(tu)
                orc.lib().oracle_normal_velocity_tendency(om.ref, orc._p(tu), orc._p(st.ssh[0]), orc._p(np.ascontiguousarray(pu)), K)
            if s < 3:
                pu, ph = cu + a[s] * tu, ch + a[s] * th
            nu, nh = nu + b[s] * tu, nh + b[s] * th
        st.u[1][...] = nu; st.h[1][...] = nh
        st.ssh[1][...] = om.update_ssh(nh)
        st.tendU[...] = tu; st.tendH[...] = th
        self._clean_diag()

    def streams(self, s13_key):
        """What moka_state_rk4_streams answers: 13 when key 7 is set, the state is Float64 and its stage launches are the default
        patch kernels of a mesh they serve (the config says), else 16."""
        return 13 if (s13_key and self.cfg.s13 and not self.cfg.f32 and self.variant in (0, 11)) else 16

    # ---- the reverse sweeps of oracle.OracleAdjoint / OracleAdjointRK4, seeded when moka_adjoint_seed_sum_sq_ssh is called ----
    def _seed(self):
        cfg, t = self.cfg, self.tape
        lam = {f: np.zeros(shape_of(cfg, f)) for f in (F_SSH, F_U, F_H, F_HEDGE)}
        if t["kind"] == 1:
            lam[F_H] = np.repeat((2.0 * self.st.ssh[1])[:, None], cfg.K, axis=1)
        else:
            lam[F_SSH] = 2.0 * self.st.ssh[1]
        self.lam = lam
        t["seeded"] = True

    def _sweep(self):
        t, om, lam = self.tape, self.om, self.lam
        m, K = self.mesh, self.cfg.K
        p = orc._p
        if t.get("teoe") is None:
            t["teoe"], t["tw"] = orc.transpose_coriolis(m)
        teoe, tw = t["teoe"], t["tw"]
        if t["kind"] == 0:
            lamS, lamU, lamH, lamE = lam[F_SSH], lam[F_U], lam[F_H], lam[F_HEDGE]
            Enew, csum = np.zeros((m.nEdges, K)), np.zeros(m.nEdges)
            for u, hE, dt, flags in reversed(t["rec"]):
                oU, oH, oS, oE = np.zeros_like(lamU), np.zeros_like(lamH), np.zeros_like(lamS), np.zeros_like(lamE)
                orc.lib().oracle_step_fe_adjoint(om.ref, p(teoe), p(tw), teoe.shape[1], dt, flags, p(u), p(hE), p(lamU), p(lamH),
                                                 p(lamS), p(lamE), p(oU), p(oH), p(oS), p(oE), p(Enew), p(csum))
                lamU, lamH, lamS, lamE = oU, oH, oS, oE
            self.lam = {F_SSH: lamS, F_U: lamU, F_H: lamH, F_HEDGE: lamE}
        elif t["rec"]:
            def tt(u, h, kU, kH):
                oU, oH = np.zeros((m.nEdges, K)), np.zeros((m.nCells, K))
                En, cs = np.zeros((m.nEdges, K)), np.zeros(m.nEdges)
                c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
                orc.lib().oracle_tendency_transpose(om.ref, p(teoe), p(tw), teoe.shape[1], p(c(u)), p(c(h)), p(c(kU)), p(c(kH)),
                                                    p(oU), p(oH), p(En), p(cs))
                return oU, oH
            XU, XH = lam[F_U], lam[F_H]
            for P, dt in reversed(t["rec"]):
                a = (dt / 2., dt / 2., dt)
                b = (dt / 6., dt / 3., dt / 3., dt / 6.)
                PU, PH = tt(P[3][0], P[3][1], b[3] * XU, b[3] * XH)
                accU, accH = XU + PU, XH + PH
                for s in (2, 1, 0):
                    PU, PH = tt(P[s][0], P[s][1], b[s] * XU + a[s] * PU, b[s] * XH + a[s] * PH)
                    accU, accH = accU + PU, accH + PH
                XU, XH = accU, accH
            self.lam = {F_SSH: np.zeros_like(lam[F_SSH]), F_U: XU, F_H: XH, F_HEDGE: np.zeros_like(lam[F_HEDGE])}
        t["rec"] = []

    # ---- one op ----
    def _refuse(self, kind, code, name):
        return Obs(kind, code, refusal=name)

    def _fe_refusal(self, kind, flags):
        if self.nonlinear:
            return self._refuse(kind, ERR_UNSUPPORTED, "fe_nonlinear")
        if self.cfg.f32 and flags & FE_LEVEL1:
            return self._refuse(kind, ERR_UNSUPPORTED, "fe_level1_f32")
        if self.cfg.f32 and self.diag_gone and flags & (FE_STALE | FE_ACCUM):
            return self._refuse(kind, ERR_UNSUPPORTED, "fe_carry_after_rk4")
        return None

    def _read_guard(self, kind, f):
        if self.cfg.f32 and self.diag_gone and f in DIAG:
            return self._refuse(kind, ERR_UNSUPPORTED, "diag_after_rk4")
        return None

    def apply(self, op):
        cfg, st, k, a = self.cfg, self.st, op.kind, op.args
        dt, K, t = cfg.dt, cfg.K, self.tape
        if k == "fe":
            r = self._fe_refusal(k, a[0])
            if r:
                return r
            self._step_fe(dt, a[0])
            return Obs(k, OK)
        if k in ("rk4", "rk4_s13"):
            n = self.streams(k == "rk4_s13")
            self._step_rk4(dt, s13=n == 13)
            return Obs(k, OK, value=n)
        if k == "run":
            integ, n, flags = a
            if integ == 0:
                r = self._fe_refusal(k, flags)
                if r:
                    return r
            for _ in range(n):
                self._step_fe(dt, flags) if integ == 0 else self._step_rk4(dt)
            return Obs(k, OK)
        if k == "tend":
            self._materialize()
            if self.mutant == "ssh_stored" and self.ssh_loose and not self.nonlinear:
                tu = np.zeros_like(st.tendU)
                orc.lib().oracle_normal_velocity_tendency(self.om.ref, orc._p(tu), orc._p(st.ssh[1]), orc._p(st.u[1]), K)
                _, th, _ = self._tendencies(st.u[1], st.h[1])
                st.tendU[...] = self._rnd(tu); st.tendH[...] = th
            else:
                tu, th, ssh = self._tendencies(st.u[1], st.h[1])
                st.tendU[...] = tu; st.tendH[...] = th; st.ssh[1][...] = ssh
            self.ssh_loose = False
            return Obs(k, OK)
        if k == "advance":
            if a[0] & FE_LEVEL1 and K > 1:
                return self._refuse(k, ERR_UNSUPPORTED, "advance_level1")
            for x in (st.ssh, st.u, st.h):
                x[0][...] = x[1]
            return Obs(k, OK)
        if k in ("diag", "tendU", "tendH"):
            if self.nonlinear:
                return self._refuse(k, ERR_UNSUPPORTED, "piecewise_nonlinear")
            if cfg.f32:
                return self._refuse(k, ERR_UNSUPPORTED, "piecewise_f32")
            self._materialize()
            flags = a[0]
            nlev = 1 if flags & FE_LEVEL1 else K
            L, p, om = orc.lib(), orc._p, self.om
            if k == "diag":
                if not flags & FE_ACCUM:
                    st.vort[...] = 0.0
                if flags & FE_STALE:
                    L.oracle_diagnostic_compute(om.ref, p(st.hEdge), p(st.F), p(st.div), p(st.vort), p(st.u[1]), p(st.h[1]), nlev)
                else:
                    scratch = np.zeros_like(st.u[1])
                    L.oracle_interpolate_cell2edge(om.ref, p(st.hEdge), p(st.h[1]), nlev)
                    L.oracle_thickness_flux(om.ref, p(st.F), p(st.u[1]), p(st.hEdge), nlev)
                    L.oracle_divergence_on_cell(om.ref, p(st.div), p(st.u[1]), p(scratch))
                    L.oracle_curl_on_vertex(om.ref, p(st.vort), p(st.u[1]))
            elif k == "tendU":
                L.oracle_normal_velocity_tendency(om.ref, p(st.tendU), p(st.ssh[1]), p(st.u[1]), nlev)
            else:
                L.oracle_layer_thickness_tendency(om.ref, p(st.tendH), p(st.F), nlev)
            return Obs(k, OK)
        if k == "upload":
            f, l, vs = a
            r = self._read_guard(k, f)
            if r:
                return r
            if f not in PROG:
                self._materialize()
            self.array((f, l))[...] = values(cfg, f, vs)
            if l == 1 and f in (F_SSH, F_H):
                self.ssh_loose = True
            return Obs(k, OK, key=(f, l))
        if k in READ_KINDS:
            f, l = a[0], a[1]
            r = self._read_guard(k, f)
            if r:
                return r
            if f not in PROG:
                self._materialize()
            arr = self.array((f, l))
            if k == "download":
                v = arr.copy()
            elif k == "rows":
                v = arr[list(a[2])].reshape(len(a[2]), -1).copy()
            else:
                c = np.ascontiguousarray(arr)
                v = float(orc.lib().oracle_sum_sq(orc._p(c), c.size))
            return Obs(k, OK, key=(f, l), value=v)
        if k == "placement":
            if t is not None:
                return self._refuse(k, ERR_UNSUPPORTED, "placement_tape")
            return Obs(k, OK)
        if k == "variant":
            if a[0] not in VARIANTS:
                return self._refuse(k, ERR_UNSUPPORTED, "variant_gone")
            self.variant = a[0]
            return Obs(k, OK)
        if k == "tuning":
            return Obs(k, OK)
        if k == "nonlinear":
            if a[0] and cfg.f32:
                return self._refuse(k, ERR_UNSUPPORTED, "nonlinear_f32")
            if a[0] and t is not None:
                return self._refuse(k, ERR_UNSUPPORTED, "nonlinear_tape")
            self.nonlinear = bool(a[0])
            return Obs(k, OK)
        if k == "del2":
            if a[0] and not self.nonlinear:
                return self._refuse(k, ERR_UNSUPPORTED, "del2_without_nonlinear")
            self.visc = visc_del2(cfg) if a[0] else 0.0
            return Obs(k, OK)
        if k == "del4":
            if a[0] and not self.nonlinear:
                return self._refuse(k, ERR_UNSUPPORTED, "del4_without_nonlinear")
            self.visc4 = a[0]
            return Obs(k, OK)
        if k == "tape_create":
            if cfg.f32:
                return self._refuse(k, ERR_UNSUPPORTED, "tape_f32")
            if self.nonlinear:
                return self._refuse(k, ERR_UNSUPPORTED, "tape_nonlinear")
            self.tape = dict(cap=a[0], kind=None, rec=[], seeded=False)
            self.lam = {f: np.zeros(shape_of(cfg, f)) for f in (F_SSH, F_U, F_H, F_HEDGE)}
            return Obs(k, OK)
        if k == "tape_destroy":
            self.tape = self.lam = None
            return Obs(k, OK)
        if k == "fe_taped":
            flags = a[0]
            if len(t["rec"]) >= t["cap"]:
                return self._refuse(k, ERR_ARG, "tape_full")
            if flags & FE_LEVEL1 and K != 1:
                return self._refuse(k, ERR_UNSUPPORTED, "taped_level1")
            if t["rec"] and t["kind"] != 0:
                return self._refuse(k, ERR_UNSUPPORTED, "mix_integrators")
            self._materialize()
            u = st.u[1].copy()
            hE = st.hEdge.copy() if flags & FE_STALE else self._interp(st.h[1])
            self._step_fe(dt, flags)
            t["rec"].append((u, hE, float(dt), int(flags)))
            t["kind"], t["seeded"] = 0, False
            return Obs(k, OK)
        if k == "rk4_taped":
            if len(t["rec"]) >= t["cap"]:
                return self._refuse(k, ERR_ARG, "tape_full")
            if t["rec"] and t["kind"] != 1:
                return self._refuse(k, ERR_UNSUPPORTED, "mix_integrators")
            u0, h0 = st.u[1].copy(), st.h[1].copy()
            P, pu, ph = [(u0, h0)], u0, h0
            for s in (dt / 2., dt / 2., dt):
                tu, th, _ = self.om.tendencies_clean(pu, ph)
                pu, ph = u0 + s * tu, h0 + s * th
                P.append((pu, ph))
            self._step_rk4(dt)                                   # a taped step keeps the reference's running sum
            t["rec"].append((P, float(dt)))
            t["kind"], t["seeded"] = 1, False
            return Obs(k, OK)
        if k == "seed":
            self._seed()
            return Obs(k, OK)
        if k == "sweep":
            self._sweep()
            return Obs(k, OK)
        if k == "adj_download":
            return Obs(k, OK, key=("adj", a[0]), value=self.array(("adj", a[0])).copy())
        raise ValueError(f"unknown op {op}")

    def run(self, ops):
        """The observations, one per op.  Beside the value each carries what the CPU checks need: whether the array changed since
        its last read, and which writer kinds ran since then (those that changed it, and those that came while a change was unread)."""
        out = []
        before = self._snapshot()
        for op in ops:
            o = self.apply(op)
            if op.kind in READ_KINDS + ("adj_download",):
                if o.rc == OK:
                    key = o.key
                    last = self._last_read.get(key)
                    cur = self.array(key)
                    o.fresh = not np.array_equal(last, cur)
                    o.after = frozenset(self._changed[key])
                    self._changed[key] = set()
                    self._last_read[key] = cur.copy()
            else:
                now = self._snapshot()
                for key in STATE_KEYS + ADJ_KEYS:
                    if not np.array_equal(before[key], now[key]):
                        self._changed[key].add(op.kind)
                    elif o.rc == OK and op.kind in NON_ARRAY_OPS and self._changed[key]:
                        self._changed[key].add(op.kind)          # came while a change of this array was still unread
                before = now
            out.append(o)
        return out


# ---------------------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------------------
def first_mismatch(cfg, seed, ops, expect, got):
    """None when every observation of `got` equals the model's; else the message the GPU test fails with (nothing is replayed)."""
    for i, (op, e, g) in enumerate(zip(ops, expect, got)):
        what = None
        if e.rc != g.rc:
            what = f"status {g.rc}, the model predicts {e.rc}" + (f" ({e.refusal})" if e.refusal else "")
        elif isinstance(e.value, np.ndarray):
            gv = np.asarray(g.value).reshape(e.value.shape)
            if not np.array_equal(gv, e.value):
                bad = gv != e.value
                with np.errstate(invalid="ignore"):
                    what = f"{int(bad.sum())} of {bad.size} elements differ, largest difference {np.nanmax(np.abs(gv - e.value)[bad]):.3e}"
        elif e.value is not None and e.value != g.value:
            what = f"{g.value!r}, the model has {e.value!r}"
        if what:
            head = f"config {cfg.name} seed {seed}: op {i} ({op.kind}) " + (f"of {key_name(e.key)} " if e.key else "") + "-- " + what
            return head + "\nops up to there:\n" + "\n".join(f"  {j:2d} {o}" for j, o in enumerate(ops[:i + 1]))
    if len(expect) != len(got):
        return f"config {cfg.name} seed {seed}: {len(got)} observations for {len(expect)} ops"
    return None


# ---------------------------------------------------------------------------------------------------------------------------------
# device runner
# ---------------------------------------------------------------------------------------------------------------------------------
class Device:
    """One device mesh per config, shared by its seeds; run() gives each sequence a fresh state."""

    def __init__(self, backend, cfg):
        import moka_hip as mk
        from moka_hip import lib as L
        self.L, self.lib, self.backend, self.cfg = L, L.lib(), backend, cfg
        mesh = get_mesh(cfg.meshname)
        hm = mk.HorzMesh(mesh)
        vm = mk.VerticalMesh(hm, nVertLevels=cfg.K, restingThickness=resting_thickness(cfg), multilayer=True)
        mlt = mask_of(cfg)
        if mlt is not None:
            vm.maxLevelEdge.Top[:] = mlt
        self.M = mk.Mesh(hm, vm, backend=backend, state_bytes=cfg.sbytes)
        self.counters = {"sequences": 0, "fe_steps": 0, "lean": 0, "fe_paths": set(), "rk4_steps": 0, "s13": 0}

    def close(self):
        self.M.close()

    def run(self, ops, seed):
        """The observations of the same ops through moka_hip.lib, in the model's form.  The process-global kernel variant and every
        tuning key touched are put back whatever happens; the tape goes before its state (its destructor dereferences the state)."""
        L, lib, cfg, ctx = self.L, self.lib, self.cfg, self.backend._h
        cnt = self.counters
        hS, hT = C.c_void_p(), C.c_void_p()
        saved = {}
        out = []

        def tune(key, value):
            if key not in saved:
                v = C.c_int()
                L.check(lib.moka_get_tuning(key, C.byref(v)))
                saved[key] = v.value
            return lib.moka_set_tuning(key, value)

        def after_fe():
            cnt["fe_steps"] += 1
            cnt["lean"] += lib.moka_fe_lazy_pending(hS)
            cnt["fe_paths"].add(lib.moka_last_fe_path(hS))

        try:
            L.check(lib.moka_state_create(ctx, self.M._h, C.byref(hS)), ctx)
            for (f, l), a in initial_state(cfg, seed).items():
                L.check(lib.moka_state_upload(hS, f, l, L.f64(a)), ctx)
            for op in ops:
                k, a = op.kind, op.args
                value = None
                if k == "fe":
                    rc = lib.moka_step_fe(hS, cfg.dt, a[0])
                    if rc == OK:
                        after_fe()
                elif k in ("rk4", "rk4_s13"):
                    if k == "rk4_s13":
                        L.check(tune(7, 1))
                    try:
                        value = lib.moka_state_rk4_streams(hS)
                        rc = lib.moka_step_rk4(hS, cfg.dt)
                    finally:
                        if k == "rk4_s13":
                            L.check(tune(7, 0))
                    if rc == OK:
                        cnt["rk4_steps"] += 1
                        cnt["s13"] += value == 13
                elif k == "run":
                    rc = lib.moka_run(hS, a[0], cfg.dt, a[1], a[2])
                    if rc == OK and a[0] == 0:
                        after_fe()
                    elif rc == OK:
                        cnt["rk4_steps"] += a[1]
                elif k == "tend":
                    rc = lib.moka_tendencies(hS)
                elif k == "advance":
                    rc = lib.moka_advance_time_levels(hS, a[0])
                elif k == "diag":
                    rc = lib.moka_diagnostic_compute(hS, a[0])
                elif k == "tendU":
                    rc = lib.moka_compute_normal_velocity_tendency(hS, a[0])
                elif k == "tendH":
                    rc = lib.moka_compute_layer_thickness_tendency(hS, a[0])
                elif k == "upload":
                    rc = lib.moka_state_upload(hS, a[0], a[1], L.f64(values(cfg, a[0], a[2])))
                elif k == "download":
                    buf = np.full(shape_of(cfg, a[0]), np.nan)
                    rc = lib.moka_state_download(hS, a[0], a[1], L.f64(buf))
                    value = buf
                elif k == "rows":
                    rows = np.asarray(a[2], dtype=np.int32)
                    buf = np.full((rows.size, 1 if a[0] == F_SSH else cfg.K), np.nan)
                    rc = lib.moka_state_download_rows(hS, a[0], a[1], rows.size, L.i32(rows), L.f64(buf))
                    value = buf
                elif k == "sumsq":
                    s = C.c_double(np.nan)
                    rc = lib.moka_sum_sq(hS, a[0], a[1], C.byref(s))
                    value = s.value
                elif k == "placement":
                    rc = lib.moka_state_optimize_placement(hS, a[0], None, None)
                elif k == "variant":
                    rc = lib.moka_set_kernel_variant(ctx, a[0])
                elif k == "tuning":
                    rc = tune(a[0], a[1])
                elif k == "nonlinear":
                    rc = lib.moka_set_nonlinear(hS, a[0])
                elif k == "del2":
                    rc = lib.moka_set_viscosity_del2(hS, visc_del2(cfg) if a[0] else 0.0)
                elif k == "del4":
                    sc = del4_scaling(cfg) if a[0] == 2 else None
                    rc = lib.moka_set_viscosity_del4(hS, visc_del4(cfg) if a[0] else 0.0, None if sc is None else sc.ctypes.data_as(C.c_void_p))
                elif k == "tape_create":
                    rc = lib.moka_tape_create(hS, a[0], C.byref(hT))
                elif k == "tape_destroy":
                    lib.moka_tape_destroy(hT)
                    hT, rc = C.c_void_p(), OK
                elif k == "fe_taped":
                    rc = lib.moka_step_fe_taped(hT, cfg.dt, a[0])
                    if rc == OK:
                        after_fe()
                elif k == "rk4_taped":
                    rc = lib.moka_step_rk4_taped(hT, cfg.dt)
                elif k == "seed":
                    rc = lib.moka_adjoint_seed_sum_sq_ssh(hT)
                elif k == "sweep":
                    rc = lib.moka_adjoint_sweep(hT)
                elif k == "adj_download":
                    buf = np.full(shape_of(cfg, a[0]), np.nan)
                    rc = lib.moka_adjoint_download(hT, a[0], L.f64(buf))
                    value = buf
                else:
                    raise ValueError(f"unknown op {op}")
                out.append(Obs(k, int(rc), value=value if rc == OK else None))
            cnt["sequences"] += 1
        finally:
            if hT:
                lib.moka_tape_destroy(hT)
            if hS:
                lib.moka_state_destroy(hS)
            lib.moka_set_kernel_variant(ctx, 0)
            for key, v in saved.items():
                lib.moka_set_tuning(key, v)
        return out


# ---------------------------------------------------------------------------------------------------------------------------------
# machine B: passive tracers over the dycore the sequence currently has.  Model: KgradTwin / KgradAdjointTwin of
# tests/tracer_kgrad_twin.py (the top of the twin stack) over the OracleMesh (linear terms) or del4_twin.Del4Twin (nonlinear, Del2).
# ---------------------------------------------------------------------------------------------------------------------------------
B_MUTANTS = ("coeff_late", "prev_level_lost", "ssh_stored", "late")
KFACT = (0.02, 0.0, 0.005, 0.011, 0.016)          # kappa_j dt / dcEdge_min^2: pairwise distinct, one exact zero
K4FACT = (0.002, 0.0, 0.0005, 0.001, 0.0015)      # kappa4_j dt / dcEdge_min^4
B_READS = ("download", "rows", "sumsq", "tr_download", "x_download", "g_download", "k_scalar", "k_density")


@dataclass(frozen=True)
class TracerConfig(Config):
    nT: int = 3
    patch_cells: int = 0
    tracer_path: int = 1

    machine = "B"


CONFIGS.update({c.name: c for c in (
    # 72-cell patches at K = 34: the patch form keeps two tracers resident, the third takes a second pass (tracer_cases.patch_chunk)
    TracerConfig("B1", "planar", 34, dt=2.0, s13=True, nT=3, patch_cells=72, tracer_path=1, nops=32),
    TracerConfig("B2", "ico6f", 6, dt=20.0, nT=5, tracer_path=2, nops=34),
)})


def coefficients(cfg, which, pattern, n):
    """The vector a moka_set_tracer_diffusion / _biharmonic op carries: "zero" (NULL), "some" (one exact zero among the values) or
    "other" (the same values, reversed)."""
    if pattern == "zero" or n == 0:
        return None
    dc = float(get_mesh(cfg.meshname).dcEdge.min())
    f = [x * dc ** (2 if which == "kappa" else 4) / cfg.dt for x in (KFACT if which == "kappa" else K4FACT)][:n]
    return f if pattern == "some" else f[::-1]


def tracer_values(cfg, kind, vseed):
    """kind: "phi" in [0.5, 1.5], "unit" (1 everywhere), "source" (tracer m/s), "zero", "seed" (an adjoint seed)."""
    shp = shape_of(cfg, F_H)
    if kind == "unit":
        return np.ones(shp)
    if kind == "zero":
        return np.zeros(shp)
    rng = np.random.default_rng([cfg.K, 99, vseed])
    if kind == "phi":
        return rng.uniform(0.5, 1.5, shp)
    return rng.uniform(-1e-2, 1e-2, shp) if kind == "source" else rng.uniform(-1, 1, shp)


def b_vocabulary(cfg):
    return ("set_tracers", "tr_upload", "tr_download", "kappa", "kappa4", "source", "rk4", "rk4_s13", "run", "advance", "nonlinear",
            "del2", "del4", "placement", "upload", "download", "rows", "sumsq", "fe", "tape_create", "tr_tape_create", "tr_taped", "tr_seed",
            "tr_sweep", "x_download", "g_download", "k_scalar", "k_density", "tr_tape_destroy")


def b_refusals(cfg):
    return ("fe_tracers", "run_fe_tracers", "tape_tracers", "placement_tape", "set_tracers_tape", "tape_full", "sweep_unseeded",
            "del2_without_nonlinear", "del4_without_nonlinear")


def sequence_b(cfg, seed):
    rng = np.random.default_rng([zlib_crc(cfg.name), seed])
    ops = []
    vs = [0]
    nT, tape, nonlinear, visc, visc4 = 0, None, False, False, 0
    plan = []
    unit0 = True
    dirty_tr, dirty_prog = [], []
    has_kappa = has_k4 = False

    def draw(items, weights=None):
        if weights is None:
            return items[int(rng.integers(len(items)))]
        w = np.asarray(weights, dtype=np.float64)
        return items[int(rng.choice(len(items), p=w / w.sum()))]

    def vseed():
        vs[0] += 1
        return 104729 * (seed + 1) + vs[0]

    unit_read = set()                  # the unit tracer stays exactly 1.0: one read per level shows it, more would count the same bits

    def stepped():
        nonlocal dirty_tr, dirty_prog
        dirty_tr = [(j, l) for l in (1, 0) for j in range(nT) if not (j == 0 and unit0 and l in unit_read)]
        unit_read.update(l for j, l in dirty_tr if j == 0 and unit0)
        dirty_prog = [(f, 1) for f in TEND] + [(f, l) for l in (1, 0) for f in PROG]

    def a_read():
        if dirty_tr and (not dirty_prog or rng.random() < 0.65):
            return Op("tr_download", dirty_tr.pop(0))
        if dirty_prog:
            key = dirty_prog.pop(0)
            kind = draw(READ_KINDS)
            if kind == "rows":
                n = shape_of(cfg, key[0])[0]
                return Op("rows", key + (tuple(int(r) for r in rng.integers(0, n, 3)),))
            return Op(kind, key)
        return None

    ops.append(Op("set_tracers", (cfg.nT,)))
    nT = cfg.nT
    for j in range(nT):
        ops.append(Op("tr_upload", (j, 1, "unit" if j == 0 else "phi", vseed())))
    while len(ops) < cfg.nops:
        t = tape
        if plan:
            nxt = plan.pop(0)
            nxt = nxt() if callable(nxt) else nxt
            if nxt is not None:
                ops.append(nxt)
            continue
        if t and t["swept"]:
            pend = t["reads"]
            if pend:
                ops.append(pend.pop(0))
                continue
        if rng.random() < 0.4:
            r = a_read()
            if r is not None:
                ops.append(r)
                continue
        c = [("rk4", 6), ("run", 1.5), ("rk4_s13", 1), ("coef", 6), ("tr_upload", 2), ("upload", 1.5), ("advance", 1), ("toggle", 2),
             ("placement", 1), ("refusal", 2.5), ("set_tracers", 0.8)]
        c += [("tape", 14)] if t else [("tr_tape_create", 3 if nT else 0.001)]
        name = draw([x[0] for x in c], [x[1] for x in c])
        if nT == 0 and name in ("coef", "tr_upload", "tape", "tr_tape_create"):
            name = "set_tracers"
        if name in ("rk4", "rk4_s13"):
            ops.append(Op(name)); stepped()
        elif name == "run":
            ops.append(Op("run", (1, int(rng.integers(2, 4)), 0))); stepped()
        elif name == "coef":
            which = draw(("kappa", "kappa4", "source"), (3, 2, 3))
            if which == "source":
                ops.append(Op("source", (int(rng.integers(nT)), draw(("source", "zero", "none"), (3, 1, 1)), vseed())))
            else:
                on = has_kappa if which == "kappa" else has_k4
                pat = draw(("zero", "some", "other"), (3 if on else 1, 3, 2))
                ops.append(Op(which, (pat,)))
                if which == "kappa":
                    has_kappa = pat != "zero"
                else:
                    has_k4 = pat != "zero"
        elif name == "tr_upload":
            j, l = int(rng.integers(nT)), int(rng.integers(2))
            if j == 0 and unit0:
                j = nT - 1                                       # tracer 0 stays the unit tracer
            ops.append(Op("tr_upload", (j, l, "phi", vseed())))
            if (j, l) in dirty_tr:
                dirty_tr.remove((j, l))
            dirty_tr.insert(0, (j, l))
        elif name == "upload":
            f, l = draw(PROG), int(rng.integers(2))
            ops.append(Op("upload", (f, l, vseed())))
            if (f, l) in dirty_prog:
                dirty_prog.remove((f, l))
            dirty_prog.insert(0, (f, l))
        elif name == "advance":
            ops.append(Op("advance", (0,)))
            dirty_tr = [(j, 0) for j in range(1, nT)] + [k for k in dirty_tr if k[1] == 1]
            dirty_prog = [(f, 0) for f in PROG] + [k for k in dirty_prog if k[1] == 1]
        elif name == "toggle":
            if nonlinear and rng.random() < 0.6:
                if rng.random() < 0.5:
                    visc = not visc
                    ops.append(Op("del2", (int(visc),)))
                else:
                    visc4 = 0 if visc4 else int(rng.integers(1, 3))
                    ops.append(Op("del4", (visc4,)))
            elif not nonlinear and rng.random() < 0.25:
                ops.append(Op(draw(("del2", "del4")), (1,)))                   # refused without the nonlinear terms
            else:
                nonlinear = not nonlinear
                ops.append(Op("nonlinear", (int(nonlinear),)))
        elif name == "placement":
            ops.append(Op("placement", (int(rng.integers(0, 3)),)))
        elif name == "set_tracers":
            if t:
                ops.append(Op("set_tracers", (draw((2, cfg.nT)),)))          # refused while the tape lives
                continue
            n = draw((0, 2, cfg.nT), (2, 2, 3))
            ops.append(Op("set_tracers", (n,)))
            nT, has_kappa, has_k4 = n, False, False
            dirty_tr = []
            unit_read.clear()
            if n == 0:
                # the dycore alone again: a step (now and then under key 7), reads of it, then tracers come back
                def alone():
                    stepped()
                    kind = draw(("rk4", "rk4_s13", "run"), (2, 0.001 if nonlinear else 3, 1))
                    return Op("run", (1, 2, 0)) if kind == "run" else Op(kind)
                def back():
                    nonlocal nT
                    nT = cfg.nT
                    ups = [Op("tr_upload", (j, 1, "unit" if j == 0 else "phi", vseed())) for j in range(nT)]
                    plan[:0] = ups[1:]
                    return Op("set_tracers", (nT,))
                plan = [alone, a_read, a_read, back, lambda: Op("tr_upload", (0, 1, "unit", vseed()))]
            for j in range(nT):
                ops.append(Op("tr_upload", (j, 1, "unit" if j == 0 else "phi", vseed())))
        elif name == "refusal":
            cand = [Op("fe", (int(rng.integers(0, 4)),)), Op("run", (0, 2, 0)), Op("tape_create", (2,))] if nT else []
            if t:
                cand += [Op("placement", (1,)), Op("set_tracers", (draw((2, cfg.nT)),))]
                if t["n"] >= t["cap"]:
                    cand += [Op("tr_taped")] * 3
                if not t["seeded"] and t["n"] > 0:
                    cand += [Op("tr_sweep")] * 2
            if cand:
                ops.append(draw(cand))
        elif name == "tr_tape_create":
            want = tuple(j for j in range(nT) if rng.random() < 0.4)
            kfl = tuple((j, int(rng.integers(1, 4))) for j in range(nT) if rng.random() < 0.4)
            ops.append(Op("tr_tape_create", (int(rng.integers(1, 4)), want, kfl)))
            tape = dict(cap=ops[-1].args[0], n=0, seeded=False, swept=False, want=want, kfl=kfl, reads=[], nT=nT)
        else:                                                    # a tape is open
            if not t["seeded"] and not t["swept"] and t["n"] > 0 and rng.random() < 0.2:
                ops.append(Op("tr_sweep"))                       # refused: not seeded
            elif t["swept"]:
                ops.append(Op("tr_tape_destroy")); tape = None
            elif t["seeded"]:
                ops.append(Op("tr_sweep"))
                t["swept"], t["n"] = True, 0
                rd = [Op("x_download", (j,)) for j in range(t["nT"])] + [Op("g_download", (j,)) for j in t["want"]]
                for j, bits in t["kfl"]:
                    for w in (1, 2):
                        if bits & w:
                            rd.append(Op(draw(("k_scalar", "k_density")), (j, w)))
                order = rng.permutation(len(rd))
                t["reads"] = [rd[i] for i in order][:5]
            elif t["n"] > 0 and (t["n"] >= t["cap"] or rng.random() < 0.5):
                ops.append(Op("tr_seed", (vseed(),))); t["seeded"] = True
            elif t["n"] < t["cap"]:
                ops.append(Op("tr_taped")); t["n"] += 1; stepped()
                if rng.random() < 0.6 and t["n"] < t["cap"]:       # a change of a coefficient between two taped steps
                    which = draw(("kappa", "kappa4", "source"))
                    if which == "source":
                        ops.append(Op("source", (int(rng.integers(nT)), draw(("source", "zero", "none"), (3, 1, 1)), vseed())))
                    else:
                        ops.append(Op(which, (draw(("some", "other", "zero")),)))
                        if which == "kappa":
                            has_kappa = ops[-1].args[0] != "zero"
                        else:
                            has_k4 = ops[-1].args[0] != "zero"
    return ops[:cfg.nops]


class _StoredSsh:
    """Mutant "ssh_stored": the first tendency evaluation of a step (linear terms) takes the stored ssh."""

    def __init__(self, om, ssh):
        self.om, self.ssh, self.first = om, np.ascontiguousarray(ssh), True

    def tendencies_clean(self, u, h):
        tu, th, s = self.om.tendencies_clean(u, h)
        if self.first:
            self.first = False
            tu = np.zeros_like(tu)
            orc.lib().oracle_normal_velocity_tendency(self.om.ref, orc._p(tu), orc._p(self.ssh), orc._p(np.ascontiguousarray(u)), self.om.K)
        return tu, th, s


class TracerModel:
    """Machine B on the twin stack, eagerly.  Mutants: B_MUTANTS."""

    def __init__(self, cfg, seed, mutant=None):
        import tracer_kgrad_twin as tk
        from del4_twin import Del4Twin, TwinState
        assert mutant is None or mutant in B_MUTANTS
        self.tk, self.Del4Twin = tk, Del4Twin
        self.cfg, self.seed, self.mutant = cfg, seed, mutant
        self.mesh = get_mesh(cfg.meshname)
        self.om = orc.OracleMesh(self.mesh, cfg.K, resting_thickness_sum=resting_thickness(cfg).sum(1), max_level_edge_top=cfg.K)
        z = lambda f: np.zeros(shape_of(cfg, f))
        self.st = TwinState(z(F_SSH), z(F_U), z(F_H))
        for (f, l), a in initial_state(cfg, seed).items():
            self.prog(f)[l] = a.copy()
        self.twin = tk.KgradTwin(self.om, self.om, [])
        self.phis = [[], []]
        self.kappa, self.kappa4, self.source = [], [], []
        self.lag = None                # mutant "coeff_late": the coefficients the previous step ran with
        self.nonlinear, self.visc, self.visc4 = False, 0.0, 0
        self.ssh_loose = True
        self.tape = None
        self._last, self._changed = {}, {}
        self.pending = None

    def prog(self, f):
        if f in TEND:                  # the stage-4 tendencies of the last step (zeros before the first), read at level 1
            if self.st.tendU is None:
                self.st.tendU, self.st.tendH = np.zeros(shape_of(self.cfg, F_U)), np.zeros(shape_of(self.cfg, F_H))
            self._materialize()
            return [None, self.st.tendU if f == F_TENDU else self.st.tendH]
        return {F_SSH: self.st.ssh, F_U: self.st.u, F_H: self.st.h}[f]

    def _materialize(self):
        """Mutant "late": the stage-4 tendencies are formed at read time, under the terms in force then."""
        p, self.pending = self.pending, None
        if p is not None:
            self.twin.base = self._base()
            self.st.tendU, self.st.tendH = self.twin.dycore(*p)

    @property
    def nT(self):
        return len(self.phis[1])

    def _base(self):
        if not self.nonlinear:
            return self.om
        return self.Del4Twin(self.om, visc_del2=self.visc, visc_del4=visc_del4(self.cfg) if self.visc4 else 0.0,
                             scaling=del4_scaling(self.cfg) if self.visc4 == 2 else None)

    def _coeffs(self):
        n = self.nT
        return (list(self.kappa) + [0.0] * n)[:n], (list(self.kappa4) + [0.0] * n)[:n], (list(self.source) + [None] * n)[:n]

    def _step(self, dt, taped=False):
        st, tw = self.st, self.twin
        cur = self._coeffs()
        use = cur
        if self.mutant == "coeff_late":
            use = self.lag if self.lag is not None and len(self.lag[0]) == self.nT else cur
            self.lag = cur
        tw.kappa, tw.kappa4, tw.source = list(use[0]), list(use[1]), list(use[2])
        tw.base = self._base()
        if self.mutant == "ssh_stored" and self.ssh_loose and not self.nonlinear:
            tw.base = _StoredSsh(self.om, st.ssh[1])
        kept = [[a.copy() for a in (st.ssh[0], st.u[0], st.h[0])], [p.copy() for p in self.phis[0]]] if self.mutant == "prev_level_lost" else None
        tw.step_rk4(st, self.phis, dt)
        rec = tw.tape.pop()
        self.pending = rec["P"][3] if self.mutant == "late" else None
        if kept is not None:
            st.ssh[0], st.u[0], st.h[0] = kept[0]
            if len(kept[1]) == self.nT:
                self.phis[0] = kept[1]
        self.ssh_loose = False
        if taped:
            self.tape["rec"].append(rec)

    def keys(self):
        k = [(f, l) for f in PROG for l in (0, 1)] + [("tr", j, l) for j in range(self.nT) for l in (0, 1)]
        return k + ([] if self.mutant == "late" else [(f, 1) for f in TEND])

    def array(self, key):
        return self.phis[key[2]][key[1]] if key[0] == "tr" else self.prog(key[0])[key[1]]

    def apply(self, op):
        cfg, st, k, a, t = self.cfg, self.st, op.kind, op.args, self.tape
        dt, nT = cfg.dt, self.nT
        R = lambda code, name: Obs(k, code, refusal=name)
        if k == "set_tracers":
            if t is not None and a[0] > 0:
                return R(ERR_UNSUPPORTED, "set_tracers_tape")
            self.phis = [[np.zeros(shape_of(cfg, F_H)) for _ in range(a[0])] for _ in range(2)]
            self.kappa, self.kappa4, self.source = [], [], []
            return Obs(k, OK)
        if k == "tr_upload":
            self.phis[a[1]][a[0]] = tracer_values(cfg, a[2], a[3])
            return Obs(k, OK)
        if k == "tr_download":
            return Obs(k, OK, key=("tr", a[0], a[1]), value=self.phis[a[1]][a[0]].copy())
        if k in ("kappa", "kappa4"):
            v = coefficients(cfg, k, a[0], nT)
            setattr(self, k, [] if v is None else list(v))
            return Obs(k, OK)
        if k == "source":
            self.source = (list(self.source) + [None] * nT)[:nT]
            self.source[a[0]] = None if a[1] == "none" else tracer_values(cfg, a[1], a[2])
            return Obs(k, OK)
        if k in ("rk4", "rk4_s13"):
            n = 13 if (k == "rk4_s13" and nT == 0 and cfg.s13 and not (self.nonlinear and self.visc4)) else 16
            if n == 13:                # the dycore alone under key 7: the 13-stream twins of the oracle
                o = orc.OracleState(self.om, st.ssh[1], st.u[1], st.h[1])
                if self.nonlinear:
                    orc.OracleNonlinear(self.om, visc_del2=self.visc).step_rk4_s13(o, dt)
                else:
                    o.step_rk4_s13(dt)
                for l in (0, 1):
                    st.ssh[l], st.u[l], st.h[l] = o.ssh[l].copy(), o.u[l].copy(), o.h[l].copy()
                st.tendU, st.tendH = o.tendU.copy(), o.tendH.copy()
                self.ssh_loose, self.pending = False, None
            else:
                self._step(dt)
            return Obs(k, OK, value=n)
        if k == "run":
            if a[0] == 0:
                return R(ERR_UNSUPPORTED, "run_fe_tracers")
            for _ in range(a[1]):
                self._step(dt)
            return Obs(k, OK)
        if k == "fe":
            return R(ERR_UNSUPPORTED, "fe_tracers")
        if k == "tape_create":
            return R(ERR_UNSUPPORTED, "tape_tracers")
        if k == "advance":
            st.ssh[0], st.u[0], st.h[0] = st.ssh[1].copy(), st.u[1].copy(), st.h[1].copy()
            self.phis[0] = [p.copy() for p in self.phis[1]]
            return Obs(k, OK)
        if k == "nonlinear":
            self.nonlinear = bool(a[0])
            return Obs(k, OK)
        if k == "del2":
            if a[0] and not self.nonlinear:
                return R(ERR_UNSUPPORTED, "del2_without_nonlinear")
            self.visc = visc_del2(cfg) if a[0] else 0.0
            return Obs(k, OK)
        if k == "del4":
            if a[0] and not self.nonlinear:
                return R(ERR_UNSUPPORTED, "del4_without_nonlinear")
            self.visc4 = a[0]
            return Obs(k, OK)
        if k == "placement":
            return R(ERR_UNSUPPORTED, "placement_tape") if t is not None else Obs(k, OK)
        if k == "upload":
            self.prog(a[0])[a[1]] = values(cfg, a[0], a[2])
            if a[1] == 1 and a[0] in (F_SSH, F_H):
                self.ssh_loose = True
            return Obs(k, OK)
        if k in READ_KINDS:
            arr = self.prog(a[0])[a[1]]
            if k == "download":
                v = arr.copy()
            elif k == "rows":
                v = arr[list(a[2])].reshape(len(a[2]), -1).copy()
            else:
                c = np.ascontiguousarray(arr)
                v = float(orc.lib().oracle_sum_sq(orc._p(c), c.size))
            return Obs(k, OK, key=(a[0], a[1]), value=v)
        if k == "tr_tape_create":
            self.tape = dict(cap=a[0], nT=nT, rec=[], want=tuple(a[1]), kfl=dict(a[2]), seeded=False, X=None, G=None, W=None)
            return Obs(k, OK)
        if k == "tr_tape_destroy":
            self.tape = None
            return Obs(k, OK)
        if k == "tr_taped":
            if len(t["rec"]) >= t["cap"]:
                return R(ERR_ARG, "tape_full")
            if nT != t["nT"]:
                return R(ERR_ARG, "taped_count_changed")
            self._step(dt, taped=True)
            t["seeded"] = False
            return Obs(k, OK)
        if k == "tr_seed":
            t["X"] = [tracer_values(cfg, "seed", a[0] + 31 * j) for j in range(t["nT"])]
            t["seeded"] = True
            return Obs(k, OK)
        if k == "tr_sweep":
            if not t["seeded"]:
                return R(ERR_ARG, "sweep_unseeded")
            recs = t["rec"]
            if self.mutant == "coeff_late":            # the coefficients in force now, not those recorded
                kap, kap4, _ = self._coeffs()
                recs = [dict(r, kappa=list(kap), kappa4=list(kap4)) for r in recs]
            adj = self.tk.KgradAdjointTwin(self.twin)
            t["X"], t["G"], t["W"] = adj.sweep_kgrad(recs, [x.copy() for x in t["X"]], dict(t["kfl"]), tuple(t["want"]))
            t["rec"] = []
            return Obs(k, OK)
        if k == "x_download":
            return Obs(k, OK, key=("X", a[0]), value=t["X"][a[0]].copy())
        if k == "g_download":
            return Obs(k, OK, key=("G", a[0]), value=t["G"][a[0]].copy())
        if k in ("k_scalar", "k_density"):
            w = t["W"][a[0]][a[1] - 1]
            return Obs(k, OK, key=("W", a[0], a[1]), value=self.tk.host_sum(w) if k == "k_scalar" else w.copy())
        raise ValueError(f"unknown op {op}")

    def run(self, ops):
        out = []
        before = {key: self.array(key).copy() for key in self.keys()}
        self._last = dict(before)
        for op in ops:
            o = self.apply(op)
            if op.kind in B_READS:
                if o.rc == OK and o.key[0] not in ("X", "G", "W"):
                    o.fresh = o.key not in self._last or not np.array_equal(self._last[o.key], self.array(o.key))
                    o.after = frozenset(self._changed.get(o.key, ()))
                    self._changed[o.key] = set()
                    self._last[o.key] = self.array(o.key).copy()
            else:
                now = {key: self.array(key).copy() for key in self.keys()}
                for key, v in now.items():
                    if key not in before or not np.array_equal(before[key], v) or \
                            (o.rc == OK and op.kind in NON_ARRAY_OPS and self._changed.get(key)):
                        self._changed.setdefault(key, set()).add(op.kind)
                before = now
            out.append(o)
        return out


class TracerDevice:
    """Machine B through moka_hip.lib: one mesh per config, a fresh state per sequence."""

    def __init__(self, backend, cfg):
        import moka_hip as mk
        from moka_hip import lib as L
        self.L, self.lib, self.backend, self.cfg = L, L.lib(), backend, cfg
        hm = mk.HorzMesh(get_mesh(cfg.meshname))
        vm = mk.VerticalMesh(hm, nVertLevels=cfg.K, restingThickness=resting_thickness(cfg), multilayer=True)
        self.M = mk.Mesh(hm, vm, backend=backend, patch_cells=cfg.patch_cells)
        self.counters = {"sequences": 0, "rk4_steps": 0, "tracer_paths": set(), "adjoint_paths": set()}

    def close(self):
        self.M.close()

    def run(self, ops, seed):
        L, lib, cfg, ctx = self.L, self.lib, self.cfg, self.backend._h
        cnt = self.counters
        hS, hT = C.c_void_p(), C.c_void_p()
        out, nT, tapeNT = [], 0, 0
        key7 = C.c_int()
        L.check(lib.moka_get_tuning(7, C.byref(key7)))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        hfield = lambda: np.full(shape_of(cfg, F_H), np.nan)
        try:
            L.check(lib.moka_state_create(ctx, self.M._h, C.byref(hS)), ctx)
            for (f, l), a in initial_state(cfg, seed).items():
                L.check(lib.moka_state_upload(hS, f, l, L.f64(a)), ctx)
            for op in ops:
                k, a = op.kind, op.args
                value = None
                if k == "set_tracers":
                    rc = lib.moka_set_tracers(hS, a[0])
                    if rc == OK:
                        nT = a[0]
                elif k == "tr_upload":
                    rc = lib.moka_tracer_upload(hS, a[0], a[1], vp(tracer_values(cfg, a[2], a[3])))
                elif k == "tr_download":
                    value = hfield()
                    rc = lib.moka_tracer_download(hS, a[0], a[1], vp(value))
                elif k in ("kappa", "kappa4"):
                    v = coefficients(cfg, k, a[0], nT)
                    arr = None if v is None else np.asarray(v, dtype=np.float64)
                    fn = lib.moka_set_tracer_diffusion if k == "kappa" else lib.moka_set_tracer_biharmonic
                    rc = fn(hS, None if arr is None else vp(arr))
                elif k == "source":
                    rc = lib.moka_tracer_source_upload(hS, a[0], None if a[1] == "none" else vp(tracer_values(cfg, a[1], a[2])))
                elif k in ("rk4", "rk4_s13"):
                    if k == "rk4_s13":
                        L.check(lib.moka_set_tuning(7, 1))
                    try:
                        value = lib.moka_state_rk4_streams(hS)
                        rc = lib.moka_step_rk4(hS, cfg.dt)
                    finally:
                        if k == "rk4_s13":
                            L.check(lib.moka_set_tuning(7, key7.value))
                elif k == "run":
                    rc = lib.moka_run(hS, a[0], cfg.dt, a[1], a[2])
                elif k == "fe":
                    rc = lib.moka_step_fe(hS, cfg.dt, a[0])
                elif k == "tape_create":
                    h = C.c_void_p()
                    rc = lib.moka_tape_create(hS, a[0], C.byref(h))
                    if rc == OK:
                        lib.moka_tape_destroy(h)
                elif k == "advance":
                    rc = lib.moka_advance_time_levels(hS, a[0])
                elif k == "nonlinear":
                    rc = lib.moka_set_nonlinear(hS, a[0])
                elif k == "del2":
                    rc = lib.moka_set_viscosity_del2(hS, visc_del2(cfg) if a[0] else 0.0)
                elif k == "del4":
                    sc = del4_scaling(cfg) if a[0] == 2 else None
                    rc = lib.moka_set_viscosity_del4(hS, visc_del4(cfg) if a[0] else 0.0, None if sc is None else vp(sc))
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
                elif k == "tr_tape_create":
                    rc = lib.moka_tracer_tape_create(hS, a[0], C.byref(hT))
                    tapeNT = nT
                    for j in a[1]:
                        L.check(lib.moka_tracer_adjoint_want_source_gradient(hT, j, 1), ctx)
                    for j, bits in a[2]:
                        L.check(lib.moka_tracer_adjoint_want_diffusivity_gradient(hT, j, bits, 1), ctx)
                elif k == "tr_tape_destroy":
                    lib.moka_tracer_tape_destroy(hT)
                    hT, rc = C.c_void_p(), OK
                elif k == "tr_taped":
                    rc = lib.moka_step_rk4_tracer_taped(hT, cfg.dt)
                elif k == "tr_seed":
                    rc = OK
                    for j in range(tapeNT):
                        rc = rc or lib.moka_tracer_adjoint_seed(hT, j, vp(tracer_values(cfg, "seed", a[0] + 31 * j)))
                elif k == "tr_sweep":
                    rc = lib.moka_tracer_adjoint_sweep(hT)
                    if rc == OK:
                        cnt["adjoint_paths"].add(lib.moka_tracer_adjoint_path(hT))
                elif k == "x_download":
                    value = hfield()
                    rc = lib.moka_tracer_adjoint_download(hT, a[0], vp(value))
                elif k == "g_download":
                    value = hfield()
                    rc = lib.moka_tracer_adjoint_source_download(hT, a[0], vp(value))
                elif k == "k_scalar":
                    s = C.c_double(np.nan)
                    rc = lib.moka_tracer_adjoint_diffusivity_gradient(hT, a[0], a[1], C.byref(s))
                    value = s.value
                elif k == "k_density":
                    value = np.full(shape_of(cfg, F_SSH), np.nan)
                    rc = lib.moka_tracer_adjoint_diffusivity_density_download(hT, a[0], a[1], vp(value))
                else:
                    raise ValueError(f"unknown op {op}")
                if rc == OK and k in ("rk4", "rk4_s13", "run", "tr_taped") and nT > 0:
                    cnt["rk4_steps"] += a[1] if k == "run" else 1
                    cnt["tracer_paths"].add(lib.moka_state_tracer_path(hS))
                out.append(Obs(k, int(rc), value=value if rc == OK else None))
            cnt["sequences"] += 1
        finally:
            # either order is allowed for a tracer tape (include/moka_hip.h): alternate
            first, second = ((hT, lib.moka_tracer_tape_destroy), (hS, lib.moka_state_destroy))[::1 if seed % 2 else -1]
            for h, fn in (first, second):
                if h:
                    fn(h)
            lib.moka_set_kernel_variant(ctx, 0)
            lib.moka_set_tuning(7, key7.value)
        return out


# ---------------------------------------------------------------------------------------------------------------------------------
# triage on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def describe(o):
    if o.rc != OK:
        return f"status {o.rc}" + (f" ({o.refusal})" if o.refusal else "")
    if isinstance(o.value, np.ndarray):
        return f"{key_name(o.key)} shape {o.value.shape} crc32 {zlib.crc32(np.ascontiguousarray(o.value).tobytes()):08x}" + \
            ("" if o.fresh else " (unchanged since its last read)")
    if o.value is not None:
        return (f"{key_name(o.key)} " if o.key else "") + repr(o.value)
    return "ok"


def main(argv):
    if len(argv) < 2 or argv[0] not in CONFIGS:
        print(f"usage: call_sequences.py CONFIG SEED [--upto N]   (CONFIG: {' '.join(CONFIGS)})")
        return 2
    cfg, seed = CONFIGS[argv[0]], int(argv[1])
    ops = sequence(cfg, seed)
    if "--upto" in argv:
        ops = ops[:int(argv[argv.index("--upto") + 1]) + 1]
    for i, (op, o) in enumerate(zip(ops, model_of(cfg, seed).run(ops))):
        print(f"{i:2d} {str(op):44s} -> {describe(o)}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
