"""Host-side mirror of the MOKA.jl forward-model interface for the `MokaHIP` backend.

Every class/function names the reference definition it mirrors.  Arrays handed in and out are
numpy arrays in the reference's memory layout ((n, K) C-order == Julia (K, n)).  Device-resident
fields are exposed as `DeviceField` objects (the Julia shim's lazily synchronised arrays): reading
one downloads it, assigning to it uploads.
"""
from __future__ import annotations

import ctypes as C
import datetime as _dt
import math
import weakref

import numpy as np

from . import lib as L
from . import mpasio
from .config import ConfigGet, ConfigRead, GlobalConfig, yaml_config
from .timemanager import (Alarm, Clock, OneTimeAlarm, PeriodicAlarm, Second, advance, attachAlarm, changeTimeStep, isRinging,
                          mpas_create_clock, period_seconds, reset, setCurrentTime, stop)

__all__ = [
    "MokaHIP", "MokaError", "ForwardEuler", "RungeKutta4", "HorzMesh", "VerticalMesh", "Mesh", "ModelSetup",
    "PrognosticVars", "DiagnosticVars", "TendencyVars", "DeviceField",
    "GradientOnEdge", "DivergenceOnCell", "CurlOnVertex", "interpolateCell2Edge",
    "GradientOnEdge_vjp", "GradientOnEdge_jvp", "DivergenceOnCell_vjp", "DivergenceOnCell_jvp", "CurlOnVertex_vjp", "CurlOnVertex_jvp",
    "advanceTimeLevels", "diagnostic_compute", "computeNormalVelocityTendency", "computeLayerThicknessTendency",
    "computeTendency", "ocn_timestep", "ocn_run_loop", "run_steps", "ocn_init_from_arrays", "ocn_init_alarms",
    "Clock", "OneTimeAlarm", "PeriodicAlarm", "Alarm", "advance", "isRinging", "reset", "stop", "changeTimeStep",
    "attachAlarm", "setCurrentTime", "ocn_setup_clock", "ocn_setup_mesh", "ocn_init", "write_netcdf",
    "ConfigRead", "ConfigGet", "GlobalConfig", "AdjointTape", "set_nonlinear", "REFERENCE_COMPAT", "prognostic_vars_best_placement",
    "set_tracers", "Tracers", "TracerAdjointTape", "ForcedAdjointTape",
    "set_vertical_mixing", "vertical_mixing", "vertical_viscosity_field", "momentum_vmix_path",
    "quadratic_drag", "bottom_speed", "last_bottom_speed",
    "set_richardson_mixing", "richardson_mixing", "richardson_fields", "richardson_number",
]

MokaError = L.MokaError
REFERENCE_COMPAT = L.FE_REFERENCE_COMPAT


class ForwardEuler:      # abstract type ForwardEuler <: timeStepper   (time_integration.jl:4)
    pass


class RungeKutta4:       # abstract type RungeKutta4 <: timeStepper    (time_integration.jl:5)
    pass


class MokaHIP:
    """The backend tag (`struct MokaHIP <: KA.Backend` in the Julia shim); owns one moka_ctx.
    Replaces `backend = CUDABackend()` at src/driver/mpas_ocean.jl:28."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        L.check(L.lib().moka_ctx_create(int(device), C.byref(self._h)))
        self.device = device
        _own(self, L.lib().moka_ctx_destroy, self._h)

    def synchronize(self):           # KA.synchronize(backend)
        L.check(L.lib().moka_sync(self._h), self._h)

    def timer_start(self):
        L.check(L.lib().moka_timer_start(self._h), self._h)

    def timer_stop(self) -> float:
        ms = C.c_float()
        L.check(L.lib().moka_timer_stop(self._h, C.byref(ms)), self._h)
        return float(ms.value)

    def stage_timing(self, enable: bool):
        """Record HIP events around every stage launch of the RK4 steps that follow (moka_stage_timing)."""
        L.check(L.lib().moka_stage_timing(self._h, 1 if enable else 0), self._h)

    def stage_timing_read(self):
        """(mean ms of the stage-1..4 launches, number of steps recorded)."""
        ms, n = (C.c_double * 4)(), C.c_int64()
        L.check(L.lib().moka_stage_timing_read(self._h, ms, C.byref(n)), self._h)
        return [float(x) for x in ms], int(n.value)

    def mark(self):
        """One HIP event on the compute stream (moka_mark): n marks give n - 1 step times."""
        L.check(L.lib().moka_mark(self._h), self._h)

    def marks_reset(self):
        L.check(L.lib().moka_marks_reset(self._h), self._h)

    def marks_read(self):
        """ms between consecutive marks (synchronises the compute stream)."""
        n = C.c_int64()
        L.check(L.lib().moka_marks_read(self._h, 0, None, C.byref(n)), self._h)
        ms = (C.c_double * max(n.value, 1))()
        L.check(L.lib().moka_marks_read(self._h, n.value, ms, C.byref(n)), self._h)
        return [float(ms[i]) for i in range(n.value)]

    def bw_probe(self, nbytes=4 << 30, iters=5):
        """Same-run bandwidth calibration (moka_bw_probe): {copy_GBs, read_GBs, copy_GBs_mean} of this device right now."""
        g = (C.c_double * 4)()
        L.check(L.lib().moka_bw_probe(self._h, int(nbytes), int(iters), g), self._h)
        if nbytes <= 0:
            return {}
        s5 = C.c_double()
        L.check(L.lib().moka_bw_probe_streams(self._h, int(iters), C.byref(s5)), self._h)
        rr, gb = C.c_double(), C.c_double()
        L.check(L.lib().moka_bw_probe_reread(self._h, 128 << 20, 16, int(iters), C.byref(rr)), self._h)
        # the state-sized gather: at most 32 GiB and at most a quarter of what is free now (ranks may share a device, a
        # smaller GPU, placement candidates alive); a refused allocation is a missing figure, not an error of the run
        big = None
        try:
            import torch
            free_b = int(torch.cuda.mem_get_info(self.device)[0])
        except Exception:
            free_b = 32 << 30
        want = min(32 << 30, free_b // 4) & ~((1 << 24) - 1)
        if want >= (1 << 30) and L.lib().moka_bw_probe_gather_big(self._h, int(want), 3, C.byref(gb)) == L.OK:
            big = float(gb.value)
        return {"copy_GBs": float(g[0]), "read_GBs": float(g[1]), "copy_GBs_mean": float(g[2]),
                "gather_GBs": float(g[3]), "streams5_GBs": float(s5.value), "reread128_GBs": float(rr.value),
                "gather32G_GBs": big, "gather_big_bytes": int(want)}

    def pci_bus_id(self) -> str:
        buf = C.create_string_buffer(32)
        L.check(L.lib().moka_ctx_pci_bus_id(self._h, buf, 32), self._h)
        return buf.value.decode().lower()

    def set_kernel_variant(self, v: int):
        L.check(L.lib().moka_set_kernel_variant(self._h, int(v)), self._h)

    def close(self):
        if self._h:
            _release(self, L.lib().moka_ctx_destroy, self._h)
            self._h = C.c_void_p()


# ---------------------------------------------------------------------------------------------
# mesh  (src/infra/MPASMesh)
# ---------------------------------------------------------------------------------------------
class HorzMesh:
    """HorzMesh{PrimaryCells, DualCells, Edges} (HorzMesh.jl:45-49); `data` carries the SoA arrays
    with ASCII field names (moka_hip.meshgen.MeshData or anything with the same attributes)."""

    def __init__(self, data):
        self.data = data
        self.PrimaryCells = data
        self.DualCells = data
        self.Edges = data


class _ActiveLevels:     # ActiveLevels (VertMesh.jl:19-26)
    def __init__(self, n, top):
        self.Top = np.full(n, top, dtype=np.int32)
        self.Bot = np.full(n, top, dtype=np.int32)


class VerticalMesh:
    """VerticalMesh (VertMesh.jl:3-17).  `VerticalMesh(horz, nVertLevels=K)` is the unit-test
    constructor (:92-117: unit resting thickness, maxLevelEdge.Top all ones).  Passing
    `restingThickness` (nCells, K) mirrors the file constructor (:46-82).  `multilayer=True`
    selects the N3 semantics maxLevelEdge.Top = nVertLevels (the commented-out factor at :32)."""

    def __init__(self, horz: HorzMesh, nVertLevels: int = 1, restingThickness=None, multilayer: bool = False):
        m = horz.data
        self.nVertLevels = int(nVertLevels)
        self.minLevelCell = np.ones(m.nCells, dtype=np.int32)
        self.maxLevelCell = np.full(m.nCells, nVertLevels, dtype=np.int32)
        top = self.nVertLevels if multilayer else 1
        self.maxLevelEdge = _ActiveLevels(m.nEdges, top)
        self.maxLevelVertex = _ActiveLevels(m.nVertices, top)
        if restingThickness is None:
            self.restingThickness = np.ones(m.nCells)
            self.restingThicknessSum = np.ones(m.nCells)
        else:
            self.restingThickness = np.asarray(restingThickness, dtype=np.float64)
            self.restingThicknessSum = self.restingThickness.reshape(m.nCells, -1).sum(axis=1)   # sum(dims=1), :73


class Mesh:
    """struct Mesh{HM,VM} (MPASMesh.jl:19-24).  `Mesh(h, v, backend=...)` is
    Adapt.adapt_structure(backend, mesh) (:26): the library reorders and uploads the mesh."""

    def __init__(self, horz: HorzMesh, vert: VerticalMesh, backend: MokaHIP | None = None,
                 ordering: int = L.ORDER_DEFAULT, patch_cells: int = 0, state_bytes: int = 8):
        """state_bytes=4: the states on this mesh store every array of Prog, Diag and Tend as fp32 (fp64 arithmetic; RK4 and
        the one-call Forward-Euler step) -- BASELINE config 5, not a reference feature."""
        self.HorzMesh, self.VertMesh = horz, vert
        self.backend = backend
        self.state_bytes = int(state_bytes)
        self._h = C.c_void_p()
        if backend is not None:
            desc, keep = L.make_desc(horz.data, vert.nVertLevels, vert.restingThicknessSum,
                                     vert.maxLevelEdge.Top, ordering, patch_cells, state_bytes=state_bytes)
            L.check(L.lib().moka_mesh_create(backend._h, C.byref(desc), C.byref(self._h)), backend._h)
            _own(self, L.lib().moka_mesh_destroy, self._h, backend)

    def info(self) -> dict:
        inf = L.MeshInfo()
        L.check(L.lib().moka_mesh_info_get(self._h, C.byref(inf)))
        return inf.as_dict()

    def _need_device(self):
        if not self._h:
            raise MokaError(L.ERR_ARG, "Mesh is not on a MokaHIP backend (there is no CPU path in this package)")

    def close(self):
        if self._h:
            _release(self, L.lib().moka_mesh_destroy, self._h)
            self._h = C.c_void_p()


def _own(obj, destroy, handle, *keep_alive):
    """Destroy the library object when its Python owner is collected (or at interpreter exit), unless close() did it
    first.  `keep_alive` are the owners of what the object lives on (state -> mesh -> backend): the finalizer holds them,
    so the library objects go in dependency order."""
    h = C.c_void_p(handle.value)

    def fin(h=h, keep=keep_alive):
        destroy(h)
    obj._fin = weakref.finalize(obj, fin)


def _release(obj, destroy, handle):
    fin = getattr(obj, "_fin", None)
    if fin is not None and fin.alive:
        fin()                       # runs destroy exactly once
    else:
        destroy(handle)


class ModelSetup:        # struct ModelSetup(config, mesh, timeManager)  (ModelSetup.jl:4)
    def __init__(self, config, mesh, timeManager):
        self.config, self.mesh, self.timeManager = config, mesh, timeManager


# ---------------------------------------------------------------------------------------------
# operators  (src/ocn/Operators.jl) -- host arrays in, host arrays out, synchronous
# ---------------------------------------------------------------------------------------------
def _chk_arr(a, shape, name):
    if not isinstance(a, np.ndarray) or a.dtype != np.float64 or not a.flags.c_contiguous or a.shape != shape:
        raise MokaError(L.ERR_ARG, f"{name} must be a C-contiguous float64 array of shape {shape}")


def GradientOnEdge(grad, h, mesh: Mesh, backend=None, workgroupsize=64):
    """GradientOnEdge!(grad, hᵢ, Mesh; backend, workgroupsize)   Operators.jl:102"""
    mesh._need_device()
    m, K = mesh.HorzMesh.data, mesh.VertMesh.nVertLevels
    _chk_arr(grad, (m.nEdges, K), "grad"); _chk_arr(h, (m.nCells, K), "h")
    L.check(L.lib().moka_gradient_on_edge(mesh._h, L.f64(h), L.f64(grad)), mesh.backend._h)


def DivergenceOnCell(div, vecEdge, temp, mesh: Mesh, backend=None, nthreads=50):
    """DivergenceOnCell!(DivCell, VecEdge, temp, Mesh; backend, nthreads)   Operators.jl:46"""
    mesh._need_device()
    m, K = mesh.HorzMesh.data, mesh.VertMesh.nVertLevels
    _chk_arr(div, (m.nCells, K), "div"); _chk_arr(vecEdge, (m.nEdges, K), "VecEdge")
    if temp is not None:
        _chk_arr(temp, (m.nEdges, K), "temp")
    L.check(L.lib().moka_divergence_on_cell(mesh._h, L.f64(vecEdge), L.f64(temp) if temp is not None else None,
                                            L.f64(div)), mesh.backend._h)


def CurlOnVertex(curl, vecEdge, mesh: Mesh, backend=None):
    """CurlOnVertex!(CurlVertex, VecEdge, Mesh; backend)   Operators.jl:151 -- accumulates into `curl`"""
    mesh._need_device()
    m, K = mesh.HorzMesh.data, mesh.VertMesh.nVertLevels
    _chk_arr(curl, (m.nVertices, K), "curl"); _chk_arr(vecEdge, (m.nEdges, K), "VecEdge")
    L.check(L.lib().moka_curl_on_vertex(mesh._h, L.f64(vecEdge), L.f64(curl)), mesh.backend._h)


def interpolateCell2Edge(edgeValue, cellValue, mesh: Mesh, backend=None, nlev: int = 1):
    """interpolateCell2Edge!(edgeValue, cellValue, Mesh; backend)   Operators.jl:179 (level 1 only)"""
    mesh._need_device()
    m, K = mesh.HorzMesh.data, mesh.VertMesh.nVertLevels
    _chk_arr(edgeValue, (m.nEdges, K), "edgeValue"); _chk_arr(cellValue, (m.nCells, K), "cellValue")
    L.check(L.lib().moka_interpolate_cell2edge(mesh._h, L.f64(cellValue), L.f64(edgeValue), int(nlev)), mesh.backend._h)


# ---- reverse (vjp) and forward (jvp) mode of the operators: what Enzyme gives the reference for
# autodiff(Reverse / Forward, GradientOnEdge!, Duplicated(grad, d_grad), Duplicated(h, d_h), ...)
# (test/enzyme/test_Enzyme_Operators.jl:61-66, 82-87, 160-166, 182-188).  Arrays are the shadows, modified in place with
# Enzyme's conventions: input shadows accumulate, overwritten-output shadows are zeroed, the curl shadow stays. ----
def GradientOnEdge_vjp(d_grad, d_h, mesh: Mesh):
    mesh._need_device()
    m, K = mesh.HorzMesh.data, mesh.VertMesh.nVertLevels
    _chk_arr(d_grad, (m.nEdges, K), "d_grad"); _chk_arr(d_h, (m.nCells, K), "d_h")
    L.check(L.lib().moka_gradient_on_edge_vjp(mesh._h, L.f64(d_grad), L.f64(d_h)), mesh.backend._h)


def GradientOnEdge_jvp(d_grad, d_h, mesh: Mesh):
    mesh._need_device()
    m, K = mesh.HorzMesh.data, mesh.VertMesh.nVertLevels
    _chk_arr(d_grad, (m.nEdges, K), "d_grad"); _chk_arr(d_h, (m.nCells, K), "d_h")
    L.check(L.lib().moka_gradient_on_edge_jvp(mesh._h, L.f64(d_h), L.f64(d_grad)), mesh.backend._h)


def DivergenceOnCell_vjp(d_div, d_vecEdge, d_temp, mesh: Mesh):
    mesh._need_device()
    m, K = mesh.HorzMesh.data, mesh.VertMesh.nVertLevels
    _chk_arr(d_div, (m.nCells, K), "d_div"); _chk_arr(d_vecEdge, (m.nEdges, K), "d_VecEdge")
    if d_temp is not None:
        _chk_arr(d_temp, (m.nEdges, K), "d_temp")
    L.check(L.lib().moka_divergence_on_cell_vjp(mesh._h, L.f64(d_div), L.f64(d_vecEdge), L.f64(d_temp) if d_temp is not None else None),
            mesh.backend._h)


def DivergenceOnCell_jvp(d_div, d_vecEdge, d_temp, mesh: Mesh):
    mesh._need_device()
    m, K = mesh.HorzMesh.data, mesh.VertMesh.nVertLevels
    _chk_arr(d_div, (m.nCells, K), "d_div"); _chk_arr(d_vecEdge, (m.nEdges, K), "d_VecEdge")
    if d_temp is not None:
        _chk_arr(d_temp, (m.nEdges, K), "d_temp")
    L.check(L.lib().moka_divergence_on_cell_jvp(mesh._h, L.f64(d_vecEdge), L.f64(d_temp) if d_temp is not None else None, L.f64(d_div)),
            mesh.backend._h)


def CurlOnVertex_vjp(d_curl, d_vecEdge, mesh: Mesh):
    mesh._need_device()
    m, K = mesh.HorzMesh.data, mesh.VertMesh.nVertLevels
    _chk_arr(d_curl, (m.nVertices, K), "d_curl"); _chk_arr(d_vecEdge, (m.nEdges, K), "d_VecEdge")
    L.check(L.lib().moka_curl_on_vertex_vjp(mesh._h, L.f64(d_curl), L.f64(d_vecEdge)), mesh.backend._h)


def CurlOnVertex_jvp(d_curl, d_vecEdge, mesh: Mesh):
    mesh._need_device()
    m, K = mesh.HorzMesh.data, mesh.VertMesh.nVertLevels
    _chk_arr(d_curl, (m.nVertices, K), "d_curl"); _chk_arr(d_vecEdge, (m.nEdges, K), "d_VecEdge")
    L.check(L.lib().moka_curl_on_vertex_jvp(mesh._h, L.f64(d_vecEdge), L.f64(d_curl)), mesh.backend._h)


# ---------------------------------------------------------------------------------------------
# state containers  (PrognosticVars.jl, DiagnosticVars.jl, TendencyVars.jl)
# ---------------------------------------------------------------------------------------------
class _State:
    """One moka_state shared by Prog / Diag / Tend of a model instance."""

    def __init__(self, mesh: Mesh):
        mesh._need_device()
        self.mesh = mesh
        self._h = C.c_void_p()
        L.check(L.lib().moka_state_create(mesh.backend._h, mesh._h, C.byref(self._h)), mesh.backend._h)
        _own(self, L.lib().moka_state_destroy, self._h, mesh, mesh.backend)
        self._dependents = []          # weak references to tapes on this state: they dereference it when they are destroyed

    FIELD_NAMES = ("cur.normalVelocity", "cur.layerThickness", "cur.ssh", "prev.normalVelocity", "prev.layerThickness", "prev.ssh",
                   "rk1.normalVelocity", "rk1.layerThickness", "rk1.ssh", "rk2.normalVelocity", "rk2.layerThickness", "rk2.ssh")

    def optimize_placement(self, max_tries: int = 24) -> dict:
        """moka_state_optimize_placement: re-allocate one array at a time where that makes the RK4 stage launches faster
        (the state's contents are unchanged).  Returns {ms_before, ms_after, tries, kept, trials: [...]}; must come before
        a halo or a tape is created on the state."""
        b, a, n = C.c_double(), C.c_double(), C.c_int32()
        ctx = self.mesh.backend._h
        L.check(L.lib().moka_state_optimize_placement(self._h, int(max_tries), C.byref(b), C.byref(a)), ctx)
        L.check(L.lib().moka_state_placement_log(self._h, 0, None, C.byref(n)), ctx)
        buf = (L.PlacementTrial * max(n.value, 1))()
        L.check(L.lib().moka_state_placement_log(self._h, n.value, buf, C.byref(n)), ctx)
        trials = [{"field": self.FIELD_NAMES[t.field], "ms_old": float(t.ms_old), "ms_new": float(t.ms_new), "kept": bool(t.kept)}
                  for t in buf[:n.value]]
        return {"ms_before": float(b.value), "ms_after": float(a.value), "tries": int(n.value),
                "stage_launches": int(L.lib().moka_state_placement_launches(self._h)),
                "kept": sum(t["kept"] for t in trials), "trials": trials}

    def close(self):
        if self._h:
            for ref in self._dependents:      # an explicit close() takes what lives on the state with it, in order
                dep = ref()
                if dep is not None:
                    dep.close()
            self._dependents = []
            _release(self, L.lib().moka_state_destroy, self._h)
            self._h = C.c_void_p()


class DeviceField:
    """A field resident in HBM; `np.asarray(f)` / `f.get()` downloads, `f.set(a)` uploads
    (Adapt.adapt(backend, a) / Adapt.adapt(KA.CPU(), a))."""

    def __init__(self, state: _State, field: int, level: int, shape):
        self._s, self.field, self.level, self.shape = state, field, level, tuple(shape)

    def get(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=np.float64)
        L.check(L.lib().moka_state_download(self._s._h, self.field, self.level, L.f64(out)), self._s.mesh.backend._h)
        return out

    def set(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != self.shape:
            a = a.reshape(self.shape)
        L.check(L.lib().moka_state_upload(self._s._h, self.field, self.level, L.f64(a)), self._s.mesh.backend._h)

    def rows(self, ids, level=None) -> np.ndarray:
        """Selected rows (the caller's ids) of the field: (len(ids), K), or (len(ids),) for ssh (moka_state_download_rows).
        level: 0 / 1 time levels (default: this field's), 2 / 3 the RK4 provisional states (inspection)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        K = self.shape[1] if len(self.shape) == 2 else 1
        out = np.empty((ids.size, K), dtype=np.float64)
        L.check(L.lib().moka_state_download_rows(self._s._h, self.field, self.level if level is None else int(level), ids.size,
                                                 L.i32(ids), L.f64(out)), self._s.mesh.backend._h)
        return out if len(self.shape) == 2 else out[:, 0]

    def __array__(self, dtype=None, copy=None):
        return self.get()

    @property
    def size(self):
        return int(np.prod(self.shape))


class PrognosticVars:
    """PrognosticVars (PrognosticVars.jl:6-57): ssh / normalVelocity / layerThickness, each a
    Vector of nTimeLevels (= 2) arrays; index 0 = previous, -1 = current (Julia 1 / end)."""

    def __init__(self, ssh, normalVelocity, layerThickness, nTimeLevels, mesh: Mesh, state: _State | None = None):
        if nTimeLevels != 2:
            raise MokaError(L.ERR_ARG, "nTimeLevels must be <= 2")       # time_integration.jl:23
        m, K = mesh.HorzMesh.data, mesh.VertMesh.nVertLevels
        self._state = state or _State(mesh)
        s = self._state
        self.ssh = [DeviceField(s, L.F_SSH, t, (m.nCells,)) for t in range(2)]
        self.normalVelocity = [DeviceField(s, L.F_NORMAL_VELOCITY, t, (m.nEdges, K)) for t in range(2)]
        self.layerThickness = [DeviceField(s, L.F_LAYER_THICKNESS, t, (m.nCells, K)) for t in range(2)]
        for t in range(2):           # deepcopy into every time level (:50-54)
            self.ssh[t].set(ssh)
            self.normalVelocity[t].set(normalVelocity)
            self.layerThickness[t].set(layerThickness)


class DiagnosticVars:
    """DiagnosticVars (DiagnosticVars.jl:6-73), zero-initialised on the backend (:90-93)."""

    def __init__(self, config, mesh: Mesh, state: _State):
        m, K = mesh.HorzMesh.data, mesh.VertMesh.nVertLevels
        self._state = state
        self.layerThicknessEdge = DeviceField(state, L.F_LAYER_THICKNESS_EDGE, 1, (m.nEdges, K))
        self.thicknessFlux = DeviceField(state, L.F_THICKNESS_FLUX, 1, (m.nEdges, K))
        self.velocityDivCell = DeviceField(state, L.F_VELOCITY_DIV_CELL, 1, (m.nCells, K))
        self.relativeVorticity = DeviceField(state, L.F_RELATIVE_VORTICITY, 1, (m.nVertices, K))


class TendencyVars:
    """TendencyVars (TendencyVars.jl:7-49)."""

    def __init__(self, config, mesh: Mesh, state: _State):
        m, K = mesh.HorzMesh.data, mesh.VertMesh.nVertLevels
        self._state = state
        self.tendNormalVelocity = DeviceField(state, L.F_TEND_NORMAL_VELOCITY, 1, (m.nEdges, K))
        self.tendLayerThickness = DeviceField(state, L.F_TEND_LAYER_THICKNESS, 1, (m.nCells, K))


# ---------------------------------------------------------------------------------------------
# forward model  (src/forward, src/ocn/DiagnosticVars.jl, src/ocn/Tendencies)
# ---------------------------------------------------------------------------------------------
def _st(x):
    return x._state._h, x._state.mesh.backend._h


def advanceTimeLevels(Prog: PrognosticVars, backend=None):
    """advanceTimeLevels!(Prog; backend)   time_integration.jl:10"""
    h, c = _st(Prog)
    L.check(L.lib().moka_advance_time_levels(h, 0), c)


def diagnostic_compute(mesh: Mesh, Diag: DiagnosticVars, Prog: PrognosticVars, backend=None,
                       flags: int = REFERENCE_COMPAT):
    """diagnostic_compute!(Mesh, Diag, Prog; backend)   DiagnosticVars.jl:108"""
    h, c = _st(Prog)
    L.check(L.lib().moka_diagnostic_compute(h, flags), c)


def computeNormalVelocityTendency(Tend, Prog, Diag, mesh, Config=None, backend=None, flags: int = REFERENCE_COMPAT):
    """computeNormalVelocityTendency!(Tend, Prog, Diag, Mesh, Config; backend)   normalVelocity.jl:21"""
    h, c = _st(Prog)
    L.check(L.lib().moka_compute_normal_velocity_tendency(h, flags), c)


def computeLayerThicknessTendency(Tend, Prog, Diag, mesh, Config=None, backend=None, flags: int = REFERENCE_COMPAT):
    """computeLayerThicknessTendency!(Tend, Prog, Diag, Mesh, Config; backend)   layerThickness.jl:14"""
    h, c = _st(Prog)
    L.check(L.lib().moka_compute_layer_thickness_tendency(h, flags), c)


def computeTendency(mesh, Diag, Prog, Tend):
    """The helper the reference's RK4 calls but never defines (time_integration.jl:114-115): one
    fused tendency evaluation (u,h) -> (tendU,tendH) with consistent diagnostics."""
    h, c = _st(Prog)
    L.check(L.lib().moka_tendencies(h), c)


def ocn_timestep(*args, backend=None, flags: int | None = None):
    """ocn_timestep(timestep, Prog, Diag, Tend, S, ForwardEuler; backend)   time_integration.jl:150
       ocn_timestep(Prog, Diag, Tend, S, RungeKutta4; backend)              time_integration.jl:61
    `timestep` is the reference's 1-element array (mpas_ocean.jl:36-37) or a float."""
    if len(args) == 6:
        timestep, Prog, Diag, Tend, S, method = args
    elif len(args) == 5:
        Prog, Diag, Tend, S, method = args
        timestep = float(S.timeManager.timeStep.total_seconds())       # :75
    else:
        raise MokaError(L.ERR_ARG, "ocn_timestep: wrong number of arguments")
    dt = float(np.asarray(timestep).reshape(-1)[0])
    h, c = _st(Prog)
    if method is ForwardEuler:
        L.check(L.lib().moka_step_fe(h, dt, REFERENCE_COMPAT if flags is None else flags), c)
    elif method is RungeKutta4:
        L.check(L.lib().moka_step_rk4(h, dt), c)
    else:
        raise MokaError(L.ERR_ARG, "unknown timeStepper")


def run_steps(Prog, method, dt: float, nsteps: int, flags: int = REFERENCE_COMPAT):
    """nsteps x ocn_timestep in one library call (moka_run): the body of ocn_run_loop (run_loop.jl:11-19) without
    the host-side alarm bookkeeping; long runs are replayed from a hipGraph."""
    h, c = _st(Prog)
    integ = L.FORWARD_EULER if method is ForwardEuler else L.RUNGE_KUTTA_4
    L.check(L.lib().moka_run(h, integ, float(dt), int(nsteps), int(flags)), c)


def ocn_run_loop(*args, backend=None, flags: int | None = None):
    """ocn_run_loop(timestep, Prog, Diag, Tend, Setup, ForwardEuler, clock, simulationAlarm, outputAlarm)
    (run_loop.jl:8-22) and the (sumCPU, sumGPU, ...) variant (:26-45) that returns sum(ssh^2)."""
    want_sum = len(args) == 11
    if want_sum:
        sumCPU, sumGPU, *args = args
    timestep, Prog, Diag, Tend, Setup, method, clock, simulationAlarm, outputAlarm = args
    while not isRinging(simulationAlarm):
        advance(clock)
        ocn_timestep(timestep, Prog, Diag, Tend, Setup, method, flags=flags)
        if isRinging(outputAlarm):
            reset(outputAlarm)
    if want_sum:
        out = C.c_double()
        h, c = _st(Prog)
        L.check(L.lib().moka_sum_sq(h, L.F_SSH, 1, C.byref(out)), c)
        sumCPU[0] = out.value
        return out.value
    return None


def prognostic_vars_best_placement(ssh, normalVelocity, layerThickness, nTimeLevels, mesh: "Mesh", tries: int = 24, report: dict | None = None):
    """PrognosticVars(...) followed by the library's own placement search (moka_state_optimize_placement, include/moka_hip.h):
    where the allocator puts a state's arrays decides 5-14 % of every stage launch, so the library re-allocates
    one array at a time -- at most `tries` times -- and keeps what makes the RK4 stage launches faster.  The state is, array for
    array and flag for flag, what a fresh PrognosticVars(...) holds (round 3 did the search here, over whole candidate states, and
    left the trial steps' traces in the kept one: ADVICE r03).  tries <= 1: no search."""
    P = PrognosticVars(ssh, normalVelocity, layerThickness, nTimeLevels, mesh)
    rep = {"tries": 0, "trials": [], "kept": 0}
    if int(tries) > 1:
        try:
            rep = P._state.optimize_placement(int(tries))
        except MokaError as exc:               # an optimisation: no memory for a candidate etc. leaves the state as it was
            if exc.code not in (L.ERR_ALLOC, L.ERR_HIP):
                raise
            rep["error"] = str(exc)
    if report is not None:
        report.update(rep)
    return P


def ocn_init_from_arrays(mesh_data, ssh, normalVelocity, layerThickness, restingThickness, config: dict,
                         backend: MokaHIP, multilayer: bool = False, ordering: int = L.ORDER_DEFAULT,
                         patch_cells: int = 0, state_bytes: int = 8, placement_tries: int = 1, placement_report: dict | None = None):
    """ocn_init(config_fp; backend) (init.jl:3-30) with the NetCDF/YAML reads replaced by arrays:
    returns (Setup, Diag, Tend, Prog) like the reference.  placement_tries > 1: see prognostic_vars_best_placement."""
    K = np.asarray(normalVelocity).reshape(mesh_data.nEdges, -1).shape[1]
    h_mesh = HorzMesh(mesh_data)
    v_mesh = VerticalMesh(h_mesh, nVertLevels=K, restingThickness=restingThickness, multilayer=multilayer)
    mesh = Mesh(h_mesh, v_mesh, backend=backend, ordering=ordering, patch_cells=patch_cells, state_bytes=state_bytes)
    clock = ocn_setup_clock(config)
    Setup = ModelSetup(config, mesh, clock)
    Prog = prognostic_vars_best_placement(ssh, normalVelocity, layerThickness,
                                          config.get("time_integration", {}).get("config_number_of_time_levels", 2), mesh,
                                          tries=placement_tries, report=placement_report)
    Diag = DiagnosticVars(config, mesh, Prog._state)
    Tend = TendencyVars(config, mesh, Prog._state)
    return Setup, Diag, Tend, Prog


def set_nonlinear(Prog: "PrognosticVars", on: bool = True, visc_del2: float = 0.0, visc_del4: float = 0.0,
                  mesh_scaling_del4=None):
    """Switch the optional nonlinear terms (potential-vorticity Coriolis, kinetic-energy gradient) of this model's
    tendencies / RK4 steps on or off.  An extension: the reference has only the linear terms; default off.
    `visc_del2` != 0 adds Del2 momentum mixing (the reference's uncalled sketch, horizontal_momentum_mixing.jl:53-80).
    `visc_del4` != 0 adds Del4 (biharmonic) mixing, subtracted last (moka_set_viscosity_del4); `mesh_scaling_del4`: None or one
    factor >= 0 per edge, in the mesh's edge order."""
    L.check(L.lib().moka_set_nonlinear(Prog._state._h, 1 if on else 0), Prog._state.mesh.backend._h)
    Prog._state.nonlinear = bool(on)
    if on:
        L.check(L.lib().moka_set_viscosity_del2(Prog._state._h, float(visc_del2)), Prog._state.mesh.backend._h)
        sc = None
        if mesh_scaling_del4 is not None:
            sc = np.ascontiguousarray(mesh_scaling_del4, dtype=np.float64).reshape(-1)
            nE = Prog._state.mesh.HorzMesh.data.nEdges
            if sc.size != nE:
                raise ValueError(f"mesh_scaling_del4: {sc.size} values for {nE} edges")
        L.check(L.lib().moka_set_viscosity_del4(Prog._state._h, float(visc_del4), None if sc is None else sc.ctypes.data),
                Prog._state.mesh.backend._h)


def set_vertical_mixing(Prog: "PrognosticVars", viscosity: float = 0.0, bottom_drag: float = 0.0, surface_stress=None, viscosity_field=None,
                        quadratic_drag: float = 0.0):
    """Implicit vertical mixing of momentum behind every RK4 step (moka_set_vertical_viscosity, moka_surface_stress_upload; an
    extension, default off; include/moka_hip.h states the recipe).  `viscosity`: nuV >= 0 in m^2/s; `bottom_drag`: a linear drag
    r >= 0 in m/s on the deepest active level of every edge; `surface_stress`: None, or one value tau / rho0 (m^2/s^2) per edge along
    the edge normal, in the mesh's edge order; `viscosity_field`: None, or an (nEdges, nVertLevels) array of nuV >= 0 per interface and
    edge (moka_vertical_viscosity_field_upload: row k of an edge column is the interface between levels k and k + 1, rows at and below
    the deepest interface are never read), which sets `viscosity` aside while it is there; `quadratic_drag`: Cd >= 0, dimensionless
    (moka_set_quadratic_bottom_drag: the drag coefficient of an edge becomes r + Cd * the speed of the flow at its bottom level).  All
    five are replaced by a call: zeros and None switch the pass off.  They take effect with the next RK4 step or run_steps."""
    st = Prog._state
    h = st.mesh.backend._h
    tau = fld = None                     # both arrays are checked before the first call: a bad shape changes nothing
    if surface_stress is not None:
        tau = np.ascontiguousarray(surface_stress, dtype=np.float64).reshape(-1)
        nE = st.mesh.HorzMesh.data.nEdges
        if tau.size != nE:
            raise ValueError(f"surface_stress: {tau.size} values for {nE} edges")
    if viscosity_field is not None:
        fld = np.ascontiguousarray(viscosity_field, dtype=np.float64)
        shape = tuple(Prog.normalVelocity[-1].shape)
        if fld.shape != shape:
            raise ValueError(f"viscosity_field: shape {fld.shape}, expected {shape}")
    L.check(L.lib().moka_set_vertical_viscosity(st._h, float(viscosity), float(bottom_drag)), h)
    L.check(L.lib().moka_set_quadratic_bottom_drag(st._h, float(quadratic_drag)), h)
    L.check(L.lib().moka_surface_stress_upload(st._h, None if tau is None else tau.ctypes.data), h)
    L.check(L.lib().moka_vertical_viscosity_field_upload(st._h, None if fld is None else fld.ctypes.data), h)


def vertical_viscosity_field(Prog: "PrognosticVars"):
    """The viscosity field as it stands, (nEdges, nVertLevels), or None when there is none."""
    st = Prog._state
    h = st.mesh.backend._h
    has = C.c_int(0)
    L.check(L.lib().moka_has_vertical_viscosity_field(st._h, C.byref(has)), h)
    if not has.value:
        return None
    fld = np.empty(tuple(Prog.normalVelocity[-1].shape), dtype=np.float64)
    L.check(L.lib().moka_vertical_viscosity_field_download(st._h, L.f64(fld)), h)
    return fld


def vertical_mixing(Prog: "PrognosticVars"):
    """(viscosity, bottom_drag, surface_stress) as they stand: the stress as an array of nEdges values, or None when there is none."""
    st = Prog._state
    h = st.mesh.backend._h
    nu, r, has = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
    L.check(L.lib().moka_vertical_viscosity(st._h, C.byref(nu), C.byref(r)), h)
    L.check(L.lib().moka_has_surface_stress(st._h, C.byref(has)), h)
    if not has.value:
        return nu.value, r.value, None
    tau = np.empty(st.mesh.HorzMesh.data.nEdges, dtype=np.float64)
    L.check(L.lib().moka_surface_stress_download(st._h, L.f64(tau)), h)
    return nu.value, r.value, tau


def quadratic_drag(Prog: "PrognosticVars") -> float:
    """Cd of the quadratic bottom drag as it stands (moka_quadratic_bottom_drag)."""
    cd = C.c_double(0.0)
    L.check(L.lib().moka_quadratic_bottom_drag(Prog._state._h, C.byref(cd)), Prog._state.mesh.backend._h)
    return cd.value


def bottom_speed(Prog: "PrognosticVars", time_level: int = 1):
    """The bottom speed sp[e] of the quadratic drag's recipe from normalVelocity of `time_level` (1 current, 0 previous), nEdges
    values, computed on the device without a step (moka_bottom_speed)."""
    st = Prog._state
    sp = np.empty(st.mesh.HorzMesh.data.nEdges, dtype=np.float64)
    L.check(L.lib().moka_bottom_speed(st._h, int(time_level), L.f64(sp)), st.mesh.backend._h)
    return sp


def last_bottom_speed(Prog: "PrognosticVars"):
    """The bottom speed the last vertical pass used, nEdges values; zeros when it ran without a quadratic drag
    (moka_bottom_speed_download)."""
    st = Prog._state
    sp = np.empty(st.mesh.HorzMesh.data.nEdges, dtype=np.float64)
    L.check(L.lib().moka_bottom_speed_download(st._h, L.f64(sp)), st.mesh.backend._h)
    return sp


def _tracer_count(st) -> int:
    """moka_tracer_count: the state's own count (a raw moka_set_tracers call changes it behind every Python object)."""
    n = C.c_int32(0)
    L.check(L.lib().moka_tracer_count(st._h, C.byref(n)), st.mesh.backend._h)
    return int(n.value)


def set_richardson_mixing(Prog: "PrognosticVars", buoyancy, nu0: float = 0.005, alpha: float = 5.0, background_viscosity: float = 1e-4,
                          background_diffusivity: float = 1e-5, convective: float = 1.0, tracers=None):
    """The Richardson-number closure of both vertical passes (moka_set_richardson_mixing; an extension, default off;
    include/moka_hip.h states the recipe): behind stage 4 of every RK4 step the viscosity per interface and edge and the diffusivity
    per interface and cell are computed on the device from the new level and handed to the momentum pass and the tracer pass.
    `buoyancy`: the index of the tracer that carries b = -g (rho - rho0) / rho0 in m/s^2, or None to switch the closure off; `nu0`,
    `alpha`, `background_viscosity`, `background_diffusivity`, `convective`: the Pacanowski-Philander parameters, all >= 0 (the
    defaults are MPAS-Ocean's); `tracers`: the indices of the tracers that take the closure's diffusivity (None: every tracer).
    The viscosity, viscosity field, vertical diffusivities and diffusivity fields set elsewhere are kept and act again when the
    closure is switched off.  Takes effect with the next RK4 step or run_steps."""
    st = Prog._state
    h = st.mesh.backend._h
    if buoyancy is None:
        L.check(L.lib().moka_set_richardson_mixing(st._h, None), h)
        return
    n = _tracer_count(st)
    mask = None
    if tracers is not None:
        mask = np.zeros(n, dtype=np.int32)
        for j in tracers:
            if not 0 <= int(j) < n:
                raise ValueError(f"tracers: index {j} for {n} tracers")
            mask[int(j)] = 1
    p = L.RichardsonParams(int(buoyancy), float(nu0), float(alpha), float(background_viscosity), float(background_diffusivity),
                           float(convective), None if mask is None else mask.ctypes.data)
    L.check(L.lib().moka_set_richardson_mixing(st._h, C.byref(p)), h)


def richardson_mixing(Prog: "PrognosticVars"):
    """The closure as it stands (moka_richardson_mixing): None while it is off, else a dict with the keyword names of
    set_richardson_mixing (`tracers`: the sorted indices of the set)."""
    st = Prog._state
    on, p = C.c_int(0), L.RichardsonParams()
    n = _tracer_count(st)
    mask = np.zeros(max(n, 1), dtype=np.int32)
    L.check(L.lib().moka_richardson_mixing(st._h, C.byref(on), C.byref(p), mask.ctypes.data), st.mesh.backend._h)
    if not on.value:
        return None
    return {"buoyancy": int(p.buoyancyTracer), "nu0": p.nu0, "alpha": p.alpha, "background_viscosity": p.nuBackground,
            "background_diffusivity": p.kappaBackground, "convective": p.convective, "tracers": [j for j in range(n) if mask[j]]}


def _richardson_shapes(Prog):
    eshape = tuple(Prog.normalVelocity[-1].shape)
    return eshape, tuple(Prog.layerThickness[-1].shape)


def richardson_fields(Prog: "PrognosticVars"):
    """(F, G) the last RK4 step computed (moka_richardson_fields_download): the viscosity, (nEdges, nVertLevels), and the
    diffusivity, (nCells, nVertLevels); row k is the interface between levels k and k + 1.  Zeros when that step ran without the
    closure."""
    st = Prog._state
    eshape, cshape = _richardson_shapes(Prog)
    F, G = np.empty(eshape, dtype=np.float64), np.empty(cshape, dtype=np.float64)
    L.check(L.lib().moka_richardson_fields_download(st._h, L.f64(F), L.f64(G)), st.mesh.backend._h)
    return F, G


def richardson_number(Prog: "PrognosticVars", time_level: int = 1):
    """(RiEdge, RiCell) of the closure's recipe from time level `time_level` (1 current, 0 previous), computed on the device without
    a step (moka_richardson_diagnose); the closure must be on: it names the buoyancy tracer."""
    st = Prog._state
    eshape, cshape = _richardson_shapes(Prog)
    rE, rC = np.empty(eshape, dtype=np.float64), np.empty(cshape, dtype=np.float64)
    L.check(L.lib().moka_richardson_diagnose(st._h, int(time_level), L.f64(rE), L.f64(rC), None, None), st.mesh.backend._h)
    return rE, rC


def momentum_vmix_path(Prog: "PrognosticVars") -> int:
    """moka_state_momentum_vmix_path: 1 the tile form, 2 the column form of the momentum pass, 0 before the first one."""
    return int(L.lib().moka_state_momentum_vmix_path(Prog._state._h))


class Tracers:
    """The passive tracers of a model (set_tracers): cell-centred (nCells, K) fields carried by every RK4 step."""

    def __init__(self, state: "_State", n: int, shape):
        self._s, self.n, self.shape = state, int(n), tuple(shape)

    def get(self, j: int, level: int = -1) -> np.ndarray:
        """Tracer j at time level `level` (0 = previous, -1 / 1 = current)."""
        out = np.empty(self.shape, dtype=np.float64)
        L.check(L.lib().moka_tracer_download(self._s._h, int(j), level % 2, L.f64(out)), self._s.mesh.backend._h)
        return out

    def set(self, j: int, a, level: int = -1):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != self.shape:
            a = a.reshape(self.shape)
        L.check(L.lib().moka_tracer_upload(self._s._h, int(j), level % 2, L.f64(a)), self._s.mesh.backend._h)

    def path(self) -> int:
        """moka_state_tracer_path: 1 the patch form, 2 the generic form of the tracer kernel, 0 before the first RK4 step."""
        return int(L.lib().moka_state_tracer_path(self._s._h))

    def set_diffusivity(self, values):
        """moka_set_tracer_diffusion: harmonic diffusion div(kappa h_e grad phi) beside the transport.  `values`: one diffusivity
        (m^2/s, finite, >= 0) for every tracer or one per tracer; None or 0 switches diffusion off.  Takes effect with the next RK4
        step or run.  The explicit stability limit (kappa dt / dcEdge_min^2 <~ 0.35) is not checked."""
        k = None
        if values is not None:
            k = np.asarray(values, dtype=np.float64)
            k = np.full(self.n, float(k)) if k.ndim == 0 else np.ascontiguousarray(k.ravel())
            if k.size != self.n:
                raise ValueError(f"diffusivity: {k.size} values for {self.n} tracers")
        if k is not None and self.n == 0 and not k.size:
            k = None
        L.check(L.lib().moka_set_tracer_diffusion(self._s._h, None if k is None else k.ctypes.data), self._s.mesh.backend._h)

    def diffusivity(self) -> np.ndarray:
        """moka_tracer_diffusion: the diffusivity of every tracer (zeros unless set_diffusivity was called)."""
        out = np.zeros(self.n, dtype=np.float64)
        v = C.c_double()
        for j in range(self.n):
            L.check(L.lib().moka_tracer_diffusion(self._s._h, j, C.byref(v)), self._s.mesh.backend._h)
            out[j] = v.value
        return out

    def set_biharmonic(self, values):
        """moka_set_tracer_biharmonic: biharmonic diffusion -div(kappa4 h_e grad L), L the thickness-weighted Laplacian of phi, beside
        the transport and the harmonic term.  `values`: one coefficient (m^4/s, finite, >= 0) for every tracer or one per tracer; None
        or 0 switches it off.  Takes effect with the next RK4 step or run.  The explicit stability limit
        (kappa4 dt / dcEdge_min^4 <~ 0.043, shared with the harmonic part) is not checked."""
        k = None
        if values is not None:
            k = np.asarray(values, dtype=np.float64)
            k = np.full(self.n, float(k)) if k.ndim == 0 else np.ascontiguousarray(k.ravel())
            if k.size != self.n:
                raise ValueError(f"biharmonic: {k.size} values for {self.n} tracers")
        if k is not None and self.n == 0 and not k.size:
            k = None
        L.check(L.lib().moka_set_tracer_biharmonic(self._s._h, None if k is None else k.ctypes.data), self._s.mesh.backend._h)

    def biharmonic(self) -> np.ndarray:
        """moka_tracer_biharmonic: the biharmonic coefficient of every tracer (zeros unless set_biharmonic was called)."""
        out = np.zeros(self.n, dtype=np.float64)
        v = C.c_double()
        for j in range(self.n):
            L.check(L.lib().moka_tracer_biharmonic(self._s._h, j, C.byref(v)), self._s.mesh.backend._h)
            out[j] = v.value
        return out

    def set_vertical_diffusivity(self, values):
        """moka_set_tracer_vertical_diffusion: implicit vertical diffusion, a backward-Euler solve per column behind the RK4 step
        (include/moka_hip.h states the recipe).  `values`: one diffusivity (m^2/s, finite, >= 0) for every tracer or one per tracer;
        None or 0 switches it off.  Takes effect with the next RK4 step or run; unconditionally stable, but dt must not be negative."""
        k = None
        if values is not None:
            k = np.asarray(values, dtype=np.float64)
            k = np.full(self.n, float(k)) if k.ndim == 0 else np.ascontiguousarray(k.ravel())
            if k.size != self.n:
                raise ValueError(f"vertical: {k.size} values for {self.n} tracers")
        if k is not None and self.n == 0 and not k.size:
            k = None
        L.check(L.lib().moka_set_tracer_vertical_diffusion(self._s._h, None if k is None else k.ctypes.data), self._s.mesh.backend._h)

    def vertical_diffusivity(self) -> np.ndarray:
        """moka_tracer_vertical_diffusion: the vertical diffusivity of every tracer (zeros unless set_vertical_diffusivity was called)."""
        out = np.zeros(self.n, dtype=np.float64)
        v = C.c_double()
        for j in range(self.n):
            L.check(L.lib().moka_tracer_vertical_diffusion(self._s._h, j, C.byref(v)), self._s.mesh.backend._h)
            out[j] = v.value
        return out

    def vmix_path(self) -> int:
        """moka_state_tracer_vmix_path: 1 the tile form, 2 the column form of the vertical pass, 0 before the first one."""
        return int(L.lib().moka_state_tracer_vmix_path(self._s._h))

    def set_vertical_field(self, j: int, field):
        """moka_tracer_vertical_field_upload: a vertical diffusivity per interface and cell for tracer j (m^2/s, finite and >= 0 at
        every active interface).  `field`: an (nCells, K) array in the layout of every tracer field, column k the interface between
        levels k and k+1 (the last column, and every row at or below a cell's deepest interface, is never read and may hold anything);
        or a profile of K or K-1 values, taken for every cell; None removes the field, and the tracer's scalar acts again.  While the
        tracer has a field its scalar vertical diffusivity is not read.  Takes effect with the next RK4 step or run."""
        a = None
        if field is not None:
            a = np.asarray(field, dtype=np.float64)
            nC, K = self.shape
            if a.ndim == 1 and a.size in (K, K - 1):
                prof = np.zeros(K)
                prof[:a.size] = a
                a = np.broadcast_to(prof, (nC, K))
            elif a.shape != self.shape:
                raise ValueError(f"vertical field: shape {a.shape}; expected {self.shape} or a profile of {K} or {K - 1} values")
            a = np.ascontiguousarray(a, dtype=np.float64)
        L.check(L.lib().moka_tracer_vertical_field_upload(self._s._h, int(j), None if a is None else L.f64(a)), self._s.mesh.backend._h)

    def vertical_field(self, j: int):
        """moka_tracer_vertical_field_download: the diffusivity field of tracer j as it was uploaded, or None when it has none."""
        v = C.c_int()
        L.check(L.lib().moka_tracer_has_vertical_field(self._s._h, int(j), C.byref(v)), self._s.mesh.backend._h)
        if not v.value:
            return None
        out = np.empty(self.shape, dtype=np.float64)
        L.check(L.lib().moka_tracer_vertical_field_download(self._s._h, int(j), L.f64(out)), self._s.mesh.backend._h)
        return out

    def set_source(self, j: int, a):
        """moka_tracer_source_upload: the source q_j of tracer j, an (nCells, K) field in tracer * m/s (the rate of change of the
        content h phi), constant in time until changed; None removes it.  Takes effect with the next RK4 step or run.  Every value
        must be finite."""
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape != self.shape:
                a = a.reshape(self.shape)
        L.check(L.lib().moka_tracer_source_upload(self._s._h, int(j), None if a is None else L.f64(a)), self._s.mesh.backend._h)

    def source(self, j: int) -> np.ndarray:
        """moka_tracer_source_download: the source of tracer j (zeros when it has none)."""
        out = np.empty(self.shape, dtype=np.float64)
        L.check(L.lib().moka_tracer_source_download(self._s._h, int(j), L.f64(out)), self._s.mesh.backend._h)
        return out

    def has_source(self, j: int) -> bool:
        v = C.c_int()
        L.check(L.lib().moka_tracer_has_source(self._s._h, int(j), C.byref(v)), self._s.mesh.backend._h)
        return bool(v.value)


def set_tracers(Prog: "PrognosticVars", arrays, *positional, vertical=None, diffusivity=None, sources=None, biharmonic=None) -> Tracers:
    """Give this model passive tracers (moka_set_tracers): `arrays` is a list of (nCells, K) fields, uploaded into both time levels;
    an empty list removes the tracers again.  An extension (the reference has none): centred flux-form transport by the thickness
    flux inside RK4 steps (include/moka_hip.h states the algebra); Forward Euler, tapes and halos refuse a state with tracers.
    diffusivity: a scalar or one value per tracer (Tracers.set_diffusivity); None leaves the tracers undiffused.
    sources: one entry per tracer, an (nCells, K) field or None for a tracer without a source (Tracers.set_source).
    biharmonic: a scalar or one coefficient per tracer (Tracers.set_biharmonic); None leaves the term off.
    vertical (keyword only): a scalar or one vertical diffusivity per tracer (Tracers.set_vertical_diffusivity); None leaves the term
    off.  An entry of a per-tracer list may be an array instead: that tracer's diffusivity field (Tracers.set_vertical_field).  Arguments given by position beyond `arrays` are diffusivity, sources, biharmonic, as they always were."""
    if len(positional) > 3:
        raise TypeError("set_tracers: at most diffusivity, sources, biharmonic by position")
    diffusivity, sources, biharmonic = (list(positional) + [diffusivity, sources, biharmonic][len(positional):])
    s = Prog._state
    arrays = list(arrays)
    L.check(L.lib().moka_set_tracers(s._h, len(arrays)), s.mesh.backend._h)
    tr = Tracers(s, len(arrays), Prog.layerThickness[-1].shape)
    for j, a in enumerate(arrays):
        tr.set(j, a, 0)
        tr.set(j, a, 1)
    if diffusivity is not None:
        tr.set_diffusivity(diffusivity)
    if biharmonic is not None:
        tr.set_biharmonic(biharmonic)
    if isinstance(vertical, (list, tuple)) and any(np.ndim(v) > 0 for v in vertical):
        if len(vertical) != len(arrays):
            raise ValueError(f"vertical: {len(vertical)} entries for {len(arrays)} tracers")
        tr.set_vertical_diffusivity([0.0 if np.ndim(v) > 0 else float(v) for v in vertical])
        for j, v in enumerate(vertical):
            if np.ndim(v) > 0:
                tr.set_vertical_field(j, v)
    elif vertical is not None:
        tr.set_vertical_diffusivity(vertical)
    if sources is not None:
        sources = list(sources)
        if len(sources) != len(arrays):
            raise ValueError(f"sources: {len(sources)} entries for {len(arrays)} tracers")
        for j, q in enumerate(sources):
            if q is not None:
                tr.set_source(j, q)
    return tr


# ---------------------------------------------------------------------------------------------
# reverse mode (the reference: Enzyme.autodiff(Reverse, ocn_run_loop, ...), test/enzyme/test_Enzyme_end2end.jl:62-96)
# ---------------------------------------------------------------------------------------------
class AdjointTape:
    """Tape of a Forward-Euler run plus the reverse sweep: d sum(ssh^2) / d initial state, the quantity the reference's
    end-to-end AD test differentiates.  `d_Prog` of that test = (gradient()["ssh"], ["normalVelocity"], ["layerThickness"])."""

    def __init__(self, Prog: "PrognosticVars", capacity_steps: int):
        self._state = Prog._state
        self._ctx = self._state.mesh.backend._h
        m, K = self._state.mesh.HorzMesh.data, self._state.mesh.VertMesh.nVertLevels
        self._shapes = {"ssh": (m.nCells,), "normalVelocity": (m.nEdges, K), "layerThickness": (m.nCells, K),
                        "layerThicknessEdge": (m.nEdges, K)}
        self._h = C.c_void_p()
        L.check(L.lib().moka_tape_create(self._state._h, int(capacity_steps), C.byref(self._h)), self._ctx)
        _own(self, L.lib().moka_tape_destroy, self._h, self._state, self._state.mesh, self._state.mesh.backend)
        self._state._dependents.append(weakref.ref(self))

    def step(self, timestep, flags: int = REFERENCE_COMPAT, method=None):
        """ocn_timestep(timestep, ..., ForwardEuler) -- or RungeKutta4 with method=RungeKutta4 -- with the step recorded.
        One integrator per tape."""
        dt = float(np.asarray(timestep).reshape(-1)[0])
        if method is RungeKutta4:
            L.check(L.lib().moka_step_rk4_taped(self._h, dt), self._ctx)
        else:
            L.check(L.lib().moka_step_fe_taped(self._h, dt, int(flags)), self._ctx)

    def gradient(self) -> dict:
        """Seeds with d sum(ssh^2) at the current state, sweeps the tape backwards (consuming it) and returns the gradient
        with respect to the state the tape started from: ssh, normalVelocity, layerThickness (d_Prog) and the carried
        layerThicknessEdge of the reference_compat sequence."""
        lib = L.lib()
        L.check(lib.moka_adjoint_seed_sum_sq_ssh(self._h), self._ctx)
        L.check(lib.moka_adjoint_sweep(self._h), self._ctx)
        return self.download()

    def download(self) -> dict:
        """The adjoint state as it stands (after a sweep: the gradient), caller's numbering."""
        lib = L.lib()
        out = {}
        for name, fid in (("ssh", L.F_SSH), ("normalVelocity", L.F_NORMAL_VELOCITY), ("layerThickness", L.F_LAYER_THICKNESS),
                          ("layerThicknessEdge", L.F_LAYER_THICKNESS_EDGE)):
            a = np.empty(self._shapes[name], dtype=np.float64)
            L.check(lib.moka_adjoint_download(self._h, fid, L.f64(a)), self._ctx)
            out[name] = a
        return out

    def close(self):
        if self._h:
            _release(self, L.lib().moka_tape_destroy, self._h)
            self._h = C.c_void_p()


class TracerAdjointTape:
    """Reverse mode of the passive tracers over a frozen flow (moka_tracer_tape_*; include/moka_hip.h states the algebra): record RK4
    steps of a model with tracers, then turn d J / d (tracers after the last step) into d J / d (tracers before the first recorded
    step), the flow held as it ran.  The tracer step is linear in the tracers, so this is an exact transpose; it works over the
    linear, nonlinear, Del2 and Del4 dycores alike.  want_source_gradient(j) makes the sweep also return d J / d q_j for a source
    q_j that acts identically in every recorded step, want_diffusivity_gradient(j) -- before the first recorded step -- the scalars
    d J / d kappa_j and d J / d kappa4_j and their per-cell densities, want_vertical_gradient(j) -- likewise before the first recorded
    step -- d J / d kappaV_j with its density per interface and cell.  Sensitivities to the flow are out of scope."""

    def __init__(self, Prog: "PrognosticVars", capacity_steps: int):
        self._state = Prog._state
        self._ctx = self._state.mesh.backend._h
        self._shape = tuple(Prog.layerThickness[-1].shape)
        self._h = C.c_void_p()
        self._kflags = {}
        self._vflags = set()
        L.check(L.lib().moka_tracer_tape_create(self._state._h, int(capacity_steps), C.byref(self._h)), self._ctx)
        _own(self, L.lib().moka_tracer_tape_destroy, self._h, self._state, self._state.mesh, self._state.mesh.backend)
        self._state._dependents.append(weakref.ref(self))

    def step(self, timestep):
        """One RK4 step of the model (bit for bit moka_step_rk4), recorded."""
        L.check(L.lib().moka_step_rk4_tracer_taped(self._h, float(np.asarray(timestep).reshape(-1)[0])), self._ctx)

    def steps(self) -> int:
        n = C.c_int64()
        L.check(L.lib().moka_tracer_tape_steps(self._h, C.byref(n)), self._ctx)
        return int(n.value)

    def seed(self, j: int, a):
        """The adjoint of tracer j := a, an (nCells, K) field; None = zeros.  The first seed after a recorded step zeroes the others."""
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape != self._shape:
                a = a.reshape(self._shape)
        L.check(L.lib().moka_tracer_adjoint_seed(self._h, int(j), None if a is None else L.f64(a)), self._ctx)

    def sweep(self):
        """Reverse over (and pop) every recorded step; the tape is then empty and reusable."""
        L.check(L.lib().moka_tracer_adjoint_sweep(self._h), self._ctx)

    def download(self, j: int) -> np.ndarray:
        """The adjoint of tracer j as it stands (after a sweep: the gradient), caller's numbering."""
        out = np.empty(self._shape, dtype=np.float64)
        L.check(L.lib().moka_tracer_adjoint_download(self._h, int(j), L.f64(out)), self._ctx)
        return out

    def want_source_gradient(self, j: int, on: bool = True):
        """moka_tracer_adjoint_want_source_gradient: the following sweeps also accumulate d J / d q_j (on=False: no longer).  Not
        between a seed and its sweep."""
        L.check(L.lib().moka_tracer_adjoint_want_source_gradient(self._h, int(j), 1 if on else 0), self._ctx)

    def source_gradient(self, j: int) -> np.ndarray:
        """d J / d q_j as it stands (after a sweep: the gradient with respect to a source constant over the recorded steps), caller's
        numbering.  The tracer must have been flagged with want_source_gradient."""
        out = np.empty(self._shape, dtype=np.float64)
        L.check(L.lib().moka_tracer_adjoint_source_download(self._h, int(j), L.f64(out)), self._ctx)
        return out

    def want_diffusivity_gradient(self, j: int, kappa: bool = True, biharmonic: bool = False):
        """moka_tracer_adjoint_want_diffusivity_gradient: tracer j's set becomes exactly (kappa, biharmonic).  Only while the tape
        holds no recorded step: the steps recorded from now on also keep the provisional fields of a flagged tracer, and the sweep
        accumulates d J / d kappa_j and / or d J / d kappa4_j.  Changing the set of flagged tracers drops what earlier sweeps left."""
        for bit, on in ((L.TRACER_GRAD_KAPPA, kappa), (L.TRACER_GRAD_KAPPA4, biharmonic)):
            L.check(L.lib().moka_tracer_adjoint_want_diffusivity_gradient(self._h, int(j), bit, 1 if on else 0), self._ctx)
        self._kflags[int(j)] = (bool(kappa), bool(biharmonic))

    def _kgrad(self, j: int, what: int) -> float:
        out = C.c_double()
        L.check(L.lib().moka_tracer_adjoint_diffusivity_gradient(self._h, int(j), what, C.byref(out)), self._ctx)
        return float(out.value)

    def diffusivity_gradient(self, j: int) -> float:
        """d J / d kappa_j as it stands (after a sweep: the derivative with respect to a diffusivity that acts identically in every
        recorded step): the sum of diffusivity_density(j) over the cells."""
        return self._kgrad(j, L.TRACER_GRAD_KAPPA)

    def biharmonic_gradient(self, j: int) -> float:
        """d J / d kappa4_j, likewise."""
        return self._kgrad(j, L.TRACER_GRAD_KAPPA4)

    def diffusivity_density(self, j: int, biharmonic: bool = False) -> np.ndarray:
        """The per-cell sensitivity density of d J / d kappa_j (biharmonic: of d J / d kappa4_j), nCells values in the caller's
        numbering: where J feels the mixing."""
        out = np.empty(self._shape[0], dtype=np.float64)
        what = L.TRACER_GRAD_KAPPA4 if biharmonic else L.TRACER_GRAD_KAPPA
        L.check(L.lib().moka_tracer_adjoint_diffusivity_density_download(self._h, int(j), what, L.f64(out)), self._ctx)
        return out

    def want_vertical_gradient(self, j: int, on: bool = True):
        """moka_tracer_adjoint_want_vertical_gradient: the steps recorded from now on also keep tracer j's new-level field, and the
        sweep accumulates the density of d J / d kappaV_j (on=False: no longer).  Only while the tape holds no recorded step.  Changing
        the set of flagged tracers drops what earlier sweeps left."""
        L.check(L.lib().moka_tracer_adjoint_want_vertical_gradient(self._h, int(j), 1 if on else 0), self._ctx)
        (self._vflags.add if on else self._vflags.discard)(int(j))

    def vertical_gradient(self, j: int) -> float:
        """d J / d kappaV_j as it stands (after a sweep: the derivative with respect to a vertical diffusivity that acts identically in
        every recorded step): the sum of vertical_density(j) over interfaces and cells.  For a tracer that ran with a diffusivity field
        (Tracers.set_vertical_field) this is the directional derivative along the all-ones field."""
        out = C.c_double()
        L.check(L.lib().moka_tracer_adjoint_vertical_gradient(self._h, int(j), C.byref(out)), self._ctx)
        return float(out.value)

    def vertical_density(self, j: int, view: str = "interface") -> np.ndarray:
        """The sensitivity density of d J / d kappaV_j in the caller's numbering.  view="interface": (nCells, K), column k the interface
        between levels k and k+1 (d J / d kappaV at that interface of that cell -- the derivative with respect to the diffusivity field
        the steps ran with, Tracers.set_vertical_field, or, for a scalar, to a field at that uniform value; columns k >= the cell's
        active depth - 1 are zero);
        "cell": its sums over the interfaces, nCells values; "profile": its sums over the cells, K values."""
        views = {"interface": (L.VGRAD_INTERFACE, self._shape), "cell": (L.VGRAD_CELL, self._shape[0]), "profile": (L.VGRAD_PROFILE, self._shape[1])}
        if view not in views:
            raise ValueError(f"vertical_density: view must be one of {sorted(views)}, not {view!r}")
        what, shape = views[view]
        out = np.empty(shape, dtype=np.float64)
        L.check(L.lib().moka_tracer_adjoint_vertical_density_download(self._h, int(j), what, L.f64(out)), self._ctx)
        return out

    def gradient(self, seeds, sources: bool = False, diffusivity: bool = False, vertical: bool = False):
        """seeds: one entry per tracer, None meaning zero.  Seeds, sweeps and returns the list of gradients d J / d phi_0; with
        sources=True every tracer's source gradient is asked for and (dphi0, dq) is returned.  diffusivity=True appends the two
        vectors (d J / d kappa_j), (d J / d kappa4_j) over the tracers, NaN where want_diffusivity_gradient did not ask (that has to
        happen before the steps are recorded, so this call cannot do it).  vertical=True appends the vector (d J / d kappaV_j), NaN where
        want_vertical_gradient did not ask."""
        seeds = list(seeds)
        if sources:
            for j in range(len(seeds)):
                self.want_source_gradient(j)
        for j, a in enumerate(seeds):
            self.seed(j, a)
        self.sweep()
        dphi0 = [self.download(j) for j in range(len(seeds))]
        out = (dphi0,)
        if sources:
            out += ([self.source_gradient(j) for j in range(len(seeds))],)
        if diffusivity:
            dk, dk4 = np.full(len(seeds), np.nan), np.full(len(seeds), np.nan)
            for j, (k, k4) in self._kflags.items():
                if k and j < len(seeds):
                    dk[j] = self.diffusivity_gradient(j)
                if k4 and j < len(seeds):
                    dk4[j] = self.biharmonic_gradient(j)
            out += (dk, dk4)
        if vertical:
            dkv = np.full(len(seeds), np.nan)
            for j in self._vflags:
                if j < len(seeds):
                    dkv[j] = self.vertical_gradient(j)
            out += (dkv,)
        return out if len(out) > 1 else dphi0

    def path(self) -> int:
        """moka_tracer_adjoint_path: 1 the patch form, 2 the generic form of the reverse kernel, 0 before the first reverse stage."""
        return int(L.lib().moka_tracer_adjoint_path(self._h))

    def vmix_path(self) -> int:
        """moka_tracer_adjoint_vmix_path: 1 the tile form, 2 the column form of the last reverse step's vertical pass (with a tracer
        flagged by want_vertical_gradient: of its gradient instances), 0 none yet."""
        return int(L.lib().moka_tracer_adjoint_vmix_path(self._h))

    def close(self):
        if self._h:
            _release(self, L.lib().moka_tracer_tape_destroy, self._h)
            self._h = C.c_void_p()


class ForcedAdjointTape:
    """Reverse mode through the forced RK4 step (moka_forced_tape_*; include/moka_hip.h states the algebra): record RK4 steps of a
    linear-dycore model whose vertical momentum pass (set_vertical_mixing) may be on, then turn d J / d (state after the last step)
    into d J / d (state before the first recorded step) and, when flagged before the first recorded step, d J / d tau_e per edge,
    d J / d nuV and d J / d r with their per-edge densities.  The parameters act identically in every recorded step."""

    _BITS = {"surfaceStress": L.FORCED_GRAD_STRESS, "viscosity": L.FORCED_GRAD_VISCOSITY, "bottomDrag": L.FORCED_GRAD_DRAG}

    def __init__(self, Prog: "PrognosticVars", capacity_steps: int, quadratic_drag: bool = False):
        self._state = Prog._state
        self._ctx = self._state.mesh.backend._h
        self._ushape = tuple(Prog.normalVelocity[-1].shape)
        self._hshape = tuple(Prog.layerThickness[-1].shape)
        self._want = 0
        self._want_field = False
        self._want_cd = False
        self._h = C.c_void_p()
        create = L.lib().moka_forced_tape_create_quadratic if quadratic_drag else L.lib().moka_forced_tape_create
        L.check(create(self._state._h, int(capacity_steps), C.byref(self._h)), self._ctx)
        _own(self, L.lib().moka_forced_tape_destroy, self._h, self._state, self._state.mesh, self._state.mesh.backend)
        self._state._dependents.append(weakref.ref(self))

    def step(self, timestep):
        """One RK4 step of the model (bit for bit moka_step_rk4), recorded."""
        L.check(L.lib().moka_step_rk4_forced_taped(self._h, float(np.asarray(timestep).reshape(-1)[0])), self._ctx)

    def want_gradient(self, stress: bool = False, viscosity: bool = False, drag: bool = False, viscosity_field: bool = False,
                      quadratic_drag: bool = False):
        """The set of parameter gradients the following sweeps accumulate; only while no step is recorded.  `viscosity_field`: the
        density d J / d f[k,e] of a viscosity per interface and edge, "viscosityField".  `quadratic_drag`: d J / d Cd, "quadraticDrag"
        (a tape made with quadratic_drag=True only)."""
        want = (L.FORCED_GRAD_STRESS if stress else 0) | (L.FORCED_GRAD_VISCOSITY if viscosity else 0) | (L.FORCED_GRAD_DRAG if drag else 0)
        if want:
            L.check(L.lib().moka_forced_adjoint_want_gradient(self._h, want, 1), self._ctx)
        if 7 & ~want:
            L.check(L.lib().moka_forced_adjoint_want_gradient(self._h, 7 & ~want, 0), self._ctx)
        self._want = want
        if bool(viscosity_field) != self._want_field:
            L.check(L.lib().moka_forced_adjoint_want_viscosity_field_gradient(self._h, 1 if viscosity_field else 0), self._ctx)
            self._want_field = bool(viscosity_field)
        if bool(quadratic_drag) != self._want_cd:
            L.check(L.lib().moka_forced_adjoint_want_quadratic_drag_gradient(self._h, 1 if quadratic_drag else 0), self._ctx)
            self._want_cd = bool(quadratic_drag)

    def seed(self, u, h):
        """X := (u, h), (nEdges, K) and (nCells, K) fields: the adjoint of the state after the last recorded step."""
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(self._ushape)
        h = np.ascontiguousarray(h, dtype=np.float64).reshape(self._hshape)
        L.check(L.lib().moka_forced_adjoint_seed(self._h, L.f64(u), L.f64(h)), self._ctx)

    def sweep(self):
        """Reverse over (and pop) every recorded step; the tape is then empty and reusable."""
        L.check(L.lib().moka_forced_adjoint_sweep(self._h), self._ctx)

    def density(self, what: str) -> np.ndarray:
        """The per-edge density of "surfaceStress" (d J / d tau_e itself), "viscosity", "bottomDrag" or "quadraticDrag", caller's edge numbering;
        "viscosityField": (nEdges, nVertLevels), d J / d f[k,e], rows at and below an edge's deepest interface zero."""
        if what == "viscosityField":
            out = np.empty(self._ushape, dtype=np.float64)
            L.check(L.lib().moka_forced_adjoint_viscosity_field_density_download(self._h, L.f64(out)), self._ctx)
            return out
        out = np.empty(self._ushape[0], dtype=np.float64)
        if what == "quadraticDrag":
            L.check(L.lib().moka_forced_adjoint_quadratic_drag_density_download(self._h, L.f64(out)), self._ctx)
            return out
        L.check(L.lib().moka_forced_adjoint_density_download(self._h, self._BITS[what], L.f64(out)), self._ctx)
        return out

    def download(self) -> dict:
        """The adjoint state and the flagged parameter gradients as they stand."""
        lib = L.lib()
        out = {}
        for name, fid, shape in (("normalVelocity", L.F_NORMAL_VELOCITY, self._ushape), ("layerThickness", L.F_LAYER_THICKNESS, self._hshape)):
            a = np.empty(shape, dtype=np.float64)
            L.check(lib.moka_forced_adjoint_download(self._h, fid, L.f64(a)), self._ctx)
            out[name] = a
        if self._want & L.FORCED_GRAD_STRESS:
            out["surfaceStress"] = self.density("surfaceStress")
        for name in ("viscosity", "bottomDrag"):
            if self._want & self._BITS[name]:
                v = C.c_double()
                L.check(lib.moka_forced_adjoint_gradient(self._h, self._BITS[name], C.byref(v)), self._ctx)
                out[name] = float(v.value)
        if self._want_field:
            out["viscosityField"] = self.density("viscosityField")
        if self._want_cd:
            v = C.c_double()
            L.check(lib.moka_forced_adjoint_quadratic_drag_gradient(self._h, C.byref(v)), self._ctx)
            out["quadraticDrag"] = float(v.value)
        return out

    def gradient(self, seed=None) -> dict:
        """Seeds -- with d sum(ssh^2) at the current state, or with seed = (u, h) -- sweeps the tape backwards (consuming it) and returns
        normalVelocity, layerThickness and, when flagged, surfaceStress (per edge), viscosity and bottomDrag (scalars)."""
        if seed is None:
            L.check(L.lib().moka_forced_adjoint_seed_sum_sq_ssh(self._h), self._ctx)
        else:
            self.seed(*seed)
        self.sweep()
        return self.download()

    def vmix_path(self) -> int:
        """moka_forced_tape_vmix_path: 1 the tile form, 2 the column form of the last transposed pass, 0 none yet."""
        return int(L.lib().moka_forced_tape_vmix_path(self._h))

    def device_arrays(self) -> int:
        """moka_forced_tape_device_arrays: the device arrays the tape owns itself (allocated lazily, by what the steps need)."""
        return int(L.lib().moka_forced_tape_device_arrays(self._h))

    def close(self):
        if self._h:
            _release(self, L.lib().moka_forced_tape_destroy, self._h)
            self._h = C.c_void_p()


# ---------------------------------------------------------------------------------------------
# model initialisation from a configuration  (src/forward/init.jl); clock / alarms live in timemanager.py,
# the YAML configuration in config.py, the MPAS file readers / writer in mpasio.py
# ---------------------------------------------------------------------------------------------
def _cfg_get(section, key, default="none"):
    """ConfigGet on a yaml_config, or a plain dict (the array-driven tests pass already-parsed dicts)."""
    d = section.dict if isinstance(section, yaml_config) else section
    return d.get(key, default)


def ocn_setup_clock(config) -> Clock:
    """ocn_setup_clock(Config) (init.jl:57-108): `config` is a GlobalConfig, or a dict
    {"time_management": ..., "time_integration": ..., "output": ...} holding datetimes / periods."""
    if isinstance(config, GlobalConfig):
        tm, ti = ConfigGet(config.namelist, "time_management"), ConfigGet(config.namelist, "time_integration")
        out = ConfigGet(config.streams, "output")
    else:
        tm, ti, out = config["time_management"], config["time_integration"], config.get("output", {})
    start = _cfg_get(tm, "config_start_time", _dt.datetime(1, 1, 1))
    dt = _cfg_get(ti, "config_dt", _dt.timedelta(seconds=1))
    run_duration, stop_time = _cfg_get(tm, "config_run_duration"), _cfg_get(tm, "config_stop_time")
    if not isinstance(run_duration, str) or run_duration != "none":
        clock = mpas_create_clock(dt, start, runDuration=run_duration)
        if not isinstance(stop_time, str) or stop_time != "none":
            if start + run_duration != stop_time:                                  # init.jl:85
                print("Warning: config_run_duration and config_stop_time are inconsitent: using config_run_duration.")
        stop_time = start + run_duration
    elif not isinstance(stop_time, str) or stop_time != "none":
        clock = mpas_create_clock(dt, start, stopTime=stop_time)
    else:
        raise MokaError(L.ERR_ARG, "Error: Neither config_run_duration nor config_stop_time were specified.")  # :94
    attachAlarm(clock, OneTimeAlarm("simulation_end", stop_time))
    attachAlarm(clock, PeriodicAlarm("outputAlarm", _cfg_get(out, "output_interval", _dt.timedelta(days=1)),
                                     _cfg_get(out, "reference_time", start)))
    return clock


def ocn_setup_mesh(Config: GlobalConfig, backend=None, multilayer: bool = True, **layout) -> Mesh:
    """ocn_setup_mesh(Config; backend) (init.jl:41-55): the `mesh` stream names the MPAS file; ReadHorzMesh +
    VerticalMesh(mesh_fp, h_mesh) (mpasio.read_mesh / read_vertical_mesh), then onto the backend."""
    mesh_fp = ConfigGet(ConfigGet(Config.streams, "mesh"), "filename_template")
    data = mpasio.read_mesh(mesh_fp)
    vm = mpasio.read_vertical_mesh(mesh_fp, data)
    h_mesh = HorzMesh(data)
    v_mesh = VerticalMesh(h_mesh, nVertLevels=vm["nVertLevels"], restingThickness=vm["restingThickness"],
                          multilayer=multilayer)
    v_mesh.minLevelCell, v_mesh.maxLevelCell = vm["minLevelCell"], vm["maxLevelCell"]
    return Mesh(h_mesh, v_mesh, backend=backend, **layout)


def ocn_init(Config_filepath, backend=None, multilayer: bool = True, **layout):
    """ocn_init(config_fp; backend) (init.jl:3-30): returns (Setup, Diag, Tend, Prog).  The initial state is the first
    time record of the `input` stream's file (PrognosticVars.jl:59-106; restarts are not supported there either)."""
    Config = ConfigRead(Config_filepath)
    mesh = ocn_setup_mesh(Config, backend=backend, multilayer=multilayer, **layout)
    clock = ocn_setup_clock(Config)
    Setup = ModelSetup(Config, mesh, clock)
    if ConfigGet(ConfigGet(Config.namelist, "time_management"), "config_do_restart"):
        raise MokaError(L.ERR_UNSUPPORTED, "restart not yet supported")            # PrognosticVars.jl:64-66
    input_fp = ConfigGet(ConfigGet(Config.streams, "input"), "filename_template")
    nT = ConfigGet(ConfigGet(Config.namelist, "time_integration"), "config_number_of_time_levels")
    K = mesh.VertMesh.nVertLevels
    ssh, u, h = mpasio.read_initial_state(input_fp, mesh.HorzMesh.data, K)
    Prog = PrognosticVars(ssh, u, h, nT, mesh)
    Diag = DiagnosticVars(Config, mesh, Prog._state)
    Tend = TendencyVars(Config, mesh, Prog._state)
    return Setup, Diag, Tend, Prog


def write_netcdf(Setup: ModelSetup, Diag, Prog, reference_compat: bool = True):
    """write_netcdf(Setup, Diag, Prog) (OutPut.jl:117-215) to the `output` stream's file.

    reference_compat (default): the file holds what the reference's file holds -- the state ONE STEP BEHIND the final one.
    write_netcdf first pulls everything to the CPU with Adapt.adapt_structure(KA.CPU(), Prog) (OutPut.jl:124), and that
    method rebuilds the struct from the FIRST time level, `x.ssh[1]` etc. (PrognosticVars.jl:108-113), whose deep copies
    fill every level; `Prog.ssh[end]` written at OutPut.jl:210-212 is therefore the previous time level, i.e. the state the
    last ocn_timestep started from (advanceTimeLevels! copied it there, time_integration.jl:163).  A quirk of the
    reference like those of SURVEY 0.6; reference_compat=False writes the current level."""
    out_fp = ConfigGet(ConfigGet(Setup.config.streams, "output"), "filename_template")
    clock, mesh = Setup.timeManager, Setup.mesh
    lev = 0 if reference_compat else -1
    mpasio.write_output(out_fp, mesh.HorzMesh.data, mesh.VertMesh.nVertLevels, period_seconds(clock.timeStep),
                        (clock.currTime - clock.startTime).total_seconds(), Prog.ssh[lev].get(),
                        Prog.layerThickness[lev].get(), Prog.normalVelocity[lev].get())
    return out_fp


def ocn_init_alarms(Setup: ModelSetup):
    """ocn_init_alarms (init.jl:111-127): dt := floor(2*(mean dcEdge/1e3)*mean dcEdge/200e3) seconds."""
    dc = Setup.mesh.HorzMesh.data.dcEdge
    dt = math.floor(2 * (float(np.mean(dc)) / 1e3) * float(np.mean(dc)) / 200e3)
    changeTimeStep(Setup.timeManager, Second(dt))
    clock = Setup.timeManager
    return clock, clock.alarms["simulation_end"], clock.alarms["outputAlarm"]
