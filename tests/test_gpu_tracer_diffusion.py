"""Harmonic tracer diffusion on the GPU (moka_set_tracer_diffusion): both kernel forms bit for bit against the numpy twin
(tests/tracer_diffusion_twin.py) through eager steps and graph replay, with partial edge masks and over the dycore modes; the constant
tracer; several LDS passes; switching diffusion on and off; the interface; conservation."""
import ctypes as C
import datetime as dt

import numpy as np
import pytest

import oracle as orc
import moka_hip as mk
import tracer_diffusion_twin as td
import tracer_twin as tt
from del4_twin import Del4Twin, TwinState
from moka_hip import lib as L
from moka_hip import meshgen as mg

pytestmark = pytest.mark.gpu

CONFIG = {"time_management": {"config_start_time": dt.datetime(1, 1, 1), "config_run_duration": dt.timedelta(hours=10)},
          "time_integration": {"config_dt": dt.timedelta(seconds=400), "config_number_of_time_levels": 2}}
MODES = ["linear", "nonlinear", "del2+del4"]
KFACT = (0.02, 0.0, 0.005)          # kappa_j dt / dcEdge_min^2 of the three tracers
_MESHES = {}
_REFS = {}


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)
    yield b
    b.close()


def get_mesh(name):
    if name not in _MESHES:
        _MESHES[name] = {"planar": lambda: mg.planar_hex_mesh(20, 18, 1000.0, f0=1e-4),
                         "ico16": lambda: mg.icosahedral_mesh(16),
                         "ico12f": lambda: mg.icosahedral_mesh(12, flips=8, seed=4)}[name]()
    return _MESHES[name]


def dt_of(meshname):
    return 2.0 if meshname == "planar" else 20.0


def kappas(meshname, factors=KFACT):
    dcmin = float(get_mesh(meshname).dcEdge.min())
    return tuple(f * dcmin ** 2 / dt_of(meshname) for f in factors)


def random_state(mesh, K, seed):
    rng = np.random.default_rng(seed)
    rest = np.full((mesh.nCells, K), 1000.0 / K) + rng.uniform(0, 0.1, (mesh.nCells, K))
    h = rest + rng.uniform(-1, 1, (mesh.nCells, K))
    u = rng.uniform(-1, 1, (mesh.nEdges, K))
    return h.sum(1) - rest.sum(1), u, h, rest


def fields(mesh, K, n, seed=21):
    """n distinct tracer fields in [0.5, 1.5]."""
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.5, 1.5, (mesh.nCells, K)) for _ in range(n)]


def initial_fields(mesh, K, tracers):
    if tracers == "one":
        return [np.ones((mesh.nCells, K))] + fields(mesh, K, 2)
    return fields(mesh, K, 3)[:tracers]


def partial_mlt(mesh, K):
    rng = np.random.default_rng(8)
    mlt = np.where(rng.random(mesh.nEdges) < 0.33, rng.integers(0, K + 1, mesh.nEdges), K).astype(np.int32)
    mlt[:3] = 0
    return mlt


def viscosities(mesh, dtv):
    dcmin = float(mesh.dcEdge.min())
    return 0.01 * dcmin ** 2 / dtv, 0.002 * dcmin ** 4 / dtv


def twin_base(om, mesh, mode, dtv):
    if mode == "linear":
        return om
    if mode == "nonlinear":
        return orc.OracleNonlinear(om)
    v2, v4 = viscosities(mesh, dtv)
    return Del4Twin(om, visc_del2=v2, visc_del4=v4)


def reference(meshname, K, mode, partial, tracers, schedule, magnitudes=False, plain=False):
    """The twin's state after each segment of `schedule` = ((nsteps, factors), ...), factors = kappa_j dt / dcEdge_min^2 per tracer;
    computed once per case and shared: a list of (phis previous, phis current, u, h, ssh, magnitudes of the last step) per segment.
    plain: tests/tracer_twin.py's TracerTwin (no diffusion) over the same steps."""
    key = (meshname, K, mode, partial, tracers, schedule, magnitudes, plain)
    if key not in _REFS:
        mesh = get_mesh(meshname)
        ssh, u, h, rest = random_state(mesh, K, 101 + K)
        mlt = partial_mlt(mesh, K) if partial else K
        om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=mlt)
        base = twin_base(om, mesh, mode, dt_of(meshname))
        twin = tt.TracerTwin(om, base) if plain else td.TracerDiffusionTwin(om, base, [0.0] * 3)
        st = TwinState(ssh, u, h)
        f = initial_fields(mesh, K, tracers)
        phis = [[a.copy() for a in f], [a.copy() for a in f]]
        out = []
        for nsteps, factors in schedule:
            twin.kappa = list(kappas(meshname, factors))
            for _ in range(nsteps):
                twin.step_rk4(st, phis, dt_of(meshname), magnitudes=magnitudes)
            out.append(([a.copy() for a in phis[0]], [a.copy() for a in phis[1]], st.u[1].copy(), st.h[1].copy(), st.ssh[1].copy(),
                        twin.last_M))
        _REFS[key] = out
    return _REFS[key]


class Model:
    """A model on the device, from ocn_init_from_arrays or (partial edge masks) from the mesh objects."""

    def __init__(self, backend, meshname, K, mode="linear", partial=False, variant=0, **kw):
        self.mesh = mesh = get_mesh(meshname)
        self.K, self.dt, self.backend = K, dt_of(meshname), backend
        self.ssh, self.u, self.h, self.rest = random_state(mesh, K, 101 + K)
        backend.set_kernel_variant(variant)
        if partial:
            hm = mk.HorzMesh(mesh)
            vm = mk.VerticalMesh(hm, nVertLevels=K, restingThickness=self.rest)
            vm.maxLevelEdge.Top[:] = partial_mlt(mesh, K)
            self.M = mk.Mesh(hm, vm, backend=backend)
            self.Prog = mk.PrognosticVars(self.ssh, self.u, self.h, 2, self.M)
            self.Setup = None
        else:
            self.Setup, self.Diag, self.Tend, self.Prog = mk.ocn_init_from_arrays(mesh, self.ssh, self.u, self.h, self.rest, CONFIG,
                                                                                  backend, multilayer=True, **kw)
            self.M = self.Setup.mesh
            mk.changeTimeStep(self.Setup.timeManager, dt.timedelta(seconds=self.dt))
        if mode != "linear":
            v2, v4 = viscosities(mesh, self.dt) if mode == "del2+del4" else (0.0, 0.0)
            mk.set_nonlinear(self.Prog, True, visc_del2=v2, visc_del4=v4)

    def eager(self, n):
        for _ in range(n):
            mk.ocn_timestep(self.Prog, self.Diag, self.Tend, self.Setup, mk.RungeKutta4)

    def run(self, n):
        mk.run_steps(self.Prog, mk.RungeKutta4, self.dt, n)

    def close(self):
        self.Prog._state.close(); self.M.close()
        self.backend.set_kernel_variant(0)


def check_tracers(tr, ref, which=None):
    prev, cur = ref[0], ref[1]
    for j in (range(len(cur)) if which is None else which):
        assert np.array_equal(tr.get(j), cur[j]), ("current", j)
        assert np.array_equal(tr.get(j, 0), prev[j]), ("previous", j)


def check_dycore(Prog, ref):
    assert np.array_equal(Prog.normalVelocity[-1].get(), ref[2])
    assert np.array_equal(Prog.layerThickness[-1].get(), ref[3])
    assert np.array_equal(Prog.ssh[-1].get(), ref[4])


def expected_path(meshname, K):
    return 1 if K % 2 == 0 and 34 <= K <= 64 and meshname != "ico12f" else 2


SHAPES = [("planar", 4), ("ico12f", 5), ("planar", 34), ("ico16", 60), ("planar", 64), ("ico16", 66)]


@pytest.mark.parametrize("meshname,K", SHAPES)
def test_diffused_tracers_bitwise_against_the_twin(backend, meshname, K):
    """2 eager steps and 5 more through mk.run_steps (graph replay), kappa = (0.02, 0, 0.005) dcEdge_min^2 / dt: both levels of every
    tracer equal the twin bit for bit, the kappa = 0 tracer equals the plain TracerTwin's, the dycore is the twin's.  The patch form
    exactly where K is even, 34 <= K <= 64 and the mesh has no heptagons (34 and 64: its limits; 66, 4, heptagons: the generic form)."""
    ref = reference(meshname, K, "linear", False, 3, ((7, KFACT),))[0]
    plain = reference(meshname, K, "linear", False, 3, ((7, KFACT),), plain=True)[0]
    md = Model(backend, meshname, K)
    try:
        tr = mk.set_tracers(md.Prog, initial_fields(md.mesh, K, 3), diffusivity=kappas(meshname))
        assert tr.path() == 0
        md.eager(2)
        assert tr.path() == expected_path(meshname, K)
        md.run(5)
        check_tracers(tr, ref)
        check_tracers(tr, plain, which=(1,))
        assert not np.array_equal(ref[1][0], plain[1][0]) and not np.array_equal(ref[1][2], plain[1][2])     # diffusion acted
        check_dycore(md.Prog, ref)
    finally:
        md.close()


@pytest.mark.parametrize("variant", [0, 3])
def test_diffusion_with_partial_edge_masks(backend, variant):
    """maxLevelEdgeTop < K on a third of the edges, 0 included, in the patch form (default kernels) and the generic form (variant 3):
    tracers and dycore bitwise after 3 steps."""
    meshname, K = "ico16", 60
    ref = reference(meshname, K, "linear", True, 3, ((3, KFACT),))[0]
    md = Model(backend, meshname, K, partial=True, variant=variant)
    try:
        tr = mk.set_tracers(md.Prog, initial_fields(md.mesh, K, 3), diffusivity=kappas(meshname))
        md.run(3)
        assert tr.path() == (1 if variant == 0 else 2)
        check_tracers(tr, ref)
        check_dycore(md.Prog, ref)
    finally:
        md.close()


@pytest.mark.parametrize("mode", MODES)
def test_diffusion_over_the_dycore_modes(backend, mode):
    """Linear, nonlinear and nonlinear + Del2 + Del4 dycores: the tracers equal the twin, and the dycore fields equal a run of the same
    state without tracers bit for bit -- tracers never feed back."""
    meshname, K = "ico16", 60
    ref = reference(meshname, K, mode, False, 3, ((7, KFACT),))[0]
    got = []
    for with_tracers in (True, False):
        md = Model(backend, meshname, K, mode=mode)
        try:
            if with_tracers:
                tr = mk.set_tracers(md.Prog, initial_fields(md.mesh, K, 3), diffusivity=kappas(meshname))
            md.eager(1)
            md.run(6)
            if with_tracers:
                check_tracers(tr, ref)
                assert tr.path() == 1
            check_dycore(md.Prog, ref)
            got.append([md.Prog.normalVelocity[t].get() for t in (0, 1)] + [md.Prog.layerThickness[t].get() for t in (0, 1)] +
                       [md.Prog.ssh[t].get() for t in (0, 1)])
        finally:
            md.close()
    for a, b in zip(*got):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("variant", [0, 3])
def test_unit_tracer_stays_exactly_one_with_diffusion(backend, variant):
    """phi == 1 with kappa > 0 beside two random tracers is exactly 1.0 at both time levels after 10 steps through graph replay, in
    both kernel forms; the tracers beside it equal the twin."""
    meshname, K = "ico16", 60
    fact = (0.02, 0.02, 0.005)
    ref = reference(meshname, K, "nonlinear", False, "one", ((10, fact),))[0]
    md = Model(backend, meshname, K, mode="nonlinear", variant=variant)
    try:
        tr = mk.set_tracers(md.Prog, initial_fields(md.mesh, K, "one"), diffusivity=kappas(meshname, fact))
        md.run(10)
        assert tr.path() == (1 if variant == 0 else 2)
        one = np.ones((md.mesh.nCells, K))
        assert np.array_equal(tr.get(0), one) and np.array_equal(tr.get(0, 0), one)
        check_tracers(tr, ref)
    finally:
        md.close()


def test_many_diffused_tracers_take_several_passes_of_the_patch_form(backend):
    """Nine tracers at K = 64 with diffusion on: more rows than the patch form keeps resident, and the staged dvdc shifts the chunk;
    every tracer equals the single-field twin of its field and diffusivity."""
    meshname, K = "planar", 64
    ref = reference(meshname, K, "linear", False, 3, ((7, KFACT),))[0]
    md = Model(backend, meshname, K)
    try:
        f = initial_fields(md.mesh, K, 3)
        kap = kappas(meshname)
        tr = mk.set_tracers(md.Prog, [f[j % 3] for j in range(9)], diffusivity=[kap[j % 3] for j in range(9)])
        md.eager(2)
        md.run(5)
        assert tr.path() == 1
        for j in range(9):
            assert np.array_equal(tr.get(j), ref[1][j % 3]), j
            assert np.array_equal(tr.get(j, 0), ref[0][j % 3]), j
    finally:
        md.close()


@pytest.mark.parametrize("meshname,K", [("ico16", 60), ("ico12f", 5)])
def test_switching_diffusion_between_runs(backend, meshname, K):
    """2 steps with diffusion on, set_diffusivity(0), 2 more, on again, 2 more: each segment equals the twin (a change between two
    moka_run calls takes effect).  While every diffusivity is zero the state runs like one that never set any, bit for bit: a second
    model, never given a diffusivity, takes over the first one's tracers after the first segment and stays equal to it."""
    zero = (0.0, 0.0, 0.0)
    ref = reference(meshname, K, "linear", False, 3, ((2, KFACT), (2, zero), (2, KFACT)))
    md, never = Model(backend, meshname, K), Model(backend, meshname, K)
    try:
        tr = mk.set_tracers(md.Prog, initial_fields(md.mesh, K, 3), diffusivity=kappas(meshname))
        trn = mk.set_tracers(never.Prog, initial_fields(md.mesh, K, 3))
        md.run(2); never.run(2)
        check_tracers(tr, ref[0])
        for j in range(3):
            for level in (0, 1):
                trn.set(j, tr.get(j, level), level)
        tr.set_diffusivity(0)
        assert np.array_equal(tr.diffusivity(), np.zeros(3))
        md.run(2); never.run(2)
        check_tracers(tr, ref[1])
        for j in range(3):
            for level in (0, 1):
                assert np.array_equal(tr.get(j, level), trn.get(j, level))
        check_dycore(never.Prog, ref[1])
        tr.set_diffusivity(kappas(meshname))
        md.run(2)
        check_tracers(tr, ref[2])
        check_dycore(md.Prog, ref[2])
        assert tr.path() == expected_path(meshname, K)
    finally:
        md.close(); never.close()


def test_diffusion_interface(backend):
    """The getter round-trips; negative, NaN and infinite values return MOKA_ERR_ARG and leave the old values in place;
    moka_set_tracers resets the diffusivities; a non-NULL kappa without tracers and an index out of range return MOKA_ERR_ARG."""
    meshname, K = "ico16", 4
    md = Model(backend, meshname, K)
    lib = L.lib()
    try:
        sh = md.Prog._state._h
        tr = mk.set_tracers(md.Prog, fields(md.mesh, K, 3))
        assert np.array_equal(tr.diffusivity(), np.zeros(3))
        good = np.array([12.5, 0.0, 3.0])
        tr.set_diffusivity(good)
        assert np.array_equal(tr.diffusivity(), good)
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            k = np.array([1.0, bad, 2.0])
            assert lib.moka_set_tracer_diffusion(sh, k.ctypes.data) == L.ERR_ARG, bad
            assert np.array_equal(tr.diffusivity(), good), bad
        with pytest.raises(ValueError):
            tr.set_diffusivity([1.0, 2.0])
        out = C.c_double(-7.0)
        assert lib.moka_tracer_diffusion(sh, 3, C.byref(out)) == L.ERR_ARG
        assert lib.moka_tracer_diffusion(sh, -1, C.byref(out)) == L.ERR_ARG
        tr.set_diffusivity(2.0)                      # a scalar serves every tracer
        assert np.array_equal(tr.diffusivity(), np.full(3, 2.0))
        tr.set_diffusivity(None)                     # NULL: all zero
        assert np.array_equal(tr.diffusivity(), np.zeros(3))
        tr.set_diffusivity(good)
        tr2 = mk.set_tracers(md.Prog, fields(md.mesh, K, 2))          # moka_set_tracers resets
        assert np.array_equal(tr2.diffusivity(), np.zeros(2))
        tr2.set_diffusivity(good[:2])
        mk.set_tracers(md.Prog, [])
        assert lib.moka_tracer_diffusion(sh, 0, C.byref(out)) == L.ERR_ARG
        assert lib.moka_set_tracer_diffusion(sh, good.ctypes.data) == L.ERR_ARG
        assert lib.moka_set_tracer_diffusion(sh, None) == 0
        tr3 = mk.set_tracers(md.Prog, fields(md.mesh, K, 1))
        assert np.array_equal(tr3.diffusivity(), np.zeros(1))
        md.run(1)
    finally:
        md.close()


@pytest.mark.parametrize("meshname,K", [("ico16", 60), ("ico12f", 5)])
def test_content_is_conserved_on_the_gpu_with_diffusion(backend, meshname, K):
    """sum_c A_c sum_k phi h of the GPU's own output, in long double, changes per step by no more than
    tracer_diffusion_twin.content_bound (its magnitudes come from the twin's run of the same steps), nonlinear dycore, 3 steps."""
    refs = reference(meshname, K, "nonlinear", False, 3, ((1, KFACT), (1, KFACT), (1, KFACT)), magnitudes=True)
    md = Model(backend, meshname, K, mode="nonlinear")
    try:
        tr = mk.set_tracers(md.Prog, initial_fields(md.mesh, K, 3), diffusivity=kappas(meshname))
        s0 = [tt.content(md.mesh, tr.get(j), md.Prog.layerThickness[-1].get()) for j in range(3)]
        for step in range(3):
            md.run(1)
            h = md.Prog.layerThickness[-1].get()
            for j in range(3):
                s1 = tt.content(md.mesh, tr.get(j), h)
                bound = td.content_bound(md.mesh, *refs[step][5][j])
                print(f"step {step + 1} tracer {j}: dS = {float(s1 - s0[j]):.3e}, bound = {float(bound):.3e}")
                assert abs(s1 - s0[j]) <= bound
                s0[j] = s1
    finally:
        md.close()
