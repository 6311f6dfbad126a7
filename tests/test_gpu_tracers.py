"""Passive tracer transport on the GPU (moka_set_tracers): both kernel forms bit for bit against the numpy twin (tests/tracer_twin.py)
through eager steps and graph replay, over the dycore modes and with partial edge masks; the constant tracer; conservation; the
interface and its refusals."""
import ctypes as C
import datetime as dt

import numpy as np
import pytest

import oracle as orc
import moka_hip as mk
import tracer_twin as tt
from del4_twin import Del4Twin, TwinState
from moka_hip import lib as L
from moka_hip import meshgen as mg

pytestmark = pytest.mark.gpu

CONFIG = {"time_management": {"config_start_time": dt.datetime(1, 1, 1), "config_run_duration": dt.timedelta(hours=10)},
          "time_integration": {"config_dt": dt.timedelta(seconds=400), "config_number_of_time_levels": 2}}
MODES = ["linear", "nonlinear", "del2+del4"]
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
                         "ico32": lambda: mg.icosahedral_mesh(32),
                         "ico12f": lambda: mg.icosahedral_mesh(12, flips=8, seed=4)}[name]()
    return _MESHES[name]


def dt_of(meshname):
    return 2.0 if meshname == "planar" else 20.0


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


def reference(meshname, K, mode, partial, tracers, checkpoints, magnitudes=False):
    """The twin's state after each step count in `checkpoints`, computed once per case and shared: a dict
    step -> (phis previous, phis current, u, h, ssh[, magnitudes of the step]).  `tracers`: a tuple naming the fields (an int n = the
    first n of fields(), "one" = a field of ones first, then two of fields())."""
    key = (meshname, K, mode, partial, tracers, tuple(checkpoints), magnitudes)
    if key not in _REFS:
        mesh = get_mesh(meshname)
        ssh, u, h, rest = random_state(mesh, K, 101 + K)
        mlt = partial_mlt(mesh, K) if partial else K
        om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=mlt)
        twin = tt.TracerTwin(om, twin_base(om, mesh, mode, dt_of(meshname)))
        st = TwinState(ssh, u, h)
        f = initial_fields(mesh, K, tracers)
        phis = [[a.copy() for a in f], [a.copy() for a in f]]
        out = {}
        for step in range(1, max(checkpoints) + 1):
            twin.step_rk4(st, phis, dt_of(meshname), magnitudes=magnitudes)
            if step in checkpoints:
                out[step] = ([a.copy() for a in phis[0]], [a.copy() for a in phis[1]], st.u[1].copy(), st.h[1].copy(), st.ssh[1].copy(),
                             twin.last_M)
        _REFS[key] = out
    return _REFS[key]


def initial_fields(mesh, K, tracers):
    if tracers == "one":
        return [np.ones((mesh.nCells, K))] + fields(mesh, K, 2)
    return fields(mesh, K, 3)[:tracers]


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


def check_tracers(tr, ref):
    prev, cur = ref[0], ref[1]
    for j in range(len(cur)):
        assert np.array_equal(tr.get(j), cur[j]), ("current", j)
        assert np.array_equal(tr.get(j, 0), prev[j]), ("previous", j)


def check_dycore(Prog, ref):
    assert np.array_equal(Prog.normalVelocity[-1].get(), ref[2])
    assert np.array_equal(Prog.layerThickness[-1].get(), ref[3])
    assert np.array_equal(Prog.ssh[-1].get(), ref[4])


def expected_path(meshname, K):
    return 1 if K % 2 == 0 and 34 <= K <= 64 and meshname != "ico12f" else 2


SHAPES = [("ico16", 1), ("planar", 4), ("ico12f", 5), ("planar", 34), ("ico32", 34), ("ico16", 60), ("planar", 64), ("ico12f", 40),
          ("ico16", 66)]


@pytest.mark.parametrize("nT", [1, 3])
@pytest.mark.parametrize("meshname,K", SHAPES)
def test_tracers_bitwise_against_the_twin(backend, meshname, K, nT):
    """2 eager steps and 5 more through mk.run_steps, then 6 more (one eager, the rest replayed from the captured graph): the previous
    and the current level of every tracer equal the twin bit for bit each time -- the rotation check.  Three distinct fields: the
    tracer loop does not mix rows.  The patch form exactly where K is even, 34 <= K <= 64 and the mesh has no heptagons."""
    ref = reference(meshname, K, "linear", False, 3, (7, 13))
    md = Model(backend, meshname, K)
    try:
        tr = mk.set_tracers(md.Prog, initial_fields(md.mesh, K, 3)[:nT])
        assert tr.path() == 0
        md.eager(2)
        assert tr.path() == expected_path(meshname, K)
        md.run(5)
        check_tracers(tr, [r[:nT] for r in ref[7][:2]])
        check_dycore(md.Prog, ref[7])
        md.run(6)
        check_tracers(tr, [r[:nT] for r in ref[13][:2]])
        check_dycore(md.Prog, ref[13])
    finally:
        md.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("meshname,K", [("ico16", 60), ("ico12f", 5)])
def test_tracers_over_the_dycore_modes(backend, meshname, K, mode):
    """Linear, nonlinear and nonlinear + Del2 + Del4 dycores: tracers and dycore fields equal their twins, and the dycore fields equal
    a run of the same state without tracers bit for bit -- tracers never feed back."""
    ref = reference(meshname, K, mode, False, 3, (7,))
    got = []
    for with_tracers in (True, False):
        md = Model(backend, meshname, K, mode=mode)
        try:
            if with_tracers:
                tr = mk.set_tracers(md.Prog, initial_fields(md.mesh, K, 3))
            md.eager(1)
            md.run(6)
            if with_tracers:
                check_tracers(tr, ref[7])
                assert tr.path() == expected_path(meshname, K)
            check_dycore(md.Prog, ref[7])
            got.append([md.Prog.normalVelocity[t].get() for t in (0, 1)] + [md.Prog.layerThickness[t].get() for t in (0, 1)] +
                       [md.Prog.ssh[t].get() for t in (0, 1)])
        finally:
            md.close()
    for a, b in zip(*got):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("variant", [0, 3])
@pytest.mark.parametrize("meshname,K", [("ico16", 60), ("planar", 64)])
def test_tracers_with_partial_edge_masks(backend, meshname, K, variant):
    """maxLevelEdgeTop < K on a third of the edges, 0 included, in the patch form (default kernels) and the generic form (variant 3)."""
    ref = reference(meshname, K, "linear", True, 3, (3,))
    md = Model(backend, meshname, K, partial=True, variant=variant)
    try:
        tr = mk.set_tracers(md.Prog, initial_fields(md.mesh, K, 3))
        md.run(3)
        assert tr.path() == (1 if variant == 0 else 2)
        check_tracers(tr, ref[3])
        check_dycore(md.Prog, ref[3])
    finally:
        md.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", [0, 3])
def test_unit_tracer_stays_exactly_one(backend, variant, mode):
    """phi == 1 beside two random tracers is exactly 1.0 at both time levels after 10 steps through graph replay, in both kernel forms
    and over the three dycore modes; the tracers beside it equal the twin."""
    meshname, K = "ico16", 60
    ref = reference(meshname, K, mode, False, "one", (10,))
    md = Model(backend, meshname, K, mode=mode, variant=variant)
    try:
        tr = mk.set_tracers(md.Prog, initial_fields(md.mesh, K, "one"))
        md.run(10)
        assert tr.path() == (1 if variant == 0 else 2)
        one = np.ones((md.mesh.nCells, K))
        assert np.array_equal(tr.get(0), one) and np.array_equal(tr.get(0, 0), one)
        check_tracers(tr, ref[10])
    finally:
        md.close()


def test_many_tracers_take_several_passes_of_the_patch_form(backend):
    """Nine tracers at K = 64: more rows than the patch form keeps resident (two passes, dynamic LDS above 64 KB); every tracer equals
    the single-tracer twin of its field."""
    meshname, K = "planar", 64
    ref = reference(meshname, K, "linear", False, 3, (7, 13))
    md = Model(backend, meshname, K)
    try:
        f = initial_fields(md.mesh, K, 3)
        tr = mk.set_tracers(md.Prog, [f[j % 3] for j in range(9)])
        md.eager(2)
        md.run(5)
        assert tr.path() == 1
        for j in range(9):
            assert np.array_equal(tr.get(j), ref[7][1][j % 3]), j
            assert np.array_equal(tr.get(j, 0), ref[7][0][j % 3]), j
    finally:
        md.close()


@pytest.mark.parametrize("meshname,K", [("ico16", 60), ("ico12f", 5)])
def test_content_is_conserved_on_the_gpu(backend, meshname, K):
    """sum_c A_c sum_k phi h of the GPU's own output, in long double, changes per step by no more than tracer_twin.content_bound
    (the CPU test's bound; its magnitudes come from the twin's run of the same steps)."""
    ref = reference(meshname, K, "nonlinear", False, 3, (1, 2, 3), magnitudes=True)
    md = Model(backend, meshname, K, mode="nonlinear")
    try:
        tr = mk.set_tracers(md.Prog, initial_fields(md.mesh, K, 3))
        s0 = [tt.content(md.mesh, tr.get(j), md.Prog.layerThickness[-1].get()) for j in range(3)]
        for step in (1, 2, 3):
            md.run(1)
            h = md.Prog.layerThickness[-1].get()
            for j in range(3):
                s1 = tt.content(md.mesh, tr.get(j), h)
                bound = tt.content_bound(md.mesh, *ref[step][5][j])
                print(f"step {step} tracer {j}: dS = {float(s1 - s0[j]):.3e}, bound = {float(bound):.3e}")
                assert abs(s1 - s0[j]) <= bound
                s0[j] = s1
    finally:
        md.close()


def test_tracer_interface(backend):
    """Upload then download is exact at both levels; set_tracers([]) restores a state that steps like one that never had tracers; key 7
    leaves the state on the running sum; optimize_placement succeeds and leaves the tracers untouched."""
    meshname, K = "ico16", 60
    md, plain = Model(backend, meshname, K), Model(backend, meshname, K)
    lib = L.lib()
    try:
        sh = md.Prog._state._h
        f = fields(md.mesh, K, 4, seed=5)
        tr = mk.set_tracers(md.Prog, f[:2])
        assert np.array_equal(tr.get(0), f[0]) and np.array_equal(tr.get(1, 0), f[1])
        tr.set(0, f[2], 0); tr.set(1, f[3], 1)
        assert np.array_equal(tr.get(0, 0), f[2]) and np.array_equal(tr.get(0, 1), f[0])
        assert np.array_equal(tr.get(1, 1), f[3]) and np.array_equal(tr.get(1, 0), f[1])
        assert lib.moka_set_tracers(sh, -1) == L.ERR_ARG
        buf = np.zeros((md.mesh.nCells, K))
        assert lib.moka_tracer_download(sh, 2, 1, buf.ctypes.data) == L.ERR_ARG
        assert lib.moka_tracer_download(sh, 0, 2, buf.ctypes.data) == L.ERR_ARG
        # the 13-stream form is not restated for tracers: the running sum
        L.check(lib.moka_set_tuning(7, 1))
        try:
            assert lib.moka_state_rk4_streams(plain.Prog._state._h) == 13
            assert lib.moka_state_rk4_streams(sh) == 16
        finally:
            L.check(lib.moka_set_tuning(7, 0))
        md.run(2)
        before = [tr.get(j, t) for j in range(2) for t in (0, 1)]
        rep = md.Prog._state.optimize_placement(2)
        assert rep["tries"] >= 0
        after = [tr.get(j, t) for j in range(2) for t in (0, 1)]
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
        # advanceTimeLevels carries the tracers: previous <- current
        mk.advanceTimeLevels(md.Prog)
        assert np.array_equal(tr.get(0, 0), tr.get(0, 1))
        # tracers off again: the state steps like one that never had any (it is 2 steps ahead of `plain`)
        mk.set_tracers(md.Prog, [])
        assert lib.moka_state_tracer_path(sh) == 0
        assert lib.moka_tracer_download(sh, 0, 1, buf.ctypes.data) == L.ERR_ARG
        plain.run(2)
        mk.advanceTimeLevels(plain.Prog)
        md.run(7); plain.run(7)
        for t in (0, 1):
            assert np.array_equal(md.Prog.normalVelocity[t].get(), plain.Prog.normalVelocity[t].get())
            assert np.array_equal(md.Prog.layerThickness[t].get(), plain.Prog.layerThickness[t].get())
            assert np.array_equal(md.Prog.ssh[t].get(), plain.Prog.ssh[t].get())
    finally:
        md.close(); plain.close()


def test_tracer_refusals(backend):
    """Forward Euler (step and run), tapes and halos refuse a state with tracers with MOKA_ERR_UNSUPPORTED and a message that names
    tracers; fp32-storage states refuse tracers."""
    meshname, K = "ico16", 4
    md = Model(backend, meshname, K)
    lib = L.lib()
    try:
        sh = md.Prog._state._h
        mk.set_tracers(md.Prog, fields(md.mesh, K, 1))
        assert lib.moka_step_fe(sh, md.dt, L.FE_REFERENCE_COMPAT) == L.ERR_UNSUPPORTED
        assert b"tracers" in lib.moka_last_error(md.backend._h)
        assert lib.moka_run(sh, L.FORWARD_EULER, md.dt, 3, L.FE_REFERENCE_COMPAT) == L.ERR_UNSUPPORTED
        tape = C.c_void_p()
        assert lib.moka_tape_create(sh, 2, C.byref(tape)) == L.ERR_UNSUPPORTED
        assert b"tracers" in lib.moka_last_error(md.backend._h) and not tape.value
        z32, z64 = np.zeros(1, np.int32), np.zeros(1, np.int64)
        p32, p64 = z32.ctypes.data_as(C.POINTER(C.c_int32)), z64.ctypes.data_as(C.POINTER(C.c_int64))
        hh = C.c_void_p()
        assert lib.moka_halo_create(sh, 0, p32, p64, p32, p64, p32, p64, p32, p64, 0, 0, C.byref(hh)) == L.ERR_UNSUPPORTED
        assert b"tracers" in lib.moka_last_error(md.backend._h) and not hh.value
        # ... and the other way round: a state with a tape takes no tracers
        mk.set_tracers(md.Prog, [])
        t = mk.AdjointTape(md.Prog, 2)
        assert lib.moka_set_tracers(sh, 1) == L.ERR_UNSUPPORTED
        t.close()
        assert lib.moka_set_tracers(sh, 1) == 0
    finally:
        md.close()
    f32 = Model(backend, meshname, K, state_bytes=4)
    try:
        assert lib.moka_set_tracers(f32.Prog._state._h, 1) == L.ERR_UNSUPPORTED
        assert lib.moka_set_tracers(f32.Prog._state._h, 0) == 0
    finally:
        f32.close()


def test_tracers_refused_on_a_rank_with_a_halo():
    """One rank of a two-way LocalCluster: tracers cannot be switched on while its halo exists."""
    from moka_hip import parallel as par
    mesh = get_mesh("ico16")
    K = 4
    ssh, u, h, rest = random_state(mesh, K, 12)
    cl = par.LocalCluster(mesh, ssh, u, h, rest, 20.0, 2, direct=False)
    try:
        assert L.lib().moka_set_tracers(cl.models[0].Prog._state._h, 1) == L.ERR_UNSUPPORTED
    finally:
        cl.close()
