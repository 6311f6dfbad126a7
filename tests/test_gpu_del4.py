"""Del4 (biharmonic) momentum mixing on the GPU (moka_set_viscosity_del4): every kernel form, bit for bit against the numpy twin
(tests/del4_twin.py), the refusals, and a damped run."""
import ctypes as C
import datetime as dt

import numpy as np
import pytest

import oracle as orc
import moka_hip as mk
from del4_twin import Del4Twin, TwinState
from moka_hip import lib as L
from moka_hip import meshgen as mg

pytestmark = pytest.mark.gpu

CONFIG = {"time_management": {"config_start_time": dt.datetime(1, 1, 1), "config_run_duration": dt.timedelta(hours=10)},
          "time_integration": {"config_dt": dt.timedelta(seconds=400), "config_number_of_time_levels": 2}}
_MESHES = {}


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)
    yield b
    b.close()


def get_mesh(name):
    if name not in _MESHES:
        _MESHES[name] = {"planar": lambda: mg.planar_hex_mesh(20, 18, 1000.0, f0=1e-4),
                         "planar0": lambda: mg.planar_hex_mesh(20, 18, 1000.0),
                         "ico16": lambda: mg.icosahedral_mesh(16),
                         "ico32": lambda: mg.icosahedral_mesh(32),
                         "ico64": lambda: mg.icosahedral_mesh(64),
                         "ico12f": lambda: mg.icosahedral_mesh(12, flips=8, seed=4)}[name]()
    return _MESHES[name]


def random_state(mesh, K, seed):
    rng = np.random.default_rng(seed)
    rest = np.full((mesh.nCells, K), 1000.0 / K) + rng.uniform(0, 0.1, (mesh.nCells, K))
    h = rest + rng.uniform(-1, 1, (mesh.nCells, K))
    u = rng.uniform(-1, 1, (mesh.nEdges, K))
    return h.sum(1) - rest.sum(1), u, h, rest


def viscosities(mesh, dtv):
    dcmin = float(mesh.dcEdge.min())
    return 0.01 * dcmin ** 2 / dtv, 0.002 * dcmin ** 4 / dtv


def del4_path(Prog):
    return L.lib().moka_state_del4_path(Prog._state._h)


def check_levels(Prog, st):
    assert np.array_equal(Prog.normalVelocity[-1].get(), st.u[1])
    assert np.array_equal(Prog.layerThickness[-1].get(), st.h[1])
    assert np.array_equal(Prog.ssh[-1].get(), st.ssh[1])


@pytest.mark.parametrize("mode", ["del4", "del2+del4", "scaled"])
@pytest.mark.parametrize("meshname,K,nsteps", [("ico16", 1, 3), ("ico16", 60, 2), ("planar", 4, 3), ("ico12f", 5, 2), ("ico16", 70, 2),
                                               ("ico12f", 40, 2), ("planar", 34, 2), ("ico32", 34, 2)])
def test_del4_bitwise(backend, meshname, K, nsteps, mode):
    """Tendencies, RK4 steps (the lazily produced stage-4 tendencies too) and graph replay with Del4 on, bit for bit against the
    twin: Del4 alone, on top of Del2, and with a per-edge scaling array (all ones: the same bits as none)."""
    mesh = get_mesh(meshname)
    ssh, u, h, rest = random_state(mesh, K, 101 + K)
    dtv = 2.0 if meshname == "planar" else 20.0
    v2, v4 = viscosities(mesh, dtv)
    v2 = v2 if mode == "del2+del4" else 0.0
    scaling = np.random.default_rng(K).uniform(0.5, 2.0, mesh.nEdges) if mode == "scaled" else None
    Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, CONFIG, backend, multilayer=True)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=K)
    tw = Del4Twin(om, visc_del2=v2, visc_del4=v4, scaling=scaling)
    assert del4_path(Prog) == 0
    mk.set_nonlinear(Prog, True, visc_del2=v2, visc_del4=v4, mesh_scaling_del4=scaling)
    tu, th, ossh = tw.tendencies(u, h)
    mk.computeTendency(Setup.mesh, Diag, Prog, Tend)
    assert np.array_equal(Tend.tendNormalVelocity.get(), tu)
    assert not np.array_equal(tu, Del4Twin(om, visc_del2=v2).tendencies(u, h)[0])
    assert np.array_equal(Tend.tendLayerThickness.get(), th) and np.array_equal(Prog.ssh[-1].get(), ossh)
    # the fused kernel wherever the nonlinear path runs its patch preparation pass: even 34 <= K <= 64, hexagon-width records
    assert del4_path(Prog) == (1 if K % 2 == 0 and 33 <= K <= 64 and meshname != "ico12f" else 2)
    if mode == "scaled":             # a scaling array of ones is no scaling array
        mk.set_nonlinear(Prog, True, visc_del4=v4, mesh_scaling_del4=np.ones(mesh.nEdges))
        mk.computeTendency(Setup.mesh, Diag, Prog, Tend)
        assert np.array_equal(Tend.tendNormalVelocity.get(), Del4Twin(om, visc_del4=v4).tendencies(u, h)[0])
        mk.set_nonlinear(Prog, True, visc_del2=v2, visc_del4=v4, mesh_scaling_del4=scaling)
    st = TwinState(ssh, u, h)
    mk.changeTimeStep(Setup.timeManager, dt.timedelta(seconds=dtv))
    for _ in range(nsteps):
        mk.ocn_timestep(Prog, Diag, Tend, Setup, mk.RungeKutta4)
        tw.step_rk4(st, dtv)
    check_levels(Prog, st)
    assert np.array_equal(Tend.tendNormalVelocity.get(), st.tendU)
    mk.run_steps(Prog, mk.RungeKutta4, dtv, 5)                          # graph replay
    for _ in range(5):
        tw.step_rk4(st, dtv)
    check_levels(Prog, st)
    Prog._state.close(); Setup.mesh.close()


@pytest.mark.parametrize("variant,shape", [(0, 0), (0, 1), (0, 2), (0, 3), (0, 10), (4, 0), (4, 1), (3, 0)])
@pytest.mark.parametrize("meshname,K,visc2", [("ico16", 60, 0.0), ("planar", 64, 1.0)])
def test_del4_kernel_forms_with_partial_edge_masks(backend, meshname, K, visc2, variant, shape):
    """Every form of the nonlinear kernels (variant 0 with launch shapes 0 / 1 / 2 / 3 / 10 -- moka_set_tuning keys 5 and 6 --,
    variant 4, variant 3) with Del4 on and maxLevelEdgeTop < K on a third of the edges, bit for bit against the twin; the patch
    forms take the fused Del4 kernel, variant 3 the entity kernels."""
    L.check(L.lib().moka_set_tuning(5, shape % 10))
    L.check(L.lib().moka_set_tuning(6, 40 if shape == 10 else 0))
    mesh = get_mesh(meshname)
    ssh, u, h, rest = random_state(mesh, K, 93 + K)
    dtv = 2.0 if meshname == "planar" else 20.0
    rng = np.random.default_rng(8)
    mlt = np.where(rng.random(mesh.nEdges) < 0.33, rng.integers(0, K + 1, mesh.nEdges), K).astype(np.int32)
    hm = mk.HorzMesh(mesh)
    vm = mk.VerticalMesh(hm, nVertLevels=K, restingThickness=rest)
    vm.maxLevelEdge.Top[:] = mlt
    backend.set_kernel_variant(variant)
    try:
        M = mk.Mesh(hm, vm, backend=backend)
        Prog = mk.PrognosticVars(ssh, u, h, 2, M)
        Diag, Tend = mk.DiagnosticVars(None, M, Prog._state), mk.TendencyVars(None, M, Prog._state)
        om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=mlt)
        v2, v4 = viscosities(mesh, dtv)
        v2 *= visc2
        tw = Del4Twin(om, visc_del2=v2, visc_del4=v4)
        mk.set_nonlinear(Prog, True, visc_del2=v2, visc_del4=v4)
        tu, th, ossh = tw.tendencies(u, h)
        mk.computeTendency(M, Diag, Prog, Tend)
        assert np.array_equal(Tend.tendNormalVelocity.get(), tu)
        assert np.array_equal(Tend.tendLayerThickness.get(), th)
        assert del4_path(Prog) == (2 if variant == 3 else 1)
        st = TwinState(ssh, u, h)
        mk.run_steps(Prog, mk.RungeKutta4, dtv, 3)
        for _ in range(3):
            tw.step_rk4(st, dtv)
        check_levels(Prog, st)
        Prog._state.close(); M.close()
    finally:
        backend.set_kernel_variant(0)
        L.check(L.lib().moka_set_tuning(5, 0))
        L.check(L.lib().moka_set_tuning(6, 0))


@pytest.mark.parametrize("variant", [0, 3])
def test_del4_config3_patch_form(backend, variant):
    """Config 3 size (icosahedral m = 64: 40 962 cells x 60 levels): one tendency evaluation and two RK4 steps, bit for bit; the
    default form is served by the fused patch kernel (path 1), kernel variant 3 by the entity kernels (path 2)."""
    mesh = get_mesh("ico64")
    K = 60
    ssh, u, h, rest = random_state(mesh, K, 5)
    dtv = 20.0
    backend.set_kernel_variant(variant)
    try:
        Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, CONFIG, backend, multilayer=True)
        om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=K)
        v2, v4 = viscosities(mesh, dtv)
        tw = Del4Twin(om, visc_del4=v4)
        mk.set_nonlinear(Prog, True, visc_del4=v4)
        tu, th, _ = tw.tendencies(u, h)
        mk.computeTendency(Setup.mesh, Diag, Prog, Tend)
        assert np.array_equal(Tend.tendNormalVelocity.get(), tu) and np.array_equal(Tend.tendLayerThickness.get(), th)
        assert del4_path(Prog) == (1 if variant == 0 else 2)
        st = TwinState(ssh, u, h)
        mk.changeTimeStep(Setup.timeManager, dt.timedelta(seconds=dtv))
        for _ in range(2):
            mk.ocn_timestep(Prog, Diag, Tend, Setup, mk.RungeKutta4)
            tw.step_rk4(st, dtv)
        check_levels(Prog, st)
        Prog._state.close(); Setup.mesh.close()
    finally:
        backend.set_kernel_variant(0)


def test_del4_switching_and_refusals(backend):
    mesh = get_mesh("ico16")
    K = 8
    ssh, u, h, rest = random_state(mesh, K, 17)
    dtv = 20.0
    v2, v4 = viscosities(mesh, dtv)
    lib = L.lib()
    Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, CONFIG, backend, multilayer=True)
    sh = Prog._state._h
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=K)
    with pytest.raises(mk.MokaError, match="moka_set_nonlinear"):                    # no nonlinear terms yet
        L.check(lib.moka_set_viscosity_del4(sh, v4, None), Setup.mesh.backend._h)
    assert lib.moka_set_viscosity_del4(sh, 0.0, None) == 0                            # off is always fine
    mk.set_nonlinear(Prog, True)
    assert lib.moka_set_viscosity_del4(sh, -1.0, None) == L.ERR_ARG
    bad = np.ones(mesh.nEdges); bad[3] = -0.5
    assert lib.moka_set_viscosity_del4(sh, v4, bad.ctypes.data) == L.ERR_ARG
    mk.set_nonlinear(Prog, True, visc_del4=v4)
    # Forward Euler and tapes stay refused
    with pytest.raises(mk.MokaError):
        mk.ocn_timestep(np.array([dtv]), Prog, Diag, Tend, Setup, mk.ForwardEuler)
    with pytest.raises(mk.MokaError):
        mk.AdjointTape(Prog, 2)
    # a halo cannot be created on a Del4 state
    z32, z64 = np.zeros(1, np.int32), np.zeros(1, np.int64)
    p32, p64 = z32.ctypes.data_as(C.POINTER(C.c_int32)), z64.ctypes.data_as(C.POINTER(C.c_int64))
    hh = C.c_void_p()
    assert lib.moka_halo_create(sh, 0, p32, p64, p32, p64, p32, p64, p32, p64, 0, 0, C.byref(hh)) == L.ERR_UNSUPPORTED
    assert not hh.value
    # the 13-stream form is not restated for Del4: the running sum
    L.check(lib.moka_set_tuning(7, 1))
    try:
        assert lib.moka_state_rk4_streams(sh) == 16
        st = TwinState(ssh, u, h)
        tw = Del4Twin(om, visc_del4=v4)
        mk.changeTimeStep(Setup.timeManager, dt.timedelta(seconds=dtv))
        mk.ocn_timestep(Prog, Diag, Tend, Setup, mk.RungeKutta4)
        tw.step_rk4(st, dtv)
        check_levels(Prog, st)
    finally:
        L.check(lib.moka_set_tuning(7, 0))
    # Del4 off again: the plain nonlinear form, bit for bit
    mk.set_nonlinear(Prog, True, visc_del4=0.0)
    plain = orc.OracleNonlinear(om)
    ost = orc.OracleState(om, st.ssh[1], st.u[1], st.h[1])
    mk.ocn_timestep(Prog, Diag, Tend, Setup, mk.RungeKutta4)
    plain.step_rk4(ost, dtv)
    assert np.array_equal(Prog.normalVelocity[-1].get(), ost.u[1]) and np.array_equal(Prog.ssh[-1].get(), ost.ssh[1])
    Prog._state.close(); Setup.mesh.close()


def test_del4_refused_on_fp32_states(backend):
    mesh = get_mesh("ico16")
    ssh, u, h, rest = random_state(mesh, 4, 2)
    Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, CONFIG, backend, multilayer=True, state_bytes=4)
    assert L.lib().moka_set_viscosity_del4(Prog._state._h, 1.0, None) == L.ERR_UNSUPPORTED
    Prog._state.close(); Setup.mesh.close()


def test_del4_refused_on_a_rank_with_a_halo():
    """One rank of a two-way LocalCluster (nonlinear terms, two-ring halo): Del4 cannot be switched on while its halo exists."""
    from moka_hip import parallel as par
    mesh = get_mesh("ico16")
    K = 4
    ssh, u, h, rest = random_state(mesh, K, 12)
    cl = par.LocalCluster(mesh, ssh, u, h, rest, 20.0, 2, direct=False, nonlinear=True)
    try:
        rc = L.lib().moka_set_viscosity_del4(cl.models[0].Prog._state._h, 1.0, None)
        assert rc == L.ERR_UNSUPPORTED
    finally:
        cl.close()


def test_del4_damps_a_run(backend):
    """f = 0, viscDel4 = 0.002 dcEdge.min()^4 / dt, 100 RK4 steps through graph replay: kinetic energy stays finite and ends below the
    same run without Del4; the result equals the twin's 100 steps (bitwise expected; the bar is 1e-10 relative)."""
    mesh = get_mesh("planar0")
    K = 4
    ssh, u, h, rest = random_state(mesh, K, 31)
    u *= 0.1
    dtv = 2.0
    _, v4 = viscosities(mesh, dtv)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=K)
    w = (mesh.dcEdge * mesh.dvEdge)[:, None]
    ke = {}
    for visc in (0.0, v4):
        Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, CONFIG, backend, multilayer=True)
        mk.set_nonlinear(Prog, True, visc_del4=visc)
        mk.run_steps(Prog, mk.RungeKutta4, dtv, 100)
        got = Prog.normalVelocity[-1].get()
        ke[visc] = float(np.sum(w * got ** 2))
        assert np.isfinite(ke[visc])
        if visc:
            tw, st = Del4Twin(om, visc_del4=visc), TwinState(ssh, u, h)
            for _ in range(100):
                tw.step_rk4(st, dtv)
            assert np.max(np.abs(got - st.u[1])) <= 1e-10 * np.max(np.abs(st.u[1]))
            assert np.max(np.abs(Prog.layerThickness[-1].get() - st.h[1])) <= 1e-10 * np.max(np.abs(st.h[1]))
        Prog._state.close(); Setup.mesh.close()
    assert ke[v4] < ke[0.0], ke
