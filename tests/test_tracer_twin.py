"""Passive tracer transport: the numpy twin (tests/tracer_twin.py) against its long-double restatement, the scheme's identities
(a constant tracer stays constant bit for bit, the content is conserved to round-off), self-tests that show the checks rejecting, and
the C ABI / host-layer entry points.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import oracle as orc
import tracer_cases as tc
import tracer_twin as tt
import trisk_reference as tr
from del4_twin import Del4Twin, TwinState
from moka_hip import meshgen as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MESHES = {}


def get_mesh(name):
    if name not in _MESHES:
        _MESHES[name] = {"planar": lambda: mg.planar_hex_mesh(20, 18, 1000.0, f0=1e-4),
                         "ico16": lambda: mg.icosahedral_mesh(16),
                         "ico12f": lambda: mg.icosahedral_mesh(12, flips=8, seed=4)}[name]()
    return _MESHES[name]


def random_state(mesh, K, seed):
    rng = np.random.default_rng(seed)
    rest = np.full((mesh.nCells, K), 1000.0 / K) + rng.uniform(0, 0.1, (mesh.nCells, K))
    h = rest + rng.uniform(-1, 1, (mesh.nCells, K))
    u = rng.uniform(-1, 1, (mesh.nEdges, K))
    return h.sum(1) - rest.sum(1), u, h, rest


def smooth_tracer(mesh, K, seed):
    """A smooth field in [0.5, 1.5]: a few random low wavenumbers of the cell positions, another phase per level."""
    rng = np.random.default_rng(seed)
    x = np.stack([mesh.xCell, mesh.yCell, mesh.zCell], axis=1)
    x = x / max(float(np.abs(x).max()), 1.0)
    w = rng.uniform(-4, 4, (3, 3))
    ph = rng.uniform(0, 2 * np.pi, (3, K))
    f = sum(np.sin(x @ w[j][:, None] + ph[j][None, :]) for j in range(3)) / 3.0
    return 1.0 + 0.5 * f


def partial_mlt(mesh, K, seed=8):
    rng = np.random.default_rng(seed)
    mlt = np.where(rng.random(mesh.nEdges) < 0.33, rng.integers(0, K + 1, mesh.nEdges), K).astype(np.int32)
    mlt[:3] = 0
    return mlt


def bases(om, mesh, dtv):
    dcmin = float(mesh.dcEdge.min())
    return {"linear": om, "nonlinear": orc.OracleNonlinear(om),
            "del2+del4": Del4Twin(om, visc_del2=0.01 * dcmin ** 2 / dtv, visc_del4=0.002 * dcmin ** 4 / dtv)}


def dt_of(meshname):
    return 2.0 if meshname == "planar" else 20.0


def check_T(twin, mesh, u, h, phi, mlt):
    ref, M = tt.tendency_ld(mesh, u, h, phi, mlt)
    return tr.within(twin.tendency(u, h, phi), ref, M, tt.C_T)


@pytest.mark.parametrize("partial", [False, True], ids=["full", "partial"])
@pytest.mark.parametrize("K", [1, 5, 34])
@pytest.mark.parametrize("meshname", ["ico16", "planar", "ico12f"])
def test_twin_tendency_within_bound_of_long_double(meshname, K, partial):
    """Per element |T - T_ref| <= C_T 2^-53 M (C_T = 18, tracer_twin.py counts the chain), with full and with partial edge masks
    (maxLevelEdgeTop = 0 included)."""
    mesh = get_mesh(meshname)
    _, u, h, rest = random_state(mesh, K, 7 + K)
    mlt = partial_mlt(mesh, K) if partial else np.full(mesh.nEdges, K, dtype=np.int32)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=mlt)
    twin = tt.TracerTwin(om, om)
    phi = smooth_tracer(mesh, K, 3)
    assert phi.min() >= 0.5 and phi.max() <= 1.5
    ok = check_T(twin, mesh, u, h, phi, mlt)
    assert ok.all(), int((~ok).sum())
    assert np.abs(twin.tendency(u, h, phi)).max() > 0


@pytest.mark.parametrize("partial", [False, True], ids=["full", "partial"])
@pytest.mark.parametrize("meshname,K", [("ico16", 5), ("ico12f", 3), ("planar", 4)])
def test_unit_tracer_tendency_is_the_thickness_tendency(meshname, K, partial):
    """With phi == 1 the twin's T equals the oracle's tendLayerThickness bit for bit: the operand order is the thickness tendency's."""
    mesh = get_mesh(meshname)
    _, u, h, rest = random_state(mesh, K, 11)
    mlt = partial_mlt(mesh, K) if partial else K
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=mlt)
    twin = tt.TracerTwin(om, om)
    assert np.array_equal(twin.tendency(u, h, np.ones_like(h)), om.tendencies_clean(u, h)[1])


def test_twin_stage_loop_is_the_oracles():
    """The dycore part of TracerTwin.step_rk4 over the linear base is oracle_step_rk4, bit for bit, both time levels."""
    mesh = get_mesh("ico16")
    K = 5
    ssh, u, h, rest = random_state(mesh, K, 2)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=K)
    a, b = orc.OracleState(om, ssh, u, h), TwinState(ssh, u, h)
    twin = tt.TracerTwin(om, om)
    phis = [[np.ones_like(h)], [np.ones_like(h)]]
    for _ in range(3):
        a.step_rk4(20.0)
        twin.step_rk4(b, phis, 20.0)
    for lev in (0, 1):
        assert np.array_equal(b.u[lev], a.u[lev]) and np.array_equal(b.h[lev], a.h[lev]) and np.array_equal(b.ssh[lev], a.ssh[lev])


@pytest.mark.parametrize("mode", ["linear", "nonlinear", "del2+del4"])
@pytest.mark.parametrize("meshname,K", [("ico16", 5), ("ico12f", 3)])
def test_unit_tracer_stays_exactly_one(meshname, K, mode):
    """phi == 1 is exactly 1.0 after 5 twin steps over each dycore base, at both time levels; a random tracer beside it moves."""
    mesh = get_mesh(meshname)
    ssh, u, h, rest = random_state(mesh, K, 5)
    dtv = dt_of(meshname)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=K)
    twin = tt.TracerTwin(om, bases(om, mesh, dtv)[mode])
    st = TwinState(ssh, u, h)
    other = smooth_tracer(mesh, K, 9)
    phis = [[np.ones_like(h), other.copy()], [np.ones_like(h), other.copy()]]
    for _ in range(5):
        twin.step_rk4(st, phis, dtv)
    one = np.ones_like(h)
    assert np.array_equal(phis[1][0], one) and np.array_equal(phis[0][0], one)
    assert not np.array_equal(phis[1][1], other) and np.isfinite(phis[1][1]).all()


@pytest.mark.parametrize("partial", [False, True], ids=["full", "partial"])
@pytest.mark.parametrize("meshname,K", [("ico16", 5), ("planar", 4), ("ico12f", 3)])
def test_content_is_conserved_to_the_bound(meshname, K, partial):
    """sum_c A_c sum_k phi h in long double changes per step by no more than tracer_twin.content_bound (derived in that file's
    docstring from the magnitudes of Qc and T), over 4 steps of the nonlinear dycore."""
    mesh = get_mesh(meshname)
    ssh, u, h, rest = random_state(mesh, K, 6)
    dtv = dt_of(meshname)
    mlt = partial_mlt(mesh, K) if partial else K
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=mlt)
    twin = tt.TracerTwin(om, orc.OracleNonlinear(om))
    st = TwinState(ssh, u, h)
    phi = smooth_tracer(mesh, K, 4)
    phis = [[phi.copy()], [phi.copy()]]
    for _ in range(4):
        s0 = tt.content(mesh, phis[1][0], st.h[1])
        twin.step_rk4(st, phis, dtv, magnitudes=True)
        s1 = tt.content(mesh, phis[1][0], st.h[1])
        bound = tt.content_bound(mesh, *twin.last_M[0])
        assert abs(s1 - s0) <= bound, (float(s1 - s0), float(bound))
        assert bound <= 1e-12 * abs(s0)                   # the bound is a round-off bound, not a loose one
    assert np.abs(phis[1][0] - phi).max() > 1e-6           # ... and the tracer did move


# ---- self-tests: the checks reject -----------------------------------------------------------------------------------------------
def _selftest_setup(K=5):
    mesh = get_mesh("ico16")
    _, u, h, rest = random_state(mesh, K, 13)
    mlt = partial_mlt(mesh, K)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=mlt)
    return mesh, u, h, mlt, om, smooth_tracer(mesh, K, 5)


def test_check_rejects_one_sdv_entry_off_by_1e9():
    mesh, u, h, _, om, phi = _selftest_setup()
    full = np.full(mesh.nEdges, 5, dtype=np.int32)
    om = orc.OracleMesh(mesh, 5, max_level_edge_top=full)
    twin = tt.TracerTwin(om, om)
    assert check_T(twin, mesh, u, h, phi, full).all()
    twin.sdv[17, 2] *= 1.0 + 1e-9
    ok = check_T(twin, mesh, u, h, phi, full)
    assert not ok[17].all() and ok[np.arange(mesh.nCells) != 17].all()


def test_check_rejects_an_edge_value_from_one_cell_only():
    mesh, u, h, mlt, om, phi = _selftest_setup()
    twin = tt.TracerTwin(om, om)
    assert check_T(twin, mesh, u, h, phi, mlt).all()
    twin.edge_value = lambda pphi, i: pphi
    ok = check_T(twin, mesh, u, h, phi, mlt)
    assert (~ok).mean() > 0.5
    # (a constant tracer cannot tell: the long-double reference is what catches this one)
    assert np.array_equal(twin.tendency(u, h, np.ones_like(h)), om.tendencies_clean(u, h)[1])


def test_check_rejects_a_slot_mask_from_the_cells_level_count():
    mesh, u, h, mlt, om, phi = _selftest_setup()
    twin = tt.TracerTwin(om, om)
    cell_levels = np.where(twin.valid, mlt[twin.eoc], 0).max(axis=1)          # the deepest edge of the cell
    twin.slot_mask = lambda i: twin.valid[:, i, None] & (np.arange(twin.K)[None, :] < cell_levels[:, None])
    ok = check_T(twin, mesh, u, h, phi, mlt)
    assert not ok.all()
    # ... and the constant tracer no longer reproduces the thickness tendency either
    assert not np.array_equal(twin.tendency(u, h, np.ones_like(h)), om.tendencies_clean(u, h)[1])


def test_content_check_rejects_a_non_conservative_edge_value():
    """An edge value taken from the cell's own side breaks the pairing of the two cells of an edge: the content drifts past the bound."""
    mesh = get_mesh("ico16")
    K = 5
    ssh, u, h, rest = random_state(mesh, K, 6)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=K)
    twin = tt.TracerTwin(om, om)
    twin.edge_value = lambda pphi, i: pphi
    st = TwinState(ssh, u, h)
    phi = smooth_tracer(mesh, K, 4)
    phis = [[phi.copy()], [phi.copy()]]
    s0 = tt.content(mesh, phi, h)
    twin.step_rk4(st, phis, 20.0, magnitudes=True)
    assert abs(tt.content(mesh, phis[1][0], st.h[1]) - s0) > tt.content_bound(mesh, *twin.last_M[0])


def test_tracer_entry_points_exist():
    """The library exports the tracer entry points, the header declares them, the Python layer and the Julia shim wrap them."""
    import moka_hip as mk
    from moka_hip import lib as L
    lib = L.lib()
    names = ("moka_set_tracers", "moka_tracer_upload", "moka_tracer_download", "moka_state_tracer_path")
    for name in names:
        assert hasattr(lib, name), name
        assert name in L.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "moka_hip.h")).read()
    assert re.search(r"int\s+moka_set_tracers\(moka_state \*st, int32_t nTracers\);", hdr)
    assert re.search(r"int\s+moka_tracer_upload\(moka_state \*st, int32_t j, int time_level, const double \*host\);", hdr)
    assert re.search(r"int\s+moka_tracer_download\(moka_state \*st, int32_t j, int time_level, double \*host\);", hdr)
    assert re.search(r"int\s+moka_state_tracer_path\(const moka_state \*st\);", hdr)
    jl = open(os.path.join(ROOT, "mpas-ocean.jl_amd", "julia", "MokaHIP.jl")).read()
    for name in names:
        assert f"ccall((:{name}, lib)" in jl, name
    assert callable(mk.set_tracers) and hasattr(mk.Tracers, "get") and hasattr(mk.Tracers, "set") and hasattr(mk.Tracers, "path")
    mk_src = open(os.path.join(ROOT, "mpas-ocean.jl_amd", "Makefile")).read()
    assert "tracers.o" in mk_src


# ---- repeated neighbours, and the stage weights ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,K", tc.TINY)
def test_twin_tendency_on_tiny_periodic_meshes(nx, ny, K):
    """The smallest doubly periodic meshes, where a cell meets the same neighbour through several slots (2 x 4, 4 x 2: through both
    boundaries): per element |T - T_ref| <= C_T 2^-53 M as on the large meshes, and the unit tracer's T is tendLayerThickness.  The
    GPU test on these meshes (test_gpu_tracer_shapes.py) rests on a twin known to handle them."""
    mesh = tc.get_mesh(f"tiny-{nx}-{ny}")
    _, u, h, rest = tc.state_of(f"tiny-{nx}-{ny}", K)
    mlt = np.full(mesh.nEdges, K, dtype=np.int32)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=mlt)
    twin = tt.TracerTwin(om, om)
    for phi in tc.distinct_fields(mesh, K, 2):
        ok = check_T(twin, mesh, u, h, phi, mlt)
        assert ok.all(), int((~ok).sum())
    assert np.array_equal(twin.tendency(u, h, np.ones_like(h)), om.tendencies_clean(u, h)[1])


def _eigenmode_run(twin_cls):
    mesh, (ssh, u, h, rest), phi0 = tc.eigenmode_state(4)
    om = orc.OracleMesh(mesh, 4, resting_thickness_sum=rest.sum(1), max_level_edge_top=4)
    twin = twin_cls(om, om)
    st = TwinState(ssh, u, h)
    phis = [[phi0.copy()], [phi0.copy()]]
    for _ in range(tc.EIG_STEPS):
        twin.step_rk4(st, phis, tc.EIG_DT)
    assert np.array_equal(st.u[1], u) and np.array_equal(st.h[1], h)          # the uniform flow is steady, exactly
    return mesh, phis[1][0], phi0


def test_advection_is_integrated_by_rk4_on_an_exact_eigenmode():
    """A plane wave in a uniform flow U = (70, 40) over regular hexagons (tracer_cases.py derives the mode): 10 steps of
    phi0 = 1 + 0.5 cos(k . x) must give 1 + 0.5 Re(R(z)^10 exp(i k . x)), z = mu dt, R the RK4 stability polynomial, within
    10 steps * 32 * 2^-53 * max|phi0| = 5.3e-14 (the diffusion eigenmode test's tolerance).  z is imaginary here, so this pins the
    stage weights a, b and the Qc / Qn recipe where the unit-tracer and the content identities, which hold for any weights, cannot.
    Measured on the CPU: z = -0.11201i, |R|^10 = 1.00000, deviation 1.3e-15; the same bound refuses a third-order loop by 3.3e-5
    and the exact exponential by 7.3e-7; the dycore drift is exactly 0."""
    mesh, phi, phi0 = _eigenmode_run(tt.TracerTwin)
    tc.eigenmode_check(phi, mesh, 4, 0.0, phi0, "TracerTwin, kappa = 0")
