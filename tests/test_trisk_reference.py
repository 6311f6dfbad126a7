"""The oracle and the Del4 twin against the independent long-double reference (tests/trisk_reference.py), per element within the
reference's error bound, and the discrete identities of the TRiSK scheme on both.  The optional terms (nonlinear, Del2, Del4) have no
reference output to be pinned to; this is their anchor.  Every check is shown to reject a subtly wrong result (the sensitivity
self-tests at the end).  No GPU needed."""
import dataclasses

import numpy as np
import pytest

import oracle as orc
import trisk_reference as tr
from del4_twin import Del4Twin
from moka_hip import meshgen as mg

_MESHES = {}


def get_mesh(name):
    if name not in _MESHES:
        _MESHES[name] = {"ico8": lambda: mg.icosahedral_mesh(8),
                         "ico12f": lambda: mg.icosahedral_mesh(12, flips=8, seed=4),    # signed kites, 5- and 7-gons
                         "planar": lambda: mg.planar_hex_mesh(20, 18, 1000.0, f0=1e-4)}[name]()
    return _MESHES[name]


def random_state(mesh, K, seed, uamp=1.0):
    rng = np.random.default_rng(seed)
    rest = np.full((mesh.nCells, K), 1000.0 / K) + rng.uniform(0, 0.1, (mesh.nCells, K))
    h = rest + rng.uniform(-1, 1, rest.shape)
    u = uamp * rng.uniform(-1, 1, (mesh.nEdges, K))
    return u, h, rest.sum(1)


def edge_mask(mesh, K, kind, seed=3):
    """full: K everywhere; partial: maxLevelEdgeTop < K (0 included) on a third of the edges."""
    if kind == "full":
        return np.full(mesh.nEdges, K, dtype=np.int32)
    rng = np.random.default_rng(seed)
    mlt = np.where(rng.random(mesh.nEdges) < 1 / 3, rng.integers(0, K, mesh.nEdges), K).astype(np.int32)
    mlt[:3] = 0
    return mlt


def viscosities(mesh):
    dcmin = float(mesh.dcEdge.min())
    dtv = 0.2 * dcmin / np.sqrt(tr.G * 1000.0)
    return float(0.01 * dcmin ** 2 / dtv), float(0.002 * dcmin ** 4 / dtv)


def assert_within(x, ref, M, C, what):
    ok = tr.within(x, ref, M, C)
    if not ok.all():
        i = np.unravel_index(np.argmin(ok), ok.shape)
        raise AssertionError(f"{what}: {int((~ok).sum())} elements outside {C} * 2^-53 * M; first {i}: "
                             f"got {float(np.asarray(x)[i])!r}, reference {float(ref[i])!r}, M {float(M[i])!r}")


# ---- reference vs oracle / twin ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["full", "partial"])
@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("meshname", ["ico8", "ico12f", "planar"])
def test_oracle_and_twin_within_the_reference_bound(meshname, K, mask):
    """Linear, nonlinear, + Del2, + Del4, Del2 + Del4 with a scaling array: tendU, tendH and ssh of the oracle (OracleMesh /
    OracleNonlinear) and the twin (Del4Twin) per element within C 2^-53 M of the long-double reference."""
    mesh = get_mesh(meshname)
    u, h, rs = random_state(mesh, K, 40 + K)
    mlt = edge_mask(mesh, K, mask)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rs, max_level_edge_top=mlt)
    v2, v4 = viscosities(mesh)
    lin = tr.terms(mesh, u, h, rs, mlt, nonlinear=False)
    tu, th, ssh = om.tendencies_clean(u, h)
    assert_within(tu, *lin["U"], tr.C_U, "linear tendU")
    assert_within(th, *lin["H"], tr.C_H, "linear tendH")
    assert_within(ssh, *lin["ssh"], tr.C_SSH, "ssh")
    nl = tr.terms(mesh, u, h, rs, mlt, nonlinear=True)
    scaling = np.random.default_rng(K).uniform(0.5, 2.0, mesh.nEdges)
    for name, a, b, s in (("nonlinear", 0.0, 0.0, None), ("+Del2", v2, 0.0, None), ("+Del4", 0.0, v4, None),
                          ("+Del2+Del4 scaled", v2, v4, scaling)):
        if b:
            tu, th, ssh = Del4Twin(om, visc_del2=a, visc_del4=b, scaling=s).tendencies(u, h)
        else:
            tu, th, ssh, _ = (orc.OracleNonlinear(om, visc_del2=a) if a else orc.OracleNonlinear(om)).tendencies(u, h)
        U, MU = tr.combine(nl, a, b, s)
        assert_within(tu, U, MU, tr.C_U, f"{name} tendU")
        assert_within(th, *nl["H"], tr.C_H, f"{name} tendH")
        assert_within(ssh, *nl["ssh"], tr.C_SSH, f"{name} ssh")
        assert not np.array_equal(U, nl["U"][0]) or not (a or b)


def test_reference_tendencies_entry_point_matches_the_terms():
    """tendencies() (one combination) and terms() + combine() (all of them from one pass) are the same long-double numbers."""
    mesh = get_mesh("ico12f")
    u, h, rs = random_state(mesh, 2, 7)
    mlt = edge_mask(mesh, 2, "partial")
    v2, v4 = viscosities(mesh)
    t = tr.terms(mesh, u, h, rs, mlt, nonlinear=True)
    tu, th, ssh = tr.tendencies(mesh, u, h, rs, mlt, nonlinear=True, visc_del2=v2, visc_del4=v4)
    mu, mh, ms = tr.tendencies(mesh, u, h, rs, mlt, nonlinear=True, visc_del2=v2, visc_del4=v4, abs=True)
    U, MU = tr.combine(t, v2, v4)
    assert np.array_equal(tu, U) and np.array_equal(mu, MU)
    assert np.array_equal(th, t["H"][0]) and np.array_equal(mh, t["H"][1]) and np.array_equal(ms, t["ssh"][1])
    assert (mu >= np.abs(tu)).all() and (mh >= np.abs(th)).all() and (ms >= np.abs(ssh)).all()
    assert not tu[mlt == 0].any()                                     # inactive levels carry no tendency


def test_rk4_reference_against_the_oracle_step():
    """One nonlinear + Del2 RK4 step: the oracle within 1e-12 (max-norm relative) of the long-double RK4."""
    mesh = get_mesh("ico8")
    K = 3
    u, h, rs = random_state(mesh, K, 5)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rs, max_level_edge_top=K)
    v2, _ = viscosities(mesh)
    dtv = 0.2 * float(mesh.dcEdge.min()) / np.sqrt(tr.G * 1000.0)
    st = orc.OracleState(om, h.sum(1) - rs, u, h)
    orc.OracleNonlinear(om, visc_del2=v2).step_rk4(st, dtv)
    ru, rh, rssh = tr.rk4(mesh, u, h, rs, np.full(mesh.nEdges, K), dtv, nonlinear=True, visc_del2=v2)
    for got, ref in ((st.u[1], ru), (st.h[1], rh), (st.ssh[1], rssh)):
        assert float(np.abs(got - ref).max() / np.abs(ref).max()) <= 1e-12
    assert float(np.abs(st.u[1] - u).max()) > 1e-6 * float(np.abs(u).max())      # the step did something


# ---- identities of the scheme ----------------------------------------------------------------------------------------------------
def inviscid_cases(meshname, K, mask, seed):
    """State with u = 0 on the inactive levels (MPAS's state) and the oracle's tendencies of it."""
    mesh = get_mesh(meshname)
    u, h, rs = random_state(mesh, K, seed, uamp=5.0)
    mlt = edge_mask(mesh, K, mask)
    u = np.where(np.arange(K)[None, :] < mlt[:, None], u, 0.0)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rs, max_level_edge_top=mlt)
    return mesh, u, h, rs, mlt, om


@pytest.mark.parametrize("mask", ["full", "partial"])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("meshname", ["ico8", "ico12f", "planar"])
def test_energy_and_mass_budgets(meshname, K, mask):
    """Inviscid nonlinear tendencies conserve total energy and mass: on the reference (to its own round-off) and on the oracle's
    output (within the summed bounds)."""
    mesh, u, h, rs, mlt, om = inviscid_cases(meshname, K, mask, 60 + K)
    ref = tr.terms(mesh, u, h, rs, mlt, nonlinear=True, mixing=False)
    tu, th, ssh, _ = orc.OracleNonlinear(om).tendencies(u, h)
    # bounds with the oracle's ssh as a leaf: the pressure work cancels against the ssh the gradient was formed from
    MU, MH, _ = tr.tendencies(mesh, u, h, rs, mlt, nonlinear=True, abs=True, ssh=ssh)
    for name, U, H, S in (("reference", ref["U"][0], ref["H"][0], ref["ssh"][0]), ("oracle", tu, th, ssh)):
        res, tol = tr.energy_budget(mesh, u, h, S, U, H, MU, MH)
        assert abs(res) <= tol, (name, float(res), float(tol))
        mres, mtol = tr.mass_budget(mesh, H, MH)
        assert (np.abs(mres) <= mtol).all(), (name, mres, mtol)
    res, tol = tr.energy_budget(mesh, u, h, ref["ssh"][0], ref["U"][0], ref["H"][0], MU, MH)
    assert abs(res) <= tol * 2.0 ** -8                      # the reference alone: far inside (2^-64 round-off)


@pytest.mark.parametrize("meshname", ["ico8", "ico12f", "planar"])
def test_pv_compatibility(meshname):
    """fVertex = q0 h_v - zeta_v makes q uniform; then curl(tendU)_v = q0 sum_j kite_j tendH_{c_j} / areaTriangle_v (Ringler et al.
    2010: the PV flux is consistent with the thickness equation).  Reference and oracle, every vertex."""
    mesh = get_mesh(meshname)
    u, h, rs = random_state(mesh, 1, 77, uamp=5.0)
    q0 = 1e-4 / 1000.0
    fv = tr.uniform_q_fvertex(mesh, u, h, q0)
    m2 = dataclasses.replace(mesh, fVertex=fv)
    mlt = np.ones(mesh.nEdges, dtype=np.int32)
    om = orc.OracleMesh(m2, 1, resting_thickness_sum=rs, max_level_edge_top=1)
    tu, th, ssh, diag = orc.OracleNonlinear(om).tendencies(u, h)
    assert float(np.abs(diag["pv_vertex"] - q0).max()) <= 1e-12 * q0
    ref = tr.terms(m2, u, h, rs, mlt, nonlinear=True, mixing=False)
    MU, MH, _ = tr.tendencies(m2, u, h, rs, mlt, nonlinear=True, abs=True, ssh=ssh)
    for name, U, H in (("reference", ref["U"][0], ref["H"][0]), ("oracle", tu, th)):
        res, tol = tr.pv_compatibility(mesh, q0, U, H, MU, MH)
        assert (np.abs(res) <= tol).all(), (name, float(np.max(np.abs(res) / tol)))


def rotational_and_divergent(mesh, seed):
    rng = np.random.default_rng(seed)
    psi, phi = rng.standard_normal(mesh.nVertices), rng.standard_normal(mesh.nCells)
    v1, v2 = mesh.verticesOnEdge[:, 0] - 1, mesh.verticesOnEdge[:, 1] - 1
    c1, c2 = mesh.cellsOnEdge[:, 0] - 1, mesh.cellsOnEdge[:, 1] - 1
    return ((psi[v2] - psi[v1]) / mesh.dvEdge)[:, None], ((phi[c2] - phi[c1]) / mesh.dcEdge)[:, None]


@pytest.mark.parametrize("meshname", ["ico8", "ico12f", "planar"])
def test_del2_self_adjoint_and_del4_dissipative(meshname):
    """<v, L u>_e = -<div u, div v>_c - <zeta u, zeta v>_v with <a, b>_e = sum dc dv a b, <,>_c over areaCell, <,>_v over
    areaTriangle; <u, L u> < 0 for a purely rotational and a purely divergent u; <u, L(L(u))> >= 0.  For the reference's L and the
    twin's (the oracle's operators)."""
    mesh = get_mesh(meshname)
    g = tr.geometry(mesh)
    rng = np.random.default_rng(3)
    u, v = rng.uniform(-1, 1, (mesh.nEdges, 1)), rng.uniform(-1, 1, (mesh.nEdges, 1))
    act = np.ones((mesh.nEdges, 1), dtype=bool)
    twin = Del4Twin(orc.OracleMesh(mesh, 1, max_level_edge_top=1), visc_del4=1.0)
    wE = tr._col(g.dc * g.dv)
    ul, vl = u.astype(tr.LD), v.astype(tr.LD)
    du, dv_ = tr.divergence(g, ul)[0], tr.divergence(g, vl)[0]
    zu, zv = tr.curl(g, ul)[0], tr.curl(g, vl)[0]
    rhs = -(tr._col(g.areaC) * du * dv_).sum() - (tr._col(g.areaT) * zu * zv).sum()
    Lu, MLu = tr.laplacian(g, ul, np.abs(ul), act)
    for name, L in (("reference", Lu), ("twin", twin.L(u))):
        lhs = (wE * vl * tr._ld(L, Lu.shape)).sum()
        assert abs(lhs - rhs) <= tr.C_U * tr.U53 * (wE * np.abs(vl) * MLu).sum(), (name, float(lhs), float(rhs))
    for w in rotational_and_divergent(mesh, 5):
        wl = w.astype(tr.LD)
        for L in (tr.laplacian(g, wl, None, act)[0], twin.L(w)):
            assert (wE * wl * tr._ld(L, wl.shape)).sum() < 0
    LLu = tr.laplacian(g, Lu, None, act)[0]
    assert (wE * ul * LLu).sum() >= 0 and (wE * u * twin.del4_bracket(u)).sum() >= 0


@pytest.mark.parametrize("meshname", ["ico8", "ico12f", "planar"])
def test_mesh_properties_the_identities_rest_on(meshname):
    """TRiSK antisymmetry dc_e dv_e w_ee' = -dc_e' dv_e' w_e'e (equivalently dc_e w_ee' / dv_e' is antisymmetric), and
    curl(grad(phi)) = 0."""
    mesh = get_mesh(meshname)
    a, b = tr.coriolis_pairs(mesh)
    assert not np.isnan(b).any(), "an edgesOnEdge entry without its mirror"
    assert (np.abs(a + b) <= 1e-13 * np.abs(a).max()).all()
    g = tr.geometry(mesh)
    phi = np.random.default_rng(1).standard_normal((mesh.nCells, 1)).astype(tr.LD)
    gr, mgr = tr.grad_cell(g, phi, np.abs(phi))
    z, mz = tr.curl(g, gr, mgr)
    assert (np.abs(z) <= 16 * tr.LD(2.0) ** -63 * mz).all()


# ---- sensitivity: each check rejects a subtly wrong result ---------------------------------------------------------------------
# On ico12f (signed kites, 5- and 7-gons).  The planar hexagon mesh has uniform kites and weights, so wrong kite or weight slots are
# invisible there; it is not used for these.
def _fails(x, ref, M, C):
    return not tr.within(x, ref, M, C).all()


def test_sensitivity_kites_rotated_at_one_vertex():
    mesh = get_mesh("ico12f")
    u, h, rs = random_state(mesh, 1, 77, uamp=5.0)
    q0 = 1e-7
    fv = tr.uniform_q_fvertex(mesh, u, h, q0)
    good = dataclasses.replace(mesh, fVertex=fv)
    kites = mesh.kiteAreasOnVertex.copy()
    v = int(np.argmax(kites.max(1) - kites.min(1)))
    kites[v] = np.roll(kites[v], 1)
    bad = dataclasses.replace(good, kiteAreasOnVertex=kites)
    mlt = np.ones(mesh.nEdges, dtype=np.int32)
    tu, th, ssh, _ = orc.OracleNonlinear(orc.OracleMesh(bad, 1, resting_thickness_sum=rs, max_level_edge_top=1)).tendencies(u, h)
    U, MU = tr.combine(tr.terms(good, u, h, rs, mlt, nonlinear=True, mixing=False))
    assert _fails(tu, U, MU, tr.C_U)
    MU, MH, _ = tr.tendencies(good, u, h, rs, mlt, nonlinear=True, abs=True, ssh=ssh)
    res, tol = tr.pv_compatibility(good, q0, tu, th, MU, MH)
    assert not (np.abs(res) <= tol).all()


def test_sensitivity_one_weight_scaled():
    mesh = get_mesh("ico12f")
    u, h, rs = random_state(mesh, 1, 78, uamp=5.0)
    g = tr.geometry(mesh)
    F = u[:, 0] * (h[g.c1, 0] + h[g.c2, 0]) / 2
    size = np.abs(mesh.weightsOnEdge * F[g.eoe]) * g.e_ok * (mesh.dcEdge * mesh.dvEdge * np.abs(F))[:, None]
    e, j = np.unravel_index(int(np.argmax(size)), size.shape)
    w = mesh.weightsOnEdge.copy()
    w[e, j] *= 1 + 1e-9
    bad = dataclasses.replace(mesh, weightsOnEdge=w)
    mlt = np.ones(mesh.nEdges, dtype=np.int32)
    om = orc.OracleMesh(bad, 1, resting_thickness_sum=rs, max_level_edge_top=1)
    tu, th, ssh, _ = orc.OracleNonlinear(om).tendencies(u, h)
    U, MU = tr.combine(tr.terms(mesh, u, h, rs, mlt, nonlinear=True, mixing=False))
    assert _fails(tu, U, MU, tr.C_U)
    MU, MH, _ = tr.tendencies(mesh, u, h, rs, mlt, nonlinear=True, abs=True, ssh=ssh)
    res, tol = tr.energy_budget(mesh, u, h, ssh, tu, th, MU, MH)
    assert abs(res) > tol
    a, b = tr.coriolis_pairs(bad)
    assert not (np.abs(a + b) <= 1e-13 * np.abs(a).max()).all()
    # and the linear form (Coriolis over the same weights)
    tu = om.tendencies_clean(u, h)[0]
    assert _fails(tu, *tr.terms(mesh, u, h, rs, mlt, nonlinear=False)["U"], tr.C_U)


def test_sensitivity_one_tendency_element():
    mesh = get_mesh("ico12f")
    K = 3
    u, h, rs = random_state(mesh, K, 79, uamp=5.0)
    mlt = np.full(mesh.nEdges, K, dtype=np.int32)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rs, max_level_edge_top=K)
    tu, th, ssh, _ = orc.OracleNonlinear(om).tendencies(u, h)
    ref = tr.terms(mesh, u, h, rs, mlt, nonlinear=True, mixing=False)
    MU, MH, _ = tr.tendencies(mesh, u, h, rs, mlt, nonlinear=True, abs=True, ssh=ssh)
    g = tr.geometry(mesh)
    F = u * (h[g.c1] + h[g.c2]) / 2
    e, k = np.unravel_index(int(np.argmax((mesh.dcEdge * mesh.dvEdge)[:, None] * np.abs(F) * MU.astype(float))), u.shape)
    bad = tu.copy()
    bad[e, k] += 1e-9 * float(ref["U"][1][e, k])
    assert not _fails(tu, *ref["U"], tr.C_U) and _fails(bad, *ref["U"], tr.C_U)
    res, tol = tr.energy_budget(mesh, u, h, ssh, tu, th, MU, MH)
    assert abs(res) <= tol
    res, tol = tr.energy_budget(mesh, u, h, ssh, bad, th, MU, MH)
    assert abs(res) > tol


def test_sensitivity_laplacian_with_the_wrong_rotational_sign():
    """L built with +k x grad(zeta): the comparison with the twin's Del2 and the self-adjointness identity both reject it."""
    mesh = get_mesh("ico12f")
    K = 2
    u, h, rs = random_state(mesh, K, 80)
    mlt = np.full(mesh.nEdges, K, dtype=np.int32)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rs, max_level_edge_top=K)
    v2, _ = viscosities(mesh)
    tu = orc.OracleNonlinear(om, visc_del2=v2).tendencies(u, h)[0]
    good = tr.tendencies(mesh, u, h, rs, mlt, nonlinear=True, visc_del2=v2)[0]
    wrong = tr.tendencies(mesh, u, h, rs, mlt, nonlinear=True, visc_del2=v2, rot_sign=+1)[0]
    MU = tr.tendencies(mesh, u, h, rs, mlt, nonlinear=True, visc_del2=v2, abs=True)[0]
    assert not _fails(tu, good, MU, tr.C_U) and _fails(tu, wrong, MU, tr.C_U)
    g = tr.geometry(mesh)
    act = np.ones((mesh.nEdges, 1), dtype=bool)
    rng = np.random.default_rng(3)
    ul, vl = (rng.uniform(-1, 1, (mesh.nEdges, 1)).astype(tr.LD) for _ in range(2))
    wE = tr._col(g.dc * g.dv)
    rhs = -(tr._col(g.areaC) * tr.divergence(g, ul)[0] * tr.divergence(g, vl)[0]).sum() \
        - (tr._col(g.areaT) * tr.curl(g, ul)[0] * tr.curl(g, vl)[0]).sum()
    Lw, MLw = tr.laplacian(g, ul, np.abs(ul), act, rot_sign=+1)
    assert abs((wE * vl * Lw).sum() - rhs) > tr.C_U * tr.U53 * (wE * np.abs(vl) * MLw).sum()
