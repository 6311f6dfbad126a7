"""Harmonic tracer diffusion: the numpy twin (tests/tracer_diffusion_twin.py) against its long-double restatement, the identities of
the scheme (kappa = 0 is the undiffused scheme bit for bit, a constant tracer stays constant, the content is conserved to round-off,
the term dissipates), an exact eigenmode that pins the meaning of kappa, and the entry points.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import oracle as orc
import tracer_diffusion_twin as td
import tracer_cases as tc
import tracer_twin as tt
import trisk_reference as tr
from del4_twin import TwinState
from moka_hip import meshgen as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = tr.LD
_MESHES = {}


def get_mesh(name):
    if name not in _MESHES:
        _MESHES[name] = {"planar": lambda: mg.planar_hex_mesh(20, 18, 1000.0),
                         "ico16": lambda: mg.icosahedral_mesh(16),
                         "ico12f": lambda: mg.icosahedral_mesh(12, flips=8, seed=4)}[name]()
    return _MESHES[name]


def dt_of(meshname):
    return 2.0 if meshname == "planar" else 20.0


def kappa_of(meshname, factor=0.02):
    return factor * float(get_mesh(meshname).dcEdge.min()) ** 2 / dt_of(meshname)


def random_state(mesh, K, seed):
    rng = np.random.default_rng(seed)
    rest = np.full((mesh.nCells, K), 1000.0 / K) + rng.uniform(0, 0.1, (mesh.nCells, K))
    h = rest + rng.uniform(-1, 1, (mesh.nCells, K))
    u = rng.uniform(-1, 1, (mesh.nEdges, K))
    return h.sum(1) - rest.sum(1), u, h, rest


def fields(mesh, K, n, seed=21):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.5, 1.5, (mesh.nCells, K)) for _ in range(n)]


def partial_mlt(mesh, K, seed=8):
    rng = np.random.default_rng(seed)
    mlt = np.where(rng.random(mesh.nEdges) < 0.33, rng.integers(0, K + 1, mesh.nEdges), K).astype(np.int32)
    mlt[:3] = 0
    return mlt


MESHNAMES = ["planar", "ico16", "ico12f"]


@pytest.mark.parametrize("partial", [False, True], ids=["full", "partial"])
@pytest.mark.parametrize("meshname", MESHNAMES)
def test_twin_tendency_within_bound_of_long_double(meshname, partial):
    """Per element |T - T_ld| <= C_TD 2^-53 M (C_TD = 26, tracer_diffusion_twin.py counts the chain), K = 5, with full and with partial
    edge masks, kappa = 0.02 dcEdge_min^2 / dt."""
    mesh, K = get_mesh(meshname), 5
    _, u, h, rest = random_state(mesh, K, 7 + K)
    mlt = partial_mlt(mesh, K) if partial else np.full(mesh.nEdges, K, dtype=np.int32)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=mlt)
    kappa = kappa_of(meshname)
    twin = td.TracerDiffusionTwin(om, om, [kappa])
    phi = fields(mesh, K, 1)[0]
    T = twin.tendency(u, h, phi, kappa)
    ref, M = td.tendency_ld(mesh, u, h, phi, mlt, kappa)
    ok = tr.within(T, ref, M, td.C_TD)
    err = np.abs(T.astype(LD) - ref) / (tr.U53 * np.where(M > 0, M, 1))
    print(f"max |T - T_ld| / (2^-53 M) = {float(err.max()):.2f} (C_TD = {td.C_TD})")
    assert ok.all(), int((~ok).sum())
    # the diffusive term is there: it moves T by far more than the bound
    assert not tr.within(twin.tendency(u, h, phi, 0.0), ref, M, td.C_TD).all()


def _run(twin, mesh, K, phis0, nsteps, dtv, seed=5, magnitudes=False):
    ssh, u, h, _ = random_state(mesh, K, seed)
    st = TwinState(ssh, u, h)
    phis = [[p.copy() for p in phis0], [p.copy() for p in phis0]]
    for _ in range(nsteps):
        twin.step_rk4(st, phis, dtv, magnitudes=magnitudes)
    return st, phis


def _om(mesh, K, seed=5, partial=False):
    _, _, _, rest = random_state(mesh, K, seed)
    return orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=partial_mlt(mesh, K) if partial else K)


@pytest.mark.parametrize("partial", [False, True], ids=["full", "partial"])
@pytest.mark.parametrize("meshname", ["ico16", "ico12f"])
def test_zero_kappa_is_the_undiffused_twin_bit_for_bit(meshname, partial):
    """kappa = 0 for every tracer: TracerTwin.step_rk4's tracers and dycore, both levels, bit for bit, after 3 steps."""
    mesh, K = get_mesh(meshname), 5
    om = _om(mesh, K, partial=partial)
    f = fields(mesh, K, 2)
    sa, pa = _run(tt.TracerTwin(om, om), mesh, K, f, 3, dt_of(meshname))
    sb, pb = _run(td.TracerDiffusionTwin(om, om, [0.0, 0.0]), mesh, K, f, 3, dt_of(meshname))
    for lev in (0, 1):
        for j in range(2):
            assert np.array_equal(pa[lev][j], pb[lev][j])
        assert np.array_equal(sa.u[lev], sb.u[lev]) and np.array_equal(sa.h[lev], sb.h[lev])


@pytest.mark.parametrize("meshname", ["ico16", "planar"])
def test_zero_kappa_tracer_beside_diffused_ones_is_undiffused(meshname):
    """kappa = (k, 0, k / 4): the middle tracer equals TracerTwin.step_rk4's bit for bit; the diffused ones differ from it."""
    mesh, K = get_mesh(meshname), 5
    om = _om(mesh, K, partial=True)
    f = fields(mesh, K, 3)
    k = kappa_of(meshname)
    _, pa = _run(tt.TracerTwin(om, om), mesh, K, f, 3, dt_of(meshname))
    _, pb = _run(td.TracerDiffusionTwin(om, om, [k, 0.0, k / 4]), mesh, K, f, 3, dt_of(meshname))
    for lev in (0, 1):
        assert np.array_equal(pa[lev][1], pb[lev][1])
    assert not np.array_equal(pa[1][0], pb[1][0]) and not np.array_equal(pa[1][2], pb[1][2])


@pytest.mark.parametrize("meshname", ["ico16", "ico12f"])
def test_unit_tracer_stays_exactly_one_with_diffusion(meshname):
    """phi == 1 with kappa > 0 is exactly 1.0 at both levels after 10 steps over a random flow; a random tracer beside it moves."""
    mesh, K = get_mesh(meshname), 5
    om = _om(mesh, K)
    k = kappa_of(meshname)
    other = fields(mesh, K, 1)[0]
    _, p = _run(td.TracerDiffusionTwin(om, orc.OracleNonlinear(om), [k, k]), mesh, K, [np.ones_like(other), other], 10, dt_of(meshname))
    one = np.ones_like(other)
    assert np.array_equal(p[1][0], one) and np.array_equal(p[0][0], one)
    assert not np.array_equal(p[1][1], other) and np.isfinite(p[1][1]).all()


@pytest.mark.parametrize("partial", [False, True], ids=["full", "partial"])
@pytest.mark.parametrize("meshname", MESHNAMES)
def test_content_is_conserved_to_the_extended_bound(meshname, partial):
    """sum_c A_c sum_k phi h in long double changes per step by no more than tracer_diffusion_twin.content_bound, over 3 steps of the
    nonlinear dycore with diffusion on."""
    mesh, K = get_mesh(meshname), 5
    dtv = dt_of(meshname)
    ssh, u, h, rest = random_state(mesh, K, 6)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=partial_mlt(mesh, K) if partial else K)
    twin = td.TracerDiffusionTwin(om, orc.OracleNonlinear(om), [kappa_of(meshname)])
    st = TwinState(ssh, u, h)
    phi = fields(mesh, K, 1)[0]
    phis = [[phi.copy()], [phi.copy()]]
    for _ in range(3):
        s0 = tt.content(mesh, phis[1][0], st.h[1])
        twin.step_rk4(st, phis, dtv, magnitudes=True)
        s1 = tt.content(mesh, phis[1][0], st.h[1])
        bound = td.content_bound(mesh, *twin.last_M[0])
        print(f"dS = {float(s1 - s0):.3e}, bound = {float(bound):.3e}")
        assert abs(s1 - s0) <= bound, (float(s1 - s0), float(bound))
        assert bound <= 1e-12 * abs(s0)
    assert np.abs(phis[1][0] - phi).max() > 1e-6


@pytest.mark.parametrize("partial", [False, True], ids=["full", "partial"])
@pytest.mark.parametrize("meshname", MESHNAMES)
def test_diffusion_dissipates_by_the_edge_sum(meshname, partial):
    """With pu = 0, sum_c A_c sum_k phi T of the twin equals -sum_{active e,k} kappa hE (dv / dc) (dphi)^2 (long double, <= 0 by
    construction) within 2^-53 C_TD sum_c A_c sum_k |phi| M."""
    mesh, K = get_mesh(meshname), 5
    _, u, h, rest = random_state(mesh, K, 9)
    mlt = partial_mlt(mesh, K) if partial else np.full(mesh.nEdges, K, dtype=np.int32)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=mlt)
    kappa = kappa_of(meshname)
    twin = td.TracerDiffusionTwin(om, om, [kappa])
    phi = fields(mesh, K, 1)[0]
    pu = np.zeros_like(u)
    T = twin.tendency(pu, h, phi, kappa)
    _, M = td.tendency_ld(mesh, pu, h, phi, mlt, kappa)
    a = np.asarray(mesh.areaCell, dtype=np.float64).astype(LD)
    got = (a * (phi.astype(LD) * T.astype(LD)).sum(axis=1)).sum()
    ref = td.dissipation_ld(mesh, h, phi, mlt, kappa)
    tol = tr.U53 * td.C_TD * (a * (np.abs(phi).astype(LD) * M).sum(axis=1)).sum()
    print(f"sum A phi T = {float(got):.6e}, edge sum = {float(ref):.6e}, |diff| = {float(abs(got - ref)):.3e}, tol = {float(tol):.3e}")
    assert ref < 0
    assert abs(got - ref) <= tol
    assert tol < 1e-10 * abs(ref)


def test_kappa_means_what_it_says_on_an_exact_eigenmode():
    """A plane wave is an eigenvector of the regular hexagon Laplacian.  At rest (u = 0, h = 250, linear dycore) 10 steps of
    phi0 = 1 + 0.5 cos(kx x + ky y) with kappa = 0.02 dc^2 / dt must give 1 + (phi0 - 1) R(z)^10, z = kappa lam dt,
    lam = 2 / (3 dc^2) sum_m (cos(k . d_m) - 1), R the RK4 stability polynomial, within 10 steps * 32 * 2^-53 * max|phi| (~5e-14: per
    step the path from Qc to phi_new rounds about 10 times, 32 leaves room for T's own error).  Measured on the CPU: 8.9e-16, with
    z = -0.010762 and R^10 = 0.89797.  The discrete-to-continuum gap is 3.4e-3, so a wrong scale or sign of kappa cannot pass."""
    mesh, K, dc, dtv, nsteps = get_mesh("planar"), 4, 1000.0, 2.0, 10
    assert np.allclose(mesh.dcEdge, dc, rtol=1e-12)
    h = np.full((mesh.nCells, K), 250.0)
    u = np.zeros((mesh.nEdges, K))
    ssh = np.zeros(mesh.nCells)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=h.sum(1), max_level_edge_top=K)
    kappa = 0.02 * 1000.0 ** 2 / 2
    kx, ky = 2 * np.pi * 2 / 20000.0, 2 * np.pi / (18 * 1000.0 * np.sqrt(3.0) / 2)
    phi0 = np.repeat((1 + 0.5 * np.cos(kx * np.asarray(mesh.xCell) + ky * np.asarray(mesh.yCell)))[:, None], K, axis=1)
    twin = td.TracerDiffusionTwin(om, om, [kappa])
    st = TwinState(ssh, u, h)
    phis = [[phi0.copy()], [phi0.copy()]]
    for _ in range(nsteps):
        twin.step_rk4(st, phis, dtv)
    assert np.array_equal(st.u[1], u) and np.array_equal(st.h[1], h)          # the dycore stayed at rest exactly
    lam = 2 / (3 * dc ** 2) * sum(np.cos(kx * dc * np.cos(m * np.pi / 3) + ky * dc * np.sin(m * np.pi / 3)) - 1 for m in range(6))
    z = kappa * lam * dtv
    R = 1 + z + z ** 2 / 2 + z ** 3 / 6 + z ** 4 / 24
    expect = 1 + (phi0 - 1) * R ** nsteps
    dev = float(np.abs(phis[1][0] - expect).max())
    tol = nsteps * 32 * 2.0 ** -53 * float(np.abs(phi0).max())
    lam_c = -(kx ** 2 + ky ** 2)
    print(f"z = {z:.6f}, R^10 = {R ** nsteps:.5f}, max deviation = {dev:.3e}, tolerance = {tol:.3e}, "
          f"discrete-to-continuum gap = {abs(np.exp(kappa * lam_c * dtv * nsteps) - R ** nsteps):.2e}")
    assert dev <= tol


def test_diffusion_entry_points_exist():
    """The library exports the two entry points, the header declares them with the algebra and the stability rule beside them, the
    Python layer and the Julia shim wrap them, and the documents no longer list tracer diffusion as missing."""
    import inspect

    import moka_hip as mk
    from moka_hip import lib as L
    lib = L.lib()
    for name in ("moka_set_tracer_diffusion", "moka_tracer_diffusion"):
        assert hasattr(lib, name), name
        assert name in L.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "moka_hip.h")).read()
    assert re.search(r"int\s+moka_set_tracer_diffusion\(moka_state \*st, const double \*kappa\);", hdr)
    assert re.search(r"int\s+moka_tracer_diffusion\(const moka_state \*st, int32_t j, double \*out\);", hdr)
    assert "dvdc[c,i] = dvEdge[e] / dcEdge[e]" in hdr and "0.35" in hdr
    jl = open(os.path.join(ROOT, "mpas-ocean.jl_amd", "julia", "MokaHIP.jl")).read()
    assert "ccall((:moka_set_tracer_diffusion, lib)" in jl and "ccall((:moka_tracer_diffusion, lib)" in jl
    assert re.search(r"function set_tracers!\([^)]*;\s*diffusivity", jl) and "function tracer_diffusivity(" in jl
    assert "diffusivity" in inspect.signature(mk.set_tracers).parameters
    assert inspect.signature(mk.set_tracers).parameters["diffusivity"].default is None
    assert hasattr(mk.Tracers, "set_diffusivity") and hasattr(mk.Tracers, "diffusivity")
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("include", "moka_hip.h")):
        assert ", tracer diffusion," not in open(os.path.join(ROOT, doc)).read(), doc


@pytest.mark.parametrize("nx,ny,K", tc.TINY)
def test_twin_tendency_on_tiny_periodic_meshes(nx, ny, K):
    """The smallest doubly periodic meshes, where a cell meets the same neighbour through several slots: per element
    |T - T_ld| <= C_TD 2^-53 M as on the large meshes, and a constant tracer's diffusive part vanishes exactly.  The GPU test on
    these meshes (test_gpu_tracer_shapes.py) rests on a twin known to handle them."""
    name = f"tiny-{nx}-{ny}"
    mesh = tc.get_mesh(name)
    _, u, h, rest = tc.state_of(name, K)
    mlt = np.full(mesh.nEdges, K, dtype=np.int32)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=mlt)
    kappa = tc.kappas(name, 3)[0]
    twin = td.TracerDiffusionTwin(om, om, [kappa])
    for phi in tc.distinct_fields(mesh, K, 2):
        ref, M = td.tendency_ld(mesh, u, h, phi, mlt, kappa)
        ok = tr.within(twin.tendency(u, h, phi, kappa), ref, M, td.C_TD)
        assert ok.all(), int((~ok).sum())
        assert not tr.within(twin.tendency(u, h, phi, 0.0), ref, M, td.C_TD).all()         # the diffusive term is there
    one = np.ones_like(h)
    assert np.array_equal(twin.tendency(u, h, one, kappa), om.tendencies_clean(u, h)[1])


def test_advection_and_diffusion_are_integrated_by_rk4_on_an_exact_eigenmode():
    """The plane wave of test_kappa_means_what_it_says_on_an_exact_eigenmode in a uniform flow U = (70, 40) (tracer_cases.py derives
    the mode): 10 steps must give 1 + 0.5 Re(R(z)^10 exp(i k . x)) with z = (mu + kappa lam) dt off both axes, within that test's
    10 * 32 * 2^-53 * max|phi0| = 5.3e-14.  Measured on the CPU: z = -0.010762 - 0.11201i, |R|^10 = 0.89797, deviation 1.1e-15; the
    same bound refuses a third-order stage loop by 3.0e-5 and the exact exponential by 6.8e-7; the dycore drift is exactly 0."""
    mesh, (ssh, u, h, rest), phi0 = tc.eigenmode_state(4)
    om = orc.OracleMesh(mesh, 4, resting_thickness_sum=rest.sum(1), max_level_edge_top=4)
    twin = td.TracerDiffusionTwin(om, om, [tc.EIG_KAPPA])
    st = TwinState(ssh, u, h)
    phis = [[phi0.copy()], [phi0.copy()]]
    for _ in range(tc.EIG_STEPS):
        twin.step_rk4(st, phis, tc.EIG_DT)
    assert np.array_equal(st.u[1], u) and np.array_equal(st.h[1], h)          # the uniform flow is steady, exactly
    tc.eigenmode_check(phis[1][0], mesh, 4, tc.EIG_KAPPA, phi0, "TracerDiffusionTwin, kappa = 0.02 dc^2 / dt")
