"""Del4 (biharmonic) momentum mixing: the numpy twin (tests/del4_twin.py) against the oracle, the operator's algebra, and the
C ABI / Julia shim entry points.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import oracle as orc
from del4_twin import Del4Twin, TwinState
from moka_hip import meshgen as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 9.80616


def _setup(mesh, K, seed=5):
    rng = np.random.default_rng(seed)
    rest = np.full((mesh.nCells, K), 400.0)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=K)
    u = rng.uniform(-1, 1, (mesh.nEdges, K))
    h = rest + rng.uniform(-1, 1, rest.shape)
    return om, u, h, h.sum(1) - rest.sum(1)


@pytest.mark.parametrize("visc_del2", [0.0, 1.0])
def test_twin_without_del4_is_the_oracle_bit_for_bit(visc_del2):
    """viscDel4 = 0: the twin's tendencies and three RK4 steps equal OracleNonlinear's (with and without Del2), bit for bit --
    the restated stage loop is oracle_step_rk4_nonlinear_del2's."""
    mesh = mg.icosahedral_mesh(8)
    K = 4
    om, u, h, ssh = _setup(mesh, K, seed=3)
    dt = 0.2 * float(mesh.dcEdge.min()) / np.sqrt(G * 1600.0)
    v2 = visc_del2 * 0.01 * float(mesh.dcEdge.min()) ** 2 / dt
    nl = orc.OracleNonlinear(om, visc_del2=v2) if v2 else orc.OracleNonlinear(om)
    tw = Del4Twin(om, visc_del2=v2, visc_del4=0.0)
    tu, th, s = tw.tendencies(u, h)
    ou, oh, os_, _ = nl.tendencies(u, h)
    assert np.array_equal(tu, ou) and np.array_equal(th, oh) and np.array_equal(s, os_)
    a, b = orc.OracleState(om, ssh, u, h), TwinState(ssh, u, h)
    for _ in range(3):
        nl.step_rk4(a, dt)
        tw.step_rk4(b, dt)
    for lev in (0, 1):
        assert np.array_equal(b.u[lev], a.u[lev]) and np.array_equal(b.h[lev], a.h[lev]) and np.array_equal(b.ssh[lev], a.ssh[lev])
    assert np.array_equal(b.tendU, a.tendU) and np.array_equal(b.tendH, a.tendH)


def test_del4_term_is_the_last_operation():
    """With Del4 on, the tendency is the Del2 tendency minus L(L(u)) * coef4 on the active levels, and nothing else changes."""
    mesh = mg.planar_hex_mesh(10, 8, 1000.0)
    K = 3
    om, u, h, _ = _setup(mesh, K, seed=4)
    tw0, tw = Del4Twin(om, visc_del2=2.0), Del4Twin(om, visc_del2=2.0, visc_del4=5.0)
    t0, t = tw0.tendencies(u, h), tw.tendencies(u, h)
    assert np.array_equal(t[1], t0[1]) and np.array_equal(t[2], t0[2])
    assert np.array_equal(t[0], t0[0] - tw.del4_bracket(u) * 5.0)
    assert not np.array_equal(t[0], t0[0])
    ones = Del4Twin(om, visc_del4=5.0, scaling=np.ones(mesh.nEdges))
    assert np.array_equal(ones.tendencies(u, h)[0], Del4Twin(om, visc_del4=5.0).tendencies(u, h)[0])


@pytest.mark.parametrize("n", [1, 2, 5])
def test_eigenmode_scale_selectivity(n):
    """On a doubly periodic hex mesh phi = cos(2 pi n x / Lx) is a discrete eigenfunction of div(grad): with u = grad(phi),
    L(u) = lambda u and L(L(u)) = lambda^2 u -- Del4 damps at lambda^2 where Del2 damps at lambda."""
    nx, ny, dc = 20, 18, 1000.0
    mesh = mg.planar_hex_mesh(nx, ny, dc)
    om = orc.OracleMesh(mesh, 1, max_level_edge_top=1)
    tw = Del4Twin(om, visc_del4=1.0)
    c1, c2 = mesh.cellsOnEdge[:, 0] - 1, mesh.cellsOnEdge[:, 1] - 1
    phi = np.cos(2 * np.pi * n * mesh.xCell / (nx * dc))[:, None]
    u = (phi[c2] - phi[c1]) / mesh.dcEdge[:, None]
    div = om.divergence_on_cell(u)
    lam = float(np.sum(div * phi) / np.sum(phi * phi))
    assert lam < 0
    assert np.abs(div - lam * phi).max() <= 1e-12 * np.abs(lam * phi).max()
    Lu = tw.L(u)
    assert np.abs(Lu - lam * u).max() <= 1e-10 * np.abs(lam * u).max()
    T = tw.del4_bracket(u)
    assert np.abs(T - lam ** 2 * u).max() <= 1e-10 * np.abs(lam ** 2 * u).max()
    # the divergence-free counterpart: a skew gradient of a vertex streamfunction has no divergence
    v1, v2 = mesh.verticesOnEdge[:, 0] - 1, mesh.verticesOnEdge[:, 1] - 1
    psi = np.cos(2 * np.pi * n * mesh.xVertex / (nx * dc))[:, None]
    w = (psi[v2] - psi[v1]) / mesh.dvEdge[:, None]
    assert np.abs(w).max() > 0
    assert np.abs(om.divergence_on_cell(w)).max() <= 1e-12 * np.abs(w).max() / dc


@pytest.mark.parametrize("mesh", [mg.icosahedral_mesh(8), mg.planar_hex_mesh(10, 8, 1000.0)], ids=["ico8", "planar"])
def test_del4_dissipates_kinetic_energy(mesh):
    """L is symmetric in the dcEdge * dvEdge inner product (the discrete integration by parts behind the Del2 test, twice):
    sum dc dv u L(L(u)) = sum dc dv L(u)^2 > 0, and the term enters the tendency with a minus sign."""
    om, u, h, _ = _setup(mesh, 1, seed=9)
    tw = Del4Twin(om, visc_del4=1.0)
    w = (mesh.dcEdge * mesh.dvEdge)[:, None]
    d2 = tw.L(u)
    lhs = float(np.sum(w * u * tw.del4_bracket(u)))
    rhs = float(np.sum(w * d2 * d2))
    assert rhs > 0 and abs(lhs - rhs) <= 1e-9 * rhs, (lhs, rhs)
    base = Del4Twin(om).tendencies(u, h)[0]
    assert float(np.sum(w * u * (tw.tendencies(u, h)[0] - base))) < 0


def test_del4_entry_points_exist():
    """The library exports the Del4 entry points, the header declares them and the Julia shim calls the setter."""
    from moka_hip import lib as L
    lib = L.lib()
    for name in ("moka_set_viscosity_del4", "moka_state_del4_path"):
        assert hasattr(lib, name), name
        assert name in L.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "moka_hip.h")).read()
    assert re.search(r"int\s+moka_set_viscosity_del4\(moka_state \*st, double viscDel4, const double \*meshScalingDel4\);", hdr)
    jl = open(os.path.join(ROOT, "mpas-ocean.jl_amd", "julia", "MokaHIP.jl")).read()
    assert "function set_viscosity_del4!(" in jl and "ccall((:moka_set_viscosity_del4, lib)" in jl
