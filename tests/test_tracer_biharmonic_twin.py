"""Biharmonic tracer diffusion: the numpy twins (tests/tracer_biharmonic_twin.py) against their long-double restatements, pass by pass;
the identities of the scheme (kappa4 = 0 is the scheme without the term bit for bit, a constant tracer stays constant, content is
conserved, variance decays by -kappa4 sum A h L^2); the plane wave forwards and backwards, which pins the meaning and the sign of kappa4;
the adjoint and the source-gradient identities; and the entry points.  No GPU needed."""
import inspect
import os
import re

import numpy as np
import pytest

import oracle as orc
import tracer_adjoint_twin as ta
import tracer_biharmonic_twin as tb
import tracer_cases as tc
import tracer_diffusion_twin as td
import tracer_source_twin as ts
import tracer_twin as tt
import trisk_reference as tr
from del4_twin import TwinState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = tr.LD


@pytest.fixture(autouse=True, scope="module")
def _the_entry_point_the_twins_specify():
    """The twins of this file are the specification of moka_set_tracer_biharmonic: without that entry point they specify nothing."""
    from moka_hip import lib as L
    assert hasattr(L.lib(), "moka_set_tracer_biharmonic") and "moka_set_tracer_biharmonic" in L.EXPORTS
MESHNAMES = ["planar", "ico16", "ico12f"]


def _case(meshname, K, partial, seed=7):
    mesh = tc.get_mesh(meshname)
    _, u, h, rest = tc.random_state(mesh, K, seed + K)
    mlt = tc.partial_mlt(mesh, K) if partial else np.full(mesh.nEdges, K, dtype=np.int32)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=mlt)
    return mesh, u, h, mlt, om


def _k(meshname, j=0):
    return tc.kappas(meshname, 9)[j], tb.kappa4s(meshname, 9)[j]


def _check_two_passes(mesh, om, u, h, mlt, kappa, kappa4, phi):
    twin = tb.TracerBiharmonicTwin(om, om, [kappa], kappa4=[kappa4])
    # pass 1: lap against lap_ld
    Ld = twin.lap(h, phi)
    Lr, ML = tb.lap_ld(mesh, h, phi, mlt)
    ok = tr.within(Ld, Lr, ML, tb.C_LAP)
    e1 = float((np.abs(Ld.astype(LD) - Lr) / (tr.U53 * np.where(ML > 0, ML, 1))).max())
    assert ok.all(), int((~ok).sum())
    # pass 2: the tendency against tendency_ld with the long-double L; the double L's error enters the magnitude
    T = twin.tendency_bih(u, h, phi, kappa, kappa4, Ld)
    ref, M = tb.tendency_ld(mesh, u, h, phi, mlt, kappa, kappa4, Lr, np.abs(Lr))
    Mp = tb.bih_magnitude(mesh, h, ML, mlt, kappa4)
    bound = tr.U53 * (tb.C_TB * M + tb.C_LAP * Mp)
    err = np.abs(T.astype(LD) - ref)
    e2 = float((err / np.where(bound > 0, bound, 1)).max())
    print(f"max |L - L_ld| / (2^-53 ML) = {e1:.2f} (C_LAP = {tb.C_LAP}); max |T - T_ld| / bound = {e2:.3f}")
    assert (err <= bound).all(), int((err > bound).sum())
    # the term is there: without it T falls outside the bound
    T0 = td.TracerDiffusionTwin(om, om, [kappa]).tendency(u, h, phi, kappa)
    assert not (np.abs(T0.astype(LD) - ref) <= bound).all()
    return twin


@pytest.mark.parametrize("partial", [False, True], ids=["full", "partial"])
@pytest.mark.parametrize("meshname", MESHNAMES)
def test_twin_passes_within_bound_of_long_double(meshname, partial):
    """Per element and per pass, K = 5: |Lap - Lap_ld| <= C_LAP 2^-53 ML and |T - T_ld(L_ld)| <= 2^-53 (C_TB M + C_LAP Mp), with
    kappa = 0.02 dc^2 / dt and kappa4 = 0.002 dc^4 / dt; the tendency without the term falls outside."""
    mesh, u, h, mlt, om = _case(meshname, 5, partial)
    kappa, kappa4 = _k(meshname)
    _check_two_passes(mesh, om, u, h, mlt, kappa, kappa4, tc.distinct_fields(mesh, 5, 1)[0])


@pytest.mark.parametrize("nx,ny,K", tc.TINY)
def test_twin_passes_on_tiny_periodic_meshes(nx, ny, K):
    """The smallest doubly periodic meshes (a cell meets the same neighbour through several slots): the same per-element bounds, and a
    constant tracer has L == 0 and the thickness tendency exactly."""
    name = f"tiny-{nx}-{ny}"
    mesh = tc.get_mesh(name)
    _, u, h, rest = tc.state_of(name, K)
    mlt = np.full(mesh.nEdges, K, dtype=np.int32)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=mlt)
    kappa, kappa4 = _k(name)
    twin = _check_two_passes(mesh, om, u, h, mlt, kappa, kappa4, tc.distinct_fields(mesh, K, 1)[0])
    one = np.ones_like(h)
    L1 = twin.lap(h, one)
    assert np.array_equal(L1, np.zeros_like(h))
    assert np.array_equal(twin.tendency_bih(u, h, one, kappa, kappa4, L1), om.tendencies_clean(u, h)[1])


def _run(twin, meshname, K, phis0, nsteps, seed=5, magnitudes=False):
    mesh = tc.get_mesh(meshname)
    ssh, u, h, _ = tc.random_state(mesh, K, seed)
    st = TwinState(ssh, u, h)
    phis = [[p.copy() for p in phis0], [p.copy() for p in phis0]]
    for _ in range(nsteps):
        twin.step_rk4(st, phis, tc.dt_of(meshname), magnitudes=magnitudes)
    return st, phis


def _om(meshname, K, seed=5, partial=False):
    mesh = tc.get_mesh(meshname)
    _, _, _, rest = tc.random_state(mesh, K, seed)
    return orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=tc.partial_mlt(mesh, K) if partial else K)


@pytest.mark.parametrize("partial", [False, True], ids=["full", "partial"])
@pytest.mark.parametrize("meshname", ["ico16", "ico12f"])
def test_zero_kappa4_is_the_diffusion_twin_bit_for_bit(meshname, partial):
    """kappa4 = 0 for every tracer: TracerDiffusionTwin's tracers and dycore after 3 steps, bit for bit -- through the parents' code
    (every kappa4 zero) and through the third addition with kappa4 = 0 (tendency_bih directly)."""
    mesh, K = tc.get_mesh(meshname), 5
    om = _om(meshname, K, partial=partial)
    f = tc.distinct_fields(mesh, K, 2)
    kap = tc.kappas(meshname, 2)
    sa, pa = _run(td.TracerDiffusionTwin(om, om, kap), meshname, K, f, 3)
    twin = tb.TracerBiharmonicTwin(om, om, kap, kappa4=[0.0, 0.0])
    sb, pb = _run(twin, meshname, K, f, 3)
    for lev in (0, 1):
        for j in range(2):
            assert np.array_equal(pa[lev][j], pb[lev][j])
        assert np.array_equal(sa.u[lev], sb.u[lev]) and np.array_equal(sa.h[lev], sb.h[lev])
    _, u, h, _ = tc.random_state(mesh, K, 5)
    for j in range(2):
        assert np.array_equal(twin.tendency_bih(u, h, f[j], kap[j], 0.0, twin.lap(h, f[j])), twin.tendency(u, h, f[j], kap[j]))


@pytest.mark.parametrize("meshname", ["ico16", "planar"])
def test_zero_kappa4_tracer_beside_others_is_without_the_term(meshname):
    """kappa4 = (k4, 0, k4 / 4) over kappa = (k, 0, k'): the middle tracer equals TracerDiffusionTwin's bit for bit (its third addition
    adds +-0.0); the others differ from it."""
    mesh, K = tc.get_mesh(meshname), 5
    om = _om(meshname, K, partial=True)
    f = tc.distinct_fields(mesh, K, 3)
    kap = tc.kappas(meshname, 3)
    k4 = tb.kappa4s(meshname, 1)[0]
    _, pa = _run(td.TracerDiffusionTwin(om, om, kap), meshname, K, f, 3)
    _, pb = _run(tb.TracerBiharmonicTwin(om, om, kap, kappa4=[k4, 0.0, k4 / 4]), meshname, K, f, 3)
    for lev in (0, 1):
        assert np.array_equal(pa[lev][1], pb[lev][1])
    assert not np.array_equal(pa[1][0], pb[1][0]) and not np.array_equal(pa[1][2], pb[1][2])


@pytest.mark.parametrize("kappa_on", [True, False], ids=["kappa", "kappa-free"])
@pytest.mark.parametrize("meshname", ["ico16", "ico12f"])
def test_unit_tracer_stays_exactly_one(meshname, kappa_on):
    """phi == 1 with kappa4 > 0 (with and without kappa) is exactly 1.0 at both levels after 10 steps of the nonlinear dycore; a random
    tracer beside it moves and stays finite."""
    mesh, K = tc.get_mesh(meshname), 5
    om = _om(meshname, K)
    k, k4 = _k(meshname)
    other = tc.distinct_fields(mesh, K, 1)[0]
    one = np.ones_like(other)
    twin = tb.TracerBiharmonicTwin(om, orc.OracleNonlinear(om), [k if kappa_on else 0.0] * 2, kappa4=[k4, k4])
    _, p = _run(twin, meshname, K, [one, other], 10)
    assert np.array_equal(p[1][0], one) and np.array_equal(p[0][0], one)
    assert not np.array_equal(p[1][1], other) and np.isfinite(p[1][1]).all()


@pytest.mark.parametrize("partial", [False, True], ids=["full", "partial"])
@pytest.mark.parametrize("meshname", MESHNAMES)
def test_content_is_conserved_to_the_derived_bound(meshname, partial):
    """sum_c A_c sum_k phi h in long double changes per step by no more than tracer_biharmonic_twin.content_bound, over 3 steps of the
    nonlinear dycore with both terms on."""
    mesh, K = tc.get_mesh(meshname), 5
    ssh, u, h, rest = tc.random_state(mesh, K, 6)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=tc.partial_mlt(mesh, K) if partial else K)
    k, k4 = _k(meshname)
    twin = tb.TracerBiharmonicTwin(om, orc.OracleNonlinear(om), [k], kappa4=[k4])
    st = TwinState(ssh, u, h)
    phi = tc.distinct_fields(mesh, K, 1)[0]
    phis = [[phi.copy()], [phi.copy()]]
    for _ in range(3):
        s0 = tt.content(mesh, phis[1][0], st.h[1])
        twin.step_rk4(st, phis, tc.dt_of(meshname), magnitudes=True)
        s1 = tt.content(mesh, phis[1][0], st.h[1])
        bound = tb.content_bound(mesh, *twin.last_M[0])
        print(f"dS = {float(s1 - s0):.3e}, bound = {float(bound):.3e}")
        assert abs(s1 - s0) <= bound, (float(s1 - s0), float(bound))
        assert bound <= 1e-11 * abs(s0)
    assert np.abs(phis[1][0] - phi).max() > 1e-6


@pytest.mark.parametrize("partial", [False, True], ids=["full", "partial"])
@pytest.mark.parametrize("meshname", MESHNAMES)
def test_variance_decays_by_kappa4_times_the_weighted_square_of_L(meshname, partial):
    """With pu = 0 and kappa = 0: sum_c A_c sum_k phi T4 = -kappa4 sum_c A_c sum_k h L^2.  In long double the identity holds to the
    reference's own round-off (both sides from lap_ld / tendency_ld), and is <= 0; the twin's T meets it within its per-element bound
    summed with the weights A |phi|."""
    mesh, u, h, mlt, om = _case(meshname, 5, partial, seed=9)
    _, k4 = _k(meshname)
    phi = tc.distinct_fields(mesh, 5, 1)[0]
    pu = np.zeros_like(u)
    Lr, ML = tb.lap_ld(mesh, h, phi, mlt)
    Tr, M = tb.tendency_ld(mesh, pu, h, phi, mlt, 0.0, k4, Lr, np.abs(Lr))
    a = np.asarray(mesh.areaCell, dtype=np.float64).astype(LD)
    ref = tb.dissipation_ld(mesh, h, Lr, k4)
    wsum = lambda x: (a * (np.abs(phi).astype(LD) * x).sum(axis=1)).sum()                     # noqa: E731
    got_ld = (a * (phi.astype(LD) * Tr).sum(axis=1)).sum()
    Mfull = tb.tendency_ld(mesh, pu, h, phi, mlt, 0.0, k4, Lr, ML)[1]
    tol_ld = LD(2.0) ** -60 * wsum(Mfull)         # the long-double sums' own round-off (2^-64 per operation, tens of operations deep)
    twin = tb.TracerBiharmonicTwin(om, om, [0.0], kappa4=[k4])
    T = twin.tendency_bih(pu, h, phi, 0.0, k4, twin.lap(h, phi))
    got = (a * (phi.astype(LD) * T.astype(LD)).sum(axis=1)).sum()
    tol = tr.U53 * (tb.C_TB * wsum(M) + tb.C_LAP * wsum(tb.bih_magnitude(mesh, h, ML, mlt, k4)))
    print(f"-kappa4 sum A h L^2 = {float(ref):.6e}; long double: |diff| = {float(abs(got_ld - ref)):.3e} (rel {float(abs(got_ld - ref) / abs(ref)):.1e}), "
          f"tol = {float(tol_ld):.3e}; twin: |diff| = {float(abs(got - ref)):.3e}, tol = {float(tol):.3e}")
    assert ref < 0
    assert abs(got_ld - ref) <= tol_ld
    assert abs(got - ref) <= tol + tol_ld
    assert tol < 1e-7 * abs(ref)


def _eig_twin(kappa, kappa4, K=4):
    mesh, (ssh, u, h, rest), phi0 = tc.eigenmode_state(K)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=K)
    twin = tb.TracerBiharmonicTwin(om, om, [kappa], kappa4=[kappa4])
    return mesh, twin, TwinState(ssh, u, h), u, h, phi0


def test_plane_wave_forwards():
    """tracer_cases.eigenmode_state(4) with kappa = EIG_KAPPA and kappa4 = 0.002 dc^4 / dt: 10 steps follow R(z)^10 with
    z = (mu + kappa lam - kappa4 lam^2) dt within 10 * 32 * 2^-53 * max|phi0| = 5.3e-14; the same tolerance refuses kappa4 = 0, the wrong
    sign and a third-order stage loop (tracer_biharmonic_twin.plane_wave_check prints every figure)."""
    mesh, twin, st, u, h, phi0 = _eig_twin(tc.EIG_KAPPA, tb.EIG_KAPPA4)
    phis = [[phi0.copy()], [phi0.copy()]]
    for _ in range(tc.EIG_STEPS):
        twin.step_rk4(st, phis, tc.EIG_DT)
    assert np.array_equal(st.u[1], u) and np.array_equal(st.h[1], h)          # the uniform flow is steady, exactly
    tb.plane_wave_check(phis[1][0], mesh, 4, tc.EIG_KAPPA, tb.EIG_KAPPA4, phi0, "TracerBiharmonicTwin forwards")


def test_plane_wave_backwards():
    """The reverse sweep over the same 10 recorded steps multiplies the mode by conj(R(z))^10: same tolerance, same refusals, and the
    forward factor is refused too."""
    mesh, twin, st, u, h, phi0 = _eig_twin(tc.EIG_KAPPA, tb.EIG_KAPPA4)
    phis = [[phi0.copy()], [phi0.copy()]]
    for _ in range(tc.EIG_STEPS):
        twin.step_rk4(st, phis, tc.EIG_DT)
    # seed X = phi0, as tests/test_tracer_adjoint_twin.py does: A and h are uniform here, so the transposed step keeps the mode
    grad, _ = tb.BiharmonicAdjointTwin(twin).sweep(twin.tape, [phi0.copy()])
    tb.plane_wave_check(grad[0], mesh, 4, tc.EIG_KAPPA, tb.EIG_KAPPA4, phi0, "BiharmonicAdjointTwin backwards", backwards=True)


def _small_run(mode, nT, nsteps, srcs=(), K=3, meshname="ico12f", partial=True):
    """nsteps recorded steps of the first nT distinct fields on `meshname` (small, heptagons, a partial mask) over the dycore `mode`."""
    mesh = tc.get_mesh(meshname)
    t = tc.twin_of(meshname, K, mode, partial)
    twin = tb.TracerBiharmonicTwin(t.om, t.base, tc.kappas(meshname, 9)[:nT], kappa4=tb.kappa4s(meshname, 9)[:nT])
    q = ts.source_fields(meshname, K, 9)
    twin.source = [q[j] if j in srcs else None for j in range(nT)]
    ssh, u, h, _ = tc.state_of(meshname, K)
    st = TwinState(ssh, u, h)
    f = tc.distinct_fields(mesh, K, 9)[:nT]
    phis = [[a.copy() for a in f], [a.copy() for a in f]]
    for _ in range(nsteps):
        twin.step_rk4(st, phis, tc.dt_of(meshname))
    return mesh, twin, f, phis


@pytest.mark.parametrize("mode", ["linear", "nonlinear", "del2+del4"])
def test_adjoint_identity_in_long_double(mode):
    """<X, M d> = <M^T X, d> over 2 recorded steps: M d from step_ld on the twin's recorded states (long double), M^T X from the adjoint
    twin's sweep, within 2 * C_STEP_B * 2^-53 * sum |X| W (the docstring's count), for the tracers with both terms, the biharmonic one
    alone and the harmonic one alone."""
    nT, nsteps, K = 3, 2, 3
    mesh, twin, f, _ = _small_run(mode, nT, nsteps)
    X = ta.seeds(mesh, K, nT)
    grad, _ = tb.BiharmonicAdjointTwin(twin).sweep(twin.tape, [x.copy() for x in X])
    rng = np.random.default_rng(3)
    for j in range(nT):
        d = rng.uniform(-1.0, 1.0, f[j].shape)
        kap, kap4 = twin.tape[0]["kappa"][j], twin.tape[0]["kappa4"][j]
        p, w = d.astype(LD), np.abs(d).astype(LD)
        for rec in twin.tape:
            p = tb.step_ld(mesh, twin.mlt, rec, p, kap, kap4, None)
            w = tb.forward_magnitude(mesh, twin.mlt, rec, w, kap, kap4)
        lhs, rhs = ta.dot_ld(X[j], p), ta.dot_ld(grad[j], d)
        bound = nsteps * tb.C_STEP_B * tr.U53 * (np.abs(X[j]).astype(LD) * w).sum()
        print(f"{mode}, tracer {j}: <X, M d> = {float(lhs):.12e}, |diff| = {float(abs(lhs - rhs)):.3e}, bound = {float(bound):.3e}")
        assert abs(lhs - rhs) <= bound
        assert bound < 1e-9 * abs(lhs) or abs(lhs) < 1e-3
    # the M term is there: the sweep without it (the recorded kappa4 zeroed) misses the identity of tracer 0
    tape0 = [dict(rec, kappa4=[0.0] * nT) for rec in twin.tape]
    g0, _ = tb.BiharmonicAdjointTwin(twin).sweep(tape0, [x.copy() for x in X])
    assert not np.array_equal(g0[0], grad[0]) and np.array_equal(g0[2], grad[2])


def test_source_gradient_identity_with_biharmonic_diffusion():
    """<X, phi_N(q) - phi_N(0)> = <G, q> with kappa4 != 0: both runs from step_ld on the recorded states, G from the adjoint twin's sweep,
    within 2 * C_STEP_BSRC * 2^-53 * sum |X| W."""
    nT, nsteps, K = 2, 2, 3
    mesh, twin, f, _ = _small_run("nonlinear", nT, nsteps, srcs=(0, 1))
    X = ta.seeds(mesh, K, nT)
    _, G = tb.BiharmonicAdjointTwin(twin).sweep(twin.tape, [x.copy() for x in X], want=(0, 1))
    for j in range(nT):
        q = twin.source[j]
        kap, kap4 = twin.tape[0]["kappa"][j], twin.tape[0]["kappa4"][j]
        assert kap4 != 0.0
        pq, p0, w = f[j].astype(LD), f[j].astype(LD), np.abs(f[j]).astype(LD)
        for rec in twin.tape:
            pq = tb.step_ld(mesh, twin.mlt, rec, pq, kap, kap4, q)
            p0 = tb.step_ld(mesh, twin.mlt, rec, p0, kap, kap4, None)
            w = tb.forward_magnitude(mesh, twin.mlt, rec, w, kap, kap4, np.abs(q))
        lhs, rhs = ta.dot_ld(X[j], pq - p0), ta.dot_ld(G[j], q)
        bound = nsteps * tb.C_STEP_BSRC * tr.U53 * (np.abs(X[j]).astype(LD) * w).sum()
        print(f"tracer {j}: <X, dphi> = {float(lhs):.12e}, <G, q> = {float(rhs):.12e}, |diff| = {float(abs(lhs - rhs)):.3e}, bound = {float(bound):.3e}")
        assert abs(lhs - rhs) <= bound
        assert abs(lhs) > 1e3 * bound


def test_biharmonic_entry_points_exist():
    """The library exports the two entry points, the header declares them with the algebra and the stability rule beside them, the Python
    layer and the Julia shim wrap them, and the documents no longer list biharmonic tracer diffusion as missing."""
    import moka_hip as mk
    from moka_hip import lib as L
    lib = L.lib()
    for name in ("moka_set_tracer_biharmonic", "moka_tracer_biharmonic"):
        assert hasattr(lib, name), name
        assert name in L.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "moka_hip.h")).read()
    assert re.search(r"int\s+moka_set_tracer_biharmonic\(moka_state \*st, const double \*kappa4\);", hdr)
    assert re.search(r"int\s+moka_tracer_biharmonic\(const moka_state \*st, int32_t j, double \*out\);", hdr)
    assert "s += (hE * (x[k,c'] - x[k,c])) * dvdc[c,i]" in hdr and "0.043" in hdr
    assert "T = T - ((((kappa4_j * hE) * (L_j[k,c'] - L_j[k,c])) * dvdc[c,i]) * (1/areaCell[c]))" in hdr
    assert "r = r - ((kappa4_j * hE) * dvdc[c,i]) * (M_j[k,c'] - M_j[k,c])" in hdr
    jl = open(os.path.join(ROOT, "mpas-ocean.jl_amd", "julia", "MokaHIP.jl")).read()
    assert "ccall((:moka_set_tracer_biharmonic, lib)" in jl and "ccall((:moka_tracer_biharmonic, lib)" in jl
    assert re.search(r"function set_tracers!\([^)]*;\s*diffusivity = nothing,\s*biharmonic = nothing\)", jl)
    assert "function tracer_biharmonic(" in jl
    sig = inspect.signature(mk.set_tracers).parameters
    assert list(sig)[-3:] == ["diffusivity", "sources", "biharmonic"] and sig["biharmonic"].default is None
    assert hasattr(mk.Tracers, "set_biharmonic") and hasattr(mk.Tracers, "biharmonic")
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("include", "moka_hip.h")):
        text = open(os.path.join(ROOT, doc)).read()
        assert "moka_set_tracer_biharmonic" in text, doc
        for line in text.split("\n"):
            if re.search(r"out of scope", line, re.I) and "tracer" in line.lower():
                assert "biharmonic" not in line.lower(), (doc, line)
