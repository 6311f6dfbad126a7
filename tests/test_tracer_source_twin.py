"""Tracer sources and the gradient with respect to them on the CPU: the numpy twins of tests/tracer_source_twin.py against long-double
restatements, the bit identities include/moka_hip.h states, the rest state, the content budget, the forced plane wave forwards and
backwards, the step identity, and the interface text.  No GPU needed."""
import inspect
import os
import re

import numpy as np
import pytest

import oracle as orc
import tracer_adjoint_twin as ta
import tracer_cases as tc
import tracer_diffusion_twin as td
import tracer_source_twin as ts
import tracer_twin as tt
import trisk_reference as tr
from del4_twin import TwinState

LD = tr.LD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(twin, meshname, K, fields, nsteps=2):
    ssh, u, h, _ = tc.state_of(meshname, K)
    st = TwinState(ssh, u, h)
    phis = [[a.copy() for a in fields], [a.copy() for a in fields]]
    for _ in range(nsteps):
        twin.step_rk4(st, phis, tc.dt_of(meshname))
    return st, phis


@pytest.mark.parametrize("meshname", ["tiny-4-4", "planar", "ico12f"])
def test_twin_tendency_plus_source_within_bound_of_long_double(meshname):
    """One stage tendency with the source: |(T + q) - (T_ld + q)| <= C_TS 2^-53 (M + |q|) per element (tracer_source_twin.py counts
    C_TS = 27: the diffusive chain one addition deeper)."""
    K = 3
    mesh = tc.get_mesh(meshname)
    twin = ts.source_twin(meshname, K, "linear", True)
    _, u, h, _ = tc.state_of(meshname, K)
    phi, q, kappa = tc.distinct_fields(mesh, K, 1)[0], ts.source_fields(meshname, K, 1)[0], tc.kappas(meshname, 2)[0]
    ref, M = td.tendency_ld(mesh, u, h, phi, twin.mlt, kappa)
    got = twin.tendency(u, h, phi, kappa) + q
    assert tr.within(got, ref + q.astype(LD), M + np.abs(q).astype(LD), ts.C_TS).all()
    assert not tr.within(got, ref, M, ts.C_TS).all()          # the source is there


# ---- bit identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["linear", "nonlinear", "del2+del4"])
def test_forward_bit_identities(mode):
    """A zero source of either sign equals no source; an unsourced tracer beside sourced ones equals its run in a state without
    sources; the dycore never sees tracers or sources; the unit tracer without a source stays exactly 1.0; and the source-free
    SourceTwin is TracerDiffusionTwin bit for bit."""
    meshname, K, nT = "ico12f", 3, 3
    mesh = tc.get_mesh(meshname)
    f = tc.distinct_fields(mesh, K, nT, unit_first=True)
    q = ts.source_fields(meshname, K, nT)
    kap = tc.kappas(meshname, nT)
    base = tc.twin_of(meshname, K, mode, True)
    base.kappa = kap
    st0, plain = run(base, meshname, K, f)
    runs = {}
    for name, src in (("none", []), ("+0", [np.zeros_like(q[0])] * nT), ("-0", [-np.zeros_like(q[0])] * nT), ("some", [None, q[1], q[2]])):
        tw = ts.source_twin(meshname, K, mode, True)
        tw.kappa, tw.source = kap, src
        runs[name] = run(tw, meshname, K, f)
    assert np.signbit(-np.zeros_like(q[0])).all()
    for name in ("none", "+0", "-0"):
        for lvl in (0, 1):
            for j in range(nT):
                assert np.array_equal(runs[name][1][lvl][j], plain[lvl][j]), (name, lvl, j)
    st, some = runs["some"]
    assert np.array_equal(some[1][0], plain[1][0]) and np.array_equal(some[1][0], np.ones_like(f[0]))
    assert not np.array_equal(some[1][1], plain[1][1]) and not np.array_equal(some[1][2], plain[1][2])
    for a, b in ((st.u[1], st0.u[1]), (st.h[1], st0.h[1]), (st.ssh[1], st0.ssh[1])):
        assert np.array_equal(a, b)


def test_reverse_bit_identities():
    """G and X do not depend on q (two forward runs that differ only in their sources record the same tape); X has the bits of
    AdjointTwin's sweep with G on or off; a zero seed gives G == 0 exactly; G is nonzero for a nonzero seed."""
    meshname, K, nT = "ico12f", 3, 3
    mesh = tc.get_mesh(meshname)
    f, q, X = tc.distinct_fields(mesh, K, nT), ts.source_fields(meshname, K, nT), ta.seeds(mesh, K, nT)
    X[2] = np.zeros_like(X[2])
    out = []
    for src in ([q[0], None, q[2]], [None, 3.0 * q[1], None], []):
        tw = ts.source_twin(meshname, K, "nonlinear", True)
        tw.kappa, tw.source = tc.kappas(meshname, nT), src
        run(tw, meshname, K, f)
        adj = ts.SourceAdjointTwin(tw)
        g_on, G = adj.sweep(tw.tape, [x.copy() for x in X], (0, 2))
        g_off, G_off = adj.sweep(tw.tape, [x.copy() for x in X], ())
        g_parent = ta.AdjointTwin(tw).sweep(tw.tape, [x.copy() for x in X])
        assert G[1] is None and G_off == [None] * nT
        for j in range(nT):
            assert np.array_equal(g_on[j], g_off[j]) and np.array_equal(g_on[j], g_parent[j])
        assert np.array_equal(G[2], np.zeros_like(X[2])) and np.array_equal(g_on[2], np.zeros_like(X[2]))
        assert np.any(G[0] != 0.0)
        out.append((g_on, G))
    for g_on, G in out[1:]:
        for j in range(nT):
            assert np.array_equal(g_on[j], out[0][0][j])
        assert np.array_equal(G[0], out[0][1][0])


# ---- rest state -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kappa", [0.0, tc.EIG_KAPPA], ids=["kappa0", "kappa"])
def test_rest_state_fills_linearly(kappa):
    """planar-f0 at rest (u = 0, ssh = 0, h = 250 everywhere), phi_0 = 0, q uniform per level with its own value on every level: the
    dycore stays bitwise at rest, the slot sum is exactly +0.0 (F == 0, and the tracer is level-wise uniform, so the diffusive
    difference is 0 too) and phi_n = n dt q / h within n * C_REST * 2^-53 * |phi_n|, C_REST = 8 (tracer_source_twin.py: Qc 1, the four
    b[s] * q together 2, four additions, the quotient).  Prints observed / bound."""
    K, n = 5, 4
    mesh = tc.get_mesh("planar-f0")
    h = np.full((mesh.nCells, K), tc.EIG_H)
    u, ssh = np.zeros((mesh.nEdges, K)), np.zeros(mesh.nCells)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=h.sum(1), max_level_edge_top=K)
    qk = np.array([0.37, 1.9, 0.0113, 7.25, 0.61])
    q = np.repeat(qk[None, :], mesh.nCells, axis=0)
    twin = ts.SourceTwin(om, om, [kappa], [q])
    st = TwinState(ssh, u, h)
    zero = np.zeros_like(h)
    phis = [[zero.copy()], [zero.copy()]]
    for _ in range(n):
        twin.step_rk4(st, phis, tc.EIG_DT)
    assert np.array_equal(st.u[1], u) and np.array_equal(st.h[1], h) and np.array_equal(st.ssh[1], ssh)
    expect = LD(n) * LD(tc.EIG_DT) * q.astype(LD) / LD(tc.EIG_H)
    err = np.abs(phis[1][0].astype(LD) - expect)
    bound = n * ts.C_REST * tr.U53 * np.abs(expect)
    print(f"kappa = {kappa:g}: max |phi_n - n dt q / h| / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert len(set(phis[1][0][0])) == K and (phis[1][0] == phis[1][0][0]).all()       # level-wise uniform, every level its own


# ---- content budget ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("partial", [False, True], ids=["full", "partial"])
@pytest.mark.parametrize("meshname", ["planar", "ico12f"])
def test_content_changes_by_the_source_integral(meshname, partial):
    """sum_c A_c sum_k phi h changes per step by dt sum_c A_c sum_k q within tracer_source_twin.content_bound (the flux sum is
    boundary-free), over 3 steps of the nonlinear dycore with diffusion on; the source's share is far above the bound."""
    K = 5
    mesh = tc.get_mesh(meshname)
    twin = ts.source_twin(meshname, K, "nonlinear", partial)
    twin.kappa = [tc.kappas(meshname, 2)[0]]
    q = np.abs(ts.source_fields(meshname, K, 1)[0])
    twin.source = [q]
    ssh, u, h, _ = tc.state_of(meshname, K)
    st = TwinState(ssh, u, h)
    phi = tc.distinct_fields(mesh, K, 1)[0]
    phis = [[phi.copy()], [phi.copy()]]
    a = np.asarray(mesh.areaCell, dtype=np.float64).astype(LD)
    budget = LD(tc.dt_of(meshname)) * (a * q.astype(LD).sum(axis=1)).sum()
    for _ in range(3):
        s0 = tt.content(mesh, phis[1][0], st.h[1])
        twin.step_rk4(st, phis, tc.dt_of(meshname), magnitudes=True)
        s1 = tt.content(mesh, phis[1][0], st.h[1])
        bound = ts.content_bound(mesh, *twin.last_M[0])
        print(f"dS - dt sum A q = {float(s1 - s0 - budget):.3e}, bound = {float(bound):.3e}, dt sum A q = {float(budget):.3e}")
        assert abs(s1 - s0 - budget) <= bound
        assert budget > 1e6 * bound


# ---- the forced plane wave --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kappa", [0.0, tc.EIG_KAPPA], ids=["kappa0", "kappa"])
def test_forced_plane_wave_forwards_and_backwards(kappa):
    """tc.eigenmode_state with q = h sigma cos(k . x): the mode obeys phi^_{n+1} = R(z) phi^_n + dt psi(z) sigma, psi = 1 + z/2 + z^2/6 +
    z^3/24 -- the one check that the source enters every stage with the RK4 weights; backwards, the seed 1 + 0.5 cos(k . x) gives the
    conjugate response (ts.forced_wave_check / forced_wave_gradient_check; both bounds n * 32 * 2^-53 * max|.| and both refuse psi = 1
    and psi after z^2/6).  Measured on the CPU, kappa = 0 / EIG_KAPPA: forward deviation 2.3e-15 / 1.6e-15 against 5.3e-14, gaps
    to psi = 1 5.3e-2 / 5.1e-2 and to the truncated psi 5.6e-5 / 5.4e-5; backward deviation 6.9e-17 / 6.2e-17 against 4.2e-15 / 4.1e-15,
    gaps 2.1e-3 / 2.0e-3 and 2.2e-6 / 2.1e-6."""
    K = 4
    mesh, (ssh, u, h, rest), phi0 = tc.eigenmode_state(K)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=K)
    twin = ts.SourceTwin(om, om, [kappa], [ts.eigen_source(mesh, K)])
    st = TwinState(ssh, u, h)
    phis = [[phi0.copy()], [phi0.copy()]]
    for _ in range(tc.EIG_STEPS):
        twin.step_rk4(st, phis, tc.EIG_DT)
    assert np.array_equal(st.u[1], u) and np.array_equal(st.h[1], h)
    ts.forced_wave_check(phis[1][0], mesh, K, kappa, phi0, f"SourceTwin, kappa = {kappa:g}")
    _, G = ts.SourceAdjointTwin(twin).sweep(twin.tape, [phi0.copy()], (0,))
    ts.forced_wave_gradient_check(G[0], mesh, K, kappa, phi0, f"SourceAdjointTwin, kappa = {kappa:g}")


# ---- the step identity and the R-level check ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname", ["planar", "ico12f"])
@pytest.mark.parametrize("mode", ["linear", "nonlinear", "del2+del4"])
def test_step_identity_in_long_double(meshname, mode):
    """<X, phi_N(phi_0, q) - phi_N(phi_0, 0)> = <G, q> per tracer over two recorded steps, partial masks, tc.kappas (one exact zero):
    both forward runs from SourceTwin, G from SourceAdjointTwin over the first run's records, the difference and the inner products
    in long double.  Bound: 2 steps * C_STEP_SRC * 2^-53 * sum |X| W, C_STEP_SRC = 308 and W the magnitude evaluation of the forward
    steps on |phi_0| with |q| (tracer_source_twin.py).  Prints observed / bound."""
    K, nT, nsteps = 3, 3, 2
    mesh = tc.get_mesh(meshname)
    f, X = tc.distinct_fields(mesh, K, nT), ta.seeds(mesh, K, nT)
    q = [20.0 * a for a in ts.source_fields(meshname, K, nT)]           # a response of the order of phi itself
    ends = []
    for src in (q, []):
        twin = ts.source_twin(meshname, K, mode, True)
        twin.kappa, twin.source = tc.kappas(meshname, nT), src
        ends.append(run(twin, meshname, K, f, nsteps)[1][1])
        if src:
            tape, mlt = twin.tape, twin.mlt
            _, G = ts.SourceAdjointTwin(twin).sweep(tape, [x.copy() for x in X], range(nT))
    for j in range(nT):
        lhs = (X[j].astype(LD) * (ends[0][j].astype(LD) - ends[1][j].astype(LD))).sum()
        rhs = ta.dot_ld(G[j], q[j])
        W = np.abs(f[j]).astype(LD)
        for rec in tape:
            W = ts.forward_magnitude(mesh, mlt, rec, W, rec["kappa"][j], np.abs(q[j]))
        bound = nsteps * ts.C_STEP_SRC * tr.U53 * (np.abs(X[j]).astype(LD) * W).sum()
        print(f"{meshname} {mode} tracer {j}: |<X, dphi_N> - <G, q>| = {float(abs(lhs - rhs)):.3e}, bound = {float(bound):.3e}, "
              f"ratio = {float(abs(lhs - rhs) / bound):.4f}, <G, q> = {float(rhs):.6e}")
        assert abs(lhs - rhs) <= bound
        assert abs(rhs) > 1e3 * bound          # the identity is not met by two zeros


@pytest.mark.parametrize("meshname,K", [("tiny-4-4", 2), ("tiny-2-4", 3), ("tiny-4-6", 1)])
def test_forward_step_and_taus_against_long_double(meshname, K):
    """On the tiny meshes, over one recorded step with a partial mask and kappa != 0: the twin's phi_new equals ts.step_ld (tendency_ld
    plus q through the header's recipe) within 104 + 5 roundings on the forward magnitude, and the four increments of G equal tau_3 ..
    tau_0 of ts.taus_ld (the transposed long-double tendency) within C_TAU = 79 on their magnitudes.  Prints observed / bound."""
    mesh = tc.get_mesh(meshname)
    twin = ts.source_twin(meshname, K, "linear", True)
    kappa = tc.kappas(meshname, 2)[0]
    phi, q = tc.distinct_fields(mesh, K, 1)[0], 20.0 * ts.source_fields(meshname, K, 1)[0]
    twin.kappa, twin.source = [kappa], [q]
    _, phis = run(twin, meshname, K, [phi], 1)
    rec = twin.tape[0]
    ref = ts.step_ld(mesh, twin.mlt, rec, phi, kappa, q)
    W = ts.forward_magnitude(mesh, twin.mlt, rec, np.abs(phi).astype(LD), kappa, np.abs(q))
    assert tr.within(phis[1][0], ref, W, 104 + ts.SLACK).all()
    assert not tr.within(phis[1][0], ts.step_ld(mesh, twin.mlt, rec, phi, kappa, None), W, 104 + ts.SLACK).all()
    x = ta.seeds(mesh, K, 1)[0]
    taus, G = [], [np.zeros_like(x)]
    ts.SourceAdjointTwin(twin).reverse_step(rec, [x], True, G, taus)
    ref_t, mag_t = ts.taus_ld(mesh, twin.mlt, rec, x, kappa)
    acc = np.zeros_like(x)
    for s, (t, r, m) in enumerate(zip(taus[0], ref_t, mag_t)):
        worst = float((np.abs(t.astype(LD) - r) / np.where(m > 0, ts.C_TAU * tr.U53 * m, 1)).max())
        print(f"{meshname} K = {K} tau_{3 - s}: max |tau - tau_ld| / (C_TAU 2^-53 M) = {worst:.3f}")
        assert tr.within(t, r, m, ts.C_TAU).all() and np.any(t != 0.0)
        acc = acc + t
    assert np.array_equal(G[0], acc)                   # G is the running sum of the increments, in this order


# ---- interface text ---------------------------------------------------------------------------------------------------------------
def test_source_entry_points_exist():
    """The library exports the five entry points, the header declares them with the algebra beside them, the Python layer and the
    Julia shim wrap them."""
    import moka_hip as mk
    from moka_hip import lib as L
    lib = L.lib()
    names = ("moka_tracer_source_upload", "moka_tracer_source_download", "moka_tracer_has_source",
             "moka_tracer_adjoint_want_source_gradient", "moka_tracer_adjoint_source_download")
    hdr = open(os.path.join(ROOT, "include", "moka_hip.h")).read()
    jl = open(os.path.join(ROOT, "mpas-ocean.jl_amd", "julia", "MokaHIP.jl")).read()
    for name in names:
        assert hasattr(lib, name) and name in L.EXPORTS, name
        assert f"ccall((:{name}, lib)" in jl, name
    assert re.search(r"int\s+moka_tracer_source_upload\(moka_state \*st, int32_t j, const double \*host\);", hdr)
    assert re.search(r"int\s+moka_tracer_source_download\(moka_state \*st, int32_t j, double \*host\);", hdr)
    assert re.search(r"int\s+moka_tracer_has_source\(const moka_state \*st, int32_t j, int \*out\);", hdr)
    assert re.search(r"int\s+moka_tracer_adjoint_want_source_gradient\(moka_tracer_tape \*t, int32_t j, int on\);", hdr)
    assert re.search(r"int\s+moka_tracer_adjoint_source_download\(moka_tracer_tape \*t, int32_t j, double \*host\);", hdr)
    assert "T = T + q_j[k,c]" in hdr and "G = G + tau_3" in hdr and "<G, q>" in hdr
    for attr in ("set_source", "source", "has_source"):
        assert hasattr(mk.Tracers, attr), attr
    for attr in ("want_source_gradient", "source_gradient"):
        assert hasattr(mk.TracerAdjointTape, attr), attr
    assert inspect.signature(mk.set_tracers).parameters["sources"].default is None
    assert inspect.signature(mk.TracerAdjointTape.gradient).parameters["sources"].default is False
