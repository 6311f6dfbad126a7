"""Reverse mode of passive tracer transport on the CPU: the numpy twin of the transposed tendency against a long-double transpose of the
forward one, the step-level identity <X, M d> = <M^T X, d>, the plane wave backwards, and the consequences include/moka_hip.h
states.  No GPU needed."""
import numpy as np
import pytest

import oracle as orc
import tracer_adjoint_twin as ta
import tracer_cases as tc
import trisk_reference as tr
from del4_twin import TwinState

LD = tr.LD


@pytest.mark.parametrize("partial", [False, True], ids=["full", "partial"])
@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("meshname", ["tiny-4-4", "tiny-2-4", "tiny-4-6"])
def test_transposed_tendency_against_the_long_double_transpose(meshname, K, partial):
    """|R - R_ld| <= C 2^-53 M per element, R_ld = T^T w from the matrix tracer_diffusion_twin.tendency_ld yields on unit vectors,
    w = y * areaCell in long double, M = (the same calls' magnitude matrix)^T |w|; C = C_R0 = 16 with kappa = 0 (the instances without
    diffusion) and C_R = 24 with kappa = 0.02 dc^2 / dt (tracer_adjoint_twin.py counts both).  Prints observed / bound."""
    mesh = tc.get_mesh(meshname)
    twin = tc.twin_of(meshname, K, "linear", partial)
    adj = ta.AdjointTwin(twin)
    _, u, h, _ = tc.state_of(meshname, K)
    y = np.random.default_rng(5 + K).uniform(-1.0, 1.0, (mesh.nCells, K))
    w = y.astype(LD) * np.asarray(mesh.areaCell, dtype=np.float64).astype(LD)[:, None]
    for kappa, C in ((0.0, ta.C_R0), (tc.kappas(meshname, 2)[0], ta.C_R)):
        assert (kappa == 0.0) == (C == ta.C_R0)
        r = adj.R(u, h, y, kappa, diff=kappa != 0.0)
        T, M = ta.forward_matrices_ld(mesh, u, h, twin.mlt, kappa)
        ref, mag = ta.transpose_apply(T, M, w)
        err = np.abs(r.astype(LD) - ref)
        worst = float((err / np.where(mag > 0, C * tr.U53 * mag, 1)).max())
        print(f"{meshname} K = {K} {'partial' if partial else 'full'} kappa = {kappa:g}: max |R - R_ld| / (C 2^-53 M) = {worst:.3f} (C = {C})")
        assert tr.within(r, ref, mag, C).all()
        assert np.any(r != 0.0)
        if kappa == 0.0:       # the diffusion instances with kappa == 0: the same bits
            assert np.array_equal(adj.R(u, h, y, 0.0, diff=True), r)


@pytest.mark.parametrize("meshname", ["planar", "ico16", "ico12f"])
@pytest.mark.parametrize("mode", ["linear", "nonlinear", "del2+del4"])
def test_step_identity_in_long_double(meshname, mode):
    """<X, M d> = <M^T X, d> per tracer over two recorded steps, partial masks, three tracers with tc.kappas (one exact zero): M d from
    TracerDiffusionTwin.step_rk4 run with the tracer d (M is linear: no differencing), M^T X from the reverse twin driven by that
    run's provisional states, both inner products in long double.  Bound: 2 steps * (100 + 96) * 2^-53 * sum |X| W, W the magnitude
    evaluation of the two forward steps on |d| (tracer_adjoint_twin.py derives the count).  Prints observed / bound."""
    K, nT, nsteps = 3, 3, 2
    mesh = tc.get_mesh(meshname)
    twin = ta.recording_twin(meshname, K, mode, partial=True)
    twin.kappa = tc.kappas(meshname, nT)
    ssh, u, h, _ = tc.state_of(meshname, K)
    st = TwinState(ssh, u, h)
    rng = np.random.default_rng(31)
    d = [rng.uniform(-1.0, 1.0, (mesh.nCells, K)) for _ in range(nT)]
    X = [rng.uniform(-1.0, 1.0, (mesh.nCells, K)) for _ in range(nT)]
    phis = [[a.copy() for a in d], [a.copy() for a in d]]
    for _ in range(nsteps):
        twin.step_rk4(st, phis, tc.dt_of(meshname))
    grad = ta.AdjointTwin(twin).sweep(twin.tape, [x.copy() for x in X])
    for j in range(nT):
        lhs, rhs = ta.dot_ld(X[j], phis[1][j]), ta.dot_ld(grad[j], d[j])
        W = np.abs(d[j]).astype(LD)
        for rec in twin.tape:
            W = ta.forward_magnitude(mesh, twin.mlt, rec, W, rec["kappa"][j])
        bound = nsteps * ta.C_STEP * tr.U53 * (np.abs(X[j]).astype(LD) * W).sum()
        print(f"{meshname} {mode} tracer {j} (kappa = {twin.kappa[j]:g}): |<X, M d> - <M^T X, d>| = {float(abs(lhs - rhs)):.3e}, "
              f"bound = {float(bound):.3e}, ratio = {float(abs(lhs - rhs) / bound):.4f}, <X, M d> = {float(lhs):.6e}")
        assert abs(lhs - rhs) <= bound
        assert abs(lhs) > 1e3 * bound          # the identity is not met by two zeros


@pytest.mark.parametrize("kappa", [0.0, tc.EIG_KAPPA], ids=["kappa0", "kappa"])
def test_plane_wave_backwards(kappa):
    """tc.eigenmode_state, seed X = phi0, EIG_STEPS recorded steps: the gradient is 1 + 0.5 Re(conj(R4(z))^n e^{i k . x}).  This pins
    the reverse stage weights without sharing code with the twin's derivation."""
    K = 4
    mesh, (ssh, u, h, rest), phi0 = tc.eigenmode_state(K)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=K)
    twin = ta.RecordingTwin(om, om, [kappa])
    st = TwinState(ssh, u, h)
    phis = [[phi0.copy()], [phi0.copy()]]
    for _ in range(tc.EIG_STEPS):
        twin.step_rk4(st, phis, tc.EIG_DT)
    grad = ta.AdjointTwin(twin).sweep(twin.tape, [phi0.copy()])[0]
    ta.plane_wave_check(grad, mesh, K, kappa, phi0, f"reverse twin, kappa = {kappa:g}")


def test_consequences_zero_seed_and_undiffused_neighbour():
    """A zero seed stays exactly zero; a tracer with kappa == 0 beside diffused ones has the bits of the sweep without diffusion."""
    meshname, K, nT = "ico12f", 3, 3
    mesh = tc.get_mesh(meshname)
    twin = ta.recording_twin(meshname, K, "nonlinear", partial=True)
    twin.kappa = tc.kappas(meshname, nT)
    assert twin.kappa[1] == 0.0 and twin.kappa[0] != 0.0
    ssh, u, h, _ = tc.state_of(meshname, K)
    st = TwinState(ssh, u, h)
    f = tc.distinct_fields(mesh, K, nT)
    phis = [[a.copy() for a in f], [a.copy() for a in f]]
    for _ in range(2):
        twin.step_rk4(st, phis, tc.dt_of(meshname))
    adj = ta.AdjointTwin(twin)
    x = np.random.default_rng(3).uniform(-1.0, 1.0, (mesh.nCells, K))
    zero = np.zeros_like(x)
    grad = adj.sweep(twin.tape, [x.copy(), x.copy(), zero.copy()])
    assert np.array_equal(grad[2], zero)
    plain = [dict(rec, kappa=[0.0] * nT) for rec in twin.tape]
    ref = adj.sweep(plain, [x.copy(), x.copy(), zero.copy()])
    assert np.array_equal(grad[1], ref[1])
    assert not np.array_equal(grad[0], ref[0])
    assert np.array_equal(ref[0], ref[1])
