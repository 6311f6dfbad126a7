"""The numpy twin of the implicit vertical tracer diffusion (tests/tracer_vmix_twin.py) against its long-double restatement, the
properties include/moka_hip.h states, the plan's nLev, and an analytic vertical cosine mode.  No GPU.  The counted constants (C_BR, C_LV)
and their derivation are in the twin's docstring; every test prints the largest ratio to its bound."""
import numpy as np
import pytest

import oracle as orc
import tracer_biharmonic_twin as tb
import tracer_cases as tc
import tracer_kgrad_twin as tk
import tracer_vmix_twin as tv
from del4_twin import TwinState
from moka_hip import lib as L

LD = tv.LD
U = tv.U53
NCOL, K = 40, 60
DEPTHS = np.array([0, 1, 2, 2, 3, 3, 5, 17, 34, 59] + [60] * 30)
SH2 = (1e-9, 1e-3, 0.3, 2.0, 36.0, 1e3, 1e5)             # s / h^2


def columns(seed=3):
    """40 columns of K = 60 with mixed depths (0, 1 and 2 among them), thicknesses within a factor of four, values in [0.5, 1.5]."""
    rng = np.random.default_rng(seed)
    h = 10.0 * rng.uniform(0.5, 2.0, (NCOL, K))
    return h, rng.uniform(0.5, 1.5, (NCOL, K)), rng.uniform(-1.0, 1.0, (NCOL, K))


def groups():
    for n in np.unique(DEPTHS):
        if n >= 2:
            yield int(n), np.nonzero(DEPTHS == n)[0]


def solve_with_bounds(h, r, s, dense=None):
    """(z^, A, Ainv, res, fwd) of columns of one depth: the twin's solve of A z = r, and the two bounds' right-hand sides per element,
    res = |A||z^| + |r| and fwd = |A^-1| res, in long double.  dense: tv.dense_ld(h, s) when the caller has it already."""
    w = tv.weights(h, s)
    z = tv.solve(w, tv.diagonal(h, w), r)
    A, inv = dense if dense is not None else tv.dense_ld(h, s)
    res = tv.mv(np.abs(A), np.abs(z)) + np.abs(r).astype(LD)
    return z, A, inv, res, tv.mv(np.abs(inv), res)


@pytest.mark.parametrize("rhs", ["Lv(x)", "X"])
def test_backward_residual_and_forward_error(rhs):
    h, x, X = columns()
    worst_r = worst_f = 0.0
    for sh2 in SH2:
        s = sh2 * 100.0
        for n, idx in groups():
            hh = h[idx, :n]
            r = tv.Lv(tv.weights(hh, s), x[idx, :n]) if rhs == "Lv(x)" else X[idx, :n]
            z, A, inv, res, fwd = solve_with_bounds(hh, r, s)
            resid = np.abs(tv.mv(A, z) - r.astype(LD))
            err = np.abs(z.astype(LD) - tv.mv(inv, r))
            worst_r = max(worst_r, float((resid / (U * res)).max()))
            worst_f = max(worst_f, float((err / (U * fwd)).max()))
            assert np.all(resid <= tv.C_BR * U * res), (sh2, n)
            assert np.all(err <= tv.C_BR * U * fwd), (sh2, n)
    print(f"{rhs}: largest |A z - r| / (2^-53 (|A||z| + |r|)) = {worst_r:.2f}, largest forward error / (2^-53 |A^-1| (...)) = {worst_f:.2f}, "
          f"C_BR = {tv.C_BR}")


def test_unit_column_inactive_levels_and_shallow_columns():
    h, x, _ = columns()
    for sh2 in SH2:
        one = tv.apply(h, np.ones((NCOL, K)), DEPTHS, sh2 * 100.0)
        assert np.all(one == 1.0)
        for rev in (False, True):
            out = tv.apply(h, x, DEPTHS, sh2 * 100.0, reverse=rev)
            dead = np.arange(K)[None, :] >= DEPTHS[:, None]
            assert np.array_equal(out[dead], x[dead])
            assert np.array_equal(out[DEPTHS < 2], x[DEPTHS < 2])
            assert not np.array_equal(out[DEPTHS >= 2], x[DEPTHS >= 2])
    poisoned = np.where(np.arange(K)[None, :] >= DEPTHS[:, None], np.nan, x)
    out = tv.apply(h, poisoned, DEPTHS, 200.0)
    live = ~np.isnan(poisoned)
    assert np.array_equal(out[live], tv.apply(h, x, DEPTHS, 200.0)[live]) and np.all(np.isnan(out[~live]))


def test_content_and_maximum_principle():
    h, x, _ = columns()
    worst_c = worst_m = 0.0
    for sh2 in SH2:
        s = sh2 * 100.0
        for n, idx in groups():
            hh, xx = h[idx, :n], x[idx, :n]
            w = tv.weights(hh, s)
            r = tv.Lv(w, xx)
            z, A, inv, res, fwd = solve_with_bounds(hh, r, s)
            new = xx + z
            assert np.array_equal(new, tv.forward_cols(hh, xx, s))
            hl = hh.astype(LD)
            drift = np.abs((hl * new).sum(axis=1) - (hl * xx).sum(axis=1))
            bound = U * (tv.C_BR * res + tv.C_LV * tv.Lv_abs(w, xx) + hl * np.abs(new)).sum(axis=1)
            worst_c = max(worst_c, float((drift / bound).max()))
            assert np.all(drift <= bound), (sh2, n)
            # the range of the column, up to the forward error of z^ (and of r: A^-1 carries C_LV mLv) and the final addition
            slack = U * (tv.C_BR * fwd + tv.C_LV * tv.mv(np.abs(inv), tv.Lv_abs(w, xx)) + np.abs(new))
            lo, hi = xx.min(axis=1)[:, None], xx.max(axis=1)[:, None]
            over = np.maximum(new - hi, lo - new)
            worst_m = max(worst_m, float((over / slack).max()))
            assert np.all(over <= slack), (sh2, n)
    print(f"content drift / bound: {worst_c:.3f}; largest excursion beyond the column's range / slack: {worst_m:.3f}")


def test_transpose_identity():
    """<X, S phi> = <S^T X, phi> within the forward-error bounds of both sides."""
    h, x, X = columns()
    worst = 0.0
    for sh2 in SH2:
        s = sh2 * 100.0
        for n, idx in groups():
            hh, xx, XX = h[idx, :n], x[idx, :n], X[idx, :n]
            w = tv.weights(hh, s)
            dense = tv.dense_ld(hh, s)
            _, _, inv, _, fwd = solve_with_bounds(hh, tv.Lv(w, xx), s, dense)
            Sx = tv.forward_cols(hh, xx, s)
            errF = U * (tv.C_BR * fwd + tv.C_LV * tv.mv(np.abs(inv), tv.Lv_abs(w, xx)) + np.abs(Sx))
            zr, _, _, _, fwdr = solve_with_bounds(hh, XX, s, dense)
            StX = tv.reverse_cols(hh, XX, s)
            errR = U * (tv.C_BR * tv.Lv_abs(w, fwdr) + tv.C_LV * tv.Lv_abs(w, zr) + np.abs(StX))
            lhs, rhs = (XX.astype(LD) * Sx).sum(axis=1), (StX.astype(LD) * xx).sum(axis=1)
            bound = (np.abs(XX) * errF).sum(axis=1) + (errR * np.abs(xx)).sum(axis=1)
            worst = max(worst, float((np.abs(lhs - rhs) / bound).max()))
            assert np.all(np.abs(lhs - rhs) <= bound), (sh2, n)
            # ... and each side against long double
            hl = hh.astype(LD)
            assert np.all(np.abs(Sx - tv.mv(inv, hl * xx)) <= errF)              # S = A^-1 diag(h)
            assert np.all(np.abs(StX - hl * tv.mv(inv, XX)) <= errR)             # S^T = diag(h) A^-1
    print(f"|<X, S phi> - <S^T X, phi>| / bound: {worst:.3f}")


# ---- the whole step -----------------------------------------------------------------------------------------------------------------
def whole_step_case():
    meshname, Kc = "tiny-4-4", 8
    mesh = tc.get_mesh(meshname)
    mlt = tv.column_mlt(mesh, Kc)
    twin = tv.vmix_twin(meshname, Kc, mlt=mlt)
    ssh, u, h, _ = tc.state_of(meshname, Kc)
    st = TwinState(ssh, u, h)
    f = tc.distinct_fields(mesh, Kc, 3)
    phis = [[a.copy() for a in f], [a.copy() for a in f]]
    twin.kappa, twin.kappa4 = tc.kappas(meshname, 3), tb.kappa4s(meshname, 3)
    twin.kappaV = tv.kappavs(meshname, Kc, 3)
    twin.step_rk4(st, phis, tc.dt_of(meshname))
    return mesh, Kc, mlt, twin, f, phis


def step_of(twin, rec, j, phi):
    new = twin.replay(rec, j, phi)[1]
    kv = rec["kappaV"][j]
    return new if kv == 0.0 else tv.apply(rec["hn"], new, twin.nlev(phi.shape[1]), np.float64(rec["dt"]) * np.float64(kv))


def test_zero_coefficient_keeps_the_bits_of_the_plain_twin():
    mesh, Kc, mlt, twin, f, phis = whole_step_case()
    t = tc.twin_of("tiny-4-4", Kc, mlt=mlt)
    plain = tk.KgradTwin(t.om, t.base, [])
    ssh, u, h, _ = tc.state_of("tiny-4-4", Kc)
    st = TwinState(ssh, u, h)
    q = [[a.copy() for a in f], [a.copy() for a in f]]
    plain.kappa, plain.kappa4 = twin.kappa, twin.kappa4
    plain.step_rk4(st, q, tc.dt_of("tiny-4-4"))
    assert twin.kappaV[1] == 0.0 and np.array_equal(phis[1][1], q[1][1])
    assert not np.array_equal(phis[1][0], q[1][0]) and not np.array_equal(phis[1][2], q[1][2])
    X = [np.random.default_rng(5 + j).uniform(-1, 1, f[0].shape) for j in range(3)]
    a = tv.VmixAdjointTwin(twin).sweep(twin.tape, [x.copy() for x in X])[0]
    b = tk.KgradAdjointTwin(plain).sweep(plain.tape, [x.copy() for x in X])[0]
    assert np.array_equal(a[1], b[1]) and not np.array_equal(a[0], b[0])


def test_whole_reverse_step_against_differences_and_the_long_double_tangent():
    """The step is linear in phi: <X, (step(phi + d) - step(phi - d)) / 2> and <X, step_ld(d)> equal <reverse_step(X), d> within
    2^-53 sum |X| Wmax (C_STEP_B + 2 (C_BR + C_LV + 1) (1 + 8 s / hm^2)): tracer_biharmonic_twin's count of the RK4 step on its magnitude
    W, carried through S (row-stochastic: |S W| <= the column's largest W) with the solve's forward-error factor |A^-1||A| <= 1 + 8 s / hm^2
    in each direction; the difference quotient adds the cancellation of phi, 4 max|phi| / max|d| roundings."""
    mesh, Kc, mlt, twin, f, _ = whole_step_case()
    rec = twin.tape[0]
    adj = tv.VmixAdjointTwin(twin)
    rng = np.random.default_rng(9)
    nlev = twin.nlev(Kc)
    for j in range(3):
        X = rng.uniform(-1, 1, f[j].shape)
        d = rng.uniform(-1, 1, f[j].shape)
        Xs = [np.zeros_like(X) for _ in range(3)]
        Xs[j] = X
        back = adj.sweep([rec], Xs)[0][j]
        rhs = (back.astype(LD) * d).sum()
        cd = (step_of(twin, rec, j, f[j] + d).astype(LD) - step_of(twin, rec, j, f[j] - d)) / 2
        ld = tb.step_ld(mesh, mlt, rec, d, rec["kappa"][j], rec["kappa4"][j], None)
        s = np.float64(rec["dt"]) * np.float64(rec["kappaV"][j])
        if s != 0.0:
            for n in np.unique(nlev):
                if n >= 2:
                    idx = np.nonzero(nlev == n)[0]
                    A, inv = tv.dense_ld(rec["hn"][idx, :n], s)
                    ld[idx, :n] = tv.mv(inv, rec["hn"][idx, :n].astype(LD) * ld[idx, :n])
        W = tb.forward_magnitude(mesh, mlt, rec, np.abs(d), rec["kappa"][j], rec["kappa4"][j])
        Wmax = W.max(axis=1)[:, None]
        cond = 1 + 8 * float(s) / float(rec["hn"].min()) ** 2
        C = tb.C_STEP_B + 2 * (tv.C_BR + tv.C_LV + 1) * cond
        bound = U * C * (np.abs(X) * Wmax).sum()
        bound_cd = bound + U * 4 * 1.5 * (tb.C_STEP_B / 2 + (tv.C_BR + tv.C_LV + 1) * cond) * (np.abs(X) * (Wmax / np.abs(d).max())).sum()
        e_ld, e_cd = abs((X.astype(LD) * ld).sum() - rhs), abs((X.astype(LD) * cd).sum() - rhs)
        print(f"tracer {j} (kappaV = {rec['kappaV'][j]:.4g}): long double {float(e_ld):.3e} / {float(bound):.3e}, differences {float(e_cd):.3e} / {float(bound_cd):.3e}")
        assert e_ld <= bound and e_cd <= bound_cd


# ---- the plan's active depth ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ordering", [L.ORDER_NONE, L.ORDER_RCB])
@pytest.mark.parametrize("mask", ["partial_mlt", "floor", "full"])
def test_nlev_of_the_plan_is_the_maximum_over_the_slots(mask, ordering):
    mesh, Kc = tc.get_mesh("planar"), 7
    mlt = {"partial_mlt": tc.partial_mlt(mesh, Kc), "floor": tv.column_mlt(mesh, Kc), "full": np.full(mesh.nEdges, Kc, dtype=np.int32)}[mask]
    plan = L.Plan(mesh, Kc, resting_thickness_sum=np.full(mesh.nCells, 1000.0), max_level_edge_top=mlt, ordering=ordering, patch_cells=16)
    nlev = plan.array("nLev")
    perm = plan.permutation(L.CELL)
    eoc = np.asarray(mesh.edgesOnCell, dtype=np.int64) - 1
    expect = np.zeros(mesh.nCells, dtype=np.int64)
    for c in range(mesh.nCells):
        for i in range(int(mesh.nEdgesOnCell[c])):
            expect[c] = max(expect[c], min(int(mlt[eoc[c, i]]), Kc))
    assert nlev.dtype == np.int32 and np.array_equal(nlev, expect[perm])
    if mask == "floor":
        assert {0, 1, 2} <= set(nlev.tolist())
    # ... and what the twin derives from its slot masks
    assert np.array_equal(tv.vmix_twin("planar", Kc, mlt=mlt).nlev(Kc), expect)
    plan.close()


# ---- the vertical cosine mode ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 7])
def test_vertical_cosine_mode(m):
    """Uniform h, u = 0, n = K = 8: phi0 = 1 + 0.5 cos(pi m (k + 1/2) / n) is an eigenvector of the interface-flux matrix with eigenvalue
    (2 - 2 cos(pi m / n)) / h, so five steps with s / h^2 = 2 give 1 + 0.5 (1 / (1 + 2 (2 - 2 cos(pi m / n))))^5 cos(...).  Nothing in
    that expression shares code with the twin or the kernels.
    Tolerance, per step and element: the forward error C_BR 2^-53 |A^-1| (|A||z| + |r|) with row sums |A| <= h (1 + 4 s / h^2) = 9 h,
    |A^-1| = 1 / h (A^-1 diag(h) is row-stochastic), |z| <= 1 and |r| <= 2 (s / h) = 4 h: 13 C_BR; Lv's own roundings through A^-1:
    C_LV * 4; the final addition 1.5; the RK4 step around it (u = 0: Qc = phi h and Qn / h, two roundings of values <= 1.5): 3.
    tol = 5 (13 C_BR + 12 + 1.5 + 3) 2^-53."""
    n, hval, dtv, nsteps = 8, 8.0, 2.0, 5
    mesh = tc.get_mesh("tiny-4-4")
    om = orc.OracleMesh(mesh, n, resting_thickness_sum=np.full(mesh.nCells, n * hval), max_level_edge_top=n)
    twin = tv.VmixTwin(om, om, [0.0], [2.0 * hval * hval / dtv])
    h = np.full((mesh.nCells, n), hval)
    st = TwinState(np.zeros(mesh.nCells), np.zeros((mesh.nEdges, n)), h)
    mode = np.cos(np.pi * m * (np.arange(n) + 0.5) / n)
    phi0 = np.repeat((1 + 0.5 * mode)[None, :], mesh.nCells, axis=0)
    phis = [[phi0.copy()], [phi0.copy()]]
    for _ in range(nsteps):
        twin.step_rk4(st, phis, dtv)
        assert np.array_equal(st.h[1], h) and np.all(st.u[1] == 0.0)         # the flow stays at rest
    lam = 2 - 2 * np.cos(np.pi * m / n)
    expect = lambda f: 1 + 0.5 * f ** nsteps * mode                          # noqa: E731
    tol = nsteps * (13 * tv.C_BR + 4 * tv.C_LV + 1.5 + 3) * U
    dev = float(np.abs(phis[1][0] - expect(1 / (1 + 2 * lam))[None, :]).max())
    gap_cn = float(np.abs(phis[1][0] - expect((1 - lam) / (1 + lam))[None, :]).max())
    gap_ex = float(np.abs(phis[1][0] - expect(1 - 2 * lam)[None, :]).max())
    print(f"m = {m}: deviation {dev:.3e}, tolerance {tol:.3e}, gap to Crank-Nicolson {gap_cn:.3e}, to the explicit factor {gap_ex:.3e}")
    assert dev <= tol
    assert gap_cn > tol and gap_ex > tol
