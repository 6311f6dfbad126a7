"""The numpy twin of moka_forced_tape (tests/forced_adjoint_twin.py) against a long-double model, against differences of the forward
twin, and against the identities the header states.  No GPU; tests/test_gpu_forced_adjoint.py holds the device to this twin bit for bit.

Differences.  J = sum ssh^2 after three forced steps, the forward in doubles (the oracle's RK4 step and momentum_vmix_twin's pass), so
a difference quotient carries 2 eps_J / delta of forward round-off with
    eps_J = NSTEPS * C_STEP * 2^-53 * sum_c 2 |ssh_c| sum_k |h[k,c]|,   C_STEP = tracer_biharmonic_twin.C_STEP_B,
the count of a (longer) RK4 step of these twins on the magnitude of what it updates; ssh is a difference of column sums of h.  The
discrepancy of a central difference must fall by 3 .. 5 per halving of delta (one-sided: 1.5 .. 2.5) unless it is already below that
floor, and the decay must be seen at least once: the pattern of test_tracer_vgrad_twin.py."""
import numpy as np
import pytest

import forced_adjoint_twin as fa
import momentum_vmix_twin as mv
import oracle as orc
import poison_cases as pc
import tracer_biharmonic_twin as tb
import tracer_cases as tc

LD = fa.LD
NSTEPS = 3
_WORST = {"ratio": 0.0}


def make(meshname, K, nu, drag, tau, want=0, mlt=None, partial=False, state=None):
    om = tc.oracle_mesh(meshname, K, partial, mlt)
    ssh, u, h, _ = state if state is not None else tc.state_of(meshname, K)
    tw = fa.ForcedTwin(om, ssh, u, h, want)
    tw.nu, tw.drag, tw.tau = nu, drag, tau
    return tw


def settings(meshname, K, stress=True):
    nu, r = mv.coefficients(meshname, K)
    return nu, r, (mv.stress_field(tc.get_mesh(meshname), K) if stress else None)


# ---- exact transpose, column by column, against long double -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 6, 34])
@pytest.mark.parametrize("what", ["nu", "drag", "stress", "nu+drag+stress", "none"])
def test_exact_transpose_against_long_double(n, what):
    """<X, J_ld delta> against <(XU', hbar, G_tau, D_nu, D_r), delta> for random X and random directions in (u*, h_e, tau, nu, r), 64
    columns a case.  "none": nu = r = 0 and no stress, the derivative at zero."""
    rng = np.random.default_rng(1000 + 7 * n + len(what))
    ncol, hm, dt = 64, 1000.0 / 34, 2.0
    parts = what.split("+")
    nu = 4.0 * hm * hm / dt if "nu" in parts else 0.0
    r = 0.5 * hm / dt if "drag" in parts else 0.0
    tau = rng.uniform(-1, 1, ncol) * hm / 2 if "stress" in parts else None
    h = hm * rng.uniform(0.5, 1.5, (ncol, n))
    x, X = rng.uniform(-1, 1, (ncol, n)), rng.uniform(-1, 1, (ncol, n))
    d = (rng.uniform(-1, 1, (ncol, n)), hm * rng.uniform(-1, 1, (ncol, n)), rng.uniform(-1, 1, ncol) * hm, nu_scale(hm, dt) * rng.uniform(-1, 1),
         hm / dt * rng.uniform(-1, 1))
    T_ld, ld = fa.pairing_ld(h, x, X, dt, nu, r, tau, d)
    T_tw, tw = fa.pairing_twin(h, x, X, dt, nu, r, tau, d)
    bound = fa.pairing_bound(h, x, X, dt, nu, r, tau, d, ld, tw)
    err = np.abs(T_tw - T_ld)
    ratio = float((err / bound).max())
    _WORST["ratio"] = max(_WORST["ratio"], ratio)
    print(f"n = {n} {what}: largest error / bound = {ratio:.3f} (largest so far {_WORST['ratio']:.3f}); pairing magnitude {float(np.abs(T_ld).max()):.3e}")
    assert np.all(np.abs(T_ld) > 0) and np.all(err <= bound)


def nu_scale(hm, dt):
    return hm * hm / dt


# ---- differences of the forward twin ------------------------------------------------------------------------------------------------
def J_of(meshname, K, nu, drag, tau, u0=None, h0=None):
    ssh, u, h, _ = tc.state_of(meshname, K)
    u = u if u0 is None else u0
    h = h if h0 is None else h0
    tw = make(meshname, K, nu, drag, tau, state=(ssh, u, h, None))       # (the RK4 step recomputes ssh from h in every tendency)
    for _ in range(NSTEPS):
        tw.step(tc.dt_of(meshname))
    s = tw.st.ssh[1].astype(LD)
    return (s * s).sum(), tw


def eps_J(tw):
    return NSTEPS * tb.C_STEP_B * fa.U53 * (2 * np.abs(tw.st.ssh[1]).astype(LD) * np.abs(tw.st.h[1]).astype(LD).sum(axis=1)).sum()


def decay(J, grad, d0, order, eJ, label):
    J0 = J(0.0) if order == 1 else None
    disc = []
    for i in range(3):
        d = d0 / 2 ** i
        fd = (J(d) - J0) / LD(d) if order == 1 else (J(d) - J(-d)) / (2 * LD(d))
        disc.append((abs(fd - LD(grad)), 2 * eJ / LD(d)))
    ratios = [float(disc[i][0] / disc[i + 1][0]) for i in range(2)]
    lo, hi = (3.0, 5.0) if order == 2 else (1.5, 2.5)
    print(f"{label}: gradient {float(grad):.6e}, discrepancies {[f'{float(x[0]):.3e}' for x in disc]}, ratios {[f'{r:.3f}' for r in ratios]}, "
          f"floors {[f'{float(x[1]):.3e}' for x in disc]}")
    for i in range(2):
        assert lo <= ratios[i] <= hi or disc[i + 1][0] <= disc[i + 1][1]
    assert lo <= ratios[0] <= hi
    assert disc[2][0] < 0.05 * abs(grad)


def swept(meshname, K, nu, drag, tau):
    Jv, tw = J_of(meshname, K, nu, drag, tau)
    eJ = eps_J(tw)
    tw2 = make(meshname, K, nu, drag, tau, want=7)
    for _ in range(NSTEPS):
        tw2.step(tc.dt_of(meshname))
    XU, XH = tw2.sweep(*tw2.seed_sum_sq_ssh())
    return XU, XH, tw2.gradients(), eJ


@pytest.mark.parametrize("meshname,K", [("tiny-4-4", 5), ("planar", 6)])
def test_central_differences(meshname, K):
    nu, r, tau = settings(meshname, K)
    XU, XH, g, eJ = swept(meshname, K, nu, r, tau)
    ssh, u, h, _ = tc.state_of(meshname, K)
    e, c, k = 7, 5, K // 2

    def Ju(d):
        v = u.copy(); v[e, k] += d
        return J_of(meshname, K, nu, r, tau, u0=v)[0]

    def Jh(d):
        v = h.copy(); v[c, k] += d
        return J_of(meshname, K, nu, r, tau, h0=v)[0]

    def Jt(d):
        v = tau.copy(); v[e] += d
        return J_of(meshname, K, nu, r, v)[0]

    hm = 1000.0 / K
    decay(Ju, XU[e, k], 0.5, 2, eJ, f"{meshname} u0[{e},{k}]")
    decay(Jh, XH[c, k], 0.25, 2, eJ, f"{meshname} h0[{c},{k}]")
    decay(Jt, g["surfaceStress"][e], hm / 4, 2, eJ, f"{meshname} tau[{e}]")
    decay(lambda d: J_of(meshname, K, nu + d, r, tau)[0], g["viscosity"], nu / 8, 2, eJ, f"{meshname} nu")
    decay(lambda d: J_of(meshname, K, nu, r + d, tau)[0], g["bottomDrag"], r / 8, 2, eJ, f"{meshname} r")


@pytest.mark.parametrize("meshname,K", [("tiny-4-4", 5)])
def test_one_sided_difference_at_zero(meshname, K):
    """nu = r = 0 and no stress: every step ran without the pass, the flagged sweep solves A = diag(h) for the densities alone."""
    nu, r, _ = settings(meshname, K)
    XU, XH, g, eJ = swept(meshname, K, 0.0, 0.0, None)
    plain = make(meshname, K, 0.0, 0.0, None)
    for _ in range(NSTEPS):
        plain.step(tc.dt_of(meshname))
    PU, PH = plain.sweep(*plain.seed_sum_sq_ssh())
    assert np.array_equal(PU, XU) and np.array_equal(PH, XH)            # the flags change no bit of X
    assert g["viscosity"] != 0.0 and g["bottomDrag"] != 0.0 and np.any(g["surfaceStress"] != 0.0)
    decay(lambda d: J_of(meshname, K, d, 0.0, None)[0], g["viscosity"], nu / 4096, 1, eJ, "nu at zero")
    decay(lambda d: J_of(meshname, K, 0.0, d, None)[0], g["bottomDrag"], r / 4096, 1, eJ, "r at zero")
    zero = np.zeros(tc.get_mesh(meshname).nEdges)

    def Jt(d):
        v = zero.copy(); v[7] = d
        return J_of(meshname, K, 0.0, 0.0, v)[0]
    decay(Jt, g["surfaceStress"][7], (1000.0 / K) / 64, 2, eJ, "tau at zero")


# ---- identities ---------------------------------------------------------------------------------------------------------------------
def test_pass_off_is_the_oracle_sweep_bit_for_bit():
    meshname, K = "planar", 6
    tw = make(meshname, K, 0.0, 0.0, None)
    ssh, u, h, _ = tc.state_of(meshname, K)
    st = orc.OracleState(tw.om, ssh, u, h)
    rk = orc.OracleAdjointRK4(st)
    for _ in range(NSTEPS):
        tw.step(tc.dt_of(meshname))
        rk.step_rk4(tc.dt_of(meshname))
    XU, XH = tw.sweep(*tw.seed_sum_sq_ssh())
    RU, RH = rk.gradient_sum_sq_ssh()
    assert np.array_equal(XU, RU) and np.array_equal(XH, RH)


def test_identity_with_nothing_switched_on():
    """nu = r = 0, no stress, columns taken as computed: z = XU / h, XU' = h z = XU to round-off and hbar == -z * 0 / h == -0.0 or 0.0."""
    rng = np.random.default_rng(3)
    h, X, un = rng.uniform(10, 20, (32, 6)), rng.uniform(-1, 1, (32, 6)), rng.uniform(-1, 1, (32, 6))
    z, xnew, hbar, nusum = fa.adjoint_cols(h, X, un, 0.0)
    assert np.all(np.abs(xnew - X) <= 2 * fa.U53 * np.abs(X)) and np.all(hbar == 0.0)
    mesh = tc.get_mesh("tiny-4-4")
    XU, XH = rng.uniform(-1, 1, (mesh.nEdges, 6)), rng.uniform(-1, 1, (mesh.nCells, 6))
    un, hn = rng.uniform(-1, 1, XU.shape), rng.uniform(10, 20, XH.shape)
    oU, oH = fa.transposed_pass(mesh, np.full(mesh.nEdges, 6), XU, XH, un, hn, 2.0, 0.0, 0.0, None)
    assert np.array_equal(oU, XU) and np.array_equal(oH, XH)             # the pass is off: X keeps its bits


def test_fixed_point_profile_leaves_the_P_terms():
    """u[n-1] = tau / r, u[k] - u[k+1] = tau hm[k] / nu: R(un) is zero to round-off, so hbar reduces to 0.5 (P[k-1] + P[k])."""
    rng = np.random.default_rng(4)
    n, dt, nu, r = 8, 2.0, 300.0, 5.0
    h = rng.uniform(10, 20, (16, n))
    tau = rng.uniform(1, 2, 16)
    hm = 0.5 * (h[:, :-1] + h[:, 1:])
    un = np.empty_like(h)
    un[:, -1] = tau / r
    for k in range(n - 2, -1, -1):
        un[:, k] = un[:, k + 1] + tau * hm[:, k] / nu
    X = rng.uniform(-1, 1, h.shape)
    s, q, b = dt * nu, dt * r, dt * tau
    z, xnew, hbar, _ = fa.adjoint_cols(h, X, un, s, q, b)
    Rn = mv.rhs_cols(h, un, s, q, b)[2]
    assert np.all(np.abs(Rn) <= 16 * fa.U53 * mv.rhs_abs(h, un, s, q, b).astype(float))
    P = (s / hm / hm) * ((z[:, :-1] - z[:, 1:]) * (un[:, :-1] - un[:, 1:]))
    Pm = np.zeros_like(h)
    Pm[:, :-1] += 0.5 * P
    Pm[:, 1:] += 0.5 * P
    assert np.all(np.abs(hbar - Pm) <= np.abs(z * Rn / h) + 4 * fa.U53 * np.abs(Pm)) and np.any(Pm != 0)


# ---- masks and poison ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["partial", "basin"])
def test_n1_columns_partial_masks_and_nan_below_every_level(mask):
    meshname, K = "planar", 6
    mesh = tc.get_mesh(meshname)
    mlt = pc.mask_of(meshname, K) if mask == "basin" else tc.partial_mlt(mesh, K)
    assert (mlt == 0).any() and (mlt == 1).any() and (mlt == K).any()
    nu, r, tau = settings(meshname, K)
    rng = np.random.default_rng(5)
    XU, XH = rng.uniform(-1, 1, (mesh.nEdges, K)), rng.uniform(-1, 1, (mesh.nCells, K))
    un, hn = rng.uniform(-1, 1, XU.shape), (1000.0 / K) * rng.uniform(0.5, 1.5, XH.shape)
    below = np.arange(K)[None, :] >= np.minimum(mlt, K)[:, None]
    clean = fa.transposed_pass(mesh, mlt, XU, XH, un, hn, 2.0, nu, r, tau, {b: np.zeros(mesh.nEdges) for b in (1, 2, 4)})
    dens = {b: np.zeros(mesh.nEdges) for b in (1, 2, 4)}
    pU, pun = XU.copy(), un.copy()
    pU[below], pun[below] = np.nan, np.nan
    oU, oH = fa.transposed_pass(mesh, mlt, pU, XH, pun, hn, 2.0, nu, r, tau, dens)
    assert np.all(np.isnan(oU[below])) and np.array_equal(oU[~below], clean[0][~below])
    assert np.all(np.isfinite(oH)) and np.array_equal(oH, clean[1])
    assert all(np.all(np.isfinite(d)) for d in dens.values())
    assert np.all(dens[1][mlt == 0] == 0.0) and np.all(dens[1][mlt >= 1] != 0.0)
    # nu alone: the n == 1 columns are not computed -- XU keeps its bits there -- yet their z reaches the densities of a flagged sweep
    dens = {b: np.zeros(mesh.nEdges) for b in (1, 2, 4)}
    oU, oH = fa.transposed_pass(mesh, mlt, XU, XH, un, hn, 2.0, nu, 0.0, None, dens)
    one = mlt == 1
    assert np.array_equal(oU[one], XU[one]) and np.all(dens[1][one] != 0.0) and np.all(dens[2][one] == 0.0)
    plain = fa.transposed_pass(mesh, mlt, XU, XH, un, hn, 2.0, nu, 0.0, None)
    assert np.array_equal(plain[0], oU) and np.array_equal(plain[1], oH)
