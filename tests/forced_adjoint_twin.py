"""Numpy twin of the transposed vertical momentum pass and of the densities of moka_forced_tape (include/moka_hip.h states the
recipe; csrc/momentum_vmix.hip: mvadj_column, k_mvadj_gather), composed with oracle.OracleAdjointRK4's per-step transposition into the
whole sweep, and a long-double restatement on momentum_vmix_twin.dense_ld.

Recipe, per edge column of depth n computed by the forward pass, h[k] = 0.5 * (hn[k,c1] + hn[k,c2]), un the recorded u_new, s = dt nuV,
q = dt r, b = dt tau[e], every operation rounded once in this order:
    z     = Solve_A(XU)                             momentum_vmix_twin's w, d and tracer_vmix_twin.solve with XU as the right-hand side
    hm[k] = 0.5 * (h[k] + h[k+1]);  w[k] = s / hm[k];  de[k] = (z[k] - z[k+1]) * (un[k] - un[k+1]);  P[k] = (w[k] / hm[k]) * de[k]
    Rn    = R(un)                                   momentum_vmix_twin.rhs_cols with x := un
    hbar[k] = 0.5 * (P[k-1] + P[k]) - z[k] * (Rn[k] / h[k])   (end rows: 0.5 * the one P; n == 1: 0.0 - z[0] * (Rn[0] / h[0]))
    XU[k] = h[k] * z[k]
    XH[k,c] = XH[k,c] + 0.5 * (sum from 0.0 over the slots of edgesOnCell[c], ascending, of hbar[k,e]: computed columns with k < n_e)
    G_tau[e] += dt * z[0];   D_nu[e] -= dt * (sum from 0.0 over k ascending of de[k] / hm[k])  (n >= 2);   D_r[e] -= dt * (z[n-1] * un[n-1])
With a density wanted, z is also formed in the columns with n >= 1 the forward pass skipped; those write neither XU nor hbar.

Round-off of the pairing <X, J delta> for one column against the long-double model (`pairing_bound`), delta = (dx, dh, dtau, dnu, dr)
and v = h o dx + db e_0 + dh o x - dA u the vector z is paired with (dA = diag(dh) + ds W + s dW(dh) + dq e e^T), first order in 2^-53:
  the solve: |z^ - z| <= |A^-1| C_SOLVE (|A||z^| + |X|) =: ez (momentum_vmix_twin's count), paired with |v|;
  the recorded un is the forward twin's, off the long-double u by at most eu (momentum_vmix_twin.bounds): it enters through the
  off-diagonal part of dA, |z^| (|ds||W| + s|dW| + |dq| e e^T) eu, and through Rn / h, which stands for un - u*: R(un) differs from
  h o (u - u*) by at most C_R mR(un) roundings and (s|W| + q e e^T) eu, paired with |z^||dh| / h;
  local roundings: P[k] carries hm (1), w (1), w / hm (1), the two differences (2), their product (1), the product with w / hm (1), and
  the addition P[k-1] + P[k] one more: C_P = 8 on 0.5 (|P[k-1]| + |P[k]|); z (Rn / h) a division and a product, and the subtraction
  that forms hbar one rounding of everything: C_HB = 3 on 0.5 (|P[k-1]| + |P[k]|) + |z||Rn| / h; XU = h z one; G_tau one; the D_nu sum
  de / hm carries hm, two differences, a product and a division (5), n - 2 additions and the product with dt: n + 4; D_r two.
  C_P, C_HB, 1, 1, n + 4, 2 are the constants; nothing is fitted."""
import numpy as np

import momentum_vmix_twin as mv
import oracle as orc
import tracer_vmix_twin as tv

LD = tv.LD
U53 = tv.U53
C_P, C_HB = 8, 3
STRESS, VISCOSITY, DRAG = 1, 2, 4


# ---- the recipe on columns of one depth ---------------------------------------------------------------------------------------------
def adjoint_cols(h, xu, un, s, q=None, b=None):
    """(z, xu_new, hbar, nusum) of columns h, xu, un (ncol, n); nusum: the D_nu sum per column (None for n == 1)."""
    n = h.shape[1]
    w, d, _ = mv.rhs_cols(h, xu, s, q, None)
    z = mv.solve_cols(w, d, xu)
    Rn = mv.rhs_cols(h, un, s, q, b)[2]
    t = z * (Rn / h)
    if n == 1:
        return z, h * z, 0.0 - t, None
    hm = 0.5 * (h[:, :-1] + h[:, 1:])
    ww = np.float64(s) / hm
    de = (z[:, :-1] - z[:, 1:]) * (un[:, :-1] - un[:, 1:])
    P = (ww / hm) * de
    hbar = np.empty_like(h)
    hbar[:, 0] = 0.5 * P[:, 0] - t[:, 0]
    hbar[:, -1] = 0.5 * P[:, -1] - t[:, -1]
    hbar[:, 1:-1] = 0.5 * (P[:, :-1] + P[:, 1:]) - t[:, 1:-1]
    nusum = np.zeros(h.shape[0])
    for k in range(n - 1):
        nusum = nusum + de[:, k] / hm[:, k]
    return z, h * z, hbar, nusum


def computed_depth(mlt, K, q, st, on):
    """The depth of the columns the forward pass computed (0: none) -- csrc's mvmix_depth, 0 everywhere for a step without the pass."""
    nn = np.clip(np.asarray(mlt, dtype=np.int64), 0, K)
    keep = (nn >= 2) | ((nn == 1) & ((q is not None) or st))
    return np.where(keep & bool(on), nn, 0)


def transposed_pass(mesh, mlt, XU, XH, un, hn, dt, nu, drag, tau, dens=None, depth_of=None):
    """One transposed pass on copies of XU (nEdges, K), XH (nCells, K); dens: {STRESS: G_tau, VISCOSITY: D_nu, DRAG: D_r} arrays of
    nEdges, updated in place (absent keys are not wanted).  depth_of: another rule in the place of `computed_depth` (the call
    sequences' mutant of it).  Returns (XU, XH)."""
    XU, XH = XU.copy(), XH.copy()
    dens = dens or {}
    K = XU.shape[1]
    on = mv.pass_on(nu, drag, tau, mlt)
    if dt == 0.0 or not (on or dens):
        return XU, XH
    c1, c2 = mv.edge_cells(mesh)
    s = np.float64(dt) * np.float64(nu)
    q = np.float64(dt) * np.float64(drag) if drag != 0.0 else None
    st = mv.stress_on(tau, mlt)
    nw = (depth_of or computed_depth)(mlt, K, q, st, on)
    nn = np.clip(np.asarray(mlt, dtype=np.int64), 0, K) if dens else nw
    hbar = np.full(XU.shape, np.nan)
    for n in np.unique(nn):
        if n < 1:
            continue
        idx = np.nonzero(nn == n)[0]
        he = 0.5 * (hn[c1[idx], :n] + hn[c2[idx], :n])
        b = np.float64(dt) * np.asarray(tau, dtype=np.float64)[idx] if st else None
        z, xnew, hb, nusum = adjoint_cols(he, XU[idx, :n], un[idx, :n], s, q, b)
        wr = nw[idx] > 0
        XU[idx[wr], :n] = xnew[wr]
        hbar[idx[wr], :n] = hb[wr]
        if STRESS in dens:
            dens[STRESS][idx] = dens[STRESS][idx] + np.float64(dt) * z[:, 0]
        if VISCOSITY in dens and nusum is not None:
            dens[VISCOSITY][idx] = dens[VISCOSITY][idx] - np.float64(dt) * nusum
        if DRAG in dens:
            dens[DRAG][idx] = dens[DRAG][idx] - np.float64(dt) * (z[:, -1] * un[idx, n - 1])
    if nw.any():
        eoc = np.asarray(mesh.edgesOnCell, dtype=np.int64) - 1
        nec = np.asarray(mesh.nEdgesOnCell)
        S = np.zeros(XH.shape)
        any_ = np.zeros(XH.shape, dtype=bool)
        kk = np.arange(K)[None, :]
        for i in range(eoc.shape[1]):
            e = eoc[:, i]
            ok = (i < nec) & (e >= 0)
            take = ok[:, None] & (kk < nw[np.where(ok, e, 0)][:, None])
            S = np.where(take, S + np.where(take, hbar[np.where(ok, e, 0)], 0.0), S)
            any_ |= take
        XH = np.where(any_, XH + 0.5 * S, XH)
    return XU, XH


def host_sum(d):
    """The library's host view of a density: ascending over the caller's edges in long double, rounded once."""
    return float(_ldsum(d))


def _ldsum(d):
    s = LD(0)
    for v in np.asarray(d, dtype=np.float64):
        s += LD(v)
    return np.float64(s)


# ---- the whole sweep ----------------------------------------------------------------------------------------------------------------
class ForcedTwin:
    """oracle.OracleAdjointRK4's tape with the pass behind every step: step(dt) with the nu, drag, tau in force, sweep(XU, XH)."""

    def __init__(self, om, ssh, u, h, want=0):
        self.om, self.mesh, self.K = om, om.mesh, om.K
        self.mlt = np.asarray(om.arrays["maxLevelEdgeTop"])
        self.st = orc.OracleState(om, ssh, u, h)
        self.rk = orc.OracleAdjointRK4(self.st)
        self.c1, self.c2 = mv.edge_cells(self.mesh)
        self.nu, self.drag, self.tau = 0.0, 0.0, None
        self.want = want
        self.recs = []
        self.dens = {b: np.zeros(self.mesh.nEdges) for b in (STRESS, VISCOSITY, DRAG) if want & b}

    def step(self, dt):
        self.rk.step_rk4(dt)
        self.st.u[1][...] = mv.apply(self.st.u[1], self.st.h[1], self.mlt, self.c1, self.c2, dt, self.nu, self.drag, self.tau)
        self.recs.append((self.st.u[1].copy(), self.st.h[1].copy(), self.nu, self.drag, self.tau))

    def seed_sum_sq_ssh(self):
        m = self.mesh
        return np.zeros((m.nEdges, self.K)), np.repeat((2.0 * self.st.ssh[1])[:, None], self.K, axis=1)

    def reverse_rk4(self, P, dt, XU, XH):
        """One step of OracleAdjointRK4.gradient_sum_sq_ssh's loop."""
        a = (dt / 2., dt / 2., dt)
        b = (dt / 6., dt / 3., dt / 3., dt / 6.)
        kU, kH = b[3] * XU, b[3] * XH
        PU, PH = self.rk._tt(P[3][0], P[3][1], kU, kH)
        accU, accH = XU + PU, XH + PH
        for s in (2, 1, 0):
            kU, kH = b[s] * XU + a[s] * PU, b[s] * XH + a[s] * PH
            PU, PH = self.rk._tt(P[s][0], P[s][1], kU, kH)
            accU, accH = accU + PU, accH + PH
        return accU, accH

    def sweep(self, XU, XH):
        """Consumes the tape; the densities accumulate in self.dens (zeroed here, as a seed zeroes them)."""
        for d in self.dens.values():
            d[...] = 0.0
        while self.recs:
            un, hn, nu, drag, tau = self.recs.pop()
            P, dt = self.rk.tape.pop()
            XU, XH = transposed_pass(self.mesh, self.mlt, XU, XH, un, hn, dt, nu, drag, tau, self.dens)
            XU, XH = self.reverse_rk4(P, dt, XU, XH)
        return XU, XH

    def gradients(self):
        out = {}
        if STRESS in self.dens:
            out["surfaceStress"] = self.dens[STRESS].copy()
        if VISCOSITY in self.dens:
            out["viscosity"] = _ldsum(self.dens[VISCOSITY])
        if DRAG in self.dens:
            out["bottomDrag"] = _ldsum(self.dens[DRAG])
        return out


# ---- long double: the pairing of one transposed column with a tangent direction ------------------------------------------------------
def _W_parts(h, s):
    """(W, dWdhm-factor) in long double: W tridiagonal with 1 / hm; returns hm too."""
    h = np.asarray(h).astype(LD)
    ncol, n = h.shape
    hm = (h[:, :-1] + h[:, 1:]) / 2
    return h, hm


def _tri_apply(c, v):
    """(sum_k c[k] (e_k - e_{k+1})(e_k - e_{k+1})^T) v for interface coefficients c (ncol, n-1)."""
    out = np.zeros(v.shape, dtype=LD)
    if v.shape[1] > 1:
        f = c * (v[:, :-1] - v[:, 1:])
        out[:, :-1] += f
        out[:, 1:] -= f
    return out


def _tri_abs(c, v):
    out = np.zeros(v.shape, dtype=LD)
    if v.shape[1] > 1:
        f = np.abs(c) * (np.abs(v[:, :-1]) + np.abs(v[:, 1:]))
        out[:, :-1] += f
        out[:, 1:] += f
    return out


def pairing_ld(h, x, X, dt, nu, r, tau, d):
    """<X, J_ld delta> per column, long double, from A u = h o x + b e_0 differentiated analytically; d = (dx, dh, dtau, dnu, dr) with
    dx, dh (ncol, n), dtau (ncol,), dnu, dr scalars; tau (ncol,) or None; r == 0: no drag.  Also returns what the bound needs."""
    dx, dh, dtau, dnu, dr = d
    # s, q, b: the doubles the forward recipe forms, as momentum_vmix_twin's long-double model takes them
    s, q = LD(float(np.float64(dt) * np.float64(nu))), (LD(float(np.float64(dt) * np.float64(r))) if r != 0.0 else None)
    b = (np.float64(dt) * np.asarray(tau, dtype=np.float64)).astype(LD) if tau is not None else None
    A, inv = mv.dense_ld(h, float(np.float64(dt) * np.float64(nu)), (float(np.float64(dt) * np.float64(r)) if r != 0.0 else None))
    hL, hm = _W_parts(h, s)
    u = mv.pass_ld(h, x, None, None, b, (A, inv))
    z = tv.mv(inv, np.asarray(X).astype(LD))
    dhL, dxL = np.asarray(dh).astype(LD), np.asarray(dx).astype(LD)
    ds, dq = LD(float(dt)) * LD(float(dnu)), LD(float(dt)) * LD(float(dr))
    dhm = (dhL[:, :-1] + dhL[:, 1:]) / 2
    v = hL * dxL + dhL * np.asarray(x).astype(LD) - dhL * u
    v[:, 0] += LD(float(dt)) * np.asarray(dtau).astype(LD)
    coef = ds / hm - s * dhm / (hm * hm) if hL.shape[1] > 1 else np.zeros((hL.shape[0], 0), dtype=LD)
    v -= _tri_apply(coef, u)
    v[:, -1] -= dq * u[:, -1]
    vabs = hL * np.abs(dxL) + np.abs(dhL) * (np.abs(np.asarray(x).astype(LD)) + np.abs(u))
    vabs[:, 0] += np.abs(LD(float(dt)) * np.asarray(dtau).astype(LD))
    cabs = np.abs(ds) / hm + s * np.abs(dhm) / (hm * hm) if hL.shape[1] > 1 else coef
    vabs += _tri_abs(cabs, u)
    vabs[:, -1] += np.abs(dq) * np.abs(u[:, -1])
    return (z * v).sum(axis=1), {"A": A, "inv": inv, "vabs": vabs, "cabs": cabs, "hm": hm, "s": s, "q": q, "dq": dq, "ds": ds}


def pairing_twin(h, x, X, dt, nu, r, tau, d):
    """The twin's side: un from the forward twin, the transposed column, and <(XU', hbar, G, D_nu, D_r), delta> accumulated in long
    double; returns (pairing, parts for the bound)."""
    dx, dh, dtau, dnu, dr = d
    s = np.float64(dt) * np.float64(nu)
    q = np.float64(dt) * np.float64(r) if r != 0.0 else None
    b = np.float64(dt) * np.asarray(tau, dtype=np.float64) if tau is not None else None
    un = mv.pass_cols(h, x, s, q, b)
    z, xnew, hbar, nusum = adjoint_cols(h, X, un, s, q, b)
    T = (xnew.astype(LD) * dx).sum(axis=1) + (hbar.astype(LD) * dh).sum(axis=1)
    T += (np.float64(dt) * z[:, 0]).astype(LD) * dtau
    if nusum is not None:
        T += (0.0 - np.float64(dt) * nusum).astype(LD) * LD(float(dnu))
    T += (0.0 - np.float64(dt) * (z[:, -1] * un[:, -1])).astype(LD) * LD(float(dr))
    return T, {"un": un, "z": z, "xnew": xnew, "hbar": hbar, "nusum": nusum, "s": s, "q": q, "b": b}


def pairing_bound(h, x, X, dt, nu, r, tau, d, ld, tw):
    """The docstring's bound on |pairing_twin - pairing_ld| per column, with the factor 2^-53."""
    dx, dh, dtau, dnu, dr = d
    n = h.shape[1]
    z, un = np.abs(tw["z"]).astype(LD), tw["un"]
    hL = np.asarray(h).astype(LD)
    ez = tv.mv(np.abs(ld["inv"]), mv.C_SOLVE * (tv.mv(np.abs(ld["A"]), z) + np.abs(X).astype(LD)))
    B = (ez * ld["vabs"]).sum(axis=1)
    eu = mv.bounds(h, x, tw["s"], tw["q"], tw["b"])[2]
    B += (z * (_tri_abs(ld["cabs"], eu))).sum(axis=1) + z[:, -1] * np.abs(ld["dq"]) * eu[:, -1]
    mR = mv.rhs_abs(h, un, tw["s"], tw["q"], tw["b"])
    sw = ld["s"] / ld["hm"] if n > 1 else ld["cabs"]
    spread = _tri_abs(sw, eu)
    if tw["q"] is not None:
        spread[:, -1] += LD(float(tw["q"])) * eu[:, -1]
    adh = np.abs(dh).astype(LD)
    B += (z * adh * (mv.C_R * mR + spread) / hL).sum(axis=1)
    Rn = np.abs(mv.rhs_cols(h, un, tw["s"], tw["q"], tw["b"])[2]).astype(LD)
    Pm = np.zeros(h.shape, dtype=LD)
    if n > 1:
        hm = 0.5 * (h[:, :-1] + h[:, 1:])
        P = np.abs((tw["s"] / hm / hm) * ((tw["z"][:, :-1] - tw["z"][:, 1:]) * (un[:, :-1] - un[:, 1:]))).astype(LD)
        Pm[:, :-1] += P / 2
        Pm[:, 1:] += P / 2
        de_hm = np.abs((tw["z"][:, :-1] - tw["z"][:, 1:]) * (un[:, :-1] - un[:, 1:]) / hm).astype(LD)
        B += (n + 4) * abs(float(dt) * float(dnu)) * de_hm.sum(axis=1)
    B += (adh * (C_P * Pm + C_HB * (Pm + z * Rn / hL))).sum(axis=1)
    B += (np.abs(tw["xnew"]).astype(LD) * np.abs(dx)).sum(axis=1)
    B += np.abs(float(dt) * tw["z"][:, 0] * dtau)
    B += 2 * np.abs(float(dt) * float(dr) * tw["z"][:, -1] * un[:, -1])
    return B * U53
