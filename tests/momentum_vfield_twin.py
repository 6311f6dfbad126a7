"""Numpy twin of the implicit vertical mixing of momentum with a viscosity per interface and edge
(moka_vertical_viscosity_field_upload), forwards, transposed (moka_forced_tape) and in the density DF, and a long-double restatement
that builds the column matrix densely from per-interface s[k].  Built on tests/momentum_vmix_twin.py and tests/forced_adjoint_twin.py:
every line of their recipes but one is theirs, taken with s as an (ncol, n-1) array where they take a number (tracer_vmix_twin.weights
does, as tests/tracer_vfield_twin.py uses it for the tracers).

Recipe (include/moka_hip.h).  The field f is (nEdges, K) here, the host layout of normalVelocity; column k of an edge is the interface
between levels k and k+1; with n_e = min(maxLevelEdgeTop[e], K) the entries k >= n_e - 1 are never read (NaN allowed).  With a field
    s[k] = dt * f[k,e]                          one product, rounded once
    w[k] = s[k] / (0.5 * (h[k] + h[k+1]))       k = 0 .. n-2
and d, R, the stress and drag lines, Solve and u_new = x + Solve(R) stay letter for letter; nuV is not read.  A field whose active
entries are all zero (`field_on`, the host scan of the upload) counts as nuV == 0.  The transposed pass takes w[k] = s[k] / hm[k] in
both places; G_tau, D_nu and D_r keep their formulas; the new density, per reversed step with dt != 0, edge with n >= 2, k <= n-2:
    DF[k,e] = DF[k,e] - dt * (de[k] / hm[k])    each operation rounded once
with or without a field in that step.

Long double (`dense_ld_field`): momentum_vmix_twin.dense_ld with iw[k] = s[k] / hm[k], s[k] the double the recipe forms taken into
long double, as that model takes the one s.  The round-off counts of momentum_vmix_twin (C_SOLVE, C_R) and forced_adjoint_twin (C_P,
C_HB, n + 4) therefore hold unchanged: s[k] is still one product formed before the model starts, and nothing else in a row's
arithmetic changed.  `bounds_field`, `pairing_*_field` restate mv.bounds and fa.pairing_* with that matrix; the direction of the
viscosity is a field df (ncol, n-1), paired with the twin's -dt * (de[k] / hm[k]), whose count (hm, two differences, a product, a
division, the product with dt: 6) is covered by the n + 4 >= 6 of the D_nu line on the same magnitudes."""
import numpy as np

import forced_adjoint_twin as fa
import momentum_vmix_twin as mv
import tracer_cases as tc
import tracer_vmix_twin as tv

LD = tv.LD
U53 = tv.U53


# ---- the host scan --------------------------------------------------------------------------------------------------------------------
def live_of(mlt, K):
    """(nEdges, K) mask of the interfaces a launch reads: k < min(maxLevelEdgeTop[e], K) - 1."""
    nn = np.minimum(np.asarray(mlt, dtype=np.int64), K)
    return np.arange(K)[None, :] < (nn - 1)[:, None]


def field_on(f, mlt):
    return bool(np.any(f[live_of(mlt, f.shape[1])] != 0.0))


def check_field(f, mlt):
    """What moka_vertical_viscosity_field_upload refuses: a negative, NaN or infinite value at an active interface."""
    v = f[live_of(mlt, f.shape[1])]
    return bool(np.all(np.isfinite(v)) and np.all(v >= 0.0))


def pass_on(nu, drag, tau, mlt, fld=None):
    """A field sets nu aside: it counts when an active entry is nonzero."""
    return (field_on(fld, mlt) if fld is not None else nu != 0.0) or drag != 0.0 or mv.stress_on(tau, mlt)


def taken(nu, fld, mlt):
    """(nu, fld) as the pass takes them: the field that is on, else the scalar -- 0.0 under a field whose active entries are all zero."""
    if fld is None:
        return float(nu), None
    return 0.0, (fld if field_on(fld, mlt) else None)


# ---- forward ------------------------------------------------------------------------------------------------------------------------
def apply(u, h, mlt, c1, c2, dt, nu, drag=0.0, tau=None, fld=None):
    """momentum_vmix_twin.apply with s[k] = dt * fld[e,k] when a field is on; a new array."""
    nu, fld = taken(nu, fld, mlt)
    if fld is None:
        return mv.apply(u, h, mlt, c1, c2, dt, nu, drag, tau)
    K = u.shape[1]
    out = u.copy()
    if dt == 0.0:
        return out
    q = np.float64(dt) * np.float64(drag) if drag != 0.0 else None
    st = mv.stress_on(tau, mlt)
    nn = np.minimum(np.asarray(mlt, dtype=np.int64), K)
    for n in np.unique(nn):
        if n < 1 or (n == 1 and q is None and not st):
            continue
        idx = np.nonzero(nn == n)[0]
        he = 0.5 * (h[c1[idx], :n] + h[c2[idx], :n])
        b = np.float64(dt) * np.asarray(tau, dtype=np.float64)[idx] if st else None
        out[idx, :n] = mv.pass_cols(he, u[idx, :n], np.float64(dt) * fld[idx, :n - 1], q, b)
    return out


class MomentumVfieldTwin(mv.MomentumVmixTwin):
    """momentum_vmix_twin.MomentumVmixTwin whose pass may take a field: `fld` (None = the scalar nu) may be replaced between steps."""

    def __init__(self, tw, nu=0.0, drag=0.0, tau=None, fld=None):
        super().__init__(tw, nu, drag, tau)
        self.fld = fld

    def mix(self, u, h, dt):
        assert self.fld is None or check_field(self.fld, self.mlt)
        return apply(u, h, self.mlt, self.c1, self.c2, dt, self.nu, self.drag, self.tau, self.fld)


def momentum_twin(meshname, K, mode="linear", mlt=None):
    return MomentumVfieldTwin(tv.vmix_twin(meshname, K, mode, False, mlt))


# ---- transposed ---------------------------------------------------------------------------------------------------------------------
def df_terms(h, z, un, dt):
    """dt * (de[k] / hm[k]) of columns of one depth n >= 2, (ncol, n-1)."""
    hm = 0.5 * (h[:, :-1] + h[:, 1:])
    de = (z[:, :-1] - z[:, 1:]) * (un[:, :-1] - un[:, 1:])
    return np.float64(dt) * (de / hm)


def transposed_pass(mesh, mlt, XU, XH, un, hn, dt, nu, drag, tau, fld=None, dens=None, DF=None):
    """forced_adjoint_twin.transposed_pass with the step's field (None: the scalar nu) and the density DF (nEdges, K), updated in place
    (None: not wanted).  `nu`, `fld` are what the step took (`taken`).  Returns (XU, XH)."""
    XU, XH = XU.copy(), XH.copy()
    dens = dens or {}
    grad = bool(dens) or DF is not None
    K = XU.shape[1]
    on = (fld is not None) or mv.pass_on(nu, drag, tau, mlt)
    if dt == 0.0 or not (on or grad):
        return XU, XH
    c1, c2 = mv.edge_cells(mesh)
    q = np.float64(dt) * np.float64(drag) if drag != 0.0 else None
    st = mv.stress_on(tau, mlt)
    nw = fa.computed_depth(mlt, K, q, st, on)
    nn = np.clip(np.asarray(mlt, dtype=np.int64), 0, K) if grad else nw
    hbar = np.full(XU.shape, np.nan)
    for n in np.unique(nn):
        if n < 1:
            continue
        idx = np.nonzero(nn == n)[0]
        he = 0.5 * (hn[c1[idx], :n] + hn[c2[idx], :n])
        b = np.float64(dt) * np.asarray(tau, dtype=np.float64)[idx] if st else None
        s = np.float64(dt) * fld[idx, :n - 1] if fld is not None else np.float64(dt) * np.float64(nu)
        z, xnew, hb, nusum = fa.adjoint_cols(he, XU[idx, :n], un[idx, :n], s, q, b)
        wr = nw[idx] > 0
        XU[idx[wr], :n] = xnew[wr]
        hbar[idx[wr], :n] = hb[wr]
        if fa.STRESS in dens:
            dens[fa.STRESS][idx] = dens[fa.STRESS][idx] + np.float64(dt) * z[:, 0]
        if fa.VISCOSITY in dens and nusum is not None:
            dens[fa.VISCOSITY][idx] = dens[fa.VISCOSITY][idx] - np.float64(dt) * nusum
        if fa.DRAG in dens:
            dens[fa.DRAG][idx] = dens[fa.DRAG][idx] - np.float64(dt) * (z[:, -1] * un[idx, n - 1])
        if DF is not None and n >= 2:
            DF[idx, :n - 1] = DF[idx, :n - 1] - df_terms(he, z, un[idx, :n], dt)
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


class ForcedFieldTwin(fa.ForcedTwin):
    """forced_adjoint_twin.ForcedTwin whose steps may run with a field: `fld` (None = the scalar nu) may be replaced between steps;
    want_field: the density DF, in self.DF after a sweep."""

    def __init__(self, om, ssh, u, h, want=0, want_field=False):
        super().__init__(om, ssh, u, h, want)
        self.fld = None
        self.DF = np.zeros((self.mesh.nEdges, self.K)) if want_field else None

    def step(self, dt):
        assert self.fld is None or check_field(self.fld, self.mlt)
        self.rk.step_rk4(dt)
        self.st.u[1][...] = apply(self.st.u[1], self.st.h[1], self.mlt, self.c1, self.c2, dt, self.nu, self.drag, self.tau, self.fld)
        nu, fld = taken(self.nu, self.fld, self.mlt)
        self.recs.append((self.st.u[1].copy(), self.st.h[1].copy(), nu, self.drag, self.tau, None if fld is None else fld.copy()))

    def sweep(self, XU, XH):
        for d in self.dens.values():
            d[...] = 0.0
        if self.DF is not None:
            self.DF[...] = 0.0
        while self.recs:
            un, hn, nu, drag, tau, fld = self.recs.pop()
            P, dt = self.rk.tape.pop()
            XU, XH = transposed_pass(self.mesh, self.mlt, XU, XH, un, hn, dt, nu, drag, tau, fld, self.dens, self.DF)
            XU, XH = self.reverse_rk4(P, dt, XU, XH)
        return XU, XH


# ---- long double ------------------------------------------------------------------------------------------------------------------
def dense_ld_field(h, s, q=None):
    """(A, Ainv) in long double of columns h (ncol, n) with the per-interface doubles s (ncol, n-1): momentum_vmix_twin.dense_ld
    generalised to iw[k] = s[k] / hm[k]."""
    h = np.asarray(h).astype(LD)
    ncol, n = h.shape
    k = np.arange(n)
    A = np.zeros((ncol, n, n), dtype=LD)
    A[:, k, k] = h
    if n > 1:
        iw = np.asarray(s, dtype=np.float64).astype(LD) / ((h[:, :-1] + h[:, 1:]) / 2)
        A[:, k[:-1], k[:-1]] += iw
        A[:, k[1:], k[1:]] += iw
        A[:, k[:-1], k[1:]] = -iw
        A[:, k[1:], k[:-1]] = -iw
    if q is not None:
        A[:, n - 1, n - 1] += LD(float(q))
    M = A.copy()
    inv = np.zeros_like(A)
    inv[:, k, k] = 1
    for p in range(n):
        piv = M[:, p, p][:, None].copy()
        M[:, p, :] = M[:, p, :] / piv
        inv[:, p, :] = inv[:, p, :] / piv
        for r in range(n):
            if r != p:
                f = M[:, r, p][:, None].copy()
                M[:, r, :] -= f * M[:, p, :]
                inv[:, r, :] -= f * inv[:, p, :]
    return A, inv


def bounds_field(h, x, s, q=None, b=None):
    """momentum_vmix_twin.bounds with s (ncol, n-1): (u^, u, err, mom), the bounds without the factor 2^-53."""
    w, d, R = mv.rhs_cols(h, x, s, q, b)
    z = mv.solve_cols(w, d, R)
    new = x + z
    A, inv = dense_ld_field(h, s, q)
    res = tv.mv(np.abs(A), np.abs(z)) + np.abs(R).astype(LD)
    inner = mv.C_SOLVE * res + mv.C_R * mv.rhs_abs(h, x, s, q, b)
    err = tv.mv(np.abs(inv), inner) + np.abs(new)
    mom = (inner + np.asarray(h).astype(LD) * np.abs(new)).sum(axis=1) + (LD(float(q)) * np.abs(new[:, -1]) if q is not None else 0)
    return new, mv.pass_ld(h, x, None, q, b, (A, inv)), err, mom


def pairing_ld_field(h, x, X, dt, f, r, tau, d):
    """forced_adjoint_twin.pairing_ld with the field f (ncol, n-1) and d = (dx, dh, dtau, df, dr), df (ncol, n-1)."""
    dx, dh, dtau, df, dr = d
    s64 = np.float64(dt) * np.asarray(f, dtype=np.float64)
    s = s64.astype(LD)
    q64 = float(np.float64(dt) * np.float64(r)) if r != 0.0 else None
    b = (np.float64(dt) * np.asarray(tau, dtype=np.float64)).astype(LD) if tau is not None else None
    A, inv = dense_ld_field(h, s64, q64)
    hL = np.asarray(h).astype(LD)
    hm = (hL[:, :-1] + hL[:, 1:]) / 2
    u = mv.pass_ld(h, x, None, None, b, (A, inv))
    z = tv.mv(inv, np.asarray(X).astype(LD))
    dhL, dxL = np.asarray(dh).astype(LD), np.asarray(dx).astype(LD)
    ds, dq = LD(float(dt)) * np.asarray(df, dtype=np.float64).astype(LD), LD(float(dt)) * LD(float(dr))
    dhm = (dhL[:, :-1] + dhL[:, 1:]) / 2
    v = hL * dxL + dhL * np.asarray(x).astype(LD) - dhL * u
    v[:, 0] += LD(float(dt)) * np.asarray(dtau).astype(LD)
    coef = ds / hm - s * dhm / (hm * hm)
    v -= fa._tri_apply(coef, u)
    v[:, -1] -= dq * u[:, -1]
    vabs = hL * np.abs(dxL) + np.abs(dhL) * (np.abs(np.asarray(x).astype(LD)) + np.abs(u))
    vabs[:, 0] += np.abs(LD(float(dt)) * np.asarray(dtau).astype(LD))
    cabs = np.abs(ds) / hm + s * np.abs(dhm) / (hm * hm)
    vabs += fa._tri_abs(cabs, u)
    vabs[:, -1] += np.abs(dq) * np.abs(u[:, -1])
    return (z * v).sum(axis=1), {"A": A, "inv": inv, "vabs": vabs, "cabs": cabs, "hm": hm, "s": s, "dq": dq, "ds": ds}


def pairing_twin_field(h, x, X, dt, f, r, tau, d):
    """The twin's side: un from the forward twin, the transposed column, and <(XU', hbar, G_tau, DF, D_r), delta> in long double."""
    dx, dh, dtau, df, dr = d
    s = np.float64(dt) * np.asarray(f, dtype=np.float64)
    q = np.float64(dt) * np.float64(r) if r != 0.0 else None
    b = np.float64(dt) * np.asarray(tau, dtype=np.float64) if tau is not None else None
    un = mv.pass_cols(h, x, s, q, b)
    z, xnew, hbar, nusum = fa.adjoint_cols(h, X, un, s, q, b)
    DF = 0.0 - df_terms(h, z, un, dt)
    T = (xnew.astype(LD) * dx).sum(axis=1) + (hbar.astype(LD) * dh).sum(axis=1)
    T += (np.float64(dt) * z[:, 0]).astype(LD) * dtau
    T += (DF.astype(LD) * np.asarray(df, dtype=np.float64).astype(LD)).sum(axis=1)
    T += (0.0 - np.float64(dt) * (z[:, -1] * un[:, -1])).astype(LD) * LD(float(dr))
    return T, {"un": un, "z": z, "xnew": xnew, "hbar": hbar, "nusum": nusum, "DF": DF, "s": s, "q": q, "b": b}


def pairing_bound_field(h, x, X, dt, f, r, tau, d, ld, tw):
    """forced_adjoint_twin.pairing_bound, term for term, with the per-interface s and df; with the factor 2^-53."""
    dx, dh, dtau, df, dr = d
    n = h.shape[1]
    z, un = np.abs(tw["z"]).astype(LD), tw["un"]
    hL = np.asarray(h).astype(LD)
    ez = tv.mv(np.abs(ld["inv"]), mv.C_SOLVE * (tv.mv(np.abs(ld["A"]), z) + np.abs(X).astype(LD)))
    B = (ez * ld["vabs"]).sum(axis=1)
    eu = bounds_field(h, x, tw["s"], tw["q"], tw["b"])[2]
    B += (z * (fa._tri_abs(ld["cabs"], eu))).sum(axis=1) + z[:, -1] * np.abs(ld["dq"]) * eu[:, -1]
    mR = mv.rhs_abs(h, un, tw["s"], tw["q"], tw["b"])
    spread = fa._tri_abs(ld["s"] / ld["hm"], eu)
    if tw["q"] is not None:
        spread[:, -1] += LD(float(tw["q"])) * eu[:, -1]
    adh = np.abs(dh).astype(LD)
    B += (z * adh * (mv.C_R * mR + spread) / hL).sum(axis=1)
    Rn = np.abs(mv.rhs_cols(h, un, tw["s"], tw["q"], tw["b"])[2]).astype(LD)
    hm = 0.5 * (h[:, :-1] + h[:, 1:])
    dz_du = (tw["z"][:, :-1] - tw["z"][:, 1:]) * (un[:, :-1] - un[:, 1:])
    P = np.abs((tw["s"] / hm / hm) * dz_du).astype(LD)
    Pm = np.zeros(h.shape, dtype=LD)
    Pm[:, :-1] += P / 2
    Pm[:, 1:] += P / 2
    de_hm = np.abs(dz_du / hm).astype(LD)
    B += (n + 4) * (np.abs(float(dt) * np.asarray(df, dtype=np.float64)).astype(LD) * de_hm).sum(axis=1)
    B += (adh * (fa.C_P * Pm + fa.C_HB * (Pm + z * Rn / hL))).sum(axis=1)
    B += (np.abs(tw["xnew"]).astype(LD) * np.abs(dx)).sum(axis=1)
    B += np.abs(float(dt) * tw["z"][:, 0] * dtau)
    B += 2 * np.abs(float(dt) * float(dr) * tw["z"][:, -1] * un[:, -1])
    return B * U53


# ---- kernel forms -----------------------------------------------------------------------------------------------------------------
def adjoint_form(K, field, generic=False):
    """The form of the transposed pass restated from csrc/tracer_vmix.hip's vmix_kernel: four column sets of cs = K | 1 doubles a
    resident column, five for a step that ran with a field; 64-column tiles while four fit a CU's 160 KiB, 32-column tiles while two
    do, else (and for K < 2 and kernel variant 3) the column form."""
    sets, cs = (5 if field else 4), K | 1
    if not generic and K >= 2:
        for t, fit in ((64, 4), (32, 2)):
            if (sets * t * cs * 8 + t * 4) * fit <= 160 * 1024:
                return 1, t
    return 2, 0


# ---- shared cases -----------------------------------------------------------------------------------------------------------------
def case_field(meshname, K, mlt, seed=77, nan=True):
    """The viscosity field of the cases: uniform in [0, 2] x momentum_vmix_twin.coefficients' nuV, a surface-intensified factor on
    top (x 4 at the first interface), exact zeros at interface 1 of every fifth edge and at every interface but the first of edge 3,
    and NaN in every never-read entry (k >= n_e - 1)."""
    mesh = tc.get_mesh(meshname)
    nu = mv.coefficients(meshname, max(K, 1))[0]
    f = np.random.default_rng(seed).uniform(0.0, 2.0, (mesh.nEdges, K)) * nu
    f[:, 0] *= 4.0
    if K > 1:
        f[::5, 1] = 0.0
    f[3, 1:] = 0.0
    if nan:
        f[~live_of(mlt, K)] = np.nan
    return f


def uniform_field(nE, K, mlt, value, nan=True):
    f = np.full((nE, K), float(value))
    if nan:
        f[~live_of(mlt, K)] = np.nan
    return f
