"""Numpy twin of the implicit vertical diffusion of passive tracers with a diffusivity per interface and cell
(moka_tracer_vertical_field_upload), forwards, backwards and in the density D, and a long-double restatement that builds the column
matrix densely from per-interface weights.  Extends tests/tracer_vgrad_twin.py (hence tracer_vmix_twin.py): the RK4 step, its transpose
and every line of the vertical recipe but one are theirs.

Recipe (include/moka_hip.h).  Tracer j may carry a field f (nCells, K) here, the host layout of every field; column k of a cell is the
interface between levels k and k+1; entries k >= nLev[c] - 1 are never read (NaN allowed).  For such a tracer
    s[k] = dt * f[k,c]                          one product, rounded once
    w[k] = s[k] / (0.5 * (h[k] + h[k+1]))       k = 0 .. n-2
and d, Lv, Solve, forward x + Solve(Lv(x)), reverse X + Lv(Solve(X)) and the gradient lines q, c, e, D = D - e stay letter for letter
(tracer_vmix_twin.weights / diagonal / Lv / solve take s as an (ncol, n-1) array as they take a number).  While a tracer has a field
its scalar kappaV is not read.  A field whose active entries are all zero (`field_on`, the host scan of the upload) counts as
kappaV == 0: the tracer is skipped, bits kept, and a gradient takes z = X / h.

Records: "fieldV" = per tracer the field the step ran with (a copy) or None -- None also for a field that is off --, and "kappaV" the
coefficient the pass took: the scalar, or 0.0 for a tracer whose field is off (beside a field that is on it is not read: 0.0 too).

Long double (`dense_ld_field`): tracer_vmix_twin.dense_ld with iw[k] = dt f[k] / hm[k] per interface, the product formed in long
double from the doubles dt and f: the restatement does not share the twin's rounding of s.

Round-off count C_BR_F of one solve with a field, for |A z^ - r| <= C_BR_F 2^-53 (|A| |z^| + |r|) per element, A the long-double matrix:
  the factorisation and the two sweeps are tracer_vmix_twin's: 12 (Higham, Theorems 9.12 and 9.14; row diagonal dominance holds for
  f >= 0, h > 0, an f == 0 interface included: there w = g = 0 and beta = d > 0);
  the entries of A as the twin forms them against the long-double ones: w now takes the product dt * f, the addition in hm and the
  division (0.5 * is exact): 3 where the scalar recipe has 2 (its long-double matrix starts from the rounded s); d two more
  additions, every term non-negative: 5 where the scalar count has 4;
  the house slack of 5 (tracer_biharmonic_twin.SLACK).   C_BR_F = 12 + 5 + 5 = 22.
Lv: the row count C_LV = 3 is on w as the twin holds it; against the long-double w the 3 roundings of w come on top: C_LV_F = 6 on the
same magnitude mLv.  The density: tracer_vgrad_twin's count with C_BR_F for C_BR (q, c and e do not see the field): C_E = 6."""
import numpy as np

import tracer_adjoint_twin as ta
import tracer_biharmonic_twin as tb
import tracer_cases as tc
import tracer_vgrad_twin as tg
import tracer_vmix_twin as tv
from del4_twin import TwinState
from moka_hip import meshgen as mg

LD = tv.LD
U53 = tv.U53
C_BR_F = 12 + 5 + tb.SLACK
C_LV_F = tv.C_LV + 3
C_E = tg.C_E
assert C_BR_F == 22 and C_LV_F == 6


# ---- the recipe on a whole (nCells, K) field ----------------------------------------------------------------------------------------
def field_on(f, nlev):
    """The host scan of the upload: some active interface (k < nLev[c] - 1) holds a nonzero value."""
    live = np.arange(f.shape[1])[None, :] < (np.asarray(nlev) - 1)[:, None]
    return bool(np.any(f[live] != 0.0))


def check_field(f, nlev):
    """What moka_tracer_vertical_field_upload refuses: a negative, NaN or infinite value at an active interface."""
    live = np.arange(f.shape[1])[None, :] < (np.asarray(nlev) - 1)[:, None]
    v = f[live]
    return bool(np.all(np.isfinite(v)) and np.all(v >= 0.0))


def s_cols(dt, f, idx, n):
    return np.float64(dt) * f[idx, :n - 1]


def apply_field(h, x, nlev, dt, f, reverse=False):
    """tracer_vmix_twin.apply with s[k] = dt * f[k,c]: columns of depth >= 2, their active levels and interfaces only; a new array."""
    out = x.copy()
    for n in np.unique(nlev):
        if n < 2:
            continue
        idx = np.nonzero(nlev == n)[0]
        fn = tv.reverse_cols if reverse else tv.forward_cols
        out[idx, :n] = fn(h[idx, :n], x[idx, :n], s_cols(dt, f, idx, n))
    return out


def accumulate_field(D, h, X, p, nlev, dt, f):
    """tracer_vgrad_twin.accumulate with z from the field's solve: D = D - e, in place."""
    K = D.shape[1]
    if K < 2 or dt == 0.0:
        return
    for n in np.unique(nlev):
        if n >= 2:
            idx = np.nonzero(nlev == n)[0]
            hh = h[idx, :n]
            w = tv.weights(hh, s_cols(dt, f, idx, n))
            z = tv.solve(w, tv.diagonal(hh, w), X[idx, :n])
            q = np.float64(dt) / (0.5 * (hh[:, :-1] + hh[:, 1:]))
            c = (p[idx, :n - 1] - p[idx, 1:n]) * q
            D[idx, :n - 1] = D[idx, :n - 1] - (z[:, :-1] - z[:, 1:]) * c


# ---- long double ------------------------------------------------------------------------------------------------------------------
def dense_ld_field(h, dt, f):
    """(A, Ainv) of columns h (ncol, n) with the interface diffusivities f (ncol, n-1) in long double, (ncol, n, n) each:
    tracer_vmix_twin.dense_ld generalised to iw[k] = dt f[k] / hm[k]."""
    h = np.asarray(h, dtype=np.float64).astype(LD)
    ncol, n = h.shape
    iw = LD(float(dt)) * np.asarray(f, dtype=np.float64).astype(LD) / ((h[:, :-1] + h[:, 1:]) / 2)
    A = np.zeros((ncol, n, n), dtype=LD)
    k = np.arange(n)
    A[:, k, k] = h
    A[:, k[:-1], k[:-1]] += iw
    A[:, k[1:], k[1:]] += iw
    A[:, k[:-1], k[1:]] = -iw
    A[:, k[1:], k[:-1]] = -iw
    M = A.copy()
    inv = np.zeros_like(A)
    inv[:, k, k] = 1
    for p in range(n):
        piv = M[:, p, p][:, None].copy()
        M[:, p, :] = M[:, p, :] / piv
        inv[:, p, :] = inv[:, p, :] / piv
        for q in range(n):
            if q != p:
                g = M[:, q, p][:, None].copy()
                M[:, q, :] -= g * M[:, p, :]
                inv[:, q, :] -= g * inv[:, p, :]
    return A, inv


def density_ld_field(adj, tape, X, j):
    """tracer_vgrad_twin.density_ld for a tape whose records may carry a field for tracer j: (D, bound), (nCells, K) each, with
    C_BR_F in the place of C_BR in the steps that ran with a field."""
    K = X[0].shape[1]
    nlev = adj.tw.nlev(K)
    heads, _ = adj.heads_of(tape, X)
    D = np.zeros(X[0].shape, dtype=LD)
    B = np.zeros(X[0].shape, dtype=LD)
    Dt = np.zeros(X[0].shape)
    for n in range(len(tape) - 1, -1, -1):
        rec = tape[n]
        dt, kv, f = rec["dt"], rec["kappaV"][j], rec["fieldV"][j]
        if K < 2 or dt == 0.0:
            continue
        if f is not None:
            accumulate_field(Dt, rec["hn"], heads[n][j], rec["phi_new"][j], nlev, dt, f)
        else:
            tg.accumulate(Dt, rec["hn"], heads[n][j], rec["phi_new"][j], nlev, dt, kv)
        for m in np.unique(nlev):
            if m < 2:
                continue
            idx = np.nonzero(nlev == m)[0]
            h, x, p = rec["hn"][idx, :m], heads[n][j][idx, :m], rec["phi_new"][j][idx, :m]
            if f is not None:
                A, inv = dense_ld_field(h, dt, f[idx, :m - 1])
                w = tv.weights(h, s_cols(dt, f, idx, m))
                zt, cbr = tv.solve(w, tv.diagonal(h, w), x), C_BR_F
            else:
                s = np.float64(dt) * np.float64(kv)
                A, inv = tv.dense_ld(h, s)
                zt, cbr = (tv.solve(tv.weights(h, s), tv.diagonal(h, tv.weights(h, s)), x) if kv != 0.0 else x / h), tv.C_BR
            z = tv.mv(inv, x)
            hl, pl = h.astype(LD), p.astype(LD)
            hm = (hl[:, :-1] + hl[:, 1:]) / 2
            D[idx, :m - 1] -= LD(float(dt)) * (z[:, :-1] - z[:, 1:]) * (pl[:, :-1] - pl[:, 1:]) / hm
            ez = cbr * U53 * tv.mv(np.abs(inv), tv.mv(np.abs(A), np.abs(zt)) + np.abs(x).astype(LD))
            c = (p[:, :-1] - p[:, 1:]) * (np.float64(dt) / (0.5 * (h[:, :-1] + h[:, 1:])))
            e = (zt[:, :-1] - zt[:, 1:]) * c
            B[idx, :m - 1] += (ez[:, :-1] + ez[:, 1:]) * np.abs(c) + C_E * U53 * np.abs(e).astype(LD)
        B += U53 * np.abs(Dt).astype(LD)
    return D, B


# ---- the twins --------------------------------------------------------------------------------------------------------------------
class VfieldTwin(tg.VgradTwin):
    """VgradTwin whose tracers may carry a diffusivity field: `fieldV[j]` (None = the scalar) may be replaced between steps."""

    def __init__(self, om, base, kappa, kappaV=(), fieldV=()):
        super().__init__(om, base, kappa, kappaV)
        self.fieldV = list(fieldV)

    def field_of(self, j):
        return self.fieldV[j] if j < len(self.fieldV) else None

    def step_rk4(self, st, phis, dt, magnitudes=False):
        n, K = len(phis[1]), st.h[1].shape[1]
        nlev = self.nlev(K)
        flds = [self.field_of(j) for j in range(n)]
        for f in flds:
            assert f is None or check_field(f, nlev)
        on = [f is not None and field_on(f, nlev) for f in flds]
        keep = self.kappaV
        self.kappaV = [0.0 if flds[j] is not None else self.kappaV_of(j) for j in range(n)]      # the scalar of a field tracer is not read
        try:
            super().step_rk4(st, phis, dt, magnitudes)
        finally:
            self.kappaV = keep
        rec = self.tape[-1]
        rec["fieldV"] = [flds[j].copy() if on[j] else None for j in range(n)]
        if K >= 2 and dt != 0.0:
            for j in range(n):
                if on[j]:
                    phis[1][j] = apply_field(st.h[1], phis[1][j], nlev, dt, flds[j])
        rec["phi_new"] = [p.copy() for p in phis[1]]


class VfieldAdjointTwin(tg.VgradAdjointTwin):
    """VgradAdjointTwin whose S^T and whose density take the field a record ran with."""

    def head(self, rec, x, j):
        f = rec.get("fieldV", [None] * (j + 1))[j]
        if f is None:
            return super().head(rec, x, j)
        if x.shape[1] < 2 or rec["dt"] == 0.0:
            return x
        return apply_field(rec["hn"], x, self.tw.nlev(x.shape[1]), rec["dt"], f, reverse=True)

    def sweep_vgrad(self, tape, X, vflags, flags=None, want=()):
        K = X[0].shape[1]
        nlev = self.tw.nlev(K)
        D = {int(j): np.zeros(X[0].shape) for j in vflags}
        heads, X0 = self.heads_of(tape, X)
        for n in range(len(tape) - 1, -1, -1):
            rec = tape[n]
            for j, d in D.items():
                f = rec.get("fieldV", [None] * (j + 1))[j]
                if f is not None:
                    accumulate_field(d, rec["hn"], heads[n][j], rec["phi_new"][j], nlev, rec["dt"], f)
                else:
                    tg.accumulate(d, rec["hn"], heads[n][j], rec["phi_new"][j], nlev, rec["dt"], rec["kappaV"][j])
        Xf, G, W = self.sweep_kgrad(tape, [x.copy() for x in X], dict(flags or {}), tuple(want))
        for xa, xb in zip(X0, Xf):
            assert np.array_equal(xa, xb)
        return Xf, G, W, D


# ---- shared cases -----------------------------------------------------------------------------------------------------------------
ZEROS = ((0, 0), (1, 2), (5, 1), (7, 0))          # (cell, interface) of the exact zeros of case_field, where they exist


def case_field(meshname, K, nlev, seed=77, nan=True):
    """The diffusivity field of the GPU cases: uniform in [0, 2] x the largest of tracer_vmix_twin.kappavs' three values, exact zeros
    at the interfaces ZEROS, at every interface of cell 3 but the first, and NaN in every never-read entry (k >= nLev[c] - 1)."""
    mesh = tc.get_mesh(meshname)
    scale = tv.kappavs(meshname, K, 3)[0] if K >= 1 else 1.0
    f = np.random.default_rng(seed).uniform(0.0, 2.0, (mesh.nCells, K)) * scale
    for c, k in ZEROS:
        if c < mesh.nCells and k < K:
            f[c, k] = 0.0
    if mesh.nCells > 3:
        f[3, 1:] = 0.0
    if nan:
        f[np.arange(K)[None, :] >= (np.asarray(nlev) - 1)[:, None]] = np.nan
    return f


_REFS = {}


def sheared_mesh(nx, ny):
    """The name under which tracer_cases.get_mesh (hence every twin, reference and Model) finds the doubly periodic hex mesh of nx x ny
    cells closed as a sheared torus (meshgen.planar_hex_mesh(..., sheared=True)): ny may be odd, so the cell count may be -- no other
    mesh of the tests has an odd one, and with an odd nVertLevels on top the tracers of a state lie an odd number of doubles apart."""
    name = f"sheared-{nx}-{ny}"
    if name not in tc._MESHES:
        tc._MESHES[name] = mg.planar_hex_mesh(nx, ny, 1000.0, f0=1e-4, sheared=True)
    return name


def vfield_twin(meshname, K, mode="linear", partial=False, mlt=None):
    t = tc.twin_of(meshname, K, mode, partial, mlt)
    return VfieldTwin(t.om, t.base, [])


def reference(meshname, K, partial, plan, vflags=(), nT=3, mode="linear", fill=None, wants=()):
    """Computed once per case and shared (never modified by a test).  nT tracers of tc.distinct_fields over tc.state_of's state;
    plan = one (fields, scalars) per step: fields a tuple of nT entries, each None (the scalar), "A" / "B" (case_field with seed 77 /
    78), "zero" (all zero, NaN in the never-read entries), "uniform" (the tracer's scalar of kappavs at every entry); scalars None =
    tv.kappavs(meshname, K, nT) or a tuple.  Then the sweep of ta.seeds with the vertical gradients `vflags` and the source gradients
    `wants`.  partial: False, or
    "floor" (tv.column_mlt).  fill: written into every level k >= nLev[c] of the tracers and the seeds.
    A dict: twin, fields, forward, X, grad, G, D, steps = [(fields as arrays or None, scalars, dt)], nlev, dead."""
    key = (meshname, K, partial, tuple(plan), tuple(vflags), nT, mode, fill, tuple(wants))
    if key not in _REFS:
        mesh = tc.get_mesh(meshname)
        twin = vfield_twin(meshname, K, mode, False, tv.column_mlt(mesh, K) if partial == "floor" else None)
        nlev = twin.nlev(K)
        dead = np.arange(K)[None, :] >= nlev[:, None]
        twin.source = [None] * nT
        ssh, u, h, _ = tc.state_of(meshname, K)
        st = TwinState(ssh, u, h)
        f = tc.distinct_fields(mesh, K, 9)[:nT]
        X = ta.seeds(mesh, K, 9)[:nT]
        if fill is not None:
            f = [np.where(dead, fill, a) for a in f]
            X = [np.where(dead, fill, a) for a in X]
        phis = [[a.copy() for a in f], [a.copy() for a in f]]
        twin.kappa, twin.kappa4 = [0.0] * nT, [0.0] * nT
        never = np.arange(K)[None, :] >= (nlev - 1)[:, None]
        fwd, ran = [], []
        for names, scal in plan:
            kv = tv.kappavs(meshname, K, 9)[:nT] if scal is None else [float(k) for k in scal]
            made = []
            for j, name in enumerate(names):
                if name is None:
                    made.append(None)
                elif name in ("A", "B"):
                    made.append(case_field(meshname, K, nlev, 77 if name == "A" else 78))
                elif name == "zero":
                    made.append(np.where(never, np.nan, 0.0))
                elif name == "uniform":
                    made.append(np.where(never, np.nan, kv[j]))
                else:
                    raise ValueError(name)
            twin.kappaV, twin.fieldV = kv, made
            dt = tc.dt_of(meshname)
            twin.step_rk4(st, phis, dt)
            ran.append((made, kv, dt))
            fwd.append(([a.copy() for a in phis[0]], [a.copy() for a in phis[1]], st.u[1].copy(), st.h[1].copy(), st.ssh[1].copy()))
        grad = G = D = None
        if fill is None:
            grad, G, _, D = VfieldAdjointTwin(twin).sweep_vgrad(twin.tape, [x.copy() for x in X], tuple(vflags), None, tuple(wants))
        _REFS[key] = {"twin": twin, "fields": f, "forward": fwd, "X": X, "grad": grad, "G": G, "D": D, "steps": ran, "nlev": nlev, "dead": dead}
    return _REFS[key]
