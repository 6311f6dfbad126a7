"""Numpy twin of the gradient of a tracer objective with respect to the vertical diffusivity kappaV_j
(moka_tracer_adjoint_want_vertical_gradient), a long-double restatement from tracer_vmix_twin.dense_ld, and a long-double forward
step with a diffusivity per interface and cell to difference against.  Extends tests/tracer_vmix_twin.py.

Recipe (include/moka_hip.h).  Per recorded step (its dt, hn = h, kappaV_j), flagged tracer j and column with n = nLev[c] >= 2, with X
the adjoint of phi_new at the head of the reversed step (before S^T) and p = phi_new as the step left it, every operation rounded once:
    z = Solve(X)  (tracer_vmix_twin.solve, s = dt * kappaV_j)  when kappaV_j != 0;      z[k] = X[k] / h[k]  when kappaV_j == 0
    k = 0 .. n-2:   q = dt / (0.5 * (h[k] + h[k+1]));   c = (p[k] - p[k+1]) * q;   e = (z[k] - z[k+1]) * c;   D[k,c] = D[k,c] - e
D is (nCells, K) here (the host layout of every field); row k is the interface between levels k and k+1; rows k >= nLev[c] - 1 stay 0.0.
A step with dt == 0.0 and a mesh with K < 2 contribute nothing.  Views (`views`): cell Wv[c] = sum_k D, profile Pv[k] = sum_c D, the
scalar sum_c sum_k D, each ascending in long double and rounded once (tracer_kgrad_twin.host_sum).

Long double (`density_ld`): A from dense_ld(h, s) (s = 0: A = diag(h)), z = A^-1 X, D = -dt (z[k] - z[k+1]) (p[k] - p[k+1]) / hm[k],
hm[k] = (h[k] + h[k+1]) / 2, from the doubles h, X, p, dt and s that the twin used.

Round-off bound of one element of D after N recorded steps, first order in u = 2^-53 (`density_ld` returns it):
  the solve: |z^ - z| <= ez := C_BR u |A^-1| (|A| |z^| + |X|) per level (tracer_vmix_twin.py counts C_BR = 21, slack included; for
  kappaV == 0 the one division z^ = X / h is far inside it), so the difference z[k] - z[k+1] is off by at most ez[k] + ez[k+1], which
  reaches e through the factor |c^|;
  the recipe: e^ is the exact product (z^[k] - z^[k+1]) (p[k] - p[k+1]) dt / hm[k] with the relative errors of the addition in hm (0.5 *
  is exact), and of the five operations behind it: the division q, the two differences and the two products: C_E = 6 on |e^|;
  the accumulation D = D - e: one rounding of |D| as it stands after each step.
  bound = sum over the steps of ((ez[k] + ez[k+1]) |c^| + C_E u |e^| + u |D^ after the step|).
The scalar and the views add one rounding of their own sum (host_sum rounds once): u |sum| on top of the sum of the element bounds.

`tile_columns_grad(K, generic)` restates csrc/tracer_vmix.hip's rule for the gradient instances of the reverse pass."""
import numpy as np

import tracer_adjoint_twin as ta
import tracer_biharmonic_twin as tb
import tracer_cases as tc
import tracer_kgrad_twin as tk
import tracer_vmix_twin as tv
from del4_twin import TwinState

LD = tv.LD
U53 = tv.U53
C_E = 6


def density_cols(h, X, p, dt, kv):
    """e (ncol, n-1) of columns of one depth n >= 2: what the step subtracts from D."""
    if kv != 0.0:
        w = tv.weights(h, np.float64(dt) * np.float64(kv))
        z = tv.solve(w, tv.diagonal(h, w), X)
    else:
        z = X / h
    q = np.float64(dt) / (0.5 * (h[:, :-1] + h[:, 1:]))
    c = (p[:, :-1] - p[:, 1:]) * q
    return (z[:, :-1] - z[:, 1:]) * c


def accumulate(D, h, X, p, nlev, dt, kv):
    """D = D - e over every column of depth >= 2, in place; levels k >= nLev[c] of h, X and p are never read."""
    K = D.shape[1]
    if K < 2 or dt == 0.0:
        return
    for n in np.unique(nlev):
        if n >= 2:
            idx = np.nonzero(nlev == n)[0]
            D[idx, :n - 1] = D[idx, :n - 1] - density_cols(h[idx, :n], X[idx, :n], p[idx, :n], dt, kv)


def views(D):
    """(cell (nCells,), profile (K,), scalar) of a density."""
    cell = np.array([tk.host_sum(D[c]) for c in range(D.shape[0])])
    prof = np.array([tk.host_sum(D[:, k]) for k in range(D.shape[1])])
    return cell, prof, tk.host_sum(D.ravel())


class VgradTwin(tv.VmixTwin):
    """VmixTwin whose records gain "phi_new": every tracer's new-level field as the step left it."""

    def step_rk4(self, st, phis, dt, magnitudes=False):
        super().step_rk4(st, phis, dt, magnitudes)
        self.tape[-1]["phi_new"] = [p.copy() for p in phis[1]]


class VgradAdjointTwin(tv.VmixAdjointTwin):
    """VmixAdjointTwin that also accumulates D of the tracers flagged for d J / d kappaV."""

    def heads_of(self, tape, X):
        """[X at the head of record n, before S^T] for every n, by the sweep the whole tape selects."""
        Xs = [x.copy() for x in X]
        out = [None] * len(tape)
        for n in range(len(tape) - 1, -1, -1):
            out[n] = Xs
            Xs = self.sweep_tail(tape, n, Xs)
        return out, Xs

    def sweep_vgrad(self, tape, X, vflags, flags=None, want=()):
        """(X, G, W, D): sweep_kgrad's three, untouched, and D[j] (nCells, K) for every j of `vflags`."""
        K = X[0].shape[1]
        nlev = self.tw.nlev(K)
        D = {int(j): np.zeros(X[0].shape) for j in vflags}
        heads, X0 = self.heads_of(tape, X)
        for n in range(len(tape) - 1, -1, -1):
            rec = tape[n]
            for j, d in D.items():
                accumulate(d, rec["hn"], heads[n][j], rec["phi_new"][j], nlev, rec["dt"], rec["kappaV"][j])
        if any(np.isnan(x).any() for x in X):        # a filled case: the parent's sweep compares its fields without equal_nan
            assert not flags and not want
            return X0, None, {}, D
        Xf, G, W = self.sweep_kgrad(tape, [x.copy() for x in X], dict(flags or {}), tuple(want))
        for xa, xb in zip(X0, Xf):
            assert np.array_equal(xa, xb)            # record by record is the parent's sweep
        return Xf, G, W, D


# ---- long double ------------------------------------------------------------------------------------------------------------------
def density_ld(adj, tape, X, j):
    """(D, bound): the density of tracer j in long double from the twin's X at the head of every record, and the module docstring's
    bound per element, (nCells, K) each."""
    K = X[0].shape[1]
    nlev = adj.tw.nlev(K)
    heads, _ = adj.heads_of(tape, X)
    D = np.zeros(X[0].shape, dtype=LD)
    B = np.zeros(X[0].shape, dtype=LD)
    Dt = np.zeros(X[0].shape)                        # the twin's D as it stands
    for n in range(len(tape) - 1, -1, -1):
        rec = tape[n]
        dt, kv = rec["dt"], rec["kappaV"][j]
        if K < 2 or dt == 0.0:
            continue
        s = np.float64(dt) * np.float64(kv)
        accumulate(Dt, rec["hn"], heads[n][j], rec["phi_new"][j], nlev, dt, kv)
        for m in np.unique(nlev):
            if m < 2:
                continue
            idx = np.nonzero(nlev == m)[0]
            h, x, p = rec["hn"][idx, :m], heads[n][j][idx, :m], rec["phi_new"][j][idx, :m]
            A, inv = tv.dense_ld(h, s)
            z = tv.mv(inv, x)
            hl, pl = h.astype(LD), p.astype(LD)
            hm = (hl[:, :-1] + hl[:, 1:]) / 2
            D[idx, :m - 1] -= LD(float(dt)) * (z[:, :-1] - z[:, 1:]) * (pl[:, :-1] - pl[:, 1:]) / hm
            # the twin's own figures
            if kv != 0.0:
                w = tv.weights(h, s)
                zt = tv.solve(w, tv.diagonal(h, w), x)
            else:
                zt = x / h
            ez = tv.C_BR * U53 * tv.mv(np.abs(inv), tv.mv(np.abs(A), np.abs(zt)) + np.abs(x).astype(LD))
            c = (p[:, :-1] - p[:, 1:]) * (np.float64(dt) / (0.5 * (h[:, :-1] + h[:, 1:])))
            e = (zt[:, :-1] - zt[:, 1:]) * c
            B[idx, :m - 1] += (ez[:, :-1] + ez[:, 1:]) * np.abs(c) + C_E * U53 * np.abs(e).astype(LD)
        B += U53 * np.abs(Dt).astype(LD)
    return D, B


def forward_ld_kfield(h, x, nlev, dt, kvf):
    """phi_new of the vertical pass in long double with a diffusivity per interface and cell: kvf (nCells, K), row k of a column the
    interface between k and k+1; A = diag(h) + tridiag of w[k] = dt kvf[k] / hm[k].  Columns of depth >= 2, active levels only."""
    out = np.asarray(x).astype(LD).copy()
    K = out.shape[1]
    if K < 2 or dt == 0.0:
        return out
    for n in np.unique(nlev):
        if n < 2:
            continue
        idx = np.nonzero(nlev == n)[0]
        hl = np.asarray(h)[idx, :n].astype(LD)
        w = LD(float(dt)) * np.asarray(kvf)[idx, :n - 1].astype(LD) / ((hl[:, :-1] + hl[:, 1:]) / 2)
        d = hl.copy()
        d[:, :-1] += w
        d[:, 1:] += w
        r = hl * out[idx, :n]
        # Thomas in long double (A is strictly diagonally dominant)
        beta = d[:, 0].copy()
        y = np.empty_like(r)
        g = np.empty_like(w)
        y[:, 0] = r[:, 0] / beta
        for k in range(1, n):
            g[:, k - 1] = w[:, k - 1] / beta
            beta = d[:, k] - w[:, k - 1] * g[:, k - 1]
            y[:, k] = (r[:, k] + w[:, k - 1] * y[:, k - 1]) / beta
        z = np.empty_like(r)
        z[:, n - 1] = y[:, n - 1]
        for k in range(n - 2, -1, -1):
            z[:, k] = y[:, k] + g[:, k] * z[:, k + 1]
        out[idx, :n] = z
    return out


def tile_columns_grad(K, generic=False):
    """csrc/tracer_vmix.hip's vmix_kernel for the gradient instances, restated from its comment: a resident column takes FOUR sets of
    cs = K | 1 doubles (h / g, X / w, y / Lv, p / c / e), a tile tc * 4 bytes more; 64 columns while four such tiles fit a CU's 160 KiB
    (K <= 19), 32 while two do (K <= 79) -- or 0: the column form (also for K < 2, where nothing is launched, and for kernel variant 3)."""
    cs = K | 1
    if not generic and K >= 2:
        for t, fit in ((64, 4), (32, 2)):
            if (4 * t * cs * 8 + 4 * t) * fit <= 160 * 1024:
                return t
    return 0


# ---- shared cases -----------------------------------------------------------------------------------------------------------------
_REFS = {}


def vgrad_twin(meshname, K, mode="linear", partial=False, mlt=None):
    t = tc.twin_of(meshname, K, mode, partial, mlt)
    return VgradTwin(t.om, t.base, [])


def reference(meshname, K, mode, partial, nT, steps, vflags, diff=False, bih=False, flags=(), wants=(), fields=None, fill=None):
    """Computed once per case and shared (never modified by a test).  As tracer_vmix_twin.reference, with: steps = an int (that many
    steps with kappavs(...) and tc.dt_of) or a tuple of (kappaV list or None = kappavs, dt or None = tc.dt_of) per step; vflags = the
    tracers flagged for d J / d kappaV; fill also in a swept case (the dead levels of X and of the recorded fields then hold it).
    A dict: tv.reference's keys, and D = {j: (nCells, K)}, steps = [(kappaV, dt)]."""
    key = (meshname, K, mode, partial, nT, steps if isinstance(steps, int) else tuple((None if k is None else tuple(k), d) for k, d in steps),
           tuple(vflags), diff, bih, tuple(flags), tuple(wants), fields, fill)
    if key not in _REFS:
        mesh = tc.get_mesh(meshname)
        twin = vgrad_twin(meshname, K, mode, partial is True, tv.column_mlt(mesh, K) if partial == "floor" else None)
        nlev = twin.nlev(K)
        dead = np.arange(K)[None, :] >= nlev[:, None]
        twin.source = [None] * nT
        ssh, u, h, _ = tc.state_of(meshname, K)
        st = TwinState(ssh, u, h)
        f = tc.distinct_fields(mesh, K, 9)[:nT]
        if fields == "unit-first":
            f[0] = np.ones((mesh.nCells, K))
        X = ta.seeds(mesh, K, 9)[:nT]
        if fill is not None:
            f = [np.where(dead, fill, a) for a in f]
            X = [np.where(dead, fill, a) for a in X]
        phis = [[a.copy() for a in f], [a.copy() for a in f]]
        twin.kappa = tc.kappas(meshname, 9)[:nT] if diff else [0.0] * nT
        twin.kappa4 = tb.kappa4s(meshname, 9)[:nT] if bih else [0.0] * nT
        plan = [(None, None)] * steps if isinstance(steps, int) else list(steps)
        fwd, ran = [], []
        for kv, dt in plan:
            twin.kappaV = tv.kappavs(meshname, K, 9)[:nT] if kv is None else [float(k) for k in kv]
            dt = tc.dt_of(meshname) if dt is None else dt
            twin.step_rk4(st, phis, dt)
            ran.append((list(twin.kappaV), dt))
            fwd.append(([a.copy() for a in phis[0]], [a.copy() for a in phis[1]], st.u[1].copy(), st.h[1].copy(), st.ssh[1].copy()))
        grad, G, W, D = VgradAdjointTwin(twin).sweep_vgrad(twin.tape, [x.copy() for x in X], tuple(vflags), dict(flags), tuple(wants))
        _REFS[key] = {"twin": twin, "fields": f, "sources": [None] * nT, "forward": fwd, "X": X, "grad": grad, "G": G, "W": W, "D": D,
                      "kappa": list(twin.kappa), "kappa4": list(twin.kappa4), "steps": ran, "nlev": nlev, "dead": dead}
    return _REFS[key]
