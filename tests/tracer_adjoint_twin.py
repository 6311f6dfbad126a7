"""Numpy twin of the reverse mode of passive tracer transport over a frozen flow (moka_tracer_tape_*), and a long-double reference of
its transposed tendency that shares no code with it.  Extends tests/tracer_diffusion_twin.py (the forward scheme and its twin).

Scheme (include/moka_hip.h).  With the flow given, one RK4 tracer step is a linear map M of phi.  Its transpose needs the step's
provisional states P_s = (pu_s, ph_s), s = 0..3, the new thickness hn and the diffusivities only.  The transposed tendency r = R(P, y)
of a field y that carries invArea already accumulates, per cell c and level k, from 0.0 over the slots i of edgesOnCell in slot order
(empty slots and slots with k >= maxLevelEdgeTop[e] skipped; c' = the cell across slot i):
    hE = 0.5 * (ph[k,c] + ph[k,c']);  F = pu[k,e] * hE
    r += ((0.5 * F) * sdv[c,i]) * (y[k,c] - y[k,c'])
    r += ((kappa_j * hE) * dvdc[c,i]) * (y[k,c'] - y[k,c])            a second, separate addition (0.0 * ... = +-0.0 for kappa_j == 0)
and one step backwards is, with a = (dt/2, dt/2, dt), b = (dt/6, dt/3, dt/3, dt/6), X the adjoint of phi_new:
    g = X / hn;  y = (b[3] * g) * invA
    s = 3, 2, 1:  r = R(P_s, y);  v = r / ph_s;  S = (s == 3 ? v : S + v);  y = (b[s-1] * g + a[s-1] * v) * invA
    r = R(P_0, y);  X_prev = ph_0 * (g + S) + r
`AdjointTwin.R` and `AdjointTwin.reverse_step` are these lines in double, one slot at a time over all cells (the library's bits).
`RecordingTwin` is TracerDiffusionTwin with the provisional states of every step kept (its dycore hook sees each stage's state), so
that the reverse twin is driven by the forward twin's own run.

Round-off chain of one element of R in the library's order (one rounding per +, -, *, /, including forming dvdc; 0.5 and the signs are
exact; y is an input).  An advective term is 5 deep: hE 1, F 1, * sdv 1, the difference 1 (on |y_c| + |y_c'|, which the magnitude
carries), the product 1.  A diffusive term is 6 deep: hE 1, kappa * hE 1, dvdc 1, * dvdc 1, the difference 1, the product 1.  The
accumulator takes up to 14 additions (7 slots, two terms each), the first onto 0.0 exact: 13 -- 7 additions, 6 counted, without
diffusion.  Longest chain 6 + 13 = 19 with diffusion, 5 + 6 = 11 without.  trisk_reference.py carries its tendH count of 11 as
C_H = 16 and the tracer twins keep that slack of 5 (C_T, C_TD):
    C_R = 19 + 5 = 24,    C_R0 = 11 + 5 = 16 (every kappa zero),
and each element is checked as |R - R_ref| <= C 2^-53 M.

The reference.  `forward_matrices_ld` builds the matrix of the FORWARD tendency T(P, .) column by column from
tracer_diffusion_twin.tendency_ld on unit vectors (levels do not couple: one call per cell yields that cell's column on every level),
together with the matrix of magnitudes from the same calls -- trisk_reference.py's magnitude evaluation, every leaf and intermediate
replaced by a bound, differences summed, so the diagonal does not cancel.  `transpose_apply` forms T^T w and M^T |w|.  Since R takes
y = w * invArea, the check hands the reference w = y * areaCell in long double: no rounding of invArea is charged to either side.

One step, counted the same way for the step-level identity <X, M d> = <M^T X, d> (the longest chain of dependent roundings):
    forward: Qc 1; four tendencies of 21 (tracer_diffusion_twin.py) 84; three provisional tracers (a * t, +, /) 9; the last b * t 1
             and the four additions of Qn 4; / hn 1:  100
    reverse: g 1; the first y (b * g, * invA with forming invA) 3; three times R 19, v 1, the next y (a * v, +, * invA) 4: 72; the last
             R 19 and the final addition 1:  96
so that n steps are within n * (100 + 96) * 2^-53 * sum |X| W of each other, W the magnitude evaluation of the forward steps on
|d| (`forward_magnitude`: tendency_ld's magnitudes through the RK4 recipe, every sum of magnitudes, every quotient by |ph|)."""
import numpy as np

import tracer_cases as tc
import tracer_diffusion_twin as td
import trisk_reference as tr
from del4_twin import TwinState

LD = tr.LD
SLACK = tr.C_H - 11
C_R = 19 + SLACK
C_R0 = 11 + SLACK
C_STEP = 100 + 96
assert (C_R, C_R0) == (24, 16)


class RecordingTwin(td.TracerDiffusionTwin):
    """TracerDiffusionTwin whose step_rk4 leaves a record of the step in self.tape: a dict with P = [(pu_s, ph_s)] * 4, hn, kappa
    (the values in force), dt.  The forward arithmetic is the parent's, untouched."""

    def __init__(self, om, base, kappa):
        super().__init__(om, base, kappa)
        self.tape = []
        self._P = None

    def dycore(self, u, h):
        if self._P is not None:
            self._P.append((np.array(u, copy=True), np.array(h, copy=True)))
        return super().dycore(u, h)

    def step_rk4(self, st, phis, dt, magnitudes=False):
        self._P = []
        super().step_rk4(st, phis, dt, magnitudes)
        assert len(self._P) == 4
        self.tape.append({"P": self._P, "hn": st.h[1].copy(), "kappa": [float(k) for k in self.kappa[:len(phis[1])]], "dt": dt})
        self._P = None


class AdjointTwin:
    """The reverse recipe over the stencil arrays of a tracer twin `tw` (eoc, coc, sdv, dvdc, invArea, slot_mask)."""

    def __init__(self, tw):
        self.tw = tw

    def R(self, pu, ph, y, kappa=0.0, diff=True):
        """diff=False: the instances without diffusion (no second addition at all)."""
        tw = self.tw
        r = np.zeros_like(ph)
        kappa = np.float64(kappa)
        for i in range(tw.eoc.shape[1]):
            n = tw.coc[:, i]
            hE = 0.5 * (ph + ph[n])
            F = pu[tw.eoc[:, i]] * hE
            m = tw.slot_mask(i)
            r = np.where(m, r + ((0.5 * F) * tw.sdv[:, i, None]) * (y - y[n]), r)
            if diff:
                r = np.where(m, r + ((kappa * hE) * tw.dvdc[:, i, None]) * (y[n] - y), r)
        return r

    def reverse_step(self, rec, X, diff=True):
        """X: the adjoints of the new tracers (a list of (nCells, K) arrays); returns those of the step's current tracers."""
        dt = rec["dt"]
        a = (dt / 2., dt / 2., dt)
        b = (dt / 6., dt / 3., dt / 3., dt / 6.)
        invA = self.tw.invArea[:, None]
        out = []
        for j, x in enumerate(X):
            kap = rec["kappa"][j]
            g = x / rec["hn"]
            y = (b[3] * g) * invA
            S = None
            for s in (3, 2, 1):
                pu, ph = rec["P"][s]
                r = self.R(pu, ph, y, kap, diff)
                v = r / ph
                S = v if s == 3 else S + v
                y = (b[s - 1] * g + a[s - 1] * v) * invA
            pu, ph = rec["P"][0]
            r = self.R(pu, ph, y, kap, diff)
            out.append(ph * (g + S) + r)
        return out

    def sweep(self, tape, X):
        """Reverse over every record of `tape`, last first.  The diffusion instances run when any recorded kappa is nonzero."""
        diff = any(k != 0.0 for rec in tape for k in rec["kappa"])
        for rec in reversed(tape):
            X = self.reverse_step(rec, X, diff)
        return X


# ---- the long-double reference: the forward tendency's matrix, transposed ---------------------------------------------------------
def forward_matrices_ld(mesh, pu, ph, mlt, kappa):
    """(T, M): (K, nC, nC) long-double arrays, T[k][:, j] = the forward tendency of the unit field of cell j on level k, M its
    magnitude (tracer_diffusion_twin.tendency_ld)."""
    nC, K = np.asarray(ph).shape
    T = np.zeros((K, nC, nC), dtype=LD)
    M = np.zeros((K, nC, nC), dtype=LD)
    for j in range(nC):
        e = np.zeros((nC, K))
        e[j, :] = 1.0
        t, m = td.tendency_ld(mesh, pu, ph, e, mlt, kappa)
        T[:, :, j] = t.T
        M[:, :, j] = m.T
    return T, M


def transpose_apply(T, M, w):
    """(T^T w, M^T |w|) per level, w (nC, K) long double."""
    w = np.asarray(w, dtype=LD)
    r = np.stack([T[k].T @ w[:, k] for k in range(T.shape[0])], axis=1)
    m = np.stack([M[k].T @ np.abs(w[:, k]) for k in range(T.shape[0])], axis=1)
    return r, m


def forward_magnitude(mesh, mlt, rec, absd, kappa):
    """W: the magnitude evaluation of one recorded forward step on the nonnegative field `absd` (long double)."""
    dt = LD(rec["dt"])
    a = (dt / 2, dt / 2, dt)
    b = (dt / 6, dt / 3, dt / 3, dt / 6)
    h = [np.abs(np.asarray(p[1], dtype=np.float64).astype(LD)) for p in rec["P"]]
    Qc = np.asarray(absd, dtype=LD) * h[0]
    Qn = Qc.copy()
    p = np.asarray(absd, dtype=LD)
    for s in range(4):
        m = td.tendency_ld(mesh, rec["P"][s][0], rec["P"][s][1], p, mlt, kappa)[1]
        if s < 3:
            p = (Qc + a[s] * m) / h[s + 1]
        Qn = Qn + b[s] * m
    return Qn / np.abs(np.asarray(rec["hn"], dtype=np.float64).astype(LD))


def dot_ld(x, y):
    return (np.asarray(x).astype(LD) * np.asarray(y).astype(LD)).sum()


# ---- shared cases: the forward twin's run recorded once per case, seeds and the twin's gradient ------------------------------------
_REFS = {}


def recording_twin(meshname, K, mode="linear", partial=False):
    t = tc.twin_of(meshname, K, mode, partial)
    return RecordingTwin(t.om, t.base, [])


def seeds(mesh, K, n, seed=77):
    """n pairwise distinct adjoint seeds in [-1, 1]."""
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1.0, 1.0, (mesh.nCells, K)) for _ in range(n)]


def reference(meshname, K, mode, partial, diff, nsteps=2, nT=9):
    """Computed once per case and shared (never modified by a test): nsteps recorded RK4 steps of tc.state_of's state with the nT
    tracers tc.distinct_fields(mesh, K, nT) and, when diff, the diffusivities tc.kappas(meshname, nT); then the reverse sweep of the
    seeds(mesh, K, nT).  A dict: twin (its .tape holds the records), fields, forward = tc.reference's tuple per step, X, grad.  The
    first n tracers of the nine are what a model with n tracers computes: tracers do not interact."""
    key = (meshname, K, mode, partial, diff, nsteps, nT)
    if key not in _REFS:
        mesh = tc.get_mesh(meshname)
        twin = recording_twin(meshname, K, mode, partial)
        twin.kappa = tc.kappas(meshname, nT) if diff else [0.0] * nT
        ssh, u, h, _ = tc.state_of(meshname, K)
        st = TwinState(ssh, u, h)
        f = tc.distinct_fields(mesh, K, nT)
        phis = [[a.copy() for a in f], [a.copy() for a in f]]
        fwd = []
        for _ in range(nsteps):
            twin.step_rk4(st, phis, tc.dt_of(meshname))
            fwd.append(([a.copy() for a in phis[0]], [a.copy() for a in phis[1]], st.u[1].copy(), st.h[1].copy(), st.ssh[1].copy()))
        X = seeds(mesh, K, nT)
        grad = AdjointTwin(twin).sweep(twin.tape, [x.copy() for x in X])
        _REFS[key] = {"twin": twin, "fields": f, "forward": fwd, "X": X, "grad": grad}
    return _REFS[key]


def plane_wave_check(grad, mesh, K, kappa, phi0, label):
    """The reverse sweep of the plane wave multiplies the mode by conj(R4(z))^n: within n * 32 * 2^-53 * max|phi0| (tc.eigenmode_check's
    tolerance); the same bound refuses the forward factor R4^n and a third-order reverse loop conj(R3)^n by >= 1e6, and the exact
    exponential exp(conj(z) n).  Prints every figure; returns the deviation."""
    n = tc.EIG_STEPS
    z = tc.eigenmode_z(kappa)
    R4 = 1 + z + z ** 2 / 2 + z ** 3 / 6 + z ** 4 / 24
    R3 = 1 + z + z ** 2 / 2 + z ** 3 / 6
    tol = n * 32 * 2.0 ** -53 * float(np.abs(phi0).max())
    gap = lambda f: float(np.abs(grad - tc.eigenmode_expect(mesh, K, f)).max())      # noqa: E731
    dev, gapf, gap3, gapx = gap(np.conj(R4) ** n), gap(R4 ** n), gap(np.conj(R3) ** n), gap(np.exp(np.conj(z) * n))
    print(f"{label}: z = {z:.6g}, max deviation from conj(R4)^{n} = {dev:.3e}, tolerance = {tol:.3e}, gap to the forward factor = "
          f"{gapf:.3e}, to third order = {gap3:.3e}, to exp(conj(z) n) = {gapx:.3e}")
    assert dev <= tol
    assert gapf >= 1e6 * tol and gap3 >= 1e6 * tol and gapx > tol
    return dev
