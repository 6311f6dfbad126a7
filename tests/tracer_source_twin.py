"""Numpy twins of tracer sources (moka_tracer_source_upload) and of the gradient with respect to them
(moka_tracer_adjoint_want_source_gradient), and long-double restatements that share no code with them.  Extends
tests/tracer_diffusion_twin.py and tests/tracer_adjoint_twin.py, whose docstrings state the schemes this file adds one line to.

Forward (include/moka_hip.h): d(h phi)/dt = -div(F phi_e) + div(kappa h_e grad phi) + q.  For every stage tendency, after the whole slot
loop, one more addition with a rounding of its own: T = T + q_j[k,c].  The RK4 recipe is untouched and all four stages see the same q.
`SourceTwin.step_rk4` restates TracerDiffusionTwin.step_rk4 with that line (tracer j without a source: no addition at all) and keeps
RecordingTwin's records.  T is never -0.0 before the addition (it starts at +0.0 and x + (-x) = +0.0 under round-to-nearest), so a
source of +-0.0 leaves its bits alone.

Reverse.  tau_3 = b[3] * g and tau_{s-1} = b[s-1] * g + a[s-1] * v (s = 3, 2, 1) are the values tracer_adjoint_twin's recipe multiplies
by invA; tau_s is the adjoint of stage s's tendency, hence of q.  Per recorded step, in this order, G = G + tau_3, + tau_2, + tau_1,
+ tau_0, each with its own rounding.  `SourceAdjointTwin.reverse_step` is AdjointTwin.reverse_step with tau named and those additions;
y = tau * invA has the bits of the parent's y.

Long double.  `step_ld` is one forward step over recorded provisional states from tracer_diffusion_twin.tendency_ld plus q;
`taus_ld` is the reverse recipe's tau_3..tau_0 with R = T^T from tracer_adjoint_twin.forward_matrices_ld (w = y * areaCell = tau in
long double: no rounding of invArea on the reference's side).

Round-off counts (one rounding per +, -, *, /; the conventions of the files above, whose slack of C_H - 11 = 5 is kept).
  C_TS   one element of T: tracer_diffusion_twin.py's longest chain of 21, one addition deeper: 22, + 5 = 27.
  C_TAU  one element of tau_0, the deepest of the four: g 1, b[3] * g 1 (tau_3: 2); from tau_s to tau_{s-1}: y = tau * invA 2 (forming
         invA, the product), R 19 (tracer_adjoint_twin.py, with diffusion), v 1, a * v 1, the sum with b * g 1: 24; 2 + 3 * 24 = 74,
         + 5 = 79.  Magnitudes through the same recipe: |g|, b |g|, M^T of them, quotients by |ph|.
  C_STEP_SRC  the identity <X, phi_N(phi_0, q) - phi_N(phi_0, 0)> = <G, q> per recorded step.  Forward: tracer_adjoint_twin.py's 100
         with each of the four tendencies one addition deeper: 104, and two runs are differenced (the difference itself is taken in
         long double, exact): 208.  Reverse: that file's 96 for the chain of X through the step, and the four additions of G: 100.
         C_STEP_SRC = 308, on sum |X| W with W the magnitude evaluation of the forward steps on |phi_0| with the source |q|
         (`forward_magnitude`: every sum of magnitudes, the run with q bounds the run without).
  C_REST the rest state (u = 0, uniform h, phi level-wise uniform, so the slot sum is exactly +0.0 and T == q exactly): per step
         Qc = phi * h 1; every b[s] * q is off the exact b_s q by 2 (forming b[s] = dt/6 or dt/3, the product), and the four terms
         have one sign and sum to the increment, so together they weigh 2; the four additions of Qn 4; the quotient 1: C_REST = 8, on
         |phi_n| (every partial sum has the sign of q and is below the final value).  n steps: n * 8 * 2^-53 * |phi_n|.
  Content: tracer_diffusion_twin.py's bound with C_TS for C_TD, M_s including |q|, and one more per b[s] M_s for forming b[s], which the
         exact budget n dt sum A q (unlike conservation) depends on:
             |S_new - S_old - dt sum_c A_c sum_k q| <= 2^-53 sum_c A_c sum_k (12 (|Qc| + sum_s b[s] M_s) + (C_TS + 3) sum_s b[s] M_s)."""
import numpy as np

import tracer_adjoint_twin as ta
import tracer_cases as tc
import tracer_diffusion_twin as td
import trisk_reference as tr
from del4_twin import TwinState

LD = tr.LD
SLACK = tr.C_H - 11
C_TS = 22 + SLACK
C_TAU = 74 + SLACK
C_STEP_SRC = 2 * 104 + 96 + 4
C_REST = 8
assert (C_TS, C_TAU, C_STEP_SRC) == (27, 79, 308)


class SourceTwin(ta.RecordingTwin):
    """RecordingTwin with one optional source per tracer: `source` is a list (tracer j takes source[j]; None or a missing entry =
    no source) and may be replaced between steps."""

    def __init__(self, om, base, kappa, source=()):
        super().__init__(om, base, kappa)
        self.source = list(source)

    def source_of(self, j):
        return self.source[j] if j < len(self.source) else None

    def step_rk4(self, st, phis, dt, magnitudes=False):
        """TracerDiffusionTwin.step_rk4 line by line, with T = T + q_j behind every tendency of a sourced tracer; the step is recorded
        as RecordingTwin does (the dycore hook sees each stage's state)."""
        self._P = []
        a = (dt / 2., dt / 2., dt)
        b = (dt / 6., dt / 3., dt / 3., dt / 6.)
        st.ssh[0], st.u[0], st.h[0] = st.ssh[1].copy(), st.u[1].copy(), st.h[1].copy()
        phis[0] = [p.copy() for p in phis[1]]
        cu, ch = st.u[0], st.h[0]
        newU, newH = st.u[1].copy(), st.h[1].copy()
        pu, ph = st.u[1], st.h[1]
        Qc = [p * ch for p in phis[0]]
        Qn = [q.copy() for q in Qc]
        pphi = list(phis[0])
        n = len(Qc)
        assert len(self.kappa) >= n
        mesh = self.om.mesh
        bM = [np.zeros(ch.shape, dtype=LD) for _ in Qc] if magnitudes else None
        for s in range(4):
            tu, th = self.dycore(pu, ph)
            tend = []
            for j in range(n):
                T = self.tendency(pu, ph, pphi[j], self.kappa[j])
                q = self.source_of(j)
                tend.append(T if q is None else T + q)
            if magnitudes:
                for j in range(n):
                    m = td.tendency_ld(mesh, pu, ph, pphi[j], self.mlt, self.kappa[j])[1]
                    q = self.source_of(j)
                    bM[j] += LD(b[s]) * (m if q is None else m + np.abs(q).astype(LD))
            if s < 3:
                pu, ph = cu + a[s] * tu, ch + a[s] * th
                pphi = [(Qc[j] + a[s] * tend[j]) / ph for j in range(n)]
            newU, newH = newU + b[s] * tu, newH + b[s] * th
            Qn = [Qn[j] + b[s] * tend[j] for j in range(n)]
        st.tendU, st.tendH = tu, th
        st.u[1], st.h[1] = newU, newH
        st.ssh[1] = self.om.update_ssh(newH)
        phis[1] = [Qn[j] / newH for j in range(n)]
        if magnitudes:
            self.last_M = [(np.abs(Qc[j]).astype(LD), bM[j]) for j in range(n)]
        assert len(self._P) == 4
        self.tape.append({"P": self._P, "hn": st.h[1].copy(), "kappa": [float(k) for k in self.kappa[:n]], "dt": dt})
        self._P = None


def content_bound(mesh, absQc, bM):
    """The docstring's bound on |S_new - S_old - dt sum A q| of one step from the magnitudes SourceTwin.step_rk4(magnitudes=True) leaves."""
    a = np.asarray(mesh.areaCell, dtype=np.float64).astype(LD)
    return tr.U53 * (a * (12 * (absQc + bM) + (C_TS + 3) * bM).sum(axis=1)).sum()


class SourceAdjointTwin(ta.AdjointTwin):
    """AdjointTwin whose reverse step also accumulates the gradient with respect to the sources."""

    def reverse_step(self, rec, X, diff=True, G=None, taus=None):
        """G: None, or a list with one accumulator (updated in place) or None per tracer.  taus: None, or a list that receives, per
        tracer, [tau_3, tau_2, tau_1, tau_0]."""
        dt = rec["dt"]
        a = (dt / 2., dt / 2., dt)
        b = (dt / 6., dt / 3., dt / 3., dt / 6.)
        invA = self.tw.invArea[:, None]
        out = []
        for j, x in enumerate(X):
            kap = rec["kappa"][j]
            Gj = None if G is None else G[j]
            tl = []
            g = x / rec["hn"]
            tau = b[3] * g
            y = tau * invA
            tl.append(tau)
            if Gj is not None:
                Gj += tau
            S = None
            for s in (3, 2, 1):
                pu, ph = rec["P"][s]
                r = self.R(pu, ph, y, kap, diff)
                v = r / ph
                S = v if s == 3 else S + v
                tau = b[s - 1] * g + a[s - 1] * v
                y = tau * invA
                tl.append(tau)
                if Gj is not None:
                    Gj += tau
            pu, ph = rec["P"][0]
            r = self.R(pu, ph, y, kap, diff)
            out.append(ph * (g + S) + r)
            if taus is not None:
                taus.append(tl)
        return out

    def sweep(self, tape, X, want=()):
        """Reverse over every record, last first.  Returns (X, G): G[j] = the gradient with respect to tracer j's source for j in
        `want`, else None."""
        diff = any(k != 0.0 for rec in tape for k in rec["kappa"])
        G = [np.zeros_like(x) if j in want else None for j, x in enumerate(X)]
        for rec in reversed(tape):
            X = self.reverse_step(rec, X, diff, G)
        return X, G


# ---- long double ------------------------------------------------------------------------------------------------------------------
def step_ld(mesh, mlt, rec, phi, kappa, q):
    """phi_new of one recorded step in long double: the header's recipe over the record's provisional states, every tendency
    tracer_diffusion_twin.tendency_ld + q (q None: no source)."""
    dt = LD(rec["dt"])
    a = (dt / 2, dt / 2, dt)
    b = (dt / 6, dt / 3, dt / 3, dt / 6)
    h = [np.asarray(p[1], dtype=np.float64).astype(LD) for p in rec["P"]]
    p = np.asarray(phi).astype(LD) if np.asarray(phi).dtype != LD else np.asarray(phi)
    Qc = p * h[0]
    Qn = Qc.copy()
    for s in range(4):
        t = td.tendency_ld(mesh, rec["P"][s][0], rec["P"][s][1], p, mlt, kappa, want_m=False)[0]
        if q is not None:
            t = t + np.asarray(q, dtype=np.float64).astype(LD)
        if s < 3:
            p = (Qc + a[s] * t) / h[s + 1]
        Qn = Qn + b[s] * t
    return Qn / np.asarray(rec["hn"], dtype=np.float64).astype(LD)


def forward_magnitude(mesh, mlt, rec, absd, kappa, absq):
    """W: the magnitude evaluation of one recorded forward step on the nonnegative field `absd` with the source magnitude `absq`."""
    dt = LD(rec["dt"])
    a = (dt / 2, dt / 2, dt)
    b = (dt / 6, dt / 3, dt / 3, dt / 6)
    h = [np.abs(np.asarray(p[1], dtype=np.float64).astype(LD)) for p in rec["P"]]
    mq = np.asarray(absq, dtype=np.float64).astype(LD)
    Qc = np.asarray(absd, dtype=LD) * h[0]
    Qn = Qc.copy()
    p = np.asarray(absd, dtype=LD)
    for s in range(4):
        m = td.tendency_ld(mesh, rec["P"][s][0], rec["P"][s][1], p, mlt, kappa)[1] + mq
        if s < 3:
            p = (Qc + a[s] * m) / h[s + 1]
        Qn = Qn + b[s] * m
    return Qn / np.abs(np.asarray(rec["hn"], dtype=np.float64).astype(LD))


def taus_ld(mesh, mlt, rec, x, kappa):
    """([tau_3, tau_2, tau_1, tau_0], their magnitudes) of one recorded step in long double: the header's reverse recipe with
    R(P_s, tau * invA) = T_s^T tau from the forward tendency's matrix on unit vectors."""
    dt = LD(rec["dt"])
    a = (dt / 2, dt / 2, dt)
    b = (dt / 6, dt / 3, dt / 3, dt / 6)
    g = np.asarray(x, dtype=np.float64).astype(LD) / np.asarray(rec["hn"], dtype=np.float64).astype(LD)
    mg = np.abs(g)
    tau, mtau = b[3] * g, b[3] * mg
    taus, mags = [tau], [mtau]
    for s in (3, 2, 1):
        pu, ph = rec["P"][s]
        T, M = ta.forward_matrices_ld(mesh, pu, ph, mlt, kappa)
        r, _ = ta.transpose_apply(T, M, tau)
        mr = np.stack([M[k].T @ mtau[:, k] for k in range(M.shape[0])], axis=1)
        phl = np.asarray(ph, dtype=np.float64).astype(LD)
        v, mv = r / phl, mr / np.abs(phl)
        tau, mtau = b[s - 1] * g + a[s - 1] * v, b[s - 1] * mg + a[s - 1] * mv
        taus.append(tau)
        mags.append(mtau)
    return taus, mags


# ---- the forced plane wave (tracer_cases.py's mode with a source of the same wave vector) ------------------------------------------
EIG_SIGMA = 1.0 / (tc.EIG_STEPS * tc.EIG_DT)       # the forced part n dt sigma is of order one


def eigen_source(mesh, K):
    """q = h sigma cos(k . x) on every level."""
    c = np.cos(tc.EIG_K[0] * np.asarray(mesh.xCell) + tc.EIG_K[1] * np.asarray(mesh.yCell))
    return np.repeat((tc.EIG_H * EIG_SIGMA * c)[:, None], K, axis=1)


def eigen_factors(kappa):
    """(z, R(z), psi(z), psi after z^2/6): phi^_{n+1} = R phi^_n + dt psi sigma for the mode amplitude under RK4 with a constant forcing."""
    z = tc.eigenmode_z(kappa)
    R = 1 + z + z ** 2 / 2 + z ** 3 / 6 + z ** 4 / 24
    return z, R, 1 + z / 2 + z ** 2 / 6 + z ** 3 / 24, 1 + z / 2 + z ** 2 / 6


def forced_wave_check(phi, mesh, K, kappa, phi0, label):
    """phi0 = 1 + 0.5 cos(k . x) (amplitude 0.5) forced by eigen_source: after n = EIG_STEPS steps the amplitude is
    R^n 0.5 + dt psi sigma (R^n - 1) / (R - 1).  Asserts the deviation <= n * 32 * 2^-53 * max(max|phi0|, |forced amplitude|) and that the
    same bound refuses psi = 1 (a source applied to Qn only) and psi truncated after z^2/6.  Prints every figure; returns the deviation."""
    n = tc.EIG_STEPS
    z, R, psi, psi2 = eigen_factors(kappa)
    geo = (R ** n - 1) / (R - 1)
    amp = lambda ps: R ** n * 0.5 + tc.EIG_DT * ps * EIG_SIGMA * geo                 # noqa: E731
    forced = abs(tc.EIG_DT * psi * EIG_SIGMA * geo)
    tol = n * 32 * 2.0 ** -53 * max(float(np.abs(phi0).max()), forced)
    gap = lambda ps: float(np.abs(phi - tc.eigenmode_expect(mesh, K, 2 * amp(ps))).max())      # noqa: E731
    dev, gap1, gap2 = gap(psi), gap(1.0), gap(psi2)
    print(f"{label}: z = {z:.6g}, forced amplitude = {forced:.5f}, max deviation = {dev:.3e}, tolerance = {tol:.3e}, "
          f"gap to psi = 1: {gap1:.3e}, to psi after z^2/6: {gap2:.3e}")
    assert 0.1 < forced < 10.0
    assert dev <= tol
    assert gap1 > tol and gap2 > tol
    return dev


def forced_wave_gradient_check(G, mesh, K, kappa, X0, label):
    """Seed X = X0 = 1 + 0.5 cos(k . x): the gradient with respect to the source after n recorded steps is, mode by mode, the conjugate
    of the forward response: n dt / h for the constant part (psi(0) = 1, R(0) = 1) and dt conj(psi) (conj(R)^n - 1) / (conj(R) - 1) / h
    times 0.5 for the wave.  Same form of bound: n * 32 * 2^-53 * max|G expected|; it refuses psi = 1, psi after z^2/6 and the
    unconjugated factor.  Prints every figure; returns the deviation."""
    n = tc.EIG_STEPS
    z, R, psi, psi2 = eigen_factors(kappa)
    wave = np.exp(1j * (tc.EIG_K[0] * np.asarray(mesh.xCell) + tc.EIG_K[1] * np.asarray(mesh.yCell)))

    def expect(ps, Rf):
        f = tc.EIG_DT * ps * (Rf ** n - 1) / (Rf - 1) / tc.EIG_H
        return np.repeat((n * tc.EIG_DT / tc.EIG_H + 0.5 * (f * wave).real)[:, None], K, axis=1)

    ex = expect(np.conj(psi), np.conj(R))
    tol = n * 32 * 2.0 ** -53 * float(np.abs(ex).max())
    gap = lambda e: float(np.abs(G - e).max())                                       # noqa: E731
    dev, gap1, gap2, gapf = gap(ex), gap(expect(1.0, np.conj(R))), gap(expect(np.conj(psi2), np.conj(R))), gap(expect(psi, R))
    print(f"{label}: max deviation = {dev:.3e}, tolerance = {tol:.3e}, gap to psi = 1: {gap1:.3e}, to psi after z^2/6: {gap2:.3e}, "
          f"to the forward factor: {gapf:.3e}")
    assert dev <= tol
    assert gap1 > tol and gap2 > tol and gapf > tol
    return dev


# ---- shared cases -------------------------------------------------------------------------------------------------------------------
_REFS = {}


def source_twin(meshname, K, mode="linear", partial=False):
    t = tc.twin_of(meshname, K, mode, partial)
    return SourceTwin(t.om, t.base, [])


def source_fields(meshname, K, n, seed=55):
    """n pairwise distinct sources of both signs: over the case's steps they move h phi by a few per cent of h."""
    mesh = tc.get_mesh(meshname)
    rng = np.random.default_rng(seed)
    scale = (1000.0 / K) / (50.0 * tc.dt_of(meshname))
    return [rng.uniform(-1.0, 1.0, (mesh.nCells, K)) * scale for _ in range(n)]


def reference(meshname, K, mode, partial, diff, nT, srcs, wants, nsteps=2):
    """Computed once per case and shared (never modified by a test): nsteps recorded RK4 steps of tc.state_of's state with the first nT
    of tc.distinct_fields(mesh, K, 9), the sources source_fields(meshname, K, 9)[j] for j in srcs and, when diff, the diffusivities
    tc.kappas(meshname, 9)[:nT]; then the reverse sweep of ta.seeds(mesh, K, 9)[:nT] with the source gradients of `wants`.  A dict:
    twin, fields, sources (None where there is none), forward = tc.reference's tuple per step, X, grad, G (None where not wanted)."""
    key = (meshname, K, mode, partial, diff, nT, tuple(srcs), tuple(wants), nsteps)
    if key not in _REFS:
        mesh = tc.get_mesh(meshname)
        twin = source_twin(meshname, K, mode, partial)
        twin.kappa = tc.kappas(meshname, 9)[:nT] if diff else [0.0] * nT
        q = source_fields(meshname, K, 9)
        twin.source = [q[j] if j in srcs else None for j in range(nT)]
        ssh, u, h, _ = tc.state_of(meshname, K)
        st = TwinState(ssh, u, h)
        f = tc.distinct_fields(mesh, K, 9)[:nT]
        phis = [[a.copy() for a in f], [a.copy() for a in f]]
        fwd = []
        for _ in range(nsteps):
            twin.step_rk4(st, phis, tc.dt_of(meshname))
            fwd.append(([a.copy() for a in phis[0]], [a.copy() for a in phis[1]], st.u[1].copy(), st.h[1].copy(), st.ssh[1].copy()))
        X = ta.seeds(mesh, K, 9)[:nT]
        grad, G = SourceAdjointTwin(twin).sweep(twin.tape, [x.copy() for x in X], tuple(wants))
        _REFS[key] = {"twin": twin, "fields": f, "sources": list(twin.source), "forward": fwd, "X": X, "grad": grad, "G": G}
    return _REFS[key]
