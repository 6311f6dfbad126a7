"""Numpy twins of biharmonic tracer diffusion (moka_set_tracer_biharmonic), forwards and backwards, and long-double restatements that
share no code with them.  Extends tests/tracer_source_twin.py (the recording / source twin chain), whose docstrings state the schemes
this file adds one pass and one addition to.

Scheme (include/moka_hip.h): d(h phi)/dt = -div(F phi_e) + div(kappa h_e grad phi) - div(kappa4 h_e grad L) + q with
L = (1 / (A h)) sum_e h_e (dv/dc) (phi_c' - phi_c).
Laplacian pass (`TracerBiharmonicTwin.lap`), per cell c and level k, s from 0.0 over the slots in slot order, the tendency's skip rules:
    hE = 0.5 * (ph[k,c] + ph[k,c']);  s += (hE * (x[k,c'] - x[k,c])) * dvdc[c,i];      Lap(ph, x)[k,c] = (s * invArea[c]) / ph[k,c]
Forward: L = Lap(ph_s, pphi) per stage, and in the tendency's slot loop a third, separate addition behind the advective and harmonic ones,
    T = T - ((((kappa4 * hE) * (L[k,c'] - L[k,c])) * dvdc[c,i]) * invArea[c]).
Reverse: M = Lap(ph_s, y) per reverse stage, and in R after the harmonic addition of a slot
    r = r - ((kappa4 * hE) * dvdc[c,i]) * (M[k,c'] - M[k,c]).
The twins form L (M) for EVERY tracer and perform the third addition with kappa4 == 0 too: the term is then +-0.0 on a T (r) that is never
-0.0, so the bits are those without the term -- which is what lets the library skip the pass and the addition for such a tracer.  A step
or sweep in which every kappa4 is zero runs the parents' code (the library's launches are then the parents').

Long double.  `lap_ld` and `tendency_ld` are built from the edge-flux formula with trisk_reference's geometry, active and divergence:
    Lap = div(where(active, hE (x[c2] - x[c1]) / dc, 0)) / h
    T   = -div(where(active, u hE pE - kappa hE (phi[c2] - phi[c1]) / dc + kappa4 hE (L[c2] - L[c1]) / dc, 0))
Magnitudes as in tracer_diffusion_twin.py: every leaf and intermediate replaced by a bound, a difference carried as the sum of the two
magnitudes.  tendency_ld takes L and the magnitude mL to carry for it.

Round-off counts (one rounding per +, -, *, /, including forming 1/areaCell and dvdc; 0.5 and the signs are exact; the house slack of
C_H - 11 = 5 on top, as in the files above).
  C_LAP  one element of Lap: a slot's term is 5 deep (hE 1, the difference 1, their product 1, forming dvdc 1, * dvdc 1); up to 7
         additions, the first onto 0.0 exact: 6; * invArea 2 (forming it, the product); / ph 1.  5 + 6 + 3 = 14, + 5 = 19.
  C_TB   one element of T given L: the biharmonic term is 8 deep like the harmonic one (hE 1, kappa4 * hE 1, the difference 1, * 1, dvdc
         1, * dvdc 1, * invArea 2); the accumulator takes up to 21 additions (7 slots, three terms each), the first exact: 20.
         8 + 20 = 28, + 5 = 33.  Checked against tendency_ld with the LONG-DOUBLE L and mL = |L|; the double L the twin used is off that
         one by <= C_LAP 2^-53 ML (ML the magnitude lap_ld returns), and this error passes through the term linearly:
             |T - T_ref| <= 2^-53 (C_TB M + C_LAP Mp),     Mp = `bih_magnitude` of ML = div-magnitude of kappa4 hE (ML[c1] + ML[c2]) / dc.
  C_TBF  one element of T from phi alone, against magnitudes that carry ML for L (M_full >= M, and Mp is its biharmonic part): the
         longest chain runs through L: 14, then the difference 1, * 1, * dvdc 1, * invArea 2, the accumulator 20: 39, + 5 = 44.
  C_RB   one element of R given M: the biharmonic term is 6 deep like the harmonic one (hE 1, kappa4 * hE 1, dvdc 1, * dvdc 1, the
         difference 1, the product 1), the accumulator 20: 26, + 5 = 31; M's own error enters as above with C_LAP.
  C_STEP_B  the step-level identity <X, M d> = <M^T X, d> per recorded step (tracer_adjoint_twin.py's count with the deeper chains).
         forward: Qc 1; four tendencies of 39: 156; three provisional tracers 9; the last b * t 1 and the four additions of Qn 4;
                  / hn 1:  172
         reverse: g 1; the first y 3; three times R through M (14, the difference 1, the product 1, the accumulator 20: 36), v 1, the
                  next y 4: 123; the last R 36 and the final addition 1:  164
         C_STEP_B = 336, on sum |X| W with W = `forward_magnitude`: tendency_ld's magnitudes with mL = ML through the RK4 recipe.
  C_STEP_BSRC  the source identity <X, phi_N(q) - phi_N(0)> = <G, q>: tracer_source_twin.py's count with these chains -- forward 172 with
         each tendency one addition deeper: 176, two runs: 352; reverse 164 and the four additions of G: 168.  C_STEP_BSRC = 520.
  Content: tracer_diffusion_twin.py's bound with C_TBF for C_TD and M_full for M."""
import numpy as np

import tracer_adjoint_twin as ta
import tracer_cases as tc
import tracer_source_twin as ts
import trisk_reference as tr
from del4_twin import TwinState

LD = tr.LD
SLACK = tr.C_H - 11
C_LAP = 14 + SLACK
C_TB = 28 + SLACK
C_TBF = 39 + SLACK
C_RB = 26 + SLACK
C_STEP_B = 172 + 164
C_STEP_BSRC = 2 * 176 + 164 + 4
assert (C_LAP, C_TB, C_TBF, C_RB, C_STEP_B, C_STEP_BSRC) == (19, 33, 44, 31, 336, 520)

# kappa4_j dt / dcEdge_min^4 of up to nine tracers: pairwise distinct, all <= 0.002, one exact zero (the third: tracer_cases.kappas has
# its zero in the second place, so the first three tracers carry both terms, the biharmonic one alone and the harmonic one alone)
K4FACT9 = (0.002, 0.0015, 0.0, 0.0011, 0.0017, 0.0004, 0.0008, 0.0013, 0.0019)


def kappa4s(meshname, n, factors=K4FACT9):
    """n pairwise distinct biharmonic coefficients, exactly one of them 0.0 when n >= 3."""
    dcmin = float(tc.get_mesh(meshname).dcEdge.min())
    k = [f * dcmin ** 4 / tc.dt_of(meshname) for f in factors[:n]]
    assert len(set(k)) == n and (n < 3 or k.count(0.0) == 1) and max(factors) <= 0.002
    return k


# ---- long double ------------------------------------------------------------------------------------------------------------------
def lap_ld(mesh, ph, x, mlt):
    """(Lap, ML) in long double: div(where(active, hE (x[c2] - x[c1]) / dc, 0)) / h."""
    g = tr.geometry(mesh)
    K = np.asarray(ph).shape[1]
    h, p = tr._ld(ph, (g.nC, K)), tr._ld(x, (g.nC, K))
    act = tr.active(g, mlt, K)
    flux = np.where(act, ((h[g.c1] + h[g.c2]) / 2) * (p[g.c2] - p[g.c1]) / g.dc[:, None], 0)
    mflux = np.where(act, ((np.abs(h[g.c1]) + np.abs(h[g.c2])) / 2) * (np.abs(p[g.c2]) + np.abs(p[g.c1])) / g.dc[:, None], 0)
    d, md = tr.divergence(g, flux, mflux)
    return d / h, md / np.abs(h)


def tendency_ld(mesh, pu, ph, pphi, mlt, kappa, kappa4, L, mL, want_m=True):
    """(T, M) in long double from the edge-flux formula; L (long double) and the magnitude mL to carry for it are inputs."""
    g = tr.geometry(mesh)
    K = np.asarray(pu).shape[1]
    u, h, p = tr._ld(pu, (g.nE, K)), tr._ld(ph, (g.nC, K)), tr._ld(pphi, (g.nC, K))
    kap, kap4 = LD(float(kappa)), LD(float(kappa4))
    act = tr.active(g, mlt, K)
    hE = (h[g.c1] + h[g.c2]) / 2
    dc = g.dc[:, None]
    X = np.where(act, u * hE * ((p[g.c1] + p[g.c2]) / 2) - kap * hE * (p[g.c2] - p[g.c1]) / dc + kap4 * hE * (L[g.c2] - L[g.c1]) / dc, 0)
    mX = None
    if want_m:
        mhE = (np.abs(h[g.c1]) + np.abs(h[g.c2])) / 2
        mp = np.abs(p[g.c1]) + np.abs(p[g.c2])
        mX = np.where(act, np.abs(u) * mhE * (mp / 2) + kap * mhE * mp / dc + kap4 * mhE * (mL[g.c1] + mL[g.c2]) / dc, 0)
    t, mt = tr.divergence(g, X, mX)
    return -t, mt


def bih_magnitude(mesh, ph, mL, mlt, kappa4):
    """The div-magnitude of kappa4 hE (mL[c1] + mL[c2]) / dc: what an error of size mL in L does to T."""
    g = tr.geometry(mesh)
    K = np.asarray(ph).shape[1]
    h = tr._ld(ph, (g.nC, K))
    act = tr.active(g, mlt, K)
    mX = np.where(act, LD(float(kappa4)) * ((np.abs(h[g.c1]) + np.abs(h[g.c2])) / 2) * (mL[g.c1] + mL[g.c2]) / g.dc[:, None], 0)
    return tr.divergence(g, mX, mX)[1]


def tendency_full_ld(mesh, pu, ph, pphi, mlt, kappa, kappa4, want_m=True):
    """(T, M_full) from phi alone: L = lap_ld, carried with its magnitude ML."""
    L, mL = lap_ld(mesh, ph, pphi, mlt)
    return tendency_ld(mesh, pu, ph, pphi, mlt, kappa, kappa4, L, mL, want_m)


def dissipation_ld(mesh, ph, L, kappa4):
    """-kappa4 sum_c A_c sum_k h L^2 in long double: <= 0 by construction."""
    a = np.asarray(mesh.areaCell, dtype=np.float64).astype(LD)
    h = np.asarray(ph, dtype=np.float64).astype(LD)
    return -LD(float(kappa4)) * (a * (h * L * L).sum(axis=1)).sum()


def step_ld(mesh, mlt, rec, phi, kappa, kappa4, q):
    """phi_new of one recorded step in long double (tracer_source_twin.step_ld with the biharmonic term)."""
    dt = LD(rec["dt"])
    a = (dt / 2, dt / 2, dt)
    b = (dt / 6, dt / 3, dt / 3, dt / 6)
    h = [np.asarray(p[1], dtype=np.float64).astype(LD) for p in rec["P"]]
    p = np.asarray(phi).astype(LD) if np.asarray(phi).dtype != LD else np.asarray(phi)
    Qc = p * h[0]
    Qn = Qc.copy()
    for s in range(4):
        t = tendency_full_ld(mesh, rec["P"][s][0], rec["P"][s][1], p, mlt, kappa, kappa4, want_m=False)[0]
        if q is not None:
            t = t + np.asarray(q, dtype=np.float64).astype(LD)
        if s < 3:
            p = (Qc + a[s] * t) / h[s + 1]
        Qn = Qn + b[s] * t
    return Qn / np.asarray(rec["hn"], dtype=np.float64).astype(LD)


def forward_magnitude(mesh, mlt, rec, absd, kappa, kappa4, absq=None):
    """W: the magnitude evaluation of one recorded forward step on the nonnegative field `absd` (source magnitude absq, or None)."""
    dt = LD(rec["dt"])
    a = (dt / 2, dt / 2, dt)
    b = (dt / 6, dt / 3, dt / 3, dt / 6)
    h = [np.abs(np.asarray(p[1], dtype=np.float64).astype(LD)) for p in rec["P"]]
    Qc = np.asarray(absd, dtype=LD) * h[0]
    Qn = Qc.copy()
    p = np.asarray(absd, dtype=LD)
    for s in range(4):
        m = tendency_full_ld(mesh, rec["P"][s][0], rec["P"][s][1], p, mlt, kappa, kappa4)[1]
        if absq is not None:
            m = m + np.asarray(absq, dtype=np.float64).astype(LD)
        if s < 3:
            p = (Qc + a[s] * m) / h[s + 1]
        Qn = Qn + b[s] * m
    return Qn / np.abs(np.asarray(rec["hn"], dtype=np.float64).astype(LD))


def forward_matrices_ld(mesh, pu, ph, mlt, kappa, kappa4):
    """tracer_adjoint_twin.forward_matrices_ld with the biharmonic term: (T, M), (K, nC, nC), column j = the tendency of cell j's unit field."""
    nC, K = np.asarray(ph).shape
    T = np.zeros((K, nC, nC), dtype=LD)
    M = np.zeros((K, nC, nC), dtype=LD)
    for j in range(nC):
        e = np.zeros((nC, K))
        e[j, :] = 1.0
        t, m = tendency_full_ld(mesh, pu, ph, e, mlt, kappa, kappa4)
        T[:, :, j] = t.T
        M[:, :, j] = m.T
    return T, M


# ---- the twins --------------------------------------------------------------------------------------------------------------------
class TracerBiharmonicTwin(ts.SourceTwin):
    """SourceTwin with one biharmonic coefficient per tracer: `kappa4` is a sequence like `kappa` and may be replaced between steps.
    The records gain "kappa4"."""

    def __init__(self, om, base, kappa, source=(), kappa4=()):
        super().__init__(om, base, kappa, source)
        self.kappa4 = [float(k) for k in kappa4]

    def kappa4_of(self, j):
        return self.kappa4[j] if j < len(self.kappa4) else 0.0

    def lap(self, ph, x):
        s = np.zeros_like(ph)
        for i in range(self.eoc.shape[1]):
            n = self.coc[:, i]
            hE = 0.5 * (ph + ph[n])
            s = np.where(self.slot_mask(i), s + (hE * (x[n] - x)) * self.dvdc[:, i, None], s)
        return (s * self.invArea[:, None]) / ph

    def tendency_bih(self, pu, ph, pphi, kappa, kappa4, L):
        T = np.zeros_like(ph)
        kappa, kappa4 = np.float64(kappa), np.float64(kappa4)
        for i in range(self.eoc.shape[1]):
            n = self.coc[:, i]
            hE = 0.5 * (ph + ph[n])
            F = pu[self.eoc[:, i]] * hE
            pE = self.edge_value(pphi, i)
            m = self.slot_mask(i)
            T = np.where(m, T + ((F * pE) * self.sdv[:, i, None]) * self.invArea[:, None], T)
            G = pphi[n] - pphi
            T = np.where(m, T + ((((kappa * hE) * G) * self.dvdc[:, i, None]) * self.invArea[:, None]), T)
            T = np.where(m, T - ((((kappa4 * hE) * (L[n] - L)) * self.dvdc[:, i, None]) * self.invArea[:, None]), T)
        return T

    def step_rk4(self, st, phis, dt, magnitudes=False):
        """SourceTwin.step_rk4 line by line with L = lap(ph_s, pphi) and tendency_bih for every tracer while any kappa4 is nonzero."""
        n = len(phis[1])
        k4 = [self.kappa4_of(j) for j in range(n)]
        if not any(k != 0.0 for k in k4):
            super().step_rk4(st, phis, dt, magnitudes)
            self.tape[-1]["kappa4"] = k4
            return
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
        assert len(self.kappa) >= n
        mesh = self.om.mesh
        bM = [np.zeros(ch.shape, dtype=LD) for _ in Qc] if magnitudes else None
        for s in range(4):
            tu, th = self.dycore(pu, ph)
            tend = []
            for j in range(n):
                T = self.tendency_bih(pu, ph, pphi[j], self.kappa[j], k4[j], self.lap(ph, pphi[j]))
                q = self.source_of(j)
                tend.append(T if q is None else T + q)
            if magnitudes:
                for j in range(n):
                    m = tendency_full_ld(mesh, pu, ph, pphi[j], self.mlt, self.kappa[j], k4[j])[1]
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
        self.tape.append({"P": self._P, "hn": st.h[1].copy(), "kappa": [float(k) for k in self.kappa[:n]], "kappa4": k4, "dt": dt})
        self._P = None


def content_bound(mesh, absQc, bM):
    """tracer_diffusion_twin.content_bound with C_TBF for C_TD, from the magnitudes TracerBiharmonicTwin.step_rk4(magnitudes=True) leaves."""
    a = np.asarray(mesh.areaCell, dtype=np.float64).astype(LD)
    return tr.U53 * (a * (12 * (absQc + bM) + (C_TBF + 2) * bM).sum(axis=1)).sum()


class BiharmonicAdjointTwin(ts.SourceAdjointTwin):
    """SourceAdjointTwin whose R carries the M term; `tw` must have lap (a TracerBiharmonicTwin)."""

    def R_bih(self, pu, ph, y, kappa, kappa4):
        tw = self.tw
        M = tw.lap(ph, y)
        r = np.zeros_like(ph)
        kappa, kappa4 = np.float64(kappa), np.float64(kappa4)
        for i in range(tw.eoc.shape[1]):
            n = tw.coc[:, i]
            hE = 0.5 * (ph + ph[n])
            F = pu[tw.eoc[:, i]] * hE
            m = tw.slot_mask(i)
            r = np.where(m, r + ((0.5 * F) * tw.sdv[:, i, None]) * (y - y[n]), r)
            r = np.where(m, r + ((kappa * hE) * tw.dvdc[:, i, None]) * (y[n] - y), r)
            r = np.where(m, r - ((kappa4 * hE) * tw.dvdc[:, i, None]) * (M[n] - M), r)
        return r

    def reverse_step_bih(self, rec, X, G=None):
        """SourceAdjointTwin.reverse_step with R_bih and the record's kappa4."""
        dt = rec["dt"]
        a = (dt / 2., dt / 2., dt)
        b = (dt / 6., dt / 3., dt / 3., dt / 6.)
        invA = self.tw.invArea[:, None]
        out = []
        for j, x in enumerate(X):
            kap, kap4 = rec["kappa"][j], rec["kappa4"][j]
            Gj = None if G is None else G[j]
            g = x / rec["hn"]
            tau = b[3] * g
            y = tau * invA
            if Gj is not None:
                Gj += tau
            S = None
            for s in (3, 2, 1):
                pu, ph = rec["P"][s]
                r = self.R_bih(pu, ph, y, kap, kap4)
                v = r / ph
                S = v if s == 3 else S + v
                tau = b[s - 1] * g + a[s - 1] * v
                y = tau * invA
                if Gj is not None:
                    Gj += tau
            pu, ph = rec["P"][0]
            r = self.R_bih(pu, ph, y, kap, kap4)
            out.append(ph * (g + S) + r)
        return out

    def sweep(self, tape, X, want=()):
        """Reverse over every record, last first; (X, G) as SourceAdjointTwin.sweep.  The biharmonic instances run when any recorded kappa4
        is nonzero, else the parent's sweep."""
        if not any(k != 0.0 for rec in tape for k in rec.get("kappa4", ())):
            return super().sweep(tape, X, want)
        G = [np.zeros_like(x) if j in want else None for j, x in enumerate(X)]
        for rec in reversed(tape):
            X = self.reverse_step_bih(rec, X, G)
        return X, G


# ---- shared cases -----------------------------------------------------------------------------------------------------------------
_REFS = {}


def biharmonic_twin(meshname, K, mode="linear", partial=False):
    t = tc.twin_of(meshname, K, mode, partial)
    return TracerBiharmonicTwin(t.om, t.base, [])


def reference(meshname, K, mode, partial, nT, segments, srcs=(), wants=(), pre=0):
    """Computed once per case and shared (never modified by a test).  The first nT of tc.distinct_fields(mesh, K, 9) over tc.state_of's
    state; segments = ((nsteps, diff, bih),
    ...): nsteps recorded RK4 steps with tc.kappas(meshname, 9)[:nT] if diff (else zeros) and kappa4s(meshname, 9)[:nT] if bih (else
    zeros); bih may also be a tuple of factors of kappa4s' values, one per tracer.  Sources tracer_source_twin.source_fields(...)[j] for j
    in srcs.  pre: tracer-free steps of the dycore ahead of all that (tracers set late; not recorded).  Then the reverse sweep of ta.seeds(mesh, K, 9)[:nT] with the source gradients of `wants`.  A dict: twin, fields, sources,
    forward = tc.reference's tuple per step, X, grad, G, kappa / kappa4 = the values of each segment."""
    key = (meshname, K, mode, partial, nT, tuple(segments), tuple(srcs), tuple(wants), pre)
    if key not in _REFS:
        mesh = tc.get_mesh(meshname)
        twin = biharmonic_twin(meshname, K, mode, partial)
        q = ts.source_fields(meshname, K, 9)
        twin.source = [q[j] if j in srcs else None for j in range(nT)]
        ssh, u, h, _ = tc.state_of(meshname, K)
        st = TwinState(ssh, u, h)
        for _ in range(pre):
            twin.step_rk4(st, [[], []], tc.dt_of(meshname))
        twin.tape.clear()
        f = tc.distinct_fields(mesh, K, 9)[:nT]
        phis = [[a.copy() for a in f], [a.copy() for a in f]]
        fwd, kaps, kap4s = [], [], []
        for nsteps, diff, bih in segments:
            twin.kappa = tc.kappas(meshname, 9)[:nT] if diff else [0.0] * nT
            k4 = kappa4s(meshname, 9)[:nT]
            twin.kappa4 = ([c * k for c, k in zip(bih, k4)] if isinstance(bih, tuple) else k4) if bih else [0.0] * nT
            kaps.append(list(twin.kappa))
            kap4s.append(list(twin.kappa4))
            for _ in range(nsteps):
                twin.step_rk4(st, phis, tc.dt_of(meshname))
                fwd.append(([a.copy() for a in phis[0]], [a.copy() for a in phis[1]], st.u[1].copy(), st.h[1].copy(), st.ssh[1].copy()))
        X = ta.seeds(mesh, K, 9)[:nT]
        grad, G = BiharmonicAdjointTwin(twin).sweep(twin.tape, [x.copy() for x in X], tuple(wants))
        _REFS[key] = {"twin": twin, "fields": f, "sources": list(twin.source), "forward": fwd, "X": X, "grad": grad, "G": G,
                      "kappa": kaps, "kappa4": kap4s}
    return _REFS[key]


# ---- the plane wave (tracer_cases.py's mode; the hexagon Laplacian's eigenvalue lam enters the biharmonic term as -kappa4 lam^2) ----
EIG_KAPPA4 = 0.002 * tc.EIG_DC ** 4 / tc.EIG_DT


def eigenmode_z(kappa, kappa4):
    """z = (mu + kappa lam - kappa4 lam^2) dt, written out from the six neighbour vectors (nothing shared with tc.eigenmode_z)."""
    kx, ky = tc.EIG_K
    dc = tc.EIG_DC
    mu, lam = 0j, 0.0
    for m in range(6):
        c, s = np.cos(m * np.pi / 3), np.sin(m * np.pi / 3)
        kd = (kx * c + ky * s) * dc
        mu = mu - (tc.EIG_U[0] * c + tc.EIG_U[1] * s) * np.exp(1j * kd) / (3 * dc)
        lam = lam + (2 / (3 * dc * dc)) * (np.cos(kd) - 1)
    return (mu + kappa * lam - kappa4 * lam * lam) * tc.EIG_DT


def _poly(z, order=4):
    return sum(z ** i / float(np.prod(np.arange(1, i + 1))) for i in range(order + 1))


def plane_wave_check(phi, mesh, K, kappa, kappa4, phi0, label, backwards=False):
    """|phi - (1 + 0.5 Re(f^n e^{ikx}))| <= n * 32 * 2^-53 * max|phi0| with f = R4(z) forwards, conj(R4(z)) backwards; the same tolerance
    refuses kappa4 = 0, the wrong sign of the term, and a third-order stage loop.  Prints every figure; returns the deviation."""
    n = tc.EIG_STEPS
    cj = np.conj if backwards else (lambda v: v)
    tol = n * 32 * 2.0 ** -53 * float(np.abs(phi0).max())
    gap = lambda f: float(np.abs(phi - tc.eigenmode_expect(mesh, K, f)).max())      # noqa: E731
    z = eigenmode_z(kappa, kappa4)
    dev = gap(cj(_poly(z)) ** n)
    gap0 = gap(cj(_poly(eigenmode_z(kappa, 0.0))) ** n)
    gapm = gap(cj(_poly(eigenmode_z(kappa, -kappa4))) ** n)
    gap3 = gap(cj(_poly(z, 3)) ** n)
    print(f"{label}: z = {z:.6g}, max deviation = {dev:.3e}, tolerance = {tol:.3e}, gap to kappa4 = 0: {gap0:.3e}, to the wrong sign: "
          f"{gapm:.3e}, to third order: {gap3:.3e}")
    assert dev <= tol
    assert gap0 > tol and gapm > tol and gap3 > tol
    if backwards:
        assert gap(_poly(z) ** n) > tol          # the forward factor
    return dev
