"""Numpy twin of passive tracer transport with harmonic diffusion (moka_set_tracer_diffusion), and a long-double restatement of its
tendency.  Extends tests/tracer_twin.py, whose docstring states the transport part and the RK4 recipe (untouched here).

Scheme (include/moka_hip.h): d(h phi)/dt = -div(F phi_e) + div(kappa_j h_e grad phi), kappa_j >= 0 per tracer.  Per cell c, level k
and slot i of edgesOnCell (empty slots and slots with k >= maxLevelEdgeTop[e] skipped for both terms), after the advective addition
    hE = 0.5 * (ph[k,c] + ph[k,c']);  F = pu[k,e] * hE;  pE = 0.5 * (pphi[k,c] + pphi[k,c']);  T += ((F * pE) * sdv[c,i]) * invArea[c]
of that slot a second, separate addition follows:
    G  = pphi[k,c'] - pphi[k,c]
    T += ((((kappa_j * hE) * G) * dvdc[c,i]) * invArea[c])        dvdc[c,i] = dvEdge[e] / dcEdge[e]   (one double division)
`TracerDiffusionTwin.tendency` is that loop in double, one slot at a time over all cells (the library's bits).  With kappa_j == 0 the
second addition adds +-0.0 to a T that is never -0.0 (it starts at +0.0; x + (-x) = +0.0 under round-to-nearest): the bits are
TracerTwin.tendency's.  A constant tracer has G == 0 exactly.

`tendency_ld` is T from the formula in np.longdouble: the edge flux
    X = u hE pE - kappa hE (phi[c2] - phi[c1]) / dcEdge         where (e, k) is active, else 0
and T = -div(X) with tests/trisk_reference.py's divergence; magnitudes as there, the difference carried as |phi[c1]| + |phi[c2]|.

Round-off chain of one element of T in the library's order (one rounding per +, -, *, /, including forming 1/areaCell and dvdc; 0.5
and the signs are exact).  An advective term is 7 deep (tracer_twin.py: hE 1, F 1, pE 1, F * pE 1, * sdv 1, * (1/A) 2); a diffusive
term is 8 deep: hE 1, kappa * hE 1, G 1 (on |phi_c| + |phi_c'|, which the magnitude carries), * G 1, dvdc 1, * dvdc 1, * (1/A) 2.  The
accumulator now takes up to 14 additions (7 slots, two terms each), the first onto 0.0 exact: 13.  Longest chain 8 + 13 = 21, against
13 without diffusion.  trisk_reference.py carries its tendH count of 11 as C_H = 16; the same slack of 5 gives
    C_TD = 21 + 5 = 26,
and each element is checked as |T - T_ref| <= C_TD 2^-53 M with M the magnitude of both terms.

Content.  S = sum_c A_c sum_k phi h stays conserved up to round-off: per active (e, k) the diffusive product ((kappa hE) G) dvdc is, like
the advective (F pE) sdv, the exact negative in the second cell of the edge of what it is in the first (hE and dvdc are symmetric, G
changes its sign exactly), and each is then weighted by A_c invArea_c = 1 + O(2 * 2^-53).  tracer_twin.py's derivation holds with C_TD
for C_T and with M_s the magnitude of both terms:
    |S_new - S_old| <= 2^-53 sum_c A_c sum_k (12 (|Qc| + sum_s b[s] M_s) + (C_TD + 2) sum_s b[s] M_s),
which `content_bound` evaluates in long double from the magnitudes `step_rk4(magnitudes=True)` leaves."""
import numpy as np

import tracer_twin as tt
import trisk_reference as tr

LD = tr.LD
C_TD = 21 + (tr.C_H - 11)
assert C_TD == 26


def tendency_ld(mesh, pu, ph, pphi, mlt, kappa, want_m=True):
    """(T, M) in long double from the formula: T = -div(where(active, u hE pE - kappa hE (phi[c2] - phi[c1]) / dc, 0))."""
    g = tr.geometry(mesh)
    K = np.asarray(pu).shape[1]
    u, h, p = tr._ld(pu, (g.nE, K)), tr._ld(ph, (g.nC, K)), tr._ld(pphi, (g.nC, K))
    kap = LD(float(kappa))
    act = tr.active(g, mlt, K)
    hE = (h[g.c1] + h[g.c2]) / 2
    X = np.where(act, u * hE * ((p[g.c1] + p[g.c2]) / 2) - kap * hE * (p[g.c2] - p[g.c1]) / g.dc[:, None], 0)
    mX = None
    if want_m:
        mhE = (np.abs(h[g.c1]) + np.abs(h[g.c2])) / 2
        mp = np.abs(p[g.c1]) + np.abs(p[g.c2])
        mX = np.where(act, np.abs(u) * mhE * (mp / 2) + kap * mhE * mp / g.dc[:, None], 0)
    t, mt = tr.divergence(g, X, mX)
    return -t, mt


def dissipation_ld(mesh, ph, pphi, mlt, kappa):
    """-sum over the active (e, k) of kappa hE (dv / dc) (phi[c2] - phi[c1])^2 in long double: <= 0 by construction."""
    g = tr.geometry(mesh)
    K = np.asarray(ph).shape[1]
    h, p = tr._ld(ph, (g.nC, K)), tr._ld(pphi, (g.nC, K))
    act = tr.active(g, mlt, K)
    hE = (h[g.c1] + h[g.c2]) / 2
    d = p[g.c2] - p[g.c1]
    return -np.where(act, LD(float(kappa)) * hE * (g.dv / g.dc)[:, None] * d * d, 0).sum()


class TracerDiffusionTwin(tt.TracerTwin):
    """TracerTwin with one diffusivity per tracer: `kappa` is a sequence (tracer j of step_rk4's lists takes kappa[j]) and may be
    replaced between steps."""

    def __init__(self, om, base, kappa):
        super().__init__(om, base)
        m = om.mesh
        self.kappa = [float(k) for k in kappa]
        self.dvdc = np.asarray(m.dvEdge, dtype=np.float64)[self.eoc] / np.asarray(m.dcEdge, dtype=np.float64)[self.eoc]

    def tendency(self, pu, ph, pphi, kappa=0.0):
        T = np.zeros_like(ph)
        kappa = np.float64(kappa)
        for i in range(self.eoc.shape[1]):
            hE = 0.5 * (ph + ph[self.coc[:, i]])
            F = pu[self.eoc[:, i]] * hE
            pE = self.edge_value(pphi, i)
            m = self.slot_mask(i)
            T = np.where(m, T + ((F * pE) * self.sdv[:, i, None]) * self.invArea[:, None], T)
            G = pphi[self.coc[:, i]] - pphi
            T = np.where(m, T + ((((kappa * hE) * G) * self.dvdc[:, i, None]) * self.invArea[:, None]), T)
        return T

    def step_rk4(self, st, phis, dt, magnitudes=False):
        """TracerTwin.step_rk4 with tracer j's tendency taking self.kappa[j] (the recipe itself is that one's, line by line)."""
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
            tend = [self.tendency(pu, ph, pphi[j], self.kappa[j]) for j in range(n)]
            if magnitudes:
                for j in range(n):
                    bM[j] += LD(b[s]) * tendency_ld(mesh, pu, ph, pphi[j], self.mlt, self.kappa[j])[1]
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


def content_bound(mesh, absQc, bM):
    """The docstring's bound on |S_new - S_old| of one step from the magnitudes TracerDiffusionTwin.step_rk4(magnitudes=True) leaves."""
    a = np.asarray(mesh.areaCell, dtype=np.float64).astype(LD)
    return tr.U53 * (a * (12 * (absQc + bM) + (C_TD + 2) * bM).sum(axis=1)).sum()
