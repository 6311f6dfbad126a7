"""Numpy twin of the passive tracer transport beside the RK4 step (moka_set_tracers), and a long-double restatement of its tendency.

Scheme (include/moka_hip.h): conservative flux form d(h phi)/dt = -div(F phi_e), F = u * h_e the thickness flux of the thickness
equation, phi_e the centred edge value.  For a provisional state (pu, ph, pphi), cell c, level k (0-based) the tendency T accumulates
from 0.0 over the slots i of edgesOnCell in slot order; empty slots and slots with k >= maxLevelEdgeTop[e] are skipped:
    hE = 0.5 * (ph[k,c] + ph[k,c'])        c' = the cell across slot i
    F  = pu[k,e] * hE
    pE = 0.5 * (pphi[k,c] + pphi[k,c'])
    T += ((F * pE) * sdv[c,i]) * invArea[c]        sdv = dvEdge[e] * edgeSignOnCell[i,c] (exact), invArea = 1 / areaCell
-- oracle_layer_thickness_tendency with F * pE for F: with pphi == 1, pE is exactly 1 and T is tendLayerThickness bit for bit.
`TracerTwin.tendency` is that loop in double, one slot at a time over all cells (the library's bits); `step_rk4` restates the stage
loop of Del4Twin.step_rk4 with the tracer recipe beside it:
    Qc = phi_cur * h_cur;  Qn = Qc;  pphi = phi_cur
    s = 0..3:  t = T(pu_s, ph_s, pphi);  s < 3: pphi = (Qc + a[s] * t) / ph_{s+1};  Qn = Qn + b[s] * t
    phi_new = Qn / h_new

`tendency_ld` is T from the formula in np.longdouble, written like tests/trisk_reference.py's thickness_tendency (whose helpers it
uses: the divergence over fancy-indexed gathers), with that file's magnitude evaluation: every leaf and intermediate replaced by a
bound, differences summed.  Round-off chain of one element of T in the library's order (one rounding per +, *, and for forming
1/areaCell; 0.5 and the signs are exact): hE 1, F 1, pE 1 (beside hE: it adds its own relative error to the product), F * pE 1,
* sdv 1, * (1/A) 2, the sum over <= 7 slots 6: 13 -- the thickness tendency's 11 plus one addition and one multiplication.
trisk_reference.py carries its tendH count of 11 as C_H = 16; the tracer bound keeps the same slack: C_T = C_H + 2 = 18, and each
element is checked as |T - T_ref| <= C_T 2^-53 M.

Content.  S = sum_c A_c sum_k phi h is conserved by the scheme up to round-off, also with partial maxLevelEdgeTop: every active (e, k)
contributes A_c1 (X sdv_1 invA_1) + A_c2 (X sdv_2 invA_2) with sdv_2 = -sdv_1 and A invA = 1 + O(2^-53), each b[s]-weighted.  Per
step the double-precision path from Qc to phi_new h_new rounds: Qc 1, per stage b*t 1 and the addition 1 (8), the division 1, the
product phi_new * h_new taken by the check 1 -- 11 roundings on magnitudes <= |Qc| + sum_s b[s] M_s, with M_s the magnitude of T at
stage s -- and T itself is off its exact value by <= C_T 2^-53 M_s; A_c * invArea_c deviates from 1 by 2 roundings.  Hence
    |S_new - S_old| <= 2^-53 sum_c A_c sum_k (12 (|Qc| + sum_s b[s] M_s) + (C_T + 2) sum_s b[s] M_s)
(12 = the 11 above + 1 for the check's own product phi_cur * h_cur), which `content_bound` evaluates in long double."""
import numpy as np

import trisk_reference as tr

LD = tr.LD
C_T = tr.C_H + 2


def tendency_ld(mesh, pu, ph, pphi, mlt, want_m=True):
    """(T, M) in long double from the formula: T = -div(where(active, u hE pE, 0)) with the centred hE and pE."""
    g = tr.geometry(mesh)
    K = np.asarray(pu).shape[1]
    u, h, p = tr._ld(pu, (g.nE, K)), tr._ld(ph, (g.nC, K)), tr._ld(pphi, (g.nC, K))
    act = tr.active(g, mlt, K)
    X = np.where(act, u * ((h[g.c1] + h[g.c2]) / 2) * ((p[g.c1] + p[g.c2]) / 2), 0)
    mX = None
    if want_m:
        mX = np.where(act, np.abs(u) * ((np.abs(h[g.c1]) + np.abs(h[g.c2])) / 2) * ((np.abs(p[g.c1]) + np.abs(p[g.c2])) / 2), 0)
    t, mt = tr.divergence(g, X, mX)
    return -t, mt


def content(mesh, phi, h):
    """sum_c A_c sum_k phi h in long double."""
    a = np.asarray(mesh.areaCell, dtype=np.float64).astype(LD)
    return (a * (np.asarray(phi).astype(LD) * np.asarray(h).astype(LD)).sum(axis=1)).sum()


class TracerTwin:
    """om: the OracleMesh; base: what drives the dycore -- an object with tendencies(u, h) -> (tendU, tendH, ssh, ...)
    (OracleNonlinear, Del4Twin), or the OracleMesh itself for the linear terms (its tendencies_clean)."""

    def __init__(self, om, base):
        m = om.mesh
        self.om, self.base = om, base
        self.K = om.K
        self.mlt = np.asarray(om.arrays["maxLevelEdgeTop"])
        ME = m.edgesOnCell.shape[1]
        self.valid = np.arange(ME)[None, :] < np.asarray(m.nEdgesOnCell)[:, None]
        self.eoc = np.where(self.valid, np.asarray(m.edgesOnCell, dtype=np.int64) - 1, 0)
        c1, c2 = np.asarray(m.cellsOnEdge[:, 0], dtype=np.int64) - 1, np.asarray(m.cellsOnEdge[:, 1], dtype=np.int64) - 1
        own = np.arange(m.nCells)[:, None]
        self.coc = np.where(c1[self.eoc] == own, c2[self.eoc], c1[self.eoc])
        self.sdv = np.asarray(m.dvEdge, dtype=np.float64)[self.eoc] * np.asarray(m.edgeSignOnCell)[:, :ME].astype(np.float64)
        self.invArea = 1.0 / np.asarray(m.areaCell, dtype=np.float64)
        self.last_M = None

    def dycore(self, u, h):
        t = self.base.tendencies_clean(u, h) if hasattr(self.base, "tendencies_clean") else self.base.tendencies(u, h)
        return t[0], t[1]

    def slot_mask(self, i):
        """(nCells, K): slot i exists and its edge is active on the level."""
        return self.valid[:, i, None] & (np.arange(self.K)[None, :] < self.mlt[self.eoc[:, i]][:, None])

    def edge_value(self, pphi, i):
        return 0.5 * (pphi + pphi[self.coc[:, i]])

    def tendency(self, pu, ph, pphi):
        T = np.zeros_like(ph)
        for i in range(self.eoc.shape[1]):
            hE = 0.5 * (ph + ph[self.coc[:, i]])
            F = pu[self.eoc[:, i]] * hE
            pE = self.edge_value(pphi, i)
            T = np.where(self.slot_mask(i), T + ((F * pE) * self.sdv[:, i, None]) * self.invArea[:, None], T)
        return T

    def step_rk4(self, st, phis, dt, magnitudes=False):
        """One RK4 step of the dycore state `st` (a del4_twin.TwinState) and of the tracers `phis` = [previous, current], each a
        list of (nCells, K) arrays; both rotate.  magnitudes=True also leaves in self.last_M, per tracer, (|Qc|, sum_s b[s] M_s) in
        long double for content_bound."""
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
        mesh = self.om.mesh
        bM = [np.zeros(ch.shape, dtype=LD) for _ in Qc] if magnitudes else None
        for s in range(4):
            tu, th = self.dycore(pu, ph)
            tt = [self.tendency(pu, ph, p) for p in pphi]
            if magnitudes:
                for j, p in enumerate(pphi):
                    bM[j] += LD(b[s]) * tendency_ld(mesh, pu, ph, p, self.mlt)[1]
            if s < 3:
                pu, ph = cu + a[s] * tu, ch + a[s] * th
                pphi = [(Qc[j] + a[s] * tt[j]) / ph for j in range(len(Qc))]
            newU, newH = newU + b[s] * tu, newH + b[s] * th
            Qn = [Qn[j] + b[s] * tt[j] for j in range(len(Qc))]
        st.tendU, st.tendH = tu, th
        st.u[1], st.h[1] = newU, newH
        st.ssh[1] = self.om.update_ssh(newH)
        phis[1] = [Qn[j] / newH for j in range(len(Qc))]
        if magnitudes:
            self.last_M = [(np.abs(Qc[j]).astype(LD), bM[j]) for j in range(len(Qc))]


def content_bound(mesh, absQc, bM):
    """The docstring's bound on |S_new - S_old| of one step from the magnitudes TracerTwin.step_rk4(magnitudes=True) leaves."""
    a = np.asarray(mesh.areaCell, dtype=np.float64).astype(LD)
    return tr.U53 * (a * (12 * (absQc + bM) + (C_T + 2) * bM).sum(axis=1)).sum()
