"""Numpy twin of reverse mode through the quadratic bottom drag (moka_forced_tape_create_quadratic; csrc/momentum_vmix.hip: the QD
instances of mvadj_column and k_mvadj_bottom_speed), on top of forced_adjoint_twin.ForcedTwin, momentum_vfield_twin and
quadratic_drag_twin, all untouched, and a long-double restatement of the same transpose.

Recipe (include/moka_hip.h), for a recorded step with Cd != 0 and dt != 0; un, hn the recorded new level, us the recorded u*, sp the
recorded bottom speed, n = n_e = min(maxLevelEdgeTop[e], K), kb_e = n_e - 1, every operation rounded once:
    q_e  = dt * (r + Cd * sp[e])                   quadratic_drag_twin.apply's expression: the forward's bits
    z, hbar, XU = h o z, the cell gather, G_tau, D_nu, D_r, DF     forced_adjoint_twin's / momentum_vfield_twin's recipe with q_e; every
                                                   column with n >= 1 is a computed column (Cd != 0 switches the drag lines on)
    t    = z[n-1] * un[n-1]
    M[e] = (0.0 - (dt * Cd) * t) / sp[e]  where sp[e] > 0, else 0.0        (0.0 for n_e == 0)
    D_cd[e] = D_cd[e] - (dt * t) * sp[e]           when wanted; also in a step with Cd == 0, from an sp recorded for it alone
then `speed_transpose`, per edge e' with n' = n_e' >= 1 and per level k that is kb_e of a slot e of cellsOnEdge[e'] = (c1, c2) with
n_e >= 1 and kb_e < n':
    a_j = 0.0;  over the slots i < nEdgesOnCell[c_j], ascending, with kb_e == k:  a_j = a_j + M[e]
    g   = a_1 * invArea[c1] + a_2 * invArea[c2]
    XU[k,e'] = XU[k,e'] + (kc[e'] * us[k,e']) * g
us[k,e'] is read only where some slot hits level k (0.0 is put in its place before any arithmetic otherwise), M of a slot that fails
the test is not read, rows k >= n' are never touched.  `speed_transpose(depth_test=False)` drops the kb_e < n' test and
`speed_transpose(both_cells=False)` counts the edge e' itself in its first cell only: the two deliberate mistakes.

Long double (`transpose_ld`): for the same inputs, sp = quadratic_drag_twin.speed_ld(us), q = dt (r + Cd sp), (A, A^-1) =
quadratic_drag_twin.dense_ld, z = A^-1 XU, t, M = -dt Cd t / sp, D_cd = -dt t sp, and the chain term scattered from the edges:
C[c,k] = sum over ALL edges e with c in cellsOnEdge[e], n_e >= 1 and kb_e == k of M[e] (np.add.at through cellsOnEdge -- no slot of
edgesOnCell is visited), XU[k,e'] = h[k] z[k] + (dcEdge dvEdge / 4)[e'] us[k,e'] (C[c1,k] / areaCell[c1] + C[c2,k] / areaCell[c2]) for
k < n'.  un, hn, us and XU are data to both sides (h = 0.5 * (hn[c1] + hn[c2]) is the double both take).

Round-off count (`transpose_ld` returns the bounds; first order in 2^-53; m = maxEdges; C_SP, C_Q quadratic_drag_twin.counts):
  z:  the twin solves with its double q^, |q^ - q| <= C_Q 2^-53 q, and z(q^) - z(q) = -(q^ - q) A^-1 e_{n-1} z[n-1]; with
      momentum_vmix_twin's count of the solve,  ez = |A^-1| (C_SOLVE (|A||z^| + |XU|) + C_Q q |z^[n-1]| e_{n-1});
  h o z: one rounding of |h z^| and h ez;
  t = z[n-1] un[n-1]: one rounding, and ez[n-1] |un[n-1]|;
  M:  dt * Cd (1), its product with t (1), the division (1), t's own rounding (1), sp^ against sp (C_SP): C_M = 4 + C_SP on |M^|, and
      dt Cd ez[n-1] |un[n-1]| / sp;
  a_j: the first addition, to 0.0, is exact, at most m - 1 more: m - 1 on sum |M|; invArea and the product with it: 2; the addition
      that forms g: 1; kc: 2 (as quadratic_drag_twin counts it); kc * us: 1; the product with g: 1:
      C_CH = C_M + (m - 1) + 2 + 1 + 2 + 1 + 1 = C_M + m + 6 on kc |us| sum_j invArea_j sum |M^|;
  the addition to XU: one rounding of |XU_new^|;
  D_cd: t (1), dt * t (1), the product with sp (1), sp^ (C_SP), 0.0 - x exact: C_D = 3 + C_SP on |D_cd^|, and dt ez[n-1] |un[n-1]| sp.
Nothing is fitted."""
import numpy as np

import forced_adjoint_twin as fa
import momentum_vfield_twin as mf
import momentum_vmix_twin as mv
import quadratic_drag_twin as qd
import tracer_vmix_twin as tv

LD = tv.LD
U53 = tv.U53
QUADRATIC = 8        # the key of D_cd in the `dens` dictionaries, beside forced_adjoint_twin's STRESS, VISCOSITY, DRAG


# ---- the transpose of the bottom-speed stencil ----------------------------------------------------------------------------------------
def _depths(mlt, nE, K):
    return np.clip(np.asarray(mlt, dtype=np.int64) * np.ones(nE, dtype=np.int64), 0, K)


def speed_transpose(mesh, mlt, XU, us, M, depth_test=True, both_cells=True):
    """XU (nEdges, K) with the chain term of the recipe added: a new array."""
    XU = XU.copy()
    nE, K = XU.shape
    nn = _depths(mlt, nE, K)
    eoc, cnt, kc, inv = qd._stencil(mesh)
    c1, c2 = mv.edge_cells(mesh)
    on, me = nn >= 1, np.arange(nE)
    slots = ([], [])
    for j, c in enumerate((c1, c2)):
        for i in range(eoc.shape[1]):
            valid = on & (i < cnt[c])
            ep = np.where(valid, eoc[c, i], 0)
            ml = nn[ep]
            ok = valid & (ml >= 1)
            if depth_test:
                ok = ok & (ml - 1 < nn)
            if not both_cells and j == 1:
                ok = ok & (ep != me)
            slots[j].append((ok, ml - 1, np.where(ok, M[np.where(ok, ep, 0)], 0.0)))
    for k in range(K):
        a, touched = [], np.zeros(nE, dtype=bool)
        for j in range(2):
            acc = np.zeros(nE)
            for ok, kb, m in slots[j]:
                hit = ok & (kb == k)
                acc = np.where(hit, acc + m, acc)
                touched |= hit
            a.append(acc)
        g = a[0] * inv[c1] + a[1] * inv[c2]
        x = np.where(touched, us[:, k], 0.0)               # an element no slot reaches contributes no operand at all
        XU[:, k] = np.where(touched, np.where(touched, XU[:, k], 0.0) + (kc * x) * g, XU[:, k])
    return XU


def speed_transpose_no_depth_test(mesh, mlt, XU, us, M):
    """The deliberate mistake that drops the kb_e < n_e' test."""
    return speed_transpose(mesh, mlt, XU, us, M, depth_test=False)


def speed_transpose_one_cell(mesh, mlt, XU, us, M):
    """The deliberate mistake that counts the edge e' itself in its first cell only."""
    return speed_transpose(mesh, mlt, XU, us, M, both_cells=False)


def neighbour_levels(mesh, mlt, K):
    """(deeper, shallower): per edge e', whether some slot of its two cells holds an edge with kb_e >= n_e' (the skip test fires) and
    whether some holds one with 0 <= kb_e < n_e' - 1 (a level above e''s own bottom is hit)."""
    nE = mesh.nEdges
    nn = _depths(mlt, nE, K)
    eoc, cnt, _, _ = qd._stencil(mesh)
    deeper, shallower = np.zeros(nE, dtype=bool), np.zeros(nE, dtype=bool)
    for c in mv.edge_cells(mesh):
        for i in range(eoc.shape[1]):
            valid = (nn >= 1) & (i < cnt[c])
            ml = nn[np.where(valid, eoc[c, i], 0)]
            deeper |= valid & (ml >= 1) & (ml - 1 >= nn)
            shallower |= valid & (ml >= 1) & (ml - 1 < nn - 1)
    return deeper, shallower


# ---- one transposed pass ------------------------------------------------------------------------------------------------------------
def transposed_pass(mesh, mlt, XU, XH, un, hn, dt, nu, drag, tau, fld=None, dens=None, DF=None, cd=0.0, sp=None, us=None,
                    chain=speed_transpose, parts=None):
    """momentum_vfield_twin.transposed_pass with the step's Cd, its recorded sp (nEdges; None: not recorded) and u* `us` (needed with
    cd != 0); dens may hold QUADRATIC: D_cd, updated in place when sp is there.  `parts`: a dict that receives M.  Returns (XU, XH)."""
    XU, XH = XU.copy(), XH.copy()
    dens = dens or {}
    qdrag = cd != 0.0
    wcd = QUADRATIC in dens and sp is not None
    grad = any(b in dens for b in (fa.STRESS, fa.VISCOSITY, fa.DRAG)) or DF is not None or wcd
    nE, K = XU.shape
    on = (fld is not None) or mv.pass_on(nu, drag, tau, mlt) or qdrag
    if dt == 0.0 or not (on or grad):
        return XU, XH
    c1, c2 = mv.edge_cells(mesh)
    st = mv.stress_on(tau, mlt)
    nw = fa.computed_depth(mlt, K, (True if (drag != 0.0 or qdrag) else None), st, on)
    nn = _depths(mlt, nE, K) if grad else nw
    hbar = np.full(XU.shape, np.nan)
    M = np.zeros(nE)
    dtcd = np.float64(dt) * np.float64(cd)
    for n in np.unique(nn):
        if n < 1:
            continue
        idx = np.nonzero(nn == n)[0]
        he = 0.5 * (hn[c1[idx], :n] + hn[c2[idx], :n])
        b = np.float64(dt) * np.asarray(tau, dtype=np.float64)[idx] if st else None
        s = np.float64(dt) * fld[idx, :n - 1] if fld is not None else np.float64(dt) * np.float64(nu)
        if qdrag:
            q = np.float64(dt) * (np.float64(drag) + np.float64(cd) * sp[idx])
        else:
            q = np.float64(dt) * np.float64(drag) if drag != 0.0 else None
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
            DF[idx, :n - 1] = DF[idx, :n - 1] - mf.df_terms(he, z, un[idx, :n], dt)
        if qdrag or wcd:
            t = z[:, -1] * un[idx, n - 1]
            if qdrag:
                pos = sp[idx] > 0.0
                M[idx] = np.where(pos, (0.0 - dtcd * t) / np.where(pos, sp[idx], 1.0), 0.0)
            if wcd:
                dens[QUADRATIC][idx] = dens[QUADRATIC][idx] - (np.float64(dt) * t) * sp[idx]
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
    if parts is not None:
        parts["M"] = M
    if qdrag:
        XU = chain(mesh, mlt, XU, us, M)
    return XU, XH


# ---- the whole sweep ----------------------------------------------------------------------------------------------------------------
class QuadraticForcedTwin(mf.ForcedFieldTwin):
    """momentum_vfield_twin.ForcedFieldTwin whose steps may run with a Cd (`cd`, replaceable between steps, like nu, drag, fld);
    want_cd: the density D_cd, in self.dens[QUADRATIC].  `sps`: after every step, the sp of the last pass that was launched (what
    moka_bottom_speed_download hands out: zeros when that pass ran without Cd)."""

    def __init__(self, om, ssh, u, h, want=0, want_field=False, want_cd=False, chain=speed_transpose):
        super().__init__(om, ssh, u, h, want, want_field)
        self.cd, self.want_cd, self.chain = 0.0, want_cd, chain
        if want_cd:
            self.dens[QUADRATIC] = np.zeros(self.mesh.nEdges)
        self.sps, self.sp_last = [], np.zeros(self.mesh.nEdges)

    def step(self, dt):
        assert self.fld is None or mf.check_field(self.fld, self.mlt)
        self.rk.step_rk4(dt)
        us = self.st.u[1].copy()
        new, sp = qd.apply(us, self.st.h[1], self.mlt, self.c1, self.c2, dt, self.nu, self.drag, self.tau, self.cd, self.mesh, qd.bottom_speed,
                           self.fld)
        self.st.u[1][...] = new
        drag = self.cd != 0.0 or self.drag != 0.0         # quadratic_drag_twin.QuadraticDragTwin.mix: a launched pass replaces `sp`
        if (drag or mf.pass_on(self.nu, self.drag, self.tau, self.mlt, self.fld)) and dt != 0.0 \
                and not (us.shape[1] < 2 and not drag and not mv.stress_on(self.tau, self.mlt)):
            self.sp_last = sp
        self.sps.append(self.sp_last.copy())
        nu, fld = mf.taken(self.nu, self.fld, self.mlt)
        qdrag = self.cd != 0.0 and dt != 0.0
        rec = sp if qdrag else qd.bottom_speed(us, self.mlt, self.mesh) if (self.want_cd and dt != 0.0) else None
        self.recs.append((self.st.u[1].copy(), self.st.h[1].copy(), nu, self.drag, self.tau, None if fld is None else fld.copy(),
                          self.cd if qdrag else 0.0, rec, us if qdrag else None))

    def sweep(self, XU, XH):
        for d in self.dens.values():
            d[...] = 0.0
        if self.DF is not None:
            self.DF[...] = 0.0
        while self.recs:
            un, hn, nu, drag, tau, fld, cd, sp, us = self.recs.pop()
            P, dt = self.rk.tape.pop()
            XU, XH = transposed_pass(self.mesh, self.mlt, XU, XH, un, hn, dt, nu, drag, tau, fld, self.dens, self.DF, cd, sp, us, self.chain)
            XU, XH = self.reverse_rk4(P, dt, XU, XH)
        return XU, XH

    def gradients(self):
        out = super().gradients()
        if QUADRATIC in self.dens:
            out["quadraticDrag"] = fa._ldsum(self.dens[QUADRATIC])
        return out


# ---- long double --------------------------------------------------------------------------------------------------------------------
def transpose_ld(mesh, mlt, XU, un, hn, us, dt, nu, drag, cd):
    """The docstring's long-double model of one transposed pass with Cd != 0 (scalar nu): returns (XU_ld, Dcd_ld, bXU, bD) with the
    bounds on |twin - ld| (the factor 2^-53 included), bXU zero in the rows k >= n_e."""
    nE, K = XU.shape
    nn = _depths(mlt, nE, K)
    c1, c2 = mv.edge_cells(mesh)
    m = int(np.asarray(mesh.edgesOnCell).shape[1])
    _, c_sp, c_q = qd.counts(mesh)
    c_m, c_d = 4 + c_sp, 3 + c_sp
    c_ch = c_m + m + 6
    sp_ld = qd.speed_ld(us, mlt, mesh)
    sp_tw = qd.bottom_speed(us, mlt, mesh)
    s64 = float(np.float64(dt) * np.float64(nu))
    q_ld = LD(float(dt)) * (LD(float(drag)) + LD(float(cd)) * sp_ld)
    q_tw = np.float64(dt) * (np.float64(drag) + np.float64(cd) * sp_tw)
    dtcd = LD(float(dt)) * LD(float(cd))
    out, bXU = np.asarray(XU).astype(LD), np.zeros(XU.shape, dtype=LD)
    M, Mabs, Mez = np.zeros(nE, dtype=LD), np.zeros(nE, dtype=LD), np.zeros(nE, dtype=LD)
    Dcd, bD = np.zeros(nE, dtype=LD), np.zeros(nE, dtype=LD)
    for n in np.unique(nn):
        if n < 1:
            continue
        idx = np.nonzero(nn == n)[0]
        he = 0.5 * (hn[c1[idx], :n] + hn[c2[idx], :n])
        A, inv = qd.dense_ld(he, s64, q_ld[idx])
        X = np.asarray(XU[idx, :n]).astype(LD)
        z = tv.mv(inv, X)
        zt = fa.adjoint_cols(he, XU[idx, :n], un[idx, :n], np.float64(s64), q_tw[idx], None)[0]
        inner = mv.C_SOLVE * (tv.mv(np.abs(A), np.abs(zt)) + np.abs(X))
        inner[:, -1] += c_q * q_ld[idx] * np.abs(zt[:, -1]).astype(LD)
        ez = tv.mv(np.abs(inv), inner)
        hL = he.astype(LD)
        out[idx, :n] = hL * z
        bXU[idx, :n] = hL * ez + np.abs(hL * zt)
        ub = np.abs(un[idx, n - 1]).astype(LD)
        t = z[:, -1] * un[idx, n - 1].astype(LD)
        pos = sp_ld[idx] > 0
        spp = np.where(pos, sp_ld[idx], LD(1))
        M[idx] = np.where(pos, -dtcd * t / spp, LD(0))
        tt = np.abs(zt[:, -1] * un[idx, n - 1]).astype(LD)
        Mabs[idx] = np.where(pos, np.abs(dtcd) * tt / spp, LD(0))
        Mez[idx] = np.where(pos, np.abs(dtcd) * ez[:, -1] * ub / spp, LD(0))
        Dcd[idx] = -(LD(float(dt)) * t) * sp_ld[idx]
        bD[idx] = c_d * LD(float(dt)) * tt * sp_ld[idx] + LD(float(dt)) * ez[:, -1] * ub * sp_ld[idx]
    live = np.arange(K)[None, :] < nn[:, None]
    area = np.asarray(mesh.areaCell).astype(LD)
    kcu = (np.asarray(mesh.dcEdge).astype(LD) * np.asarray(mesh.dvEdge).astype(LD) / 4)[:, None] * np.where(live, us, 0.0).astype(LD)
    has = np.nonzero(nn >= 1)[0]
    terms = []
    for v in (M, Mabs, Mez):                       # scattered from the edges through cellsOnEdge
        C = np.zeros((mesh.nCells, K), dtype=LD)
        np.add.at(C, (c1[has], nn[has] - 1), v[has])
        np.add.at(C, (c2[has], nn[has] - 1), v[has])
        C = C / area[:, None]
        terms.append(np.where(live, C[c1] + C[c2], LD(0)))
    out = out + np.where(live, kcu * terms[0], LD(0))
    bXU = bXU + np.abs(kcu) * (c_ch * terms[1] + terms[2])
    bXU = np.where(live, bXU + np.abs(out), LD(0))
    return out, Dcd, bXU * U53, bD * U53
