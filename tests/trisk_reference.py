"""Extended-precision reference of the TRiSK tendencies: the linear form of the reference, the optional nonlinear terms, Del2 and
Del4 momentum mixing -- written from the formulas, independent of the oracle and of the HIP library.  TEST INFRASTRUCTURE ONLY.

Everything here is numpy in np.longdouble (x87 extended: 64-bit mantissa, unit round-off 2^-64): gathers and scatters over the
mesh's connectivity with fancy indexing.  Only the MeshData it is handed is read; no oracle, no twin, no library.

Formulas (Ringler et al. 2010, J. Comput. Phys. 229; MPAS-Ocean ocn_vel_hmix_del2 / ocn_vel_hmix_del4) in the conventions of
the oracle's header and DESIGN.md: connectivity 1-based, edgeSignOnCell / edgeSignOnVertex -1 where the cell / vertex is the edge's first,
fields (entity, level), a level k (0-based) of edge e is active when k < maxLevelEdgeTop[e] (mlt).
    ssh_i    = sum_k h_ik - restingThicknessSum_i
    hEdge_e  = (h_c1 + h_c2) / 2,   F_e = u_e hEdge_e
    div(x)_i = -(1 / A_i) sum_j edgeSignOnCell_ij dv_e x_e                        (e = edgesOnCell_ij)
    curl(x)_v = (1 / At_v) sum_j edgeSignOnVertex_vj dc_e x_e                     (e = edgesOnVertex_vj)
    tendH_ik = -(1 / A_i) sum_j (-edgeSignOnCell_ij) dv_e F_ek   over the active (e, k) only
  linear (the reference):
    tendU_e  = -g (ssh_c2 - ssh_c1) / dc_e + sum_j w_ej u_e' fEdge_e'            (e' = edgesOnEdge_ej; active levels, else 0)
  nonlinear (vector-invariant TRiSK):
    h_v = (1 / At_v) sum_j kite_vj h_{cellsOnVertex_vj},   q_v = (fVertex_v + curl(u)_v) / h_v,   q_e = (q_v1 + q_v2) / 2
    KE_i = (1 / A_i) sum_j dc_e dv_e u_e^2 / 4
    tendU_e = -g (ssh_c2 - ssh_c1) / dc_e - (KE_c2 - KE_c1) / dc_e + sum_j w_ej F_e' (q_e + q_e') / 2   (active levels, else 0)
  mixing, L(x)_e = (div(x)_c2 - div(x)_c1) / dc_e - (curl(x)_v2 - curl(x)_v1) / dv_e  (= grad div - k x grad curl), 0 on inactive levels:
    Del2: tendU += visc_del2 L(u)
    Del4: tendU -= visc_del4 s_e L(L(u))       (s = the per-edge scaling array, 1 without one)

Error bound.  `abs=True` evaluates the same expressions with every leaf and every intermediate replaced by a magnitude M that
bounds it: M(a +- b) = M(a) + M(b), M(a b) = M(a) M(b), M(a / b) = M(a) / |b| + |a| M(b) / b^2, exact inputs M(x) = |x|.  In
particular ssh contributes sum_k |h| + |rest| (not |ssh|: the cancellation of the column sum is what a kernel pays for) and
differences become sums.  A double-precision evaluation of the expression in any order whose longest chain of dependent
roundings has n steps is then within gamma_n M ~ n 2^-53 M of the exact value, so each element is checked as
    |x - x_ref| <= C 2^-53 M
with C the longest chain of the output, counted for the evaluation orders the library and the oracle use (a chain is one
rounding per +, -, *, /, including forming 1/dc, 1/A; the factors 0.5 / 0.25 and the +-1 signs are exact):
    C_SSH  = 16  column sum: 6 butterfly steps + ceil(K / 64) - 1 strided adds + the subtraction of restingThicknessSum
                 (<= 9 for K <= 192; also covers any pairwise order to K = 2^14)
    C_H    = 16  hEdge 1, F 1, * dv 1, * (1/A) 2, the sum over <= 7 edges 6: 11
    C_U    = 48  the longest is Del4's: L(u) 12, its div 9 more, the difference and 1/dc 3, coef4 = visc_del4 s 1, the sum of up
                 to 14 PV-flux terms, KE gradient, pressure gradient and Del2 term in the accumulator 17: <= 42 (the PV-flux term
                 itself is 10 deep, the KE gradient 15, the pressure gradient 11)
The reference's own error (2^-64 relative per operation, on the same magnitudes) is below 2^-7 of the bound.  Storage in fp32
adds half an ulp of fp32 on top (see `within`).

`rk4` is the reference's RK4 step with the running sum (time_integration.jl:61-148: Provis = Curr + a_s t, New += b_s t),
`forward_euler` its Forward-Euler step (time_integration.jl:160-190) on the state (u, h, ssh, layerThicknessEdge)."""
from __future__ import annotations

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "the reference needs an extended long double (x87 80-bit or binary128), not plain double"

G = LD(9.80616)  # the literal of pressure_gradient.jl:63, as the double the kernels use
U53 = LD(2.0) ** -53
C_SSH, C_H, C_U = 16, 16, 48

_GEOM = {}


class Geometry:
    """Long-double geometry and 0-based connectivity of one MeshData."""

    def __init__(self, mesh):
        self.mesh = mesh
        ld = lambda a: np.asarray(a, dtype=np.float64).astype(LD)
        i0 = lambda a: np.asarray(a, dtype=np.int64) - 1
        self.nC, self.nE, self.nV = mesh.nCells, mesh.nEdges, mesh.nVertices
        self.c1, self.c2 = i0(mesh.cellsOnEdge[:, 0]), i0(mesh.cellsOnEdge[:, 1])
        self.v1, self.v2 = i0(mesh.verticesOnEdge[:, 0]), i0(mesh.verticesOnEdge[:, 1])
        self.dc, self.dv = ld(mesh.dcEdge), ld(mesh.dvEdge)
        self.areaC, self.areaT = ld(mesh.areaCell), ld(mesh.areaTriangle)
        ME = mesh.edgesOnCell.shape[1]
        self.c_ok = np.arange(ME)[None, :] < np.asarray(mesh.nEdgesOnCell)[:, None]
        self.eoc = np.where(self.c_ok, i0(mesh.edgesOnCell), 0)
        self.sC = np.where(self.c_ok, np.asarray(mesh.edgeSignOnCell), 0).astype(LD)
        VD = mesh.vertexDegree
        self.eov = i0(mesh.edgesOnVertex[:, :VD])
        self.sV = np.asarray(mesh.edgeSignOnVertex)[:, :VD].astype(LD)
        self.cov = i0(mesh.cellsOnVertex[:, :VD])
        self.kite = ld(mesh.kiteAreasOnVertex) if mesh.kiteAreasOnVertex is not None else None
        ME2 = mesh.edgesOnEdge.shape[1]
        eoe = np.asarray(mesh.edgesOnEdge, dtype=np.int64)
        self.e_ok = (np.arange(ME2)[None, :] < np.asarray(mesh.nEdgesOnEdge)[:, None]) & (eoe > 0)
        self.eoe = np.where(self.e_ok, eoe - 1, 0)
        self.w = np.where(self.e_ok, np.asarray(mesh.weightsOnEdge, dtype=np.float64), 0.0).astype(LD)
        self.fE, self.fV = ld(mesh.fEdge), ld(mesh.fVertex)


def geometry(mesh) -> Geometry:
    """Cached per MeshData object (the cache holds the mesh, so its id is not reused)."""
    g = _GEOM.get(id(mesh))
    if g is None or g.mesh is not mesh:
        g = _GEOM[id(mesh)] = Geometry(mesh)
    return g


# ---- operators on (value, magnitude) pairs; a magnitude of None skips the abs evaluation ----------------------------------------
def _col(a):
    return a[:, None]


def _ld(a, shape):
    """Long double view of an input: doubles (or fp32 values) widened exactly, long doubles kept (the RK4 stages)."""
    a = np.asarray(a)
    return (a if a.dtype == LD else a.astype(np.float64).astype(LD)).reshape(shape)


def divergence(g, x, mx=None):
    """div(x) on cells: -(1/A) sum_j sign dv x."""
    d = np.zeros((g.nC, x.shape[1]), dtype=LD)
    md = None if mx is None else np.zeros_like(d)
    for j in range(g.eoc.shape[1]):
        e = g.eoc[:, j]
        d -= _col(g.sC[:, j] * g.dv[e]) * x[e]
        if mx is not None:
            md += _col(np.abs(g.sC[:, j]) * g.dv[e]) * mx[e]
    return d / _col(g.areaC), None if mx is None else md / _col(g.areaC)


def curl(g, x, mx=None):
    """curl(x) on vertices: (1/At) sum_j sign dc x."""
    z = np.zeros((g.nV, x.shape[1]), dtype=LD)
    mz = None if mx is None else np.zeros_like(z)
    for j in range(g.eov.shape[1]):
        e = g.eov[:, j]
        z += _col(g.sV[:, j] * g.dc[e]) * x[e]
        if mx is not None:
            mz += _col(g.dc[e]) * mx[e]
    return z / _col(g.areaT), None if mx is None else mz / _col(g.areaT)


def grad_cell(g, s, ms=None):
    """(s_c2 - s_c1) / dc on edges; s (nCells, K) or (nCells,)."""
    s2 = s if s.ndim == 2 else s[:, None]
    v = (s2[g.c2] - s2[g.c1]) / _col(g.dc)
    if ms is None:
        return v, None
    m2 = ms if ms.ndim == 2 else ms[:, None]
    return v, (m2[g.c2] + m2[g.c1]) / _col(g.dc)


def grad_vertex(g, z, mz=None):
    """(z_v2 - z_v1) / dv on edges."""
    v = (z[g.v2] - z[g.v1]) / _col(g.dv)
    return v, None if mz is None else (mz[g.v2] + mz[g.v1]) / _col(g.dv)


def active(g, mlt, K):
    return np.arange(K)[None, :] < np.asarray(mlt)[:, None]


def laplacian(g, x, mx, act, rot_sign=-1):
    """L(x) = grad div x + rot_sign * skew grad curl x (rot_sign = -1: the vector Laplacian; +1 only for the self-tests), 0 on the
    inactive levels."""
    d, md = divergence(g, x, mx)
    z, mz = curl(g, x, mx)
    a, ma = grad_cell(g, d, md)
    b, mb = grad_vertex(g, z, mz)
    v = np.where(act, a + rot_sign * b, 0)
    return v, None if mx is None else np.where(act, ma + mb, 0)


def ssh_of(h, rest, want_m=True):
    v = h.sum(axis=1) - rest
    return v, (np.abs(h).sum(axis=1) + np.abs(rest)) if want_m else None


def thickness_tendency(g, u, h, act, want_m=True):
    hE = (h[g.c1] + h[g.c2]) / 2
    F = np.where(act, u * hE, 0)
    mF = np.where(act, np.abs(u) * (np.abs(h[g.c1]) + np.abs(h[g.c2])) / 2, 0) if want_m else None
    t, mt = divergence(g, F, mF)
    return -t, mt


def terms(mesh, u, h, rest_sum, mlt, *, nonlinear, mixing=True, abs=True, ssh=None, rot_sign=-1, fvertex=None):
    """The separate terms of the tendencies in long double: a dict of (value, magnitude) pairs
        "U": tendU without mixing, "H": tendH, "ssh": ssh, and with `mixing` (nonlinear only) "D2" = L(u), "D4" = L(L(u))
    so that every combination of viscosities is tendU = U + visc_del2 D2 - visc_del4 s D4.  `ssh`: a stored surface height to use in
    the pressure gradient instead of the column sum (fp32-storage states store it before the gradient reads it); `fvertex`: a
    Coriolis parameter on vertices in place of the mesh's.  abs=False leaves the magnitudes None."""
    g = geometry(mesh)
    u = _ld(u, (g.nE, -1))
    K = u.shape[1]
    h = _ld(h, (g.nC, K))
    rest = _ld(rest_sum, (g.nC,))
    act = active(g, mlt, K)
    mu = np.abs(u) if abs else None
    out = {}
    sv, sm = ssh_of(h, rest, abs)
    out["ssh"] = (sv, sm)
    if ssh is not None:
        sv = _ld(ssh, (g.nC,))
        sm = np.abs(sv) if abs else None
    pv, pm = grad_cell(g, sv, sm)
    tU = -G * pv
    mU = G * pm if abs else None
    out["H"] = thickness_tendency(g, u, h, act, abs)
    if not nonlinear:
        for j in range(g.eoe.shape[1]):
            e = g.eoe[:, j]
            wf = _col(g.w[:, j] * g.fE[e])
            tU = tU + wf * u[e]
            if abs:
                mU = mU + np.abs(wf) * mu[e]
        out["U"] = (np.where(act, tU, 0), np.where(act, mU, 0) if abs else None)
        return out
    # kinetic energy and its gradient
    ke = np.zeros((g.nC, K), dtype=LD)
    for j in range(g.eoc.shape[1]):
        e = g.eoc[:, j]
        ke += _col(np.where(g.c_ok[:, j], g.dc[e] * g.dv[e] / 4, 0)) * u[e] * u[e]
    ke /= _col(g.areaC)
    kv, km = grad_cell(g, ke, ke if abs else None)              # KE is a sum of non-negative terms: M(KE) = KE
    tU = tU - kv
    mU = mU + km if abs else None
    # potential vorticity
    z, mz = curl(g, u, mu)
    hv = np.zeros((g.nV, K), dtype=LD)
    mhv = np.zeros_like(hv) if abs else None
    for j in range(g.cov.shape[1]):
        c = g.cov[:, j]
        hv += _col(g.kite[:, j]) * h[c]
        if abs:
            mhv += _col(np.abs(g.kite[:, j])) * np.abs(h[c])
    hv /= _col(g.areaT)
    fv = g.fV if fvertex is None else _ld(fvertex, (g.nV,))
    num = _col(fv) + z
    q = num / hv
    if abs:
        mhv /= _col(g.areaT)
        mq = (_col(np.abs(fv)) + mz) / np.abs(hv) + np.abs(num) * mhv / (hv * hv)
    qe = (q[g.v1] + q[g.v2]) / 2
    mqe = (mq[g.v1] + mq[g.v2]) / 2 if abs else None
    hE = (h[g.c1] + h[g.c2]) / 2
    F = u * hE
    mF = mu * (np.abs(h[g.c1]) + np.abs(h[g.c2])) / 2 if abs else None
    for j in range(g.eoe.shape[1]):
        e = g.eoe[:, j]
        w = _col(g.w[:, j])
        tU = tU + w * F[e] * ((qe + qe[e]) / 2)
        if abs:
            mU = mU + np.abs(w) * mF[e] * ((mqe + mqe[e]) / 2)
    out["U"] = (np.where(act, tU, 0), np.where(act, mU, 0) if abs else None)
    if mixing:
        d2 = laplacian(g, u, mu, act, rot_sign)
        out["D2"] = d2
        out["D4"] = laplacian(g, d2[0], d2[1], act, rot_sign)
    return out


def combine(t, visc_del2=0.0, visc_del4=0.0, scaling_del4=None):
    """(tendU, M(tendU)) of one combination of viscosities from `terms`."""
    U, MU = t["U"]
    if visc_del2:
        U = U + LD(visc_del2) * t["D2"][0]
        MU = None if MU is None else MU + LD(np.abs(visc_del2)) * t["D2"][1]
    if visc_del4:
        s = LD(visc_del4) * (np.asarray(scaling_del4, dtype=np.float64).astype(LD) if scaling_del4 is not None else LD(1))
        s = np.broadcast_to(s, (U.shape[0],))[:, None]
        U = U - s * t["D4"][0]
        MU = None if MU is None else MU + np.abs(s) * t["D4"][1]
    return U, MU


def tendencies(mesh, u, h, rest_sum, mlt, *, nonlinear, visc_del2=0.0, visc_del4=0.0, scaling_del4=None, abs=False, ssh=None,
               rot_sign=-1, fvertex=None):
    """(tendU, tendH, ssh) in long double; abs=True: their magnitudes M instead (the bound of the module docstring)."""
    mixing = bool(nonlinear and (visc_del2 or visc_del4))
    t = terms(mesh, u, h, rest_sum, mlt, nonlinear=nonlinear, mixing=mixing, abs=abs, ssh=ssh, rot_sign=rot_sign, fvertex=fvertex)
    U = combine(t, visc_del2, visc_del4, scaling_del4)
    k = 1 if abs else 0
    return U[k], t["H"][k], t["ssh"][k]


def rk4(mesh, u, h, rest_sum, mlt, dt, nsteps=1, *, nonlinear, visc_del2=0.0, visc_del4=0.0, scaling_del4=None):
    """nsteps RK4 steps (running sum; the stage states stay long double) in long double; returns (u, h, ssh)."""
    g = geometry(mesh)
    cu, ch = _ld(u, (g.nE, -1)), _ld(h, (g.nC, -1))
    dt = LD(dt)
    a = (dt / 2, dt / 2, dt)
    b = (dt / 6, dt / 3, dt / 3, dt / 6)
    kw = dict(nonlinear=nonlinear, visc_del2=visc_del2, visc_del4=visc_del4, scaling_del4=scaling_del4)
    for _ in range(nsteps):
        nu, nh = cu, ch
        pu, ph = cu, ch
        for s in range(4):
            tu, th, _ = tendencies(mesh, pu, ph, rest_sum, mlt, **kw)
            if s < 3:
                pu, ph = cu + a[s] * tu, ch + a[s] * th
            nu, nh = nu + b[s] * tu, nh + b[s] * th
        cu, ch = nu, nh
    return cu, ch, ch.sum(axis=1) - _ld(rest_sum, (g.nC,))


def forward_euler(mesh, u, h, ssh, rest_sum, mlt, dt, nsteps=1, *, hE=None, stale=False):
    """nsteps Forward-Euler steps of the linear form in long double (time_integration.jl:160-190): the pressure gradient reads the
    carried ssh, the flux the carried layerThicknessEdge hE when `stale` (else interp(h)); u' = u + dt tendU, h' = h + dt tendH,
    ssh' = sum_k h' - rest, hE' = interp(h).  Returns (u, h, ssh, hE)."""
    g = geometry(mesh)
    u, h = _ld(u, (g.nE, -1)), _ld(h, (g.nC, -1))
    K = u.shape[1]
    ssh, rest = _ld(ssh, (g.nC,)), _ld(rest_sum, (g.nC,))
    hE = (h[g.c1] + h[g.c2]) / 2 if hE is None else _ld(hE, (g.nE, K))
    act = active(g, mlt, K)
    dt = LD(dt)
    for _ in range(nsteps):
        hI = (h[g.c1] + h[g.c2]) / 2
        tU = terms(mesh, u, h, rest, mlt, nonlinear=False, abs=False, ssh=ssh)["U"][0]
        tH = -divergence(g, np.where(act, u * (hE if stale else hI), 0))[0]
        u, h, hE = u + dt * tU, h + dt * tH, hI
        ssh = h.sum(axis=1) - rest
    return u, h, ssh, hE


# ---- the per-element check ------------------------------------------------------------------------------------------------------
def within(x, ref, M, C, f32=False):
    """Boolean array: |x - ref| <= C 2^-53 M elementwise; f32=True (an fp32-stored output) adds half an ulp of fp32 of the largest
    value the double result can have, |ref| + C 2^-53 M."""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    tol = C * U53 * M
    if f32:
        top = (np.abs(ref) + tol).astype(np.float64).astype(np.float32)
        tol = tol + np.spacing(np.abs(top)).astype(np.float64).astype(LD) / 2
    return np.abs(x - ref) <= tol


# ---- identities of the scheme, every quantity but the tendencies formed here from the state -------------------------------------
def energy_budget(mesh, u, h, ssh, tendU, tendH, MU, MH):
    """sum_k [sum_e dc dv F tendU + sum_i A KE tendH] + sum_i A g ssh sum_k tendH (= 0 for the inviscid nonlinear tendencies when u
    is 0 on the inactive levels) and the magnitude it is to be compared with, C_U 2^-53 times the same sum over the bounds.  `ssh`
    is the surface height the tendencies were formed with (the discrete pressure work cancels against it exactly)."""
    g = geometry(mesh)
    u, h = _ld(u, (g.nE, -1)), _ld(h, (g.nC, -1))
    K = u.shape[1]
    tU, tH = _ld(tendU, (g.nE, K)), _ld(tendH, (g.nC, K))
    s = _ld(ssh, (g.nC,))
    F = u * (h[g.c1] + h[g.c2]) / 2
    ke = np.zeros((g.nC, K), dtype=LD)
    for j in range(g.eoc.shape[1]):
        e = g.eoc[:, j]
        ke += _col(np.where(g.c_ok[:, j], g.dc[e] * g.dv[e] / 4, 0)) * u[e] * u[e]
    ke /= _col(g.areaC)
    wE, wC = _col(g.dc * g.dv), _col(g.areaC)
    res = (wE * F * tU).sum() + (wC * ke * tH).sum() + (g.areaC * G * s * tH.sum(axis=1)).sum()
    scale = (wE * np.abs(F) * MU).sum() + (wC * ke * MH).sum() + (g.areaC * G * np.abs(s) * MH.sum(axis=1)).sum()
    return res, C_U * U53 * scale


def mass_budget(mesh, tendH, MH):
    """sum_i A_i tendH_ik per level (= 0) and its tolerance C_H 2^-53 sum_i A_i M(tendH)_ik."""
    g = geometry(mesh)
    tH = _ld(tendH, (g.nC, -1))
    return (_col(g.areaC) * tH).sum(axis=0), C_H * U53 * (_col(g.areaC) * MH).sum(axis=0)


def uniform_q_fvertex(mesh, u, h, q0):
    """fVertex = q0 h_v - curl(u)_v (one layer): the potential vorticity is q0 everywhere.  Returned as the doubles a mesh holds."""
    g = geometry(mesh)
    u, h = _ld(u, (g.nE, 1)), _ld(h, (g.nC, 1))
    hv = np.zeros((g.nV, 1), dtype=LD)
    for j in range(g.cov.shape[1]):
        hv += _col(g.kite[:, j]) * h[g.cov[:, j]]
    hv /= _col(g.areaT)
    z, _ = curl(g, u)
    return (LD(q0) * hv - z)[:, 0].astype(np.float64)


def pv_compatibility(mesh, q0, tendU, tendH, MU, MH):
    """curl(tendU)_v - q0 sum_j kite_vj tendH_{c_j} / At_v (= 0 when q = q0 everywhere and the masks are full) per (vertex, level),
    and the tolerance per element: the curl / kite average of the bounds of the two tendencies."""
    g = geometry(mesh)
    K = np.asarray(tendU).reshape(g.nE, -1).shape[1]
    tU, tH = _ld(tendU, (g.nE, K)), _ld(tendH, (g.nC, K))
    z, mz = curl(g, tU, MU)
    avg = np.zeros((g.nV, K), dtype=LD)
    mavg = np.zeros_like(avg)
    for j in range(g.cov.shape[1]):
        c = g.cov[:, j]
        avg += _col(g.kite[:, j]) * tH[c]
        mavg += _col(np.abs(g.kite[:, j])) * MH[c]
    q0 = LD(q0)
    return z - q0 * avg / _col(g.areaT), C_U * U53 * mz + C_H * U53 * np.abs(q0) * mavg / _col(g.areaT)


def coriolis_pairs(mesh):
    """For every edgesOnEdge entry (e, e'): dc_e dv_e w_ee' and the same of the mirrored entry (e', e) (TRiSK: their sum is 0)."""
    g = geometry(mesh)
    e = np.repeat(np.arange(g.nE), g.eoe.shape[1]).reshape(g.eoe.shape)[g.e_ok]
    ep = g.eoe[g.e_ok]
    a = (_col(g.dc * g.dv) * g.w)[g.e_ok]
    key = e * g.nE + ep
    order = np.argsort(key)
    pos = np.searchsorted(key[order], ep * g.nE + e)
    pos = np.minimum(pos, key.size - 1)
    found = key[order][pos] == ep * g.nE + e
    return a, np.where(found, a[order][pos], np.nan)
