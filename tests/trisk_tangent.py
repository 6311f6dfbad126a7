"""Extended-precision tangent-linear model of the Forward-Euler and RK4 maps, for the objective J = sum(ssh_N^2) of the reverse
mode -- written from the formulas, independent of the oracle's adjoint and of the HIP library, and with no transpose anywhere.
TEST INFRASTRUCTURE ONLY.

The reverse sweep gives g = dJ / d(initial state).  For a direction v of the initial state the tangent gives dJ = <g, v> exactly
(the maps are polynomials, no truncation), so both a dot product along v and, with v = e_i, a single entry g_i are pinned.
Everything is numpy in np.longdouble, on the linear operators of trisk_reference (divergence, grad_cell, active) plus the
Coriolis gather below, which reads edgesOnEdge from the mesh itself; the tangent of a linear operator is the operator itself, the
only product rule is that of the thickness flux F = u hE: dF = du hE + u dhE.

Forward Euler (the reference's ocn_timestep(..., ForwardEuler), time_integration.jl:160-190, on DiagnosticVars.jl's
diagnostic_compute! and Operators.jl's interpolation / flux; state (u, h, ssh, hE), hE = DiagnosticVars.layerThicknessEdge carried
between steps, ssh_0 and hE_0 independent inputs):
    hEuse = stale ? hE : interp(h)                           interp(h)_e = (h_c1 + h_c2) / 2        (Operators.jl:217)
    tendU = active (-g grad(ssh) + sum_j w_ej fEdge_e' u_e')         (pressure_gradient.jl:61-63, coriolis.jl:61-73)
    tendH = -div(active u hEuse)                                     (horizontal_advection.jl:55-70)
    u' = u + dt tendU,  h' = h + dt tendH,  ssh' = sum_k h' - restingThicknessSum,  hE' = interp(h)
flags: 1 = stale hEdge; 2 (accumulated vorticity) does not enter J; 4 (level 1 only) is the same map at K = 1.
RK4 (time_integration.jl:61-148, the running sum): on (u, h), T(u, h) = (tendU, tendH) with ssh = sum_k h - rest and hE = interp(h)
inside every evaluation; P_1 = x, t_s = T(P_s), P_{s+1} = x + a_s t_s, x' = x + sum_s b_s t_s, a = (dt/2, dt/2, dt),
b = (dt/6, dt/3, dt/3, dt/6).  Objective: J = sum_i ssh_N,i^2, dJ = 2 <ssh_N, dssh_N> (ssh_N = sum_k h_N - rest for RK4).

Error bound.  Magnitudes as in trisk_reference (abs=True): every forward value x carries M(x) >= |x| + its own error budget,
M(a +- b) = M(a) + M(b), M(a b) = M(a) M(b), inputs exact (M(x) = |x|), and the steps carry them (M(u') = M(u) + dt M(tendU), ...).
The tangent evaluated with |partials|, |v| and the forward magnitudes in place of the forward values gives M_d >= |dJ|, the sum
over every path from v to J of |product of partials|.  A double-precision reverse sweep along a double forward run computes each
path term with the relative error of its longest chain of dependent roundings -- the forward values it reads (u_n, hEuse_n, the
seed 2 ssh_N) bring their forward chain, its own transposed arithmetic the transposed chain -- so
    |<g, v> - dJ| <= C_adj 2^-53 M_d,     C_adj = nsteps (C_F + C_T)
with <g, v> summed in long double.  Chains, counted as in trisk_reference (one rounding per +, -, *, /, forming 1/dc, 1/A and
g/dc included; 0.5, 2 and the signs exact; a product adds the chains of its factors plus one):
  Forward Euler, per step
    C_F  = 34  the seed's chain: h' = h + dt tendH is tendH (C_H = 16) + 2, then the column sum of ssh' (C_SSH = 16); u' is
               shorter (Coriolis: w f 1, * u 1, a sum of <= 14 slots 13, + the pressure gradient (g / dc 2, difference 1, * 1) 1,
               * dt 1, + u 1 = 18), hE' = interp(h) 2
    C_T  = 22  the transposed step: Fbar = sd1 dt (lamH1 + lamS1) + sd2 ... (sd = dv sign (1/A): 2; tH: 2; * 1; + 1) 6;
               lamU0 = (lamU1 + hEuse Fbar) + cor, cor = sum of <= 14 (tw f) (dt lamU1) terms: 3 + 13 = 16, + 1 = 17;
               csum = ksum_k dt lamU1 (1 + 6 butterfly + ceil(K / 64) - 1 <= 9, K <= 192) 10; lamS0 = sum of <= 7 (-sign)
               (g / dc) csum terms: 10 + 3 + 6 = 19; lamH0 = (lamH1 + lamS1) + 0.5 sum of <= 7 u Fbar: 7 + 6 + 1 = 14;
               rounded up to 22 for the forms that sum a column in another order (16-byte lanes: two butterflies + 1)
    C_FE = C_F + C_T = 56 per step
  RK4, per step
    C_F  = 96  four stages, each a tendency evaluation on the previous provisional state (ssh 16 + pressure gradient 4 + the
               Coriolis sum 15 + 1 = 36 for tendU, tendH 16) and P = x + a t (2): 4 x 22 = 88 on the tendU -> P chain through
               the stages (the tendU chain's 36 only once, at its end), the running sum of four terms 4, rounded up to 96
    C_T  = 96  per stage kb = b X + a Pb (3) and Pb = T^T kb (outU: hI Fbar (1 + 4 + 1) + cor (16) + 1 = 17;
               outH: 0.5 acc + ls, ls = sum of <= 7 (g / dc) csum with csum = ksum (9): 18 + 1 = 19), four stages chained
               4 x 22 = 88, the accumulation X + Pb4 + ... + Pb1 4 more: 92, rounded up to 96
    C_RK4 = 192 per step
The reference's own error (2^-64 per operation on the same magnitudes) is below 2^-6 of the bound."""
from __future__ import annotations

import numpy as np

import trisk_reference as tr
from trisk_reference import LD, G, U53

C_FE, C_RK4 = 56, 192
STALE, LEVEL1 = 1, 4
FIELDS = ("ssh", "u", "h", "hE")
_SLOTS = {}


def _c3(a):
    return a[:, None, None]


def coriolis_slots(mesh):
    """(e' (nEdges, ME2) 0-based, w_ej fEdge_e'): the Coriolis stencil read from the mesh; slots past nEdgesOnEdge and slots with
    edgesOnEdge == 0 (skipped, horizontal_advection_and_coriolis.jl:67) carry a zero coefficient."""
    got = _SLOTS.get(id(mesh))
    if got is not None and got[0] is mesh:
        return got[1]
    eoe = np.asarray(mesh.edgesOnEdge, dtype=np.int64)
    ok = (np.arange(eoe.shape[1])[None, :] < np.asarray(mesh.nEdgesOnEdge)[:, None]) & (eoe > 0)
    src = np.maximum(eoe, 1) - 1
    fE = np.asarray(mesh.fEdge, dtype=np.float64).astype(LD)
    wf = np.where(ok, np.asarray(mesh.weightsOnEdge, dtype=np.float64).astype(LD) * fE[src], 0)
    _SLOTS[id(mesh)] = (mesh, (src, wf))
    return src, wf


def coriolis(mesh, x, mx=None):
    """sum_j w_ej fEdge_e' x_e' on (nEdges, B, K), and its magnitude from mx."""
    src, wf = coriolis_slots(mesh)
    c = np.zeros_like(x)
    mc = None if mx is None else np.zeros_like(mx)
    for j in range(src.shape[1]):
        e = src[:, j]
        c += _c3(wf[:, j]) * x[e]
        if mx is not None:
            mc += _c3(np.abs(wf[:, j])) * mx[e]
    return c, mc


def divergence(g, x, mx=None):
    """trisk_reference.divergence on (nEdges, B, K)."""
    n, B, K = x.shape
    d, md = tr.divergence(g, x.reshape(n, -1), None if mx is None else mx.reshape(n, -1))
    return d.reshape(g.nC, B, K), None if md is None else md.reshape(g.nC, B, K)


def pressure_gradient(g, s, ms=None):
    """-g grad(ssh) on edges, s (nCells, B) -> (nEdges, B, 1); the magnitude g (M_c2 + M_c1) / dc."""
    v, m = tr.grad_cell(g, s, ms)
    return -G * v[:, :, None], None if m is None else G * m[:, :, None]


def interp(g, h, mh=None):
    return (h[g.c1] + h[g.c2]) / 2, None if mh is None else (mh[g.c1] + mh[g.c2]) / 2


class _Pair:
    """A value and its magnitude (None when magnitudes are off)."""
    __slots__ = ("v", "m")

    def __init__(self, v, m):
        self.v, self.m = v, m


def _add(a, s, b):
    """a + s b on pairs, s a positive scalar (dt, a_s, b_s)."""
    return _Pair(a.v + s * b.v, None if a.m is None else a.m + s * b.m)


def _interp(g, h):
    return _Pair(*interp(g, h.v, h.m))


def _colsum(h, rest=None):
    """ssh = sum_k h - rest: (nCells, B); without rest the tangent's column sum."""
    if rest is None:
        return _Pair(h.v.sum(axis=2), None if h.m is None else h.m.sum(axis=2))
    return _Pair(h.v.sum(axis=2) - rest[:, None], None if h.m is None else h.m.sum(axis=2) + np.abs(rest)[:, None])


def _tendencies(g, act, u, ssh, hE, du, dssh, dhE):
    """(tendU, tendH) at the point and their tangents; every argument a _Pair, ssh / hE the ones the evaluation uses."""
    mags = u.m is not None
    out = []
    for x, s, in ((u, ssh), (du, dssh)):
        pv, pm = pressure_gradient(g, s.v, s.m)
        cv, cm = coriolis(g.mesh, x.v, x.m)
        out.append(_Pair(act * (pv + cv), act * (pm + cm) if mags else None))
    tU, dU = out
    t, m = divergence(g, act * u.v * hE.v, act * u.m * hE.m if mags else None)
    tH = _Pair(-t, m)
    t, m = divergence(g, act * (du.v * hE.v + u.v * dhE.v),                # the product rule of F = u hE
                      act * (du.m * hE.m + u.m * dhE.m) if mags else None)
    dH = _Pair(-t, m)
    return tU, tH, dU, dH


def _fe_step(g, act, rest, x, d, dt, stale):
    u, h, ssh, hE = x
    du, dh, dssh, dhE = d
    hEuse, dhEuse = (hE, dhE) if stale else (_interp(g, h), _interp(g, dh))
    tU, tH, dU, dH = _tendencies(g, act, u, ssh, hEuse, du, dssh, dhEuse)
    h1, dh1 = _add(h, dt, tH), _add(dh, dt, dH)
    return ((_add(u, dt, tU), h1, _colsum(h1, rest), _interp(g, h)),
            (_add(du, dt, dU), dh1, _colsum(dh1), _interp(g, dh)))


def _rk4_step(g, act, rest, x, d, dt):
    u, h, du, dh = x[0], x[1], d[0], d[1]
    a = (dt / 2, dt / 2, dt)
    b = (dt / 6, dt / 3, dt / 3, dt / 6)
    pu, ph, dpu, dph = u, h, du, dh
    nu, nh, dnu, dnh = u, h, du, dh
    for s in range(4):
        tU, tH, dU, dH = _tendencies(g, act, pu, _colsum(ph, rest), _interp(g, ph), dpu, _colsum(dph), _interp(g, dph))
        if s < 3:
            pu, ph, dpu, dph = _add(u, a[s], tU), _add(h, a[s], tH), _add(du, a[s], dU), _add(dh, a[s], dH)
        nu, nh, dnu, dnh = _add(nu, b[s], tU), _add(nh, b[s], tH), _add(dnu, b[s], dU), _add(dnh, b[s], dH)
    return (nu, nh, _colsum(nh, rest), None), (dnu, dnh, _colsum(dnh), None)


def shapes(mesh, K):
    return {"ssh": (mesh.nCells,), "u": (mesh.nEdges, K), "h": (mesh.nCells, K), "hE": (mesh.nEdges, K)}


def run(mesh, mlt, rest_sum, state, dirs, dt, nsteps, *, method="fe", flags=0, mags=True):
    """The directional derivatives of J after nsteps steps from `state`.
        state: dict ssh (nCells,), u (nEdges, K), h (nCells, K), hE (nEdges, K; Forward Euler with the stale flag)
        dirs:  dict of the same keys with a leading batch axis (B, ...); a missing key is a zero direction
    Returns (dJ (B,), M_d (B,) or None).  method "fe" or "rk4" (ssh_0 and hE_0 do not enter RK4)."""
    g = tr.geometry(mesh)
    K = np.asarray(state["u"]).reshape(g.nE, -1).shape[1]
    if method == "fe" and (flags & LEVEL1) and K != 1:
        raise ValueError("level-1-only stepping is the same map only at K = 1")
    stale = method == "fe" and bool(flags & STALE)
    act = tr.active(g, mlt, K)[:, None, :]
    rest = tr._ld(rest_sum, (g.nC,))
    shp = shapes(mesh, K)
    B = next(np.asarray(v).shape[0] for v in dirs.values())

    def leaf(name):
        a = state.get(name)
        a = np.zeros(shp[name], dtype=LD) if a is None else tr._ld(a, shp[name])
        a = a[:, None] if name == "ssh" else a[:, None, :]
        return _Pair(a, np.abs(a) if mags else None)

    def dleaf(name):
        a = dirs.get(name)
        a = np.zeros((B,) + shp[name], dtype=LD) if a is None else tr._ld(a, (B,) + shp[name])
        a = np.ascontiguousarray(np.moveaxis(a, 0, 1))                # (n, B[, K])
        return _Pair(a, np.abs(a) if mags else None)

    x = tuple(leaf(n) for n in ("u", "h", "ssh", "hE"))                 # the state's order in the steps
    d = tuple(dleaf(n) for n in ("u", "h", "ssh", "hE"))
    dt = LD(dt)
    for _ in range(nsteps):
        x, d = _fe_step(g, act, rest, x, d, dt, stale) if method == "fe" else _rk4_step(g, act, rest, x, d, dt)
    s, ds = x[2], d[2]
    dJ = 2 * (s.v * ds.v).sum(axis=0)
    Md = 2 * (s.m * ds.m).sum(axis=0) if mags else None
    return dJ, Md


def constant(method, nsteps):
    """C_adj of the module docstring."""
    return (C_FE if method == "fe" else C_RK4) * nsteps


# ---- checks -----------------------------------------------------------------------------------------------------------------------
def unit_directions(mesh, K, entries):
    """Directions e_i for entries (field, index), index an int (ssh) or (row, level)."""
    shp = shapes(mesh, K)
    dirs = {}
    for b, (name, idx) in enumerate(entries):
        if name not in dirs:
            dirs[name] = np.zeros((len(entries),) + shp[name], dtype=LD)
        dirs[name][(b,) + (idx if isinstance(idx, tuple) else (idx,))] = 1
    return dirs


def dot(grad, dirs):
    """<g, v> per direction, in long double; grad a dict of the state's fields (doubles)."""
    B = next(np.asarray(v).shape[0] for v in dirs.values())
    out = np.zeros(B, dtype=LD)
    for name, v in dirs.items():
        gv = np.asarray(grad[name], dtype=np.float64).astype(LD).reshape(1, -1)
        out += (np.asarray(v).astype(LD).reshape(B, -1) * gv).sum(axis=1)
    return out


def within(got, dJ, Md, C):
    """|got - dJ| <= C 2^-53 M_d elementwise (M_d == 0: got must be exactly 0)."""
    return np.abs(np.asarray(got).astype(LD) - dJ) <= C * U53 * Md


def sharpness(got, dJ, Md, C):
    """(largest |err| / bound, largest bound / |dJ|) over the entries with a nonzero bound."""
    tol = C * U53 * Md
    nz = tol > 0
    if not nz.any():
        return 0.0, 0.0
    err = np.abs(np.asarray(got).astype(LD) - dJ)[nz]
    return float((err / tol[nz]).max()), float((tol[nz] / np.maximum(np.abs(dJ[nz]), LD(1e-300))).max())
