"""Numpy twin of the quadratic bottom drag of the implicit vertical momentum pass (moka_set_quadratic_bottom_drag, moka_bottom_speed), on
top of momentum_vmix_twin, and a long-double restatement that forms the kinetic energy densely and solves the column matrix with no
increment form.  momentum_vmix_twin is untouched: `apply` hands its pass_cols a per-edge q, QuadraticDragTwin wraps its twin.

Recipe (include/moka_hip.h), for an edge e the pass computes, n = min(maxLevelEdgeTop[e], K) >= 1, kb = n - 1, x = u*, (c1, c2) =
cellsOnEdge[e], kc = (0.25 * dcEdge) * dvEdge, invArea = 1 / areaCell, every operation rounded once:
    for c in (c1, c2):  acc = 0.0
        for slot i < nEdgesOnCell[c], e' = edgesOnCell[c, i]:  if min(maxLevelEdgeTop[e'], K) > kb:  acc = acc + (kc[e'] * x[kb,e']) * x[kb,e']
        KE_c = acc * invArea[c]
    sp[e] = sqrt(KE_c1 + KE_c2);   rq = r + Cd * sp[e];   q_e = dt * rq
and momentum_vmix_twin's recipe with q_e where it has q.  Drag is on when r != 0 or Cd != 0.  u[kb,e'] of a slot that fails the depth
test is not read (`bottom_speed` puts 0.0 in its place before any arithmetic; `bottom_speed_wrong` is the deliberate mistake that reads
it).  Cd == 0 is momentum_vmix_twin.apply itself.

Long double (`speed_ld`, `bounds`): KE[c,k] = (sum over ALL edges e' with c in cellsOnEdge[e'] and min(mlt[e'], K) > k of
dcEdge dvEdge u[k,e']^2 / 4) / areaCell[c], scattered from the edges through cellsOnEdge -- no slot of edgesOnCell is visited --,
sp = sqrt(KE[c1,kb] + KE[c2,kb]), q_e = dt (r + Cd sp); A = A0 + q_e e_{n-1} e_{n-1}^T with (A0, A0^-1) = momentum_vmix_twin.dense_ld(h,
s) and the rank-one update of the inverse, A^-1 = A0^-1 - q_e A0^-1 e e^T A0^-1 / (1 + q_e e^T A0^-1 e), all in long double (dense_ld
itself takes one q for all columns, and takes it as a double).

Round-off count, m = maxEdges, q^ the twin's double, q the long-double one.  Every term of acc is >= 0, so relative errors do not grow
in the sums:
  a term (kc x) x: the two products of kc (0.25 * dcEdge counted although it is exact) and the two products with x: 4;
  the additions of acc: the first, to 0.0, is exact, at most m - 1 more touch a term: m - 1;
  invArea: the division and the product: 2;  KE_c1 + KE_c2: 1.          C_KE = m + 6 roundings on sp^2
  the square root halves the relative error and rounds once:          C_SP = C_KE / 2 + 1
  rq = r + Cd * sp: the product and the addition, on non-negative terms: C_SP + 2;   q = dt * rq:  C_Q = C_SP + 3
so |q^ - q| <= C_Q 2^-53 q.  The twin solves with q^ and momentum_vmix_twin's count holds for it as it stands (C_SOLVE on the solve's
residual, C_R on the right-hand side, one rounding of |u^|); A(q) u = h o x + b e_0 has a right-hand side free of q, hence
u(q^) - u(q) = -(q^ - q) A(q)^-1 e_{n-1} u(q^)[n-1], which joins the chain as one more right-hand-side term of C_Q roundings:
  |u^ - u| <= 2^-53 (|A^-1| (C_SOLVE (|A||z^| + |R^|) + C_R mR + C_Q q |u^[n-1]| e_{n-1}) + |u^|).
Momentum: the twin's own q^ is one double per column, so the budget of momentum_vmix_twin holds letter for letter with it:
  |sum_k h u^ - sum_k h x - (b - q^ u^[n-1])| <= 2^-53 (sum_k (C_SOLVE (|A||z^| + |R^|) + C_R mR + h |u^|)[k] + q^ |u^[n-1]|).

Exact decay (`decay_*`).  "planar-f0", K = 1, uniform h, flat ssh, u_e = U . n_e, nuV = 0, r = 0, no stress.  On regular hexagons
sum_m (U . n_m)^2 = 3 |U|^2, dvEdge = dcEdge / sqrt 3 and areaCell = sqrt 3 dcEdge^2 / 2 give KE_c = |U|^2 / 2 and sp = |U|; the
n == 1 row of the pass is u_new = x - q x / (h + q) = x h / (h + q), every edge shrinks by the same factor and
1 / |U_new| = 1 / |U| + dt Cd / h, the exact solution of d|U|/dt = -Cd |U|^2 / h sampled at the steps:
    u_e(N) F = u_e(0),   F = 1 + N dt Cd |U_0| / h.
The map u -> u h / (h + dt Cd u) has slope h^2 / (h + q)^2 <= 1: an error made in one step is not amplified by the later ones, so the
per-step errors add, and the left-hand side multiplies their sum by F.  `decay_bound` counts them to first order, per step, in units
of 2^-53 |U_0| (every |u_e| <= |U|, and |U| only shrinks; rho = dt Cd |U_0| / h >= q / h bounds the increment q x / (h + q) <= rho |U|):
  E0 = 8: what separates the stored u_e(0) and metric from an exactly uniform flow on exact hexagons, relative to |U| -- angleEdge's
  rounding through cos and sin (3), cos, sin, the two products and the sum (5);
  the drag row: q^ against dt Cd |U|: C_Q, E0 for sp of the stored flow, 2 for the rounded dcEdge, dvEdge, areaCell in sp (3 on sp^2),
  and d = h + q, q * x, r / d, x + inc: 4 -- on an increment of at most |U|: C_Q + E0 + 6;
  the dycore: the flow is discretely non-divergent and ssh is flat, so every tendency is 0 in exact arithmetic.  A stage's
  tendLayerThickness is (sum of six (dvEdge sign) (h_e u_e)) invArea: h_e 2, the flux product 1, the metric product 1, five additions,
  the area product 1: 10 roundings on six terms of at most dvEdge h |U| each, and the flow's own E0 on the same six terms; invArea =
  2 / (sqrt 3 dcEdge^2) and dvEdge = dcEdge / sqrt 3: a residual of at most D = (10 + E0) * 6 * dvEdge * invArea * h |U| = 4 (10 + E0)
  h |U| / dcEdge per unit time, the four stages weighing dt in total: after j steps |ssh| and |h - h_0| <= j D dt, in 2^-53.
  tendNormalVelocity = -g (ssh2 - ssh1) / dcEdge is at most 2 g |ssh| / dcEdge (its own roundings are relative to that: second order),
  so step j adds at most dt * 2 g j D dt / dcEdge = 8 j (10 + E0) G |U|,  G = g h dt^2 / dcEdge^2;
  the RK4 combination of u rounds at most 5 times on |U|: 5;
  h_e = 0.5 * (h1 + h2) of the drifted thickness: (1 + j D dt / h) on the increment: 1 + 4 j (10 + E0) (dt |U_0| / dcEdge) rho.
  Over N steps:  N (C_Q + E0 + 6 + 5 + 1) + N (N + 1) (10 + E0) (4 G + 2 rho dt |U_0| / dcEdge).
The gravity waves that carry those residuals are not amplified by RK4 at this dt (|R(i w dt)| <= 1 for w dt <= 2.8; here
w dt <= 2 sqrt(3 G) << 1); the count takes every residual at full weight in every later step, which is what N (N + 1) says.
Nothing here is measured from the twin or the device."""
import numpy as np

import momentum_vfield_twin as mf
import momentum_vmix_twin as mv
import tracer_cases as tc
import tracer_vmix_twin as tv

LD = mv.LD
U53 = mv.U53
C_SOLVE = mv.C_SOLVE
C_R = mv.C_R


def counts(mesh):
    """(C_KE, C_SP, C_Q) of the docstring for a mesh."""
    m = int(np.asarray(mesh.edgesOnCell).shape[1])
    c_ke = m + 6
    c_sp = c_ke / 2 + 1
    return c_ke, c_sp, c_sp + 3


# ---- the bottom speed ---------------------------------------------------------------------------------------------------------------
def _stencil(mesh):
    eoc = np.asarray(mesh.edgesOnCell, dtype=np.int64) - 1
    cnt = np.asarray(mesh.nEdgesOnCell, dtype=np.int64)
    kc = (0.25 * np.asarray(mesh.dcEdge, dtype=np.float64)) * np.asarray(mesh.dvEdge, dtype=np.float64)
    inv = 1.0 / np.asarray(mesh.areaCell, dtype=np.float64)
    return eoc, cnt, kc, inv


def _speed(u, mlt, mesh, depth_test):
    u = np.asarray(u, dtype=np.float64)
    nE, K = u.shape
    nn = np.minimum(np.asarray(mlt, dtype=np.int64) * np.ones(nE, dtype=np.int64), K)
    eoc, cnt, kc, inv = _stencil(mesh)
    c1, c2 = mv.edge_cells(mesh)
    on = nn >= 1
    kb = np.where(on, nn - 1, 0)
    ke = []
    for c in (c1, c2):
        acc = np.zeros(nE)
        for i in range(eoc.shape[1]):
            valid = on & (i < cnt[c])
            ep = np.where(valid, eoc[c, i], 0)
            ok = valid & (nn[ep] > kb) if depth_test else valid
            x = np.where(ok, u[ep, kb], 0.0)              # a slot that fails the test contributes no operand at all
            acc = np.where(ok, acc + (kc[ep] * x) * x, acc)
        ke.append(acc * inv[c])
    with np.errstate(invalid="ignore"):
        return np.where(on, np.sqrt(ke[0] + ke[1]), 0.0)


def bottom_speed(u, mlt, mesh):
    """sp[e] of the recipe from a (nEdges, K) field; 0.0 for edges with no active level."""
    return _speed(u, mlt, mesh, True)


def bottom_speed_wrong(u, mlt, mesh):
    """The deliberate mistake: the `> kb` test is dropped, u[kb,e'] is read at every listed edge."""
    return _speed(u, mlt, mesh, False)


def speed_ld(u, mlt, mesh):
    """sp in long double, KE scattered from the edges through cellsOnEdge (no slot of edgesOnCell is visited)."""
    u = np.asarray(u, dtype=np.float64)
    nE, K = u.shape
    nn = np.minimum(np.asarray(mlt, dtype=np.int64) * np.ones(nE, dtype=np.int64), K)
    c1, c2 = mv.edge_cells(mesh)
    live = np.arange(K)[None, :] < nn[:, None]
    dens = (np.asarray(mesh.dcEdge).astype(LD) * np.asarray(mesh.dvEdge).astype(LD) / 4)[:, None] * np.where(live, u, 0.0).astype(LD) ** 2
    KE = np.zeros((mesh.nCells, K), dtype=LD)
    np.add.at(KE, c1, dens)
    np.add.at(KE, c2, dens)
    KE = KE / np.asarray(mesh.areaCell).astype(LD)[:, None]
    kb = np.maximum(nn - 1, 0)
    return np.where(nn >= 1, np.sqrt(KE[c1, kb] + KE[c2, kb]), LD(0))


# ---- the pass -----------------------------------------------------------------------------------------------------------------------
def pass_on(nu, drag, tau, mlt, cd=0.0):
    return cd != 0.0 or mv.pass_on(nu, drag, tau, mlt)


def apply(u, h, mlt, c1, c2, dt, nu, drag=0.0, tau=None, cd=0.0, mesh=None, speed=bottom_speed, fld=None):
    """(the pass on a whole (nEdges, K) field, the sp it used -- zeros without Cd or when nothing is launched).  cd == 0:
    momentum_vmix_twin.apply (momentum_vfield_twin.apply with a viscosity field `fld`, which sets nu aside as it does there)."""
    if cd == 0.0:
        return mf.apply(u, h, mlt, c1, c2, dt, nu, drag, tau, fld), np.zeros(u.shape[0])
    nu, fld = mf.taken(nu, fld, mlt)
    K = u.shape[1]
    out = u.copy()
    if dt == 0.0:
        return out, np.zeros(u.shape[0])
    sp = speed(u, mlt, mesh)
    rq = np.float64(drag) + np.float64(cd) * sp
    q = np.float64(dt) * rq
    s = np.float64(dt) * np.float64(nu)
    st = mv.stress_on(tau, mlt)
    nn = np.minimum(np.asarray(mlt, dtype=np.int64) * np.ones(u.shape[0], dtype=np.int64), K)
    for n in np.unique(nn):
        if n < 1:
            continue
        idx = np.nonzero(nn == n)[0]
        he = 0.5 * (h[c1[idx], :n] + h[c2[idx], :n])
        b = np.float64(dt) * np.asarray(tau, dtype=np.float64)[idx] if st else None
        out[idx, :n] = mv.pass_cols(he, u[idx, :n], s if fld is None else np.float64(dt) * fld[idx, :n - 1], q[idx], b)
    return out, sp


def dense_ld(h, s, q):
    """(A, Ainv) in long double of columns h (ncol, n) with one q (long double or double) per column: momentum_vmix_twin.dense_ld
    without a drag and the rank-one update."""
    A, inv = mv.dense_ld(h, s)
    q = np.asarray(q).astype(LD)
    A = A.copy()
    A[:, -1, -1] += q
    col = inv[:, :, -1]                                   # A0^-1 e   (A0 is symmetric: e^T A0^-1 is its transpose)
    inv = inv - (q / (1 + q * col[:, -1]))[:, None, None] * col[:, :, None] * col[:, None, :]
    return A, inv


def bounds(h, x, s, q, q_ld, b, c_q):
    """(u^, u, err, mom) of columns of one depth: the twin's result with its doubles q, the long-double one with q_ld, the docstring's
    bound on |u^ - u| per element and on the momentum identity per column, without the factor 2^-53."""
    w, d, R = mv.rhs_cols(h, x, s, q, b)
    z = mv.solve_cols(w, d, R)
    new = x + z
    A, inv = dense_ld(h, s, q_ld)
    res = tv.mv(np.abs(A), np.abs(z)) + np.abs(R).astype(LD)
    inner = C_SOLVE * res + C_R * mv.rhs_abs(h, x, s, q, b)
    mom = (inner + np.asarray(h).astype(LD) * np.abs(new)).sum(axis=1) + np.asarray(q).astype(LD) * np.abs(new[:, -1])
    inner[:, -1] += c_q * np.asarray(q_ld).astype(LD) * np.abs(new[:, -1])
    err = tv.mv(np.abs(inv), inner) + np.abs(new)
    rhs = np.asarray(h).astype(LD) * np.asarray(x).astype(LD)
    if b is not None:
        rhs[:, 0] += np.asarray(b).astype(LD)
    return new, tv.mv(inv, rhs), err, mom


# ---- the twins ----------------------------------------------------------------------------------------------------------------------
class QuadraticDragTwin:
    """momentum_vmix_twin.MomentumVmixTwin (`mt`) with a Cd: its step, then the pass with the per-edge q.  nu, drag and tau live in
    `mt`; cd and a viscosity field `fld` (None: the scalar nu) here; `sp` is what the last pass used.  `speed`: bottom_speed, or
    bottom_speed_wrong for the deliberate mistake."""

    def __init__(self, mt, cd=0.0, speed=bottom_speed, fld=None):
        self.mt, self.cd, self.speed, self.fld = mt, float(cd), speed, fld
        self.mesh = mt.tw.om.mesh
        self.sp = np.zeros(self.mesh.nEdges)

    def mix(self, u, h, dt):
        m = self.mt
        out, sp = apply(u, h, m.mlt, m.c1, m.c2, dt, m.nu, m.drag, m.tau, self.cd, self.mesh, self.speed, self.fld)
        drag = self.cd != 0.0 or m.drag != 0.0
        on = drag or mf.pass_on(m.nu, m.drag, m.tau, m.mlt, self.fld)
        if on and dt != 0.0 and not (u.shape[1] < 2 and not drag and not mv.stress_on(m.tau, m.mlt)):
            self.sp = sp                                   # a pass was launched: `sp` is what it used (zeros without Cd)
        return out

    def step_rk4(self, st, phis, dt):
        self.mt.tw.step_rk4(st, phis, dt)
        st.u[1] = self.mix(st.u[1], st.h[1], dt)

    def step_s13(self, st, dt, nl=None):
        if nl is None:
            st.step_rk4_s13(dt)
        else:
            nl.step_rk4_s13(st, dt)
        st.u[1][...] = self.mix(st.u[1], st.h[1], dt)


def quadratic_twin(meshname, K, mode="linear", partial=False, mlt=None, nu=0.0, drag=0.0, tau=None, cd=0.0, speed=bottom_speed):
    return QuadraticDragTwin(mv.momentum_twin(meshname, K, mode, partial, mlt, nu, drag, tau), cd, speed)


# ---- shared parameters --------------------------------------------------------------------------------------------------------------
def cd_of(K, dt, ratio=0.5):
    """Cd with dt Cd sp / hm = ratio at sp = 1 m/s (u of tc.state_of is uniform in [-1, 1]: sp is of order one), hm = 1000 / K: the
    quadratic term is as visible as momentum_vmix_twin.coefficients' linear one."""
    return ratio * (1000.0 / K) / dt


# ---- exact decay ----------------------------------------------------------------------------------------------------------------------
DECAY_STEPS = 10
DECAY_E0 = 8
G_ACC = 9.80616


def decay_state():
    """(mesh, (ssh, u, h, rest), |U_0|) of the exact-decay case: tc.eigenmode_state at K = 1."""
    mesh, state, _ = tc.eigenmode_state(1)
    return mesh, state, float(np.hypot(*tc.EIG_U))


def decay_twin(cd):
    """The twin chain over the case's own mesh constants: the resting thickness is the uniform h, so ssh is flat (tc.oracle_mesh takes
    tc.state_of's random one)."""
    import oracle as orc
    mesh, (_, _, _, rest), _ = decay_state()
    om = orc.OracleMesh(mesh, 1, resting_thickness_sum=rest.sum(1), max_level_edge_top=1)
    return QuadraticDragTwin(mv.MomentumVmixTwin(tv.VmixTwin(om, om, [])), cd)


def decay_cd(nsteps=DECAY_STEPS):
    """Cd with N dt Cd |U_0| / h = 1: the flow halves over the case's steps."""
    return tc.EIG_H / (nsteps * tc.EIG_DT * float(np.hypot(*tc.EIG_U)))


def decay_factor(cd, nsteps=DECAY_STEPS):
    """F = 1 + N dt Cd |U_0| / h, in long double."""
    return 1 + LD(nsteps) * LD(tc.EIG_DT) * LD(cd) * np.hypot(LD(tc.EIG_U[0]), LD(tc.EIG_U[1])) / LD(tc.EIG_H)


def decay_bound(mesh, cd, nsteps=DECAY_STEPS):
    """The docstring's count of the summed per-step errors, in units of 2^-53 |U_0| (the assertion multiplies it by F)."""
    c_q = counts(mesh)[2]
    U0 = float(np.hypot(*tc.EIG_U))
    G = G_ACC * tc.EIG_H * tc.EIG_DT ** 2 / tc.EIG_DC ** 2
    rho = tc.EIG_DT * cd * U0 / tc.EIG_H
    return (nsteps * (c_q + DECAY_E0 + 6 + 5 + 1)
            + nsteps * (nsteps + 1) * (10 + DECAY_E0) * (4 * G + 2 * rho * tc.EIG_DT * U0 / tc.EIG_DC))


def decay_check(u_final, u_start, mesh, cd, label, nsteps=DECAY_STEPS):
    """Assert |u_e(N) F - u_e(0)| <= F * decay_bound * 2^-53 * |U_0| on every edge, and that the same bound would refuse a run without
    the drag and one with the linearised drag r = Cd |U_0| (u_e(N) = u_e(0) / (1 + dt r / h)^N).  Prints every figure."""
    U0 = float(np.hypot(*tc.EIG_U))
    F = decay_factor(cd, nsteps)
    tol = F * LD(decay_bound(mesh, cd, nsteps)) * LD(U53) * LD(U0)
    a, b = np.asarray(u_final)[:, 0].astype(LD), np.asarray(u_start)[:, 0].astype(LD)
    dev = np.abs(a * F - b).max()
    lin = (1 + LD(tc.EIG_DT) * LD(cd) * LD(U0) / LD(tc.EIG_H)) ** nsteps
    gap_none, gap_lin = np.abs(b * F - b).max(), np.abs(b / lin * F - b).max()
    print(f"{label}: F = {float(F):.6f}, max |u(N) F - u(0)| = {float(dev):.3e}, tolerance = {float(tol):.3e} "
          f"({decay_bound(mesh, cd, nsteps):.1f} x 2^-53 |U_0| x F), gap without drag = {float(gap_none):.3e}, "
          f"gap to the linearised drag = {float(gap_lin):.3e}")
    assert dev <= tol
    assert gap_none >= 1e6 * tol and gap_lin >= 1e6 * tol
    return float(dev)
