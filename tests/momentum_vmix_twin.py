"""Numpy twin of the implicit vertical mixing of momentum with a surface stress and a linear bottom drag (moka_set_vertical_viscosity,
moka_surface_stress_upload), and a long-double restatement that builds the column matrix densely and solves it with no increment form.
Sits on top of the tracer twin chain: the RK4 step is tracer_vmix_twin.VmixTwin's over tracer_cases.twin_of, untouched; the pass
follows it on st.u[1] with st.h[1].  The pass alone is offered behind the oracle's 13-stream steps too.

Recipe (include/moka_hip.h), per edge e with n = min(maxLevelEdgeTop[e], K) and c1, c2 = cellsOnEdge, every operation rounded once:
    x[k] = u*[k,e];  h[k] = 0.5 * (h_new[k,c1] + h_new[k,c2]);  s = dt * nuV;  q = dt * r;  b = dt * tau[e]
    w[k] = s / (0.5 * (h[k] + h[k+1]));   d[0] = h[0] + w[0];  d[k] = (h[k] + w[k-1]) + w[k];  d[n-1] = h[n-1] + w[n-2]   (n == 1: d[0] = h[0])
    drag on (r != 0):  d[n-1] = d[n-1] + q
    R = Lv(x)  (n == 1: R[0] = 0.0);   stress present: R[0] = R[0] + b;   drag on: R[n-1] = R[n-1] - q * x[n-1]
    u_new = x + Solve(R)  (n == 1: y[0] = R[0] / d[0])
with weights, Lv and Solve those of tracer_vmix_twin.  A column is computed when n >= 2, or when n == 1 and drag or stress is on.  A
stress that is zero at every edge with n >= 1 counts as absent; the pass is on when nuV != 0, r != 0 or a stress is present in that sense.

Long double (`dense_ld`): A = diag(h) + s W + q e_{n-1} e_{n-1}^T with tracer_vmix_twin.dense_ld's W, h formed in long double from the
doubles of the two cells; A u = h o x + b e_0 solved by Gaussian elimination without pivoting (A is strictly diagonally dominant).

Round-off count against that solution, per element, u^ the twin's result, z^ its Solve, R^ its right-hand side:
  the solve: |A z^ - R^| <= (C_BR + 1) 2^-53 (|A||z^| + |R^|): tracer_vmix_twin's C_BR, whose count of the entries of A (4) grows by
  the one addition of q to d[n-1];
  the right-hand side: a term w (x' - x) of Lv carries w's addition and division, the difference and the product (4), the sum of a
  row's two terms one more (5), the stress addition one more (6), the drag's product and subtraction two more (8); every term of
  mR = mLv(x) + |b| e_0 + q |x[n-1]| e_{n-1} therefore carries at most C_R = 8 roundings;
  the final addition x + z^: one rounding of |u^|.
  |u^ - u| <= 2^-53 (|A^-1| ((C_BR + 1) (|A||z^| + |R^|) + C_R mR) + |u^|).
Momentum: 1^T A = h^T + q e_{n-1}^T and Lv with the twin's own w telescopes to 0 in exact arithmetic, so
  |sum_k h u^ - sum_k h x - (b - q u^[n-1])| <= 2^-53 (sum_k ((C_BR + 1) (|A||z^| + |R^|) + C_R mR + h |u^|)[k] + q |u^[n-1]|)."""
import numpy as np

import tracer_cases as tc
import tracer_vmix_twin as tv

LD = tv.LD
U53 = tv.U53
C_SOLVE = tv.C_BR + 1
C_R = 8


# ---- the recipe on columns of one depth: h, x (ncol, n); s, q scalars (q None: no drag); b (ncol,) or None (no stress) ------------------
def rhs_cols(h, x, s, q=None, b=None):
    """(w, d, R) as the recipe forms them; n == 1: w is empty."""
    n = h.shape[1]
    if n == 1:
        w = np.empty((h.shape[0], 0))
        d = h.copy()
        R = np.zeros_like(x)
    else:
        w = tv.weights(h, s)
        d = tv.diagonal(h, w)
        R = tv.Lv(w, x)
    if q is not None:
        d[:, -1] = d[:, -1] + q
    if b is not None:
        R[:, 0] = R[:, 0] + b
    if q is not None:
        R[:, -1] = R[:, -1] - q * x[:, -1]
    return w, d, R


def solve_cols(w, d, R):
    return R / d if R.shape[1] == 1 else tv.solve(w, d, R)


def pass_cols(h, x, s, q=None, b=None):
    w, d, R = rhs_cols(h, x, s, q, b)
    return x + solve_cols(w, d, R)


def rhs_abs(h, x, s, q=None, b=None):
    """mR of the docstring, in long double."""
    m = np.zeros(x.shape, dtype=LD)
    if h.shape[1] > 1:
        m += tv.Lv_abs(tv.weights(h, s), x)
    if b is not None:
        m[:, 0] += np.abs(b)
    if q is not None:
        m[:, -1] += q * np.abs(x[:, -1])
    return m


def stress_on(tau, mlt):
    return tau is not None and bool(np.any(np.asarray(tau)[np.asarray(mlt) >= 1] != 0.0))


def pass_on(nu, drag, tau, mlt):
    return nu != 0.0 or drag != 0.0 or stress_on(tau, mlt)


def edge_cells(mesh):
    coe = np.asarray(mesh.cellsOnEdge, dtype=np.int64) - 1
    return coe[:, 0], coe[:, 1]


def apply(u, h, mlt, c1, c2, dt, nu, drag=0.0, tau=None):
    """The pass on a whole (nEdges, K) field over the (nCells, K) thickness: a new array; levels k >= n, edges that are not computed
    and the cells of edges with n == 0 are not read."""
    K = u.shape[1]
    out = u.copy()
    if dt == 0.0 or not pass_on(nu, drag, tau, mlt):
        return out
    s = np.float64(dt) * np.float64(nu)
    q = np.float64(dt) * np.float64(drag) if drag != 0.0 else None
    st = stress_on(tau, mlt)
    nn = np.minimum(np.asarray(mlt, dtype=np.int64), K)
    for n in np.unique(nn):
        if n < 1 or (n == 1 and q is None and not st):
            continue
        idx = np.nonzero(nn == n)[0]
        he = 0.5 * (h[c1[idx], :n] + h[c2[idx], :n])
        b = np.float64(dt) * np.asarray(tau, dtype=np.float64)[idx] if st else None
        out[idx, :n] = pass_cols(he, u[idx, :n], s, q, b)
    return out


# ---- long double ------------------------------------------------------------------------------------------------------------------
def dense_ld(h, s, q=None):
    """(A, Ainv) in long double of columns h (ncol, n) (doubles or long doubles), n >= 1."""
    h = np.asarray(h).astype(LD)
    ncol, n = h.shape
    k = np.arange(n)
    A = np.zeros((ncol, n, n), dtype=LD)
    A[:, k, k] = h
    if n > 1:
        iw = LD(float(s)) / ((h[:, :-1] + h[:, 1:]) / 2)
        A[:, k[:-1], k[:-1]] += iw
        A[:, k[1:], k[1:]] += iw
        A[:, k[:-1], k[1:]] = -iw
        A[:, k[1:], k[:-1]] = -iw
    if q is not None:
        A[:, n - 1, n - 1] += LD(float(q))
    M = A.copy()
    inv = np.zeros_like(A)
    inv[:, k, k] = 1
    for p in range(n):
        piv = M[:, p, p][:, None].copy()
        M[:, p, :] = M[:, p, :] / piv
        inv[:, p, :] = inv[:, p, :] / piv
        for r in range(n):
            if r != p:
                f = M[:, r, p][:, None].copy()
                M[:, r, :] -= f * M[:, p, :]
                inv[:, r, :] -= f * inv[:, p, :]
    return A, inv


def pass_ld(h, x, s, q=None, b=None, dense=None):
    """u = A^-1 (h o x + b e_0), no increment form."""
    A, inv = dense if dense is not None else dense_ld(h, s, q)
    rhs = np.asarray(h).astype(LD) * np.asarray(x).astype(LD)
    if b is not None:
        rhs[:, 0] += np.asarray(b).astype(LD)
    return tv.mv(inv, rhs)


def bounds(h, x, s, q=None, b=None):
    """(u^, u, err, mom) of columns of one depth: the twin's result, the long-double one, the docstring's bound on |u^ - u| per element
    and on the momentum identity per column, without the factor 2^-53."""
    w, d, R = rhs_cols(h, x, s, q, b)
    z = solve_cols(w, d, R)
    new = x + z
    A, inv = dense_ld(h, s, q)
    res = tv.mv(np.abs(A), np.abs(z)) + np.abs(R).astype(LD)
    inner = C_SOLVE * res + C_R * rhs_abs(h, x, s, q, b)
    err = tv.mv(np.abs(inv), inner) + np.abs(new)
    mom = (inner + np.asarray(h).astype(LD) * np.abs(new)).sum(axis=1) + (LD(float(q)) * np.abs(new[:, -1]) if q is not None else 0)
    return new, pass_ld(h, x, s, q, b, (A, inv)), err, mom


# ---- the twins --------------------------------------------------------------------------------------------------------------------
class MomentumVmixTwin:
    """The tracer chain's step (`tw`: a tv.VmixTwin) followed by the pass; nu, drag and tau may be replaced between steps."""

    def __init__(self, tw, nu=0.0, drag=0.0, tau=None):
        self.tw, self.nu, self.drag, self.tau = tw, float(nu), float(drag), tau
        self.mlt = np.asarray(tw.om.arrays["maxLevelEdgeTop"])
        self.c1, self.c2 = edge_cells(tw.om.mesh)

    def mix(self, u, h, dt):
        return apply(u, h, self.mlt, self.c1, self.c2, dt, self.nu, self.drag, self.tau)

    def step_rk4(self, st, phis, dt):
        """st: a del4_twin.TwinState; phis = [previous, current] tracer lists (may be empty)."""
        self.tw.step_rk4(st, phis, dt)
        st.u[1] = self.mix(st.u[1], st.h[1], dt)

    def step_s13(self, st, dt, nl=None):
        """st: an oracle.OracleState (its arrays are updated in place); nl: an oracle.OracleNonlinear, or None for the linear terms."""
        if nl is None:
            st.step_rk4_s13(dt)
        else:
            nl.step_rk4_s13(st, dt)
        st.u[1][...] = self.mix(st.u[1], st.h[1], dt)


def momentum_twin(meshname, K, mode="linear", partial=False, mlt=None, nu=0.0, drag=0.0, tau=None):
    return MomentumVmixTwin(tv.vmix_twin(meshname, K, mode, partial, mlt), nu, drag, tau)


def form_of(K, generic=False):
    """Which form serves a K: 1 the tile form, 2 the column form (csrc/momentum_vmix.hip takes tracer_vmix.hip's vmix_kernel with three
    sets; K == 1 has no tile)."""
    return 1 if tv.tile_columns(K, generic) else 2


# ---- shared parameters ------------------------------------------------------------------------------------------------------------
def coefficients(meshname, K, sh2=4.0, drag_ratio=0.5):
    """(nuV, r) with s / hm^2 = sh2 and q / hm = drag_ratio for hm = 1000 / K."""
    hm, dt = 1000.0 / K, tc.dt_of(meshname)
    return sh2 * hm * hm / dt, drag_ratio * hm / dt


def stress_field(mesh, K, seed=31, zeros=False):
    """tau with dt tau / hm of order one (the increment of the top level is visible); zeros: every third edge exactly 0.0."""
    rng = np.random.default_rng(seed)
    tau = rng.uniform(-1.0, 1.0, mesh.nEdges) * (1000.0 / K) / 2.0
    if zeros:
        tau[::3] = 0.0
    return tau
