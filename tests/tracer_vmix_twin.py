"""Numpy twins of the implicit vertical diffusion of passive tracers (moka_set_tracer_vertical_diffusion), forwards and backwards, and
a long-double restatement that builds the column matrix densely.  Wraps tests/tracer_kgrad_twin.py (the top of the tracer twin chain):
the RK4 step and its transpose are untouched, the vertical solve follows the step and precedes the reversed step.

Recipe (include/moka_hip.h), per tracer with kappaV != 0 and column with n = nLev[c] >= 2 active levels, s = dt * kappaV, every
operation rounded once:
    w[k] = s / (0.5 * (h[k] + h[k+1]));   d[0] = h[0] + w[0];  d[k] = (h[k] + w[k-1]) + w[k];  d[n-1] = h[n-1] + w[n-2]
    Lv(v)[k] = w[k-1] * (v[k-1] - v[k]) + w[k] * (v[k+1] - v[k])            (end rows: the one term that exists)
    Solve(r): beta = d[0]; y[0] = r[0] / beta;  g[k-1] = w[k-1] / beta; beta = d[k] - w[k-1] * g[k-1]; y[k] = (r[k] + w[k-1] * y[k-1]) / beta
              z[n-1] = y[n-1];  z[k] = y[k] + g[k] * z[k+1]
    forward: phi_new = x + Solve(Lv(x))          reverse: X <- X + Lv(Solve(X))
The twin is vectorised over the columns of one depth and serial in k.  nLev[c] is taken from the twin's own slot masks (the number of
levels at which any slot of the cell is active), not from the plan.

Long double (`dense_ld`): A = diag(h) + s W with W[k,k] += 1/hm[k], W[k+1,k+1] += 1/hm[k], W[k,k+1] = W[k+1,k] = -1/hm[k],
hm[k] = (h[k] + h[k+1]) / 2, formed and inverted (Gauss-Jordan, no pivoting: A is strictly diagonally dominant) in long double from
the doubles h and s.  Forward S = A^-1 diag(h), reverse S^T = diag(h) A^-1.

Round-off count C_BR of one solve, for |A z^ - r| <= C_BR 2^-53 (|A| |z^| + |r|) per element with A the long-double matrix, r the
right-hand side as the twin formed it and z^ the twin's solution:
  the factorisation and the two sweeps: the sweep is the Crout form of the LU factorisation of a tridiagonal matrix (L = bidiag(-w, beta),
  U = unit bidiag(-g)); Higham, Accuracy and Stability, Theorems 9.12 and 9.14: (A + dA) z^ = r with |dA| <= (4u + 3u^2 + u^3) |L^||U^|
  and |L^||U^| <= 3 |A| for a matrix diagonally dominant by rows: 12;
  the entries of A as the twin forms them against the long-double ones: w takes an addition and a division (0.5 * is exact), d two
  more additions, every term positive: 4;
  the house slack of 5 on top (tracer_biharmonic_twin.SLACK).   C_BR = 12 + 4 + 5 = 21.
The forward error follows: z^ - z = A^-1 (A z^ - r), so |z^ - z| <= C_BR 2^-53 |A^-1| (|A| |z^| + |r|).
Lv itself: a row is two products of a difference (2 roundings each) and one addition: C_LV = 3 on the magnitude
mLv(v)[k] = w[k-1] (|v[k-1]| + |v[k]|) + w[k] (|v[k+1]| + |v[k]|).
Content: 1^T W = 0, so sum_k h z = sum_k (A z)[k] = sum_k r[k] + sum_k (A z^ - r)[k], and sum_k Lv(x)[k] telescopes to 0 exactly in
exact arithmetic: |sum_k h phi_new - sum_k h x| <= 2^-53 sum_k (C_BR (|A||z^| + |r|) + C_LV mLv(x) + h |phi_new|)[k]  (the last term:
the final addition x + z)."""
import numpy as np

import tracer_adjoint_twin as ta
import tracer_biharmonic_twin as tb
import tracer_cases as tc
import tracer_kgrad_twin as tk
import tracer_source_twin as ts
import trisk_reference as tr
from del4_twin import TwinState

LD = tr.LD
U53 = 2.0 ** -53
C_BR = 12 + 4 + tb.SLACK
C_LV = 3
assert C_BR == 21

# s / hm^2 of up to nine tracers (hm ~ 1000 / K): pairwise distinct apart from the exact zero (the second), up to 30
VFACT9 = (30.0, 0.0, 7.0, 11.0, 3.0, 19.0, 0.5, 23.0, 13.0)


def kappavs(meshname, K, n, factors=VFACT9):
    k = [f * (1000.0 / K) ** 2 / tc.dt_of(meshname) for f in factors[:n]]
    assert len(set(k)) == n and (n < 2 or k.count(0.0) == 1)
    return k


def column_mlt(mesh, K, seed=12):
    """A maxLevelEdgeTop from a sea floor: every cell gets a depth (the first cells 0, 1, 2, 3 and K; of the others half the full K, half
    uniform in 0..K) and an edge the smaller depth of its two cells, so that nLev[c] <= depth[c] and columns of depth 0, 1 and 2 exist."""
    rng = np.random.default_rng(seed)
    depth = np.where(rng.random(mesh.nCells) < 0.5, K, rng.integers(0, K + 1, mesh.nCells))
    depth[:5] = (0, 1, min(2, K), min(3, K), K)
    coe = np.asarray(mesh.cellsOnEdge, dtype=np.int64) - 1
    return np.minimum(depth[coe[:, 0]], depth[coe[:, 1]]).astype(np.int32)


# ---- the recipe on columns of one depth: h, x (ncol, n) ---------------------------------------------------------------------------
def weights(h, s):
    return np.float64(s) / (0.5 * (h[:, :-1] + h[:, 1:]))


def diagonal(h, w):
    d = np.empty_like(h)
    d[:, 0] = h[:, 0] + w[:, 0]
    d[:, 1:-1] = (h[:, 1:-1] + w[:, :-1]) + w[:, 1:]
    d[:, -1] = h[:, -1] + w[:, -1]
    return d


def Lv(w, v):
    out = np.empty_like(v)
    out[:, 0] = w[:, 0] * (v[:, 1] - v[:, 0])
    out[:, -1] = w[:, -1] * (v[:, -2] - v[:, -1])
    out[:, 1:-1] = w[:, :-1] * (v[:, :-2] - v[:, 1:-1]) + w[:, 1:] * (v[:, 2:] - v[:, 1:-1])
    return out


def Lv_abs(w, v):
    a = np.abs(v)
    out = np.zeros_like(a)
    out[:, :-1] += w * (a[:, 1:] + a[:, :-1])
    out[:, 1:] += w * (a[:, :-1] + a[:, 1:])
    return out


def solve(w, d, r):
    n = r.shape[1]
    y, g = np.empty_like(r), np.empty_like(w)
    beta = d[:, 0].copy()
    y[:, 0] = r[:, 0] / beta
    for k in range(1, n):
        g[:, k - 1] = w[:, k - 1] / beta
        beta = d[:, k] - w[:, k - 1] * g[:, k - 1]
        y[:, k] = (r[:, k] + w[:, k - 1] * y[:, k - 1]) / beta
    z = np.empty_like(r)
    z[:, n - 1] = y[:, n - 1]
    for k in range(n - 2, -1, -1):
        z[:, k] = y[:, k] + g[:, k] * z[:, k + 1]
    return z


def forward_cols(h, x, s):
    w = weights(h, s)
    return x + solve(w, diagonal(h, w), Lv(w, x))


def reverse_cols(h, X, s):
    w = weights(h, s)
    return X + Lv(w, solve(w, diagonal(h, w), X))


def apply(h, x, nlev, s, reverse=False):
    """The vertical pass on a whole (nCells, K) field: columns of depth >= 2, their active levels only; a new array."""
    out = x.copy()
    for n in np.unique(nlev):
        if n < 2:
            continue
        idx = np.nonzero(nlev == n)[0]
        f = reverse_cols if reverse else forward_cols
        out[idx, :n] = f(h[idx, :n], x[idx, :n], s)
    return out


# ---- long double ------------------------------------------------------------------------------------------------------------------
def dense_ld(h, s):
    """(A, Ainv) of columns h (ncol, n) in long double, (ncol, n, n) each."""
    h = np.asarray(h, dtype=np.float64).astype(LD)
    ncol, n = h.shape
    iw = LD(float(s)) / ((h[:, :-1] + h[:, 1:]) / 2)
    A = np.zeros((ncol, n, n), dtype=LD)
    k = np.arange(n)
    A[:, k, k] = h
    A[:, k[:-1], k[:-1]] += iw
    A[:, k[1:], k[1:]] += iw
    A[:, k[:-1], k[1:]] = -iw
    A[:, k[1:], k[:-1]] = -iw
    M = A.copy()
    inv = np.zeros_like(A)
    inv[:, k, k] = 1
    for p in range(n):
        piv = M[:, p, p][:, None].copy()
        M[:, p, :] = M[:, p, :] / piv
        inv[:, p, :] = inv[:, p, :] / piv
        for q in range(n):
            if q != p:
                f = M[:, q, p][:, None].copy()
                M[:, q, :] -= f * M[:, p, :]
                inv[:, q, :] -= f * inv[:, p, :]
    return A, inv


def mv(M, v):
    return np.einsum("cij,cj->ci", M, np.asarray(v).astype(LD))


def forward_ld(h, x, s):
    A, inv = dense_ld(h, s)
    return mv(inv, np.asarray(h).astype(LD) * np.asarray(x).astype(LD))


def reverse_ld(h, X, s):
    A, inv = dense_ld(h, s)
    return np.asarray(h).astype(LD) * mv(inv, X)


# ---- the twins --------------------------------------------------------------------------------------------------------------------
def nlev_of(tw, K):
    """The active depth of every cell from the twin's slot masks: the most levels any of its slots is active at."""
    n = np.zeros(tw.eoc.shape[0], dtype=np.int64)
    for i in range(tw.eoc.shape[1]):
        n = np.maximum(n, np.broadcast_to(tw.slot_mask(i), (tw.eoc.shape[0], K)).sum(axis=1))
    return n


class VmixTwin(tk.KgradTwin):
    """KgradTwin with one vertical diffusivity per tracer: `kappaV` may be replaced between steps; the records gain "kappaV"."""

    def __init__(self, om, base, kappa, kappaV=()):
        super().__init__(om, base, kappa)
        self.kappaV = [float(k) for k in kappaV]
        self._nlev = None

    def nlev(self, K):
        if self._nlev is None:
            self._nlev = nlev_of(self, K)
        return self._nlev

    def kappaV_of(self, j):
        return self.kappaV[j] if j < len(self.kappaV) else 0.0

    def step_rk4(self, st, phis, dt, magnitudes=False):
        # KgradTwin.step_rk4 with a comparison that lets the fill of never-read levels be NaN
        phi0 = [p.copy() for p in phis[1]]
        tb.TracerBiharmonicTwin.step_rk4(self, st, phis, dt, magnitudes)
        self.tape[-1]["pphi"] = []
        for j, p0 in enumerate(phi0):
            stages, new = self.replay(self.tape[-1], j, p0)
            assert np.array_equal(new, phis[1][j], equal_nan=True), ("the replay over the record is not the step", j)
            self.tape[-1]["pphi"].append(stages)
        n = len(phis[1])
        kv = [self.kappaV_of(j) for j in range(n)]
        self.tape[-1]["kappaV"] = kv
        K = st.h[1].shape[1]
        if K < 2 or dt == 0.0:
            return
        for j in range(n):
            if kv[j] != 0.0:                       # a tracer with kappaV == 0 is not touched
                phis[1][j] = apply(st.h[1], phis[1][j], self.nlev(K), np.float64(dt) * np.float64(kv[j]))


class VmixAdjointTwin(tk.KgradAdjointTwin):
    """KgradAdjointTwin whose reversed step begins with S^T on X: every entry into a record goes through `head`."""

    def head(self, rec, x, j):
        kv = rec.get("kappaV", [0.0] * (j + 1))[j]
        K = x.shape[1]
        if kv == 0.0 or K < 2 or rec["dt"] == 0.0:
            return x
        return apply(rec["hn"], x, self.tw.nlev(K), np.float64(rec["dt"]) * np.float64(kv), reverse=True)

    def heads(self, rec, X):
        return [self.head(rec, x, j) for j, x in enumerate(X)]

    def stage_fields(self, rec, x, j, diff, bih):
        return super().stage_fields(rec, self.head(rec, x, j), j, diff, bih)

    def reverse_step(self, rec, X, diff=True, G=None, taus=None):
        return super().reverse_step(rec, self.heads(rec, X), diff, G, taus)

    def reverse_step_bih(self, rec, X, G=None):
        return super().reverse_step_bih(rec, self.heads(rec, X), G)


# ---- shared cases -----------------------------------------------------------------------------------------------------------------
_REFS = {}


def vmix_twin(meshname, K, mode="linear", partial=False, mlt=None):
    t = tc.twin_of(meshname, K, mode, partial, mlt)
    return VmixTwin(t.om, t.base, [])


def reference(meshname, K, mode, partial, nT, nsteps, vert=True, diff=False, bih=False, srcs=(), flags=(), wants=(), fields=None, fill=None):
    """Computed once per case and shared (never modified by a test).  nT fields of tc.distinct_fields(mesh, K, 9) (fields = "unit-first":
    the first is 1 everywhere) over tc.state_of's state, nsteps recorded RK4 steps with kappavs(...) if vert, tc.kappas if diff,
    tb.kappa4s if bih, sources ts.source_fields(...)[j] for j in srcs; then the sweep of ta.seeds with the source gradients `wants` and
    the diffusivity gradients flags = ((j, bits), ...).  partial: False (full columns), True (tc.partial_mlt) or "floor" (column_mlt).
    fill: a value written into every level k >= nLev[c] of the fields and seeds.
    A dict: twin, fields, forward (tc.reference's tuple per step), X, grad, G, W, kappa, kappa4, kappaV, nlev."""
    key = (meshname, K, mode, partial, nT, nsteps, vert, diff, bih, tuple(srcs), tuple(flags), tuple(wants), fields, fill)
    if key not in _REFS:
        mesh = tc.get_mesh(meshname)
        twin = vmix_twin(meshname, K, mode, partial is True, column_mlt(mesh, K) if partial == "floor" else None)
        nlev = twin.nlev(K)
        dead = np.arange(K)[None, :] >= nlev[:, None]
        q = ts.source_fields(meshname, K, 9)
        twin.source = [q[j] if j in srcs else None for j in range(nT)]
        ssh, u, h, _ = tc.state_of(meshname, K)
        st = TwinState(ssh, u, h)
        f = tc.distinct_fields(mesh, K, 9)[:nT]
        if fields == "unit-first":
            f[0] = np.ones((mesh.nCells, K))
        X = ta.seeds(mesh, K, 9)[:nT]
        if fill is not None:
            f = [np.where(dead, fill, a) for a in f]
            X = [np.where(dead, fill, a) for a in X]
        phis = [[a.copy() for a in f], [a.copy() for a in f]]
        twin.kappa = tc.kappas(meshname, 9)[:nT] if diff else [0.0] * nT
        twin.kappa4 = tb.kappa4s(meshname, 9)[:nT] if bih else [0.0] * nT
        twin.kappaV = kappavs(meshname, K, 9)[:nT] if vert else [0.0] * nT
        fwd = []
        for _ in range(nsteps):
            twin.step_rk4(st, phis, tc.dt_of(meshname))
            fwd.append(([a.copy() for a in phis[0]], [a.copy() for a in phis[1]], st.u[1].copy(), st.h[1].copy(), st.ssh[1].copy()))
        grad = G = W = None                       # a filled case is a forward case
        if fill is None:
            grad, G, W = VmixAdjointTwin(twin).sweep_kgrad(twin.tape, [x.copy() for x in X], dict(flags), tuple(wants))
        _REFS[key] = {"twin": twin, "fields": f, "sources": list(twin.source), "forward": fwd, "X": X, "grad": grad, "G": G, "W": W,
                      "kappa": list(twin.kappa), "kappa4": list(twin.kappa4), "kappaV": list(twin.kappaV), "nlev": nlev, "dead": dead}
    return _REFS[key]


def tile_columns(K, generic=False):
    """csrc/tracer_vmix.hip's vmix_kernel restated from its comment: the columns of a tile of the tile form -- a column takes three sets of
    cs = K | 1 doubles, a tile tc * 4 bytes more; 64 columns while four such tiles fit a CU's 160 KiB, 32 while two do -- or 0: the column
    form (also for K < 2, where nothing is launched, and for kernel variant 3)."""
    cs = K | 1
    if not generic and K >= 2:
        for t, fit in ((64, 4), (32, 2)):
            if (3 * t * cs * 8 + 4 * t) * fit <= 160 * 1024:
                return t
    return 0
