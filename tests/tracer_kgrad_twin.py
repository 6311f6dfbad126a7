"""Numpy twin of the gradient of a tracer objective with respect to the mixing coefficients kappa_j and kappa4_j
(moka_tracer_adjoint_want_diffusivity_gradient), and a long-double restatement that shares no code with it.  Extends
tests/tracer_biharmonic_twin.py (the recording / source / biharmonic twin chain), whose docstrings state the schemes.

Algebra (include/moka_hip.h).  Stage s of tracer j forms T = A(P_s) pphi_s + kappa_j D_s - kappa4_j B_s (+ q) with
    D_s[k,c] = sum over the slots of ((hE * (pphi_s[k,c'] - pphi_s[k,c])) * dvdc[c,i]) * invArea[c]
and B_s the same sum over L_s = Lap(ph_s, pphi_s).  With tau_s the adjoint of T (tracer_source_twin.py names it),
    d J / d kappa_j = sum_steps sum_s sum_{k,c} tau_s D_s,        d J / d kappa4_j = - sum_steps sum_s sum_{k,c} tau_s B_s.
The device (and `KgradAdjointTwin`) goes through two identities: D_s = ph_s L_s, and Lap self-adjoint under areaCell * ph_s, so that
sum tau_s B_s = sum_c areaCell sum_k ph_s L_s M with M = Lap(ph_s, y), y = tau_s * invA.  Per reverse stage rs = 3, 2, 1, 0 and element
    p = ph[k,c] * L[k,c];     dk = p * y[k,c];     dk4 = p * M[k,c]
    Wk[c] = Wk[c] + areaCell[c] * colsum(dk)[c];      Wk4[c] = Wk4[c] - areaCell[c] * colsum(dk4)[c]
colsum (`colsum`): LPC = the smallest power of two >= K, at most 64; partial l starts at 0.0 and adds the levels k = l, l + LPC, ...
in ascending order; then for o = LPC/2, ..., 1 every partial l becomes partial[l] + partial[l xor o]; colsum = partial[0].
The scalars are the sums of the densities over the cells in ascending order in long double, rounded once (`host_sum`).

`KgradTwin` is TracerBiharmonicTwin whose records gain "pphi": per tracer the four provisional fields pphi_0..pphi_3, replayed over the
record with the twin's own tendency (the replay's new tracers are asserted to be the step's, bit for bit).

Long double.  `gradients_ld` forms sum tau_s D_s and - sum tau_s B_s DIRECTLY from the edge-flux slot sums D_s = div(hE grad pphi_s),
B_s = div(hE grad L_s) (trisk_reference's geometry, active and divergence; L_s in long double) and the twin's tau_s -- not through the
two identities, which the comparison therefore tests.  Magnitudes: every leaf replaced by its absolute value, a difference by the sum.

Round-off counts (one rounding per +, -, *, /, including forming 1/areaCell and dvdc; the house slack of C_H - 11 = 5 on top).  Both
routes share the doubles tau_s and pphi_s, so only the twin's chain from them counts.  depth(K) = ceil(K / LPC) - 1 + log2(LPC) is
the number of additions an element passes in colsum (the first onto 0.0 is exact).
  C_K(K, n)   one term of sum_c Wk: L 14 (tracer_biharmonic_twin.py's C_LAP without slack); p 1; y = tau * invA 2 (forming invA,
              the product); dk 1; depth(K); areaCell * colsum 1; the 4 n additions onto Wk over n recorded steps; the final rounding
              of the host sum 1 (its additions are long double).  20 + depth(K) + 4 n, + 5.
  C_K4(K, n)  the same with M = Lap(ph, y) behind y: 14 more.  34 + depth(K) + 4 n, + 5.
The magnitude sums are sum |tau_s| mD_s and sum |tau_s| mB_s of the direct route; by the symmetry of the stencil (both are
sum over edges of hE dv/dc (a_c + a_c') (b_c + b_c')) they are also the magnitude sums of the twin's route."""
import numpy as np

import tracer_adjoint_twin as ta
import tracer_biharmonic_twin as tb
import tracer_cases as tc
import trisk_reference as tr
from del4_twin import TwinState

LD = tr.LD
SLACK = tr.C_H - 11
KAPPA, KAPPA4 = 1, 2              # MOKA_TRACER_GRAD_KAPPA, MOKA_TRACER_GRAD_KAPPA4


def lanes(K):
    l = 1
    while l < K and l < 64:
        l <<= 1
    return l


def depth(K):
    L = lanes(K)
    return -(-K // L) - 1 + int(np.log2(L))


def c_k(K, nsteps):
    return 20 + depth(K) + 4 * nsteps + SLACK


def c_k4(K, nsteps):
    return 34 + depth(K) + 4 * nsteps + SLACK


assert (lanes(1), lanes(8), lanes(33), lanes(60), lanes(70)) == (1, 8, 64, 64, 64)
assert (depth(1), depth(8), depth(33), depth(70)) == (0, 3, 6, 7) and (c_k(60, 2), c_k4(60, 2)) == (39, 53)


def colsum(d):
    """The column sum of a (nCells, K) field in the device's order (the module docstring)."""
    nC, K = d.shape
    L = lanes(K)
    part = np.zeros((nC, L))
    for k0 in range(0, K, L):
        blk = d[:, k0:k0 + L]
        part[:, :blk.shape[1]] = part[:, :blk.shape[1]] + blk
    idx = np.arange(L)
    o = L // 2
    while o >= 1:
        part = part + part[:, idx ^ o]
        o //= 2
    return part[:, 0].copy()


def host_sum(w):
    """The scalar of a density: ascending over the cells in long double, rounded once."""
    s = LD(0)
    for v in np.asarray(w, dtype=np.float64):
        s += LD(v)
    return float(s)


class KgradTwin(tb.TracerBiharmonicTwin):
    """TracerBiharmonicTwin whose records gain "pphi" = [tracer][stage] -> (nCells, K)."""

    def replay(self, rec, j, phi, kappa=None, kappa4=None):
        """([pphi_0..pphi_3], phi_new) of tracer j over the recorded flow `rec` from phi, with the record's coefficients unless given."""
        dt = rec["dt"]
        a = (dt / 2., dt / 2., dt)
        b = (dt / 6., dt / 3., dt / 3., dt / 6.)
        kap = rec["kappa"][j] if kappa is None else kappa
        kap4 = rec["kappa4"][j] if kappa4 is None else kappa4
        q = self.source_of(j)
        Qc = phi * rec["P"][0][1]
        Qn = Qc.copy()
        p, stages = phi, []
        for s in range(4):
            pu, ph = rec["P"][s]
            stages.append(p)
            T = self.tendency_bih(pu, ph, p, kap, kap4, self.lap(ph, p))
            if q is not None:
                T = T + q
            if s < 3:
                p = (Qc + a[s] * T) / rec["P"][s + 1][1]
            Qn = Qn + b[s] * T
        return stages, Qn / rec["hn"]

    def step_rk4(self, st, phis, dt, magnitudes=False):
        phi0 = [p.copy() for p in phis[1]]
        super().step_rk4(st, phis, dt, magnitudes)
        rec = self.tape[-1]
        rec["pphi"] = []
        for j, p0 in enumerate(phi0):
            stages, new = self.replay(rec, j, p0)
            assert np.array_equal(new, phis[1][j]), ("the replay over the record is not the step", j)
            rec["pphi"].append(stages)


class KgradAdjointTwin(tb.BiharmonicAdjointTwin):
    """BiharmonicAdjointTwin that also accumulates the two sensitivity densities of the flagged tracers."""

    def stage_fields(self, rec, x, j, diff, bih):
        """[(rs, tau_rs, y_rs)] for rs = 3, 2, 1, 0 of tracer j: the sweep's recipe (the instances `diff` / `bih` select), y = tau * invA."""
        dt = rec["dt"]
        a = (dt / 2., dt / 2., dt)
        b = (dt / 6., dt / 3., dt / 3., dt / 6.)
        invA = self.tw.invArea[:, None]
        kap, kap4 = rec["kappa"][j], rec.get("kappa4", [0.0] * (j + 1))[j]
        g = x / rec["hn"]
        tau = b[3] * g
        y = tau * invA
        out = [(3, tau, y)]
        for s in (3, 2, 1):
            pu, ph = rec["P"][s]
            r = self.R_bih(pu, ph, y, kap, kap4) if bih else self.R(pu, ph, y, kap, diff)
            v = r / ph
            tau = b[s - 1] * g + a[s - 1] * v
            y = tau * invA
            out.append((s - 1, tau, y))
        return out

    def sweep_tail(self, tape, n, X):
        """Record n backwards with the instances the whole tape selects (what the parent's sweep does with it)."""
        if any(k != 0.0 for rec in tape for k in rec.get("kappa4", ())):
            return self.reverse_step_bih(tape[n], X, None)
        return self.reverse_step(tape[n], X, any(k != 0.0 for rec in tape for k in rec["kappa"]), None)

    def sweep_kgrad(self, tape, X, flags, want=()):
        """(X, G, W): the parent's sweep, untouched, and W[j] = [Wk or None, Wk4 or None] (each (nCells,)) for the tracers of
        flags = {j: bits}."""
        tw = self.tw
        area = np.asarray(tw.om.mesh.areaCell, dtype=np.float64)
        bih = any(k != 0.0 for rec in tape for k in rec.get("kappa4", ()))
        diff = any(k != 0.0 for rec in tape for k in rec["kappa"])
        W = {j: [np.zeros(area.shape) if w & KAPPA else None, np.zeros(area.shape) if w & KAPPA4 else None] for j, w in flags.items() if w}
        Xs = [x.copy() for x in X]
        for n in range(len(tape) - 1, -1, -1):
            rec = tape[n]
            for j, (Wk, Wk4) in W.items():
                for rs, _, y in self.stage_fields(rec, Xs[j], j, diff, bih):
                    ph = rec["P"][rs][1]
                    p = ph * tw.lap(ph, rec["pphi"][j][rs])
                    if Wk is not None:
                        Wk[:] = Wk + area * colsum(p * y)
                    if Wk4 is not None:
                        Wk4[:] = Wk4 - area * colsum(p * tw.lap(ph, y))
            Xs = self.sweep_tail(tape, n, Xs)
        Xf, G = self.sweep(tape, [x.copy() for x in X], want)
        for xa, xb in zip(Xs, Xf):
            assert np.array_equal(xa, xb)            # record by record is the parent's sweep
        return Xf, G, W


# ---- long double ------------------------------------------------------------------------------------------------------------------
def slot_sums_ld(mesh, ph, pphi, mlt):
    """(D, mD, B, mB) in long double from the edge fluxes: D = div(hE (p[c2] - p[c1]) / dc), B the same over L = D / h."""
    g = tr.geometry(mesh)
    K = np.asarray(ph).shape[1]
    h, p = tr._ld(ph, (g.nC, K)), tr._ld(pphi, (g.nC, K))
    act = tr.active(g, mlt, K)
    hE = (h[g.c1] + h[g.c2]) / 2
    mhE = (np.abs(h[g.c1]) + np.abs(h[g.c2])) / 2
    dc = g.dc[:, None]
    D, mD = tr.divergence(g, np.where(act, hE * (p[g.c2] - p[g.c1]) / dc, 0), np.where(act, mhE * (np.abs(p[g.c2]) + np.abs(p[g.c1])) / dc, 0))
    L, mL = D / h, mD / np.abs(h)
    B, mB = tr.divergence(g, np.where(act, hE * (L[g.c2] - L[g.c1]) / dc, 0), np.where(act, mhE * (mL[g.c2] + mL[g.c1]) / dc, 0))
    return D, mD, B, mB


def gradients_ld(adj, tape, X, j):
    """(dk, mk, dk4, mk4): sum tau_s D_s and - sum tau_s B_s of tracer j over the records, and their magnitude sums, in long double from
    the twin's tau_s (doubles) and the records' pphi_s."""
    tw = adj.tw
    mesh = tw.om.mesh
    bih = any(k != 0.0 for rec in tape for k in rec.get("kappa4", ()))
    diff = any(k != 0.0 for rec in tape for k in rec["kappa"])
    dk = mk = dk4 = mk4 = LD(0)
    Xs = [x.copy() for x in X]
    for n in range(len(tape) - 1, -1, -1):
        rec = tape[n]
        for rs, tau, _ in adj.stage_fields(rec, Xs[j], j, diff, bih):
            D, mD, B, mB = slot_sums_ld(mesh, rec["P"][rs][1], rec["pphi"][j][rs], tw.mlt)
            t = tau.astype(LD)
            dk, mk = dk + (t * D).sum(), mk + (np.abs(t) * mD).sum()
            dk4, mk4 = dk4 - (t * B).sum(), mk4 + (np.abs(t) * mB).sum()
        # the adjoints at the start of this record, by the sweep that would have run over the whole tape (its instances)
        Xs = adj.sweep_tail(tape, n, Xs)
    return dk, mk, dk4, mk4


# ---- shared cases -----------------------------------------------------------------------------------------------------------------
_REFS = {}


def kgrad_twin(meshname, K, mode="linear", partial=False):
    t = tc.twin_of(meshname, K, mode, partial)
    return KgradTwin(t.om, t.base, [])


def reference(meshname, K, mode, partial, nT, segments, flags, wants=(), fields=None):
    """tracer_biharmonic_twin.reference with the densities: computed once per case and shared (never modified by a test).  flags =
    ((j, bits), ...).  fields: None = the first nT of tc.distinct_fields(mesh, K, 9); "unit-first": the first is 1 everywhere.  A dict: twin, fields, forward,
    X, grad, G, W = {j: [Wk or None, Wk4 or None]}, kappa / kappa4 = the values of each segment."""
    key = (meshname, K, mode, partial, nT, tuple(segments), tuple(flags), tuple(wants), fields)
    if key not in _REFS:
        mesh = tc.get_mesh(meshname)
        twin = kgrad_twin(meshname, K, mode, partial)
        ssh, u, h, _ = tc.state_of(meshname, K)
        st = TwinState(ssh, u, h)
        f = tc.distinct_fields(mesh, K, 9)[:nT]
        if fields == "unit-first":
            f[0] = np.ones((mesh.nCells, K))
        phis = [[a.copy() for a in f], [a.copy() for a in f]]
        fwd, kaps, kap4s = [], [], []
        for nsteps, diff, bih in segments:
            twin.kappa = tc.kappas(meshname, 9)[:nT] if diff else [0.0] * nT
            k4 = tb.kappa4s(meshname, 9)[:nT]
            twin.kappa4 = ([c * k for c, k in zip(bih, k4)] if isinstance(bih, tuple) else k4) if bih else [0.0] * nT
            kaps.append(list(twin.kappa))
            kap4s.append(list(twin.kappa4))
            for _ in range(nsteps):
                twin.step_rk4(st, phis, tc.dt_of(meshname))
                fwd.append(([a.copy() for a in phis[0]], [a.copy() for a in phis[1]], st.u[1].copy(), st.h[1].copy(), st.ssh[1].copy()))
        X = ta.seeds(mesh, K, 9)[:nT]
        grad, G, W = KgradAdjointTwin(twin).sweep_kgrad(twin.tape, [x.copy() for x in X], dict(flags), tuple(wants))
        _REFS[key] = {"twin": twin, "fields": f, "sources": [None] * nT, "forward": fwd, "X": X, "grad": grad, "G": G, "W": W,
                      "kappa": kaps, "kappa4": kap4s}
    return _REFS[key]


# ---- the plane wave ---------------------------------------------------------------------------------------------------------------
def eigen_lambda():
    kx, ky = tc.EIG_K
    return sum((2 / (3 * tc.EIG_DC ** 2)) * (np.cos((kx * np.cos(m * np.pi / 3) + ky * np.sin(m * np.pi / 3)) * tc.EIG_DC) - 1) for m in range(6))


def plane_wave_gradients(mesh, K, kappa, kappa4, X, exact_exponential=False):
    """(dk, dk4, base): with z = (mu + kappa lam - kappa4 lam^2) dt and R the RK4 polynomial the mode amplitude after N steps is
    R(z)^N, so d phi_N / d kappa = 0.5 Re(N R^(N-1) R'(z) lam dt e^{ikx}) and the same with -lam^2 for kappa4; J = <X, phi_N>.
    base = sum |X| 0.5 |N R^(N-1) R' dt|: times |lam| (lam^2) the magnitude sum of dk (dk4).  exact_exponential: R' = R, the derivative
    a scheme that integrated the mode exactly would have.  Nothing here shares code with the twins."""
    N = tc.EIG_STEPS
    z = tb.eigenmode_z(kappa, kappa4)
    R = 1 + z + z ** 2 / 2 + z ** 3 / 6 + z ** 4 / 24
    dR = R if exact_exponential else 1 + z + z ** 2 / 2 + z ** 3 / 6
    lam = eigen_lambda()
    wave = np.exp(1j * (tc.EIG_K[0] * np.asarray(mesh.xCell) + tc.EIG_K[1] * np.asarray(mesh.yCell)))
    amp = N * R ** (N - 1) * dR * tc.EIG_DT
    Xl = np.asarray(X).astype(LD)
    ek = np.repeat((0.5 * (amp * lam * wave).real)[:, None], K, axis=1).astype(LD)
    ek4 = np.repeat((0.5 * (amp * (-lam * lam) * wave).real)[:, None], K, axis=1).astype(LD)
    return (Xl * ek).sum(), (Xl * ek4).sum(), np.abs(Xl).sum() * LD(0.5 * abs(amp))


def plane_wave_gradient_check(dk, dk4, mesh, K, kappa, kappa4, X, label):
    """|gradient - expectation| <= 5e-14 * magnitude sum for both coefficients; the same tolerance refuses R' = R and a gradient of
    zero.  Prints every figure."""
    ek, ek4, base = plane_wave_gradients(mesh, K, kappa, kappa4, X)
    xk, xk4, _ = plane_wave_gradients(mesh, K, kappa, kappa4, X, exact_exponential=True)
    lam = eigen_lambda()
    for name, got, exp, wrong, scale in (("kappa", dk, ek, xk, base * abs(lam)), ("kappa4", dk4, ek4, xk4, base * lam * lam)):
        tol = LD(5e-14) * scale
        dev, gap = abs(LD(got) - exp), abs(exp - wrong)
        print(f"{label}: d J / d {name} = {float(got):.15e}, expected {float(exp):.15e}, deviation = {float(dev):.3e}, tolerance = "
              f"{float(tol):.3e}, gap to R' = R: {float(gap):.3e}")
        assert dev <= tol
        assert gap > 1e3 * tol and abs(exp) > 1e3 * tol
