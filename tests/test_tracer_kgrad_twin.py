"""The gradient with respect to kappa_j and kappa4_j: the numpy twin (tests/tracer_kgrad_twin.py) against its long-double restatement
formed directly from the slot sums (so the two identities the device goes through are tested), against central differences of the
twin's forward run, against the plane wave's closed form, and the consequences include/moka_hip.h states.  No GPU needed."""
import inspect
import os
import re

import numpy as np
import pytest

import oracle as orc
import tracer_adjoint_twin as ta
import tracer_biharmonic_twin as tb
import tracer_cases as tc
import tracer_kgrad_twin as tk
import trisk_reference as tr
from del4_twin import TwinState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = tr.LD
NAMES = ("moka_tracer_adjoint_want_diffusivity_gradient", "moka_tracer_adjoint_diffusivity_gradient",
         "moka_tracer_adjoint_diffusivity_density_download")
ALL3 = ((0, 3), (1, 3), (2, 3))
BOTH = ((2, True, True),)


@pytest.fixture(autouse=True, scope="module")
def _the_entry_points_the_twin_specifies():
    """The twin of this file is the specification of the three entry points: without them it specifies nothing."""
    from moka_hip import lib as L
    for name in NAMES:
        assert hasattr(L.lib(), name) and name in L.EXPORTS, name


def _check_against_ld(ref, K, nsteps, label):
    """Every flagged scalar of `ref` against gradients_ld within the counted bound; prints every figure.  Returns the long-double values."""
    twin = ref["twin"]
    adj = tk.KgradAdjointTwin(twin)
    out = {}
    for j, (Wk, Wk4) in ref["W"].items():
        dk, mk, dk4, mk4 = tk.gradients_ld(adj, twin.tape, ref["X"], j)
        for name, W, val, mag, C in (("kappa", Wk, dk, mk, tk.c_k(K, nsteps)), ("kappa4", Wk4, dk4, mk4, tk.c_k4(K, nsteps))):
            if W is None:
                continue
            got = tk.host_sum(W)
            bound = C * tr.U53 * mag
            err = abs(LD(got) - val)
            print(f"{label} tracer {j} d J / d {name}: twin = {got:.15e}, long double = {float(val):.15e}, |difference| = {float(err):.3e}, "
                  f"bound = {C} * 2^-53 * {float(mag):.3e} = {float(bound):.3e}")
            assert err <= bound
            assert bound < 1e-9 * mag                       # the issue's ceiling on the count
            assert abs(val) > 1e3 * bound                   # not vacuous: the bound is far below the gradient itself
            out[(j, name)] = (val, bound)
    return out


# ---- 1, 2: the twin against the long-double restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K,mode,partial", [("planar", 8, "linear", False), ("ico12f", 5, "nonlinear", True),
                                                     ("planar", 33, "del2+del4", True), ("planar", 1, "linear", False)])
def test_twin_against_the_slot_sums_in_long_double(meshname, K, mode, partial):
    """sum tau_s D_s and - sum tau_s B_s from the edge fluxes in long double against the twin's route through D = ph L and the
    self-adjointness of Lap, two recorded steps: within C_K = 20 + depth(K) + 8 + 5 and C_K4 = C_K + 14 roundings of the magnitude sum
    (tracer_kgrad_twin.py counts the chain).  Tracer 1 has kappa == 0 and tracer 2 kappa4 == 0: derivatives at zero beside the others."""
    ref = tk.reference(meshname, K, mode, partial, 3, BOTH, ALL3)
    assert ref["kappa"][0][1] == 0.0 and ref["kappa4"][0][2] == 0.0 and ref["kappa4"][0][0] != 0.0
    assert tk.c_k(K, 2) == 33 + tk.depth(K) and tk.c_k4(K, 2) == 47 + tk.depth(K)
    assert len(_check_against_ld(ref, K, 2, f"{meshname} K = {K} {mode}")) == 6


def test_gradients_on_a_state_that_never_set_a_diffusivity():
    """Every recorded kappa and kappa4 zero (the sweep runs its diffusion-free instances): both derivatives at zero match the long-double
    values, M computed for them alone."""
    ref = tk.reference("planar", 6, "linear", False, 3, ((2, False, False),), ALL3)
    assert not any(ref["kappa"][0]) and not any(ref["kappa4"][0])
    assert len(_check_against_ld(ref, 6, 2, "no diffusivity")) == 6


def test_colsum_is_the_documented_order():
    """colsum against the order written out lane by lane for K = 1, 8, 33 and 70 (the strided loop), and against the plain sum within
    depth(K) roundings."""
    rng = np.random.default_rng(3)
    for K in (1, 8, 33, 70):
        d = rng.uniform(-1, 1, (5, K))
        Ln = tk.lanes(K)
        exp = np.empty(5)
        for c in range(5):
            part = [0.0] * Ln
            for k in range(K):                       # ascending k reaches lane k % LPC in the lane's own ascending order
                part[k % Ln] = part[k % Ln] + d[c, k]
            o = Ln // 2
            while o >= 1:
                part = [part[l] + part[l ^ o] for l in range(Ln)]
                o //= 2
            exp[c] = part[0]
        got = tk.colsum(d)
        assert np.array_equal(got, exp)
        assert np.all(np.abs(got.astype(LD) - d.astype(LD).sum(axis=1)) <= tk.depth(K) * tr.U53 * np.abs(d).astype(LD).sum(axis=1))


# ---- 3: central differences ---------------------------------------------------------------------------------------------------------
def _J(twin, j, phi, X, dkap=0.0, dkap4=0.0):
    for rec in twin.tape:
        phi = twin.replay(rec, j, phi, rec["kappa"][j] + dkap, rec["kappa4"][j] + dkap4)[1]
    return ta.dot_ld(X, phi)


@pytest.mark.parametrize("meshname,K,mode,partial", [("planar", 3, "linear", False), ("ico12f", 5, "nonlinear", True)])
def test_central_differences_decay_as_delta_squared(meshname, K, mode, partial):
    """J_j = <X_j, phi_N,j> from the twin's forward run over the recorded flow, with the coefficient of EVERY recorded step moved by
    +-delta.  J is a polynomial of degree 4 per step in it, so the central difference is off the derivative by delta^2 J''' / 6 + ...:
    halving delta must cut the discrepancy by between 3 and 5, three sizes, unless the smaller discrepancy is already at the floor
    (the long-double bound of the gradient plus the forward round-off 2 eps_J / delta, eps_J = steps * C_STEP_B * 2^-53 * sum |X| W).
    delta starts at the coefficient's own scale (0.02 dc^2 / dt and 0.002 dc^4 / dt)."""
    nsteps = 2
    ref = tk.reference(meshname, K, mode, partial, 3, BOTH, ALL3)
    twin, mesh = ref["twin"], tc.get_mesh(meshname)
    ld = _check_against_ld(ref, K, nsteps, "fd")
    d0 = {"kappa": tc.kappas(meshname, 9)[0], "kappa4": tb.kappa4s(meshname, 9)[0]}
    for j in range(3):
        W = np.abs(ref["fields"][j]).astype(LD)
        for rec in twin.tape:
            W = tb.forward_magnitude(mesh, twin.mlt, rec, W, rec["kappa"][j] + d0["kappa"], rec["kappa4"][j] + d0["kappa4"])
        epsJ = nsteps * tb.C_STEP_B * tr.U53 * (np.abs(ref["X"][j]).astype(LD) * W).sum()
        for name, b in (("kappa", 0), ("kappa4", 1)):
            grad = LD(tk.host_sum(ref["W"][j][b]))
            disc = []
            for i in range(3):
                d = d0[name] / 2 ** i
                kw = {"dkap": d} if b == 0 else {"dkap4": d}
                fd = (_J(twin, j, ref["fields"][j], ref["X"][j], **kw) - _J(twin, j, ref["fields"][j], ref["X"][j], **{k: -v for k, v in kw.items()})) / (2 * LD(d))
                disc.append((abs(fd - grad), ld[(j, name)][1] + 2 * epsJ / LD(d)))
            ratios = [float(disc[i][0] / disc[i + 1][0]) for i in range(2)]
            print(f"{meshname} tracer {j} d J / d {name} = {float(grad):.6e}: discrepancies {[f'{float(x[0]):.3e}' for x in disc]}, ratios "
                  f"{[f'{r:.3f}' for r in ratios]}, floors {[f'{float(x[1]):.3e}' for x in disc]}")
            for i in range(2):
                assert 3.0 <= ratios[i] <= 5.0 or disc[i + 1][0] <= disc[i + 1][1]
            assert 3.0 <= ratios[0] <= 5.0                      # the decay is seen at least once: the floor is not what passes the test
            assert disc[0][0] < 0.5 * abs(grad) or disc[2][0] < 0.05 * abs(grad)


# ---- 4: the plane wave --------------------------------------------------------------------------------------------------------------
def test_plane_wave_gradients():
    """tracer_cases.eigenmode_state(2), kappa = EIG_KAPPA, kappa4 = EIG_KAPPA4, ten recorded steps, J = <phi0, phi_10>:
    d phi^_N / d kappa = N R(z)^(N-1) R'(z) lam dt phi^_0 and the same with -lam^2 for kappa4, to 5e-14 of the magnitude sum."""
    K = 2
    mesh, (ssh, u, h, rest), phi0 = tc.eigenmode_state(K)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=K)
    twin = tk.KgradTwin(om, om, [tc.EIG_KAPPA], kappa4=[tb.EIG_KAPPA4])
    st = TwinState(ssh, u, h)
    phis = [[phi0.copy()], [phi0.copy()]]
    for _ in range(tc.EIG_STEPS):
        twin.step_rk4(st, phis, tc.EIG_DT)
    _, _, W = tk.KgradAdjointTwin(twin).sweep_kgrad(twin.tape, [phi0.copy()], {0: 3})
    tk.plane_wave_gradient_check(tk.host_sum(W[0][0]), tk.host_sum(W[0][1]), mesh, K, tc.EIG_KAPPA, tb.EIG_KAPPA4, phi0, "KgradAdjointTwin")


# ---- 5: consequences ----------------------------------------------------------------------------------------------------------------
def test_a_constant_tracer_has_both_gradients_exactly_zero():
    """The tracer that is 1 everywhere stays exactly 1.0 through every stage (include/moka_hip.h), so L == 0 exactly in all of them and
    both densities are +0.0 in every cell, whatever the seed."""
    ref = tk.reference("planar", 6, "nonlinear", True, 2, BOTH, ((0, 3), (1, 3)), fields="unit-first")
    assert np.all(ref["fields"][0] == 1.0) and all(np.all(p == 1.0) for p in ref["twin"].tape[-1]["pphi"][0])
    for W in ref["W"][0]:
        assert not W.any() and not np.signbit(W).any() and tk.host_sum(W) == 0.0
    assert all(W.any() for W in ref["W"][1])


def test_a_zero_seed_gives_exactly_zero_densities_and_two_seeds_add():
    ref = tk.reference("planar", 6, "linear", False, 3, BOTH, ALL3)
    twin = ref["twin"]
    adj = tk.KgradAdjointTwin(twin)
    X = ref["X"]
    zero = [np.zeros_like(x) for x in X]
    for Ws in adj.sweep_kgrad(twin.tape, zero, dict(ALL3))[2].values():
        for W in Ws:
            assert not W.any()
    other = [x[::-1].copy() for x in X]
    Wa, Wb = ref["W"], adj.sweep_kgrad(twin.tape, other, dict(ALL3))[2]
    Ws = adj.sweep_kgrad(twin.tape, [a + b for a, b in zip(X, other)], dict(ALL3))[2]
    ld = _check_against_ld(ref, 6, 2, "sum")
    for j in range(3):
        for b, name in ((0, "kappa"), (1, "kappa4")):
            lhs, rhs = LD(tk.host_sum(Ws[j][b])), LD(tk.host_sum(Wa[j][b])) + LD(tk.host_sum(Wb[j][b]))
            # three gradients, each within its bound of a linear functional of its seed; the seeds' magnitudes at most add, and
            # forming X + other rounds once per element: 4 bounds of the pair's magnitude is generous and far below the values
            bound = 8 * ld[(j, name)][1]
            print(f"tracer {j} {name}: |g(a + b) - g(a) - g(b)| = {float(abs(lhs - rhs)):.3e}, bound = {float(bound):.3e}")
            assert abs(lhs - rhs) <= bound


def test_flagging_changes_no_bit_of_X_or_G():
    """sweep_kgrad returns the parent's X and G (asserted record by record inside it) whatever is flagged."""
    a = tk.reference("planar", 6, "linear", False, 3, BOTH, ALL3, (0, 2))
    b = tk.reference("planar", 6, "linear", False, 3, BOTH, (), (0, 2))
    c = tb.reference("planar", 6, "linear", False, 3, BOTH, (), (0, 2))
    assert not b["W"] and len(a["W"]) == 3
    for j in range(3):
        assert np.array_equal(a["grad"][j], b["grad"][j]) and np.array_equal(a["grad"][j], c["grad"][j])
        assert np.array_equal(a["forward"][-1][1][j], c["forward"][-1][1][j])
    for j in (0, 2):
        assert np.array_equal(a["G"][j], b["G"][j]) and np.array_equal(a["G"][j], c["G"][j])


# ---- the entry points ---------------------------------------------------------------------------------------------------------------
def test_entry_points_exist():
    import moka_hip as mk
    from moka_hip import lib as L
    hdr = open(os.path.join(ROOT, "include", "moka_hip.h")).read()
    assert re.search(r"int\s+moka_tracer_adjoint_want_diffusivity_gradient\(moka_tracer_tape \*t, int32_t j, int what, int on\);", hdr)
    assert re.search(r"int\s+moka_tracer_adjoint_diffusivity_gradient\(moka_tracer_tape \*t, int32_t j, int what, double \*out\);", hdr)
    assert re.search(r"int\s+moka_tracer_adjoint_diffusivity_density_download\(moka_tracer_tape \*t, int32_t j, int what, double \*host\);", hdr)
    assert "MOKA_TRACER_GRAD_KAPPA = 1, MOKA_TRACER_GRAD_KAPPA4 = 2" in hdr and (L.TRACER_GRAD_KAPPA, L.TRACER_GRAD_KAPPA4) == (1, 2)
    assert "Wk_j[c]  = Wk_j[c]  + areaCell[c] * colsum(dk)[c]" in hdr and "Wk4_j[c] = Wk4_j[c] - areaCell[c] * colsum(dk4)[c]" in hdr
    assert "partial[l] + partial[l xor o]" in hdr
    jl = open(os.path.join(ROOT, "mpas-ocean.jl_amd", "julia", "MokaHIP.jl")).read()
    for name in NAMES:
        assert f"ccall((:{name}, lib)" in jl, name
    for m in ("want_diffusivity_gradient", "diffusivity_gradient", "biharmonic_gradient", "diffusivity_density"):
        assert hasattr(mk.TracerAdjointTape, m), m
    sig = inspect.signature(mk.TracerAdjointTape.want_diffusivity_gradient).parameters
    assert list(sig) == ["self", "j", "kappa", "biharmonic"] and sig["kappa"].default is True and sig["biharmonic"].default is False
    assert "diffusivity" in inspect.signature(mk.TracerAdjointTape.gradient).parameters
    for doc in ("README.md", "DESIGN.md", os.path.join("include", "moka_hip.h")):
        text = open(os.path.join(ROOT, doc)).read()
        assert "moka_tracer_adjoint_want_diffusivity_gradient" in text, doc
        for line in text.split("\n"):
            if re.search(r"out of scope", line, re.I) and re.search(r"sensitivit|reverse mode", line, re.I):
                assert "the flow" in line or "(u, h)" in line, (doc, line)
                assert not re.search(r"to (κ|kappa)\b|, (κ|kappa)4? or|to (κ|kappa)4", line), (doc, line)
