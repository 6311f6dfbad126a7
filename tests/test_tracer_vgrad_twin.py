"""The gradient with respect to the vertical diffusivity: the numpy twin (tests/tracer_vgrad_twin.py) against its long-double restatement
within the counted bound, against central differences of a long-double forward (uniform kappaV, and a diffusivity per interface and
cell), against a one-sided difference at kappaV == 0, against the vertical cosine mode's closed form, and the consequences
include/moka_hip.h states.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import oracle as orc
import tracer_adjoint_twin as ta
import tracer_biharmonic_twin as tb
import tracer_cases as tc
import tracer_kgrad_twin as tk
import tracer_vgrad_twin as tg
import tracer_vmix_twin as tv
from del4_twin import TwinState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = tv.LD
U = tv.U53
NAMES = ("moka_tracer_adjoint_want_vertical_gradient", "moka_tracer_adjoint_vertical_gradient",
         "moka_tracer_adjoint_vertical_density_download")
NSTEPS = 3
ALL3 = (0, 1, 2)


# ---- the entry points ---------------------------------------------------------------------------------------------------------------
def test_entry_points_exist():
    from moka_hip import lib as L
    for name in NAMES:
        assert hasattr(L.lib(), name) and name in L.EXPORTS, name
    hdr = open(os.path.join(ROOT, "include", "moka_hip.h")).read()
    assert re.search(r"int\s+moka_tracer_adjoint_want_vertical_gradient\(moka_tracer_tape \*t, int32_t j, int on\);", hdr)
    assert re.search(r"int\s+moka_tracer_adjoint_vertical_gradient\(moka_tracer_tape \*t, int32_t j, double \*out\);", hdr)
    assert re.search(r"int\s+moka_tracer_adjoint_vertical_density_download\(moka_tracer_tape \*t, int32_t j, int view, double \*host\);", hdr)
    assert "MOKA_VGRAD_INTERFACE = 0, MOKA_VGRAD_CELL = 1, MOKA_VGRAD_PROFILE = 2" in hdr
    assert (L.VGRAD_INTERFACE, L.VGRAD_CELL, L.VGRAD_PROFILE) == (0, 1, 2)
    assert "Not built yet" not in hdr and "c = (p[k] - p[k+1]) * q;   e = (z[k] - z[k+1]) * c;   D_j[k,c] = D_j[k,c] - e" in hdr
    jl = open(os.path.join(ROOT, "mpas-ocean.jl_amd", "julia", "MokaHIP.jl")).read()
    for name in NAMES:
        assert f"(:{name}, lib)" in jl, name


def test_rule_of_the_gradient_instances():
    """Four sets: 64 columns while 4 (2048 cs + 256) <= 163840, cs <= 19; 32 while 2 (1024 cs + 128) <= 163840, cs <= 79."""
    got = {K: tg.tile_columns_grad(K) for K in range(0, 130)}
    assert all(got[K] == (0 if K < 2 else 64 if (K | 1) <= 19 else 32 if (K | 1) <= 79 else 0) for K in got)
    assert (got[19], got[20], got[79], got[80]) == (64, 32, 32, 0) and not any(tg.tile_columns_grad(K, True) for K in got)
    assert 4 * 32 * 79 * 8 + 128 == 81024 <= 80 * 1024                              # the largest tile, inside the raised dynamic limit
    assert [tv.tile_columns(K) for K in (25, 26, 105, 106)] == [64, 32, 32, 0]      # the plain instances keep their rule
    src = open(os.path.join(ROOT, "mpas-ocean.jl_amd", "csrc", "tracer_vmix.hip")).read()
    assert "(size_t)sets * tc * cs * 8 + (size_t)tc * 4" in src and "vmix_kernel(a.K, generic, 4)" in src


# ---- the twin against long double ---------------------------------------------------------------------------------------------------
def check_against_ld(ref, label, vacuous_ok=()):
    """Every flagged density of `ref` against density_ld, element by element, and the scalar; prints the figures.  Returns
    {j: (D_ld, bound per element, scalar_ld, scalar bound)}."""
    twin = ref["twin"]
    adj = tg.VgradAdjointTwin(twin)
    out = {}
    for j, D in ref["D"].items():
        Dl, B = tg.density_ld(adj, twin.tape, ref["X"], j)
        err = np.abs(D.astype(LD) - Dl)
        assert np.all(err <= B), (label, j, float((err - B).max()))
        s, sl = tk.host_sum(D.ravel()), Dl.sum()
        sb = B.sum() + U * abs(sl)
        worst = float((err / np.where(B > 0, B, 1)).max())
        print(f"{label} tracer {j}: max |D - D_ld| = {float(err.max()):.3e} (worst element at {worst:.3f} of its bound), scalar twin = {s:.15e}, "
              f"long double = {float(sl):.15e}, |difference| = {float(abs(LD(s) - sl)):.3e}, bound = {float(sb):.3e}")
        assert abs(LD(s) - sl) <= sb
        if j not in vacuous_ok and D.shape[1] >= 2:
            assert np.abs(Dl).sum() > 1e3 * B.sum()                      # not vacuous: the bound is far below the density itself
        out[j] = (Dl, B, sl, sb)
    return out


@pytest.mark.parametrize("partial", [False, True, "floor"], ids=["full", "partial_mlt", "sea-floor"])
@pytest.mark.parametrize("K", [2, 3, 6, 34])
@pytest.mark.parametrize("meshname,mode", [("planar", "linear"), ("ico12f", "linear"), ("planar", "nonlinear")])
def test_twin_against_long_double(meshname, mode, K, partial):
    """Three recorded steps, three tracers with tv.kappavs (the second an exact zero: z = X / h), all flagged."""
    ref = tg.reference(meshname, K, mode, partial, 3, NSTEPS, ALL3)
    assert ref["steps"][0][0][1] == 0.0 and all(k != 0.0 for k in (ref["steps"][0][0][0], ref["steps"][0][0][2]))
    assert len(check_against_ld(ref, f"{meshname} K = {K} {mode} {partial}")) == 3


# ---- differences of a long-double forward -------------------------------------------------------------------------------------------
def J_of(ref, j, kvf_of):
    """J = <X_j, phi_N,j> with the vertical pass of record n solved in long double for the diffusivity field kvf_of(n), (nCells, K) per
    interface and cell.  The RK4 part of a step is the twin's replay in doubles from the rounded phi, so J carries the forward
    round-off eps_J that `eps_J` counts."""
    twin = ref["twin"]
    K = ref["X"][j].shape[1]
    nlev = twin.nlev(K)
    phi = ref["fields"][j]
    new = None
    for n, rec in enumerate(twin.tape):
        star = twin.replay(rec, j, np.asarray(phi, dtype=np.float64))[1]
        new = tg.forward_ld_kfield(rec["hn"], star, nlev, rec["dt"], kvf_of(n))
        phi = new
    return (ref["X"][j].astype(LD) * new).sum()


def eps_J(ref, meshname, j):
    """nsteps * (C_STEP_B + 1) * 2^-53 * sum |X| W: tracer_biharmonic_twin's count of the RK4 step in doubles on its magnitude W and one
    rounding of phi_new to a double between the steps; W is carried through the vertical pass by its column maximum (A^-1 diag(h) is
    row-stochastic for every kappaV >= 0)."""
    twin, mesh = ref["twin"], tc.get_mesh(meshname)
    W = np.abs(ref["fields"][j]).astype(LD)
    for rec in twin.tape:
        W = tb.forward_magnitude(mesh, twin.mlt, rec, W, rec["kappa"][j], rec["kappa4"][j])
        W = np.repeat(W.max(axis=1)[:, None], W.shape[1], axis=1)
    return len(twin.tape) * (tb.C_STEP_B + 1) * U * (np.abs(ref["X"][j]).astype(LD) * W).sum()


def decay(ref, meshname, j, grad, bound, direction, d0, order, label):
    """Differences of J along `direction` ((nCells, K), added to the uniform kappaV of every step) at d0, d0 / 2, d0 / 4 against `grad`:
    central (order 2: the discrepancy must fall by 3 .. 5 per halving) or one-sided (order 1: by 1.5 .. 2.5), unless the smaller
    discrepancy is already at the floor bound + 2 eps_J / delta; the decay must be seen at least once."""
    steps = ref["steps"]
    base = lambda n: np.full(ref["X"][j].shape, steps[n][0][j])           # noqa: E731
    eJ = eps_J(ref, meshname, j)
    J0 = J_of(ref, j, base) if order == 1 else None
    disc = []
    for i in range(3):
        d = d0 / 2 ** i
        up = J_of(ref, j, lambda n: base(n) + d * direction)
        fd = (up - J0) / LD(d) if order == 1 else (up - J_of(ref, j, lambda n: base(n) - d * direction)) / (2 * LD(d))
        disc.append((abs(fd - LD(grad)), bound + 2 * eJ / LD(d)))
    ratios = [float(disc[i][0] / disc[i + 1][0]) for i in range(2)]
    lo, hi = (3.0, 5.0) if order == 2 else (1.5, 2.5)
    print(f"{label} tracer {j}: gradient {float(grad):.6e}, discrepancies {[f'{float(x[0]):.3e}' for x in disc]}, ratios "
          f"{[f'{r:.3f}' for r in ratios]}, floors {[f'{float(x[1]):.3e}' for x in disc]}")
    for i in range(2):
        assert lo <= ratios[i] <= hi or disc[i + 1][0] <= disc[i + 1][1]
    assert lo <= ratios[0] <= hi                        # the decay is seen at least once: the floor is not what passes the test
    assert disc[2][0] < 0.05 * abs(grad)


@pytest.mark.parametrize("meshname,K", [("planar", 6), ("tiny-4-4", 5)])
def test_central_differences_uniform(meshname, K):
    """J(kappaV +- delta) with the coefficient of EVERY recorded step moved: the step is rational in kappaV, so delta starts at
    kappaV / 8 (inside the 3 .. 5 band for the long-double model alone, as the printed ratios show) and is halved twice."""
    ref = tg.reference(meshname, K, "linear", False, 3, NSTEPS, ALL3)
    ld = check_against_ld(ref, "fd")
    ones = np.ones(ref["X"][0].shape)
    for j in (0, 2):
        grad = tk.host_sum(ref["D"][j].ravel())
        decay(ref, meshname, j, grad, ld[j][3], ones, ref["steps"][0][0][j] / 8, 2, f"{meshname} uniform")


@pytest.mark.parametrize("meshname,K", [("planar", 6), ("tiny-4-4", 5)])
def test_per_interface_claim(meshname, K):
    """<D, dkappa> for a seeded random non-negative field dkappa[k,c] against central differences of the per-interface forward."""
    ref = tg.reference(meshname, K, "linear", False, 3, NSTEPS, ALL3)
    ld = check_against_ld(ref, "per interface")
    for j in (0, 2):
        dk = np.random.default_rng(40 + j).uniform(0.0, 1.0, ref["X"][j].shape)
        grad = (ref["D"][j].astype(LD) * dk).sum()
        bound = (ld[j][1] * dk).sum() + U * abs(grad)                    # the element bounds against dkappa, and the sum's own rounding
        decay(ref, meshname, j, grad, bound, dk, ref["steps"][0][0][j] / 8, 2, f"{meshname} per interface")


@pytest.mark.parametrize("meshname,K", [("planar", 6), ("tiny-4-4", 5)])
def test_derivative_at_zero(meshname, K):
    """Tracer 1 has kappaV == 0 in every step: D against the long-double D at s = 0 (A = diag(h)), and the one-sided difference
    (J(delta) - J(0)) / delta, whose discrepancy delta J'' / 2 halves with delta.  delta starts at 1 / 4096 of the smallest mixed
    coefficient (s / hm^2 = 3 / 4096): the long-double model alone is inside 1.5 .. 2.5 there, as the printed ratios show."""
    ref = tg.reference(meshname, K, "linear", False, 3, NSTEPS, ALL3)
    assert all(kv[1] == 0.0 for kv, _ in ref["steps"])
    ld = check_against_ld(ref, "at zero")
    grad = tk.host_sum(ref["D"][1].ravel())
    assert grad != 0.0
    scale = min(ref["steps"][0][0][0], ref["steps"][0][0][2])
    decay(ref, meshname, 1, grad, ld[1][3], np.ones(ref["X"][1].shape), scale / 4096, 1, f"{meshname} at zero")


# ---- the vertical cosine mode -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 7])
def test_vertical_cosine_mode(m):
    """test_tracer_vmix_twin.py's mode: uniform h, the fluid at rest, n = K = 8, phi0 = 1 + 0.5 cos(pi m (k + 1/2) / n) in every cell.  With
    lam = 2 - 2 cos(pi m / n) a step multiplies the mode by a(kappaV) = 1 / (1 + dt kappaV lam / h^2), so J = <X, phi_N> has
    d J / d kappaV = N a^(N-1) a' <X, 0.5 mode>,  a' = -(dt lam / h^2) a^2.  Nothing in that expression shares code with the twin.
    Tolerance: the counted bound of the density alone (density_ld's, summed, plus the rounding of the sum).  That the twin's p and X
    differ from the closed form's by the round-off of the steps before them is NOT added: the test asks more than a derived bound
    would."""
    n, hval, dtv, N = 8, 8.0, 2.0, 5
    kv = 2.0 * hval * hval / dtv
    mesh = tc.get_mesh("tiny-4-4")
    om = orc.OracleMesh(mesh, n, resting_thickness_sum=np.full(mesh.nCells, n * hval), max_level_edge_top=n)
    twin = tg.VgradTwin(om, om, [0.0], [kv])
    h = np.full((mesh.nCells, n), hval)
    st = TwinState(np.zeros(mesh.nCells), np.zeros((mesh.nEdges, n)), h)
    mode = np.cos(np.pi * m * (np.arange(n) + 0.5) / n)
    phi0 = np.repeat((1 + 0.5 * mode)[None, :], mesh.nCells, axis=0)
    phis = [[phi0.copy()], [phi0.copy()]]
    for _ in range(N):
        twin.step_rk4(st, phis, dtv)
    X = ta.seeds(mesh, n, 1)[:1]
    adj = tg.VgradAdjointTwin(twin)
    D = adj.sweep_vgrad(twin.tape, [X[0].copy()], (0,))[3][0]
    _, B = tg.density_ld(adj, twin.tape, X, 0)
    lam = LD(2) - 2 * np.cos(LD(np.pi) * m / n)
    a = 1 / (1 + LD(dtv) * LD(kv) * lam / LD(hval) ** 2)
    da = -(LD(dtv) * lam / LD(hval) ** 2) * a * a
    proj = (X[0].astype(LD) * (0.5 * np.cos(LD(np.pi) * m * (np.arange(n) + LD(0.5)) / n))[None, :]).sum()
    expect = N * a ** (N - 1) * da * proj
    got = tk.host_sum(D.ravel())
    tol = B.sum() + U * abs(expect)
    dev = abs(LD(got) - expect)
    wrong = N * a ** N * da * proj                      # a power too many
    print(f"m = {m}: d J / d kappaV = {got:.15e}, expected {float(expect):.15e}, deviation {float(dev):.3e}, tolerance {float(tol):.3e}, "
          f"gap to N a^N a': {float(abs(expect - wrong)):.3e}")
    assert dev <= tol
    assert abs(expect - wrong) > 1e3 * tol and abs(expect) > 1e3 * tol


# ---- consequences -------------------------------------------------------------------------------------------------------------------
def test_constant_columns_have_a_density_of_exactly_zero():
    """The unit tracer stays exactly 1.0, so c == 0 in every interface; a tracer that is constant over each column (here on a flow at
    rest, where it stays so) likewise."""
    ref = tg.reference("planar", 6, "nonlinear", True, 3, NSTEPS, ALL3, fields="unit-first")
    assert all(np.all(rec["phi_new"][0] == 1.0) for rec in ref["twin"].tape)
    assert not ref["D"][0].any() and not np.signbit(ref["D"][0]).any() and ref["D"][1].any() and ref["D"][2].any()
    n, mesh = 6, tc.get_mesh("tiny-4-4")
    om = orc.OracleMesh(mesh, n, resting_thickness_sum=np.full(mesh.nCells, 60.0), max_level_edge_top=n)
    twin = tg.VgradTwin(om, om, [0.0], [3.0])
    st = TwinState(np.zeros(mesh.nCells), np.zeros((mesh.nEdges, n)), np.full((mesh.nCells, n), 10.0))
    f = np.repeat(np.random.default_rng(2).uniform(1, 2, mesh.nCells)[:, None], n, axis=1)
    phis = [[f.copy()], [f.copy()]]
    for _ in range(2):
        twin.step_rk4(st, phis, 5.0)
    D = tg.VgradAdjointTwin(twin).sweep_vgrad(twin.tape, ta.seeds(mesh, n, 1)[:1], (0,))[3][0]
    assert not D.any()


def test_zero_seed_and_two_seeds():
    """A zero seed gives exactly zero; the map is linear in the seed: D(a + b) = D(a) + D(b) within the three counted bounds (and the
    rounding of a + b, one more of the pair's)."""
    ref = tg.reference("planar", 6, "linear", False, 3, NSTEPS, ALL3)
    twin = ref["twin"]
    adj = tg.VgradAdjointTwin(twin)
    X = ref["X"]
    for D in adj.sweep_vgrad(twin.tape, [np.zeros_like(x) for x in X], ALL3)[3].values():
        assert not D.any()
    other = [x[::-1].copy() for x in X]
    both = [a + b for a, b in zip(X, other)]
    Da, Db, Ds = ref["D"], adj.sweep_vgrad(twin.tape, other, ALL3)[3], adj.sweep_vgrad(twin.tape, both, ALL3)[3]
    for j in ALL3:
        bound = sum(tg.density_ld(adj, twin.tape, s, j)[1] for s in (X, other, both, both))
        err = np.abs(Ds[j].astype(LD) - (Da[j].astype(LD) + Db[j].astype(LD)))
        print(f"tracer {j}: max |D(a + b) - D(a) - D(b)| = {float(err.max()):.3e}, at {float((err / np.where(bound > 0, bound, 1)).max()):.3f} of its bound")
        assert np.all(err <= bound) and np.abs(Ds[j]).sum() > 1e3 * bound.sum()


def test_flagging_changes_no_bit_of_X_G_or_W():
    """sweep_vgrad returns sweep_kgrad's X, G and W (asserted record by record inside it) whatever is flagged."""
    kw = dict(diff=True, bih=True, flags=((0, 3), (2, 3)), wants=(2,))
    a = tg.reference("planar", 6, "linear", False, 3, NSTEPS, (0, 2), **kw)
    b = tg.reference("planar", 6, "linear", False, 3, NSTEPS, (), **kw)
    c = tv.reference("planar", 6, "linear", False, 3, NSTEPS, True, True, True, (), kw["flags"], kw["wants"])
    assert not b["D"] and sorted(a["D"]) == [0, 2]
    for j in range(3):
        assert np.array_equal(a["grad"][j], b["grad"][j]) and np.array_equal(a["grad"][j], c["grad"][j])
        assert np.array_equal(a["forward"][-1][1][j], c["forward"][-1][1][j])
    assert np.array_equal(a["G"][2], c["G"][2])
    for j in (0, 2):
        assert all(np.array_equal(x, y) for x, y in zip(a["W"][j], c["W"][j]))


def test_rows_under_the_floor_stay_zero_with_nan_below_it():
    ref = tg.reference("planar", 34, "linear", "floor", 3, NSTEPS, (0, 1), fill=np.nan)
    finite = tg.reference("planar", 34, "linear", "floor", 3, NSTEPS, (0, 1))
    assert ref["dead"].any() and {0, 1, 2, 3, 34} <= set(ref["nlev"].tolist())
    for j in (0, 1):
        D = ref["D"][j]
        assert np.isfinite(D).all() and D.any() and np.array_equal(D, finite["D"][j])
        assert not D[np.arange(34)[None, :] >= (ref["nlev"] - 1)[:, None]].any()
        assert all(np.isnan(rec["phi_new"][j][ref["dead"]]).all() for rec in ref["twin"].tape)


def test_views_are_consistent_with_the_density():
    ref = tg.reference("planar", 6, "linear", "floor", 3, NSTEPS, ALL3)
    for j in ALL3:
        D = ref["D"][j]
        cell, prof, scalar = tg.views(D)
        assert cell.shape == (D.shape[0],) and prof.shape == (6,) and prof[5] == 0.0
        Dl = D.astype(LD)
        assert np.array_equal(cell, Dl.sum(axis=1).astype(np.float64)) or np.all(np.abs(cell - Dl.sum(axis=1)) <= U * np.abs(Dl).sum(axis=1))
        assert np.all(np.abs(prof - Dl.sum(axis=0)) <= U * np.abs(Dl).sum(axis=0))
        # the three views sum to the scalar: each within one rounding of its own entries and one of the total
        for v in (cell, prof):
            assert abs(v.astype(LD).sum() - LD(scalar)) <= U * (np.abs(v).sum() + abs(scalar))
