"""The numpy twin of the implicit vertical mixing of momentum (tests/momentum_vmix_twin.py; moka_set_vertical_viscosity,
moka_surface_stress_upload) against a dense long-double solve, its identities, three analytic cases, its switches, and the header's
text.  No GPU."""
import os
import re

import numpy as np
import pytest

import momentum_vmix_twin as mv
import tracer_cases as tc
import tracer_vmix_twin as tv
from del4_twin import TwinState
from moka_hip import lib as L

LD = mv.LD
U = mv.U53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 34
SH2 = (1e-6, 0.3, 4.0, 1e3)                  # s / hm^2
DEPTHS = (1, 2, 3, 5, 17, 34)
NAMES = ("moka_set_vertical_viscosity", "moka_vertical_viscosity", "moka_surface_stress_upload", "moka_surface_stress_download",
         "moka_has_surface_stress", "moka_state_momentum_vmix_path")


def edge_columns(seed=5):
    """Random edge columns from tc.random_state on "tiny-4-4" (48 edges, K = 34): (h_e, u) with h_e the recipe's 0.5 * (h[c1] + h[c2])."""
    mesh = tc.get_mesh("tiny-4-4")
    _, u, h, _ = tc.random_state(mesh, K, seed)
    c1, c2 = mv.edge_cells(mesh)
    return 0.5 * (h[c1] + h[c2]), u


def forcing(kind, hm, ncol, seed=9):
    """(q, b) of a switch combination for columns of mean thickness hm: q = hm / 2, b of the order of hm."""
    q = 0.5 * hm if "drag" in kind else None
    b = np.random.default_rng(seed).uniform(-1.0, 1.0, ncol) * hm if "stress" in kind else None
    return q, b


# ---- against the dense long-double solve ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nu", "nu+drag", "nu+stress", "nu+drag+stress", "drag", "stress"])
def test_twin_against_the_dense_long_double_solve(kind):
    """|u^ - u| <= 2^-53 (|A^-1| ((C_BR + 1) (|A||z^| + |R^|) + C_R mR) + |u^|) per element -- the bound momentum_vmix_twin's docstring
    counts -- for every depth, n == 1 included (where only drag or stress leave anything to compute), and s / hm^2 from 1e-6 to 1e3."""
    he, u = edge_columns()
    hm = 1000.0 / K
    worst = 0.0
    for sh2 in SH2:
        s = sh2 * hm * hm if "nu" in kind else 0.0
        for n in DEPTHS:
            q, b = forcing(kind, hm, he.shape[0])
            if n == 1 and q is None and b is None:
                continue
            new, exact, err, _ = mv.bounds(he[:, :n], u[:, :n], s, q, b)
            assert np.array_equal(new, mv.pass_cols(he[:, :n], u[:, :n], s, q, b))
            dev = np.abs(new.astype(LD) - exact)
            worst = max(worst, float((dev / (U * err)).max()))
            assert np.all(dev <= U * err), (sh2, n)
            assert not np.array_equal(new, u[:, :n])
    print(f"{kind}: largest |u^ - u| / bound = {worst:.3f}")


# ---- identities -----------------------------------------------------------------------------------------------------------------------
def test_depth_uniform_column_comes_back():
    he, _ = edge_columns()
    for n in DEPTHS[1:]:
        for val in (0.0, 1.0, -0.37):
            x = np.full((he.shape[0], n), val)
            for sh2 in SH2:
                assert np.array_equal(mv.pass_cols(he[:, :n], x, sh2 * (1000.0 / K) ** 2), x)


@pytest.mark.parametrize("kind", ["nu", "nu+drag", "nu+stress", "nu+drag+stress"])
def test_column_momentum(kind):
    """sum_k h u_new - sum_k h u* = dt tau - dt r u_new[n-1] within the counted bound of the solve's residual."""
    he, u = edge_columns()
    hm = 1000.0 / K
    worst = 0.0
    for sh2 in SH2:
        for n in DEPTHS:
            q, b = forcing(kind, hm, he.shape[0])
            if n == 1 and q is None and b is None:
                continue
            new, _, _, mom = mv.bounds(he[:, :n], u[:, :n], sh2 * hm * hm, q, b)
            hl = he[:, :n].astype(LD)
            lhs = (hl * new).sum(axis=1) - (hl * u[:, :n]).sum(axis=1)
            rhs = (b.astype(LD) if b is not None else 0) - (LD(q) * new[:, -1] if q is not None else 0)
            drift = np.abs(lhs - rhs)
            worst = max(worst, float((drift / (U * mom)).max()))
            assert np.all(drift <= U * mom), (sh2, n)
    print(f"{kind}: largest momentum drift / bound = {worst:.3f}")


@pytest.mark.parametrize("drag", [False, True])
def test_no_forcing_contraction(drag):
    """Without stress the pass dissipates: sum h u_new^2 < sum h u*^2; without stress and drag every value stays inside the column's
    former range.  s / hm^2 = 4 on full random columns (u uniform in [-1, 1], h within a few per cent of hm): on uniform h the modes
    cos(pi m (k + 1/2) / n) decay by 1 / (1 + 4 (2 - 2 cos(pi m / n))), so white noise keeps on average
    (1/pi) int_0^pi dt / (9 - 8 cos t)^2 = 9 / 17^(3/2) = 0.13 of its energy beside the mean's 1 / n; the assertion leaves a factor of
    three: ratio < 0.5.  Range: a value of the new column is a convex combination of the old ones with no weight above
    max_k (A^-1 diag(h))[k,k] < 1 / 2 (asserted from the long-double inverse), so with 34 independent draws the new extremes sit well
    inside; asserted with a margin of 5 % of the former range on either side."""
    he, u = edge_columns()
    hm = 1000.0 / K
    s, q = 4.0 * hm * hm, (0.5 * hm if drag else None)
    new = mv.pass_cols(he, u, s, q)
    e0, e1 = (he.astype(LD) * u.astype(LD) ** 2).sum(axis=1), (he.astype(LD) * new.astype(LD) ** 2).sum(axis=1)
    print(f"drag {drag}: energy ratios {float((e1 / e0).min()):.3f} .. {float((e1 / e0).max()):.3f}")
    assert np.all(e1 < e0) and np.all(e1 < 0.5 * e0)
    if not drag:
        A, inv = mv.dense_ld(he, s)
        S = inv * he.astype(LD)[:, None, :]
        assert np.all(S >= 0) and float(np.abs(S.sum(axis=2) - 1).max()) < 1e-15
        assert float(np.einsum("cii->ci", S).max()) < 0.5
        lo, hi = u.min(axis=1), u.max(axis=1)
        margin = np.minimum(hi - new.max(axis=1), new.min(axis=1) - lo) / (hi - lo)
        print(f"smallest distance of the new extremes from the former range / that range: {float(margin.min()):.3f}")
        assert np.all(margin > 0.05)


# ---- analytic cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 7])
def test_cosine_mode(m):
    """Uniform h, n = 8: cos(pi m (k + 1/2) / n) decays by 1 / (1 + s (2 - 2 cos(pi m / n)) / h^2) per pass.  Tolerance per pass and
    element as in test_tracer_vmix_twin.py::test_vertical_cosine_mode (s / h^2 = 2, |x| <= 1): 13 C_BR for the solve, 4 C_LV for Lv's own
    roundings, 1.5 for the final addition; no RK4 step stands around the pass here."""
    n, hval, nsteps = 8, 8.0, 5
    h = np.full((3, n), hval)
    mode = np.cos(np.pi * m * (np.arange(n) + 0.5) / n)
    x = np.repeat(mode[None, :], 3, axis=0)
    for _ in range(nsteps):
        x = mv.pass_cols(h, x, 2.0 * hval * hval)
    lam = 2 - 2 * np.cos(np.pi * m / n)
    tol = nsteps * (13 * tv.C_BR + 4 * tv.C_LV + 1.5) * U
    dev = float(np.abs(x - (1 / (1 + 2 * lam)) ** nsteps * mode[None, :]).max())
    gap = float(np.abs(x - ((1 - lam) / (1 + lam)) ** nsteps * mode[None, :]).max())
    print(f"m = {m}: deviation {dev:.3e}, tolerance {tol:.3e}, gap to Crank-Nicolson {gap:.3e}")
    assert dev <= tol and gap > tol


def test_fixed_point_of_stress_and_drag():
    """u[n-1] = tau / r, u[k] - u[k+1] = tau hm / nuV: the stress flux passes every interface and leaves through the drag, so the
    profile is a fixed point: A u = h o u + b e_0 exactly, i.e. the exact right-hand side R vanishes.  The twin's result differs from
    the profile by its own error against the exact solution, which is the profile: the bound of mv.bounds."""
    n, hm, dt = 12, 25.0, 2.0
    rng = np.random.default_rng(2)
    h = np.full((4, n), hm)
    nu, r = 4.0 * hm * hm / dt, 0.5 * hm / dt
    tau = rng.uniform(0.5, 1.0, 4)
    u = np.empty((4, n))
    u[:, n - 1] = tau / r
    for k in range(n - 2, -1, -1):
        u[:, k] = u[:, k + 1] + tau * hm / nu
    s, q, b = np.float64(dt) * nu, np.float64(dt) * r, np.float64(dt) * tau
    new, exact, err, _ = mv.bounds(h, u, s, q, b)
    # the profile itself is rounded: |A u - (h o u + b e_0)| <= 2^-53 |A||u| n (each of its n values one division or addition, accumulated)
    A, inv = mv.dense_ld(h, s, q)
    prof = U * n * tv.mv(np.abs(inv), tv.mv(np.abs(A), np.abs(u)))
    dev = np.abs(new.astype(LD) - u.astype(LD))
    print(f"largest deviation from the fixed point / bound: {float((dev / (U * err + prof)).max()):.3f}")
    assert np.all(dev <= U * err + prof)
    # ... and it is this stress that holds it: twice the stress adds b A^-1[0,0] >= b / A[0,0] = b / (h + s / h) = b / (5 h) at the top
    assert np.all((mv.pass_cols(h, u, s, q, 2 * b) - u)[:, 0] > b / (6 * hm))


def test_single_level():
    """n == 1: (h u* + dt tau) / (h + dt r), to two units in the last place of the increment form's operations: the increment
    y = (b - q x) / (h + q) carries four roundings and the final addition one, so |u^ - u| <= 2 * (2 |y| + |u^|) 2^-53 generously covers
    them (2 ulp of each of the two quantities formed)."""
    he, u = edge_columns()
    h1, x = he[:, :1], u[:, :1]
    q, b = 0.5 * h1.mean(), np.random.default_rng(4).uniform(-30.0, 30.0, h1.shape[0])
    for qq, bb in ((q, b), (q, None), (None, b)):
        new = mv.pass_cols(h1, x, 123.0, qq, bb)
        hl, xl = h1[:, 0].astype(LD), x[:, 0].astype(LD)
        exact = (hl * xl + (bb.astype(LD) if bb is not None else 0)) / (hl + (LD(qq) if qq is not None else 0))
        y = np.abs(exact - xl)
        assert np.all(np.abs(new[:, 0] - exact) <= 2 * U * (2 * y + np.abs(new[:, 0])))
        assert not np.array_equal(new, x)


# ---- switches -------------------------------------------------------------------------------------------------------------------------
def test_switches():
    mesh = tc.get_mesh("tiny-4-4")
    Kc = 6
    _, u, h, _ = tc.random_state(mesh, Kc, 3)
    c1, c2 = mv.edge_cells(mesh)
    mlt = tc.partial_mlt(mesh, Kc)
    assert (mlt == 0).any() and (mlt == 1).any() and (mlt == Kc).any()
    nu, r = mv.coefficients("tiny-4-4", Kc)
    plain = mv.apply(u, h, mlt, c1, c2, 2.0, nu)
    assert not np.array_equal(plain, u)
    dead = np.arange(Kc)[None, :] >= mlt[:, None]
    assert np.array_equal(plain[dead], u[dead]) and np.array_equal(plain[mlt < 2], u[mlt < 2])
    # r = 0 with no stress: the nuV-only bits; a stress that is zero at every active edge counts as absent
    tau0 = np.where(mlt >= 1, 0.0, 7.0)
    assert not mv.stress_on(tau0, mlt) and not mv.pass_on(0.0, 0.0, tau0, mlt)
    assert np.array_equal(mv.apply(u, h, mlt, c1, c2, 2.0, nu, 0.0, tau0), plain)
    assert np.array_equal(mv.apply(u, h, mlt, c1, c2, 2.0, 0.0, 0.0, tau0), u)
    # drag and stress reach the n == 1 columns, nuV alone does not; dt == 0 and the pass switched off change nothing
    tau = mv.stress_field(mesh, Kc)
    full = mv.apply(u, h, mlt, c1, c2, 2.0, nu, r, tau)
    assert np.all(full[mlt == 1, 0] != u[mlt == 1, 0]) and np.array_equal(full[dead], u[dead])
    assert np.array_equal(mv.apply(u, h, mlt, c1, c2, 0.0, nu, r, tau), u)
    # NaN below every edge's own depth -- in u and in both cells' h where no edge of the cell is deeper -- reaches nothing
    celldepth = np.zeros(mesh.nCells, dtype=np.int64)
    np.maximum.at(celldepth, c1, mlt); np.maximum.at(celldepth, c2, mlt)
    up = np.where(dead, np.nan, u)
    hp = np.where(np.arange(Kc)[None, :] >= celldepth[:, None], np.nan, h)
    got = mv.apply(up, hp, mlt, c1, c2, 2.0, nu, r, tau)
    assert np.array_equal(got[~dead], full[~dead]) and np.all(np.isnan(got[dead]))


def test_twin_chain_step_then_pass():
    """MomentumVmixTwin.step_rk4 is the tracer chain's step followed by the pass on the new level; switched off it is that step."""
    ssh, u, h, _ = tc.state_of("tiny-4-4", 6)
    nu, r = mv.coefficients("tiny-4-4", 6)
    a, b, c = (TwinState(ssh, u, h) for _ in range(3))
    tw = mv.momentum_twin("tiny-4-4", 6, nu=nu, drag=r)
    tw.step_rk4(a, [[], []], 2.0)
    tv.vmix_twin("tiny-4-4", 6).step_rk4(b, [[], []], 2.0)
    assert np.array_equal(a.h[1], b.h[1]) and np.array_equal(a.ssh[1], b.ssh[1]) and not np.array_equal(a.u[1], b.u[1])
    assert np.array_equal(a.u[1], tw.mix(b.u[1], b.h[1], 2.0))
    mv.momentum_twin("tiny-4-4", 6).step_rk4(c, [[], []], 2.0)
    assert np.array_equal(c.u[1], b.u[1])


def test_which_form_serves_a_depth():
    assert [mv.form_of(k) for k in (1, 2, 60, 105, 106)] == [2, 1, 1, 1, 2]
    assert mv.form_of(60, generic=True) == 2


# ---- header and symbols ---------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_states_the_recipe():
    text = open(os.path.join(ROOT, "include", "moka_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\(", text), name
        assert name in L.EXPORTS, name
    flat = re.sub(r"\s+", " ", text.replace("\n *", " "))
    for line in ("w[k] = s / (0.5 * (h[k] + h[k+1]))",
                 "d[0] = h[0] + w[0]; d[k] = (h[k] + w[k-1]) + w[k]; d[n-1] = h[n-1] + w[n-2]",
                 "drag on (r != 0): d[n-1] = d[n-1] + q",
                 "R = Lv(x)",
                 "stress present: R[0] = R[0] + b",
                 "drag on: R[n-1] = R[n-1] - q * x[n-1]",
                 "u_new = x + Solve(R)",
                 "h[k] = 0.5 * (h_new[k,c1] + h_new[k,c2])",
                 "Out of scope: reverse mode through the pass"):
        assert line in flat, line
    src = open(os.path.join(ROOT, "mpas-ocean.jl_amd", "Makefile")).read()
    assert "momentum_vmix.o" in src
