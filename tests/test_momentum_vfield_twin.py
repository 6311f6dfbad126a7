"""The numpy twin of the viscosity field (tests/momentum_vfield_twin.py) against its long-double model, against the scalar twins it is
built on, against differences of the forward twin and against the identities the header states.  No GPU;
tests/test_gpu_vviscosity_field.py holds the device to this twin bit for bit.

Differences: the criterion, the floor eps_J and the step sizes are test_forced_adjoint_twin.py's (`decay`: a central difference must
fall by 3 .. 5 per halving of delta, a one-sided one by 1.5 .. 2.5, unless it already sits below the forward round-off floor, with
the decay seen at least once; delta = nu / 8 for central and nu / 4096 for one-sided differences in nu): a single entry of the field
is perturbed where that test perturbs the one nuV."""
import os
import re

import numpy as np
import pytest

import forced_adjoint_twin as fa
import momentum_vfield_twin as mf
import momentum_vmix_twin as mv
import poison_cases as pc
import test_forced_adjoint_twin as tfa
import tracer_cases as tc
from moka_hip import lib as L

LD = mf.LD
U53 = mf.U53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("moka_vertical_viscosity_field_upload", "moka_vertical_viscosity_field_download", "moka_has_vertical_viscosity_field",
       "moka_forced_adjoint_want_viscosity_field_gradient", "moka_forced_adjoint_viscosity_field_density_download")


def test_the_five_entry_points_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "moka_hip.h")).read()
    declared = set(re.findall(r"\b(moka_[a-z0-9_]+)\s*\(", hdr))
    jl = open(os.path.join(ROOT, "mpas-ocean.jl_amd", "julia", "MokaHIP.jl")).read()
    lib = L.lib()
    for name in NEW:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name) and f"(:{name}, lib)" in jl, name


# ---- forward ------------------------------------------------------------------------------------------------------------------------
def columns(n, seed, ncol=64, zeros=False):
    rng = np.random.default_rng(seed)
    hm, dt = 1000.0 / 34, 2.0
    h = hm * rng.uniform(0.5, 1.5, (ncol, n))
    x = rng.uniform(-1, 1, (ncol, n))
    f = rng.uniform(0.0, 8.0, (ncol, max(n - 1, 0))) * hm * hm / dt
    if zeros and n > 2:
        f[::3, n // 2] = 0.0
    return rng, hm, dt, h, x, f


@pytest.mark.parametrize("n", [1, 2, 3, 6, 34, 60])
@pytest.mark.parametrize("what", ["field", "field+drag", "field+stress", "field+drag+stress"])
def test_forward_within_the_counted_bound(n, what):
    rng, hm, dt, h, x, f = columns(n, 200 + n + len(what), zeros=True)
    q = np.float64(dt) * (0.5 * hm / dt) if "drag" in what else None
    b = np.float64(dt) * (rng.uniform(-1, 1, h.shape[0]) * hm / 2) if "stress" in what else None
    if n == 1 and q is None and b is None:
        return
    s = np.float64(dt) * f
    new, ld, err, mom = mf.bounds_field(h, x, s, q, b)
    ratio = float((np.abs(new - ld) / (U53 * err)).max())
    print(f"n = {n} {what}: largest error / bound = {ratio:.3f}")
    assert np.all(np.abs(new - ld) <= U53 * err)
    hL = h.astype(LD)
    budget = (hL * new).sum(axis=1) - (hL * x).sum(axis=1)
    if b is not None:
        budget -= b
    if q is not None:
        budget += LD(float(q)) * new[:, -1]
    assert np.all(np.abs(budget) <= U53 * mom)


@pytest.mark.parametrize("n", [2, 3, 7, 34])
def test_a_uniform_field_is_the_scalar_bit_for_bit(n):
    rng, hm, dt, h, x, f = columns(n, 300 + n)
    nu = 4.0 * hm * hm / dt
    q, b = np.float64(dt) * (0.5 * hm / dt), np.float64(dt) * rng.uniform(-1, 1, h.shape[0])
    s_field = np.float64(dt) * np.full((h.shape[0], n - 1), nu)
    s = np.float64(dt) * np.float64(nu)
    assert np.array_equal(mv.pass_cols(h, x, s_field, q, b), mv.pass_cols(h, x, s, q, b))
    un, X = mv.pass_cols(h, x, s, q, b), rng.uniform(-1, 1, h.shape)
    for a, c in zip(fa.adjoint_cols(h, X, un, s_field, q, b), fa.adjoint_cols(h, X, un, s, q, b)):
        assert np.array_equal(a, c)


def forced(meshname, K, nu, drag, tau, fld, want=0, want_field=False, mlt=None):
    om = tc.oracle_mesh(meshname, K, False, mlt)
    ssh, u, h, _ = tc.state_of(meshname, K)
    tw = mf.ForcedFieldTwin(om, ssh, u, h, want, want_field)
    tw.nu, tw.drag, tw.tau, tw.fld = nu, drag, tau, fld
    return tw


def run(tw, meshname, nsteps=2):
    for _ in range(nsteps):
        tw.step(tc.dt_of(meshname))
    XU, XH = tw.sweep(*tw.seed_sum_sq_ssh())
    return XU, XH


@pytest.mark.parametrize("mask", [None, "partial"])
def test_a_uniform_field_on_a_mesh_gives_the_scalar_sweep_and_densities(mask):
    meshname, K = "tiny-4-4", 5
    mesh = tc.get_mesh(meshname)
    mlt = tc.partial_mlt(mesh, K) if mask else None
    nu, r, tau = tfa.settings(meshname, K)
    a = forced(meshname, K, nu, r, tau, None, 7, True, mlt)
    b = forced(meshname, K, 123.0, r, tau, mf.uniform_field(mesh.nEdges, K, a.mlt, nu), 7, True, mlt)      # (the scalar beside a field is not read)
    ref = tfa.make(meshname, K, nu, r, tau, want=7, mlt=mlt)
    Xa, Xb, Xr = run(a, meshname), run(b, meshname), run(ref, meshname)
    assert np.array_equal(a.st.u[1], b.st.u[1]) and np.array_equal(a.st.u[1], ref.st.u[1])
    for p, q, o in zip(Xa, Xb, Xr):
        assert np.array_equal(p, q) and np.array_equal(p, o)
    for bit in (1, 2, 4):
        assert np.array_equal(a.dens[bit], b.dens[bit]) and np.array_equal(a.dens[bit], ref.dens[bit])
    assert np.array_equal(a.DF, b.DF) and np.any(a.DF != 0.0)
    assert np.all(a.DF[~mf.live_of(a.mlt, K)] == 0.0)                # rows k >= n_e - 1 are never written


def test_a_zero_interface_splits_the_column_into_two_solves():
    n, cut = 9, 4
    rng, hm, dt, h, x, f = columns(n, 41)
    f[:, cut] = 0.0
    q, b = np.float64(dt) * (0.5 * hm / dt), np.float64(dt) * rng.uniform(-1, 1, h.shape[0])
    s = np.float64(dt) * f
    whole = mv.pass_cols(h, x, s, q, b)
    top = mv.pass_cols(h[:, :cut + 1], x[:, :cut + 1], s[:, :cut], None, b)
    bot = mv.pass_cols(h[:, cut + 1:], x[:, cut + 1:], s[:, cut + 1:], q, None)
    assert np.array_equal(whole[:, :cut + 1], top) and np.array_equal(whole[:, cut + 1:], bot)


def test_an_all_zero_field_counts_as_nu_zero_and_inactive_rows_are_not_read():
    meshname, K = "planar", 6
    mesh = tc.get_mesh(meshname)
    mlt = tc.partial_mlt(mesh, K)
    c1, c2 = mv.edge_cells(mesh)
    ssh, u, h, _ = tc.state_of(meshname, K)
    nu, r, tau = tfa.settings(meshname, K)
    zero = mf.uniform_field(mesh.nEdges, K, mlt, 0.0)
    assert mf.check_field(zero, mlt) and not mf.field_on(zero, mlt) and not mf.pass_on(nu, 0.0, None, mlt, zero)
    assert np.array_equal(mf.apply(u, h, mlt, c1, c2, 2.0, nu, 0.0, None, zero), u)
    assert np.array_equal(mf.apply(u, h, mlt, c1, c2, 2.0, nu, r, tau, zero), mv.apply(u, h, mlt, c1, c2, 2.0, 0.0, r, tau))
    f = mf.case_field(meshname, K, mlt)
    assert np.isnan(f).any() and mf.check_field(f, mlt) and mf.field_on(f, mlt)
    below = np.arange(K)[None, :] >= np.minimum(mlt, K)[:, None]
    pu = np.where(below, np.nan, u)
    out = mf.apply(pu, h, mlt, c1, c2, 2.0, nu, r, tau, f)
    clean = mf.apply(u, h, mlt, c1, c2, 2.0, nu, r, tau, np.nan_to_num(f, nan=7.0))
    assert np.all(np.isnan(out[below])) and np.array_equal(out[~below], clean[~below])
    bad = f.copy()
    bad[np.nonzero(mlt >= 2)[0][0], 0] = -1.0
    assert not mf.check_field(bad, mlt)


# ---- the transposed pass against long double ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 6, 34])
@pytest.mark.parametrize("what", ["field", "field+drag+stress", "zeros+drag"])
def test_exact_transpose_against_long_double(n, what):
    rng, hm, dt, h, x, f = columns(n, 500 + 7 * n + len(what), zeros=what.startswith("zeros"))
    ncol = h.shape[0]
    r = 0.5 * hm / dt if "drag" in what else 0.0
    tau = rng.uniform(-1, 1, ncol) * hm / 2 if "stress" in what else None
    X = rng.uniform(-1, 1, (ncol, n))
    d = (rng.uniform(-1, 1, (ncol, n)), hm * rng.uniform(-1, 1, (ncol, n)), rng.uniform(-1, 1, ncol) * hm,
         tfa.nu_scale(hm, dt) * rng.uniform(-1, 1, (ncol, n - 1)), hm / dt * rng.uniform(-1, 1))
    T_ld, ld = mf.pairing_ld_field(h, x, X, dt, f, r, tau, d)
    T_tw, tw = mf.pairing_twin_field(h, x, X, dt, f, r, tau, d)
    bound = mf.pairing_bound_field(h, x, X, dt, f, r, tau, d, ld, tw)
    err = np.abs(T_tw - T_ld)
    print(f"n = {n} {what}: largest error / bound = {float((err / bound).max()):.3f}; pairing magnitude {float(np.abs(T_ld).max()):.3e}")
    assert np.all(np.abs(T_ld) > 0) and np.all(err <= bound)


def test_the_field_pairing_at_a_uniform_field_is_the_scalar_pairing():
    """df = dnu at every interface: <DF, df> is D_nu's term up to the order of summation, and the long-double sides agree closely."""
    n = 6
    rng, hm, dt, h, x, f = columns(n, 77)
    ncol = h.shape[0]
    nu, dnu = 4.0 * hm * hm / dt, 0.3 * hm * hm / dt
    X = rng.uniform(-1, 1, (ncol, n))
    zero = np.zeros((ncol, n))
    T_f, _ = mf.pairing_ld_field(h, x, X, dt, np.full((ncol, n - 1), nu), 0.0, None, (zero, zero, np.zeros(ncol), np.full((ncol, n - 1), dnu), 0.0))
    T_s, _ = fa.pairing_ld(h, x, X, dt, nu, 0.0, None, (zero, zero, np.zeros(ncol), dnu, 0.0))
    assert np.all(np.abs(T_f - T_s) <= 64 * np.finfo(LD).eps * np.abs(T_s))


# ---- differences ----------------------------------------------------------------------------------------------------------------------
def J_of(meshname, K, nu, drag, tau, fld):
    tw = forced(meshname, K, nu, drag, tau, fld)
    for _ in range(tfa.NSTEPS):
        tw.step(tc.dt_of(meshname))
    s = tw.st.ssh[1].astype(LD)
    return (s * s).sum(), tw


def swept(meshname, K, nu, drag, tau, fld):
    _, tw = J_of(meshname, K, nu, drag, tau, fld)
    eJ = tfa.eps_J(tw)
    tw2 = forced(meshname, K, nu, drag, tau, fld, 7, True)
    for _ in range(tfa.NSTEPS):
        tw2.step(tc.dt_of(meshname))
    XU, XH = tw2.sweep(*tw2.seed_sum_sq_ssh())
    return tw2, eJ


@pytest.mark.parametrize("meshname,K", [("tiny-4-4", 5), ("planar", 6)])
def test_central_differences_in_single_field_entries(meshname, K):
    """Surface interface, a middle one and the deepest one of an edge, at a field and at the scalar nuV (the uniform field)."""
    mesh = tc.get_mesh(meshname)
    nu, r, tau = tfa.settings(meshname, K)
    full = np.full(mesh.nEdges, K)
    for label, fld in (("field", np.nan_to_num(mf.case_field(meshname, K, full, nan=False))), ("scalar", None)):
        tw, eJ = swept(meshname, K, nu, r, tau, fld)
        base = fld if fld is not None else mf.uniform_field(mesh.nEdges, K, full, nu, nan=False)
        for e, k in ((7, 0), (7, K // 2), (7, K - 2), (11, K - 2)):
            def Jf(d):
                v = base.copy(); v[e, k] += d
                return J_of(meshname, K, nu, r, tau, v)[0]
            tfa.decay(Jf, tw.DF[e, k], nu / 8, 2, eJ, f"{meshname} {label} f[{e},{k}]")


def test_one_sided_difference_at_zero():
    """f == 0 everywhere and nothing else on: every step ran without the pass; DF is the derivative at zero and X keeps its bits."""
    meshname, K = "tiny-4-4", 5
    mesh = tc.get_mesh(meshname)
    nu = tfa.settings(meshname, K)[0]
    full = np.full(mesh.nEdges, K)
    tw, eJ = swept(meshname, K, 0.0, 0.0, None, None)
    plain = tfa.make(meshname, K, 0.0, 0.0, None)
    for _ in range(tfa.NSTEPS):
        plain.step(tc.dt_of(meshname))
    PU, PH = plain.sweep(*plain.seed_sum_sq_ssh())
    tw3 = forced(meshname, K, 0.0, 0.0, None, None, 7, True)
    XU, XH = run(tw3, meshname, tfa.NSTEPS)
    assert np.array_equal(PU, XU) and np.array_equal(PH, XH) and np.array_equal(tw3.DF, tw.DF)
    zero = mf.uniform_field(mesh.nEdges, K, full, 0.0, nan=False)
    for e, k in ((7, 0), (7, K - 2)):
        assert tw.DF[e, k] != 0.0

        def Jf(d):
            v = zero.copy(); v[e, k] = d
            return J_of(meshname, K, 0.0, 0.0, None, v)[0]
        tfa.decay(Jf, tw.DF[e, k], nu / 4096, 1, eJ, f"f[{e},{k}] at zero")


# ---- the sum over depth -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 6, 34])
def test_the_sum_of_DF_over_depth_is_D_nu(n):
    """One step from zero densities: D_nu[e] = 0 - dt * (sum of de / hm), DF[k] = 0 - dt * (de / hm).  Both sum the same n - 1 terms
    t[k] = dt * de[k] / hm[k] in different orders and roundings: each t[k] differs between the two by one rounding (the product with
    dt inside or outside the sum) and each sum of n - 1 terms carries n - 2 additions, so |sum_k DF[k] - D_nu| <= n 2^-53 sum |t[k]|."""
    rng, hm, dt, h, x, f = columns(n, 900 + n)
    s = np.float64(dt) * f
    un, X = mv.pass_cols(h, x, s), rng.uniform(-1, 1, h.shape)
    z, _, _, nusum = fa.adjoint_cols(h, X, un, s)
    t = mf.df_terms(h, z, un, dt)
    DF, Dnu = 0.0 - t, 0.0 - np.float64(dt) * nusum
    tot = DF.astype(LD).sum(axis=1)
    assert np.all(np.abs(tot - Dnu.astype(LD)) <= n * U53 * np.abs(t).astype(LD).sum(axis=1))


def test_the_sum_of_DF_over_depth_is_D_nu_on_a_mesh():
    meshname, K = "planar", 6
    mesh = tc.get_mesh(meshname)
    mlt = pc.mask_of(meshname, K)
    nu, r, tau = tfa.settings(meshname, K)
    tw = forced(meshname, K, nu, r, tau, mf.case_field(meshname, K, mlt), 7, True, mlt)
    run(tw, meshname, 3)
    live = mf.live_of(tw.mlt, K)
    assert np.all(tw.DF[~live] == 0.0) and np.all(np.isfinite(tw.DF))
    tot = np.where(live, tw.DF, 0.0).astype(LD).sum(axis=1)
    # three steps: the bound above per step on that step's terms; |DF| accumulates with signs, so the magnitude is taken step by step
    steps = forced(meshname, K, nu, r, tau, mf.case_field(meshname, K, mlt), 7, True, mlt)
    for _ in range(3):
        steps.step(tc.dt_of(meshname))
    XU, XH = steps.seed_sum_sq_ssh()
    mag = np.zeros(mesh.nEdges, dtype=LD)
    while steps.recs:
        un, hn, nu_, drag_, tau_, fld_ = steps.recs.pop()
        P, dt = steps.rk.tape.pop()
        one = np.zeros((mesh.nEdges, K))
        XU2, XH2 = mf.transposed_pass(mesh, steps.mlt, XU, XH, un, hn, dt, nu_, drag_, tau_, fld_, None, one)
        mag += np.abs(one).astype(LD).sum(axis=1)
        XU, XH = steps.reverse_rk4(P, dt, XU2, XH2)
    nn = np.minimum(tw.mlt, K)
    # + 6: each of the three accumulations rounds both sides once, by at most 2^-53 x the running magnitude <= mag
    assert np.all(np.abs(tot - tw.dens[2].astype(LD)) <= (nn + 6) * U53 * mag)
    assert np.all(tw.dens[2][nn < 2] == 0.0) and np.any(tw.dens[2] != 0.0)


# ---- kernel forms -----------------------------------------------------------------------------------------------------------------------
def test_the_five_set_boundaries_follow_the_formula():
    assert [mf.adjoint_form(K, True) for K in (2, 15, 16, 63, 64)] == [(1, 64), (1, 64), (1, 32), (1, 32), (2, 0)]
    assert [mf.adjoint_form(K, False) for K in (19, 20, 79, 80)] == [(1, 64), (1, 32), (1, 32), (2, 0)]
    assert mf.adjoint_form(34, True, generic=True) == (2, 0) and mf.adjoint_form(1, True) == (2, 0)
    assert 5 * 32 * 63 * 8 + 16 * 32 == 81152 <= 80 * 1024
