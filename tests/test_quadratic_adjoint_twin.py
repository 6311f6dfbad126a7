"""The numpy twin of reverse mode through the quadratic bottom drag (tests/quadratic_adjoint_twin.py) against its long-double model,
against differences of the forward twin, and against the identities the header states.  No GPU; tests/test_gpu_quadratic_adjoint.py
holds the device to this twin bit for bit.

Differences: the scheme, margins and floor of tests/test_forced_adjoint_twin.py (`decay`, `eps_J`), the forward now
quadratic_drag_twin's pass behind the oracle's RK4 step.  The quadratic pass adds, per step, the roundings momentum_vmix_twin counts
for a column (C_SOLVE + C_R) and quadratic_drag_twin's C_Q for q_e on the magnitude it updates; the floor takes
C_STEP_Q = tracer_biharmonic_twin.C_STEP_B + C_SOLVE + C_R + C_Q.  For the free-seed pairing J = <SU, u_N> + <SH, h_N> the same count
stands on sum |SU||u_N| + sum |SH||h_N|.  Every test but the last runs without the library; the last one fails without the feature."""
import numpy as np
import pytest

import forced_adjoint_twin as fa
import momentum_vfield_twin as mf
import momentum_vmix_twin as mv
import poison_cases as pc
import quadratic_adjoint_twin as qa
import quadratic_drag_twin as qd
import test_forced_adjoint_twin as tfa
import tracer_biharmonic_twin as tb
import tracer_cases as tc

LD = fa.LD
NSTEPS = 3
_WORST = {"ratio": 0.0}


def mask_of(meshname, K, mask):
    return None if not mask else pc.mask_of(meshname, K) if mask == "basin" else tc.partial_mlt(tc.get_mesh(meshname), K)


def depths(meshname, K, mask):
    mlt = mask_of(meshname, K, mask)
    return np.full(tc.get_mesh(meshname).nEdges, K, dtype=np.int32) if mlt is None else mlt


def make(meshname, K, nu, drag, tau, cd, mask=False, state=None, **kw):
    om = tc.oracle_mesh(meshname, K, False, mask_of(meshname, K, mask))
    ssh, u, h, _ = state if state is not None else tc.state_of(meshname, K)
    tw = qa.QuadraticForcedTwin(om, ssh, u, h, **kw)
    tw.nu, tw.drag, tw.tau, tw.cd = nu, drag, tau, cd
    return tw


def settings(meshname, K):
    nu, r = mv.coefficients(meshname, K)
    return nu, r, mv.stress_field(tc.get_mesh(meshname), K), qd.cd_of(K, tc.dt_of(meshname))


# ---- one transposed pass on random data -----------------------------------------------------------------------------------------------
def pass_case(meshname, K, mask, seed=11):
    mesh, mlt = tc.get_mesh(meshname), depths(meshname, K, mask)
    rng = np.random.default_rng(seed)
    XU, XH = rng.uniform(-1, 1, (mesh.nEdges, K)), rng.uniform(-1, 1, (mesh.nCells, K))
    un, us = rng.uniform(-1, 1, XU.shape), rng.uniform(-1, 1, XU.shape)
    hn = (1000.0 / K) * rng.uniform(0.5, 1.5, XH.shape)
    return mesh, mlt, XU, XH, un, hn, us


CASES = [("planar", 6, "basin"), ("planar", 6, True), ("ico12f", 5, True), ("tiny-4-4", 5, False)]


def against_ld(meshname, K, mask, chain):
    mesh, mlt, XU, XH, un, hn, us = pass_case(meshname, K, mask)
    nu, r, _, cd = settings(meshname, K)
    dt = tc.dt_of(meshname)
    dens = {qa.QUADRATIC: np.zeros(mesh.nEdges)}
    oU, _ = qa.transposed_pass(mesh, mlt, XU, XH, un, hn, dt, nu, r, None, None, dens, None, cd, qd.bottom_speed(us, mlt, mesh), us, chain)
    lU, lD, bU, bD = qa.transpose_ld(mesh, mlt, XU, un, hn, us, dt, nu, r, cd)
    live = np.arange(K)[None, :] < np.minimum(mlt, K)[:, None]
    errU, errD = np.abs(oU.astype(LD) - lU), np.abs(dens[qa.QUADRATIC].astype(LD) - lD)
    return live, errU, bU, errD, bD, oU, XU, lU


@pytest.mark.parametrize("meshname,K,mask", CASES)
def test_long_double_bound(meshname, K, mask):
    """XU after the transposed pass and the stencil's transpose, and D_cd, against the long-double model that scatters the chain term
    through cellsOnEdge, within the counted bound; the rows k >= n_e keep their bits."""
    live, errU, bU, errD, bD, oU, XU, lU = against_ld(meshname, K, mask, qa.speed_transpose)
    ratio = max(float((errU[live] / bU[live]).max()), float((errD[bD > 0] / bD[bD > 0]).max()))
    _WORST["ratio"] = max(_WORST["ratio"], ratio)
    print(f"{meshname} K = {K} mask = {mask}: largest error / bound = {ratio:.3f} (largest so far {_WORST['ratio']:.3f}); "
          f"|XU| up to {float(np.abs(lU[live]).max()):.3e}")
    assert np.all(errU[live] <= bU[live]) and np.all(errD <= bD)
    assert np.array_equal(oU[~live], XU[~live])
    assert np.any(oU[live] != 0.0)


@pytest.mark.parametrize("chain", [qa.speed_transpose_no_depth_test, qa.speed_transpose_one_cell], ids=["no-depth-test", "one-cell"])
@pytest.mark.parametrize("meshname,K,mask", CASES[:3])
def test_mutants_fail_the_long_double_bound_on_masked_meshes(meshname, K, mask, chain):
    """The two deliberate mistakes are outside the bound: the masked meshes can tell them from the recipe."""
    mesh, mlt = tc.get_mesh(meshname), depths(meshname, K, mask)
    deeper, shallower = qa.neighbour_levels(mesh, mlt, K)
    assert deeper.any() and shallower.any()
    live, errU, bU, errD, bD, oU, XU, lU = against_ld(meshname, K, mask, chain)
    bad_live = np.any(errU[live] > bU[live])
    bad_below = not np.array_equal(oU[~live], XU[~live])
    assert bad_below if chain is qa.speed_transpose_no_depth_test else bad_live


# ---- differences of the forward twin --------------------------------------------------------------------------------------------------
def c_step(meshname):
    return tb.C_STEP_B + mv.C_SOLVE + mv.C_R + qd.counts(tc.get_mesh(meshname))[2]


def run(meshname, K, nu, r, tau, cd, mask=False, u0=None, **kw):
    ssh, u, h, _ = tc.state_of(meshname, K)
    tw = make(meshname, K, nu, r, tau, cd, mask, state=(ssh, u if u0 is None else u0, h, None), **kw)
    for _ in range(NSTEPS):
        tw.step(tc.dt_of(meshname))
    return tw


def J_ssh(tw):
    s = tw.st.ssh[1].astype(LD)
    return (s * s).sum()


def eps_ssh(tw, meshname):
    return NSTEPS * c_step(meshname) * fa.U53 * (2 * np.abs(tw.st.ssh[1]).astype(LD) * np.abs(tw.st.h[1]).astype(LD).sum(axis=1)).sum()


def seeds(meshname, K, mask):
    mesh, mlt = tc.get_mesh(meshname), depths(meshname, K, mask)
    rng = np.random.default_rng(41)
    SU, SH = rng.uniform(-1, 1, (mesh.nEdges, K)), rng.uniform(-1, 1, (mesh.nCells, K))
    SU[np.arange(K)[None, :] >= np.minimum(mlt, K)[:, None]] = 0.0        # (inactive levels never change: they carry no sensitivity)
    return SU, SH


def J_pair(tw, S):
    return (S[0].astype(LD) * tw.st.u[1].astype(LD)).sum() + (S[1].astype(LD) * tw.st.h[1].astype(LD)).sum()


def eps_pair(tw, S, meshname):
    return NSTEPS * c_step(meshname) * fa.U53 * ((np.abs(S[0]) * np.abs(tw.st.u[1])).astype(LD).sum() + (np.abs(S[1]) * np.abs(tw.st.h[1])).astype(LD).sum())


def target_entries(meshname, K, mask):
    """An edge e' with a neighbour whose bottom level kb lies above e''s own: the entries (e', kb), at that neighbour's bottom level,
    and (e', kb - 1), above it."""
    mesh, mlt = tc.get_mesh(meshname), depths(meshname, K, mask)
    touched = qa.speed_transpose(mesh, mlt, np.zeros((mesh.nEdges, K)), np.ones((mesh.nEdges, K)), np.ones(mesh.nEdges)) != 0.0
    nn = np.minimum(mlt, K)
    for e in range(mesh.nEdges):
        for k in range(1, nn[e] - 1):
            if touched[e, k] and not touched[e, k - 1]:
                return (e, k), (e, k - 1)
    raise AssertionError("no such edge on this mask")


@pytest.mark.parametrize("functional", ["ssh", "pairing"])
@pytest.mark.parametrize("meshname,K,mask", [("tiny-4-4", 5, False), ("planar", 6, True)])
def test_central_differences(meshname, K, mask, functional):
    nu, r, tau, cd = settings(meshname, K)
    S = seeds(meshname, K, mask)
    J = J_ssh if functional == "ssh" else (lambda tw: J_pair(tw, S))
    base = run(meshname, K, nu, r, tau, cd, mask, want=7, want_cd=True)
    eJ = eps_ssh(base, meshname) if functional == "ssh" else eps_pair(base, S, meshname)
    XU, XH = base.sweep(*(base.seed_sum_sq_ssh() if functional == "ssh" else S))
    g = base.gradients()
    u = tc.state_of(meshname, K)[1]
    label = f"{meshname} {functional}"
    tfa.decay(lambda d: J(run(meshname, K, nu, r, tau, cd + d, mask)), g["quadraticDrag"], cd / 8, 2, eJ, f"{label} Cd")
    entries = target_entries(meshname, K, mask) if mask else ((7, K - 1), (7, K // 2))
    for e, k in entries:
        def Ju(d):
            v = u.copy(); v[e, k] += d
            return J(run(meshname, K, nu, r, tau, cd, mask, u0=v))
        tfa.decay(Ju, XU[e, k], 0.5, 2, eJ, f"{label} u0[{e},{k}]")
    tfa.decay(lambda d: J(run(meshname, K, nu, r + d, tau, cd, mask)), g["bottomDrag"], r / 8, 2, eJ, f"{label} r")
    tfa.decay(lambda d: J(run(meshname, K, nu + d, r, tau, cd, mask)), g["viscosity"], nu / 8, 2, eJ, f"{label} nu")
    e = entries[0][0]

    def Jt(d):
        v = tau.copy(); v[e] += d
        return J(run(meshname, K, nu, r, v, cd, mask))
    tfa.decay(Jt, g["surfaceStress"][e], (1000.0 / K) / 4, 2, eJ, f"{label} tau[{e}]")


def test_one_sided_difference_at_zero():
    """Cd == 0 in every step and the flag set: the density is the derivative at zero, and the flag changes no bit of X or of the
    other densities."""
    meshname, K = "tiny-4-4", 5
    nu, r, tau, cd = settings(meshname, K)
    tw = run(meshname, K, nu, r, tau, 0.0, want=7, want_cd=True)
    eJ = eps_ssh(tw, meshname)
    XU, XH = tw.sweep(*tw.seed_sum_sq_ssh())
    g = tw.gradients()
    plain = run(meshname, K, nu, r, tau, 0.0, want=7)
    PU, PH = plain.sweep(*plain.seed_sum_sq_ssh())
    assert np.array_equal(PU, XU) and np.array_equal(PH, XH)
    assert all(np.array_equal(plain.dens[b], tw.dens[b]) for b in (1, 2, 4))
    assert g["quadraticDrag"] != 0.0
    tfa.decay(lambda d: J_ssh(run(meshname, K, nu, r, tau, d)), g["quadraticDrag"], cd / 4096, 1, eJ, "Cd at zero")


# ---- identities ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K,mask", [("planar", 6, "basin"), ("tiny-4-4", 5, False)])
def test_resting_bottom_flow_is_the_linear_drag_transpose(meshname, K, mask):
    """u* exactly zero wherever a bottom speed reads it: sp == 0, M == 0 (the choice at the kink), everything finite, and XU, XH and
    the old densities have the bits of the linear-drag transpose with r alone."""
    mesh, mlt, XU, XH, un, hn, us = pass_case(meshname, K, mask)
    nu, r, _, cd = settings(meshname, K)
    tau = mv.stress_field(mesh, K)
    dt = tc.dt_of(meshname)
    read = qa.speed_transpose(mesh, mlt, np.zeros(XU.shape), np.ones(XU.shape), np.ones(mesh.nEdges)) != 0.0
    us[read] = 0.0
    sp = qd.bottom_speed(us, mlt, mesh)
    assert not sp.any() and np.any(us != 0.0)
    dens = {b: np.zeros(mesh.nEdges) for b in (1, 2, 4, qa.QUADRATIC)}
    parts = {}
    oU, oH = qa.transposed_pass(mesh, mlt, XU, XH, un, hn, dt, nu, r, tau, None, dens, None, cd, sp, us, parts=parts)
    ref = {b: np.zeros(mesh.nEdges) for b in (1, 2, 4)}
    rU, rH = mf.transposed_pass(mesh, mlt, XU, XH, un, hn, dt, nu, r, tau, None, ref)
    assert not parts["M"].any() and not dens[qa.QUADRATIC].any()
    assert np.all(np.isfinite(oU)) and np.all(np.isfinite(oH))
    assert np.array_equal(oU, rU) and np.array_equal(oH, rH) and all(np.array_equal(dens[b], ref[b]) for b in (1, 2, 4))


def test_cd_zero_without_the_flag_is_the_forced_twin_bit_for_bit():
    meshname, K = "planar", 6
    nu, r, tau, _ = settings(meshname, K)
    tw = run(meshname, K, nu, r, tau, 0.0, True, want=7)
    XU, XH = tw.sweep(*tw.seed_sum_sq_ssh())
    ref = tfa.make(meshname, K, nu, r, tau, want=7, mlt=mask_of(meshname, K, True))
    for _ in range(NSTEPS):
        ref.step(tc.dt_of(meshname))
    assert np.array_equal(tw.st.u[1], ref.st.u[1])
    RU, RH = ref.sweep(*ref.seed_sum_sq_ssh())
    assert np.array_equal(XU, RU) and np.array_equal(XH, RH)
    assert all(np.array_equal(tw.dens[b], ref.dens[b]) for b in (1, 2, 4))
    g, rg = tw.gradients(), ref.gradients()
    assert g["viscosity"] == rg["viscosity"] and g["bottomDrag"] == rg["bottomDrag"] and "quadraticDrag" not in g


def test_nan_below_every_level_does_not_travel():
    """XU, un and us NaN in the rows k >= n_e: the active rows and D_cd keep the bits of the unpoisoned pass."""
    meshname, K = "planar", 6
    mesh, mlt, XU, XH, un, hn, us = pass_case(meshname, K, "basin")
    nu, r, _, cd = settings(meshname, K)
    dt = tc.dt_of(meshname)
    below = np.arange(K)[None, :] >= np.minimum(mlt, K)[:, None]
    sp = qd.bottom_speed(us, mlt, mesh)
    clean = {qa.QUADRATIC: np.zeros(mesh.nEdges)}
    cU, cH = qa.transposed_pass(mesh, mlt, XU, XH, un, hn, dt, nu, r, None, None, clean, None, cd, sp, us)
    pU, pun, pus = XU.copy(), un.copy(), us.copy()
    pU[below], pun[below], pus[below] = np.nan, np.nan, np.nan
    dens = {qa.QUADRATIC: np.zeros(mesh.nEdges)}
    oU, oH = qa.transposed_pass(mesh, mlt, pU, XH, pun, hn, dt, nu, r, None, None, dens, None, cd, sp, pus)
    assert np.all(np.isnan(oU[below])) and np.array_equal(oU[~below], cU[~below]) and np.array_equal(oH, cH)
    assert np.array_equal(dens[qa.QUADRATIC], clean[qa.QUADRATIC])


# ---- the library --------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_new_symbols():
    from moka_hip import lib as L
    lib = L.lib()
    for name in ("moka_forced_tape_create_quadratic", "moka_forced_adjoint_want_quadratic_drag_gradient",
                 "moka_forced_adjoint_quadratic_drag_density_download", "moka_forced_adjoint_quadratic_drag_gradient"):
        assert getattr(lib, name) is not None
