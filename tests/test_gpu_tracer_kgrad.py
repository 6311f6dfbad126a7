"""The gradient with respect to kappa_j and kappa4_j on the device (csrc/tracer_adjoint.hip: k_tracer_kgrad; the recording and the
passes of moka_tracer_adjoint_sweep; moka_tracer_adjoint_want_diffusivity_gradient): densities bit for bit against the numpy twin of
tests/tracer_kgrad_twin.py, scalars bit for bit against the host sum of the twin's density.

A case flags tracers, records two RK4 steps of a model whose tracers have pairwise distinct fields, diffusivities (tracer_cases.kappas:
one exact zero, the second) and biharmonic coefficients (tracer_biharmonic_twin.kappa4s: one exact zero, the third -- so a tracer flagged
for kappa4 there has its M computed for the gradient alone), compares both time levels of every tracer and the dycore after each step
(taping with flags changes no forward bit), seeds every tracer with its own field, sweeps, and compares every X, every wanted G, every
density and every scalar; an unflagged tracer or bit refuses the download.  The twin's case is computed once (tk.reference) and shared."""
import ctypes as C

import numpy as np
import pytest

import moka_hip as mk
import tracer_biharmonic_twin as tb
import tracer_cases as tc
import tracer_kgrad_twin as tk
from moka_hip import lib as L

pytestmark = pytest.mark.gpu
BOTH = ((2, True, True),)          # two steps with kappa and kappa4
ALL3 = ((0, 3), (1, 3), (2, 3))
MIXED5 = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 3))          # kappa only, kappa4 only, both, none, both


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)
    yield b
    b.close()


def flag(tape, flags):
    for j, bits in flags:
        if bits:
            tape.want_diffusivity_gradient(j, kappa=bool(bits & 1), biharmonic=bool(bits & 2))


def check_densities(tape, ref, flags, nT):
    """Every flagged density and scalar against the twin, bit for bit; everything unflagged refuses.  Returns what was downloaded."""
    got = {}
    bits = dict(flags)
    for j in range(nT):
        for b, bih, scalar in ((1, False, tape.diffusivity_gradient), (2, True, tape.biharmonic_gradient)):
            if bits.get(j, 0) & b:
                w, exp = tape.diffusivity_density(j, biharmonic=bih), ref["W"][j][b - 1]
                assert np.array_equal(w, exp), ("density", j, b, float(np.abs(w - exp).max()), float(np.abs(exp).max()))
                s = scalar(j)
                assert s == tk.host_sum(exp), ("scalar", j, b, s, tk.host_sum(exp))
                assert np.any(w != 0.0)
                got[(j, b)] = (w, s)
            else:
                with pytest.raises(mk.MokaError):
                    tape.diffusivity_density(j, biharmonic=bih)
                with pytest.raises(mk.MokaError):
                    scalar(j)
    return got


def run_case(md, ref, flags, path=None, wants=()):
    nT = len(ref["fields"])
    tr_ = mk.set_tracers(md.Prog, ref["fields"])
    tape = mk.TracerAdjointTape(md.Prog, len(ref["forward"]))
    try:
        flag(tape, flags)
        for j in wants:
            tape.want_source_gradient(j)
        s = 0
        for kap, kap4, nsteps in zip(ref["kappa"], ref["kappa4"], ref["segments"]):
            tr_.set_diffusivity(kap)
            tr_.set_biharmonic(kap4)
            for _ in range(nsteps):
                tape.step(md.dt)
                tc.check_tracers(tr_, ref["forward"][s])
                tc.check_dycore(md.Prog, ref["forward"][s])
                s += 1
        out = tape.gradient(ref["X"], diffusivity=True)
        grad, dk, dk4 = out
        for j in range(nT):
            assert np.array_equal(grad[j], ref["grad"][j]), ("X", j, float(np.abs(grad[j] - ref["grad"][j]).max()))
            if j in wants:
                assert np.array_equal(tape.source_gradient(j), ref["G"][j]), ("G", j)
        if path is not None:
            assert tape.path() == path and tr_.path() == path
        got = check_densities(tape, ref, flags, nT)
        for j in range(nT):                 # gradient(..., diffusivity=True): the scalars, NaN where not asked
            for b, v in ((1, dk), (2, dk4)):
                assert (v[j] == got[(j, b)][1]) if (j, b) in got else np.isnan(v[j])
    finally:
        tape.close()
    return grad, got


def case(backend, meshname, K, nT, flags, path=None, mode="linear", partial=False, segments=BOTH, wants=(), guard=None, **kw):
    ref = dict(tk.reference(meshname, K, mode, partial, nT, segments, flags, wants))
    ref["segments"] = [s[0] for s in segments]
    md = tc.Model(backend, meshname, K, mode=mode, partial=partial, **kw)
    try:
        if guard:
            guard(md)
        return run_case(md, ref, flags, path, wants)
    finally:
        md.close()


# ---- column shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,lpc,path", [(1, 1, 2), (8, 8, 2), (33, 64, 2), (34, 64, 1), (60, 64, 1), (70, 64, 2)])
def test_column_shapes(backend, K, lpc, path):
    """K = 1: one lane, no shuffle.  K = 8: an eighth of a wave per cell.  K = 33: odd, more than half a wave -- 31 lanes of the tree add
    0.0.  K = 34 and 60: the sweep around it runs the patch form, the new kernel its one form.  K = 70: more levels than lanes, so lanes
    0..5 add two levels each in the strided loop before the tree."""
    def guard(md):
        assert md.info["lanesPerColumn"] == lpc == tk.lanes(K)
    case(backend, "planar", K, 3, ALL3, path, guard=guard, wants=(1,))


def test_pentagons_and_empty_slots(backend):
    case(backend, "ico12f", 5, 3, ALL3, 2)


@pytest.mark.parametrize("K,path", [(6, 2), (34, 1)], ids=["generic", "patch"])
def test_partial_masks(backend, K, path):
    """Levels at and below maxLevelEdgeTop skipped by both Laplacian passes (mlt[:3] = 0: cells whose every slot is masked have L == 0)."""
    case(backend, "planar", K, 3, ALL3, path, partial=True)


@pytest.mark.parametrize("K,path", [(6, 2), (34, 1)], ids=["generic", "patch"])
def test_mixed_flags_over_five_tracers(backend, K, path):
    """kappa only, kappa4 only, both, none, both over one state: an unflagged tracer is neither recorded nor read nor written (its
    downloads refuse), a half-flagged one reads only its factor; five tracers cross the reverse kernels' group of four.  Tracer 1 has
    kappa == 0 and tracer 2 kappa4 == 0 while flagged for exactly that: derivatives at zero, M of tracer 2 computed for the gradient alone."""
    case(backend, "planar", K, 5, MIXED5, path, wants=(3,))


def test_six_flagged_tracers_cross_the_kernels_group(backend):
    """k_tracer_kgrad carries four flagged tracers at a time: six take two groups, the second with two."""
    case(backend, "ico12f", 5, 6, tuple((j, 3) for j in range(6)), 2)


@pytest.mark.parametrize("mode", ["nonlinear", "del2+del4"])
@pytest.mark.parametrize("K,path", [(6, 2), (34, 1)], ids=["generic", "patch"])
def test_dycores(backend, K, path, mode):
    case(backend, "planar", K, 3, ALL3, path, mode=mode, partial=True)


@pytest.mark.parametrize("meshname,K,path", [("ico16", 34, 1), ("ico12f", 5, 2)])
def test_cell_orders_give_identical_results(backend, meshname, K, path):
    """ORDER_NONE and ORDER_RCM: the densities in the caller's numbering and the scalars are identical (each is the twin's, and the two
    are compared with each other): the host sum runs over the caller's numbering."""
    res = [case(backend, meshname, K, 3, ALL3, path, partial=True, ordering=o)[1] for o in (L.ORDER_NONE, L.ORDER_RCM)]
    assert res[0].keys() == res[1].keys() and len(res[0]) == 6
    for key in res[0]:
        assert np.array_equal(res[0][key][0], res[1][key][0]) and res[0][key][1] == res[1][key][1]


@pytest.mark.parametrize("diff,bih", [(False, False), (True, False), (False, True)], ids=["none", "kappa", "kappa4"])
@pytest.mark.parametrize("K,path", [(6, 2), (34, 1)], ids=["generic", "patch"])
def test_derivatives_at_zero(backend, K, path, diff, bih):
    """A state that never set a diffusivity (the plan's dvdc goes to the device for the new passes alone; the sweep keeps its
    diffusion-free instances), one with kappa only (M of every flagged tracer for the gradient alone) and one with kappa4 only."""
    case(backend, "planar", K, 3, ALL3, path, segments=((2, diff, bih),))


# ---- flags change no other bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [6, 34], ids=["generic", "patch"])
def test_flags_change_no_bit_of_anything_else(backend, K):
    """The same run with and without flags, both from the device: X, G, the tracers and the state are bitwise equal."""
    ref = tk.reference("planar", K, "linear", False, 3, BOTH, ALL3, (0, 2))
    res = []
    for flags in ((), ALL3):
        md = tc.Model(backend, "planar", K)
        try:
            tr_ = mk.set_tracers(md.Prog, ref["fields"], diffusivity=ref["kappa"][0], biharmonic=ref["kappa4"][0])
            tape = mk.TracerAdjointTape(md.Prog, 2)
            flag(tape, flags)
            for j in (0, 2):
                tape.want_source_gradient(j)
            tape.step(md.dt)
            tape.step(md.dt)
            grad = tape.gradient(ref["X"])
            res.append(grad + [tape.source_gradient(j) for j in (0, 2)] + [tr_.get(j, lev) for j in range(3) for lev in (0, 1)]
                       + [md.Prog.normalVelocity[-1].get(), md.Prog.layerThickness[-1].get(), md.Prog.ssh[-1].get()])
            tape.close()
        finally:
            md.close()
    assert len(res[0]) == len(res[1]) == 14
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    for j in range(3):
        assert np.array_equal(res[0][j], ref["grad"][j])


# ---- the plane wave -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,path", [(2, 2), (60, 1)])
def test_plane_wave_gradients_on_the_device(backend, K, path):
    """The plane wave of tracer_cases.py with kappa = EIG_KAPPA and kappa4 = EIG_KAPPA4, ten recorded steps, J = <phi0, phi_10>:
    d J / d kappa = <phi0, 0.5 Re(N R^(N-1) R'(z) lam dt e^{ikx})> and the same with -lam^2 for kappa4, to 5e-14 of the magnitude sum;
    the same tolerance refuses R' = R (the exact exponential's derivative).  Nothing in the expectation shares code with the kernels."""
    mesh, state, phi0 = tc.eigenmode_state(K)
    md = tc.Model(backend, "planar-f0", K, state=state)
    try:
        mk.set_tracers(md.Prog, [phi0], diffusivity=[tc.EIG_KAPPA], biharmonic=[tb.EIG_KAPPA4])
        tape = mk.TracerAdjointTape(md.Prog, tc.EIG_STEPS)
        tape.want_diffusivity_gradient(0, kappa=True, biharmonic=True)
        for _ in range(tc.EIG_STEPS):
            tape.step(tc.EIG_DT)
        _, dk, dk4 = tape.gradient([phi0], diffusivity=True)
        assert tape.path() == path
        tape.close()
    finally:
        md.close()
    tk.plane_wave_gradient_check(dk[0], dk4[0], mesh, K, tc.EIG_KAPPA, tb.EIG_KAPPA4, phi0, f"device, K = {K}")


# ---- interface ------------------------------------------------------------------------------------------------------------------------
def test_error_codes(backend):
    meshname, K = "planar", 6
    mesh = tc.get_mesh(meshname)
    md = tc.Model(backend, meshname, K)
    lib = L.lib()
    try:
        mk.set_tracers(md.Prog, tc.distinct_fields(mesh, K, 3))
        tape = mk.TracerAdjointTape(md.Prog, 2)
        h = tape._h
        want, grad, dens = (lib.moka_tracer_adjoint_want_diffusivity_gradient, lib.moka_tracer_adjoint_diffusivity_gradient,
                            lib.moka_tracer_adjoint_diffusivity_density_download)
        out = C.c_double(7.0)
        buf = np.zeros(mesh.nCells)
        assert want(None, 0, 1, 1) == L.ERR_ARG
        for j in (-1, 3):
            assert want(h, j, 1, 1) == L.ERR_ARG
        for bad in (0, 4, 8, 7, -1):
            assert want(h, 0, bad, 1) == L.ERR_ARG
        assert grad(h, 0, 1, C.byref(out)) == L.ERR_ARG                     # nothing flagged yet
        assert dens(h, 0, 1, L.f64(buf)) == L.ERR_ARG
        assert want(h, 0, 1, 1) == 0
        assert grad(h, 0, 1, C.byref(out)) == 0 and out.value == 0.0         # flagged, nothing swept: zeros
        assert dens(h, 0, 1, L.f64(buf)) == 0 and not buf.any()
        assert grad(h, 0, 2, C.byref(out)) == L.ERR_ARG                     # the other bit is not flagged
        assert dens(h, 0, 2, L.f64(buf)) == L.ERR_ARG
        assert grad(h, 1, 1, C.byref(out)) == L.ERR_ARG                     # nor is the other tracer
        for bad in (0, 3, 4):                                               # results take exactly one bit
            assert grad(h, 0, bad, C.byref(out)) == L.ERR_ARG and dens(h, 0, bad, L.f64(buf)) == L.ERR_ARG
        assert grad(h, 0, 1, None) == L.ERR_ARG and dens(h, 0, 1, None) == L.ERR_ARG
        assert grad(None, 0, 1, C.byref(out)) == L.ERR_ARG and dens(None, 0, 1, L.f64(buf)) == L.ERR_ARG
        for j in (-1, 3):
            assert grad(h, j, 1, C.byref(out)) == L.ERR_ARG and dens(h, j, 1, L.f64(buf)) == L.ERR_ARG
        assert want(h, 0, 2, 1) == 0 and grad(h, 0, 2, C.byref(out)) == 0    # a second bit for the same tracer
        assert want(h, 0, 2, 0) == 0 and grad(h, 0, 2, C.byref(out)) == L.ERR_ARG
        tape.step(md.dt)
        assert want(h, 1, 1, 1) == L.ERR_ARG                                # a flag after a recorded step
        assert want(h, 0, 1, 0) == L.ERR_ARG                                # ... in either direction
        with pytest.raises(mk.MokaError, match="no recorded step"):
            tape.want_diffusivity_gradient(1)
        tape.gradient([None] * 3)
        assert want(h, 1, 1, 1) == 0                                        # the tape is empty again
        assert want(h, 0, 1, 0) == 0 and want(h, 1, 1, 0) == 0              # no flag left: the tape of before
        assert grad(h, 0, 1, C.byref(out)) == L.ERR_ARG
        tape.step(md.dt)
        tape.gradient([None] * 3)
        tape.close()
    finally:
        md.close()


def test_life_cycle_and_rezeroing(backend):
    """seed -> sweep -> download; record again; the densities stay readable until the first new seed zeroes them; the second sweep
    accumulates from zero: the twin's sweep over the second pair of records alone."""
    meshname, K, nT = "planar", 6, 3
    ref = tk.reference(meshname, K, "linear", False, nT, ((4, True, True),), ALL3)
    twin = ref["twin"]
    adj = tk.KgradAdjointTwin(twin)
    exp = [adj.sweep_kgrad(twin.tape[a:b], [x.copy() for x in ref["X"]], dict(ALL3)) for a, b in ((0, 2), (2, 4))]
    md = tc.Model(backend, meshname, K)
    try:
        tr_ = mk.set_tracers(md.Prog, ref["fields"], diffusivity=ref["kappa"][0], biharmonic=ref["kappa4"][0])
        tape = mk.TracerAdjointTape(md.Prog, 2)
        flag(tape, ALL3)
        for rnd in range(2):
            tape.step(md.dt)
            tape.step(md.dt)
            tc.check_tracers(tr_, ref["forward"][2 * rnd + 1])
            if rnd == 1:
                assert np.array_equal(tape.diffusivity_density(0), exp[0][2][0][0])          # still the first sweep's
                tape.seed(0, ref["X"][0])
                for j in range(nT):
                    assert not tape.diffusivity_density(j).any() and not tape.diffusivity_density(j, biharmonic=True).any()
                    assert tape.diffusivity_gradient(j) == 0.0 and tape.biharmonic_gradient(j) == 0.0
            grad = tape.gradient(ref["X"])
            Xe, _, We = exp[rnd]
            for j in range(nT):
                assert np.array_equal(grad[j], Xe[j])
                assert np.array_equal(tape.diffusivity_density(j), We[j][0])
                assert np.array_equal(tape.diffusivity_density(j, biharmonic=True), We[j][1])
                assert tape.diffusivity_gradient(j) == tk.host_sum(We[j][0]) and tape.biharmonic_gradient(j) == tk.host_sum(We[j][1])
        assert not np.array_equal(exp[0][2][0][0], exp[1][2][0][0])
        tape.close()
        # state first, tape second, with flags on
        tape = mk.TracerAdjointTape(md.Prog, 1)
        flag(tape, ALL3)
        tape.step(md.dt)
    finally:
        md.close()
    assert not tape._h
