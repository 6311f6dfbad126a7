"""Biharmonic tracer diffusion on the device (csrc/tracers.hip: launch_tracer_lap and the BIH instantiations; csrc/tracer_adjoint.hip BIH;
moka_set_tracer_biharmonic): bit for bit against the numpy twins of tests/tracer_biharmonic_twin.py.

A case records 2-4 RK4 steps of a model whose tracers have pairwise distinct fields, diffusivities (tracer_cases.kappas: one exact zero,
the second) and biharmonic coefficients (tracer_biharmonic_twin.kappa4s: <= 0.002 dcmin^4 / dt, one exact zero, the third); compares
both time levels of every tracer and the dycore after each step; seeds every tracer with its own field; and compares every X and every
wanted G, the kernel paths and the premise that makes the case the shape it claims to be.  The twin's schedule is computed once per case
(tb.reference) and shared.  The dycore fields are compared with the twin's, which are those of a tracer-free state."""
import ctypes as C

import numpy as np
import pytest

import moka_hip as mk
import tracer_adjoint_twin as ta
import tracer_biharmonic_twin as tb
import tracer_cases as tc
import trisk_reference as tr
from moka_hip import lib as L

pytestmark = pytest.mark.gpu
BOTH = ((2, True, True),)          # two steps with kappa and kappa4


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)
    yield b
    b.close()


def bih_chunk(maxPatchCells, K, nT, bih=True, diff=True):
    """tracers.hip's tracer_kernel restated from its comment: the tracers resident per pass of the patch form in 80 KB of LDS beside the
    thickness rows and the records (per cell 8 K + 144 bytes, 48 more with diffusion); a tracer takes 8 K bytes per cell, 16 K with the
    biharmonic term (a second row set, for L); 0 = not even one tracer fits (the generic form)."""
    fixed, per = maxPatchCells * (8 * K + 144 + (48 if diff else 0)), maxPatchCells * 8 * K * (2 if bih else 1)
    return 0 if fixed + per > 80 * 1024 else min(max(nT, 1), (80 * 1024 - fixed) // per)


def expected_path(md, K, nT, variant=0, bih=True, diff=True):
    patchable = variant != 3 and K >= 34 and K <= 64 and K % 2 == 0 and md.mesh.edgesOnCell.shape[1] == 6
    return 1 if patchable and bih_chunk(md.info["maxPatchCells"], K, nT, bih, diff) > 0 else 2


def run_case(md, ref, path, wants=(), taped=True):
    """The segments of `ref` on the model: set kappa and kappa4 per segment, step (taped or eager), compare after every step; then seeds,
    sweep, every X and every wanted G."""
    nT = len(ref["fields"])
    tr_ = mk.set_tracers(md.Prog, ref["fields"], sources=ref["sources"])
    nsteps = len(ref["forward"])
    tape = mk.TracerAdjointTape(md.Prog, nsteps) if taped else None
    try:
        for j in wants:
            tape.want_source_gradient(j)
        s = 0
        for kap, kap4, rec in zip(ref["kappa"], ref["kappa4"], ref["segments"]):
            tr_.set_diffusivity(kap)
            tr_.set_biharmonic(kap4)
            assert np.array_equal(tr_.biharmonic(), np.asarray(kap4)) and np.array_equal(tr_.diffusivity(), np.asarray(kap))
            for _ in range(rec):
                if taped:
                    tape.step(md.dt)
                else:
                    md.eager(1)
                tc.check_tracers(tr_, ref["forward"][s])
                tc.check_dycore(md.Prog, ref["forward"][s])
                s += 1
        if path is not None:
            assert tr_.path() == path
        if taped:
            grad = tape.gradient(ref["X"])
            for j in range(nT):
                assert np.array_equal(grad[j], ref["grad"][j]), ("X", j, float(np.abs(grad[j] - ref["grad"][j]).max()))
                if j in wants:
                    G = tape.source_gradient(j)
                    assert np.array_equal(G, ref["G"][j]), ("G", j, float(np.abs(G - ref["G"][j]).max()))
                    assert np.any(G != 0.0)
            if path is not None:
                assert tape.path() == path
    finally:
        if tape is not None:
            tape.close()
    return tr_


def case(backend, meshname, K, nT, path, mode="linear", partial=False, segments=BOTH, srcs=(), wants=(), guard=None, taped=True, pre=0,
         **kw):
    ref = dict(tb.reference(meshname, K, mode, partial, nT, segments, srcs, wants, pre))
    ref["segments"] = [s[0] for s in segments]
    md = tc.Model(backend, meshname, K, mode=mode, partial=partial, **kw)
    try:
        if guard:
            guard(md)
        if path == "rule":
            path = expected_path(md, K, nT, kw.get("variant", 0))
        md.eager(pre)
        run_case(md, ref, path, wants, taped)
    finally:
        md.close()


# ---- the patch form ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [60, 34, 64])
@pytest.mark.parametrize("meshname", ["planar", "ico16"])
def test_patch_form(backend, meshname, K):
    """k_tracer_lap_patch, k_tracer_patch<6, true, ., true> and k_tracer_adj_patch<6, true, ., true>: three tracers -- both terms, the
    biharmonic one alone, the harmonic one alone (its L is never written: the scratch holds zeros from its allocation, and NaNs would
    show) -- forwards and backwards, G of tracer 1 wanted."""
    def guard(md):
        assert bih_chunk(md.info["maxPatchCells"], K, 3) >= 1
    case(backend, meshname, K, 3, 1, wants=(1,), guard=guard)


@pytest.mark.parametrize("nT", [1, 5, 9])
def test_patch_form_tracer_counts(backend, nT):
    """ico16 at K = 64: with two row sets per resident tracer 80 KB hold fewer tracers than the plain form's eight, so five and nine
    tracers take several passes (j0 + jj indexes kappa4 and both row sets in every pass); one tracer: no zero among the kappa4."""
    def guard(md):
        chunk = bih_chunk(md.info["maxPatchCells"], 64, nT)
        assert 1 <= chunk < 8 and (nT < 5 or chunk < nT)
    case(backend, "ico16", 64, nT, 1, guard=guard, wants=(0,))


@pytest.mark.parametrize("patch_cells,K,path", [(12, 64, 1), (24, 64, 1), (48, 60, 1), (48, 64, 2)])
def test_patch_sizes_and_the_lds_boundary(backend, patch_cells, K, path):
    """Patches of 12, 24 and 48 cells.  At 48 cells and K = 60 one tracer's two row sets still fit (78 336 of 81 920 bytes); at K = 64
    they do not (82 944), so the BIH launches take the generic form while the Laplacian pass, and the same state with every kappa4
    zero, keep the patch form: moka_state_tracer_path agrees with the restated rule on both sides of the boundary."""
    def guard(md):
        assert md.info["maxPatchCells"] == patch_cells
        assert (bih_chunk(patch_cells, K, 3) > 0) == (path == 1) and expected_path(md, K, 3) == path
        assert bih_chunk(patch_cells, K, 3, bih=False) > 0
    case(backend, "planar", K, 3, path, patch_cells=patch_cells, guard=guard)
    # ... and the same state with every kappa4 back at zero takes the patch form again, with the bits of the twin that did the same
    md = tc.Model(backend, "planar", K, patch_cells=patch_cells)
    try:
        ref = tb.reference("planar", K, "linear", False, 3, ((1, True, True), (1, True, False)))
        tr_ = mk.set_tracers(md.Prog, ref["fields"], diffusivity=ref["kappa"][0], biharmonic=ref["kappa4"][0])
        md.eager(1)
        assert tr_.path() == path
        tr_.set_biharmonic(None)
        md.eager(1)
        assert tr_.path() == 1
        tc.check_tracers(tr_, ref["forward"][1])
    finally:
        md.close()


# ---- the generic form --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K,variant,lpc", [("planar", 60, 3, 64), ("planar", 35, 0, 64), ("planar", 7, 0, 8), ("planar", 1, 0, 1),
                                                   ("ico12f", 8, 0, 8), ("planar", 2, 0, 2), ("planar", 4, 0, 4), ("planar", 16, 0, 16),
                                                   ("planar", 32, 0, 32)])
def test_generic_form(backend, meshname, K, variant, lpc):
    """k_tracer_lap_cell, k_tracer_cell<LPC, true, ., true> and k_tracer_adj_cell<LPC, true, ., true> at every lane width: kernel variant
    3 at a K the patch form would take, the odd K = 35, K = 7 and 1, heptagons; five tracers -- more than TR_TJ, so kappa4 and L are
    indexed across the group boundary."""
    def guard(md):
        assert md.info["lanesPerColumn"] == lpc
    case(backend, meshname, K, 5, 2, variant=variant, guard=guard, wants=(4,))


def test_generic_form_nine_tracers(backend):
    """Nine tracers in the generic form: three TR_TJ groups, the last with one tracer."""
    case(backend, "ico12f", 5, 9, 2, wants=(8,))


# ---- masks, orders, tiny meshes, dycores -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,partial", [("linear", True), ("nonlinear", False), ("del2+del4", False), ("nonlinear", True)])
@pytest.mark.parametrize("K,path", [(6, 2), (34, 1)], ids=["generic", "patch"])
def test_dycores_and_masks(backend, K, path, mode, partial):
    """The three dycore modes and the partial edge mask (mlt[:3] = 0): the Laplacian pass and both additions skip the same slots; a cell
    whose every slot is masked has L == 0.  The dycore fields stay those of the twin's tracer-free dycore, bit for bit."""
    case(backend, "planar", K, 3, path, mode=mode, partial=partial, wants=(0,))


@pytest.mark.parametrize("ordering", [L.ORDER_NONE, L.ORDER_RCM], ids=["none", "rcm"])
@pytest.mark.parametrize("meshname,K,path", [("ico16", 34, 1), ("ico12f", 5, 2)])
def test_other_cell_orders(backend, meshname, K, path, ordering):
    case(backend, meshname, K, 3, path, ordering=ordering, partial=True)


@pytest.mark.parametrize("nx,ny,K", tc.TINY)
def test_tiny_periodic_meshes(backend, nx, ny, K):
    """The smallest doubly periodic meshes (one patch holds the mesh; a cell meets a neighbour through several slots), in whichever form
    the restated rule gives them."""
    case(backend, f"tiny-{nx}-{ny}", K, 3, "rule")


# ---- DIFF x SRC x BIH ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", [False, True], ids=["nosrc", "src"])
@pytest.mark.parametrize("diff", [False, True], ids=["kappa0", "kappa"])
@pytest.mark.parametrize("K,path", [(6, 2), (34, 1)], ids=["generic", "patch"])
def test_diffusion_times_sources_times_biharmonic(backend, K, path, diff, src):
    """BIH with and without sources, with kappa and with every kappa == 0 (the library then hands the DIFF instantiation an array of
    zeros: the bits are the harmonic-free ones, which is what the twin computes); SG on (a gradient is wanted) and off."""
    case(backend, "planar", K, 3, path, segments=((2, diff, True),), srcs=(0, 2) if src else (), wants=(1, 2) if src else ())


# ---- eager steps, the captured graph, kappa4 switched between steps, tracers set late ------------------------------------------------
@pytest.mark.parametrize("meshname,K,path", [("ico12f", 5, 2), ("planar", 34, 1)])
def test_eager_steps_and_the_captured_graph(backend, meshname, K, path):
    """moka_step_rk4 and mk.run_steps (from 6 steps on one eager step, then the replay of a captured graph, which records the Laplacian
    launch like the others: nothing is allocated inside a step): both time levels after step 1 and after step 7 against the twin.
    Untaped: with the taped cases of this file against the same twin, taping changes no forward bit."""
    n = 7
    ref = tb.reference(meshname, K, "linear", False, 3, ((n, True, True),))
    md = tc.Model(backend, meshname, K)
    try:
        tr_ = mk.set_tracers(md.Prog, ref["fields"], diffusivity=ref["kappa"][0], biharmonic=ref["kappa4"][0])
        md.eager(1)
        tc.check_tracers(tr_, ref["forward"][0])
        md.run(n - 1)
        tc.check_tracers(tr_, ref["forward"][n - 1])
        tc.check_dycore(md.Prog, ref["forward"][n - 1])
        assert tr_.path() == path
    finally:
        md.close()


SWITCHED = ((1, True, False), (1, True, True), (1, False, (0.5, 0.25, 1.0)), (1, True, False))


@pytest.mark.parametrize("taped", [True, False], ids=["taped", "eager"])
@pytest.mark.parametrize("K,path", [(6, 2), (34, 1)], ids=["generic", "patch"])
def test_kappa4_switched_on_changed_and_off_between_steps(backend, K, path, taped):
    """Four steps: without kappa4, with it, with other values (the third tracer's zero times 1.0 stays zero) and every kappa zero, and
    back to none -- the state returns to the launches it had.  Taped, the tape records kappa4 per step and the sweep reverses each step
    with its own values; eager, the same forward bits (taping changes none)."""
    case(backend, "planar", K, 3, path, segments=SWITCHED, wants=(0,) if taped else (), taped=taped)


@pytest.mark.parametrize("K,path", [(6, 2), (34, 1)], ids=["generic", "patch"])
def test_sweep_without_kappa4_is_the_sweep_of_before(backend, K, path):
    """Every recorded kappa4 zero: the twin runs its parents' code (tracer_source_twin.py), the library the launches without BIH."""
    case(backend, "planar", K, 3, path, segments=((2, True, False),), wants=(1,))


def test_tracers_set_late(backend):
    """Two tracer-free steps first; then tracers, kappa and kappa4 arrive and the next steps match the twin that did the same."""
    case(backend, "planar", 34, 3, 1, pre=2)


# ---- end to end: identities and plane waves -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K,mode,path", [("ico12f", 5, "nonlinear", 2), ("planar", 34, "del2+del4", 1)])
def test_inner_product_identity_on_the_device(backend, meshname, K, mode, path):
    """<X, forward(d)> = <gradient, d> with both sides from the device, kappa and kappa4 on: within 2 steps * C_STEP_B * 2^-53 *
    sum |X| W (tracer_biharmonic_twin.py counts the chain), W over the twin's records of the same flow.  Prints observed / bound."""
    nT, nsteps = 2, 2
    mesh = tc.get_mesh(meshname)
    ref = tb.reference(meshname, K, mode, True, nT, BOTH)
    rng = np.random.default_rng(41)
    d = [rng.uniform(-1.0, 1.0, (mesh.nCells, K)) for _ in range(nT)]
    X = ref["X"]
    md = tc.Model(backend, meshname, K, mode=mode, partial=True)
    try:
        tr_ = mk.set_tracers(md.Prog, d, diffusivity=ref["kappa"][0], biharmonic=ref["kappa4"][0])
        tape = mk.TracerAdjointTape(md.Prog, nsteps)
        for _ in range(nsteps):
            tape.step(md.dt)
        Md = [tr_.get(j) for j in range(nT)]
        grad = tape.gradient(X)
        assert tape.path() == path
        tape.close()
    finally:
        md.close()
    twin = ref["twin"]
    for j in range(nT):
        lhs, rhs = ta.dot_ld(X[j], Md[j]), ta.dot_ld(grad[j], d[j])
        W = np.abs(d[j]).astype(tr.LD)
        for rec in twin.tape:
            W = tb.forward_magnitude(mesh, twin.mlt, rec, W, rec["kappa"][j], rec["kappa4"][j])
        bound = nsteps * tb.C_STEP_B * tr.U53 * (np.abs(X[j]).astype(tr.LD) * W).sum()
        print(f"{meshname} {mode} tracer {j}: |<X, M d> - <M^T X, d>| = {float(abs(lhs - rhs)):.3e}, bound = {float(bound):.3e}, "
              f"<X, M d> = {float(lhs):.6e}")
        assert abs(lhs - rhs) <= bound
        assert abs(lhs) > 1e3 * bound


@pytest.mark.parametrize("K,path", [(2, 2), (60, 1)])
def test_plane_waves_on_the_device(backend, K, path):
    """The plane wave of tracer_cases.py with kappa = EIG_KAPPA and kappa4 = 0.002 dc^4 / dt, forwards (R(z)^10) and backwards
    (conj(R(z))^10), z = (mu + kappa lam - kappa4 lam^2) dt, within 10 * 32 * 2^-53 * max|phi0|; the bound refuses kappa4 = 0, the wrong
    sign and a third-order loop (tb.plane_wave_check).  Nothing in the expectation shares code with the twins or the kernels."""
    mesh, state, phi0 = tc.eigenmode_state(K)
    md = tc.Model(backend, "planar-f0", K, state=state)
    try:
        tr_ = mk.set_tracers(md.Prog, [phi0], diffusivity=[tc.EIG_KAPPA], biharmonic=[tb.EIG_KAPPA4])
        tape = mk.TracerAdjointTape(md.Prog, tc.EIG_STEPS)
        for _ in range(tc.EIG_STEPS):
            tape.step(tc.EIG_DT)
        assert tr_.path() == path
        tb.plane_wave_check(tr_.get(0), mesh, K, tc.EIG_KAPPA, tb.EIG_KAPPA4, phi0, f"device forwards, K = {K}")
        grad = tape.gradient([phi0])[0]
        assert tape.path() == path
        tb.plane_wave_check(grad, mesh, K, tc.EIG_KAPPA, tb.EIG_KAPPA4, phi0, f"device backwards, K = {K}", backwards=True)
        tape.close()
    finally:
        md.close()


# ---- interface ---------------------------------------------------------------------------------------------------------------------
def test_interface_errors_reset_and_life_cycle(backend):
    meshname, K = "planar", 6
    mesh = tc.get_mesh(meshname)
    md = tc.Model(backend, meshname, K)
    lib, sh = L.lib(), md.Prog._state._h
    try:
        one = (C.c_double * 1)(1.0)
        out = C.c_double(-1.0)
        assert lib.moka_set_tracer_biharmonic(None, None) == L.ERR_ARG
        assert lib.moka_set_tracer_biharmonic(sh, one) == L.ERR_ARG          # a state without tracers
        assert lib.moka_set_tracer_biharmonic(sh, None) == 0                  # NULL = all zero: fine anywhere
        assert lib.moka_tracer_biharmonic(sh, 0, C.byref(out)) == L.ERR_ARG
        f = tc.distinct_fields(mesh, K, 3)
        k4 = tb.kappa4s(meshname, 3)
        tr_ = mk.set_tracers(md.Prog, f, biharmonic=k4)
        assert np.array_equal(tr_.biharmonic(), np.asarray(k4)) and np.array_equal(tr_.diffusivity(), np.zeros(3))
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(mk.MokaError, match="finite"):
                tr_.set_biharmonic([k4[0], bad, k4[2]])
            assert np.array_equal(tr_.biharmonic(), np.asarray(k4))           # nothing changed
        with pytest.raises(ValueError):
            tr_.set_biharmonic([1.0, 2.0])
        for j in (-1, 3):
            assert lib.moka_tracer_biharmonic(sh, j, C.byref(out)) == L.ERR_ARG
        assert lib.moka_tracer_biharmonic(sh, 0, None) == L.ERR_ARG
        tr_.set_biharmonic(k4[0])                                             # a scalar: every tracer
        assert np.array_equal(tr_.biharmonic(), np.full(3, k4[0]))
        tr_.set_biharmonic(None)
        assert np.array_equal(tr_.biharmonic(), np.zeros(3))
        tr_.set_biharmonic(k4)
        md.eager(1)                                                           # the scratch is in use
        tr_ = mk.set_tracers(md.Prog, f[:2])                                  # any count resets kappa4 (and frees the scratch)
        assert np.array_equal(tr_.biharmonic(), np.zeros(2))
        md.eager(1)
        assert np.isfinite(tr_.get(0)).all()
        # state and tape destroyed in either order, with kappa4 on
        tr_.set_biharmonic(k4[:2])
        tape = mk.TracerAdjointTape(md.Prog, 1)
        tape.step(md.dt)
        tape.close()
        tape = mk.TracerAdjointTape(md.Prog, 1)
        raw = C.c_void_p()
        L.check(lib.moka_tracer_tape_create(sh, 1, C.byref(raw)), backend._h)
        tape.step(md.dt)
    finally:
        md.close()                                                            # takes `tape` with it; `raw` outlives its state
    lib.moka_tracer_tape_destroy(raw)
    assert not tape._h
