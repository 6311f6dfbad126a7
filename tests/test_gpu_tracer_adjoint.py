"""Reverse mode of passive tracer transport on the device (csrc/tracer_adjoint.hip, moka_tracer_tape_*): gradients bit for bit against
the numpy twin of tests/tracer_adjoint_twin.py, which is driven by the provisional states of the twin's own forward run.

Every case records two RK4 steps of a model whose tracers have pairwise distinct fields and, with diffusion on, pairwise distinct
diffusivities with one exact zero; seeds every tracer with its own random field; and compares every tracer's gradient, the tracers and
the dycore after the taped steps (taping changes no bit), moka_tracer_adjoint_path and moka_state_tracer_path.  The twin computes nine
tracers once per case; a model with n tracers must reproduce the first n (tracers do not interact)."""
import ctypes as C

import numpy as np
import pytest

import moka_hip as mk
import tracer_adjoint_twin as ta
import tracer_cases as tc
import trisk_reference as tr
from moka_hip import lib as L

pytestmark = pytest.mark.gpu
DIFF = pytest.mark.parametrize("diff", [False, True], ids=["plain", "diffused"])
NSTEPS = 2


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)
    yield b
    b.close()


def set_tracers(md, meshname, fields, diff):
    kap = tc.kappas(meshname, 9)[:len(fields)] if diff else None
    return mk.set_tracers(md.Prog, fields, diffusivity=kap)


def tape_and_check(md, meshname, ref, nT, diff, path):
    """nT tracers, NSTEPS taped steps (forward bits against the twin's), seeds, sweep: every gradient equals the twin's."""
    tr_ = set_tracers(md, meshname, ref["fields"][:nT], diff)
    tape = mk.TracerAdjointTape(md.Prog, NSTEPS)
    try:
        assert tape.path() == 0 and tape.steps() == 0
        for s in range(NSTEPS):
            tape.step(md.dt)
            tc.check_tracers(tr_, ref["forward"][s], nT)
            tc.check_dycore(md.Prog, ref["forward"][s])
        assert tape.steps() == NSTEPS and tape.path() == 0
        grad = tape.gradient(ref["X"][:nT])
        assert tape.steps() == 0
        for j in range(nT):
            assert np.array_equal(grad[j], ref["grad"][j]), ("gradient", j, float(np.abs(grad[j] - ref["grad"][j]).max()))
            assert np.any(grad[j] != 0.0)
        assert tape.path() == path and tr_.path() == path
    finally:
        tape.close()


# ---- the generic form ------------------------------------------------------------------------------------------------------------
@DIFF
@pytest.mark.parametrize("nT", [1, 5])
@pytest.mark.parametrize("meshname,K,mode,partial,variant", [("ico16", 4, "linear", False, 0), ("ico12f", 8, "nonlinear", True, 0),
                                                               ("planar", 35, "del2+del4", True, 0), ("planar", 60, "linear", False, 3)])
def test_generic_form(backend, meshname, K, mode, partial, variant, nT, diff):
    """k_tracer_adj_cell: 4 lanes a column (pentagons), 8 lanes with heptagons under the nonlinear dycore and a partial mask, an odd
    K = 35 (64 lanes, no patch form) under Del2 + Del4, and K = 60 under kernel variant 3; one tracer and five, i.e. a second tracer
    group with a tail of one (TRA_TJ = 4)."""
    ref = ta.reference(meshname, K, mode, partial, diff)
    md = tc.Model(backend, meshname, K, mode=mode, partial=partial, variant=variant)
    try:
        tape_and_check(md, meshname, ref, nT, diff, 2)
    finally:
        md.close()


# ---- the patch form --------------------------------------------------------------------------------------------------------------
def second_pass_count(mC, K, diff):
    """The smallest tracer count whose rows the patch form cannot keep resident at once (tc.patch_chunk: the LDS formula restated from
    tracers.hip's comment; the reverse kernel stages the same rows -- ph and one gathered field per resident tracer -- and the same
    records, so tracer_adjoint_kernel is tracer_kernel)."""
    n = 1
    while tc.patch_chunk(mC, K, n, diff) == n:
        n += 1
    return n


@DIFF
@pytest.mark.parametrize("ordering", [L.ORDER_NONE, L.ORDER_RCM], ids=["none", "rcm"])
@pytest.mark.parametrize("patch_cells", [8, 32])
@pytest.mark.parametrize("K", [34, 60, 64])
def test_patch_form(backend, K, patch_cells, ordering, diff):
    """k_tracer_adj_patch on the planar mesh at the smallest, a middle and the largest K of the form, patches of 8 cells (nRec below
    the workgroup size) and 32 (the record tails run), cell orders NONE and RCM; one tracer, three, and -- with 32-cell patches, where
    80 KB hold at most seven tracers' rows -- the smallest count that forces a second pass over the patch."""
    meshname = "planar"
    ref = ta.reference(meshname, K, "linear", False, diff)
    counts, i = [1, 3], 0
    while i < len(counts):                  # a model per count: every run starts from the case's state, as the reference does
        md = tc.Model(backend, meshname, K, ordering=ordering, patch_cells=patch_cells)
        try:
            mC = md.info["maxPatchCells"]
            assert mC == patch_cells
            if i == 0 and patch_cells == 32:
                n2 = second_pass_count(mC, K, diff)
                assert 3 < n2 <= 9 and 1 <= tc.patch_chunk(mC, K, n2, diff) < n2
                counts.append(n2)
            assert tc.patch_chunk(mC, K, counts[i], diff) >= 1
            tape_and_check(md, meshname, ref, counts[i], diff, 1)
        finally:
            md.close()
        i += 1


def test_form_flips_with_diffusion_at_the_lds_boundary(backend):
    """Patches of 70 cells at K = 64: 70 * 1168 = 81 760 bytes <= 80 KB without diffusion (one tracer resident: three passes for three
    tracers, the largest dynamic LDS the kernel is launched with), 70 * 1216 with it: the sweep of a run whose steps were diffused
    takes the generic form, the same model's undiffused run the patch form."""
    meshname, K = "planar", 64
    for diff, path in ((False, 1), (True, 2)):
        md = tc.Model(backend, meshname, K, patch_cells=70)
        try:
            mC = md.info["maxPatchCells"]
            assert 68 <= mC <= 70
            assert tc.patch_chunk(mC, K, 3, False) == 1 and tc.patch_chunk(mC, K, 3, True) == 0
            tape_and_check(md, meshname, ta.reference(meshname, K, "linear", False, diff), 3, diff, path)
        finally:
            md.close()


@pytest.mark.parametrize("nx,ny,K", tc.TINY)
def test_tiny_periodic_meshes(backend, nx, ny, K):
    """The doubly periodic meshes: a cell meets the same neighbour through several slots and one patch holds the whole mesh (every
    gathered row a cache hit); K = 1 and 8 take the generic form.  Three diffused tracers."""
    name = f"tiny-{nx}-{ny}"
    ref = ta.reference(name, K, "linear", False, True)
    md = tc.Model(backend, name, K)
    try:
        tape_and_check(md, name, ref, 3, True, 1 if K % 2 == 0 and 34 <= K <= 64 else 2)
    finally:
        md.close()


# ---- dycore modes and masks --------------------------------------------------------------------------------------------------------
@DIFF
@pytest.mark.parametrize("partial", [False, True], ids=["full", "partial"])
@pytest.mark.parametrize("mode", ["linear", "nonlinear", "del2+del4"])
@pytest.mark.parametrize("K,path", [(6, 2), (34, 1)], ids=["generic", "patch"])
def test_dycore_modes_and_masks(backend, K, path, mode, partial, diff):
    """Each form over the linear, the nonlinear and the Del2 + Del4 dycore, full and partial edge masks, with and without diffusion:
    the recorded provisional states are whatever the dycore formed."""
    meshname = "planar"
    ref = ta.reference(meshname, K, mode, partial, diff)
    md = tc.Model(backend, meshname, K, mode=mode, partial=partial)
    try:
        tape_and_check(md, meshname, ref, 2, diff, path)
    finally:
        md.close()


@pytest.mark.parametrize("mode", ["linear", "nonlinear", "del2+del4"])
def test_taping_changes_no_forward_bit(backend, mode):
    """After taped steps, tracers and dycore equal tc.reference -- the reference of the untaped step -- for the same schedule."""
    meshname, K, nT = "planar", 34, 3
    ref = tc.reference(meshname, K, mode, True, ((3, (nT, 21, False), True),))
    md = tc.Model(backend, meshname, K, mode=mode, partial=True)
    try:
        tr_ = mk.set_tracers(md.Prog, tc.distinct_fields(md.mesh, K, nT), diffusivity=tc.kappas(meshname, nT))
        tape = mk.TracerAdjointTape(md.Prog, 3)
        for s in range(3):
            tape.step(md.dt)
            tc.check_tracers(tr_, ref[s])
            tc.check_dycore(md.Prog, ref[s])
        tape.close()
    finally:
        md.close()


# ---- recording is per step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,path", [(6, 2), (34, 1)], ids=["generic", "patch"])
def test_recording_is_per_step(backend, K, path):
    """The diffusivities change between the two recorded steps and layerThickness is uploaded anew between them: the sweep uses, step
    by step, what each step ran with (the twin's records hold the same)."""
    from del4_twin import TwinState
    meshname, nT = "planar", 3
    mesh = tc.get_mesh(meshname)
    ssh, u, h, _ = tc.state_of(meshname, K)
    h2 = h + np.random.default_rng(12).uniform(-0.5, 0.5, h.shape)
    kap1, kap2 = tc.kappas(meshname, nT), [k * 0.5 for k in reversed(tc.kappas(meshname, nT))]
    f, X = tc.distinct_fields(mesh, K, nT), ta.seeds(mesh, K, nT)
    twin = ta.recording_twin(meshname, K, "nonlinear", True)
    st = TwinState(ssh, u, h)
    phis = [[a.copy() for a in f], [a.copy() for a in f]]
    twin.kappa = kap1
    twin.step_rk4(st, phis, tc.dt_of(meshname))
    twin.kappa = kap2
    st.h[1] = h2.copy()
    twin.step_rk4(st, phis, tc.dt_of(meshname))
    expect = ta.AdjointTwin(twin).sweep(twin.tape, [x.copy() for x in X])
    stale = ta.AdjointTwin(twin).sweep([dict(r, kappa=kap1) for r in twin.tape], [x.copy() for x in X])
    md = tc.Model(backend, meshname, K, mode="nonlinear", partial=True)
    try:
        tr_ = mk.set_tracers(md.Prog, f, diffusivity=kap1)
        tape = mk.TracerAdjointTape(md.Prog, 2)
        tape.step(md.dt)
        tr_.set_diffusivity(kap2)
        md.Prog.layerThickness[-1].set(h2)
        tape.step(md.dt)
        for j in range(nT):
            assert np.array_equal(tr_.get(j), phis[1][j])
        grad = tape.gradient(X)
        for j in range(nT):
            assert np.array_equal(grad[j], expect[j]), j
        assert not np.array_equal(grad[0], stale[0])
        assert tape.path() == path
        tape.close()
    finally:
        md.close()


def test_consequences_on_the_device(backend):
    """A zero seed stays exactly zero beside seeded tracers; the tracer with kappa == 0 beside diffused ones has the bits of a sweep
    whose steps were never diffused (the instances without diffusion)."""
    meshname, K, nT = "planar", 34, 3
    diffused, plain = ta.reference(meshname, K, "linear", False, True), ta.reference(meshname, K, "linear", False, False)
    assert tc.kappas(meshname, 9)[1] == 0.0
    assert np.array_equal(diffused["grad"][1], plain["grad"][1]) and not np.array_equal(diffused["grad"][0], plain["grad"][0])
    md = tc.Model(backend, meshname, K)
    try:
        set_tracers(md, meshname, diffused["fields"][:nT], True)
        tape = mk.TracerAdjointTape(md.Prog, NSTEPS)
        for _ in range(NSTEPS):
            tape.step(md.dt)
        grad = tape.gradient([diffused["X"][0], diffused["X"][1], None])
        assert np.array_equal(grad[2], np.zeros_like(grad[2]))
        assert np.array_equal(grad[1], plain["grad"][1]) and np.array_equal(grad[0], diffused["grad"][0])
        tape.close()
    finally:
        md.close()


# ---- end to end through mk.TracerAdjointTape only ------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K,mode,path", [("ico12f", 5, "nonlinear", 2), ("planar", 34, "del2+del4", 1)])
def test_inner_product_identity_on_the_device(backend, meshname, K, mode, path):
    """<X, forward(d)> = <gradient, d> with both sides from the device: the taped steps carry the tracers d themselves (the map is
    linear), the gradient comes from mk.TracerAdjointTape.  Bound of the CPU test: 2 steps * (100 + 96) * 2^-53 * sum |X| W, W the
    magnitude evaluation of the forward steps on |d| over the twin's records of the same run.  Prints observed / bound."""
    nT = 2
    mesh = tc.get_mesh(meshname)
    ref = ta.reference(meshname, K, mode, True, True)
    rng = np.random.default_rng(41)
    d = [rng.uniform(-1.0, 1.0, (mesh.nCells, K)) for _ in range(nT)]
    X = ref["X"][:nT]
    md = tc.Model(backend, meshname, K, mode=mode, partial=True)
    try:
        tr_ = set_tracers(md, meshname, d, True)
        tape = mk.TracerAdjointTape(md.Prog, NSTEPS)
        for _ in range(NSTEPS):
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
            W = ta.forward_magnitude(mesh, twin.mlt, rec, W, rec["kappa"][j])
        bound = NSTEPS * ta.C_STEP * tr.U53 * (np.abs(X[j]).astype(tr.LD) * W).sum()
        print(f"{meshname} {mode} tracer {j}: |<X, M d> - <M^T X, d>| = {float(abs(lhs - rhs)):.3e}, bound = {float(bound):.3e}, "
              f"<X, M d> = {float(lhs):.6e}")
        assert abs(lhs - rhs) <= bound
        assert abs(lhs) > 1e3 * bound


@pytest.mark.parametrize("kappa", [0.0, tc.EIG_KAPPA], ids=["plain", "diffused"])
@pytest.mark.parametrize("K,path", [(2, 2), (60, 1)])
def test_plane_wave_backwards_on_the_device(backend, K, path, kappa):
    """The plane wave of tracer_cases.py backwards: seed X = phi0, EIG_STEPS recorded steps, the gradient is
    1 + 0.5 Re(conj(R4(z))^n e^{i k . x}) within n * 32 * 2^-53 * max|phi0|; the bound refuses the forward factor, a third-order
    reverse loop and the exponential (ta.plane_wave_check).  Nothing in the expectation shares code with the twins or the kernels."""
    mesh, state, phi0 = tc.eigenmode_state(K)
    md = tc.Model(backend, "planar-f0", K, state=state)
    try:
        mk.set_tracers(md.Prog, [phi0], diffusivity=[kappa] if kappa else None)
        tape = mk.TracerAdjointTape(md.Prog, tc.EIG_STEPS)
        for _ in range(tc.EIG_STEPS):
            tape.step(tc.EIG_DT)
        grad = tape.gradient([phi0])[0]
        assert tape.path() == path
        ta.plane_wave_check(grad, mesh, K, kappa, phi0, f"device, K = {K}, kappa = {kappa:g}")
        tape.close()
    finally:
        md.close()


# ---- lifecycle ---------------------------------------------------------------------------------------------------------------------
def test_lifecycle_and_refusals(backend):
    meshname, K = "planar", 6
    mesh = tc.get_mesh(meshname)
    md = tc.Model(backend, meshname, K)
    lib, sh, ctx = L.lib(), md.Prog._state._h, backend._h
    try:
        with pytest.raises(mk.MokaError, match="tracers"):          # a tracer-free state
            mk.TracerAdjointTape(md.Prog, 1)
        h = C.c_void_p()
        assert lib.moka_tracer_tape_create(None, 1, C.byref(h)) == L.ERR_ARG
        assert lib.moka_tracer_tape_create(sh, 1, None) == L.ERR_ARG
        f = tc.distinct_fields(mesh, K, 2)
        tr_ = mk.set_tracers(md.Prog, f)
        assert lib.moka_tracer_tape_create(sh, -1, C.byref(h)) == L.ERR_ARG
        tape = mk.TracerAdjointTape(md.Prog, 1)
        with pytest.raises(mk.MokaError):                            # unseeded
            tape.sweep()
        tape.step(md.dt)
        with pytest.raises(mk.MokaError, match="full"):
            tape.step(md.dt)
        with pytest.raises(mk.MokaError):                            # a recorded step un-seeds; still unseeded
            tape.sweep()
        for j in (-1, 2):
            with pytest.raises(mk.MokaError, match="range"):
                tape.seed(j, f[0])
            with pytest.raises(mk.MokaError, match="range"):
                tape.download(j)
        with pytest.raises(mk.MokaError):                            # a tape of the state: its arrays stay where they are
            mk.set_tracers(md.Prog, [f[0]])
        with pytest.raises(mk.MokaError):
            md.Prog._state.optimize_placement(1)
        assert np.array_equal(tr_.get(0, 0), f[0])                   # the refused calls changed nothing
        # the tape is reusable after a sweep: the second round equals the first
        X = ta.seeds(mesh, K, 2)
        g1 = tape.gradient(X)
        assert tape.steps() == 0 and tape.path() == 2
        tr_.set(0, f[0]); tr_.set(1, f[1])
        md.Prog.normalVelocity[-1].set(md.u); md.Prog.layerThickness[-1].set(md.h); md.Prog.ssh[-1].set(md.ssh)
        tape.step(md.dt)
        with pytest.raises(mk.MokaError):                            # the recorded step un-seeded the tape
            tape.sweep()
        g2 = tape.gradient(X)
        assert all(np.array_equal(a, b) for a, b in zip(g1, g2)) and np.any(g1[0] != 0.0)
        # the first seed after a recorded step zeroes the other tracers' adjoints
        tape.step(md.dt)
        tape.seed(1, X[1])
        assert np.array_equal(tape.download(0), np.zeros_like(X[0])) and np.array_equal(tape.download(1), X[1])
        tape.seed(0, X[0])
        assert np.array_equal(tape.download(1), X[1])
        tape.sweep()
        tape.close()
        tape.close()                                                 # idempotent
        tr_ = mk.set_tracers(md.Prog, [f[0]])                        # accepted once the tape is gone
        # the tracer count changed under a live tape cannot happen (set_tracers refuses); a state closed before its tape: no crash
        tape = mk.TracerAdjointTape(md.Prog, 1)
        raw = C.c_void_p()
        L.check(lib.moka_tracer_tape_create(sh, 1, C.byref(raw)), ctx)
        tape.step(md.dt)
    finally:
        md.close()                                                   # takes `tape` with it, in order; `raw` outlives its state
    lib.moka_tracer_tape_destroy(raw)
    assert not tape._h
