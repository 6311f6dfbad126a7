"""Tracer sources and the gradient with respect to them on the device (csrc/tracers.hip SRC, csrc/tracer_adjoint.hip SG,
moka_tracer_source_*, moka_tracer_adjoint_want_source_gradient): bit for bit against the numpy twins of tests/tracer_source_twin.py.

A case records two RK4 steps of a model whose tracers have pairwise distinct fields, sources on a subset of them and, with diffusion
on, pairwise distinct diffusivities with one exact zero; compares both time levels of every tracer and the dycore after each step; asks
for the source gradient of a strict subset; seeds every tracer with its own field; and compares every X and every wanted G, the kernel
paths and the premise that makes the case the shape it claims to be (Tracers.path(), tc.patch_chunk, Mesh.info()).  The twin's
schedule is computed once per case (ts.reference) and shared."""
import ctypes as C

import numpy as np
import pytest

import moka_hip as mk
import tracer_adjoint_twin as ta
import tracer_cases as tc
import tracer_source_twin as ts
import trisk_reference as tr
from moka_hip import lib as L

pytestmark = pytest.mark.gpu
NSTEPS = 2


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)
    yield b
    b.close()


def set_tracers(md, meshname, ref, diff):
    nT = len(ref["fields"])
    tr_ = mk.set_tracers(md.Prog, ref["fields"], diffusivity=tc.kappas(meshname, 9)[:nT] if diff else None, sources=ref["sources"])
    for j, q in enumerate(ref["sources"]):
        assert tr_.has_source(j) == (q is not None)
        assert np.array_equal(tr_.source(j), q if q is not None else np.zeros(tr_.shape))
    return tr_


def tape_and_check(md, meshname, ref, wants, diff, path):
    """Taped steps (forward bits against the twin's), the gradients wanted on `wants`, seeds, sweep: every X and every wanted G equal
    the twin's; a tracer that was never flagged has no G to download."""
    nT = len(ref["fields"])
    assert 0 < len(wants) < nT
    tr_ = set_tracers(md, meshname, ref, diff)
    tape = mk.TracerAdjointTape(md.Prog, NSTEPS)
    try:
        for j in wants:
            tape.want_source_gradient(j)
        for s in range(NSTEPS):
            tape.step(md.dt)
            tc.check_tracers(tr_, ref["forward"][s])
            tc.check_dycore(md.Prog, ref["forward"][s])
        grad = tape.gradient(ref["X"])
        for j in range(nT):
            assert np.array_equal(grad[j], ref["grad"][j]), ("X", j, float(np.abs(grad[j] - ref["grad"][j]).max()))
            if j in wants:
                G = tape.source_gradient(j)
                assert np.array_equal(G, ref["G"][j]), ("G", j, float(np.abs(G - ref["G"][j]).max()))
                assert np.any(G != 0.0)
            else:
                with pytest.raises(mk.MokaError):
                    tape.source_gradient(j)
        assert tape.path() == path and tr_.path() == path
    finally:
        tape.close()


def case(backend, meshname, K, nT, srcs, wants, diff, path, mode="linear", partial=False, guard=None, **kw):
    ref = ts.reference(meshname, K, mode, partial, diff, nT, srcs, wants)
    md = tc.Model(backend, meshname, K, mode=mode, partial=partial, **kw)
    try:
        if guard:
            guard(md)
        tape_and_check(md, meshname, ref, wants, diff, path)
    finally:
        md.close()


# ---- the generic form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K,variant,lpc", [("planar", 8, 3, 8), ("planar", 33, 0, 64), ("planar", 1, 0, 1), ("ico12f", 8, 0, 8)])
def test_generic_form(backend, meshname, K, variant, lpc):
    """k_tracer_cell<.., SRC> and k_tracer_adj_cell<.., SG>: six tracers -- two TR_TJ groups -- with sources on {1, 4} and gradients
    wanted on {1, 5}, so the pointer tables are read across the group boundary and a sourced tracer without a gradient, an unsourced
    one with a gradient and tracers with neither sit side by side; K = 8 under kernel variant 3, the odd K = 33 (64 lanes, no patch
    form), K = 1 (one lane a column) and heptagons."""
    def guard(md):
        assert md.info["lanesPerColumn"] == lpc
    case(backend, meshname, K, 6, (1, 4), (1, 5), True, 2, variant=variant, guard=guard)


# ---- the patch form --------------------------------------------------------------------------------------------------------------
def test_patch_form_all_resident(backend):
    """k_tracer_patch<6, .., SRC> / k_tracer_adj_patch<6, .., SG> on ico16 at K = 34: three tracers, all resident (one pass), sources
    on {0, 2}, gradients on {0, 1}."""
    def guard(md):
        assert tc.patch_chunk(md.info["maxPatchCells"], 34, 3, True) == 3
    case(backend, "ico16", 34, 3, (0, 2), (0, 1), True, 1, guard=guard)


def test_patch_form_second_pass(backend):
    """ico16 at K = 64 with nine tracers: 80 KB hold eight tracers' rows, so the ninth takes a second pass over the patch.  Sources on
    the last tracer of the first pass and the first of the second (7, 8), gradients on (0, 7, 8): j0 + jj indexes the tables in both
    passes."""
    def guard(md):
        chunk = tc.patch_chunk(md.info["maxPatchCells"], 64, 9, False)
        assert chunk == 8
    case(backend, "ico16", 64, 9, (7, 8), (0, 7, 8), False, 1, guard=guard)


@pytest.mark.parametrize("patch_cells", [12, 48])
def test_patch_form_patch_sizes(backend, patch_cells):
    """Patches of 12 cells (records below the workgroup size) and 48 (the record tails run; at K = 64 two plain tracers' rows are
    resident, so three tracers take two passes): orow of the source and gradient rows follows the patch's own cell range."""
    def guard(md):
        assert md.info["maxPatchCells"] == patch_cells
        assert tc.patch_chunk(patch_cells, 64, 3, False) == (3 if patch_cells == 12 else 2)
    case(backend, "planar", 64, 3, (1, 2), (0, 2), False, 1, patch_cells=patch_cells, guard=guard)


# ---- DIFF x SRC / SG ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", [False, True], ids=["nosrc", "src"])
@pytest.mark.parametrize("diff", [False, True], ids=["plain", "diffused"])
@pytest.mark.parametrize("K,path", [(6, 2), (34, 1)], ids=["generic", "patch"])
def test_diffusion_times_sources(backend, K, path, diff, src):
    """All four instantiations of both forms, forwards (DIFF x SRC) and backwards (DIFF x SG on; SG off is every older test):
    tc.kappas has one exact zero among the first two, and without sources the forward launches are those of a source-free state while
    the gradient is still wanted (G does not need a source to exist)."""
    case(backend, "planar", K, 3, (0, 2) if src else (), (1, 2), diff, path)


# ---- dycores and masks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,partial", [("nonlinear", False), ("del2+del4", False), ("linear", True), ("nonlinear", True)])
@pytest.mark.parametrize("K,path", [(6, 2), (34, 1)], ids=["generic", "patch"])
def test_dycores_and_masks(backend, K, path, mode, partial):
    """The nonlinear and the Del2 + Del4 dycore and the partial edge mask: the source is added behind a slot loop that skipped slots
    (a cell whose every slot is masked has T == q exactly), and the flow never sees it."""
    case(backend, "planar", K, 3, (0, 1), (0, 2), True, path, mode=mode, partial=partial)


# ---- cell orders, tiny meshes, the captured graph ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ordering", [L.ORDER_NONE, L.ORDER_RCM], ids=["none", "rcm"])
@pytest.mark.parametrize("meshname,K,path", [("ico16", 34, 1), ("ico12f", 5, 2)])
def test_other_cell_orders(backend, meshname, K, path, ordering):
    """Sources are given and gradients returned in the caller's numbering whatever the plan's cell order (set_tracers' round trip of
    every source through put_rows / get_rows is part of every case)."""
    mesh = tc.get_mesh(meshname)

    def guard(md):
        perm = np.empty(mesh.nCells, dtype=np.int32)
        L.check(L.lib().moka_mesh_permutation(md.M._h, L.CELL, L.i32(perm)))
        assert not np.array_equal(perm, L.Plan(mesh, K, max_level_edge_top=K).permutation(L.CELL))
    case(backend, meshname, K, 3, (0, 2), (1, 2), True, path, ordering=ordering, guard=guard)


@pytest.mark.parametrize("nx,ny,K", [(4, 2, 8), (4, 6, 1)])
def test_tiny_periodic_meshes(backend, nx, ny, K):
    """The smallest doubly periodic meshes (one patch holds the mesh; a cell meets a neighbour through several slots)."""
    case(backend, f"tiny-{nx}-{ny}", K, 3, (0, 1), (1, 2), True, 2)


@pytest.mark.parametrize("meshname,K,path", [("ico12f", 5, 2), ("planar", 34, 1)])
def test_eager_steps_and_the_captured_graph(backend, meshname, K, path):
    """moka_step_rk4 and mk.run_steps (from 6 steps on one eager step, then the replay of a captured graph, whose launches carry the
    source table by value): both time levels after step 1 and after step 7 against the twin."""
    nT, srcs, n = 3, (0, 2), 7
    ref = ts.reference(meshname, K, "linear", False, True, nT, srcs, (0,), nsteps=n)
    md = tc.Model(backend, meshname, K)
    try:
        tr_ = set_tracers(md, meshname, ref, True)
        md.eager(1)
        tc.check_tracers(tr_, ref["forward"][0])
        md.run(n - 1)
        tc.check_tracers(tr_, ref["forward"][n - 1])
        tc.check_dycore(md.Prog, ref["forward"][n - 1])
        assert tr_.path() == path
    finally:
        md.close()


# ---- life cycle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,path", [(6, 2), (34, 1)], ids=["generic", "patch"])
def test_source_life_cycle(backend, K, path):
    """A source set after two steps, replaced, removed (None), and the state back on the source-free bits: the twin follows the same
    schedule.  Zero sources of both signs and an unsourced tracer beside sourced ones keep the bits of the source-free reference;
    set_tracers drops the sources."""
    from del4_twin import TwinState
    meshname, nT = "planar", 3
    mesh = tc.get_mesh(meshname)
    f, q = tc.distinct_fields(mesh, K, nT), ts.source_fields(meshname, K, 4)
    plain = tc.reference(meshname, K, "linear", False, ((2, (nT, 21, False), True),))
    twin = ts.source_twin(meshname, K)
    twin.kappa = tc.kappas(meshname, nT)
    ssh, u, h, _ = tc.state_of(meshname, K)
    st = TwinState(ssh, u, h)
    phis = [[a.copy() for a in f], [a.copy() for a in f]]
    sched = ([], [None, q[1], None], [q[0], q[3], None], [q[0], None, None], [])
    expect = []
    for src in sched:
        twin.source = src
        for _ in range(2):
            twin.step_rk4(st, phis, tc.dt_of(meshname))
        expect.append(([a.copy() for a in phis[0]], [a.copy() for a in phis[1]]))
    md = tc.Model(backend, meshname, K)
    try:
        tr_ = mk.set_tracers(md.Prog, f, diffusivity=tc.kappas(meshname, nT))
        # zero sources of both signs beside an unsourced tracer: the source-free bits
        tr_.set_source(0, np.zeros(tr_.shape)); tr_.set_source(2, -np.zeros(tr_.shape))
        assert tr_.has_source(0) and not tr_.has_source(1) and tr_.has_source(2)
        md.eager(2)
        tc.check_tracers(tr_, plain[1])
        assert np.array_equal(tr_.get(1), expect[0][1][1])
        tr_.set_source(0, None); tr_.set_source(2, None)
        have = [False] * nT
        for seg, src in enumerate(sched[1:], start=1):
            for j in range(nT):
                qj = src[j] if j < len(src) else None
                if qj is not None or have[j]:
                    tr_.set_source(j, qj)
                have[j] = qj is not None
                assert tr_.has_source(j) == have[j]
            md.eager(1); md.run(1)
            tc.check_tracers(tr_, expect[seg])
            assert tr_.path() == path
        assert not np.array_equal(expect[1][1][1], plain[1][1])
        # set_tracers drops every source, as it resets the diffusivities
        tr_.set_source(1, q[1])
        tr_ = mk.set_tracers(md.Prog, f)
        assert not any(tr_.has_source(j) for j in range(nT)) and np.array_equal(tr_.source(1), np.zeros(tr_.shape))
        tr_.set_diffusivity(tc.kappas(meshname, nT))
        md.Prog.normalVelocity[-1].set(md.u); md.Prog.layerThickness[-1].set(md.h); md.Prog.ssh[-1].set(md.ssh)
        md.eager(2)
        tc.check_tracers(tr_, plain[1])
    finally:
        md.close()


def test_error_codes(backend):
    meshname, K, nT = "planar", 6, 2
    mesh = tc.get_mesh(meshname)
    md = tc.Model(backend, meshname, K)
    lib, sh = L.lib(), md.Prog._state._h
    try:
        q = ts.source_fields(meshname, K, 1)[0]
        buf, flag = np.empty_like(q), C.c_int(7)
        assert lib.moka_tracer_source_upload(sh, 0, L.f64(q)) == L.ERR_ARG            # no tracers: every j is out of range
        f = tc.distinct_fields(mesh, K, nT)
        tr_ = mk.set_tracers(md.Prog, f)
        for j in (-1, nT):
            assert lib.moka_tracer_source_upload(sh, j, L.f64(q)) == L.ERR_ARG
            assert lib.moka_tracer_source_download(sh, j, L.f64(buf)) == L.ERR_ARG
            assert lib.moka_tracer_has_source(sh, j, C.byref(flag)) == L.ERR_ARG
        assert lib.moka_tracer_source_upload(None, 0, L.f64(q)) == L.ERR_ARG
        assert lib.moka_tracer_source_download(sh, 0, None) == L.ERR_ARG
        assert lib.moka_tracer_has_source(sh, 0, None) == L.ERR_ARG
        tr_.set_source(0, q)
        for bad in (np.nan, np.inf, -np.inf):                                         # refused, nothing changed
            qb = q.copy(); qb[3, 2] = bad
            assert lib.moka_tracer_source_upload(sh, 0, L.f64(qb)) == L.ERR_ARG
            assert lib.moka_tracer_source_upload(sh, 1, L.f64(qb)) == L.ERR_ARG
            assert np.array_equal(tr_.source(0), q) and not tr_.has_source(1)
        tr_.set_source(1, None)                                                        # removing what is not there: fine
        tape = mk.TracerAdjointTape(md.Prog, 2)
        th = tape._h
        for j in (-1, nT):
            assert lib.moka_tracer_adjoint_want_source_gradient(th, j, 1) == L.ERR_ARG
            assert lib.moka_tracer_adjoint_source_download(th, j, L.f64(buf)) == L.ERR_ARG
        assert lib.moka_tracer_adjoint_want_source_gradient(None, 0, 1) == L.ERR_ARG
        assert lib.moka_tracer_adjoint_source_download(th, 0, L.f64(buf)) == L.ERR_ARG   # never flagged
        tape.want_source_gradient(0)
        assert lib.moka_tracer_adjoint_source_download(th, 0, None) == L.ERR_ARG
        assert np.array_equal(tape.source_gradient(0), np.zeros_like(q))
        tape.step(md.dt)
        tape.want_source_gradient(1); tape.want_source_gradient(1, False)              # unseeded: allowed, also after a step
        X = ta.seeds(mesh, K, nT)
        tape.seed(0, X[0])
        with pytest.raises(mk.MokaError, match="sweep"):                               # between a seed and its sweep
            tape.want_source_gradient(1)
        tape.sweep()
        tape.want_source_gradient(1)                                                   # after the sweep: allowed again
        assert np.any(tape.source_gradient(0) != 0.0) and np.array_equal(tape.source_gradient(1), np.zeros_like(q))
        # the older refusals stand with sources set
        with pytest.raises(mk.MokaError):
            L.check(lib.moka_step_fe(sh, md.dt, 3), backend._h)
        with pytest.raises(mk.MokaError):
            mk.AdjointTape(md.Prog, 1)
        tape.close()
    finally:
        md.close()


# ---- reverse: what the header promises ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,path", [(6, 2), (34, 1)], ids=["generic", "patch"])
def test_reverse_consequences_on_the_device(backend, K, path):
    """On one model, four rounds of two taped steps from the same state: (a) sources q, gradients wanted; (b) other sources, wanted;
    (c) no sources, nothing wanted; (d) wanted again, every seed zero.  X is the same bit for bit in (a), (b), (c) -- asking for G
    changes no bit of X, and neither depends on q; G is the same in (a) and (b); the first seed after a recorded step zeroes G (round
    (b) does not start from (a)'s sums, (c) leaves zeros, and (d) ends with G == 0 exactly)."""
    meshname, nT, wants = "planar", 3, (0, 2)
    ref = ts.reference(meshname, K, "linear", False, True, nT, (0, 1), wants)
    q2 = [None, 3.0 * ref["sources"][0], ref["sources"][1]]
    md = tc.Model(backend, meshname, K)
    try:
        tr_ = set_tracers(md, meshname, ref, True)
        tape = mk.TracerAdjointTape(md.Prog, NSTEPS)
        rounds = []
        for rnd, (src, want, seeds) in enumerate(((ref["sources"], True, ref["X"]), (q2, True, ref["X"]), ([None] * nT, False, ref["X"]),
                                                  (ref["sources"], True, [None] * nT))):
            for j in range(nT):
                tr_.set(j, ref["fields"][j]); tr_.set(j, ref["fields"][j], 0)
                tr_.set_source(j, src[j])
            md.Prog.normalVelocity[-1].set(md.u); md.Prog.layerThickness[-1].set(md.h); md.Prog.ssh[-1].set(md.ssh)
            for j in wants:
                tape.want_source_gradient(j, want)
            for _ in range(NSTEPS):
                tape.step(md.dt)
            if rnd == 1:                         # the sums of round (a) are still there until the first seed
                assert np.array_equal(tape.source_gradient(0), ref["G"][0])
            grad = tape.gradient(seeds)
            rounds.append((grad, [tape.source_gradient(j) for j in wants]))
            assert tape.path() == path
        for j in range(nT):
            assert np.array_equal(rounds[0][0][j], ref["grad"][j])
            assert np.array_equal(rounds[1][0][j], rounds[0][0][j]) and np.array_equal(rounds[2][0][j], rounds[0][0][j])
            assert np.array_equal(rounds[3][0][j], np.zeros_like(ref["X"][j]))
        for i, j in enumerate(wants):
            assert np.array_equal(rounds[0][1][i], ref["G"][j]) and np.array_equal(rounds[1][1][i], ref["G"][j])
            assert np.array_equal(rounds[2][1][i], np.zeros_like(ref["X"][j]))      # (c) wanted nothing: its seed zeroed G, its sweep left it
            assert np.array_equal(rounds[3][1][i], np.zeros_like(ref["X"][j]))
        tape.close()
    finally:
        md.close()


@pytest.mark.parametrize("K,path", [(6, 2), (34, 1)], ids=["generic", "patch"])
def test_recording_is_per_step(backend, K, path):
    """The diffusivities change between the two recorded steps while the sources stay: X and G use, step by step, what each step ran
    with (a sweep over records with the first step's diffusivities throughout gives another G)."""
    from del4_twin import TwinState
    meshname, nT, wants = "planar", 3, (0, 1)
    mesh = tc.get_mesh(meshname)
    f, X, q = tc.distinct_fields(mesh, K, nT), ta.seeds(mesh, K, nT), ts.source_fields(meshname, K, nT)
    kap1, kap2 = tc.kappas(meshname, nT), [k * 0.5 for k in reversed(tc.kappas(meshname, nT))]
    twin = ts.source_twin(meshname, K, "nonlinear", True)
    twin.source = [q[0], None, q[2]]
    ssh, u, h, _ = tc.state_of(meshname, K)
    st = TwinState(ssh, u, h)
    phis = [[a.copy() for a in f], [a.copy() for a in f]]
    for kap in (kap1, kap2):
        twin.kappa = kap
        twin.step_rk4(st, phis, tc.dt_of(meshname))
    adj = ts.SourceAdjointTwin(twin)
    expect, G = adj.sweep(twin.tape, [x.copy() for x in X], wants)
    _, stale = adj.sweep([dict(r, kappa=kap1) for r in twin.tape], [x.copy() for x in X], wants)
    md = tc.Model(backend, meshname, K, mode="nonlinear", partial=True)
    try:
        tr_ = mk.set_tracers(md.Prog, f, diffusivity=kap1, sources=twin.source)
        tape = mk.TracerAdjointTape(md.Prog, 2)
        for j in wants:
            tape.want_source_gradient(j)
        tape.step(md.dt)
        tr_.set_diffusivity(kap2)
        tape.step(md.dt)
        for j in range(nT):
            assert np.array_equal(tr_.get(j), phis[1][j])
        grad = tape.gradient(X)
        for j in range(nT):
            assert np.array_equal(grad[j], expect[j]), j
        for j in wants:
            assert np.array_equal(tape.source_gradient(j), G[j]), j
        assert not np.array_equal(G[0], stale[0])
        assert tape.path() == path
        tape.close()
    finally:
        md.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K,mode,path", [("ico12f", 5, "nonlinear", 2), ("planar", 34, "del2+del4", 1)])
def test_step_identity_on_the_device(backend, meshname, K, mode, path):
    """<X, phi_N(phi_0, q) - phi_N(phi_0, 0)> = <G, q> with every term from the device: two taped steps with sources, the sweep with
    the gradients wanted, then the same two steps from the same state without sources.  Bound of the CPU test:
    2 steps * C_STEP_SRC * 2^-53 * sum |X| W, W over the twin's records of the same run.  Prints observed / bound."""
    nT = 2
    mesh = tc.get_mesh(meshname)
    ref = ts.reference(meshname, K, mode, True, True, nT, (0, 1), (0,))
    f, X = ref["fields"], ref["X"]
    q = [20.0 * a for a in ref["sources"]]
    md = tc.Model(backend, meshname, K, mode=mode, partial=True)
    try:
        tr_ = mk.set_tracers(md.Prog, f, diffusivity=tc.kappas(meshname, 9)[:nT], sources=q)
        tape = mk.TracerAdjointTape(md.Prog, NSTEPS)
        for _ in range(NSTEPS):
            tape.step(md.dt)
        with_q = [tr_.get(j) for j in range(nT)]
        _, G = tape.gradient(X, sources=True)
        assert tape.path() == path
        for j in range(nT):
            tr_.set(j, f[j]); tr_.set(j, f[j], 0)
            tr_.set_source(j, None)
        md.Prog.normalVelocity[-1].set(md.u); md.Prog.layerThickness[-1].set(md.h); md.Prog.ssh[-1].set(md.ssh)
        md.eager(NSTEPS)
        without = [tr_.get(j) for j in range(nT)]
        tape.close()
    finally:
        md.close()
    twin = ref["twin"]
    for j in range(nT):
        assert np.array_equal(without[j], tc.reference(meshname, K, mode, True, ((NSTEPS, (nT, 21, False), True),))[-1][1][j])
        lhs = (X[j].astype(tr.LD) * (with_q[j].astype(tr.LD) - without[j].astype(tr.LD))).sum()
        rhs = ta.dot_ld(G[j], q[j])
        W = np.abs(f[j]).astype(tr.LD)
        for rec in twin.tape:
            W = ts.forward_magnitude(mesh, twin.mlt, rec, W, rec["kappa"][j], np.abs(q[j]))
        bound = NSTEPS * ts.C_STEP_SRC * tr.U53 * (np.abs(X[j]).astype(tr.LD) * W).sum()
        print(f"{meshname} {mode} tracer {j}: |<X, dphi_N> - <G, q>| = {float(abs(lhs - rhs)):.3e}, bound = {float(bound):.3e}, "
              f"<G, q> = {float(rhs):.6e}")
        assert abs(lhs - rhs) <= bound
        assert abs(rhs) > 1e3 * bound


@pytest.mark.parametrize("kappa", [0.0, tc.EIG_KAPPA], ids=["plain", "diffused"])
@pytest.mark.parametrize("K,path", [(2, 2), (60, 1)])
def test_forced_plane_wave_on_the_device(backend, K, path, kappa):
    """The forced plane wave of tests/tracer_source_twin.py on the device, forwards and backwards: EIG_STEPS taped steps of
    phi0 = 1 + 0.5 cos(k . x) with q = h sigma cos(k . x), then the sweep of the seed phi0 with the source gradient wanted; the CPU
    tests' bounds (ts.forced_wave_check, ts.forced_wave_gradient_check).  Nothing in the expectations shares code with the twins or
    the kernels."""
    mesh, state, phi0 = tc.eigenmode_state(K)
    md = tc.Model(backend, "planar-f0", K, state=state)
    try:
        tr_ = mk.set_tracers(md.Prog, [phi0], diffusivity=[kappa] if kappa else None, sources=[ts.eigen_source(mesh, K)])
        tape = mk.TracerAdjointTape(md.Prog, tc.EIG_STEPS)
        for _ in range(tc.EIG_STEPS):
            tape.step(tc.EIG_DT)
        ts.forced_wave_check(tr_.get(0), mesh, K, kappa, phi0, f"device, K = {K}, kappa = {kappa:g}")
        _, G = tape.gradient([phi0], sources=True)
        assert tape.path() == path and tr_.path() == path
        ts.forced_wave_gradient_check(G[0], mesh, K, kappa, phi0, f"device gradient, K = {K}, kappa = {kappa:g}")
        tape.close()
    finally:
        md.close()
