"""The launch shapes of the tracer kernels (csrc/tracers.hip) that test_gpu_tracers.py and test_gpu_tracer_diffusion.py leave out, bit for
bit against the numpy twins, and the one check of the HIP tracer path against something that shares no code with it: an exact
plane-wave mode of RK4.  Cases, twins' schedules and the device model: tests/tracer_cases.py.

Every case gives its tracers pairwise distinct fields and, with diffusion on, pairwise distinct diffusivities with one exact zero
(a tracer taken for its neighbour three or four places on cannot pass), compares both time levels of every tracer after an eager
step and after mk.run_steps, and asserts Tracers.path() plus whatever else proves that the lines named below ran:

  k_tracer_cell's j0 loop, j0 > 0: second and third tracer group, partial tail, (j0 + jj) * stride       test_generic_form_tracer_groups
  k_tracer_cell<2>, <16>, <32>; K = 33 (64 lanes, generic); K = 130 (three levels a lane of its k loop)  test_generic_form_lane_widths
  the tail loops of tracer_stage_records (tracer_patch.hpp) after the register-staged records, the LDS
      carve of tracer_patch_open for maxOwnC != 16, k_tracer_patch's pass loop with chunk == 1 and 2
      and three tracers                                                                                  test_patch_form_patch_sizes
  tracer_kernel at its 80 KB boundary, both ways                                                         test_form_flips_with_diffusion_at_the_lds_boundary,
                                                                                                         test_patches_too_large_for_the_patch_form
  moka_tracer_upload / _download through put_rows / get_rows in other cell orders                        test_tracers_in_other_cell_orders
  every ch[i] of tracer_slots a cache hit (tracer_gather takes no masked load), one neighbour through
      several slots                                                                                      test_tiny_periodic_meshes
  moka_set_tracers on a state that has stepped; 3 -> 9 -> 1 tracers (api.hip)                            test_late_and_changing_tracers
  the stage weights, on the device                                                                       test_plane_wave_on_the_device

Left alone: the invArea tail loop of tracer_stage_records needs more than 256 cells in a patch, and 257 * (16 * 34 + 144) bytes are above the 80 KB
the patch form may take, so no mesh reaches it."""
import numpy as np
import pytest

import moka_hip as mk
import tracer_cases as tc
from moka_hip import lib as L

pytestmark = pytest.mark.gpu
DIFF = pytest.mark.parametrize("diff", [False, True], ids=["plain", "diffused"])


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)
    yield b
    b.close()


def set_tracers(md, meshname, fields, diff, of=None):
    """The first len(fields) of `of` (default: as many) distinct diffusivities with them when diff."""
    kap = tc.kappas(meshname, of or len(fields))[:len(fields)] if diff else None
    return mk.set_tracers(md.Prog, fields, diffusivity=kap)


def step_and_check(md, tr, ref, nsteps, n=None, first=0):
    """One eager step, the rest through mk.run_steps (from 6 steps on: one more eager, then graph replay); tracers and dycore
    against steps first + 1 and first + nsteps of `ref`."""
    md.eager(1)
    tc.check_tracers(tr, ref[first], n)
    tc.check_dycore(md.Prog, ref[first])
    if nsteps > 1:
        md.run(nsteps - 1)
        tc.check_tracers(tr, ref[first + nsteps - 1], n)
        tc.check_dycore(md.Prog, ref[first + nsteps - 1])


# ---- the generic form ------------------------------------------------------------------------------------------------------------
@DIFF
@pytest.mark.parametrize("nT", [5, 8, 9])
@pytest.mark.parametrize("meshname,K,partial,variant,nsteps", [("ico12f", 5, False, 0, 7), ("ico16", 66, False, 0, 3),
                                                                 ("ico16", 60, True, 3, 3)])
def test_generic_form_tracer_groups(backend, meshname, K, partial, variant, nsteps, nT, diff):
    """More tracers than the TR_TJ = 4 a lane of k_tracer_cell carries at once: the j0 loop of k_tracer_cell takes a second group
    (nT = 5: a tail of one; 8: a full one) and a third (9: a tail of one behind two full groups), so `(j0 + jj) * stride` addresses
    rows beyond the first group and `jj < nj` masks a tail with j0 > 0 -- with and without DIFF, with 8 (heptagons), 64 lanes and
    with a partial edge mask under variant 3.  Nine distinct fields and diffusivities; the twin of the nine serves every nT.  The
    two large shapes take 3 steps (their twin costs seconds per step), the small one 7 with graph replay."""
    ref = tc.reference(meshname, K, "linear", partial, ((nsteps, (9, 21, False), diff),))
    md = tc.Model(backend, meshname, K, partial=partial, variant=variant)
    try:
        tr = set_tracers(md, meshname, tc.distinct_fields(md.mesh, K, 9)[:nT], diff, of=9)
        assert tr.path() == 0
        step_and_check(md, tr, ref, nsteps, n=nT)
        assert tr.path() == 2
    finally:
        md.close()


@DIFF
@pytest.mark.parametrize("meshname,K,lpc,partial", [("ico16", 2, 2, False), ("planar", 12, 16, True), ("ico16", 17, 32, False),
                                                     ("planar", 32, 32, False), ("planar", 33, 64, False), ("planar", 130, 64, False)])
def test_generic_form_lane_widths(backend, meshname, K, lpc, partial, diff):
    """The instantiations of k_tracer_cell no other test launches: 2, 16 and 32 lanes per column (NG = 128, 16, 8 cells a block;
    K = 12 and 17 leave lanes of the group idle, K = 32 none), K = 33 -- the first K with 64 lanes, odd and below 34, so the generic
    form although lpc == 64 -- and K = 130, where the level loop's `k += LPC` gives a lane a third level.  Five tracers (two groups), one
    case with the partial edge mask; 7 steps."""
    ref = tc.reference(meshname, K, "linear", partial, ((7, (5, 21, False), diff),))
    md = tc.Model(backend, meshname, K, partial=partial)
    try:
        assert md.info["lanesPerColumn"] == lpc
        tr = set_tracers(md, meshname, tc.distinct_fields(md.mesh, K, 5), diff)
        step_and_check(md, tr, ref, 7)
        assert tr.path() == 2
    finally:
        md.close()


# ---- the patch form --------------------------------------------------------------------------------------------------------------
@DIFF
@pytest.mark.parametrize("partial,mode", [(False, "linear"), (True, "del2+del4")], ids=["full-linear", "partial-del2+del4"])
@pytest.mark.parametrize("patch_cells", [12, 24, 48])
@pytest.mark.parametrize("meshname,K", [("planar", 64), ("ico16", 60)])
def test_patch_form_patch_sizes(backend, meshname, K, patch_cells, partial, mode, diff):
    """k_tracer_patch with patches of 12, 24 and 48 cells instead of the default 16, where nRec = 256 = TR_NT exactly and every tail
    loop behind the register-staged record phase is empty.  24 cells: nRec = 384, the cRec tail loop of tracer_stage_records runs; 48 cells: nSd = 288,
    its sdv / maxLevelEdgeTop and dvdc tail loops run too; 12 cells: nRec < TR_NT, the guards `tid < nRec` cut.  the sd, dd, ia, rec and
    ml arrays (the carve of tracer_patch_open) all move with maxOwnC, and the last patch is short (360 and 2562 cells).  Three tracers: at 48 cells the 80 KB
    hold one (diffused) or two (plain) tracers' rows beside the thickness rows, so k_tracer_patch's pass loop re-stages rows once or
    twice, where the only multi-pass case so far was 8 + 1.  Full masks over the linear dycore and partial masks under Del2 + Del4.
    7 steps over the linear dycore, 3 under Del2 + Del4 on the sphere (that twin's cost).  ico32 at K = 34 is left out: its twin alone
    takes longer than this whole file."""
    nsteps = 3 if (meshname, mode) == ("ico16", "del2+del4") else 7
    ref = tc.reference(meshname, K, mode, partial, ((nsteps, (3, 21, False), diff),))
    md = tc.Model(backend, meshname, K, mode=mode, partial=partial, patch_cells=patch_cells)
    try:
        mC = md.info["maxPatchCells"]
        assert mC == patch_cells
        if patch_cells == 24:
            assert 17 <= mC <= 42 and mC * 16 > 256 and mC * 6 <= 256
        if patch_cells == 48:
            assert mC >= 43 and mC * 6 > 256
        chunk = tc.patch_chunk(mC, K, 3, diff)
        assert chunk >= 1                                   # the 80 KB rule admits the patch form
        if patch_cells == 48:
            assert chunk < 3 and (K != 64 or chunk == (1 if diff else 2))       # more than one pass
        else:
            assert chunk == 3
        tr = set_tracers(md, meshname, tc.distinct_fields(md.mesh, K, 3), diff)
        step_and_check(md, tr, ref, nsteps)
        assert tr.path() == 1
    finally:
        md.close()


def test_form_flips_with_diffusion_at_the_lds_boundary(backend):
    """tracer_kernel refuses the patch form when maxOwnC * (16 K + 144 + 48 diff) exceeds 80 KB.  At K = 64 patches of 70
    cells take 70 * 1168 = 81 760 <= 81 920 bytes without diffusion (the largest dynamic LDS the kernel is ever launched with) and
    70 * 1216 = 85 120 with it: the default variant runs the patch form, the generic form once a diffusivity is set, and the patch
    form again after set_diffusivity(0).  Three segments of an eager step and a run of one, each bitwise against the twin's."""
    meshname, K, P = "planar", 64, 70
    sched = ((2, (3, 21, False), False), (2, None, True), (2, None, False))
    ref = tc.reference(meshname, K, "linear", False, sched)
    md = tc.Model(backend, meshname, K, patch_cells=P)
    try:
        mC = md.info["maxPatchCells"]
        assert 68 <= mC <= 70
        assert tc.patch_chunk(mC, K, 3, False) == 1 and tc.patch_chunk(mC, K, 3, True) == 0
        tr = set_tracers(md, meshname, tc.distinct_fields(md.mesh, K, 3), False)
        for seg, (kap, path) in enumerate(((None, 1), (tc.kappas(meshname, 3), 2), (0, 1))):
            if seg:
                tr.set_diffusivity(kap)
            step_and_check(md, tr, ref, 2, first=2 * seg)
            assert tr.path() == path, seg
    finally:
        md.close()


@DIFF
def test_patches_too_large_for_the_patch_form(backend, diff):
    """Patches of 80 cells at K = 64 need 80 * 1168 bytes: the default variant takes the generic form for want of LDS (no other
    test has a default-variant state that does), bitwise over 7 steps."""
    meshname, K = "planar", 64
    ref = tc.reference(meshname, K, "linear", False, ((7, (3, 21, False), diff),))
    md = tc.Model(backend, meshname, K, patch_cells=80)
    try:
        assert md.info["maxPatchCells"] == 80 and tc.patch_chunk(80, K, 3, diff) == 0
        tr = set_tracers(md, meshname, tc.distinct_fields(md.mesh, K, 3), diff)
        step_and_check(md, tr, ref, 7)
        assert tr.path() == 2
    finally:
        md.close()


# ---- cell orders -----------------------------------------------------------------------------------------------------------------
@DIFF
@pytest.mark.parametrize("order", ["none", "rcm", "classes"])
@pytest.mark.parametrize("meshname,K", [("ico16", 60), ("ico12f", 5)])
def test_tracers_in_other_cell_orders(backend, meshname, K, order, diff):
    """ORDER_NONE, ORDER_RCM and the default order under a two-valued cell class (class-major cells, patches that end at the class
    boundary): what moka_tracer_upload stores through put_rows, moka_tracer_download returns through get_rows exactly, at both
    levels, and 5 steps equal the twin reference of the default order -- the twin works in the caller's numbering."""
    ref = tc.reference(meshname, K, "linear", False, ((7, (3, 21, False), diff),))
    mesh = tc.get_mesh(meshname)
    kw = {"none": dict(ordering=L.ORDER_NONE), "rcm": dict(ordering=L.ORDER_RCM),
          "classes": dict(cell_class=(np.asarray(mesh.xCell) > np.median(mesh.xCell)).astype(np.int32))}[order]
    md = tc.Model(backend, meshname, K, **kw)
    try:
        perm = np.empty(mesh.nCells, dtype=np.int32)
        L.check(L.lib().moka_mesh_permutation(md.M._h, L.CELL, L.i32(perm)))
        assert not np.array_equal(perm, L.Plan(mesh, K, max_level_edge_top=K).permutation(L.CELL))      # not the default order
        f = tc.distinct_fields(mesh, K, 3)
        tr = set_tracers(md, meshname, f, diff)
        g = tc.distinct_fields(mesh, K, 2, seed=5)
        tr.set(0, g[0], 0); tr.set(2, g[1], 1)
        assert np.array_equal(tr.get(0, 0), g[0]) and np.array_equal(tr.get(0, 1), f[0]) and np.array_equal(tr.get(1, 0), f[1])
        assert np.array_equal(tr.get(2, 1), g[1]) and np.array_equal(tr.get(2, 0), f[2]) and np.array_equal(tr.get(1, 1), f[1])
        tr.set(0, f[0], 0); tr.set(2, f[2], 1)
        step_and_check(md, tr, ref, 5)
        assert tr.path() == (1 if meshname == "ico16" else 2)
    finally:
        md.close()


# ---- degenerate neighbourhoods -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,K", tc.TINY)
def test_tiny_periodic_meshes(backend, nx, ny, K):
    """The doubly periodic meshes of test_gpu_parity.py's test_tiny_periodic_meshes_bitwise: a cell meets the same neighbour through
    several slots, and one patch holds the whole mesh (4 x 4, 2 x 4 at K = 60: 16 and 8 cells), so every ch[i] of tracer_slots is a cache hit
    and `loc` ranges over all of ownN; 6 x 4 at K = 34 has a short second patch.  K = 1 and 8: the generic form.  Three diffused
    tracers, the first one 1 everywhere: it stays exactly 1.0.  (The twins' tendencies on these meshes: the CPU tests.)"""
    name = f"tiny-{nx}-{ny}"
    ref = tc.reference(name, K, "linear", False, ((7, (3, 21, True), True),))
    md = tc.Model(backend, name, K)
    try:
        tr = set_tracers(md, name, tc.distinct_fields(md.mesh, K, 3, unit_first=True), True)
        step_and_check(md, tr, ref, 7)
        assert tr.path() == (1 if K % 2 == 0 and 34 <= K <= 64 else 2)
        if tr.path() == 1 and nx * ny <= 16:
            assert md.info["nPatches"] == 1
        one = np.ones((md.mesh.nCells, K))
        assert np.array_equal(tr.get(0), one) and np.array_equal(tr.get(0, 0), one)
    finally:
        md.close()


# ---- tracers that come late and change ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K", [("ico16", 60), ("ico12f", 5)])
def test_late_and_changing_tracers(backend, meshname, K):
    """moka_set_tracers on a state that has stepped an odd number of times -- its time-level sets have swapped once, its RK buffers
    exist -- then 3 -> 9 (diffused) -> 1 tracers between runs: the arrays are released and re-made, trKappaDev with them.  3 steps
    without tracers; 3 fields, 4 steps; 9 fields with diffusivities, an eager step and a run of one (no graph); 1 field, 6 steps
    (graph replay).  Every segment equals the twin that took over the oracle's state, and the dycore equals a state that never had
    tracers throughout."""
    sched = ((3, 0, False), (4, (3, 21, False), False), (2, (9, 22, False), True), (6, (1, 23, False), False))
    ref = tc.reference(meshname, K, "linear", False, sched)
    md, plain = tc.Model(backend, meshname, K), tc.Model(backend, meshname, K)
    try:
        def same_dycore():
            for t in (0, 1):
                assert np.array_equal(md.Prog.normalVelocity[t].get(), plain.Prog.normalVelocity[t].get())
                assert np.array_equal(md.Prog.layerThickness[t].get(), plain.Prog.layerThickness[t].get())
                assert np.array_equal(md.Prog.ssh[t].get(), plain.Prog.ssh[t].get())

        md.run(3); plain.run(3)
        tc.check_dycore(md.Prog, ref[2])
        done = 3
        for nsteps, (n, seed, _), diff in sched[1:]:
            tr = set_tracers(md, meshname, tc.distinct_fields(md.mesh, K, n, seed=seed), diff)
            assert tr.path() == 0 and np.array_equal(tr.diffusivity(), tc.kappas(meshname, n) if diff else np.zeros(n))
            step_and_check(md, tr, ref, nsteps, first=done)
            plain.run(nsteps)
            done += nsteps
            same_dycore()
            assert tr.path() == (1 if meshname == "ico16" else 2)
    finally:
        md.close(); plain.close()


# ---- the stage weights -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kappa", [0.0, tc.EIG_KAPPA], ids=["plain", "diffused"])
@pytest.mark.parametrize("K,variant,path", [(4, 0, 2), (34, 0, 1), (34, 3, 2)])
def test_plane_wave_on_the_device(backend, K, variant, path, kappa):
    """The plane wave of tracer_cases.py through the C ABI: uniform flow U = (70, 40) over the regular hexagons, h = 250, ssh = 0,
    linear dycore, dt = 2; after 10 steps (one eager, nine through mk.run_steps) the downloaded tracer equals the analytic
    1 + 0.5 Re(R(z)^10 exp(i k . x)) -- not the twin -- within the CPU tests' 10 * 32 * 2^-53 * max|phi0| = 5.3e-14, the bound would
    refuse a third-order stage loop by six orders and the exponential, and the dycore fields have not moved by a bit.  Both kernel
    forms at K = 34, the generic one at K = 4; kappa = 0 and 0.02 dc^2 / dt."""
    mesh, state, phi0 = tc.eigenmode_state(K)
    md = tc.Model(backend, "planar-f0", K, variant=variant, state=state)
    try:
        tr = mk.set_tracers(md.Prog, [phi0], diffusivity=[kappa] if kappa else None)
        md.eager(1)
        md.run(tc.EIG_STEPS - 1)
        assert tr.path() == path
        tc.eigenmode_check(tr.get(0), mesh, K, kappa, phi0, f"K = {K}, variant {variant}, kappa = {kappa:g}")
        assert np.array_equal(md.Prog.normalVelocity[-1].get(), state[1]) and np.array_equal(md.Prog.layerThickness[-1].get(), state[2])
        assert np.array_equal(md.Prog.ssh[-1].get(), state[0])
    finally:
        md.close()
