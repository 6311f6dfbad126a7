"""Partitioned meshes over a bathymetry mask, with poisoned levels: the product of what test_partition_gloo.py pins over full columns and
what test_gpu_poison.py pins on whole meshes.  A rank's local mesh has what no whole mesh has -- rim edges whose cellsOnEdge names the
inside cell twice, edgesOnEdge slots zeroed because the neighbour is not local, stand-in vertices and cells in the two-ring halo,
class-major patches, stage launches over a sub-range of patches that starts at p0 > 0, split Forward-Euler launches and preparation
passes, transposed stages by class, and pack / push / unpack kernels that move whole rows, sea floor included -- and with
maxLevelEdgeTop = K every wave of that code takes its "every level active" branch.

Every test: a LocalCluster on one GPU over poison_cases' basin mask (every rank takes mlt[lm.edges_g]), the state of
poison_cases.state with NaN (one case: -inf, one: clean) on the poison set of the WHOLE mesh, and the assembled owned rows
`poison_cases.same` as the single-domain reference over whole fields, inactive levels included; layerThickness and ssh finite.
tests/test_partition_masks.py shows on the CPU that a correct partitioned implementation meets these references and that three wrong
ones do not, and that on every rank the boundary class and the interior class hold patches of partial depth and partial-depth rows are
sent (tests/partition_cases.py: conditions()).

Every test also asserts the form it names: the transport (cl.direct), that the stage launches by class are served
(moka_rk4_dist_parts_available), and every rank's lanesPerColumn / ldsBytesPerBlock / class patch counts, which are those of the host
plan in conditions().  Below K = 34 the lane-group kernels run; at K = 34, 60 and 80 (fp32) the LDS-tiled patch form; at K = 64 in
patches of 48 cells a patch of a local mesh gathers more than 254 rows, so -- unlike on the whole mesh -- the plan builds no row
lists (ldsBytesPerBlock = 0) and the stage kernels take their fallback form: that is what those cases pin."""
import numpy as np
import pytest

import partition_cases as pt
import poison_cases as pc
import tracer_cases as tc
import tracer_kgrad_twin as tk
from moka_hip import lib as L
from moka_hip import parallel as par
from test_partition_gloo import run_workers

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]


def cluster(meshname, K, world, mode="linear", poison="nan", direct=True, overlap=-1, patch_cells=0, state_bytes=8, variant=0,
            mask="basin"):
    """(cluster, mesh) with the state of pc.state uploaded and exchanged; the forms asserted."""
    mesh = tc.get_mesh(meshname)
    (ssh, u, h, rest), _ = pc.state(meshname, K, mode, poison)
    mlt = {"basin": pc.mask_of(meshname, K), "full": np.full(mesh.nEdges, K), None: None}[mask]
    visc = tc.viscosities(mesh, tc.dt_of(meshname))[0] if mode == "nonlinear+del2" else 0.0
    cl = par.LocalCluster(mesh, ssh, u, h, rest, tc.dt_of(meshname), world, patch_cells=patch_cells, state_bytes=state_bytes,
                          direct=direct, overlap=overlap, nonlinear=mode != "linear", visc_del2=visc, placement_tries=1,
                          max_level_edge_top=mlt)
    try:
        for b in cl.backends:
            b.set_kernel_variant(variant)
        assert cl.direct == direct
        if mask == "basin":
            check_forms(cl, meshname, K, world, pc.RINGS[mode], patch_cells, state_bytes, variant)
            for m, lm in zip(cl.models, pt.locals_of(meshname, world, pc.RINGS[mode])):
                assert np.array_equal(m.mesh.VertMesh.maxLevelEdge.Top, pc.mask_of(meshname, K)[lm.edges_g])
        cl.exchange_state()
    except BaseException:
        cl.close()
        raise
    return cl, mesh


def check_forms(cl, meshname, K, world, rings, patch_cells, state_bytes, variant):
    cond = pt.conditions(meshname, K, world, rings, patch_cells, state_bytes)
    ran = [(m.mesh.info()["lanesPerColumn"], m.mesh.info()["ldsBytesPerBlock"], m.p_boundary, m.p_owned - m.p_boundary,
            m.mesh.info()["nPatches"] - m.p_owned) for m in cl.models]
    what = (meshname, K, world, "per rank (lanes, LDS bytes, boundary / interior / halo patches):", ran)
    for got, c in zip(ran, cond):
        assert got == (c["lanes"], c["lds"]) + c["patches"], (what, "the host plan:", c)
        assert min(got[2:]) >= 1, what
        if K < 34:
            assert got[0] == tk.lanes(K), what
        elif variant == 0:
            assert (got[1] > 0) == (patch_cells == 0), what
    if meshname == "ico12f":
        assert all(m.mesh.info()["maxEdgesUsed"] > 6 for m in cl.models), what


def parts_available(cl):
    return [bool(L.lib().moka_rk4_dist_parts_available(m._halo)) for m in cl.models]


def expect(got, ref, what):
    assert pc.same(got, ref), (what, "elements whose NaN-ness differs, others whose bits differ:", pc.differences(got, ref))


def check_state(cl, mesh, K, ref, what):
    ssh, u, h = cl.gather_owned(mesh.nCells, mesh.nEdges, K)
    expect(u, ref["u1"], (what, "u1"))
    expect(h, ref["h1"], (what, "h1"))
    expect(ssh, ref["ssh1"], (what, "ssh1"))
    assert np.isfinite(h).all() and np.isfinite(ssh).all(), what


# ---- linear RK4 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K,world,how,overlap,poison,P,variant", pt.LINEAR_CASES)
def test_linear_rk4(meshname, K, world, how, overlap, poison, P, variant):
    """Direct and buffered transport, boundary beside or in front of the interior launch, the generic kernels at a patch-form K
    (variant 3), every stage one launch over the local mesh (step_rk4_whole): after step 2 and after step 4."""
    ref = pc.rk4(meshname, K, "linear", poison, pt.LINEAR_STEPS)
    cl, mesh = cluster(meshname, K, world, poison=poison, direct=how == "direct", overlap=overlap, patch_cells=P, variant=variant)
    try:
        assert all(parts_available(cl))
        done = 0
        for r, n in zip(ref, pt.LINEAR_STEPS):
            for _ in range(n - done):
                (cl.step_rk4_whole if how == "whole" else cl.step_rk4)()
            done = n
            check_state(cl, mesh, K, r, ("step", n))
    finally:
        cl.close()


@pytest.mark.parametrize("meshname,K,world,how", pt.FP32_CASES)
def test_fp32_storage(meshname, K, world, how):
    """fp32-stored states (the halo rows travel as floats) against the storage-emulating oracle."""
    ref = pc.rk4(meshname, K, "linear", "nan", pt.LINEAR_STEPS, "mixed")
    cl, mesh = cluster(meshname, K, world, direct=how == "direct", state_bytes=4)
    try:
        done = 0
        for r, n in zip(ref, pt.LINEAR_STEPS):
            for _ in range(n - done):
                cl.step_rk4()
            done = n
            check_state(cl, mesh, K, r, ("fp32 step", n))
    finally:
        cl.close()


# ---- Forward Euler --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K,flags,world,how,sbytes", pt.FE_CASES)
def test_forward_euler(meshname, K, flags, world, how, sbytes):
    """The split Forward-Euler launches (vertex pass, boundary, interior): the new level after every step, every array of Diag and Tend
    after the last (velocityDivCell and relativeVorticity are NaN in the oracle too below an edge's top); then an RK4 step and one
    more Forward-Euler step."""
    ref = pc.forward_euler(meshname, K, flags, "nan", pc.FE_STEPS, sbytes == 4)
    cl, mesh = cluster(meshname, K, world, direct=how == "direct", state_bytes=sbytes)
    try:
        for step in range(pc.FE_STEPS):
            cl.step_fe(flags)
            check_state(cl, mesh, K, ref[step], ("FE step", step + 1))
        d = cl.gather_diagnostics(mesh, K)
        for name in ("hEdge", "F", "div", "vort", "tendU", "tendH"):
            expect(d[name], ref[-1][name], ("FE", name))
        cl.step_rk4()
        cl.step_fe(pt.FE_TAIL_FLAGS(flags, sbytes == 4))
        check_state(cl, mesh, K, pt.fe_rk4_fe(meshname, K, flags, "nan", sbytes == 4), "FE, RK4, FE")
    finally:
        cl.close()


# ---- nonlinear terms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", pt.NL_MODES)
@pytest.mark.parametrize("meshname,K,world,how,P", pt.NL_CASES)
def test_nonlinear_terms(meshname, K, world, how, P, mode):
    """Two-ring halos with stand-in vertices and cells, poison at R = 2: the stage kernels by class with the split preparation passes
    (moka_rk4_dist_stage parts 3 and 4) over both transports, alternating with whole-mesh stages; whole-mesh stages only where the
    per-patch kernels do not serve the shape -- the library must say so."""
    ref = pc.rk4(meshname, K, mode, "nan", pc.NL_STEPS)[0]
    cl, mesh = cluster(meshname, K, world, mode=mode, direct=how == "direct", patch_cells=P)
    try:
        assert all(m.lm.rings == 2 for m in cl.models)
        parts = parts_available(cl)
        assert all(p == (meshname == "planar" and K % 2 == 0 and 34 <= K <= 64 and P == 0) for p in parts), (meshname, K, P, parts)
        assert all(parts) == (how != "whole")
        for i in range(pc.NL_STEPS[0]):
            whole = how == "whole" or (how == "alternate" and i % 2 == 1)
            (cl.step_rk4_whole if whole else cl.step_rk4)()
        check_state(cl, mesh, K, ref, (mode, how))
    finally:
        cl.close()


# ---- reverse mode ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K,world,overlap,poison", pt.ADJ_RK4_CASES)
def test_reverse_mode_rk4(meshname, K, world, overlap, poison):
    """d sum(ssh^2) / d initial state over two taped RK4 steps, transposed stages by class (moka_adjoint_rk4_stage_part) or whole.
    Compared as test_gpu_poison.py::test_dycore_adjoint compares: dJ/dnormalVelocity whole and finite, dJ/dlayerThickness where the
    oracle is finite (it is NaN in the oracle itself where that multiplies a poisoned velocity by an adjoint of zero)."""
    n = pt.ADJ_RK4_STEPS
    ref = pc.adjoint(meshname, K, "rk4", 0, poison, n)
    cl, mesh = cluster(meshname, K, world, poison=poison, direct=False)
    try:
        cl.tape(n)
        for _ in range(n):
            cl.step_rk4_taped()
        check_state(cl, mesh, K, pc.rk4(meshname, K, "linear", poison, pt.LINEAR_STEPS)[0], "taped steps")
        expect(cl.gather_owned(mesh.nCells, mesh.nEdges, K)[0], ref["ssh1"], "ssh")
        avail = [m.adjoint_parts_available() for m in cl.models]
        assert all(a == (K % 2 == 0 and 34 <= K <= 64) for a in avail), (meshname, K, avail)
        gu, gh = cl.adjoint_gradient(n, mesh.nCells, mesh.nEdges, K, overlap=overlap)
        expect(gu, ref["normalVelocity"], "dJ/du")
        assert np.isfinite(gu).all() and np.abs(gu).max() > 0
        assert pc.same_where_finite(gh, ref["layerThickness"]), ("dJ/dh", pc.differences(gh, ref["layerThickness"]))
    finally:
        cl.close()


@pytest.mark.parametrize("meshname,K,flags,world", pt.ADJ_FE_CASES)
def test_reverse_mode_forward_euler(meshname, K, flags, world):
    n = pt.ADJ_FE_STEPS
    ref = pc.adjoint(meshname, K, "fe", flags, "nan", n)
    cl, mesh = cluster(meshname, K, world, direct=world != 2)
    try:
        cl.tape(n)
        for _ in range(n):
            cl.step_fe_taped(flags)
        check_state(cl, mesh, K, pc.forward_euler(meshname, K, flags, "nan", pc.FE_STEPS)[n - 1], "taped steps")
        expect(cl.gather_owned(mesh.nCells, mesh.nEdges, K)[0], ref["ssh1"], "ssh")
        g = cl.adjoint_gradient_fe(n, mesh, K)
        expect(g["normalVelocity"], ref["normalVelocity"], "dJ/du")
        expect(g["ssh"], ref["ssh"], "dJ/dssh")
        assert np.isfinite(g["normalVelocity"]).all() and np.abs(g["normalVelocity"]).max() > 0
        for name in ("layerThickness", "layerThicknessEdge"):
            assert pc.same_where_finite(g[name], ref[name]), (name, pc.differences(g[name], ref[name]))
    finally:
        cl.close()


# ---- separate processes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,K,transport", [(2, 60, "ipc"), (3, 34, "gloo")])
def test_separate_processes(world, K, transport):
    """tests/dist_worker.py with its trailing "basin": one process per rank, one GPU shared."""
    run_workers(world, "gpu", K, 0, transport, "basin")


# ---- the argument itself --------------------------------------------------------------------------------------------------------------
def test_a_full_mask_is_no_mask():
    meshname, K, world = "planar", 34, 2
    states = []
    for mask in (None, "full"):
        cl, mesh = cluster(meshname, K, world, poison=None, mask=mask)
        try:
            for _ in range(2):
                cl.step_rk4()
            states.append(cl.gather_owned(mesh.nCells, mesh.nEdges, K) + tuple(m.snapshot() for m in cl.models))
        finally:
            cl.close()
    (a_own, a_loc), (b_own, b_loc) = ((s[:3], s[3:]) for s in states)
    assert all(np.array_equal(pc._bits(x), pc._bits(y)) for x, y in zip(a_own, b_own))
    assert all(np.array_equal(pc._bits(x), pc._bits(y)) for p, q in zip(a_loc, b_loc) for x, y in zip(p, q))
    assert np.isfinite(a_own[1]).all()


def test_bad_masks_raise():
    meshname, K = "planar", 8
    mesh, mlt = tc.get_mesh(meshname), pc.mask_of(meshname, K)
    (ssh, u, h, rest), _ = pc.state(meshname, K, "linear", None)
    over = mlt.copy()
    over[5] = K + 1
    for bad in (mlt[:-1], over):
        with pytest.raises(ValueError):
            par.LocalCluster(mesh, ssh, u, h, rest, tc.dt_of(meshname), 2, placement_tries=1, max_level_edge_top=bad)
        with pytest.raises(ValueError):
            par.DistributedModel(mesh, ssh, u, h, rest, tc.dt_of(meshname), None, 0, 2, transport="local", max_level_edge_top=bad)
