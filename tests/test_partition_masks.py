"""The partition-over-a-mask device tests (test_gpu_partition_masks.py) are not vacuous -- shown here without a GPU, for every one of
their cases (tests/partition_cases.py names them):

  * the partitioned step emulated on the CPU (partition_cases.emulate: the oracle as every rank's compute over its local mesh and its
    rows of the mask, halo rows overwritten from the owners) is `poison_cases.same` as the single-domain reference the device test
    compares with, clean and poisoned, over whole fields -- so a correct partitioned implementation satisfies those references;
  * the references are closed on the active sets (poison_cases.closed);
  * the local meshes meet the conditions the device tests rely on: on every rank the boundary class and the interior class each hold
    a patch with an edge of partial depth and the rank sends a partial-depth edge row (a); some rank sends a full-column row (b); in
    every planar case, and on ico12f at world 5, some rank sends a land row (c);
  * three wrong emulations -- ranks that ignore the mask, ranks that take mlt[:nEdgesLocal] instead of mlt[lm.edges_g], an exchange
    that skips one neighbour's rows -- differ from the reference on the active set, in a generic-form and in a patch-form case;
  * the new argument of the partitioned models as far as it can be checked without a device.

The reverse-mode cases of the device file compare their final state with the same forward references, which is what is emulated
here for them; their gradients come from poison_cases.adjoint, whose closure test_poison_twin.py pins."""
import ctypes as C

import numpy as np
import pytest

import partition_cases as pt
import poison_cases as pc
import tracer_cases as tc
from moka_hip import lib as L
from moka_hip import parallel as par

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")


def agree(got, ref, names, what):
    for n in names:
        assert pc.same(got[n], ref[n]), (what, n, "elements whose NaN-ness differs, others whose bits differ:", pc.differences(got[n], ref[n]))


def closed(meshname, K, clean, pois, names, table):
    mesh, mlt = tc.get_mesh(meshname), pc.mask_of(meshname, K)
    for n in names:
        pc.closed(clean[n], pois[n], pc.active(mesh, mlt, K, table[n]))


def differs_on_active(meshname, K, got, ref, name, where):
    act = pc.active(tc.get_mesh(meshname), pc.mask_of(meshname, K), K, where)
    sel = np.ones(ref[name].shape, dtype=bool) if act is None else act
    assert np.isfinite(ref[name][sel]).all()
    return int((pc._bits(got[name])[sel] != pc._bits(ref[name])[sel]).sum())


# ---- the emulation reproduces every reference of the device file ----------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K,world,poison", sorted({(c[0], c[1], c[2], c[5]) for c in pt.LINEAR_CASES}, key=str))
def test_linear_rk4(meshname, K, world, poison):
    ref = pc.rk4(meshname, K, "linear", poison, pt.LINEAR_STEPS)
    emu = pt.emulate(meshname, K, world, "linear", poison, max(pt.LINEAR_STEPS))
    for r, n in zip(ref, pt.LINEAR_STEPS):
        agree(emu[n - 1], r, ("u1", "h1", "ssh1"), (meshname, K, world, poison, "step", n))
        assert np.isfinite(r["h1"]).all() and np.isfinite(r["ssh1"]).all()
    if poison is not None:
        clean = pc.rk4(meshname, K, "linear", None, pt.LINEAR_STEPS)
        for a, b in zip(clean, ref):
            closed(meshname, K, a, b, ("u1", "h1", "ssh1"), pc.RK4_ACTIVE)
        assert not pc.same(clean[-1]["u1"], ref[-1]["u1"])                    # the poison is still there


@pytest.mark.parametrize("meshname,K,world,how", pt.FP32_CASES)
def test_fp32_storage(meshname, K, world, how):
    for poison in (None, "nan"):
        ref = pc.rk4(meshname, K, "linear", poison, pt.LINEAR_STEPS, "mixed")
        emu = pt.emulate(meshname, K, world, "linear", poison, max(pt.LINEAR_STEPS), mixed=True)
        for r, n in zip(ref, pt.LINEAR_STEPS):
            agree(emu[n - 1], r, ("u1", "h1", "ssh1"), (meshname, K, world, poison, "fp32 step", n))
    for a, b in zip(pc.rk4(meshname, K, "linear", None, pt.LINEAR_STEPS, "mixed"), ref):
        closed(meshname, K, a, b, ("u1", "h1", "ssh1"), pc.RK4_ACTIVE)


@pytest.mark.parametrize("meshname,K,flags,world,how,sbytes", pt.FE_CASES)
def test_forward_euler(meshname, K, flags, world, how, sbytes):
    mixed = sbytes == 4
    for poison in (None, "nan"):
        ref = pc.forward_euler(meshname, K, flags, poison, pc.FE_STEPS, mixed)
        emu = pt.emulate_fe(meshname, K, world, flags, poison, pc.FE_STEPS, mixed)
        for step in range(pc.FE_STEPS):
            agree(emu[step], ref[step], ("u1", "h1", "ssh1"), (meshname, K, flags, world, poison, "step", step + 1))
        agree(emu[-1], ref[-1], tuple(pt.FE_FIELDS), (meshname, K, flags, world, poison, "last step"))
    clean = pc.forward_euler(meshname, K, flags, None, pc.FE_STEPS, mixed)
    closed(meshname, K, clean[-1], ref[-1], tuple(pt.FE_FIELDS), pc.FE_ACTIVE)
    tail_c, tail_p = pt.fe_rk4_fe(meshname, K, flags, None, mixed), pt.fe_rk4_fe(meshname, K, flags, "nan", mixed)
    closed(meshname, K, tail_c, tail_p, ("u1", "h1", "ssh1"), pc.RK4_ACTIVE)


@pytest.mark.parametrize("mode", pt.NL_MODES)
@pytest.mark.parametrize("meshname,K,world", sorted({c[:3] for c in pt.NL_CASES}))
def test_nonlinear_terms(meshname, K, world, mode):
    for poison in (None, "nan"):
        ref = pc.rk4(meshname, K, mode, poison, pc.NL_STEPS)[0]
        emu = pt.emulate(meshname, K, world, mode, poison, pc.NL_STEPS[0])[-1]
        agree(emu, ref, ("u1", "h1", "ssh1"), (meshname, K, world, mode, poison))
    closed(meshname, K, pc.rk4(meshname, K, mode, None, pc.NL_STEPS)[0], ref, ("u1", "h1", "ssh1"), pc.RK4_ACTIVE)


@pytest.mark.parametrize("meshname,K,world,poison", sorted({(c[0], c[1], c[2], c[4]) for c in pt.ADJ_RK4_CASES}, key=str))
def test_reverse_mode_rk4_forward_state(meshname, K, world, poison):
    ref = pc.adjoint(meshname, K, "rk4", 0, poison, pt.ADJ_RK4_STEPS)
    emu = pt.emulate(meshname, K, world, "linear", poison, pt.ADJ_RK4_STEPS)[-1]
    assert pc.same(emu["ssh1"], ref["ssh1"]) and np.isfinite(ref["ssh1"]).all()
    assert np.isfinite(ref["normalVelocity"]).all() and np.abs(ref["normalVelocity"]).max() > 0


@pytest.mark.parametrize("meshname,K,flags,world", pt.ADJ_FE_CASES)
def test_reverse_mode_fe_forward_state(meshname, K, flags, world):
    ref = pc.adjoint(meshname, K, "fe", flags, "nan", pt.ADJ_FE_STEPS)
    emu = pt.emulate_fe(meshname, K, world, flags, "nan", pt.ADJ_FE_STEPS)[-1]
    assert pc.same(emu["ssh1"], ref["ssh1"]) and np.isfinite(ref["ssh1"]).all()
    assert np.isfinite(ref["normalVelocity"]).all() and np.abs(ref["normalVelocity"]).max() > 0


# ---- the conditions -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K,world,rings,P,sbytes", pt.PLAN_CASES)
def test_conditions(meshname, K, world, rings, P, sbytes):
    cond = pt.conditions(meshname, K, world, rings, P, sbytes)
    print(pt.conditions_table([(meshname, K, world, rings, P, sbytes)]))
    assert len(cond) == world
    for r, c in enumerate(cond):
        assert min(c["patches"]) >= 1, (r, c)                                            # boundary, interior and halo classes exist
        assert c["boundary"]["partial"] >= 1 and c["interior"]["partial"] >= 1, (r, c)   # (a)
        assert c["sent"]["partial"] >= 1, (r, c)                                         # (a)
    assert any(c["sent"]["full"] for c in cond)                                          # (b)
    if meshname == "planar" or world == 5:
        assert any(c["sent"]["land"] for c in cond)                                      # (c)


# ---- the mutants ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", ["no-mask", "local-index", "skip-neighbour"])
@pytest.mark.parametrize("meshname,K,world", [("planar", 8, 3), ("planar", 34, 2)])          # the generic form, the patch form
def test_mutants_differ_on_the_active_set(meshname, K, world, mutant):
    n = max(pt.LINEAR_STEPS)
    ref = pc.rk4(meshname, K, "linear", "nan", pt.LINEAR_STEPS)[-1]
    emu = pt.emulate(meshname, K, world, "linear", "nan", n, mutant=mutant)[-1]
    du, dh = differs_on_active(meshname, K, emu, ref, "u1", "edge"), differs_on_active(meshname, K, emu, ref, "h1", "all")
    print(f"{meshname} K = {K} world {world} {mutant}: differs from the reference in {du} active elements of u1 and {dh} of h1")
    assert du > 0 and dh > 0
    fref = pc.forward_euler(meshname, K, 3, "nan", pc.FE_STEPS)[-1]
    femu = pt.emulate_fe(meshname, K, world, 3, "nan", pc.FE_STEPS, mutant=mutant)[-1]
    assert differs_on_active(meshname, K, femu, fref, "u1", "edge") > 0


# ---- the argument ---------------------------------------------------------------------------------------------------------------------
def test_mask_argument_without_a_device():
    """check_level_mask is what both constructors call first; the local descriptor of a rank carries mlt[lm.edges_g], and None gives
    the all-K array the models have always handed to make_desc."""
    meshname, K, world = "planar", 8, 3
    mesh, mlt = tc.get_mesh(meshname), pc.mask_of(meshname, K)
    assert par.check_level_mask(mesh, K, None) is None
    got = par.check_level_mask(mesh, K, mlt.astype(np.int64))
    assert got.dtype == np.int32 and np.array_equal(got, mlt)
    for bad in (mlt[:-1], mlt.reshape(1, -1), np.where(np.arange(mesh.nEdges) == 7, K + 1, mlt), np.where(np.arange(mesh.nEdges) == 3, -1, mlt),
                mlt.astype(np.float64)):
        with pytest.raises(ValueError):
            par.check_level_mask(mesh, K, bad)
    from moka_hip import api
    rest = tc.state_of(meshname, K)[3]
    for lm in pt.locals_of(meshname, world, 1):
        vm = api.VerticalMesh(api.HorzMesh(lm.mesh), nVertLevels=K, restingThickness=rest[lm.cells_g], multilayer=True)
        d0, k0 = L.make_desc(lm.mesh, K, vm.restingThicknessSum, vm.maxLevelEdge.Top, 0, 0, cell_class=lm.cell_class)
        assert np.array_equal(k0["maxLevelEdgeTop"], np.full(lm.mesh.nEdges, K)) and k0["maxLevelEdgeTop"].dtype == np.int32
        vm.maxLevelEdge.Top[:] = par.check_level_mask(mesh, K, np.full(mesh.nEdges, K))[lm.edges_g]
        d1, k1 = L.make_desc(lm.mesh, K, vm.restingThicknessSum, vm.maxLevelEdge.Top, 0, 0, cell_class=lm.cell_class)
        assert set(k0) == set(k1) and all(np.array_equal(k0[n], k1[n]) and k0[n].dtype == k1[n].dtype for n in k0)
        assert all(getattr(d0, n) == getattr(d1, n) for n, t in d0._fields_ if not isinstance(getattr(d0, n), C._Pointer))
        vm.maxLevelEdge.Top[:] = mlt[lm.edges_g]
        _, k2 = L.make_desc(lm.mesh, K, vm.restingThicknessSum, vm.maxLevelEdge.Top, 0, 0, cell_class=lm.cell_class)
        assert np.array_equal(k2["maxLevelEdgeTop"], mlt[lm.edges_g]) and 0 < (k2["maxLevelEdgeTop"] < K).sum() < lm.mesh.nEdges
