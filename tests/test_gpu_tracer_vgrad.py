"""The gradient of a tracer objective with respect to the vertical diffusivity on the device (csrc/tracer_vmix.hip: k_vmix_tile_grad,
k_vmix_column_grad; the recording of moka_step_rk4_tracer_taped; moka_tracer_adjoint_want_vertical_gradient and its two readers):
everything bit for bit against the numpy twin of tests/tracer_vgrad_twin.py, through the Python API.

A case gives a model three tracers with pairwise distinct fields and vertical diffusivities (tracer_vmix_twin.kappavs: one exact zero,
the second), flags tracers 0 and 1 -- tracer 1 is the kappaV == 0 one --, records three RK4 steps on a tracer tape, seeds every tracer
with its own field, sweeps, and compares D, its three views and the scalar, and beside them X (and G, Wk, Wk4 where asked for).  The
twin's case is computed once (tracer_vgrad_twin.reference) and shared.  Every test here fails without the new entry points."""
import ctypes as C

import numpy as np
import pytest

import moka_hip as mk
import tracer_cases as tc
import tracer_kgrad_twin as tk
import tracer_vgrad_twin as tg
import tracer_vmix_twin as tv
from moka_hip import lib as L

pytestmark = pytest.mark.gpu
NSTEPS = 3


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)
    yield b
    b.close()


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def expected_path(K, variant, steps):
    """The form of the last pass a sweep with a flagged tracer runs: the gradient instances, in every step with dt != 0.0."""
    if K < 2 or all(dt == 0.0 for _, dt in steps):
        return 0
    return 1 if tg.tile_columns_grad(K, variant == 3) else 2


def model(backend, meshname, K, mode="linear", partial=False, variant=0, **kw):
    mlt = tv.column_mlt(tc.get_mesh(meshname), K) if partial == "floor" else None
    return tc.Model(backend, meshname, K, mode=mode, partial=partial is True, variant=variant, mlt=mlt, **kw)


def check_step(tr_, Prog, ref):
    for j in range(len(ref[1])):
        assert same(tr_.get(j), ref[1][j]), ("current", j)
        assert same(tr_.get(j, 0), ref[0][j]), ("previous", j)
    tc.check_dycore(Prog, ref)


def check_density(tape, j, D):
    """D_j, its three views and the scalar against the twin's D."""
    got = tape.vertical_density(j)
    assert np.array_equal(got, D), ("D", j, float(np.abs(got - D).max()))
    cell, prof, scalar = tg.views(D)
    assert np.array_equal(tape.vertical_density(j, "cell"), cell), ("cell", j)
    assert np.array_equal(tape.vertical_density(j, "profile"), prof), ("profile", j)
    assert tape.vertical_gradient(j) == scalar == tk.host_sum(D.ravel()), ("scalar", j)


def record(tape, tr_, md, ref, first=0):
    for s, (kv, dt) in enumerate(ref["steps"][first:], start=first):
        tr_.set_vertical_diffusivity(kv)
        tape.step(dt)                               # the taped step is the untaped one, bit for bit, flagged or not
        check_step(tr_, md.Prog, ref["forward"][s])


def sweep_case(backend, meshname, K, mode="linear", partial=False, variant=0, nT=3, steps=NSTEPS, vflags=(0, 1), diff=False, bih=False,
               flags=(), wants=(), fields=None, fill=None, **kw):
    ref = tg.reference(meshname, K, mode, partial, nT, steps, vflags, diff, bih, flags, wants, fields, fill)
    md = model(backend, meshname, K, mode, partial, variant, **kw)
    try:
        tr_ = mk.set_tracers(md.Prog, ref["fields"], diffusivity=ref["kappa"] if diff else None, biharmonic=ref["kappa4"] if bih else None)
        tape = mk.TracerAdjointTape(md.Prog, len(ref["steps"]))
        try:
            for j in vflags:
                tape.want_vertical_gradient(j)
            for j, bits in flags:
                tape.want_diffusivity_gradient(j, kappa=bool(bits & 1), biharmonic=bool(bits & 2))
            for j in wants:
                tape.want_source_gradient(j)
            for j in vflags:
                assert not tape.vertical_density(j).any()                # flagged and not swept: zeros
            record(tape, tr_, md, ref)
            grad, dkv = tape.gradient(ref["X"], vertical=True)
            assert tape.vmix_path() == expected_path(K, variant, ref["steps"])
            live = ~ref["dead"] if fill is not None else np.ones_like(ref["dead"])
            for j in range(nT):
                assert same(grad[j][live], ref["grad"][j][live]), ("X", j)
                assert (j in vflags) == (not np.isnan(dkv[j]))
            for j in wants:
                assert np.array_equal(tape.source_gradient(j), ref["G"][j]), ("G", j)
            for j, bits in flags:
                for b, bihf in ((1, False), (2, True)):
                    if bits & b:
                        assert np.array_equal(tape.diffusivity_density(j, biharmonic=bihf), ref["W"][j][b - 1]), ("density", j, b)
            for j in vflags:
                check_density(tape, j, ref["D"][j])
                assert dkv[j] == tg.views(ref["D"][j])[2]
            return ref
        finally:
            tape.close()
    finally:
        md.close()


# ---- forms and depths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 34, 60, 65])
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_forms_and_depths(backend, K, variant):
    """K = 2: one interface.  K = 3: the first interior row.  K = 2, 3: tiles of 64 columns; 34 .. 65: of 32, 360 cells: the last tile is
    short.  Variant 3 takes the column form; both give the twin's bits, hence each other's.  X equals tv.reference's: the plain sweep's."""
    ref = sweep_case(backend, "planar", K, variant=variant)
    plain = tv.reference("planar", K, "linear", False, 3, NSTEPS)
    assert ref["steps"][0][0][1] == 0.0 and ref["D"][1].any()           # tracer 1: the derivative at zero, not a zero
    for j in range(3):
        assert np.array_equal(ref["grad"][j], plain["grad"][j])


# ---- the boundaries of the LDS rule -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,path", [(19, 1), (20, 1), (79, 1), (80, 2)])
def test_form_boundaries_on_the_device(backend, K, path):
    """Each side of each boundary of the four-set rule (test_tracer_vgrad_twin.py tests the pure function): tiles of 64 up to K = 19, of
    32 up to K = 79 (81,024 B of LDS, above the default 64 KiB), the column form from K = 80."""
    assert expected_path(K, 0, [(None, 1.0)]) == path and tg.tile_columns_grad(K) == {19: 64, 20: 32, 79: 32, 80: 0}[K]
    sweep_case(backend, "tiny-4-4", K, steps=1)


# ---- the sea floor ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [None, np.nan], ids=["plain", "nan-below-the-floor"])
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_sea_floor(backend, variant, fill):
    """Columns of depth 0, 1, 2, 3 .. K.  With NaN in every level k >= nLev[c] of the tracers and the seeds, D is what it is without."""
    ref = sweep_case(backend, "planar", 34, variant=variant, partial="floor", fill=fill)
    assert {0, 1, 2, 3, 34} <= set(ref["nlev"].tolist()) and len(set(ref["nlev"].tolist())) > 10
    for j in (0, 1):
        D = ref["D"][j]
        assert not D[np.arange(34)[None, :] >= (ref["nlev"] - 1)[:, None]].any() and np.isfinite(D).all() and D.any()
    if fill is not None:
        finite = tg.reference("planar", 34, "linear", "floor", 3, NSTEPS, (0, 1))
        assert all(np.array_equal(ref["D"][j], finite["D"][j]) for j in (0, 1))


# ---- small and irregular meshes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K", [("tiny-4-4", 60), ("ico12f", 5)])
def test_meshes(backend, meshname, K):
    """16 cells: fewer columns than a tile.  ico12f: pentagons and heptagons, 1442 cells."""
    sweep_case(backend, meshname, K)


def test_nine_tracers(backend):
    sweep_case(backend, "planar", 34, nT=9, vflags=(1, 2, 4, 7, 8))


@pytest.mark.parametrize("mode", ["nonlinear", "del2+del4"])
def test_beside_every_other_gradient(backend, mode):
    sweep_case(backend, "planar", 34, mode=mode, diff=True, bih=True, flags=((0, 3), (2, 3)), wants=(2,), vflags=(0, 2))


# ---- cell orderings -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{"ordering": L.ORDER_NONE}, {"ordering": L.ORDER_RCM}, {"ordering": L.ORDER_RCB}, {"patch_cells": 24}],
                         ids=["none", "rcm", "rcb", "patch24"])
def test_density_does_not_know_the_cell_order(backend, kw):
    """D in the caller's numbering is the twin's under every ordering, hence identical across them."""
    sweep_case(backend, "planar", 34, partial="floor", **kw)


# ---- coefficients changing between steps --------------------------------------------------------------------------------------------
def test_coefficients_change_between_steps(backend):
    """kappavs; every kappaV zero (the pass runs gradient-only); a step with dt == 0.0 (no pass); kappaV changed again."""
    K = 34
    kv = tv.kappavs("planar", K, 3)
    steps = ((None, None), ([0.0, 0.0, 0.0], None), (None, 0.0), ([kv[2], kv[0], 0.0], None))
    ref = sweep_case(backend, "planar", K, steps=steps, vflags=(0, 1, 2))
    assert all(ref["D"][j].any() for j in range(3))


def test_a_tape_of_zero_dt_steps_launches_no_pass(backend):
    ref = sweep_case(backend, "planar", 6, steps=((None, 0.0), (None, 0.0)))
    assert not ref["D"][0].any() and not ref["D"][1].any()


def test_one_level(backend):
    ref = sweep_case(backend, "planar", 1, steps=2)
    assert not ref["D"][0].any()


def test_unit_tracer_and_zero_seed(backend):
    """The unit tracer's density is exactly 0.0; a zero seed gives zeros."""
    ref = sweep_case(backend, "planar", 34, fields="unit-first")
    assert not ref["D"][0].any() and ref["D"][1].any()
    md = model(backend, "planar", 34)
    try:
        tr_ = mk.set_tracers(md.Prog, ref["fields"])
        tape = mk.TracerAdjointTape(md.Prog, NSTEPS)
        tape.want_vertical_gradient(1)
        tape.want_vertical_gradient(2)
        record(tape, tr_, md, ref)
        grad, dkv = tape.gradient([None] * 3, vertical=True)
        assert all(not g.any() for g in grad) and np.isnan(dkv[0]) and dkv[1] == 0.0 and dkv[2] == 0.0
        assert not tape.vertical_density(1).any() and not tape.vertical_density(2).any()
        tape.close()
    finally:
        md.close()


# ---- life cycle ---------------------------------------------------------------------------------------------------------------------
def test_life_cycle(backend):
    """seed -> sweep -> read; record again: D stays readable until the first new seed zeroes it; the second sweep equals the twin's
    sweep over the second records alone."""
    K = 6
    ref = tg.reference("planar", K, "linear", False, 3, 4, (0, 1))
    twin = ref["twin"]
    first = tg.VgradAdjointTwin(twin).sweep_vgrad(twin.tape[:2], [x.copy() for x in ref["X"]], (0, 1))
    second = tg.VgradAdjointTwin(twin).sweep_vgrad(twin.tape[2:], [x.copy() for x in ref["X"]], (0, 1))
    md = model(backend, "planar", K)
    try:
        tr_ = mk.set_tracers(md.Prog, ref["fields"])
        tape = mk.TracerAdjointTape(md.Prog, 2)
        tape.want_vertical_gradient(0)
        tape.want_vertical_gradient(1)
        for half, exp in ((0, first), (1, second)):
            for s in range(2 * half, 2 * half + 2):
                kv, dt = ref["steps"][s]
                tr_.set_vertical_diffusivity(kv)
                tape.step(dt)
                check_step(tr_, md.Prog, ref["forward"][s])
            if half == 1:
                for j in (0, 1):
                    check_density(tape, j, first[3][j])              # still the first sweep's
                tape.seed(0, ref["X"][0])
                assert not tape.vertical_density(0).any() and not tape.vertical_density(1).any()
            grad = tape.gradient(ref["X"])
            for j in range(3):
                assert np.array_equal(grad[j], exp[0][j])
            for j in (0, 1):
                check_density(tape, j, exp[3][j])
            assert tape.steps() == 0
        assert not np.array_equal(first[3][0], second[3][0])
        tape.close()
    finally:
        md.close()


# ---- error codes --------------------------------------------------------------------------------------------------------------------
def test_error_codes(backend):
    K = 6
    ref = tv.reference("planar", K, "linear", False, 3, NSTEPS)
    md = model(backend, "planar", K)
    lib = L.lib()
    try:
        tr_ = mk.set_tracers(md.Prog, ref["fields"], vertical=ref["kappaV"])
        tape = mk.TracerAdjointTape(md.Prog, NSTEPS)
        h = tape._h
        out, buf = C.c_double(7.0), np.full((md.mesh.nCells, K), 7.0)
        want, scalar, dens = (lib.moka_tracer_adjoint_want_vertical_gradient, lib.moka_tracer_adjoint_vertical_gradient,
                              lib.moka_tracer_adjoint_vertical_density_download)
        assert want(None, 0, 1) == L.ERR_ARG and scalar(None, 0, C.byref(out)) == L.ERR_ARG and dens(None, 0, 0, L.f64(buf)) == L.ERR_ARG
        for j in (-1, 3):
            assert want(h, j, 1) == L.ERR_ARG and scalar(h, j, C.byref(out)) == L.ERR_ARG and dens(h, j, 0, L.f64(buf)) == L.ERR_ARG
        assert scalar(h, 0, C.byref(out)) == L.ERR_ARG and dens(h, 0, 0, L.f64(buf)) == L.ERR_ARG           # not flagged
        assert want(h, 0, 1) == 0 and want(h, 0, 1) == 0
        assert scalar(h, 0, None) == L.ERR_ARG and dens(h, 0, 0, None) == L.ERR_ARG
        for view in (-1, 3):
            assert dens(h, 0, view, L.f64(buf)) == L.ERR_ARG
        assert scalar(h, 1, C.byref(out)) == L.ERR_ARG and out.value == 7.0 and np.all(buf == 7.0)
        assert scalar(h, 0, C.byref(out)) == 0 and out.value == 0.0                                          # flagged, not swept
        assert want(h, 0, 0) == 0 and scalar(h, 0, C.byref(out)) == L.ERR_ARG
        # the plain tape: the path and X of the existing cases
        assert tape.vmix_path() == 0
        for _ in range(NSTEPS):
            tape.step(md.dt)
        assert want(h, 0, 1) == L.ERR_ARG and want(h, 0, 0) == L.ERR_ARG                                      # recorded steps
        tape.seed(0, ref["X"][0])
        assert want(h, 0, 1) == L.ERR_ARG                                                                     # between a seed and its sweep
        grad = tape.gradient(ref["X"])
        assert tape.vmix_path() == (1 if tv.tile_columns(K) else 2)
        for j in range(3):
            assert np.array_equal(grad[j], ref["grad"][j])
        assert want(h, 2, 1) == 0 and scalar(h, 2, C.byref(out)) == 0 and out.value == 0.0                   # an empty tape again
        with pytest.raises(ValueError):
            tape.vertical_density(2, "column")
        assert tr_.vmix_path() == 1
        tape.close()
    finally:
        md.close()
