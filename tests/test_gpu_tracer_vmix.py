"""Implicit vertical diffusion of passive tracers on the device (csrc/tracer_vmix.hip: k_vmix_tile, k_vmix_column; the launches of
step_rk4 and moka_tracer_adjoint_sweep; moka_set_tracer_vertical_diffusion): everything bit for bit against the numpy twin of
tests/tracer_vmix_twin.py.

A case gives a model three tracers with pairwise distinct fields and vertical diffusivities (tracer_vmix_twin.kappavs: s / hm^2 = 30, 0
and 7 -- one exact zero, the second), takes three RK4 steps and compares both time levels of every tracer and the dycore after each.
Reverse cases record the steps on a tracer tape, seed every tracer with its own field, sweep and compare X, G and the kappa / kappa4
densities.  The twin's case is computed once (tv.reference) and shared.  Every test that touches the new calls fails without them."""
import ctypes as C

import numpy as np
import pytest

import moka_hip as mk
import tracer_cases as tc
import tracer_kgrad_twin as tk
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


def expected_path(K, variant=0):
    return 0 if K < 2 else 1 if tv.tile_columns(K, variant == 3) else 2


def model(backend, meshname, K, mode="linear", partial=False, variant=0, **kw):
    mlt = tv.column_mlt(tc.get_mesh(meshname), K) if partial == "floor" else None
    return tc.Model(backend, meshname, K, mode=mode, partial=partial is True, variant=variant, mlt=mlt, **kw)


def check_step(tr_, Prog, ref):
    for j in range(len(ref[1])):
        a, b = tr_.get(j), tr_.get(j, 0)
        assert same(a, ref[1][j]), ("current", j, float(np.nanmax(np.abs(a - ref[1][j]))))
        assert same(b, ref[0][j]), ("previous", j)
    tc.check_dycore(Prog, ref)


def forward(backend, meshname, K, nT=3, mode="linear", partial=False, variant=0, diff=False, bih=False, srcs=(), use_run=False,
            nsteps=NSTEPS, fields=None, fill=None, **kw):
    ref = tv.reference(meshname, K, mode, partial, nT, nsteps, True, diff, bih, srcs, fields=fields, fill=fill)
    md = model(backend, meshname, K, mode, partial, variant, **kw)
    try:
        src = [ref["sources"][j] for j in range(nT)] if srcs else None
        tr_ = mk.set_tracers(md.Prog, ref["fields"], diffusivity=ref["kappa"] if diff else None, sources=src,
                             biharmonic=ref["kappa4"] if bih else None, vertical=ref["kappaV"])
        assert tr_.vmix_path() == 0
        assert np.array_equal(tr_.vertical_diffusivity(), ref["kappaV"])
        if use_run:
            md.run(nsteps)
            check_step(tr_, md.Prog, ref["forward"][-1])
        else:
            for s in range(nsteps):
                md.eager(1)
                check_step(tr_, md.Prog, ref["forward"][s])
        assert tr_.vmix_path() == expected_path(K, variant)
        return [tr_.get(j) for j in range(nT)], ref
    finally:
        md.close()


# ---- forward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 34, 60, 64, 65])
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_levels_and_forms(backend, K, variant):
    """K = 2: one interface, only the two end rows.  K = 3: the first interior row.  K = 34 .. 65: tiles of 32 columns (K = 2, 3: of 64),
    360 cells: the last tile is short.  Variant 3 takes the column form; both forms give the twin's bits, hence each other's."""
    forward(backend, "planar", K, variant=variant)


@pytest.mark.parametrize("meshname,K", [("tiny-4-4", 60), ("tiny-4-4", 5), ("ico12f", 5), ("ico12f", 34)])
def test_meshes(backend, meshname, K):
    """16 cells: fewer columns than a tile.  ico12f: pentagons and heptagons, 1442 cells."""
    forward(backend, meshname, K)


@pytest.mark.parametrize("partial", [True, "floor"], ids=["partial_mlt", "sea-floor"])
@pytest.mark.parametrize("K,variant", [(6, 0), (34, 0), (34, 3)])
def test_masks(backend, K, variant, partial):
    """tc.partial_mlt, and a sea floor with columns of depth 0, 1, 2, 3 .. K: columns below two active levels are left alone, the levels
    under the floor are not touched."""
    _, ref = forward(backend, "planar", K, variant=variant, partial=partial)
    if partial == "floor":
        assert set(range(min(K, 4))) <= set(ref["nlev"].tolist())


@pytest.mark.parametrize("mode", ["nonlinear", "del2+del4"])
def test_dycores(backend, mode):
    forward(backend, "planar", 34, mode=mode)


@pytest.mark.parametrize("K", [5, 34])
def test_beside_horizontal_mixing_and_sources(backend, K):
    """kappa, kappa4 and a source beside the vertical term: they act inside the stages, the solve after them."""
    forward(backend, "planar", K, diff=True, bih=True, srcs=(0, 2))


def test_nine_tracers(backend):
    """nine tracers: the tile form takes them one after the other, eight of them mixed."""
    forward(backend, "planar", 34, nT=9)


def test_run_replays_the_pass_from_a_captured_graph(backend):
    forward(backend, "planar", 3, use_run=True, nsteps=9)


def test_one_level_launches_nothing(backend):
    ref = tv.reference("planar", 1, "linear", False, 3, 2)
    md = model(backend, "planar", 1)
    try:
        tr_ = mk.set_tracers(md.Prog, ref["fields"], vertical=ref["kappaV"])
        md.eager(2)
        check_step(tr_, md.Prog, ref["forward"][-1])
        assert tr_.vmix_path() == 0
    finally:
        md.close()


# ---- never-set and zero coefficients ------------------------------------------------------------------------------------------------
def test_zero_coefficients_are_a_state_that_never_set_one(backend):
    ref = tv.reference("planar", 34, "linear", False, 3, 2, vert=False, fields="unit-first")
    out = []
    for setter in (False, True):
        md = model(backend, "planar", 34)
        try:
            tr_ = mk.set_tracers(md.Prog, ref["fields"], vertical=[0.0, 0.0, 0.0] if setter else None)
            md.eager(2)
            check_step(tr_, md.Prog, ref["forward"][-1])
            assert tr_.vmix_path() == 0
            out.append([tr_.get(j) for j in range(3)])
        finally:
            md.close()
    assert all(np.array_equal(a, b) for a, b in zip(*out))


def test_unit_tracer_and_the_unmixed_tracer(backend):
    """The unit tracer (kappaV = 30 hm^2 / dt) stays exactly 1.0; tracer 1 (kappaV == 0) has the bits of the run without the term."""
    got, ref = forward(backend, "planar", 34, fields="unit-first")
    assert np.all(got[0] == 1.0)
    plain = tv.reference("planar", 34, "linear", False, 3, NSTEPS, vert=False, fields="unit-first")
    assert np.array_equal(got[1], plain["forward"][-1][1][1])
    assert not np.array_equal(got[2], plain["forward"][-1][1][2])


# ---- poison -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_nan_below_the_floor_never_reaches_an_active_level(backend, variant):
    got, ref = forward(backend, "planar", 34, variant=variant, partial="floor", fill=np.nan)
    finite = tv.reference("planar", 34, "linear", "floor", 3, NSTEPS, fill=7.0)
    live = ~ref["dead"]
    assert ref["dead"].any()
    for j in range(3):
        assert np.all(np.isnan(got[j][ref["dead"]]))
        assert np.array_equal(got[j][live], finite["forward"][-1][1][j][live])


# ---- cell ordering ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{"ordering": L.ORDER_NONE}, {"ordering": L.ORDER_RCM}, {"ordering": L.ORDER_RCB}, {"patch_cells": 24}],
                         ids=["none", "rcm", "rcb", "patch24"])
def test_columns_do_not_know_the_cell_order(backend, kw):
    forward(backend, "planar", 34, partial="floor", **kw)


# ---- the form boundary --------------------------------------------------------------------------------------------------------------
def test_tile_form_gives_way_where_two_tiles_no_longer_fit():
    """3 * 32 * (K | 1) * 8 + 128 bytes twice in 160 KiB: K <= 105."""
    assert [tv.tile_columns(K) for K in (1, 2, 24, 25, 26, 105, 106)] == [0, 64, 64, 64, 32, 32, 0]


@pytest.mark.parametrize("K,path", [(25, 1), (26, 1), (105, 1), (106, 2)])
def test_form_boundaries_on_the_device(backend, K, path):
    assert expected_path(K) == path
    forward(backend, "tiny-4-4", K, nsteps=1)


# ---- reverse ------------------------------------------------------------------------------------------------------------------------
def reverse(backend, meshname, K, mode="linear", partial=False, variant=0, diff=False, bih=False, flags=(), wants=(), nT=3, zero_seed=False):
    ref = tv.reference(meshname, K, mode, partial, nT, NSTEPS, True, diff, bih, (), flags, wants)
    md = model(backend, meshname, K, mode, partial, variant)
    try:
        tr_ = mk.set_tracers(md.Prog, ref["fields"], diffusivity=ref["kappa"] if diff else None,
                             biharmonic=ref["kappa4"] if bih else None, vertical=ref["kappaV"])
        tape = mk.TracerAdjointTape(md.Prog, NSTEPS)
        try:
            for j, bits in flags:
                tape.want_diffusivity_gradient(j, kappa=bool(bits & 1), biharmonic=bool(bits & 2))
            for j in wants:
                tape.want_source_gradient(j)
            assert tape.vmix_path() == 0
            for s in range(NSTEPS):
                tape.step(md.dt)                        # the taped step is the untaped one, bit for bit
                check_step(tr_, md.Prog, ref["forward"][s])
            if zero_seed:
                grad = tape.gradient([None] * nT)
                assert all(np.all(g == 0.0) for g in grad)
                for j in wants:
                    assert np.all(tape.source_gradient(j) == 0.0)
                return None
            grad = tape.gradient(ref["X"])
            assert tape.vmix_path() == expected_path(K, variant)
            for j in range(nT):
                assert np.array_equal(grad[j], ref["grad"][j]), ("X", j, float(np.abs(grad[j] - ref["grad"][j]).max()))
            for j in wants:
                assert np.array_equal(tape.source_gradient(j), ref["G"][j]), ("G", j)
            for j, bits in flags:
                for b, bihf, scalar in ((1, False, tape.diffusivity_gradient), (2, True, tape.biharmonic_gradient)):
                    if bits & b:
                        w = tape.diffusivity_density(j, biharmonic=bihf)
                        assert np.array_equal(w, ref["W"][j][b - 1]), ("density", j, b)
                        assert scalar(j) == tk.host_sum(ref["W"][j][b - 1])
            return grad, [tr_.get(j) for j in range(nT)], ref
        finally:
            tape.close()
    finally:
        md.close()


@pytest.mark.parametrize("K", [2, 3, 34, 60, 65])
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_reverse_levels_and_forms(backend, K, variant):
    reverse(backend, "planar", K, variant=variant)


@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_reverse_under_a_sea_floor_with_every_gradient(backend, variant):
    """X, G of tracer 2 and the kappa / kappa4 densities of tracers 0 and 2 beside the vertical term, over columns of every depth."""
    reverse(backend, "planar", 34, variant=variant, partial="floor", diff=True, bih=True, flags=((0, 3), (2, 3)), wants=(2,))


def test_reverse_on_a_mesh_smaller_than_a_tile(backend):
    reverse(backend, "tiny-4-4", 60, wants=(0,))


def test_zero_seed_gives_zeros(backend):
    reverse(backend, "planar", 34, wants=(0, 1), zero_seed=True)


def test_asking_for_gradients_changes_no_bit_of_x(backend):
    a = reverse(backend, "planar", 6, diff=True, bih=True)[0]
    b = reverse(backend, "planar", 6, diff=True, bih=True, flags=((0, 3),), wants=(1, 2))[0]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_dot_product_identity_on_device_outputs(backend):
    """<X_N, phi_N> = <X_0, phi_0> for the linear map phi_0 -> phi_N (no sources), on what the device returned, within the twin chain's
    bound of the RK4 step (tracer_biharmonic_twin.C_STEP_B per step on sum |X| W, W <= max |phi| as S is row-stochastic) plus, per
    step and direction, the forward-error bound of the solve: C_BR (1 + 2 * 4 * 30) for s / hm^2 <= 30 (|A^-1| |A| <= 1 + 8 s / hm^2)."""
    import tracer_biharmonic_twin as tb
    grad, phiN, ref = reverse(backend, "planar", 34)
    for j in range(3):
        lhs = tk.host_sum((ref["X"][j] * phiN[j]).ravel())
        rhs = tk.host_sum((grad[j] * ref["fields"][j]).ravel())
        scale = float(np.abs(ref["X"][j]).sum()) * 1.5
        bound = NSTEPS * (tb.C_STEP_B + 2 * tv.C_BR * (1 + 8 * 30)) * 2.0 ** -53 * scale
        print(f"tracer {j}: <X_N, phi_N> = {lhs:.17g}, <X_0, phi_0> = {rhs:.17g}, difference {abs(lhs - rhs):.3e}, bound {bound:.3e}")
        assert abs(lhs - rhs) <= bound


# ---- interface ----------------------------------------------------------------------------------------------------------------------
def test_interface(backend):
    md = model(backend, "planar", 6)
    lib, h = L.lib(), md.Prog._state._h
    try:
        three = (C.c_double * 3)(1.0, 2.0, 3.0)
        assert lib.moka_set_tracer_vertical_diffusion(h, three) == L.ERR_ARG          # no tracers
        assert lib.moka_set_tracer_vertical_diffusion(h, None) == 0
        f = tc.distinct_fields(md.mesh, 6, 3)
        tr_ = mk.set_tracers(md.Prog, f, vertical=[1.0, 0.0, 3.0])
        for bad in (-1.0, np.nan, np.inf):
            with pytest.raises(mk.MokaError):
                tr_.set_vertical_diffusivity([1.0, bad, 2.0])
            assert np.array_equal(tr_.vertical_diffusivity(), [1.0, 0.0, 3.0])        # nothing changed
        v = C.c_double()
        assert lib.moka_tracer_vertical_diffusion(h, 3, C.byref(v)) == L.ERR_ARG
        assert lib.moka_tracer_vertical_diffusion(h, -1, C.byref(v)) == L.ERR_ARG
        # dt < 0 is refused before any launch while some kappaV != 0 ...
        before = [tr_.get(j) for j in range(3)]
        assert lib.moka_step_rk4(h, -md.dt) == L.ERR_ARG
        assert lib.moka_run(h, 1, -md.dt, 3, 0) == L.ERR_ARG
        tape = mk.TracerAdjointTape(md.Prog, 2)
        assert lib.moka_step_rk4_tracer_taped(tape._h, -md.dt) == L.ERR_ARG and tape.steps() == 0
        tape.close()
        assert all(np.array_equal(tr_.get(j), b) for j, b in enumerate(before)) and tr_.vmix_path() == 0
        # ... and allowed once every value is zero
        tr_.set_vertical_diffusivity(None)
        assert np.array_equal(tr_.vertical_diffusivity(), [0.0, 0.0, 0.0])
        assert lib.moka_step_rk4(h, -md.dt) == 0 and tr_.vmix_path() == 0
        # dt == 0.0 launches nothing
        tr_.set_vertical_diffusivity(2.0)
        assert np.array_equal(tr_.vertical_diffusivity(), [2.0, 2.0, 2.0])
        assert lib.moka_step_rk4(h, 0.0) == 0 and tr_.vmix_path() == 0
        md.eager(1)
        assert tr_.vmix_path() == 1
        # moka_set_tracers resets every value
        tr_ = mk.set_tracers(md.Prog, f[:2])
        assert np.array_equal(tr_.vertical_diffusivity(), [0.0, 0.0]) and tr_.vmix_path() == 0
        assert lib.moka_state_tracer_vmix_path(None) == 0 and lib.moka_tracer_adjoint_vmix_path(None) == 0
    finally:
        md.close()
