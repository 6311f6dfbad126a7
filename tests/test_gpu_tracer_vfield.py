"""A vertical diffusivity per interface and cell on the device (csrc/tracer_vmix.hip: the field instances of k_vmix_tile, k_vmix_column
and their gradient kin; moka_tracer_vertical_field_upload / _download, moka_tracer_has_vertical_field; the field copies of
moka_step_rk4_tracer_taped): everything bit for bit against the numpy twin of tests/tracer_vfield_twin.py, through the Python API.

The model: three tracers.  Tracer 0 has a field, random in [0, 2] x the largest of tracer_vmix_twin.kappavs' values, with exact zeros
at a few interfaces (a whole column but its first interface among them) and NaN in the never-read entries; tracer 1 has the scalar 0;
tracer 2 a nonzero scalar.  A case takes three RK4 steps.  The twin's case is computed once (tracer_vfield_twin.reference) and shared.
Every test calls a new entry point, so all of them fail without the feature.

The misaligned cases run on a sheared periodic hex mesh of 7 x 5 = 35 cells (tracer_vfield_twin.sheared_mesh) with an odd K: the tracers
of a state, the records of a tape and the slots of the gradient's arrays then lie an odd number of doubles apart, so every other base is
no multiple of 16 bytes and the staging loop and the write-back take their two-doubles-apart path; a tile's span nEl = ncol * K is odd
as well, so the aligned bases end on a lone double."""
import ctypes as C

import numpy as np
import pytest

import moka_hip as mk
import tracer_cases as tc
import tracer_kgrad_twin as tk
import tracer_vfield_twin as tf
import tracer_vgrad_twin as tg
import tracer_vmix_twin as tv
from moka_hip import lib as L

pytestmark = pytest.mark.gpu
STEP = (("A", None, None), None)
PLAN = (STEP,) * 3
FLAGS = (0, 2)


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)
    yield b
    b.close()


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def expected_path(K, variant=0):
    return 0 if K < 2 else 1 if tv.tile_columns(K, variant == 3) else 2


def expected_grad_path(K, variant=0):
    return 0 if K < 2 else 1 if tg.tile_columns_grad(K, variant == 3) else 2


def model(backend, meshname, K, partial=False, variant=0):
    mlt = tv.column_mlt(tc.get_mesh(meshname), K) if partial == "floor" else None
    return tc.Model(backend, meshname, K, variant=variant, mlt=mlt)


def check_step(tr_, Prog, ref):
    for j in range(len(ref[1])):
        a = tr_.get(j)
        assert same(a, ref[1][j]), ("current", j, float(np.nanmax(np.abs(a - ref[1][j]))))
        assert same(tr_.get(j, 0), ref[0][j]), ("previous", j)
    tc.check_dycore(Prog, ref)


def vertical_of(step):
    """set_tracers' `vertical` of a step of the reference: the field where the tracer has one, else its scalar."""
    fields, kv, _ = step
    return [kv[j] if f is None else f for j, f in enumerate(fields)]


def apply_step(tr_, step):
    fields, kv, _ = step
    tr_.set_vertical_diffusivity(kv)
    for j, f in enumerate(fields):
        tr_.set_vertical_field(j, f)


# ---- forward ------------------------------------------------------------------------------------------------------------------------
def forward(backend, meshname, K, variant=0, partial=False, fill=None):
    ref = tf.reference(meshname, K, partial, PLAN, () if fill is not None else FLAGS, fill=fill, wants=() if fill is not None else (2,))
    md = model(backend, meshname, K, partial, variant)
    try:
        tr_ = mk.set_tracers(md.Prog, ref["fields"], vertical=vertical_of(ref["steps"][0]))
        assert tr_.vmix_path() == 0
        assert same(tr_.vertical_field(0), ref["steps"][0][0][0]) and tr_.vertical_field(1) is None and tr_.vertical_field(2) is None
        assert np.array_equal(tr_.vertical_diffusivity(), [0.0, 0.0, ref["steps"][0][1][2]])
        for s in range(3):
            md.eager(1)
            check_step(tr_, md.Prog, ref["forward"][s])
        assert tr_.vmix_path() == expected_path(K, variant)
        return [tr_.get(j) for j in range(3)], ref
    finally:
        md.close()


@pytest.mark.parametrize("K", [2, 3, 34, 60, 65])
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_forward_levels_and_forms(backend, K, variant):
    """K = 2: one interface.  K = 3: the first interior row.  360 cells: the last tile (64 columns at K = 2, 3; 32 beyond) is short.
    Variant 3 takes the column form; both give the twin's bits."""
    got, ref = forward(backend, "planar", K, variant)
    plain = tv.reference("planar", K, "linear", False, 3, 3)
    assert np.array_equal(got[1], plain["forward"][-1][1][1]) and np.array_equal(got[2], plain["forward"][-1][1][2])
    assert not np.array_equal(got[0], plain["forward"][-1][1][0])


@pytest.mark.parametrize("meshname", ["tiny-4-4", "ico12f"])
def test_forward_meshes(backend, meshname):
    """16 cells: fewer columns than a tile.  ico12f: pentagons and heptagons, 1442 cells."""
    forward(backend, meshname, 5)


@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_forward_under_a_sea_floor(backend, variant):
    """tv.column_mlt: columns of depth 0, 1, 2, 3 .. K, NaN in every tracer level under the floor and in every never-read field entry."""
    got, ref = forward(backend, "planar", 34, variant, partial="floor", fill=np.nan)
    assert {0, 1, 2} <= set(ref["nlev"].tolist()) and ref["dead"].any()
    for j in range(3):
        assert np.all(np.isnan(got[j][ref["dead"]])) and np.isfinite(got[j][~ref["dead"]]).all()


# ---- a uniform field is the scalar ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_uniform_field_against_scalar(backend, variant):
    """K = 60: every tracer's field equal to its scalar at every entry (tracer 1: an all-zero field) gives, step by step, the bits of a
    second state run with the scalars -- which are the scalar twin's."""
    K = 60
    ref = tv.reference("planar", K, "linear", False, 3, 3)
    out = []
    for fields in (False, True):
        md = model(backend, "planar", K, variant=variant)
        try:
            kv = ref["kappaV"]
            vert = [np.full(ref["fields"][0].shape, k) for k in kv] if fields else kv
            tr_ = mk.set_tracers(md.Prog, ref["fields"], vertical=vert)
            assert [tr_.vertical_field(j) is not None for j in range(3)] == [fields] * 3
            for s in range(3):
                md.eager(1)
                check_step(tr_, md.Prog, ref["forward"][s])
            assert tr_.vmix_path() == expected_path(K, variant)
            out.append([tr_.get(j) for j in range(3)])
        finally:
            md.close()
    assert all(np.array_equal(a, b) for a, b in zip(*out))


# ---- reverse and gradient -------------------------------------------------------------------------------------------------------------
def check_density(tape, j, D):
    got = tape.vertical_density(j)
    assert np.array_equal(got, D), ("D", j, float(np.abs(got - D).max()))
    cell, prof, scalar = tg.views(D)
    assert np.array_equal(tape.vertical_density(j, "cell"), cell), ("cell", j)
    assert np.array_equal(tape.vertical_density(j, "profile"), prof), ("profile", j)
    assert tape.vertical_gradient(j) == scalar == tk.host_sum(D.ravel()), ("scalar", j)


def reverse(backend, meshname, K, variant=0, flagged=True):
    ref = tf.reference(meshname, K, False, PLAN, FLAGS, wants=(2,))
    md = model(backend, meshname, K, variant=variant)
    try:
        tr_ = mk.set_tracers(md.Prog, ref["fields"], vertical=vertical_of(ref["steps"][0]))
        tape = mk.TracerAdjointTape(md.Prog, 3)
        try:
            for j in FLAGS if flagged else ():
                tape.want_vertical_gradient(j)
            tape.want_source_gradient(2)
            for s in range(3):
                tape.step(md.dt)
                check_step(tr_, md.Prog, ref["forward"][s])
            grad = tape.gradient(ref["X"])                  # every tracer its own seed
            assert tape.vmix_path() == (expected_grad_path if flagged else expected_path)(K, variant)
            for j in range(3):
                assert np.array_equal(grad[j], ref["grad"][j]), ("X", j, float(np.abs(grad[j] - ref["grad"][j]).max()))
            assert np.array_equal(tape.source_gradient(2), ref["G"][2]), "G"
            for j in FLAGS if flagged else ():
                check_density(tape, j, ref["D"][j])
                assert ref["D"][j].any()
            assert tape.steps() == 0
        finally:
            tape.close()
    finally:
        md.close()


@pytest.mark.parametrize("K", [2, 3, 20, 60, 81])
def test_reverse_and_gradient(backend, K):
    """On either side of both thresholds of the gradient instances (tiles of 64 up to K = 19, of 32 up to 79, the column form beyond;
    the plain instances would still tile at K = 81): X, G of tracer 2, D of tracers 0 and 2 and its three views."""
    reverse(backend, "planar", K)


def test_reverse_and_gradient_column_form(backend):
    reverse(backend, "planar", 20, variant=3)


@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_unflagged_reverse(backend, variant):
    """No tracer flagged: the field instances of the plain reverse pass."""
    reverse(backend, "planar", 60, variant=variant, flagged=False)


# ---- a base that is no multiple of 16 bytes -----------------------------------------------------------------------------------------
def misaligned(backend, K, fields, vflags):
    """Three taped steps and their sweep on the 35-cell mesh; fields = the plan's names per tracer.  The forward steps, X, and D with
    its views, bit for bit."""
    name = tf.sheared_mesh(7, 5)
    assert (35 * K) % 2 == 1
    ref = tf.reference(name, K, False, ((fields, None),) * 3, vflags)
    md = model(backend, name, K)
    try:
        tr_ = mk.set_tracers(md.Prog, ref["fields"], vertical=vertical_of(ref["steps"][0]))
        assert [tr_.vertical_field(j) is not None for j in range(3)] == [f is not None for f in fields]
        tape = mk.TracerAdjointTape(md.Prog, 3)
        try:
            for j in vflags:
                tape.want_vertical_gradient(j)
            for s in range(3):
                tape.step(md.dt)
                check_step(tr_, md.Prog, ref["forward"][s])
            assert tr_.vmix_path() == 1
            grad = tape.gradient(ref["X"])
            assert tape.vmix_path() == 1
            for j in range(3):
                assert np.array_equal(grad[j], ref["grad"][j]), ("X", j, float(np.abs(grad[j] - ref["grad"][j]).max()))
            for j in vflags:
                check_density(tape, j, ref["D"][j])
                assert ref["D"][j].any()
        finally:
            tape.close()
    finally:
        md.close()


@pytest.mark.parametrize("vflags", [(), (1, 2)], ids=["plain", "gradient"])
@pytest.mark.parametrize("K", [5, 33])
def test_misaligned_base(backend, K, vflags):
    """Tracer 0 a scalar (an aligned base, inside the field instances), tracer 1 a field at a base that is 8 modulo 16, tracer 2 a field
    at an aligned base that ends on a lone double.  K = 5: one tile of 35 of 64 columns; K = 33: tiles of 32, the last one of three
    columns.  The second recorded step's thickness and phi_new sit at odd offsets of the tape as well."""
    misaligned(backend, K, (None, "A", "B"), vflags)


@pytest.mark.parametrize("vflags", [(), (0, 1)], ids=["plain", "gradient"])
def test_misaligned_base_scalar_instances(backend, vflags):
    """No field anywhere: the scalar instances on the same bases (tracer 1 has kappaV == 0: with the flag, the derivative at zero)."""
    misaligned(backend, 33, (None, None, None), vflags)


# ---- the field changes between taped steps ------------------------------------------------------------------------------------------
def test_field_changed_between_taped_steps(backend):
    """Field A, field B, then the field removed so that tracer 0's scalar acts; sweep.  Then the tape is recorded again -- field B twice,
    one upload: the second step takes the copy of the first -- and swept: the twin's sweep over those records alone."""
    K = 6
    third = ((None, None, None), None)
    plan = (STEP, (("B", None, None), None), third, (("B", None, None), None), (("B", None, None), None))
    ref = tf.reference("planar", K, False, plan, FLAGS)
    twin = ref["twin"]
    assert twin.tape[2]["fieldV"][0] is None and twin.tape[2]["kappaV"][0] != 0.0
    adj = tf.VfieldAdjointTwin(twin)
    halves = [adj.sweep_vgrad(twin.tape[a:b], [x.copy() for x in ref["X"]], FLAGS) for a, b in ((0, 3), (3, 5))]
    md = model(backend, "planar", K)
    try:
        tr_ = mk.set_tracers(md.Prog, ref["fields"])
        tape = mk.TracerAdjointTape(md.Prog, 3)
        try:
            for j in FLAGS:
                tape.want_vertical_gradient(j)
            s = 0
            for (a, b), exp in zip(((0, 3), (3, 5)), halves):
                for s in range(a, b):
                    if s != 4:
                        apply_step(tr_, ref["steps"][s])
                    tape.step(md.dt)
                    check_step(tr_, md.Prog, ref["forward"][s])
                grad = tape.gradient(ref["X"])
                for j in range(3):
                    assert np.array_equal(grad[j], exp[0][j]), ("X", a, j)
                for j in FLAGS:
                    check_density(tape, j, exp[3][j])
                assert tape.steps() == 0
            assert not np.array_equal(halves[0][3][0], halves[1][3][0])
        finally:
            tape.close()
    finally:
        md.close()


# ---- states without a field ---------------------------------------------------------------------------------------------------------
def test_no_field_anywhere(backend):
    md = model(backend, "planar", 6)
    lib, h = L.lib(), md.Prog._state._h
    try:
        f = tc.distinct_fields(md.mesh, 6, 3)
        tr_ = mk.set_tracers(md.Prog, f, vertical=[1.0, 0.0, 3.0])
        v, buf = C.c_int(7), np.full((md.mesh.nCells, 6), 7.0)
        for j in range(3):
            assert lib.moka_tracer_has_vertical_field(h, j, C.byref(v)) == 0 and v.value == 0
            assert lib.moka_tracer_vertical_field_download(h, j, L.f64(buf)) == 0 and not buf.any()
            buf[:] = 7.0
            assert tr_.vertical_field(j) is None
    finally:
        md.close()


def test_upload_then_remove_is_a_state_that_never_had_a_field(backend):
    """A state that uploads its only field and removes it again, then steps: the bits of a state that never had one (the scalar twin's)."""
    ref = tv.reference("planar", 34, "linear", False, 3, 3)
    out = []
    for touch in (False, True):
        md = model(backend, "planar", 34)
        try:
            tr_ = mk.set_tracers(md.Prog, ref["fields"], vertical=ref["kappaV"])
            if touch:
                tr_.set_vertical_field(0, tf.case_field("planar", 34, ref["nlev"]))
                assert tr_.vertical_field(0) is not None
                tr_.set_vertical_field(0, None)
                assert tr_.vertical_field(0) is None
            for s in range(3):
                md.eager(1)
                check_step(tr_, md.Prog, ref["forward"][s])
            assert tr_.vmix_path() == 1
            out.append([tr_.get(j) for j in range(3)])
        finally:
            md.close()
    assert all(np.array_equal(a, b) for a, b in zip(*out))


# ---- the interface ------------------------------------------------------------------------------------------------------------------
def test_interface(backend):
    K = 6
    md = model(backend, "planar", K, partial="floor")
    lib, h = L.lib(), md.Prog._state._h
    nC = md.mesh.nCells
    try:
        ok = np.full((nC, K), 2.0)
        v = C.c_int(7)
        assert lib.moka_tracer_vertical_field_upload(h, 0, L.f64(ok)) == L.ERR_ARG                  # no tracers
        assert lib.moka_tracer_vertical_field_upload(None, 0, L.f64(ok)) == L.ERR_ARG
        f = tc.distinct_fields(md.mesh, K, 3)
        tr_ = mk.set_tracers(md.Prog, f, vertical=[1.0, 0.0, 3.0])
        nlev = tv.vmix_twin("planar", K, mlt=tv.column_mlt(md.mesh, K)).nlev(K)
        for j in (-1, 3):
            assert lib.moka_tracer_vertical_field_upload(h, j, L.f64(ok)) == L.ERR_ARG
            assert lib.moka_tracer_vertical_field_download(h, j, L.f64(ok)) == L.ERR_ARG
            assert lib.moka_tracer_has_vertical_field(h, j, C.byref(v)) == L.ERR_ARG
        assert lib.moka_tracer_vertical_field_download(h, 0, None) == L.ERR_ARG and lib.moka_tracer_has_vertical_field(h, 0, None) == L.ERR_ARG
        deep = int(np.nonzero(nlev == K)[0][0])
        tr_.set_vertical_field(0, ok)
        for bad in (-1.0, np.nan, np.inf):
            g = ok.copy()
            g[deep, K - 2] = bad                            # the last active interface of a full column
            with pytest.raises(mk.MokaError):
                tr_.set_vertical_field(0, g)
            with pytest.raises(mk.MokaError):
                tr_.set_vertical_field(1, g)
            assert np.array_equal(tr_.vertical_field(0), ok) and tr_.vertical_field(1) is None       # nothing changed
            g = ok.copy()
            g[np.arange(K)[None, :] >= (nlev - 1)[:, None]] = bad                                    # never inspected, returned as uploaded
            tr_.set_vertical_field(1, g)
            assert same(tr_.vertical_field(1), g)
            tr_.set_vertical_field(1, None)
        with pytest.raises(ValueError):
            tr_.set_vertical_field(0, np.zeros(K + 1))
        # profiles: K or K - 1 values for every cell
        prof = np.linspace(1.0, 2.0, K - 1)
        tr_.set_vertical_field(2, prof)
        assert np.array_equal(tr_.vertical_field(2)[:, :K - 1], np.broadcast_to(prof, (nC, K - 1)))
        tr_.set_vertical_field(2, np.append(prof, 5.0))
        assert np.all(tr_.vertical_field(2)[:, K - 1] == 5.0)
        tr_.set_vertical_field(2, None)
        # the pass is on through a field alone: dt < 0 is refused, every scalar zero; an all-zero field switches it off again
        tr_.set_vertical_diffusivity(None)
        assert lib.moka_step_rk4(h, -md.dt) == L.ERR_ARG and lib.moka_run(h, 1, -md.dt, 3, 0) == L.ERR_ARG
        tape = mk.TracerAdjointTape(md.Prog, 2)
        assert lib.moka_step_rk4_tracer_taped(tape._h, -md.dt) == L.ERR_ARG and tape.steps() == 0
        tape.close()
        assert tr_.vmix_path() == 0
        assert lib.moka_step_rk4(h, 0.0) == 0 and tr_.vmix_path() == 0                              # dt == 0.0 launches nothing
        tr_.set_vertical_field(0, np.zeros((nC, K)))
        assert tr_.vertical_field(0) is not None and lib.moka_step_rk4(h, -md.dt) == 0 and tr_.vmix_path() == 0
        tr_.set_vertical_diffusivity([5.0, 0.0, 0.0])                                               # ... whatever tracer 0's scalar
        assert lib.moka_step_rk4(h, -md.dt) == 0 and tr_.vmix_path() == 0
        tr_.set_vertical_field(0, None)                                                              # the scalar acts again
        assert lib.moka_step_rk4(h, -md.dt) == L.ERR_ARG
        md.eager(1)
        assert tr_.vmix_path() == 1
        # moka_set_tracers frees every field
        tr_.set_vertical_field(1, ok)
        tr_ = mk.set_tracers(md.Prog, f[:2])
        assert tr_.vertical_field(0) is None and tr_.vertical_field(1) is None and tr_.vmix_path() == 0
    finally:
        md.close()
