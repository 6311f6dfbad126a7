"""Reverse mode through the quadratic bottom drag on the device (moka_forced_tape_create_quadratic; csrc/momentum_vmix.hip: the QD
instances of k_mvadj_tile / k_mvadj_column and k_mvadj_bottom_speed): XU, XH, every density and every scalar gradient bit for bit
against the numpy twin of tests/quadratic_adjoint_twin.py, and the forward state and bottom speed of every recorded step against
quadratic_drag_twin's pass behind the oracle's RK4 step.

A case is a plan, one entry per recorded step: switches "cd", "cd2" (half of it), "nu", "drag", "field" joined by "+"; one stress for
the whole tape; the old gradient flags (`want`), the flag of D_cd and -- with a field -- of DF; a mask; a seed (None: d sum(ssh^2));
poison.  The coefficients are momentum_vmix_twin's and quadratic_drag_twin.cd_of.  Every test fails without the feature: the entry
points do not exist there."""
import ctypes as C

import numpy as np
import pytest

import moka_hip as mk
import momentum_vfield_twin as mf
import momentum_vmix_twin as mv
import poison_cases as pc
import quadratic_adjoint_twin as qa
import quadratic_drag_twin as qd
import test_gpu_forced_adjoint as tga
import tracer_cases as tc
from moka_hip import lib as L

pytestmark = pytest.mark.gpu
ALL = "cd+nu+drag"
FULL = ((ALL, 1.0),) * 2
_REFS = {}


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)
    yield b
    b.close()


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def depths(meshname, K, mask):
    mlt = tga.mask_of(meshname, K, mask)
    return np.full(tc.get_mesh(meshname).nEdges, K, dtype=np.int32) if mlt is None else mlt


def settings(meshname, K, what, mask):
    """(nuV, r, Cd, field) of a switch combination."""
    nu, r = mv.coefficients(meshname, K)
    parts = what.split("+") if what else []
    cd = qd.cd_of(K, tc.dt_of(meshname)) * (1.0 if "cd" in parts else 0.5 if "cd2" in parts else 0.0)
    fld = mf.case_field(meshname, K, depths(meshname, K, mask)) if "field" in parts else None
    return (nu if "nu" in parts else 0.0), (r if "drag" in parts else 0.0), cd, fld


def reference(meshname, K, plan=FULL, stress="stress", want=7, want_cd=True, mask=False, seed=None, poison=False):
    want_field = any("field" in what for what, _ in plan) and want_cd
    key = (meshname, K, tuple(plan), stress, want, want_cd, mask, seed, poison)
    if key not in _REFS:
        om = tc.oracle_mesh(meshname, K, False, tga.mask_of(meshname, K, mask))
        ssh, u, h, _ = tga.start_state(meshname, K, mask, poison)
        tw = qa.QuadraticForcedTwin(om, ssh, u, h, want, want_field, want_cd)
        tw.tau = tga.stress_of(meshname, K, stress)
        fwd = []
        for what, f in plan:
            tw.nu, tw.drag, tw.cd, tw.fld = settings(meshname, K, what, mask)
            tw.step(f * tc.dt_of(meshname))
            fwd.append((tw.st.u[1].copy(), tw.st.h[1].copy(), tw.st.ssh[1].copy(), tw.sps[-1].copy()))
        X0 = tw.seed_sum_sq_ssh() if seed is None else tga.seed_of(meshname, K, mask, seed, poison)
        XU, XH = tw.sweep(*X0)
        _REFS[key] = {"forward": fwd, "XU": XU, "XH": XH, "grad": tw.gradients(), "dens": {b: d.copy() for b, d in tw.dens.items()},
                      "DF": None if tw.DF is None else tw.DF.copy(), "want_field": want_field}
    return _REFS[key]


def switch(md, meshname, what, mask):
    lib, sh, ctx = L.lib(), md.Prog._state._h, md.backend._h
    nu, r, cd, fld = settings(meshname, md.K, what, mask)
    L.check(lib.moka_set_vertical_viscosity(sh, nu, r), ctx)
    L.check(lib.moka_set_quadratic_bottom_drag(sh, cd), ctx)
    L.check(lib.moka_vertical_viscosity_field_upload(sh, None if fld is None else L.f64(fld)), ctx)


def record(md, tape, meshname, plan, mask, ref=None):
    for s, (what, f) in enumerate(plan):
        switch(md, meshname, what, mask)
        tape.step(f * md.dt)
        if ref is not None:
            a = md.Prog.normalVelocity[-1].get()
            assert pc.same(a, ref["forward"][s][0]), ("normalVelocity", s, pc.differences(a, ref["forward"][s][0]))
            assert np.array_equal(md.Prog.layerThickness[-1].get(), ref["forward"][s][1])
            assert np.array_equal(md.Prog.ssh[-1].get(), ref["forward"][s][2])
            assert np.array_equal(mk.last_bottom_speed(md.Prog), ref["forward"][s][3]), ("bottom speed", s)


def compare(tape, g, ref, want, want_cd):
    assert pc.same(g["normalVelocity"], ref["XU"]), ("XU", pc.differences(g["normalVelocity"], ref["XU"]))
    assert pc.same(g["layerThickness"], ref["XH"]), ("XH", pc.differences(g["layerThickness"], ref["XH"]))
    for bit, name in ((1, "surfaceStress"), (2, "viscosity"), (4, "bottomDrag"), (qa.QUADRATIC, "quadraticDrag")):
        flagged = want_cd if bit == qa.QUADRATIC else bool(want & bit)
        assert (name in g) == flagged
        if flagged:
            d = tape.density(name)
            assert pc.same(d, ref["dens"][bit]), (name, pc.differences(d, ref["dens"][bit]))
            if bit == 1:
                assert np.array_equal(g[name], d)
            else:
                assert g[name] == ref["grad"][name] and g[name] == tga.fa.host_sum(d)
    if ref["want_field"]:
        assert pc.same(g["viscosityField"], ref["DF"]), ("DF", pc.differences(g["viscosityField"], ref["DF"]))


def device(backend, meshname, K, plan=FULL, stress="stress", want=7, want_cd=True, mask=False, seed=None, poison=False, variant=0):
    """Runs the case on the device and compares everything with the twin; returns (gradient dict, path, device arrays of the tape)."""
    ref = reference(meshname, K, plan, stress, want, want_cd, mask, seed, poison)
    md = tc.Model(backend, meshname, K, mlt=tga.mask_of(meshname, K, mask), variant=variant, state=tga.start_state(meshname, K, mask, poison))
    try:
        mk.set_vertical_mixing(md.Prog, surface_stress=tga.stress_of(meshname, K, stress))
        tape = mk.ForcedAdjointTape(md.Prog, len(plan), quadratic_drag=True)
        try:
            tape.want_gradient(stress=bool(want & 1), viscosity=bool(want & 2), drag=bool(want & 4), viscosity_field=ref["want_field"],
                               quadratic_drag=want_cd)
            record(md, tape, meshname, plan, mask, ref)
            arrays = tape.device_arrays()
            g = tape.gradient(None if seed is None else tga.seed_of(meshname, K, mask, seed, poison))
            compare(tape, g, ref, want, want_cd)
            return g, tape.vmix_path(), arrays
        finally:
            tape.close()
    finally:
        md.close()


# ---- forms and tiles ----------------------------------------------------------------------------------------------------------------
def five_set_boundaries():
    k64 = max(K for K in range(2, 300) if tga.tile_columns(K, sets=5) == 64)
    k32 = max(K for K in range(2, 300) if tga.tile_columns(K, sets=5) == 32)
    return [k64, k64 + 1, k32, k32 + 1]


FORMS = [(K, False, 0) for K in tga.boundaries()] + [(K, True, 0) for K in five_set_boundaries()] + [(8, False, 3), (8, True, 3), (1, False, 0), (2, False, 0)]


@pytest.mark.parametrize("K,field,variant", FORMS)
def test_forms_and_tiles(backend, K, field, variant):
    """1080 edges: the last tile is short.  Both sides of 19 / 20 and 79 / 80 with four column sets, of 15 / 16 and 63 / 64 with the
    field's fifth; kernel variant 3: the column form at K = 8; K = 1: the n == 1 row alone; K = 2."""
    assert [tga.tile_columns(k) for k in tga.boundaries()] == [64, 32, 32, 0]
    assert [tga.tile_columns(k, sets=5) for k in five_set_boundaries()] == [64, 32, 32, 0]
    what = "cd+field+drag" if field else ALL
    g, path, _ = device(backend, "planar", K, plan=((what, 1.0),) * 2, variant=variant)
    assert path == (1 if tga.tile_columns(K, variant == 3, 5 if field else 4) else 2)
    assert g["quadraticDrag"] != 0.0 and g["bottomDrag"] != 0.0


# ---- switch products ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [True, False], ids=["flags", "noflags"])
@pytest.mark.parametrize("visc", ["nu", "field", ""])
@pytest.mark.parametrize("drag", [True, False], ids=["r", "r0"])
@pytest.mark.parametrize("stress", [None, "stress"])
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_switch_products(backend, variant, stress, drag, visc, flags):
    """Partial columns, so that the drag lines meet n == 1: QD with and without the stress, the field, r, the flags, in both forms."""
    what = "+".join(p for p in ("cd", visc, "drag" if drag else "") if p)
    g, path, _ = device(backend, "planar", 6, plan=((what, 1.0),) * 2, stress=stress, want=7 if flags else 0, want_cd=flags, mask=True,
                        variant=variant)
    assert path == (2 if variant == 3 else 1)


@pytest.mark.parametrize("visc", ["nu", "field"])
@pytest.mark.parametrize("drag", [True, False], ids=["r", "r0"])
@pytest.mark.parametrize("stress", [None, "stress"])
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_derivative_at_zero_instances(backend, variant, stress, drag, visc):
    """Cd == 0 in both steps with the flag set: sp comes from the launch into the tape's record, the density is the derivative at
    zero (r == 0: the instances with the density and without the drag lines), no M, and X has the bits of the same steps unflagged."""
    what = "+".join(p for p in (visc, "drag" if drag else "") if p)
    g, _, arrays = device(backend, "planar", 6, plan=((what, 1.0),) * 2, stress=stress, mask=True, variant=variant)
    assert g["quadraticDrag"] != 0.0
    plain, _, fewer = device(backend, "planar", 6, plan=((what, 1.0),) * 2, stress=stress, want=0, want_cd=False, mask=True, variant=variant)
    assert np.array_equal(g["normalVelocity"], plain["normalVelocity"]) and np.array_equal(g["layerThickness"], plain["layerThickness"])
    # D_cd and spRec, the three old densities, and with a field DF: never usRec or M
    assert arrays - fewer == 2 + 3 + (1 if visc == "field" else 0)


# ---- masks and poison ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
@pytest.mark.parametrize("meshname,K,mask", [("planar", 6, "basin"), ("planar", 34, "basin"), ("ico12f", 5, True)])
def test_masks_and_nan_below_every_floor(backend, meshname, K, mask, variant):
    """Pentagons and heptagons with empty slots (ico12f), neighbours whose bottom levels differ -- some deeper than the target's
    column, so that the skip test fires, some above its bottom --, NaN below every floor in the state (hence in un and us) and in the
    free seed: no NaN reaches an active value, and the active values have the bits of the unpoisoned case."""
    mesh, mlt = tc.get_mesh(meshname), depths(meshname, K, mask)
    deeper, shallower = qa.neighbour_levels(mesh, mlt, K)
    assert deeper.any() and shallower.any()
    if meshname == "ico12f":
        nec = np.asarray(mesh.nEdgesOnCell)
        assert (nec == 5).any() and (nec == 7).any()
    g, _, _ = device(backend, meshname, K, mask=mask, seed=17, poison=True, variant=variant)
    live, livec = pc.active(mesh, mlt, K, "edge"), pc.active(mesh, mlt, K, "cell")
    assert np.all(np.isfinite(g["normalVelocity"][live])) and np.all(np.isnan(g["normalVelocity"][~live]))
    assert np.all(np.isfinite(g["layerThickness"][livec])) and np.all(np.isfinite(g["surfaceStress"]))
    assert all(np.isfinite(g[k]) for k in ("viscosity", "bottomDrag", "quadraticDrag"))
    clean = reference(meshname, K, mask=mask, seed=17)
    assert np.array_equal(g["normalVelocity"][live], clean["XU"][live]) and np.array_equal(g["layerThickness"][livec], clean["XH"][livec])
    assert g["quadraticDrag"] == clean["grad"]["quadraticDrag"]


@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_periodic_tiny_mesh_odd_levels(backend, variant):
    """tiny-4-4, K = 5: an edge's two cells share neighbours (an edge sits in several slots of one lane), 48 edges are fewer than a
    tile, and with odd K the spans are unaligned."""
    device(backend, "tiny-4-4", 5, variant=variant)
    device(backend, "tiny-4-4", 5, seed=29, want=0, want_cd=False, variant=variant)


# ---- values changed between steps ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", [((ALL, 1.0), ("cd2+nu", 1.0)), (("nu+drag", 1.0), (ALL, 1.0)), ((ALL, 1.0), ("nu", 1.0)),
                                  (("cd+field", 1.0), ("cd2+nu+drag", 1.0)), ((ALL, 1.0), (ALL, 0.0), ("cd2", 1.0))],
                         ids=["cd-changes", "cd-zero-first", "cd-zero-last", "field-then-scalar", "dt-zero"])
@pytest.mark.parametrize("want_cd", [True, False], ids=["flag", "noflag"])
def test_coefficients_changed_between_steps(backend, plan, want_cd):
    """Cd is recorded per step; a step with Cd == 0 beside one with Cd != 0, with the flag (its sp is recorded by a launch of its own
    and it launches no chain kernel) and without; a step with dt == 0 is skipped both ways."""
    device(backend, "planar", 6, plan=plan, want=7 if want_cd else 0, want_cd=want_cd, mask=True)


# ---- determinism --------------------------------------------------------------------------------------------------------------------
def test_two_sweeps_of_the_same_contents_give_the_same_bits(backend):
    meshname, K, mask = "planar", 6, "basin"
    ref = reference(meshname, K, mask=mask)
    md = tc.Model(backend, meshname, K, mlt=tga.mask_of(meshname, K, mask))
    lib, sh, ctx = L.lib(), md.Prog._state._h, md.backend._h
    try:
        mk.set_vertical_mixing(md.Prog, surface_stress=tga.stress_of(meshname, K, "stress"))
        tape = mk.ForcedAdjointTape(md.Prog, 2, quadratic_drag=True)
        try:
            tape.want_gradient(stress=True, viscosity=True, drag=True, quadratic_drag=True)
            out = []
            for _ in range(2):
                for f, a in ((L.F_SSH, md.ssh), (L.F_NORMAL_VELOCITY, md.u), (L.F_LAYER_THICKNESS, md.h)):
                    L.check(lib.moka_state_upload(sh, f, 1, L.f64(np.ascontiguousarray(a, dtype=np.float64))), ctx)
                record(md, tape, meshname, FULL, mask, ref)
                g = tape.gradient()
                compare(tape, g, ref, 7, True)
                out.append((g, tape.density("quadraticDrag")))
            for name in out[0][0]:
                assert np.array_equal(out[0][0][name], out[1][0][name])
            assert np.array_equal(out[0][1], out[1][1])
        finally:
            tape.close()
    finally:
        md.close()


# ---- refusals and non-interference --------------------------------------------------------------------------------------------------
def test_refusals_and_the_setter(backend):
    md = tc.Model(backend, "planar", 6)
    lib, sh, ctx = L.lib(), md.Prog._state._h, md.backend._h
    cd = qd.cd_of(6, md.dt)
    h, v = C.c_void_p(), C.c_double()
    buf = np.zeros(md.mesh.nEdges)
    try:
        assert lib.moka_forced_tape_create_quadratic(None, 2, C.byref(h)) == L.ERR_ARG
        assert lib.moka_forced_tape_create_quadratic(sh, 2, None) == L.ERR_ARG
        assert lib.moka_forced_tape_create_quadratic(sh, -1, C.byref(h)) == L.ERR_ARG and not h.value
        assert lib.moka_forced_adjoint_want_quadratic_drag_gradient(None, 1) == L.ERR_ARG
        # a plain tape: the flag is unsupported, the setter refuses with the text it always had, no second forced tape of either kind
        plain = mk.ForcedAdjointTape(md.Prog, 2)
        assert lib.moka_forced_adjoint_want_quadratic_drag_gradient(plain._h, 1) == L.ERR_UNSUPPORTED
        assert lib.moka_forced_adjoint_quadratic_drag_density_download(plain._h, L.f64(buf)) == L.ERR_ARG
        assert lib.moka_set_quadratic_bottom_drag(sh, cd) == L.ERR_UNSUPPORTED and b"moka_forced_tape" in lib.moka_last_error(ctx)
        assert lib.moka_forced_tape_create_quadratic(sh, 2, C.byref(h)) == L.ERR_UNSUPPORTED and not h.value
        assert lib.moka_forced_tape_device_arrays(plain._h) == 0 and lib.moka_forced_tape_device_arrays(None) == 0
        plain.close()
        # a quadratic tape: the setter is accepted beside it, before and between recorded steps; a plain one is refused beside it
        # (a state has one forced tape: a plain and a quadratic one never stand together)
        tape = mk.ForcedAdjointTape(md.Prog, 2, quadratic_drag=True)
        th = tape._h
        assert lib.moka_forced_tape_create(sh, 2, C.byref(h)) == L.ERR_UNSUPPORTED and not h.value
        assert lib.moka_forced_tape_create_quadratic(sh, 2, C.byref(h)) == L.ERR_UNSUPPORTED and not h.value
        assert lib.moka_set_quadratic_bottom_drag(sh, cd) == 0 and mk.quadratic_drag(md.Prog) == cd
        assert lib.moka_set_quadratic_bottom_drag(sh, -1.0) == L.ERR_ARG and mk.quadratic_drag(md.Prog) == cd
        assert lib.moka_forced_adjoint_want_gradient(th, 8, 1) == L.ERR_ARG                 # the old call keeps its three bits
        assert lib.moka_forced_adjoint_quadratic_drag_gradient(th, C.byref(v)) == L.ERR_ARG   # not flagged
        assert lib.moka_forced_adjoint_quadratic_drag_density_download(th, L.f64(buf)) == L.ERR_ARG
        assert lib.moka_forced_adjoint_want_quadratic_drag_gradient(th, 1) == 0
        assert lib.moka_forced_adjoint_quadratic_drag_gradient(th, C.byref(v)) == 0 and v.value == 0.0
        assert lib.moka_forced_adjoint_quadratic_drag_gradient(th, None) == L.ERR_ARG
        assert lib.moka_forced_adjoint_quadratic_drag_density_download(th, None) == L.ERR_ARG
        assert lib.moka_forced_adjoint_want_quadratic_drag_gradient(th, 0) == 0
        tape.step(md.dt)
        assert lib.moka_forced_adjoint_want_quadratic_drag_gradient(th, 1) == L.ERR_ARG     # a step is recorded
        assert b"no step is recorded" in lib.moka_last_error(ctx)
        assert lib.moka_set_quadratic_bottom_drag(sh, 0.5 * cd) == 0
        tape.step(md.dt)
        tape.gradient()
        assert lib.moka_forced_adjoint_want_quadratic_drag_gradient(th, 1) == 0             # the tape is empty again
        tape.close()
        # Cd is still set: a plain tape refuses the state, as before
        assert lib.moka_forced_tape_create(sh, 2, C.byref(h)) == L.ERR_UNSUPPORTED and b"quadratic" in lib.moka_last_error(ctx)
        assert lib.moka_set_quadratic_bottom_drag(sh, 0.0) == 0
    finally:
        md.close()


def test_unsupported_states_refuse_the_quadratic_tape_too(backend):
    lib, h = L.lib(), C.c_void_p()
    f32 = tc.Model(backend, "ico16", 4, state_bytes=4)
    try:
        assert lib.moka_forced_tape_create_quadratic(f32.Prog._state._h, 2, C.byref(h)) == L.ERR_UNSUPPORTED and not h.value
    finally:
        f32.close()
    nl = tc.Model(backend, "planar", 6, mode="nonlinear")
    try:
        assert lib.moka_forced_tape_create_quadratic(nl.Prog._state._h, 2, C.byref(h)) == L.ERR_UNSUPPORTED and not h.value
    finally:
        nl.close()
    md = tc.Model(backend, "planar", 6)
    try:
        t = mk.AdjointTape(md.Prog, 2)
        assert lib.moka_forced_tape_create_quadratic(md.Prog._state._h, 2, C.byref(h)) == L.ERR_UNSUPPORTED and not h.value
        t.close()
        mk.set_tracers(md.Prog, tc.distinct_fields(md.mesh, 6, 1))
        assert lib.moka_forced_tape_create_quadratic(md.Prog._state._h, 2, C.byref(h)) == L.ERR_UNSUPPORTED and not h.value
    finally:
        md.close()


def test_a_plain_tape_next_to_the_new_code_keeps_its_bits(backend):
    """A plain tape on a Cd == 0 state gives the bits of test_gpu_forced_adjoint's reference, in a process that ran the new kernels."""
    device(backend, "planar", 6, mask=True)
    tga.device(backend, "planar", 6, mask=True)


def test_a_quadratic_tape_without_cd_is_a_plain_one(backend):
    """Cd == 0 and no flag: the bits and the vmix_path of a plain tape, and no spRec, usRec or M; with Cd != 0 exactly those three more."""
    plan = (("nu+drag", 1.0),) * 2
    plain, ppath = tga.device(backend, "planar", 6, mask=True)
    g, path, arrays = device(backend, "planar", 6, plan=plan, want=7, want_cd=False, mask=True)
    assert path == ppath
    for name in plain:
        assert np.array_equal(plain[name], g[name])
    md = tc.Model(backend, "planar", 6, mlt=tga.mask_of("planar", 6, True))
    try:
        mk.set_vertical_mixing(md.Prog, surface_stress=tga.stress_of("planar", 6, "stress"))
        t = mk.ForcedAdjointTape(md.Prog, 2)
        t.want_gradient(stress=True, viscosity=True, drag=True)
        record(md, t, "planar", plan, True)
        assert t.device_arrays() == arrays
        t.close()
    finally:
        md.close()
    _, _, more = device(backend, "planar", 6, plan=FULL, want=7, want_cd=False, mask=True)
    assert more == arrays + 3


# ---- destroy order ------------------------------------------------------------------------------------------------------------------
FIELDS = ((L.F_SSH, 1), (L.F_NORMAL_VELOCITY, 5), (L.F_LAYER_THICKNESS, 5))


def new_state(model):
    lib, ctx = L.lib(), model.backend._h
    hS = C.c_void_p()
    L.check(lib.moka_state_create(ctx, model.M._h, C.byref(hS)), ctx)
    for (f, _), a in zip(FIELDS, (model.ssh, model.u, model.h)):
        L.check(lib.moka_state_upload(hS, f, 1, L.f64(np.ascontiguousarray(a, dtype=np.float64))), ctx)
    return hS


def step_and_read(model, hS):
    lib, ctx, mesh = L.lib(), model.backend._h, model.mesh
    L.check(lib.moka_step_rk4(hS, model.dt), ctx)
    out = []
    for (f, k), n in zip(FIELDS, (mesh.nCells, mesh.nEdges, mesh.nCells)):
        a = np.empty((n, k))
        L.check(lib.moka_state_download(hS, f, 1, L.f64(a)), ctx)
        out.append(a)
    return out


@pytest.mark.parametrize("cd_back_to_zero", [False, True], ids=["cd-set", "cd-zeroed"])
@pytest.mark.parametrize("state_first", [False, True], ids=["tape-first", "state-first"])
def test_destroyed_with_steps_still_recorded(backend, state_first, cd_back_to_zero):
    """The tape is destroyed with two steps recorded (sp, u* and M allocated), before or after its state, with Cd still set or set
    back to 0 first; then a fresh state on the same mesh takes one RK4 step and holds what a state that never had a tape holds, and the
    surviving state has its counters back: a plain forced tape is accepted again."""
    model = tc.Model(backend, "tiny-4-4", 5)
    lib, ctx = L.lib(), backend._h
    try:
        untaped = new_state(model)
        ref = step_and_read(model, untaped)
        lib.moka_state_destroy(untaped)
        hS, hT = new_state(model), C.c_void_p()
        L.check(lib.moka_forced_tape_create_quadratic(hS, 2, C.byref(hT)), ctx)
        L.check(lib.moka_forced_adjoint_want_quadratic_drag_gradient(hT, 1), ctx)
        L.check(lib.moka_set_quadratic_bottom_drag(hS, qd.cd_of(5, model.dt)), ctx)
        for _ in range(2):
            L.check(lib.moka_step_rk4_forced_taped(hT, model.dt), ctx)
        assert lib.moka_forced_tape_device_arrays(hT) == 4 + 4          # un, hn, hbar, scratch; D_cd, sp, u*, M
        if cd_back_to_zero:
            L.check(lib.moka_set_quadratic_bottom_drag(hS, 0.0), ctx)
        if state_first:
            lib.moka_state_destroy(hS)
            lib.moka_forced_tape_destroy(hT)
        else:
            lib.moka_forced_tape_destroy(hT)
            if not cd_back_to_zero:
                other = C.c_void_p()
                assert lib.moka_forced_tape_create(hS, 1, C.byref(other)) == L.ERR_UNSUPPORTED     # Cd is still set
                L.check(lib.moka_set_quadratic_bottom_drag(hS, 0.0), ctx)
            other = C.c_void_p()
            L.check(lib.moka_forced_tape_create(hS, 1, C.byref(other)), ctx)
            assert lib.moka_set_quadratic_bottom_drag(hS, 1e-3) == L.ERR_UNSUPPORTED               # ... and it is counted as plain
            lib.moka_forced_tape_destroy(other)
            L.check(lib.moka_set_quadratic_bottom_drag(hS, 1e-3), ctx)
            L.check(lib.moka_set_tracers(hS, 1), ctx)
            lib.moka_state_destroy(hS)
        fresh = new_state(model)
        try:
            for got, want in zip(step_and_read(model, fresh), ref):
                assert np.array_equal(got, want)
        finally:
            lib.moka_state_destroy(fresh)
    finally:
        model.close()
