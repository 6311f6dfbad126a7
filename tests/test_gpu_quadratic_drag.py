"""The quadratic bottom drag on the device (csrc/momentum_vmix.hip: k_mvmix_bottom_speed and the QD instances of k_mvmix_tile and
k_mvmix_column; the two launches behind stage 4 of step_rk4; moka_set_quadratic_bottom_drag, moka_bottom_speed,
moka_bottom_speed_download): everything bit for bit against the numpy twin of tests/quadratic_drag_twin.py, through tc.check_dycore
after each of three RK4 steps.

A case names, per step, the switches in force: "cd", "nu", "drag", "stress", "field" (momentum_vfield_twin.case_field), joined by "+";
"" switches the pass off.  The coefficients are mv.coefficients, mv.stress_field and qd.cd_of.  The twin's case is computed once and
shared.  The square root has assertions of its own (moka_bottom_speed against the twin's bottom_speed): a failure of the pass can be
told from a failure of the square root.  Every test that touches a new call fails without the feature with a missing symbol; the
cd == 0 cases are the ones that pass there."""
import ctypes as C

import numpy as np
import pytest

import moka_hip as mk
import momentum_vfield_twin as mf
import momentum_vmix_twin as mv
import oracle as orc
import poison_cases as pc
import quadratic_drag_twin as qd
import tracer_cases as tc
from del4_twin import TwinState
from moka_hip import lib as L

pytestmark = pytest.mark.gpu
NSTEPS = 3
COMBOS = ("cd", "cd+drag", "cd+nu+stress", "cd+nu+drag+stress", "cd+field")
ALL = "cd+nu+drag+stress"
_REFS = {}


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)
    yield b
    b.close()


def mask_of(meshname, K, mask):
    """mask: False (full columns: None), True (tc.partial_mlt) or "basin" (poison_cases.mask_of)."""
    return None if not mask else pc.mask_of(meshname, K) if mask == "basin" else tc.partial_mlt(tc.get_mesh(meshname), K)


def depths(meshname, K, mask):
    mlt = mask_of(meshname, K, mask)
    return np.full(tc.get_mesh(meshname).nEdges, K, dtype=np.int32) if mlt is None else mlt


def settings(meshname, K, what, mask=False):
    """(nuV, r, tau, cd, field) of a switch combination."""
    nu, r = mv.coefficients(meshname, K)
    parts = what.split("+") if what else []
    tau = mv.stress_field(tc.get_mesh(meshname), K) if "stress" in parts else None
    fld = mf.case_field(meshname, K, depths(meshname, K, mask)) if "field" in parts else None
    return (nu if "nu" in parts else 0.0), (r if "drag" in parts else 0.0), tau, (qd.cd_of(K, tc.dt_of(meshname)) if "cd" in parts else 0.0), fld


def start_state(meshname, K, mask, poison):
    """(ssh, u, h, rest) of the case; poison: u is NaN on the linear dycore's set (poison_cases.edge_poison, one ring) over the mask."""
    ssh, u, h, rest = tc.state_of(meshname, K)
    if poison:
        u = pc.put(u, pc.edge_poison(tc.get_mesh(meshname), depths(meshname, K, mask), K, 1), "nan")
    return ssh, u, h, rest


def reference(meshname, K, plan, mode="linear", mask=False, poison=False, s13=False):
    """The twin's ((None, None, u, h, ssh), sp) after every step of `plan` (one switch combination per step), computed once and shared."""
    key = (meshname, K, tuple(plan), mode, mask, poison, s13)
    if key not in _REFS:
        ssh, u, h, _ = start_state(meshname, K, mask, poison)
        tw = qd.quadratic_twin(meshname, K, "linear" if s13 else mode, mlt=mask_of(meshname, K, mask))
        out = []
        if s13:
            om = tw.mt.tw.om
            st, nl = orc.OracleState(om, ssh, u, h), (orc.OracleNonlinear(om) if mode == "nonlinear" else None)
        else:
            st, phis = TwinState(ssh, u, h), [[], []]
        for what in plan:
            tw.mt.nu, tw.mt.drag, tw.mt.tau, tw.cd, tw.fld = settings(meshname, K, what, mask)
            if s13:
                tw.step_s13(st, tc.dt_of(meshname), nl)
            else:
                tw.step_rk4(st, phis, tc.dt_of(meshname))
            out.append(((None, None, st.u[1].copy(), st.h[1].copy(), st.ssh[1].copy()), tw.sp.copy()))
        _REFS[key] = out
    return _REFS[key]


def switch(md, meshname, what, mask=False):
    nu, r, tau, cd, fld = settings(meshname, md.K, what, mask)
    mk.set_vertical_mixing(md.Prog, viscosity=nu, bottom_drag=r, surface_stress=tau, viscosity_field=fld, quadratic_drag=cd)
    got = mk.vertical_mixing(md.Prog)
    assert got[0] == nu and got[1] == r and (got[2] is None if tau is None else np.array_equal(got[2], tau))
    assert mk.quadratic_drag(md.Prog) == cd


def check(Prog, ref, poison=False):
    """tc.check_dycore; under poison the comparison of normalVelocity knows that NaN equals NaN."""
    if not poison:
        tc.check_dycore(Prog, ref[0])
    else:
        a = Prog.normalVelocity[-1].get()
        assert pc.same(a, ref[0][2]), ("normalVelocity", pc.differences(a, ref[0][2]))
        assert np.array_equal(Prog.layerThickness[-1].get(), ref[0][3]) and np.array_equal(Prog.ssh[-1].get(), ref[0][4])
    assert np.array_equal(mk.last_bottom_speed(Prog), ref[1])


def expected_path(K, variant, plan):
    launched = [w for w in plan if w and not (K < 2 and w in ("nu", "field"))]
    return mv.form_of(K, variant == 3) if launched else 0


def forward(backend, meshname, K, plan=(ALL,) * NSTEPS, mode="linear", mask=False, variant=0, poison=False, **kw):
    ref = reference(meshname, K, plan, mode, mask, poison)
    md = tc.Model(backend, meshname, K, mode=mode, mlt=mask_of(meshname, K, mask), variant=variant,
                  state=start_state(meshname, K, mask, poison), **kw)
    try:
        assert mk.momentum_vmix_path(md.Prog) == 0 and not mk.last_bottom_speed(md.Prog).any()
        for s, what in enumerate(plan):
            if s == 0 or what != plan[s - 1]:
                switch(md, meshname, what, mask)
            md.eager(1)
            check(md.Prog, ref[s], poison)
        assert mk.momentum_vmix_path(md.Prog) == expected_path(K, variant, plan)
        return md.Prog.normalVelocity[-1].get(), ref
    finally:
        md.close()


# ---- the square root and the gather, alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K", [("planar", 8), ("ico12f", 5)])
@pytest.mark.parametrize("mask", [False, "basin"], ids=["full", "basin"])
def test_bottom_speed_operator_bit_for_bit(backend, meshname, K, mask):
    """moka_bottom_speed on both time levels against the twin's bottom_speed, whatever Cd is: the sums in slot order, invArea, the
    correctly rounded square root.  With u NaN at every level below an edge's own floor (pc.edge_poison with no ring: the operator reads
    nothing else) the result is finite and has the bits of the unpoisoned one."""
    mesh, mlt = tc.get_mesh(meshname), depths(meshname, K, mask)
    ssh, u, h, rest = tc.state_of(meshname, K)
    want = qd.bottom_speed(u, mlt, mesh)
    assert np.all(want[np.minimum(mlt, K) >= 1] > 0.0)
    for poison in (False, True):
        up = pc.put(u, pc.edge_poison(mesh, mlt, K, 0), "nan") if poison else u
        md = tc.Model(backend, meshname, K, mlt=mask_of(meshname, K, mask), state=(ssh, up, h, rest))
        try:
            for level in (1, 0):
                got = mk.bottom_speed(md.Prog, level)
                assert np.all(np.isfinite(got))
                assert np.array_equal(got, want), int((got != want).sum())
            assert mk.quadratic_drag(md.Prog) == 0.0 and not mk.last_bottom_speed(md.Prog).any() and mk.momentum_vmix_path(md.Prog) == 0
        finally:
            md.close()


def test_bottom_speed_follows_the_time_levels(backend):
    ref = reference("planar", 8, ("cd",) * 2)
    md = tc.Model(backend, "planar", 8)
    try:
        switch(md, "planar", "cd")
        md.eager(2)
        mesh, mlt = md.mesh, depths("planar", 8, False)
        assert np.array_equal(mk.bottom_speed(md.Prog, 1), qd.bottom_speed(ref[1][0][2], mlt, mesh))
        assert np.array_equal(mk.bottom_speed(md.Prog, 0), qd.bottom_speed(ref[0][0][2], mlt, mesh))
        # the speed the pass used is that of u*, not of the level it left
        assert np.array_equal(mk.last_bottom_speed(md.Prog), ref[1][1]) and not np.array_equal(ref[1][1], mk.bottom_speed(md.Prog, 1))
    finally:
        md.close()


# ---- the pass: switches, levels, forms, meshes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", COMBOS)
def test_tile_form_with_16_byte_lanes(backend, what):
    got, _ = forward(backend, "planar", 8, plan=(what,) * NSTEPS)
    lin = reference("planar", 8, (what.replace("cd+", "").replace("cd", ""),) * NSTEPS)
    assert not np.array_equal(got, lin[-1][0][2])


@pytest.mark.parametrize("what", COMBOS)
def test_odd_levels_pentagons_and_flipped_cells(backend, what):
    """ico12f, K = 5: 8-byte lanes of the thickness gather, cells of five, six and seven edges (empty slots in the speed's rows)."""
    forward(backend, "ico12f", 5, plan=(what,) * NSTEPS)


@pytest.mark.parametrize("what", ["cd", "cd+drag", "cd+nu+stress", "cd+nu+drag+stress"])
def test_one_level(backend, what):
    """K = 1: only n == 1 columns, which Cd alone switches on; the column form (there is no tile of one level)."""
    forward(backend, "planar", 1, plan=(what,) * NSTEPS)


@pytest.mark.parametrize("what", COMBOS)
def test_a_cell_that_meets_the_same_neighbour_twice(backend, what):
    forward(backend, "tiny-2-4", 8, plan=(what,) * NSTEPS)


@pytest.mark.parametrize("what", ["cd", "cd+nu+drag+stress", "cd+field"])
def test_column_form_beyond_the_tile_boundary(backend, what):
    assert mv.form_of(106) == 2 and mv.form_of(105) == 1
    forward(backend, "planar", 106, plan=(what,))


@pytest.mark.parametrize("what", COMBOS)
def test_kernel_variant_3(backend, what):
    forward(backend, "planar", 8, plan=(what,) * NSTEPS, variant=3)


def test_switches_change_between_steps(backend):
    forward(backend, "planar", 8, plan=("cd", "cd+nu+drag+stress", "nu+drag", "cd+field", "", "cd+drag"), mask=True)


# ---- masks and poison -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K", [("planar", 8), ("ico12f", 5)])
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
@pytest.mark.parametrize("mask", [True, "basin"], ids=["partial_mlt", "basin"])
def test_masks_and_nan_below_every_edge(backend, meshname, K, variant, mask):
    """Edges of depth 0, 1 and everything up to K side by side; u NaN on the linear dycore's poison set.  Nothing changes on that set, no
    NaN reaches an active level or the speed, and the active levels have the bits of the run without the fill."""
    mesh, mlt = tc.get_mesh(meshname), depths(meshname, K, mask)
    assert (mlt == 0).any() and (mlt == 1).any() and (mlt >= K).any()
    got, ref = forward(backend, meshname, K, mask=mask, variant=variant, poison=True)
    fill, live = pc.edge_poison(mesh, mlt, K, 1), pc.active(mesh, mlt, K, "edge")
    assert np.all(np.isnan(got[fill])) and np.all(np.isfinite(got[live])) and np.all(np.isfinite(ref[-1][1]))
    clean = reference(meshname, K, (ALL,) * NSTEPS, mask=mask)
    assert np.array_equal(got[live], clean[-1][0][2][live]) and np.array_equal(ref[-1][1], clean[-1][1])


# ---- dycores and the 13-stream form ---------------------------------------------------------------------------------------------------
def test_nonlinear_dycore(backend):
    forward(backend, "planar", 34, mode="nonlinear")


def test_del2_del4_dycore(backend):
    forward(backend, "planar", 8, mode="del2+del4")


@pytest.mark.parametrize("mode", ["linear", "nonlinear"])
def test_13_stream_form(backend, mode):
    ref = reference("planar", 34, (ALL,) * NSTEPS, mode, s13=True)
    lib = L.lib()
    L.check(lib.moka_set_tuning(7, 1))
    try:
        md = tc.Model(backend, "planar", 34, mode=mode)
        try:
            assert lib.moka_state_rk4_streams(md.Prog._state._h) == 13
            switch(md, "planar", ALL)
            for s in range(NSTEPS):
                md.eager(1)
                check(md.Prog, ref[s])
            assert mk.momentum_vmix_path(md.Prog) == 1
        finally:
            md.close()
    finally:
        L.check(lib.moka_set_tuning(7, 0))


# ---- graph replay ---------------------------------------------------------------------------------------------------------------------
def test_run_equals_single_steps(backend):
    """moka_run(RK4, 3) and, over nine steps, the replayed graph (both launches inside it) equal single steps."""
    for n in (3, 9):
        ref = reference("planar", 8, (ALL,) * n)
        md = tc.Model(backend, "planar", 8)
        try:
            switch(md, "planar", ALL)
            md.run(n)
            check(md.Prog, ref[-1])
        finally:
            md.close()


def test_cd_changed_between_two_runs_takes_effect_in_the_second(backend):
    plan = ("cd+nu",) * 8 + ("nu",) * 8 + ("cd+nu+drag",) * 8
    ref = reference("planar", 8, plan)
    md = tc.Model(backend, "planar", 8)
    try:
        for seg in range(3):
            switch(md, "planar", plan[8 * seg])
            md.run(8)
            check(md.Prog, ref[8 * seg + 7])
    finally:
        md.close()


# ---- Cd == 0 --------------------------------------------------------------------------------------------------------------------------
def test_cd_set_and_set_back_restores_the_plain_state(backend):
    """Cd != 0 and back to 0 before any step: the steps, the path and the launch record are those of a state that never set it (the
    linear twin's bits; no speed was computed); with every coefficient zero the pass is off and the steps are the plain dycore's."""
    lib = L.lib()
    lin = reference("planar", 8, ("nu+drag",) * NSTEPS)
    plain = tc.reference("planar", 8, "linear", False, ((NSTEPS, 0, False),))
    for what, want in (("nu+drag", [r[0] for r in lin]), ("", plain)):
        md = tc.Model(backend, "planar", 8)
        try:
            switch(md, "planar", "cd+" + what if what else "cd")
            L.check(lib.moka_set_quadratic_bottom_drag(md.Prog._state._h, 0.0), md.backend._h)
            assert mk.quadratic_drag(md.Prog) == 0.0
            for s in range(NSTEPS):
                md.eager(1)
                tc.check_dycore(md.Prog, want[s])
                assert not mk.last_bottom_speed(md.Prog).any()
            assert mk.momentum_vmix_path(md.Prog) == (1 if what else 0)
            if not what:
                assert lib.moka_step_rk4(md.Prog._state._h, -md.dt) == 0          # the pass is off: a negative dt is allowed again
        finally:
            md.close()


def test_a_step_without_cd_after_one_with_it_hands_out_zeros(backend):
    ref = reference("planar", 8, ("cd+nu", "nu"))
    md = tc.Model(backend, "planar", 8)
    try:
        switch(md, "planar", "cd+nu")
        md.eager(1)
        check(md.Prog, ref[0])
        assert mk.last_bottom_speed(md.Prog).all()
        switch(md, "planar", "nu")
        md.eager(1)
        check(md.Prog, ref[1])
        assert not mk.last_bottom_speed(md.Prog).any()
    finally:
        md.close()


# ---- exact decay ----------------------------------------------------------------------------------------------------------------------
def test_exact_decay_of_a_uniform_flow(backend):
    """u_e(N) (1 + N dt Cd |U_0| / h) = u_e(0) on the device, within the bound quadratic_drag_twin's docstring counts; bit for bit the
    twin's run, whose own test prints the same figures."""
    mesh, state, U0 = qd.decay_state()
    cd = qd.decay_cd()
    md = tc.Model(backend, "planar-f0", 1, state=state)
    try:
        mk.set_vertical_mixing(md.Prog, quadratic_drag=cd)
        L.check(L.lib().moka_step_rk4(md.Prog._state._h, tc.EIG_DT), md.backend._h)
        sp = mk.last_bottom_speed(md.Prog)
        assert np.all(np.abs(sp - U0) <= (qd.counts(mesh)[1] + qd.DECAY_E0 + 2) * qd.U53 * U0)
        for _ in range(qd.DECAY_STEPS - 1):
            L.check(L.lib().moka_step_rk4(md.Prog._state._h, tc.EIG_DT), md.backend._h)
        got = md.Prog.normalVelocity[-1].get()
    finally:
        md.close()
    qd.decay_check(got, state[1], mesh, cd, "device")
    tw, st = qd.decay_twin(cd), TwinState(state[0], state[1], state[2])
    for _ in range(qd.DECAY_STEPS):
        tw.step_rk4(st, [[], []], tc.EIG_DT)
    assert np.array_equal(got, st.u[1])


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def snapshot(Prog):
    return [Prog.normalVelocity[lev].get() for lev in (0, 1)] + [Prog.layerThickness[lev].get() for lev in (0, 1)] + [Prog.ssh[-1].get()]


def unchanged(Prog, snap):
    return all(np.array_equal(a, b) for a, b in zip(snapshot(Prog), snap))


def test_bad_arguments(backend):
    md = tc.Model(backend, "planar", 8)
    lib, sh, ctx = L.lib(), md.Prog._state._h, md.backend._h
    try:
        switch(md, "planar", ALL)
        md.eager(1)
        snap, was, sp = snapshot(md.Prog), mk.quadratic_drag(md.Prog), mk.last_bottom_speed(md.Prog)
        for bad in (-1.0, np.nan, np.inf, -np.inf):
            assert lib.moka_set_quadratic_bottom_drag(sh, bad) == L.ERR_ARG
            assert b"quadratic drag" in lib.moka_last_error(ctx)
        v = C.c_double()
        assert lib.moka_set_quadratic_bottom_drag(None, 1.0) == L.ERR_ARG
        assert lib.moka_quadratic_bottom_drag(sh, None) == L.ERR_ARG and lib.moka_quadratic_bottom_drag(None, C.byref(v)) == L.ERR_ARG
        assert lib.moka_bottom_speed_download(sh, None) == L.ERR_ARG and lib.moka_bottom_speed_download(None, L.f64(sp)) == L.ERR_ARG
        out = np.empty(md.mesh.nEdges)
        assert lib.moka_bottom_speed(sh, 1, None) == L.ERR_ARG and lib.moka_bottom_speed(None, 1, L.f64(out)) == L.ERR_ARG
        for level in (-1, 2):
            assert lib.moka_bottom_speed(sh, level, L.f64(out)) == L.ERR_ARG
        # dt < 0 is refused before any launch while Cd alone keeps the pass on
        mk.set_vertical_mixing(md.Prog, quadratic_drag=was)
        assert lib.moka_step_rk4(sh, -md.dt) == L.ERR_ARG and b"dt must be >= 0" in lib.moka_last_error(ctx)
        assert lib.moka_run(sh, L.RUNGE_KUTTA_4, -md.dt, 3, 0) == L.ERR_ARG
        assert mk.quadratic_drag(md.Prog) == was and unchanged(md.Prog, snap) and np.array_equal(mk.last_bottom_speed(md.Prog), sp)
        assert lib.moka_step_rk4(sh, 0.0) == 0                # dt == 0.0 launches nothing
        assert np.array_equal(mk.last_bottom_speed(md.Prog), sp)
    finally:
        md.close()


def test_unsupported_while_cd_keeps_the_pass_on(backend):
    """Everything that is refused while the pass is on is refused when Cd alone turned it on, and leaves the state and Cd as they were;
    a state with a moka_tape and an fp32-storage state refuse a nonzero Cd."""
    md = tc.Model(backend, "planar", 8)
    lib, sh, ctx = L.lib(), md.Prog._state._h, md.backend._h
    try:
        switch(md, "planar", "cd")
        md.eager(1)
        snap, was = snapshot(md.Prog), mk.quadratic_drag(md.Prog)
        assert lib.moka_step_fe(sh, md.dt, L.FE_REFERENCE_COMPAT) == L.ERR_UNSUPPORTED
        assert b"vertical momentum mixing" in lib.moka_last_error(ctx)
        assert lib.moka_run(sh, L.FORWARD_EULER, md.dt, 3, L.FE_REFERENCE_COMPAT) == L.ERR_UNSUPPORTED
        tape = C.c_void_p()
        assert lib.moka_tape_create(sh, 2, C.byref(tape)) == L.ERR_UNSUPPORTED
        assert b"vertical momentum mixing" in lib.moka_last_error(ctx) and not tape.value
        z32, z64 = np.zeros(1, np.int32), np.zeros(1, np.int64)
        p32, p64 = z32.ctypes.data_as(C.POINTER(C.c_int32)), z64.ctypes.data_as(C.POINTER(C.c_int64))
        hh = C.c_void_p()
        assert lib.moka_halo_create(sh, 0, p32, p64, p32, p64, p32, p64, p32, p64, 0, 0, C.byref(hh)) == L.ERR_UNSUPPORTED
        assert b"vertical momentum mixing" in lib.moka_last_error(ctx) and not hh.value
        # reverse mode through the forced step does not cover the quadratic drag
        ft = C.c_void_p()
        assert lib.moka_forced_tape_create(sh, 2, C.byref(ft)) == L.ERR_UNSUPPORTED
        assert b"quadratic" in lib.moka_last_error(ctx) and not ft.value
        assert mk.quadratic_drag(md.Prog) == was and unchanged(md.Prog, snap)
        # ... and the other way round: a state with a moka_tape takes no Cd
        switch(md, "planar", "")
        t = mk.AdjointTape(md.Prog, 2)
        assert lib.moka_set_quadratic_bottom_drag(sh, 1e-3) == L.ERR_UNSUPPORTED
        assert b"moka_tape" in lib.moka_last_error(ctx)
        assert lib.moka_set_quadratic_bottom_drag(sh, 0.0) == 0
        assert mk.quadratic_drag(md.Prog) == 0.0 and unchanged(md.Prog, snap)
        t.close()
        assert lib.moka_set_quadratic_bottom_drag(sh, 1e-3) == 0
    finally:
        md.close()
    f32 = tc.Model(backend, "ico16", 4, state_bytes=4)
    try:
        fh = f32.Prog._state._h
        assert lib.moka_set_quadratic_bottom_drag(fh, 1e-3) == L.ERR_UNSUPPORTED
        assert b"Float64" in lib.moka_last_error(ctx)
        out = np.empty(f32.mesh.nEdges)
        assert lib.moka_bottom_speed(fh, 1, L.f64(out)) == L.ERR_UNSUPPORTED
        assert lib.moka_set_quadratic_bottom_drag(fh, 0.0) == 0
    finally:
        f32.close()


def test_a_forced_tape_refuses_a_later_cd_and_the_tracer_tape_does_not(backend):
    """A forced tape created while Cd == 0 refuses a nonzero Cd for as long as it exists, with the state, Cd and the tape's steps as they
    were; the tracer tape records steps under the quadratic drag (tracers never see the pass inside a step)."""
    ref = reference("planar", 8, ("nu+drag",) * 2)
    md = tc.Model(backend, "planar", 8)
    lib, sh, ctx = L.lib(), md.Prog._state._h, md.backend._h
    try:
        switch(md, "planar", "nu+drag")
        ft = mk.ForcedAdjointTape(md.Prog, 2)
        try:
            ft.step(md.dt)
            snap = snapshot(md.Prog)
            assert lib.moka_set_quadratic_bottom_drag(sh, 1e-3) == L.ERR_UNSUPPORTED
            assert b"moka_forced_tape" in lib.moka_last_error(ctx)
            assert mk.quadratic_drag(md.Prog) == 0.0 and unchanged(md.Prog, snap)
            assert lib.moka_set_quadratic_bottom_drag(sh, 0.0) == 0
            ft.step(md.dt)
            tc.check_dycore(md.Prog, ref[1][0])
        finally:
            ft.close()
        assert lib.moka_set_quadratic_bottom_drag(sh, 1e-3) == 0 and mk.quadratic_drag(md.Prog) == 1e-3
    finally:
        md.close()
    ref = reference("planar", 8, (ALL,) * 2)
    md = tc.Model(backend, "planar", 8)
    try:
        f = tc.distinct_fields(md.mesh, 8, 2)
        mk.set_tracers(md.Prog, f)
        switch(md, "planar", ALL)
        tape = mk.TracerAdjointTape(md.Prog, 2)
        try:
            for s in range(2):
                tape.step(md.dt)
                check(md.Prog, ref[s])
        finally:
            tape.close()
    finally:
        md.close()


def test_refused_on_a_rank_with_a_halo():
    """One rank of a two-way LocalCluster (a partitioned mesh with a halo): Cd cannot be switched on, the operator is refused."""
    from moka_hip import parallel as par
    mesh = tc.get_mesh("ico12f")
    K = 4
    ssh, u, h, rest = tc.random_state(mesh, K, 12)
    cl = par.LocalCluster(mesh, ssh, u, h, rest, 20.0, 2, direct=False)
    try:
        sh = cl.models[0].Prog._state._h
        assert L.lib().moka_set_quadratic_bottom_drag(sh, 1e-3) == L.ERR_UNSUPPORTED
        assert L.lib().moka_set_quadratic_bottom_drag(sh, 0.0) == 0
        n = cl.models[0].Prog.normalVelocity[-1].get().shape[0]
        assert L.lib().moka_bottom_speed(sh, 1, L.f64(np.empty(n))) == L.ERR_UNSUPPORTED
    finally:
        cl.close()


# ---- the reference-order shim ---------------------------------------------------------------------------------------------------------
def test_shim_calls(tmp_path):
    """moka_hip/shim.py: the four calls on a model built in the reference's constructor order (the inertia-gravity-wave case of
    test_gpu_parity.py, one level), one RungeKutta4 step under Cd against the twin."""
    import test_gpu_parity as tp
    import tracer_vmix_twin as tv
    from moka_hip import shim
    from moka_hip.timemanager import period_seconds
    mesh, (ssh, u, h, rest), cfg_fp, _ = tp._write_igw_case(tmp_path)
    u, h = np.asarray(u, dtype=np.float64).reshape(mesh.nEdges, 1), np.asarray(h, dtype=np.float64).reshape(mesh.nCells, 1)
    b = shim.Backend(0)
    Setup, Diag, Tend, Prog = shim.ocn_init(str(cfg_fp), b)
    dts = float(period_seconds(Setup.timeManager.timeStep))
    mlt = np.ones(mesh.nEdges, dtype=np.int32)
    assert shim.quadratic_drag(Prog, Setup.mesh, b) == 0.0 and not shim.last_bottom_speed(Prog, Setup.mesh, b).any()
    sp0 = qd.bottom_speed(u, mlt, mesh)
    assert sp0.any() and np.array_equal(shim.bottom_speed(Prog, Setup.mesh, b), sp0)
    cd = 0.5 * float(h.mean()) / (dts * float(sp0.mean()))
    shim.set_quadratic_drag(Prog, Setup.mesh, cd, b)
    assert shim.quadratic_drag(Prog, Setup.mesh, b) == cd
    shim.ocn_timestep(Prog, Diag, Tend, Setup, shim.RungeKutta4, backend=b)
    om = orc.OracleMesh(mesh, 1, resting_thickness_sum=np.asarray(rest).reshape(mesh.nCells, -1).sum(1))
    tw = qd.QuadraticDragTwin(mv.MomentumVmixTwin(tv.VmixTwin(om, om, [])), cd)
    st, plain = TwinState(np.asarray(ssh), u, h), TwinState(np.asarray(ssh), u, h)
    tw.step_rk4(st, [[], []], dts)
    tw.mt.tw.step_rk4(plain, [[], []], dts)
    got = np.asarray(Prog.normalVelocity[-1])
    assert np.array_equal(got, st.u[1]) and not np.array_equal(got, plain.u[1])
    assert np.array_equal(shim.last_bottom_speed(Prog, Setup.mesh, b), tw.sp)
    assert np.array_equal(shim.bottom_speed(Prog, Setup.mesh, b, 1), qd.bottom_speed(st.u[1], mlt, mesh))
