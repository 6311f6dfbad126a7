"""Implicit vertical mixing of momentum with a surface stress and a bottom drag on the device (csrc/momentum_vmix.hip: k_mvmix_tile,
k_mvmix_column; the launch behind stage 4 of step_rk4; moka_set_vertical_viscosity, moka_surface_stress_upload): everything bit for bit
against the numpy twin of tests/momentum_vmix_twin.py, through tc.check_dycore after each of three RK4 steps.

A case names, per step, the switches in force: "nu", "drag", "stress" (a stress on every edge) or "stress0" (every third edge exactly
0.0), joined by "+"; "" switches the pass off.  The coefficients are mv.coefficients (s / hm^2 = 4, q / hm = 1/2) and mv.stress_field.
The twin's case is computed once and shared.  Every test that touches a new call fails without the feature with a missing symbol; the
"pass is off" cases are the ones that pass there."""
import ctypes as C

import numpy as np
import pytest

import moka_hip as mk
import momentum_vmix_twin as mv
import oracle as orc
import poison_cases as pc
import tracer_adjoint_twin as ta
import tracer_biharmonic_twin as tb
import tracer_cases as tc
import tracer_source_twin as ts
import tracer_vfield_twin as tf
import tracer_vmix_twin as tv
from del4_twin import TwinState
from moka_hip import lib as L

pytestmark = pytest.mark.gpu
NSTEPS = 3
ALL = "nu+drag+stress"
_REFS = {}


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)
    yield b
    b.close()


def settings(meshname, K, what):
    """(nuV, r, tau) of a switch combination."""
    nu, r = mv.coefficients(meshname, K)
    parts = what.split("+") if what else []
    tau = None
    if "stress" in parts or "stress0" in parts:
        tau = mv.stress_field(tc.get_mesh(meshname), K, zeros="stress0" in parts)
    return (nu if "nu" in parts else 0.0), (r if "drag" in parts else 0.0), tau


def mask_of(meshname, K, partial):
    """partial: False (full columns: None), True (tc.partial_mlt) or "basin" (poison_cases.mask_of: land, full columns, every depth)."""
    return None if not partial else pc.mask_of(meshname, K) if partial == "basin" else tc.partial_mlt(tc.get_mesh(meshname), K)


def start_state(meshname, K, partial, poison):
    """(ssh, u, h, rest) of the case; poison: u is NaN at every level no active element of the linear dycore reads
    (poison_cases.edge_poison over the case's mask).  layerThickness is never filled: ssh is a column sum over all K levels, so within
    a step every level of every cell is read by an active element."""
    ssh, u, h, rest = tc.state_of(meshname, K)
    if poison:
        u = pc.put(u, pc.edge_poison(tc.get_mesh(meshname), mask_of(meshname, K, partial), K, 1), "nan")
    return ssh, u, h, rest


def reference(meshname, K, mode, partial, plan, poison=False, s13=False):
    """The twin's (None, None, u, h, ssh) after every step of `plan` (one switch combination per step), computed once and shared."""
    key = (meshname, K, mode, partial, tuple(plan), poison, s13)
    if key not in _REFS:
        ssh, u, h, _ = start_state(meshname, K, partial, poison)
        tw = mv.momentum_twin(meshname, K, "linear" if s13 else mode, mlt=mask_of(meshname, K, partial))
        out = []
        if s13:
            om = tw.tw.om
            st, nl = orc.OracleState(om, ssh, u, h), (orc.OracleNonlinear(om) if mode == "nonlinear" else None)
        else:
            st, phis = TwinState(ssh, u, h), [[], []]
        for what in plan:
            tw.nu, tw.drag, tw.tau = settings(meshname, K, what)
            if s13:
                tw.step_s13(st, tc.dt_of(meshname), nl)
            else:
                tw.step_rk4(st, phis, tc.dt_of(meshname))
            out.append((None, None, st.u[1].copy(), st.h[1].copy(), st.ssh[1].copy()))
        _REFS[key] = out
    return _REFS[key]


def switch(md, meshname, what):
    nu, r, tau = settings(meshname, md.K, what)
    mk.set_vertical_mixing(md.Prog, viscosity=nu, bottom_drag=r, surface_stress=tau)
    got = mk.vertical_mixing(md.Prog)
    assert got[0] == nu and got[1] == r and (got[2] is None if tau is None else np.array_equal(got[2], tau))


def check(Prog, ref):
    a = Prog.normalVelocity[-1].get()
    assert pc.same(a, ref[2]), ("normalVelocity", pc.differences(a, ref[2]))
    assert np.array_equal(Prog.layerThickness[-1].get(), ref[3])
    assert np.array_equal(Prog.ssh[-1].get(), ref[4])


def expected_path(K, variant, plan):
    launched = [w for w in plan if w and not (K < 2 and w == "nu")]
    return mv.form_of(K, variant == 3) if launched else 0


def forward(backend, meshname, K, plan=(ALL,) * NSTEPS, mode="linear", partial=False, variant=0, poison=False, use_run=False, **kw):
    ref = reference(meshname, K, mode, partial, plan, poison)
    md = tc.Model(backend, meshname, K, mode=mode, mlt=mask_of(meshname, K, partial), variant=variant,
                  state=start_state(meshname, K, partial, poison), **kw)
    try:
        assert mk.momentum_vmix_path(md.Prog) == 0
        if use_run:
            switch(md, meshname, plan[0])
            md.run(len(plan))
            check(md.Prog, ref[-1])
        else:
            for s, what in enumerate(plan):
                if s == 0 or what != plan[s - 1]:
                    switch(md, meshname, what)
                md.eager(1)
                check(md.Prog, ref[s])
        assert mk.momentum_vmix_path(md.Prog) == expected_path(K, variant, plan)
        return md.Prog.normalVelocity[-1].get(), ref
    finally:
        md.close()


# ---- levels and forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 34, 60, 64, 65])
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_levels_and_forms(backend, K, variant):
    """1080 edges: the last tile is short.  K = 1: the n == 1 rows alone, with drag and stress (the column form: there is no tile of one
    level).  K = 2: the two end rows.  K = 3: the first interior row.  K = 34 .. 65: tiles of 32 edges (K = 2, 3: of 64); odd K: the
    8-byte gather beside the 16-byte one.  Variant 3 takes the column form; both forms give the twin's bits, hence each other's."""
    got, ref = forward(backend, "planar", K, variant=variant)
    plain = tc.reference("planar", K, "linear", False, ((NSTEPS, 0, False),))
    assert not np.array_equal(got, plain[-1][2])


def test_one_level_with_the_viscosity_alone_launches_nothing(backend):
    got, _ = forward(backend, "planar", 1, plan=("nu",) * NSTEPS)
    assert np.array_equal(got, tc.reference("planar", 1, "linear", False, ((NSTEPS, 0, False),))[-1][2])


@pytest.mark.parametrize("K,path", [(105, 1), (106, 2)])
def test_tile_and_column_boundary(backend, K, path):
    """48 edges: fewer than a tile.  3 * 32 * (K | 1) * 8 bytes and the records twice in 160 KiB: K <= 105."""
    assert mv.form_of(K) == path
    forward(backend, "tiny-4-4", K, plan=(ALL,))


# ---- meshes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 34])
def test_pentagons_and_heptagons(backend, K):
    """ico12f: the cell columns of an edge lie at irregular distances."""
    forward(backend, "ico12f", K)


@pytest.mark.parametrize("K", [5, 35])
def test_cell_columns_off_the_16_byte_grid(backend, K):
    """35 cells, odd K: every second cell column starts 8 bytes off a 16-byte boundary, so the gather takes 8-byte lanes there."""
    forward(backend, tf.sheared_mesh(7, 5), K)


# ---- masks --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [6, 34])
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
@pytest.mark.parametrize("mask", [True, "basin"], ids=["partial_mlt", "basin"])
def test_masks_and_nan_below_every_edge(backend, K, variant, mask):
    """tc.partial_mlt: edges of depth 0, 1 and everything up to K side by side, at random -- nearly every level of u is then read by
    some active neighbour, so the fill has next to nothing to sit on.  The basin of poison_cases has the same depths in bands: there
    u is NaN on a large set.  Nothing changes on that set, no NaN reaches an active level, and the active levels have the bits of the
    run without the fill."""
    mesh = tc.get_mesh("planar")
    mlt = mask_of("planar", K, mask)
    assert (mlt == 0).any() and (mlt == 1).any() and (mlt == K).any()
    got, ref = forward(backend, "planar", K, partial=mask, variant=variant, poison=True)
    fill = pc.edge_poison(mesh, mlt, K, 1)
    live = pc.active(mesh, mlt, K, "edge")
    assert mask is True or fill.mean() > 0.1
    assert np.all(np.isnan(got[fill])) and np.all(np.isfinite(got[live]))
    clean = reference("planar", K, "linear", mask, (ALL,) * NSTEPS)
    assert np.array_equal(got[live], clean[-1][2][live])
    got2, _ = forward(backend, "planar", K, partial=mask, variant=variant)
    assert np.array_equal(got2[live], got[live])


# ---- switches -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_every_switch_combination_step_by_step(backend, variant):
    """The values in force change between steps and take effect at the next one; partial columns, so that drag and stress meet n == 1."""
    forward(backend, "planar", 6, plan=("nu", "drag", "stress", ALL, "nu+drag+stress0", "stress0", "nu+drag"), partial=True, variant=variant)


@pytest.mark.parametrize("what", ["nu", "drag", "stress", "nu+stress0"])
def test_single_switches(backend, what):
    forward(backend, "planar", 34, plan=(what,) * NSTEPS)


def test_removing_the_stress_restores_the_earlier_bits(backend):
    ref = reference("planar", 34, "linear", False, ("nu+drag",) * 2)
    md = tc.Model(backend, "planar", 34)
    try:
        switch(md, "planar", ALL)
        nu, r, _ = settings("planar", 34, ALL)
        mk.set_vertical_mixing(md.Prog, viscosity=nu, bottom_drag=r, surface_stress=None)
        assert mk.vertical_mixing(md.Prog)[2] is None
        md.eager(2)
        check(md.Prog, ref[-1])
    finally:
        md.close()


# ---- dycores and the 13-stream form -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["nonlinear", "del2+del4"])
def test_dycores(backend, mode):
    forward(backend, "planar", 34, mode=mode)


@pytest.mark.parametrize("mode", ["linear", "nonlinear"])
def test_13_stream_form(backend, mode):
    """moka_set_tuning(7, 1): stage 4 writes the new level through the same two pointers; the twin is the pass behind the oracle's
    13-stream steps."""
    ref = reference("planar", 34, mode, False, (ALL,) * NSTEPS, s13=True)
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


# ---- tracers ------------------------------------------------------------------------------------------------------------------------
def tracer_case(meshname, K):
    """The chain's twin with three tracers (kappa, kappa4, kappaV, sources on tracers 0 and 2) under the pass, three recorded steps, and
    the sweep of ta.seeds over the twin's tape (the flow recorded as it ran).  Computed once."""
    key = ("tracers", meshname, K)
    if key not in _REFS:
        mesh = tc.get_mesh(meshname)
        tw = mv.momentum_twin(meshname, K)
        tw.nu, tw.drag, tw.tau = settings(meshname, K, ALL)
        q = ts.source_fields(meshname, K, 9)
        tw.tw.source = [q[0], None, q[2]]
        tw.tw.kappa, tw.tw.kappa4 = tc.kappas(meshname, 9)[:3], tb.kappa4s(meshname, 9)[:3]
        tw.tw.kappaV = tv.kappavs(meshname, K, 9)[:3]
        ssh, u, h, _ = tc.state_of(meshname, K)
        st = TwinState(ssh, u, h)
        f = tc.distinct_fields(mesh, K, 9)[:3]
        phis = [[a.copy() for a in f], [a.copy() for a in f]]
        fwd = []
        for _ in range(NSTEPS):
            tw.step_rk4(st, phis, tc.dt_of(meshname))
            fwd.append(([a.copy() for a in phis[0]], [a.copy() for a in phis[1]], st.u[1].copy(), st.h[1].copy(), st.ssh[1].copy()))
        X = ta.seeds(mesh, K, 9)[:3]
        grad = tv.VmixAdjointTwin(tw.tw).sweep_kgrad(tw.tw.tape, [x.copy() for x in X], {}, ())[0]
        _REFS[key] = {"fields": f, "sources": list(tw.tw.source), "kappa": list(tw.tw.kappa), "kappa4": list(tw.tw.kappa4),
                      "kappaV": list(tw.tw.kappaV), "forward": fwd, "X": X, "grad": grad}
    return _REFS[key]


@pytest.mark.parametrize("taped", [False, True], ids=["steps", "tape"])
def test_tracers_beside_the_pass(backend, taped):
    """Tracers never see the pass inside a step; from the next step on they ride the mixed flow.  On a tracer tape the recorded flow is
    the flow as it ran, so X is the twin's bit for bit."""
    ref = tracer_case("planar", 34)
    md = tc.Model(backend, "planar", 34)
    try:
        tr_ = mk.set_tracers(md.Prog, ref["fields"], diffusivity=ref["kappa"], sources=ref["sources"], biharmonic=ref["kappa4"],
                             vertical=ref["kappaV"])
        switch(md, "planar", ALL)
        tape = mk.TracerAdjointTape(md.Prog, NSTEPS) if taped else None
        try:
            for s in range(NSTEPS):
                if taped:
                    tape.step(md.dt)
                else:
                    md.eager(1)
                tc.check_tracers(tr_, ref["forward"][s])
                check(md.Prog, ref["forward"][s])
            if taped:
                grad = tape.gradient(ref["X"])
                for j in range(3):
                    assert np.array_equal(grad[j], ref["grad"][j]), ("X", j)
                assert L.lib().moka_step_rk4_tracer_taped(tape._h, -md.dt) == L.ERR_ARG
        finally:
            if tape is not None:
                tape.close()
        assert mk.momentum_vmix_path(md.Prog) == 1 and tr_.vmix_path() == 1
    finally:
        md.close()


# ---- graph replay -------------------------------------------------------------------------------------------------------------------
def test_run_replays_the_pass_from_a_captured_graph(backend):
    got, _ = forward(backend, "planar", 3, plan=(ALL,) * 9, use_run=True)
    eager, _ = forward(backend, "planar", 3, plan=(ALL,) * 9)
    assert np.array_equal(got, eager)


# ---- the pass is off ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("touch", [False, True], ids=["never-called", "zeros-and-null"])
def test_pass_off_is_todays_step(backend, touch):
    ref = tc.reference("planar", 34, "linear", False, ((NSTEPS, 0, False),))
    md = tc.Model(backend, "planar", 34)
    lib = L.lib()
    try:
        for s in range(NSTEPS):
            if touch:
                sh = md.Prog._state._h
                assert lib.moka_set_vertical_viscosity(sh, 0.0, 0.0) == 0 and lib.moka_surface_stress_upload(sh, None) == 0
            md.eager(1)
            tc.check_dycore(md.Prog, ref[s])
        if touch:
            # a stress that is zero at every active edge is present and counts as absent
            mk.set_vertical_mixing(md.Prog, surface_stress=np.zeros(md.mesh.nEdges))
            assert mk.vertical_mixing(md.Prog)[2] is not None
            ref4 = tc.reference("planar", 34, "linear", False, ((NSTEPS + 1, 0, False),))
            md.eager(1)
            tc.check_dycore(md.Prog, ref4[-1])
            assert lib.moka_step_rk4(md.Prog._state._h, -md.dt) == 0              # and a negative dt is still allowed
            assert lib.moka_state_momentum_vmix_path(md.Prog._state._h) == 0 and lib.moka_state_momentum_vmix_path(None) == 0
    finally:
        md.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def snapshot(Prog):
    return [Prog.normalVelocity[lev].get() for lev in (0, 1)] + [Prog.layerThickness[lev].get() for lev in (0, 1)] + [Prog.ssh[-1].get()]


def unchanged(Prog, snap):
    return all(np.array_equal(a, b) for a, b in zip(snapshot(Prog), snap))


def test_bad_arguments(backend):
    md = tc.Model(backend, "planar", 6)
    lib, sh, ctx = L.lib(), md.Prog._state._h, md.backend._h
    try:
        switch(md, "planar", ALL)
        md.eager(1)
        snap, was = snapshot(md.Prog), mk.vertical_mixing(md.Prog)
        for bad in (-1.0, np.nan, np.inf):
            assert lib.moka_set_vertical_viscosity(sh, bad, 1.0) == L.ERR_ARG
            assert b"vertical momentum mixing" in lib.moka_last_error(ctx)
            assert lib.moka_set_vertical_viscosity(sh, 1.0, bad) == L.ERR_ARG
        for bad in (np.nan, np.inf, -np.inf):
            tau = was[2].copy()
            tau[7] = bad
            assert lib.moka_surface_stress_upload(sh, L.f64(tau)) == L.ERR_ARG
            assert b"surface stress" in lib.moka_last_error(ctx)
        v, i = C.c_double(), C.c_int()
        assert lib.moka_vertical_viscosity(sh, None, C.byref(v)) == L.ERR_ARG
        assert lib.moka_vertical_viscosity(sh, C.byref(v), None) == L.ERR_ARG
        assert lib.moka_surface_stress_download(sh, None) == L.ERR_ARG
        assert lib.moka_has_surface_stress(sh, None) == L.ERR_ARG
        assert lib.moka_has_surface_stress(sh, C.byref(i)) == 0 and i.value == 1
        # dt < 0 is refused before any launch while the pass is on
        assert lib.moka_step_rk4(sh, -md.dt) == L.ERR_ARG
        assert b"dt must be >= 0" in lib.moka_last_error(ctx)
        assert lib.moka_run(sh, L.RUNGE_KUTTA_4, -md.dt, 3, 0) == L.ERR_ARG
        now = mk.vertical_mixing(md.Prog)
        assert now[:2] == was[:2] and np.array_equal(now[2], was[2]) and unchanged(md.Prog, snap)
        # dt == 0.0 launches nothing: the step of a state without the pass
        assert lib.moka_step_rk4(sh, 0.0) == 0
    finally:
        md.close()


def test_unsupported_while_the_pass_is_on(backend):
    """Forward Euler (step and run), moka_tape_create and moka_halo_create refuse a state whose pass is on, with a message that names it,
    and leave the state as it was; a state with a moka_tape and an fp32-storage state refuse the pass."""
    md = tc.Model(backend, "planar", 6)
    lib, sh, ctx = L.lib(), md.Prog._state._h, md.backend._h
    try:
        switch(md, "planar", "drag")
        md.eager(1)
        snap = snapshot(md.Prog)
        assert lib.moka_step_fe(sh, md.dt, L.FE_REFERENCE_COMPAT) == L.ERR_UNSUPPORTED
        assert b"vertical momentum mixing" in lib.moka_last_error(ctx)
        assert lib.moka_run(sh, L.FORWARD_EULER, md.dt, 3, L.FE_REFERENCE_COMPAT) == L.ERR_UNSUPPORTED
        assert b"vertical momentum mixing" in lib.moka_last_error(ctx)
        tape = C.c_void_p()
        assert lib.moka_tape_create(sh, 2, C.byref(tape)) == L.ERR_UNSUPPORTED
        assert b"vertical momentum mixing" in lib.moka_last_error(ctx) and not tape.value
        z32, z64 = np.zeros(1, np.int32), np.zeros(1, np.int64)
        p32, p64 = z32.ctypes.data_as(C.POINTER(C.c_int32)), z64.ctypes.data_as(C.POINTER(C.c_int64))
        hh = C.c_void_p()
        assert lib.moka_halo_create(sh, 0, p32, p64, p32, p64, p32, p64, p32, p64, 0, 0, C.byref(hh)) == L.ERR_UNSUPPORTED
        assert b"vertical momentum mixing" in lib.moka_last_error(ctx) and not hh.value
        assert unchanged(md.Prog, snap)
        # ... and the other way round: a state with a tape takes no pass
        switch(md, "planar", "")
        t = mk.AdjointTape(md.Prog, 2)
        assert lib.moka_set_vertical_viscosity(sh, 1.0, 0.0) == L.ERR_UNSUPPORTED
        assert b"moka_tape" in lib.moka_last_error(ctx)
        assert lib.moka_surface_stress_upload(sh, L.f64(np.ones(md.mesh.nEdges))) == L.ERR_UNSUPPORTED
        assert mk.vertical_mixing(md.Prog) == (0.0, 0.0, None) and unchanged(md.Prog, snap)
        t.close()
        assert lib.moka_set_vertical_viscosity(sh, 1.0, 0.0) == 0
    finally:
        md.close()
    f32 = tc.Model(backend, "ico16", 4, state_bytes=4)
    try:
        fh = f32.Prog._state._h
        assert lib.moka_set_vertical_viscosity(fh, 1.0, 0.0) == L.ERR_UNSUPPORTED
        assert b"Float64" in lib.moka_last_error(ctx)
        assert lib.moka_surface_stress_upload(fh, L.f64(np.ones(f32.mesh.nEdges))) == L.ERR_UNSUPPORTED
        assert lib.moka_set_vertical_viscosity(fh, 0.0, 0.0) == 0
    finally:
        f32.close()


def test_refused_on_a_rank_with_a_halo():
    """One rank of a two-way LocalCluster (a partitioned mesh with a halo): the pass cannot be switched on."""
    from moka_hip import parallel as par
    mesh = tc.get_mesh("ico12f")
    K = 4
    ssh, u, h, rest = tc.random_state(mesh, K, 12)
    cl = par.LocalCluster(mesh, ssh, u, h, rest, 20.0, 2, direct=False)
    try:
        sh = cl.models[0].Prog._state._h
        assert L.lib().moka_set_vertical_viscosity(sh, 1.0, 1.0) == L.ERR_UNSUPPORTED
        assert L.lib().moka_surface_stress_upload(sh, None) == 0
    finally:
        cl.close()
