"""The Richardson-number closure on the device (moka_set_richardson_mixing; csrc/vmix_closure.hip: k_rich_edge, k_rich_cell; the step in
csrc/api_state.hip): after every RK4 step normalVelocity, layerThickness, ssh, every tracer of both time levels, F and G
(richardson_fields) and Ri of the new level (richardson_number) are bit for bit those of the numpy twin (tests/richardson_twin.py), so
that a wrong coefficient can be told from a wrong pass.  The branch census of every case here is asserted on the CPU
(tests/test_richardson_twin.py: DEVICE_CASES).  References are computed once and shared.  Every test but the last calls an entry point the
parent commit does not have."""
import ctypes as C

import numpy as np
import pytest

import moka_hip as mk
import momentum_vfield_twin as mf
import momentum_vmix_twin as mv
import poison_cases as pc
import quadratic_drag_twin as qd
import richardson_twin as rt
import tracer_cases as tc
import tracer_vfield_twin as tf
import tracer_vmix_twin as tv
from moka_hip import lib as L

pytestmark = pytest.mark.gpu
NSTEPS = 3
P0 = rt.Params(rt.JB)
_SETTINGS = {}


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)
    yield b
    b.close()


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def settings(meshname, K, tag, mask=None):
    """The set-aside coefficients of a run by name: "" none; "forced" a drag, a stress and a quadratic drag (untouched by the closure);
    "aside" a scalar viscosity, an uploaded viscosity field, the tracers' scalars and an uploaded diffusivity field for tracer 2 (all
    set aside for what the closure covers) on top of "forced"."""
    key = (meshname, K, tag, mask)
    if key not in _SETTINGS:
        s = {}
        if tag in ("forced", "aside"):
            mesh = tc.get_mesh(meshname)
            s.update(drag=mv.coefficients(meshname, K)[1], tau=mv.stress_field(mesh, K), cd=qd.cd_of(K, tc.dt_of(meshname)))
        if tag == "aside":
            cs = rt.case(meshname, K, mask)
            s.update(nu=mv.coefficients(meshname, K)[0], fld=mf.case_field(meshname, K, cs["mlt"]), kappaV=tv.kappavs(meshname, K, 3),
                     fieldV=[None, None, tf.case_field(meshname, K, cs["nlev"])])
        _SETTINGS[key] = s
    return _SETTINGS[key]


def model(backend, meshname, K, mask=None, poison=None, mode="linear", variant=0, tag=""):
    cs = rt.case(meshname, K, mask, poison, mode)
    md = tc.Model(backend, meshname, K, mode=mode, mlt=cs["mlt"], variant=variant, state=cs["state"])
    s = settings(meshname, K, tag, mask)
    vert = None
    if "kappaV" in s:
        vert = [s["fieldV"][j] if s["fieldV"][j] is not None else s["kappaV"][j] for j in range(rt.NT)]
    md.tr = mk.set_tracers(md.Prog, cs["fields"], vertical=vert)
    if "kappaV" in s:
        md.tr.set_vertical_diffusivity(s["kappaV"])        # (a scalar beside the field of tracer 2: set aside by the field)
    mk.set_vertical_mixing(md.Prog, viscosity=s.get("nu", 0.0), bottom_drag=s.get("drag", 0.0), surface_stress=s.get("tau"),
                           viscosity_field=s.get("fld"), quadratic_drag=s.get("cd", 0.0))
    return md


def switch(md, P):
    if P is None:
        mk.set_richardson_mixing(md.Prog, None)
        assert mk.richardson_mixing(md.Prog) is None
        return
    mk.set_richardson_mixing(md.Prog, P.buoyancy, **P.kwargs())
    got = mk.richardson_mixing(md.Prog)
    want = dict(P.kwargs(), buoyancy=P.buoyancy, tracers=list(range(rt.NT)) if P.tracers is None else P.tracers)
    assert got == want


def check(md, ref, P, poison=None):
    same = pc.same_where_finite if poison else np.array_equal
    u = md.Prog.normalVelocity[-1].get()
    assert same(u, ref[2]), ("normalVelocity", pc.differences(u, ref[2]))
    assert np.array_equal(md.Prog.layerThickness[-1].get(), ref[3])
    assert np.array_equal(md.Prog.ssh[-1].get(), ref[4])
    for j in range(rt.NT):
        assert same(md.tr.get(j), ref[1][j]), ("tracer", j, pc.differences(md.tr.get(j), ref[1][j]))
        assert same(md.tr.get(j, 0), ref[0][j]), ("previous tracer", j)
    F, G = mk.richardson_fields(md.Prog)
    assert np.array_equal(F, ref[5]), ("F", pc.differences(F, ref[5]))
    assert np.array_equal(G, ref[6]), ("G", pc.differences(G, ref[6]))
    if P is not None:
        rE, rC = mk.richardson_number(md.Prog)
        assert np.array_equal(rE, ref[7]), ("RiEdge", pc.differences(rE, ref[7]))
        assert np.array_equal(rC, ref[8]), ("RiCell", pc.differences(rC, ref[8]))


def check_previous_level(md, cs, P, u, h, b):
    """moka_richardson_diagnose of time level 0 against the twin's recipe on the previous level (u, h, b): after a step the two levels
    differ, so a level mistaken for the other does not pass."""
    c1, c2 = mv.edge_cells(cs["mesh"])
    rE, rC = mk.richardson_number(md.Prog, time_level=0)
    assert np.array_equal(rE, rt.edge_field(u, h, b, cs["mlt"], c1, c2, P)[1]), "RiEdge of the previous level"
    assert np.array_equal(rC, rt.cell_field(u, h, b, cs["mlt"], cs["mesh"], P)[1]), "RiCell of the previous level"
    cur = mk.richardson_number(md.Prog, time_level=1)
    assert not np.array_equal(rE, cur[0]) or not rE.any()


def forward(backend, meshname, K, plan=(P0,) * NSTEPS, mask=None, poison=None, mode="linear", variant=0, tag=""):
    ref = rt.run(meshname, K, plan, mask, poison, mode, settings(meshname, K, tag, mask), tag)
    md = model(backend, meshname, K, mask, poison, mode, variant, tag)
    cs = rt.case(meshname, K, mask, poison, mode)
    try:
        for s, P in enumerate(plan):
            if s == 0 or (P.key() if P else None) != (plan[s - 1].key() if plan[s - 1] else None):
                switch(md, P)
            md.eager(1)
            check(md, ref[s], P, poison)
            if P is not None:
                u0, h0 = (cs["state"][1], cs["state"][2]) if s == 0 else (ref[s - 1][2], ref[s - 1][3])
                check_previous_level(md, cs, P, u0, h0, ref[s][0][P.buoyancy])
        return md.Prog.normalVelocity[-1].get(), [md.tr.get(j) for j in range(rt.NT)], ref
    finally:
        md.close()


# ---- depths, meshes, kernel variants ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [60, 8, 3, 2])
def test_depths(backend, K):
    """planar (20 x 18): K = 60 the default stage kernel and the tile forms of both passes, 60 of 64 lanes of a column group; 8, 3: narrower
    groups; 2: one interface."""
    u, _, ref = forward(backend, "planar", K)
    assert (ref[-1][5] != 0.0).any() and (ref[-1][6] != 0.0).any()


def test_one_level_launches_nothing_and_has_the_bits_of_the_closure_off(backend):
    on = forward(backend, "planar", 1, (P0,) * 2, tag="forced")
    off = forward(backend, "planar", 1, (None,) * 2, tag="forced")
    assert np.array_equal(on[0], off[0]) and all(np.array_equal(a, b) for a, b in zip(on[1], off[1]))
    assert np.all(on[2][-1][5] == 0.0) and np.all(on[2][-1][6] == 0.0)


def test_column_forms_of_both_passes(backend):
    """K = 106: past the tiles of both passes, and two rounds of the 64 lanes of a column group."""
    assert mv.form_of(106) == 2 and tv.tile_columns(106) == 0
    forward(backend, "tiny-4-4", 106, (P0,) * 2)


def test_heptagons(backend):
    assert np.asarray(tc.get_mesh("ico12f").nEdgesOnCell).max() == 7
    forward(backend, "ico12f", 8)


def test_tiny_mesh(backend):
    forward(backend, "tiny-4-4", 60)


def test_odd_cell_count_and_odd_depth(backend):
    """35 cells x 35 levels: the tracers of the state lie an odd number of doubles apart, the buoyancy is the second of them."""
    name = tf.sheared_mesh(7, 5)
    assert tc.get_mesh(name).nCells == 35
    forward(backend, name, 35)


@pytest.mark.parametrize("variant", [0, 3, 4])
def test_kernel_variants(backend, variant):
    forward(backend, "planar", 8, variant=variant, tag="forced")


@pytest.mark.parametrize("mask", ["partial", "basin"])
def test_masks_with_nan_in_every_level_no_launch_reads(backend, mask):
    """NaN in u and in every tracer on poison_cases' sets; the active sets keep the bits of the clean run and stay finite."""
    u, phis, ref = forward(backend, "planar", 8, mask=mask, poison="step", tag="forced")
    clean = rt.run("planar", 8, (P0,) * NSTEPS, mask, None, "linear", settings("planar", 8, "forced", mask), "forced")
    cs = rt.case("planar", 8, mask)
    le = pc.active(cs["mesh"], cs["mlt"], 8, "edge")
    lc = np.arange(8)[None, :] < cs["nlev"][:, None]
    assert np.isfinite(u[le]).all() and np.array_equal(u[le], clean[-1][2][le])
    for j in range(rt.NT):
        assert np.isfinite(phis[j][lc]).all() and np.array_equal(phis[j][lc], clean[-1][1][j][lc])
    assert np.array_equal(ref[-1][5], clean[-1][5]) and np.array_equal(ref[-1][6], clean[-1][6])


@pytest.mark.parametrize("mask", ["partial", "basin"])
def test_the_closure_alone_reads_no_level_below_an_edge_or_a_cell(backend, mask):
    """moka_richardson_diagnose of a state with NaN in u at every k >= n_e and in the buoyancy at every k >= nLev[c]: all four outputs
    are finite and those of the twin."""
    K = 8
    cs = rt.case("planar", K, mask, "strict")
    md = tc.Model(backend, "planar", K, mlt=cs["mlt"], state=cs["state"])
    try:
        md.tr = mk.set_tracers(md.Prog, cs["fields"])
        switch(md, P0)
        _, u, h, _ = cs["state"]
        c1, c2 = mv.edge_cells(cs["mesh"])
        F, rE = rt.edge_field(u, h, cs["fields"][rt.JB], cs["mlt"], c1, c2, P0)
        G, rC = rt.cell_field(u, h, cs["fields"][rt.JB], cs["mlt"], cs["mesh"], P0)
        got = [np.full(a.shape, -1.0) for a in (rE, rC, F, G)]
        for level in (1, 0):
            L.check(L.lib().moka_richardson_diagnose(md.Prog._state._h, level, *(L.f64(a) for a in got)), backend._h)
            for a, b in zip(got, (rE, rC, F, G)):
                assert np.isfinite(a).all() and np.array_equal(a, b)
        only = np.full(G.shape, -1.0)
        L.check(L.lib().moka_richardson_diagnose(md.Prog._state._h, 1, None, None, None, L.f64(only)), backend._h)
        assert np.array_equal(only, G)
    finally:
        md.close()


# ---- combinations -------------------------------------------------------------------------------------------------------------------
def test_drag_stress_and_quadratic_drag_are_untouched(backend):
    u, _, ref = forward(backend, "planar", 60, tag="forced")
    bare = rt.run("planar", 60, (P0,) * NSTEPS)
    assert not np.array_equal(ref[-1][2], bare[-1][2])


@pytest.mark.parametrize("inside", [True, False], ids=["buoyancy-inside", "buoyancy-outside"])
def test_a_mask_leaves_one_tracer_on_its_scalar_and_one_on_its_field(backend, inside):
    """The set is the buoyancy alone (tracer 0 keeps its scalar kappaV, tracer 2 its uploaded field), or the unit tracer alone (the
    buoyancy keeps the exact zero of kappavs and is not mixed at all)."""
    P = rt.Params(rt.JB, tracers=[rt.JB] if inside else [0])
    _, _, ref = forward(backend, "planar", 8, (P,) * NSTEPS, tag="aside")
    full = rt.run("planar", 8, (P0,) * NSTEPS, None, None, "linear", settings("planar", 8, "aside"), "aside")
    assert not np.array_equal(ref[-1][1][2], full[-1][1][2])


def test_nonlinear_del2_del4_dycore(backend):
    forward(backend, "planar", 34, mode="del2+del4", tag="forced")


def test_tuning_key_7_keeps_the_16_stream_form_under_tracers(backend):
    """The 13-stream form never carries tracers (mk::rk13_usable), and the closure needs one: with the key set the step is the
    16-stream one, launch for launch."""
    lib = L.lib()
    L.check(lib.moka_set_tuning(7, 1))
    try:
        md = model(backend, "planar", 8)
        try:
            assert lib.moka_state_rk4_streams(md.Prog._state._h) == 16
        finally:
            md.close()
        forward(backend, "planar", 8)
    finally:
        L.check(lib.moka_set_tuning(7, 0))


def test_run_replays_the_closure_in_its_graph(backend):
    """Nine steps a run: one eager, a captured period replayed, the rest eager -- three runs with the parameters switched in between,
    each against the twin that switches them at the same steps (and unlike the twin that never switches)."""
    P1 = rt.Params(rt.JB, nu0=0.02, alpha=2.0, conv=0.1)
    plan = (P0,) * 9 + (P1,) * 9 + (P0,) * 9
    ref = rt.run("planar", 8, plan, None, None, "linear", settings("planar", 8, "forced"), "forced")
    wrong = rt.run("planar", 8, (P0,) * 27, None, None, "linear", settings("planar", 8, "forced"), "forced")
    assert not np.array_equal(ref[17][5], wrong[17][5]) and not np.array_equal(ref[26][2], wrong[26][2])
    md = model(backend, "planar", 8, tag="forced")
    try:
        for i, P in enumerate((P0, P1, P0)):          # a run after a switch never replays what was captured before it: every run
            switch(md, P)                             # against the twin's 27 steps, parameters switched where the runs switch them
            md.run(9)
            check(md, ref[9 * i + 8], P)
    finally:
        md.close()


def test_on_off_and_on_again_with_other_parameters(backend):
    """While the closure is off the set-aside nuV, viscosity field, kappaV and diffusivity field act again, bit for bit against the
    existing twins; F and G read zero behind such a step."""
    P1 = rt.Params(rt.JB, nu0=0.02, alpha=2.0, nuB=3e-4, kB=2e-5, conv=0.25, tracers=[0, rt.JB])
    _, _, ref = forward(backend, "planar", 8, (P0, None, P1, None), tag="aside")
    assert np.all(ref[1][5] == 0.0) and np.all(ref[3][6] == 0.0) and (ref[2][5] != 0.0).any()


def test_constant_buoyancy_is_a_scalar_run_of_the_same_library(backend):
    """The buoyancy is the unit tracer: F = nuB + nu0 and G = kB + (nuB + nu0) everywhere, and the state has the bits of a state of
    the same library that runs with those two scalars and never switched the closure on."""
    K, P = 8, rt.Params(0)
    nuV, kV = float(P.nuB + P.nu0), float(P.kB + (P.nuB + P.nu0))
    a, b = model(backend, "planar", K, "partial"), None
    try:
        b = model(backend, "planar", K, "partial")
        switch(a, P)
        mk.set_vertical_mixing(b.Prog, viscosity=nuV)
        b.tr.set_vertical_diffusivity(kV)
        for _ in range(NSTEPS):
            a.eager(1)
            b.eager(1)
        cs = rt.case("planar", K, "partial")
        F, G = mk.richardson_fields(a.Prog)
        assert np.all(F[np.arange(K)[None, :] < (cs["nn"] - 1)[:, None]] == nuV) and np.all(G[np.arange(K)[None, :] < (cs["nlev"] - 1)[:, None]] == kV)
        assert np.array_equal(a.Prog.normalVelocity[-1].get(), b.Prog.normalVelocity[-1].get())
        for j in range(rt.NT):
            assert np.array_equal(a.tr.get(j), b.tr.get(j))
        assert np.all(a.tr.get(0) == 1.0)                        # the unit tracer stays exactly 1.0
        assert np.all(mk.richardson_fields(b.Prog)[0] == 0.0)
    finally:
        a.close()
        if b is not None:
            b.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _params(**kw):
    d = dict(buoyancyTracer=rt.JB, nu0=0.005, alpha=5.0, nuBackground=1e-4, kappaBackground=1e-5, convective=1.0)
    d.update(kw)
    return L.RichardsonParams(d["buoyancyTracer"], d["nu0"], d["alpha"], d["nuBackground"], d["kappaBackground"], d["convective"], None)


def test_refusals_leave_the_state_as_it_was(backend):
    """Every refusal of the header that a state can reach.  The three moka_rk4_dist_* guards cannot be reached: those calls take a
    halo, moka_halo_create refuses a state with the closure on and the closure refuses a state with a halo, so the two never meet;
    the guards are not covered here or anywhere."""
    lib, ctx = L.lib(), backend._h
    md = model(backend, "tiny-4-4", 8, tag="aside")
    try:
        hS = md.Prog._state._h
        switch(md, P0)
        md.eager(1)
        before = (mk.richardson_mixing(md.Prog), mk.richardson_fields(md.Prog), md.Prog.normalVelocity[-1].get(), md.tr.get(rt.JB))

        def unchanged():
            now = (mk.richardson_mixing(md.Prog), mk.richardson_fields(md.Prog), md.Prog.normalVelocity[-1].get(), md.tr.get(rt.JB))
            assert now[0] == before[0] and all(np.array_equal(x, y) for x, y in zip(now[1], before[1]))
            assert np.array_equal(now[2], before[2]) and np.array_equal(now[3], before[3])

        for bad in (dict(nu0=-1.0), dict(alpha=float("nan")), dict(nuBackground=float("inf")), dict(kappaBackground=-0.5), dict(convective=float("nan")),
                    dict(buoyancyTracer=-1), dict(buoyancyTracer=rt.NT)):
            assert lib.moka_set_richardson_mixing(hS, C.byref(_params(**bad))) == L.ERR_ARG, bad
            unchanged()
        on, out = C.c_int(0), L.RichardsonParams()
        assert lib.moka_richardson_mixing(hS, None, C.byref(out), None) == L.ERR_ARG
        assert lib.moka_richardson_mixing(hS, C.byref(on), None, None) == L.ERR_ARG
        buf = np.zeros((md.mesh.nEdges, 8))
        assert lib.moka_richardson_diagnose(hS, 2, L.f64(buf), None, None, None) == L.ERR_ARG
        assert lib.moka_richardson_diagnose(hS, -1, L.f64(buf), None, None, None) == L.ERR_ARG
        assert lib.moka_step_rk4(hS, -md.dt) == L.ERR_ARG and b"Richardson" in lib.moka_last_error(ctx)
        assert lib.moka_run(hS, 1, -md.dt, 3, 0) == L.ERR_ARG and b"Richardson" in lib.moka_last_error(ctx)
        unchanged()
        other = C.c_void_p()
        z32, z64 = np.zeros(1, np.int32), np.zeros(1, np.int64)
        p32, p64 = z32.ctypes.data_as(C.POINTER(C.c_int32)), z64.ctypes.data_as(C.POINTER(C.c_int64))
        for name, call in (("moka_tape_create", lambda: lib.moka_tape_create(hS, 2, C.byref(other))),
                           ("moka_forced_tape_create", lambda: lib.moka_forced_tape_create(hS, 2, C.byref(other))),
                           ("moka_forced_tape_create_quadratic", lambda: lib.moka_forced_tape_create_quadratic(hS, 2, C.byref(other))),
                           ("moka_tracer_tape_create", lambda: lib.moka_tracer_tape_create(hS, 2, C.byref(other))),
                           ("moka_halo_create", lambda: lib.moka_halo_create(hS, 0, p32, p64, p32, p64, p32, p64, p32, p64, 0, 0, C.byref(other))),
                           ("moka_step_fe", lambda: lib.moka_step_fe(hS, md.dt, 0)),
                           ("moka_run", lambda: lib.moka_run(hS, 0, md.dt, 3, 0))):
            assert call() == L.ERR_UNSUPPORTED and not other.value, name
            assert b"Richardson closure" in lib.moka_last_error(ctx), name
            unchanged()
        # the setters of the set-aside coefficients keep working, with their own validation
        assert lib.moka_set_vertical_viscosity(hS, -1.0, 0.0) == L.ERR_ARG
        L.check(lib.moka_set_vertical_viscosity(hS, 2.0, 0.0), ctx)
        md.tr.set_vertical_diffusivity([1.0, 2.0, 3.0])
        unchanged()
        # moka_set_tracers switches the closure off
        L.check(lib.moka_set_tracers(hS, 2), ctx)
        assert mk.richardson_mixing(md.Prog) is None
        assert lib.moka_richardson_diagnose(hS, 1, L.f64(buf), None, None, None) == L.ERR_UNSUPPORTED
        assert np.all(mk.richardson_fields(md.Prog)[0] == 0.0)
        L.check(lib.moka_set_tracers(hS, 0), ctx)
        assert lib.moka_set_richardson_mixing(hS, C.byref(_params())) == L.ERR_ARG      # a state without tracers
        L.check(lib.moka_set_richardson_mixing(hS, None), ctx)                          # off on a state that is off: nothing
    finally:
        md.close()


def _refused(hS, ctx, word, Prog=None):
    """The set call returns MOKA_ERR_UNSUPPORTED with a message that names the closure and `word`, and the closure stays off."""
    lib = L.lib()
    assert lib.moka_set_richardson_mixing(hS, C.byref(_params())) == L.ERR_UNSUPPORTED
    msg = lib.moka_last_error(ctx)
    assert b"Richardson closure" in msg and word in msg, msg
    on, out = C.c_int(1), L.RichardsonParams()
    L.check(lib.moka_richardson_mixing(hS, C.byref(on), C.byref(out), None), ctx)
    assert on.value == 0
    if Prog is not None:
        assert np.all(mk.richardson_fields(Prog)[0] == 0.0)


def test_states_that_cannot_carry_the_closure(backend):
    """fp32 storage, a partitioned mesh, an existing moka_tape and a moka_forced_tape of either kind (none of these states can have
    tracers: the closure's own refusal comes first and says why), and a moka_tracer_tape, after whose destruction the closure is
    accepted; the state is destroyed with the closure on."""
    lib, ctx = L.lib(), backend._h
    md = tc.Model(backend, "tiny-4-4", 8, state_bytes=4)
    try:
        _refused(md.Prog._state._h, ctx, b"Float64")
    finally:
        md.close()
    mesh = tc.get_mesh("planar")
    # half the cells are another rank's (class 2): their patches are never launched -- a partitioned mesh, and no moka_halo on the state
    md = tc.Model(backend, "planar", 4, cell_class=np.where(np.arange(mesh.nCells) < mesh.nCells // 2, 1, 2).astype(np.int32))
    try:
        _refused(md.Prog._state._h, ctx, b"unpartitioned", md.Prog)
    finally:
        md.close()
    md = tc.Model(backend, "tiny-4-4", 8)
    try:
        hS, hT = md.Prog._state._h, C.c_void_p()
        u0 = md.Prog.normalVelocity[-1].get()
        for create, destroy in ((lib.moka_tape_create, lib.moka_tape_destroy), (lib.moka_forced_tape_create, lib.moka_forced_tape_destroy),
                                (lib.moka_forced_tape_create_quadratic, lib.moka_forced_tape_destroy)):
            hT = C.c_void_p()
            L.check(create(hS, 1, C.byref(hT)), ctx)
            _refused(hS, ctx, b"tape", md.Prog)
            assert np.array_equal(md.Prog.normalVelocity[-1].get(), u0)
            destroy(hT)
        cs = rt.case("tiny-4-4", 8)
        md.tr = mk.set_tracers(md.Prog, cs["fields"])
        hT = C.c_void_p()
        L.check(lib.moka_tracer_tape_create(hS, 1, C.byref(hT)), ctx)
        _refused(hS, ctx, b"tape", md.Prog)
        assert mk.richardson_mixing(md.Prog) is None
        lib.moka_tracer_tape_destroy(hT)
        L.check(lib.moka_set_richardson_mixing(hS, C.byref(_params())), ctx)
        md.eager(1)
    finally:
        md.close()                                               # (with the closure on: F, G and the tables go with the state)


def test_refused_on_a_rank_with_a_halo():
    """One rank of a two-way LocalCluster (a partitioned mesh with a moka_halo): the closure cannot be switched on, and says why."""
    from moka_hip import parallel as par
    mesh = tc.get_mesh("ico12f")
    ssh, u, h, rest = tc.random_state(mesh, 4, 12)
    cl = par.LocalCluster(mesh, ssh, u, h, rest, 20.0, 2, direct=False)
    try:
        _refused(cl.models[0].Prog._state._h, cl.models[0].Prog._state.mesh.backend._h, b"halo")
    finally:
        cl.close()


# ---- the one case the parent commit passes ---------------------------------------------------------------------------------------------
def test_a_state_that_never_switches_the_closure_on_equals_the_existing_reference():
    """Three tracers with their vertical diffusivities over the existing tracer reference: no call of this file's entry points."""
    backend = mk.MokaHIP(0)
    try:
        ref = tv.reference("planar", 8, "linear", False, 3, NSTEPS)
        md = tc.Model(backend, "planar", 8)
        try:
            tr = mk.set_tracers(md.Prog, ref["fields"], vertical=ref["kappaV"])
            for s in range(NSTEPS):
                md.eager(1)
                tc.check_tracers(tr, ref["forward"][s])
                tc.check_dycore(md.Prog, ref["forward"][s])
        finally:
            md.close()
    finally:
        backend.close()
