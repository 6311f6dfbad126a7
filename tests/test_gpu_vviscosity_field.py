"""A vertical viscosity per interface and edge on the device (moka_vertical_viscosity_field_upload; csrc/momentum_vmix.hip: the FIELD
instances of k_mvmix_tile / k_mvmix_column and of k_mvadj_tile / k_mvadj_column, the density DF): everything bit for bit against the
numpy twin of tests/momentum_vfield_twin.py.

A forward case names, per step, (switches, field): switches "nu", "drag", "stress" joined by "+" as in test_gpu_momentum_vmix.py (a
"nu" beside a field is the scalar that must not be read), field None (the scalar), "A" / "B" (momentum_vfield_twin.case_field with
seed 77 / 78: exact zeros, NaN in every never-read row), "zero" (zero at every active row) or "uniform" (nuV at every active row).  A
tape case adds a dt factor per step, one stress for the whole tape, the flags and a seed.  References are computed once and shared.
Every test calls an entry point the parent commit does not have."""
import ctypes as C

import numpy as np
import pytest

import forced_adjoint_twin as fa
import moka_hip as mk
import momentum_vfield_twin as mf
import momentum_vmix_twin as mv
import oracle as orc
import poison_cases as pc
import tracer_cases as tc
import tracer_vmix_twin as tv
from del4_twin import TwinState
from moka_hip import lib as L

pytestmark = pytest.mark.gpu
NSTEPS = 3
ALL = "drag+stress"
_REFS = {}


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)
    yield b
    b.close()


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def mask_of(meshname, K, mask):
    return None if not mask else pc.mask_of(meshname, K) if mask == "basin" else tc.partial_mlt(tc.get_mesh(meshname), K)


def depths(meshname, K, mask):
    m = mask_of(meshname, K, mask)
    return np.full(tc.get_mesh(meshname).nEdges, K) if m is None else np.asarray(m)


def settings(meshname, K, what):
    nu, r = mv.coefficients(meshname, K)
    parts = what.split("+") if what else []
    tau = mv.stress_field(tc.get_mesh(meshname), K) if "stress" in parts else None
    return (nu if "nu" in parts else 0.0), (r if "drag" in parts else 0.0), tau


def field_of(meshname, K, mask, name):
    if name is None:
        return None
    mlt, nE = depths(meshname, K, mask), tc.get_mesh(meshname).nEdges
    if name in ("A", "B"):
        return mf.case_field(meshname, K, mlt, 77 if name == "A" else 78)
    return mf.uniform_field(nE, K, mlt, 0.0 if name == "zero" else mv.coefficients(meshname, K)[0])


def start_state(meshname, K, mask, poison):
    ssh, u, h, rest = tc.state_of(meshname, K)
    if poison:
        u = pc.put(u, pc.edge_poison(tc.get_mesh(meshname), mask_of(meshname, K, mask), K, 1), "nan")
    return ssh, u, h, rest


def switch(md, meshname, what, fname, mask=False):
    nu, r, tau = settings(meshname, md.K, what)
    fld = field_of(meshname, md.K, mask, fname)
    mk.set_vertical_mixing(md.Prog, viscosity=nu, bottom_drag=r, surface_stress=tau, viscosity_field=fld)
    got, back = mk.vertical_mixing(md.Prog), mk.vertical_viscosity_field(md.Prog)
    assert len(got) == 3 and got[0] == nu and got[1] == r
    assert back is None if fld is None else pc.same(back, fld)             # rows that are never read come back as they went in


def reference(meshname, K, plan, mode="linear", mask=False, poison=False, s13=False):
    key = ("fwd", meshname, K, tuple(plan), mode, mask, poison, s13)
    if key not in _REFS:
        ssh, u, h, _ = start_state(meshname, K, mask, poison)
        tw = mf.momentum_twin(meshname, K, "linear" if s13 else mode, mask_of(meshname, K, mask))
        out = []
        if s13:
            st, nl = orc.OracleState(tw.tw.om, ssh, u, h), (orc.OracleNonlinear(tw.tw.om) if mode == "nonlinear" else None)
        else:
            st, phis = TwinState(ssh, u, h), [[], []]
        for what, fname in plan:
            tw.nu, tw.drag, tw.tau = settings(meshname, K, what)
            tw.fld = field_of(meshname, K, mask, fname)
            if s13:
                tw.step_s13(st, tc.dt_of(meshname), nl)
            else:
                tw.step_rk4(st, phis, tc.dt_of(meshname))
            out.append((None, None, st.u[1].copy(), st.h[1].copy(), st.ssh[1].copy()))
        _REFS[key] = out
    return _REFS[key]


def check(Prog, ref):
    a = Prog.normalVelocity[-1].get()
    assert pc.same(a, ref[2]), ("normalVelocity", pc.differences(a, ref[2]))
    assert np.array_equal(Prog.layerThickness[-1].get(), ref[3])
    assert np.array_equal(Prog.ssh[-1].get(), ref[4])


def forward(backend, meshname, K, plan, mode="linear", mask=False, variant=0, poison=False, path=None):
    ref = reference(meshname, K, plan, mode, mask, poison)
    md = tc.Model(backend, meshname, K, mode=mode, mlt=mask_of(meshname, K, mask), variant=variant, state=start_state(meshname, K, mask, poison))
    try:
        for s, (what, fname) in enumerate(plan):
            if s == 0 or plan[s] != plan[s - 1]:
                switch(md, meshname, what, fname, mask)
            md.eager(1)
            check(md.Prog, ref[s])
        assert mk.momentum_vmix_path(md.Prog) == (path if path is not None else mv.form_of(K, variant == 3))
        return md.Prog.normalVelocity[-1].get(), ref
    finally:
        md.close()


# ---- forward: levels, forms, switches -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 34, 35, 60])
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_levels_and_forms(backend, K, variant):
    """1080 edges: the last tile is short.  K = 2: one interface; 3: the first interior row; 34 .. 60: tiles of 32 edges; odd K: the
    8-byte lanes of the staging.  A scalar nuV is set beside the field and must not be read."""
    got, _ = forward(backend, "planar", K, (("nu+" + ALL, "A"),) * NSTEPS, variant=variant)
    scalar = reference("planar", K, (("nu+" + ALL, None),) * NSTEPS)
    assert not np.array_equal(got, scalar[-1][2])


@pytest.mark.parametrize("K,path", [(105, 1), (106, 2)])
def test_tile_and_column_boundary_is_unchanged(backend, K, path):
    assert mv.form_of(K) == path
    forward(backend, "tiny-4-4", K, ((ALL, "A"),), path=path)


@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_every_drag_and_stress_combination_with_a_field(backend, variant):
    """Partial columns, so that drag and stress meet n == 1 beside a field; the field is replaced and removed between steps."""
    forward(backend, "planar", 6, (("", "A"), ("drag", "A"), ("stress", "B"), (ALL, "B"), ("nu+" + ALL, None), (ALL, "A")), mask=True, variant=variant)


@pytest.mark.parametrize("K", [6, 34])
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
@pytest.mark.parametrize("mask", [True, "basin"], ids=["partial_mlt", "basin"])
def test_masks_nan_below_every_edge_and_in_the_never_read_rows(backend, K, variant, mask):
    mesh, mlt = tc.get_mesh("planar"), mask_of("planar", K, mask)
    assert (mlt == 0).any() and (mlt == 1).any() and (mlt == K).any()
    f = field_of("planar", K, mask, "A")
    assert np.all(np.isnan(f[~mf.live_of(mlt, K)])) and np.all(np.isfinite(f[mf.live_of(mlt, K)]))
    got, _ = forward(backend, "planar", K, ((ALL, "A"),) * NSTEPS, mask=mask, variant=variant, poison=True)
    fill, live = pc.edge_poison(mesh, mlt, K, 1), pc.active(mesh, mlt, K, "edge")
    assert np.all(np.isnan(got[fill])) and np.all(np.isfinite(got[live]))
    clean = reference("planar", K, ((ALL, "A"),) * NSTEPS, mask=mask)
    assert np.array_equal(got[live], clean[-1][2][live])


@pytest.mark.parametrize("K", [5, 34])
def test_pentagons_and_heptagons(backend, K):
    forward(backend, "ico12f", K, ((ALL, "A"),) * NSTEPS)


def test_ico16(backend):
    forward(backend, "ico16", 5, ((ALL, "A"),) * 2)


@pytest.mark.parametrize("mode", ["nonlinear", "del2+del4"])
def test_dycores(backend, mode):
    forward(backend, "planar", 34, ((ALL, "A"),) * NSTEPS, mode=mode)


@pytest.mark.parametrize("mode", ["linear", "nonlinear"])
def test_13_stream_form(backend, mode):
    plan = ((ALL, "A"),) * NSTEPS
    ref = reference("planar", 34, plan, mode, s13=True)
    lib = L.lib()
    L.check(lib.moka_set_tuning(7, 1))
    try:
        md = tc.Model(backend, "planar", 34, mode=mode)
        try:
            assert lib.moka_state_rk4_streams(md.Prog._state._h) == 13
            switch(md, "planar", *plan[0])
            for s in range(NSTEPS):
                md.eager(1)
                check(md.Prog, ref[s])
            assert mk.momentum_vmix_path(md.Prog) == 1
        finally:
            md.close()
    finally:
        L.check(lib.moka_set_tuning(7, 0))


def test_run_replays_its_graph_across_an_upload_a_replacement_and_a_removal(backend):
    """Nine steps a run, as the scalar pass's graph test takes: moka_run steps once eagerly, captures a period of steps and replays it,
    so every run below launches the FIELD instances under capture and replay with the field then in force."""
    n = 9
    plan = ((ALL, "A"),) * n + ((ALL, "B"),) * n + (("nu+" + ALL, None),) * n + ((ALL, "A"),) * n
    ref = reference("planar", 3, plan)
    md = tc.Model(backend, "planar", 3)
    try:
        for i in range(4):
            switch(md, "planar", *plan[n * i])
            md.run(n)
            check(md.Prog, ref[n * i + n - 1])
    finally:
        md.close()


def test_tracers_beside_the_pass(backend):
    """Tracers never see the pass inside a step; from the next step on they ride the flow the field mixed."""
    meshname, K = "planar", 34
    mesh = tc.get_mesh(meshname)
    tw = mf.momentum_twin(meshname, K)
    tw.nu, tw.drag, tw.tau = settings(meshname, K, ALL)
    tw.fld = field_of(meshname, K, False, "A")
    tw.tw.kappa, tw.tw.kappa4, tw.tw.kappaV = tc.kappas(meshname, 9)[:2], [0.0, 0.0], tv.kappavs(meshname, K, 9)[:2]
    tw.tw.source = [None, None]
    ssh, u, h, _ = tc.state_of(meshname, K)
    st = TwinState(ssh, u, h)
    f = tc.distinct_fields(mesh, K, 9)[:2]
    phis = [[a.copy() for a in f], [a.copy() for a in f]]
    md = tc.Model(backend, meshname, K)
    try:
        tr_ = mk.set_tracers(md.Prog, f, diffusivity=tw.tw.kappa, vertical=tw.tw.kappaV)
        switch(md, meshname, ALL, "A")
        for s in range(2):
            tw.step_rk4(st, phis, tc.dt_of(meshname))
            md.eager(1)
            tc.check_tracers(tr_, ([a.copy() for a in phis[0]], [a.copy() for a in phis[1]], st.u[1], st.h[1], st.ssh[1]))
            check(md.Prog, (None, None, st.u[1], st.h[1], st.ssh[1]))
        assert mk.momentum_vmix_path(md.Prog) == 1 and tr_.vmix_path() == 1
    finally:
        md.close()


# ---- identities ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_a_uniform_field_gives_the_scalars_bits_and_removal_restores_them(backend, variant):
    scalar = reference("planar", 34, (("nu+" + ALL, None),) * 4)
    md = tc.Model(backend, "planar", 34, variant=variant)
    try:
        switch(md, "planar", ALL, "uniform")
        md.eager(2)
        check(md.Prog, scalar[1])
        switch(md, "planar", "nu+" + ALL, "A")
        switch(md, "planar", "nu+" + ALL, None)              # removed before any step ran with it: the scalar acts again
        assert mk.vertical_viscosity_field(md.Prog) is None
        md.eager(2)
        check(md.Prog, scalar[3])
    finally:
        md.close()


def test_an_all_zero_field_sets_nu_aside_and_switches_the_pass_off(backend):
    plain = tc.reference("planar", 34, "linear", False, ((NSTEPS, 0, False),))
    md = tc.Model(backend, "planar", 34)
    lib, sh = L.lib(), md.Prog._state._h
    try:
        switch(md, "planar", "nu", "zero")
        has = C.c_int(0)
        assert lib.moka_has_vertical_viscosity_field(sh, C.byref(has)) == 0 and has.value == 1
        for s in range(NSTEPS):
            md.eager(1)
            tc.check_dycore(md.Prog, plain[s])
        assert mk.momentum_vmix_path(md.Prog) == 0
        assert lib.moka_step_rk4(sh, -md.dt) == 0                # the pass is off: a negative dt is allowed
    finally:
        md.close()
    drag = reference("planar", 34, (("drag", None),) * 2)
    md = tc.Model(backend, "planar", 34)
    try:
        switch(md, "planar", "nu+drag", "zero")
        md.eager(2)
        check(md.Prog, drag[1])
    finally:
        md.close()


# ---- the tape -----------------------------------------------------------------------------------------------------------------------
def tape_reference(meshname, K, plan, stress="stress", want=7, want_field=True, mask=False, seed=None, poison=False):
    key = ("tape", meshname, K, tuple(plan), stress, want, want_field, mask, seed, poison)
    if key not in _REFS:
        om = tc.oracle_mesh(meshname, K, False, mask_of(meshname, K, mask))
        ssh, u, h, _ = start_state(meshname, K, mask, poison)
        tw = mf.ForcedFieldTwin(om, ssh, u, h, want, want_field)
        tw.tau = mv.stress_field(tc.get_mesh(meshname), K) if stress else None
        fwd = []
        for what, fname, fac in plan:
            tw.nu, tw.drag, _ = settings(meshname, K, what)
            tw.fld = field_of(meshname, K, mask, fname)
            tw.step(fac * tc.dt_of(meshname))
            fwd.append((None, None, tw.st.u[1].copy(), tw.st.h[1].copy(), tw.st.ssh[1].copy()))
        X0 = tw.seed_sum_sq_ssh() if seed is None else free_seed(meshname, K, mask, seed, poison)
        XU, XH = tw.sweep(*X0)
        _REFS[key] = {"forward": fwd, "XU": XU, "XH": XH, "dens": {b: d.copy() for b, d in tw.dens.items()},
                      "DF": None if tw.DF is None else tw.DF.copy()}
    return _REFS[key]


def free_seed(meshname, K, mask, seed, poison):
    mesh = tc.get_mesh(meshname)
    rng = np.random.default_rng(seed)
    XU, XH = rng.uniform(-1, 1, (mesh.nEdges, K)), rng.uniform(-1, 1, (mesh.nCells, K))
    if poison:
        XU[np.arange(K)[None, :] >= np.minimum(mask_of(meshname, K, mask), K)[:, None]] = np.nan
    return XU, XH


def taped(backend, meshname, K, plan, stress="stress", want=7, want_field=True, mask=False, seed=None, poison=False, variant=0):
    """Runs the case on the device and compares the forward steps, X, the three densities and DF with the twin; returns (g, path)."""
    ref = tape_reference(meshname, K, plan, stress, want, want_field, mask, seed, poison)
    md = tc.Model(backend, meshname, K, mlt=mask_of(meshname, K, mask), variant=variant, state=start_state(meshname, K, mask, poison))
    try:
        tau = mv.stress_field(tc.get_mesh(meshname), K) if stress else None
        mk.set_vertical_mixing(md.Prog, surface_stress=tau)
        tape = mk.ForcedAdjointTape(md.Prog, len(plan))
        try:
            tape.want_gradient(stress=bool(want & 1), viscosity=bool(want & 2), drag=bool(want & 4), viscosity_field=want_field)
            for s, (what, fname, fac) in enumerate(plan):
                nu, r, _ = settings(meshname, K, what)
                upload(md, meshname, K, mask, nu, r, fname)
                tape.step(fac * md.dt)
                check(md.Prog, ref["forward"][s])
            g = tape.gradient(None if seed is None else free_seed(meshname, K, mask, seed, poison))
            assert pc.same(g["normalVelocity"], ref["XU"]), ("XU", pc.differences(g["normalVelocity"], ref["XU"]))
            assert pc.same(g["layerThickness"], ref["XH"]), ("XH", pc.differences(g["layerThickness"], ref["XH"]))
            for bit, name in ((1, "surfaceStress"), (2, "viscosity"), (4, "bottomDrag")):
                if want & bit:
                    d = tape.density(name)
                    assert pc.same(d, ref["dens"][bit]), (name, pc.differences(d, ref["dens"][bit]))
            assert ("viscosityField" in g) == want_field
            if want_field:
                assert pc.same(g["viscosityField"], ref["DF"]), ("DF", pc.differences(g["viscosityField"], ref["DF"]))
                assert np.array_equal(tape.density("viscosityField"), g["viscosityField"])
            return g, tape.vmix_path()
        finally:
            tape.close()
    finally:
        md.close()


def upload(md, meshname, K, mask, nu, r, fname):
    """Between recorded steps: the scalars and the field through the C ABI (a stress upload is refused while steps are recorded)."""
    lib, sh = L.lib(), md.Prog._state._h
    L.check(lib.moka_set_vertical_viscosity(sh, nu, r), md.backend._h)
    fld = field_of(meshname, K, mask, fname)
    L.check(lib.moka_vertical_viscosity_field_upload(sh, None if fld is None else L.f64(fld)), md.backend._h)


FIELD2 = (("drag", "A", 1.0),) * 2


@pytest.mark.parametrize("K", [2, 3, 34, 60])
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_transpose_levels_and_forms(backend, K, variant):
    g, path = taped(backend, "planar", K, FIELD2, variant=variant)
    assert path == mf.adjoint_form(K, True, variant == 3)[0]
    assert np.any(g["viscosityField"] != 0.0) and g["viscosity"] != 0.0
    live = mf.live_of(depths("planar", K, False), K)
    assert np.all(g["viscosityField"][~live] == 0.0)                        # the row K - 1 is never written


@pytest.mark.parametrize("K", [15, 16, 63, 64])
def test_both_sides_of_the_five_set_boundaries(backend, K):
    """64-column tiles to K = 15, 32-column tiles to 63, the column form from 64 (48 edges: fewer than a tile)."""
    assert [mf.adjoint_form(k, True) for k in (15, 16, 63, 64)] == [(1, 64), (1, 32), (1, 32), (2, 0)]
    g, path = taped(backend, "tiny-4-4", K, FIELD2)             # (two steps: the seed's XU is zero, so one step alone leaves DF zero)
    assert path == mf.adjoint_form(K, True)[0] and np.any(g["viscosityField"] != 0.0)


def test_a_step_without_a_field_keeps_the_four_set_tile_at_79(backend):
    K = 79
    assert mf.adjoint_form(K, False) == (1, 32) and mf.adjoint_form(K, True) == (2, 0)
    md = tc.Model(backend, "tiny-4-4", K)
    try:
        tape = mk.ForcedAdjointTape(md.Prog, 1)
        try:
            tape.want_gradient(viscosity=True, viscosity_field=True)
            for fname, path in ((None, 1), ("A", 2), (None, 1)):
                upload(md, "tiny-4-4", K, False, mv.coefficients("tiny-4-4", K)[0], 0.0, fname)
                tape.step(md.dt)
                tape.gradient()
                assert tape.vmix_path() == path
        finally:
            tape.close()
    finally:
        md.close()


def test_free_seed_and_the_field_changing_between_recorded_steps(backend):
    """Upload, replace, keep, remove, an all-zero field, a step with dt == 0: each reversed step takes the field it ran with."""
    plan = (("drag", "A", 1.0), ("drag", "B", 1.0), ("nu+drag", "B", 0.5), ("nu+drag", None, 1.0), ("drag", "A", 0.0), ("nu", "zero", 1.0),
            ("", "A", 1.0))
    for variant in (0, 3):
        taped(backend, "planar", 6, plan, seed=23, mask=True, variant=variant)


@pytest.mark.parametrize("plan", [(("nu+drag", None, 1.0),) * 2, (("", None, 1.0),) * 2], ids=["scalar", "pass-off"])
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_DF_with_a_scalar_only_and_with_the_pass_off(backend, plan, variant):
    stress = "stress" if plan[0][0] else None
    g, path = taped(backend, "planar", 34, plan, stress=stress, variant=variant)
    assert np.any(g["viscosityField"] != 0.0) and path == mf.adjoint_form(34, False, variant == 3)[0]
    plainref = tape_reference("planar", 34, plan, stress, 0, False)
    assert np.array_equal(g["normalVelocity"], plainref["XU"]) and np.array_equal(g["layerThickness"], plainref["XH"])


@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_a_flagged_sweep_leaves_X_with_the_unflagged_bits(backend, variant):
    flagged, _ = taped(backend, "planar", 34, FIELD2, want=0, want_field=True, variant=variant)
    plain, _ = taped(backend, "planar", 34, FIELD2, want=0, want_field=False, variant=variant)
    assert np.array_equal(flagged["normalVelocity"], plain["normalVelocity"]) and np.array_equal(flagged["layerThickness"], plain["layerThickness"])


@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
@pytest.mark.parametrize("mask", [True, "basin"], ids=["partial_mlt", "basin"])
def test_transpose_masks_and_nan(backend, variant, mask):
    K = 34
    mlt = mask_of("planar", K, mask)
    g, _ = taped(backend, "planar", K, FIELD2, mask=mask, seed=17, poison=True, variant=variant)
    live = mf.live_of(mlt, K)
    assert np.all(np.isfinite(g["viscosityField"])) and np.all(g["viscosityField"][~live] == 0.0)
    assert np.all(np.isfinite(g["surfaceStress"])) and np.isfinite(g["viscosity"])


def test_transpose_on_pentagons_and_heptagons(backend):
    taped(backend, "ico12f", 34, FIELD2)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_bad_values_at_active_rows_only_and_nothing_changes(backend):
    K = 6
    md = tc.Model(backend, "planar", K, mlt=mask_of("planar", K, True))
    lib, sh, ctx = L.lib(), md.Prog._state._h, md.backend._h
    try:
        switch(md, "planar", ALL, "A", True)
        md.eager(1)
        mlt = depths("planar", K, True)
        good = field_of("planar", K, True, "A")
        e = int(np.nonzero(mlt >= 3)[0][0])
        u0 = md.Prog.normalVelocity[-1].get()
        for bad in (-1.0, np.nan, np.inf, -np.inf):
            f = np.nan_to_num(good, nan=-5.0)                                 # inactive rows are not inspected: negative there is fine
            assert lib.moka_vertical_viscosity_field_upload(sh, L.f64(f)) == 0
            f[e, 1] = bad
            assert lib.moka_vertical_viscosity_field_upload(sh, L.f64(f)) == L.ERR_ARG
            assert b"vertical viscosity field" in lib.moka_last_error(ctx)
            f[e, 1] = good[e, 1]
            assert pc.same(mk.vertical_viscosity_field(md.Prog), np.nan_to_num(good, nan=-5.0))
        L.check(lib.moka_vertical_viscosity_field_upload(sh, L.f64(good)), ctx)
        assert lib.moka_vertical_viscosity_field_download(sh, None) == L.ERR_ARG
        assert lib.moka_has_vertical_viscosity_field(sh, None) == L.ERR_ARG
        assert lib.moka_vertical_viscosity_field_upload(None, L.f64(good)) == L.ERR_ARG
        assert np.array_equal(md.Prog.normalVelocity[-1].get(), u0, equal_nan=True)
        assert lib.moka_step_rk4(sh, -md.dt) == L.ERR_ARG                   # a field turned the pass on: dt < 0 is refused
        md.eager(1)
        check(md.Prog, reference("planar", K, ((ALL, "A"),) * 2, mask=True)[1])
        # no field: the download gives zeros
        L.check(lib.moka_vertical_viscosity_field_upload(sh, None), ctx)
        out = np.ones((md.mesh.nEdges, K))
        L.check(lib.moka_vertical_viscosity_field_download(sh, L.f64(out)), ctx)
        assert np.all(out == 0.0)
    finally:
        md.close()


def test_unsupported_where_the_scalar_is(backend):
    md = tc.Model(backend, "planar", 6)
    lib, sh, ctx = L.lib(), md.Prog._state._h, md.backend._h
    try:
        f = field_of("planar", 6, False, "A")
        # everything that is refused while the pass is on is refused when a field turned it on
        L.check(lib.moka_vertical_viscosity_field_upload(sh, L.f64(f)), ctx)
        assert lib.moka_step_fe(sh, md.dt, L.FE_REFERENCE_COMPAT) == L.ERR_UNSUPPORTED
        t = C.c_void_p()
        assert lib.moka_tape_create(sh, 2, C.byref(t)) == L.ERR_UNSUPPORTED and not t.value
        L.check(lib.moka_vertical_viscosity_field_upload(sh, None), ctx)
        tape = mk.AdjointTape(md.Prog, 2)
        assert lib.moka_vertical_viscosity_field_upload(sh, L.f64(f)) == L.ERR_UNSUPPORTED
        assert b"moka_tape" in lib.moka_last_error(ctx) and mk.vertical_viscosity_field(md.Prog) is None
        tape.close()
        L.check(lib.moka_vertical_viscosity_field_upload(sh, L.f64(f)), ctx)
        # a removal that would let a nuV != 0 act beside a moka_tape: an all-zero field sets nuV aside, so the pass is off and the tape is
        # accepted; taking the field away would switch the pass on behind the tape's back and is refused, with the field left in place
        zero = field_of("planar", 6, False, "zero")
        L.check(lib.moka_vertical_viscosity_field_upload(sh, L.f64(zero)), ctx)
        L.check(lib.moka_set_vertical_viscosity(sh, 5.0, 0.0), ctx)
        tape = mk.AdjointTape(md.Prog, 2)
        assert lib.moka_vertical_viscosity_field_upload(sh, None) == L.ERR_UNSUPPORTED
        assert b"moka_tape" in lib.moka_last_error(ctx) and pc.same(mk.vertical_viscosity_field(md.Prog), zero)
        assert lib.moka_set_vertical_viscosity(sh, 0.0, 0.0) == 0                       # with nuV == 0 nothing would act: the removal goes through
        assert lib.moka_vertical_viscosity_field_upload(sh, None) == 0 and mk.vertical_viscosity_field(md.Prog) is None
        assert lib.moka_vertical_viscosity_field_upload(sh, None) == 0                   # nothing to remove: nothing happens
        tape.close()
        with pytest.raises(ValueError):                                                  # a bad shape changes nothing
            mk.set_vertical_mixing(md.Prog, viscosity=3.0, bottom_drag=1.0, viscosity_field=np.ones((md.mesh.nEdges, 5)))
        assert mk.vertical_mixing(md.Prog)[:2] == (0.0, 0.0)
    finally:
        md.close()
    f32 = tc.Model(backend, "ico16", 4, state_bytes=4)
    try:
        fh = f32.Prog._state._h
        assert lib.moka_vertical_viscosity_field_upload(fh, L.f64(np.ones((f32.mesh.nEdges, 4)))) == L.ERR_UNSUPPORTED
        assert b"Float64" in lib.moka_last_error(ctx)
        assert lib.moka_vertical_viscosity_field_upload(fh, None) == 0
    finally:
        f32.close()


def test_refused_on_a_rank_with_a_halo():
    from moka_hip import parallel as par
    mesh = tc.get_mesh("ico12f")
    K = 4
    ssh, u, h, rest = tc.random_state(mesh, K, 12)
    cl = par.LocalCluster(mesh, ssh, u, h, rest, 20.0, 2, direct=False)
    try:
        st = cl.models[0].Prog._state
        nE = st.mesh.HorzMesh.data.nEdges
        assert L.lib().moka_vertical_viscosity_field_upload(st._h, L.f64(np.ones((nE, K)))) == L.ERR_UNSUPPORTED
        assert L.lib().moka_vertical_viscosity_field_upload(st._h, None) == 0
    finally:
        cl.close()


def test_the_flag_with_recorded_steps_and_a_download_without_the_flag(backend):
    md = tc.Model(backend, "planar", 6)
    lib, ctx = L.lib(), md.backend._h
    try:
        tape = mk.ForcedAdjointTape(md.Prog, 2)
        try:
            out = np.zeros((md.mesh.nEdges, 6))
            assert lib.moka_forced_adjoint_viscosity_field_density_download(tape._h, L.f64(out)) == L.ERR_ARG
            assert lib.moka_forced_adjoint_want_viscosity_field_gradient(None, 1) == L.ERR_ARG
            assert lib.moka_forced_adjoint_want_gradient(tape._h, 8, 1) == L.ERR_ARG         # the field has calls of its own
            L.check(lib.moka_forced_adjoint_want_viscosity_field_gradient(tape._h, 1), ctx)
            assert lib.moka_forced_adjoint_viscosity_field_density_download(tape._h, None) == L.ERR_ARG
            tape.step(md.dt)
            assert lib.moka_forced_adjoint_want_viscosity_field_gradient(tape._h, 0) == L.ERR_ARG
            assert lib.moka_forced_adjoint_want_viscosity_field_gradient(tape._h, 1) == L.ERR_ARG
            assert b"no step is recorded" in lib.moka_last_error(ctx)
            tape.gradient()
            L.check(lib.moka_forced_adjoint_want_viscosity_field_gradient(tape._h, 0), ctx)
            assert lib.moka_forced_adjoint_viscosity_field_density_download(tape._h, L.f64(out)) == L.ERR_ARG
        finally:
            tape.close()
    finally:
        md.close()


# ---- order of calls -------------------------------------------------------------------------------------------------------------------
def test_one_seeded_sequence_of_calls_against_the_eager_twin(backend):
    """Twenty-two calls drawn with a fixed seed -- field uploads and removals, scalar changes, plain steps, taped steps, sweeps --
    mirrored call by call on ForcedFieldTwin; the state after every step and X, the densities and DF after every sweep are the twin's."""
    meshname, K, mask = "planar", 6, True
    rng = np.random.default_rng(1)           # the first seed whose draw holds every kind of call and a sweep over field and scalar steps
    ops = [str(o) for o in rng.choice(["A", "B", "zero", "remove", "scalar", "step", "taped", "taped", "taped", "sweep"], 20)] + ["taped", "sweep"]
    assert {"A", "B", "zero", "remove", "scalar", "step", "taped", "sweep"} <= set(ops) and ops.count("sweep") >= 3
    nu0, r0 = mv.coefficients(meshname, K)
    tau = mv.stress_field(tc.get_mesh(meshname), K)
    om = tc.oracle_mesh(meshname, K, False, mask_of(meshname, K, mask))
    ssh, u, h, _ = tc.state_of(meshname, K)
    tw = mf.ForcedFieldTwin(om, ssh, u, h, 7, True)
    tw.tau = tau
    md = tc.Model(backend, meshname, K, mlt=mask_of(meshname, K, mask))
    lib, sh, ctx = L.lib(), md.Prog._state._h, md.backend._h
    try:
        mk.set_vertical_mixing(md.Prog, surface_stress=tau)
        tape = mk.ForcedAdjointTape(md.Prog, len(ops))
        try:
            tape.want_gradient(stress=True, viscosity=True, drag=True, viscosity_field=True)
            for i, op in enumerate(ops):
                if op in ("A", "B", "zero"):
                    tw.fld = field_of(meshname, K, mask, op)
                    L.check(lib.moka_vertical_viscosity_field_upload(sh, L.f64(tw.fld)), ctx)
                elif op == "remove":
                    tw.fld = None
                    L.check(lib.moka_vertical_viscosity_field_upload(sh, None), ctx)
                elif op == "scalar":
                    tw.nu, tw.drag = float(rng.choice([0.0, nu0, 2 * nu0])), float(rng.choice([0.0, r0]))
                    L.check(lib.moka_set_vertical_viscosity(sh, tw.nu, tw.drag), ctx)
                elif op in ("step", "taped"):
                    tw.step(md.dt)
                    if op == "step":                   # not recorded: the twin drops its record of the step
                        tw.recs.pop(); tw.rk.tape.pop()
                        md.eager(1)
                    else:
                        tape.step(md.dt)
                    check(md.Prog, (None, None, tw.st.u[1], tw.st.h[1], tw.st.ssh[1]))
                else:
                    XU, XH = tw.sweep(*tw.seed_sum_sq_ssh())
                    g = tape.gradient()
                    assert pc.same(g["normalVelocity"], XU) and pc.same(g["layerThickness"], XH), (i, op)
                    assert pc.same(g["viscosityField"], tw.DF), (i, pc.differences(g["viscosityField"], tw.DF))
                    for bit, name in ((1, "surfaceStress"), (2, "viscosity"), (4, "bottomDrag")):
                        assert pc.same(tape.density(name), tw.dens[bit]), (i, name)
        finally:
            tape.close()
    finally:
        md.close()
