"""Reverse mode through the forced RK4 step on the device (moka_forced_tape; csrc/momentum_vmix.hip: k_mvadj_tile, k_mvadj_column,
k_mvadj_gather): X, the three densities and the two scalar gradients bit for bit against the numpy twin of tests/forced_adjoint_twin.py.

A case is a plan, one entry per recorded step: (switches, dt factor) with switches "nu", "drag" joined by "+" or "" -- the values in
force change between steps -- plus one stress for the whole tape ("stress", "stress0": every third edge exactly 0.0, "zero": all zero,
None), the gradient flags, a mask and a seed: None = d sum(ssh^2), or a seed number for the free seed.  The coefficients are
momentum_vmix_twin's.  Every test fails without the feature: the symbols do not exist there."""
import ctypes as C

import numpy as np
import pytest

import forced_adjoint_twin as fa
import moka_hip as mk
import momentum_vmix_twin as mv
import poison_cases as pc
import tracer_cases as tc
import tracer_vfield_twin as tf
from moka_hip import lib as L

pytestmark = pytest.mark.gpu
FULL = (("nu+drag", 1.0),) * 2
_REFS = {}


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)
    yield b
    b.close()


# ---- the forms, from vmix_kernel's formula with four column sets ----------------------------------------------------------------------
def tile_columns(K, generic=False, sets=4):
    cs = K | 1
    if not generic and K >= 2:
        for t, fit in ((64, 4), (32, 2)):
            if (sets * t * cs * 8 + 4 * t) * fit <= 160 * 1024:
                return t
    return 0


def boundaries():
    """The largest K of 64-column tiles and of the tile form, each with its successor."""
    k64 = max(K for K in range(2, 300) if tile_columns(K) == 64)
    k32 = max(K for K in range(2, 300) if tile_columns(K) == 32)
    return [k64, k64 + 1, k32, k32 + 1]


def form_of(K, variant):
    return 1 if tile_columns(K, variant == 3) else 2


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def coefficients(meshname, K, what):
    nu, r = mv.coefficients(meshname, K)
    parts = what.split("+") if what else []
    return (nu if "nu" in parts else 0.0), (r if "drag" in parts else 0.0)


def stress_of(meshname, K, stress):
    mesh = tc.get_mesh(meshname)
    if stress is None:
        return None
    if stress == "zero":
        return np.zeros(mesh.nEdges)
    return mv.stress_field(mesh, K, zeros=stress == "stress0")


def mask_of(meshname, K, mask):
    return None if not mask else pc.mask_of(meshname, K) if mask == "basin" else tc.partial_mlt(tc.get_mesh(meshname), K)


def start_state(meshname, K, mask, poison):
    ssh, u, h, rest = tc.state_of(meshname, K)
    if poison:
        u = pc.put(u, pc.edge_poison(tc.get_mesh(meshname), mask_of(meshname, K, mask), K, 1), "nan")
    return ssh, u, h, rest


def seed_of(meshname, K, mask, seed, poison):
    """The free seed: random everywhere, the rows below an edge's depth included (NaN there with poison)."""
    mesh = tc.get_mesh(meshname)
    rng = np.random.default_rng(seed)
    XU, XH = rng.uniform(-1, 1, (mesh.nEdges, K)), rng.uniform(-1, 1, (mesh.nCells, K))
    if poison:
        mlt = mask_of(meshname, K, mask)
        XU[np.arange(K)[None, :] >= np.minimum(mlt, K)[:, None]] = np.nan
    return XU, XH


def reference(meshname, K, plan=FULL, stress="stress", want=7, mask=False, seed=None, poison=False):
    key = (meshname, K, tuple(plan), stress, want, mask, seed, poison)
    if key not in _REFS:
        om = tc.oracle_mesh(meshname, K, False, mask_of(meshname, K, mask))
        ssh, u, h, _ = start_state(meshname, K, mask, poison)
        tw = fa.ForcedTwin(om, ssh, u, h, want)
        tw.tau = stress_of(meshname, K, stress)
        fwd = []
        for what, f in plan:
            tw.nu, tw.drag = coefficients(meshname, K, what)
            tw.step(f * tc.dt_of(meshname))
            fwd.append((tw.st.u[1].copy(), tw.st.h[1].copy(), tw.st.ssh[1].copy()))
        X0 = tw.seed_sum_sq_ssh() if seed is None else seed_of(meshname, K, mask, seed, poison)
        XU, XH = tw.sweep(*X0)
        _REFS[key] = {"forward": fwd, "XU": XU, "XH": XH, "grad": tw.gradients(), "dens": {b: d.copy() for b, d in tw.dens.items()}}
    return _REFS[key]


def device(backend, meshname, K, plan=FULL, stress="stress", want=7, mask=False, seed=None, poison=False, variant=0, check_forward=True):
    """Runs the case on the device and compares everything with the twin; returns (gradient dict, path)."""
    ref = reference(meshname, K, plan, stress, want, mask, seed, poison)
    md = tc.Model(backend, meshname, K, mlt=mask_of(meshname, K, mask), variant=variant, state=start_state(meshname, K, mask, poison))
    lib, sh = L.lib(), md.Prog._state._h
    try:
        tau = stress_of(meshname, K, stress)
        mk.set_vertical_mixing(md.Prog, surface_stress=tau)
        tape = mk.ForcedAdjointTape(md.Prog, len(plan))
        try:
            assert tape.vmix_path() == 0
            tape.want_gradient(stress=bool(want & 1), viscosity=bool(want & 2), drag=bool(want & 4))
            for s, (what, f) in enumerate(plan):
                L.check(lib.moka_set_vertical_viscosity(sh, *coefficients(meshname, K, what)), backend._h)
                tape.step(f * md.dt)
                if check_forward:
                    a = md.Prog.normalVelocity[-1].get()
                    assert pc.same(a, ref["forward"][s][0]), ("normalVelocity", s, pc.differences(a, ref["forward"][s][0]))
                    assert np.array_equal(md.Prog.layerThickness[-1].get(), ref["forward"][s][1])
                    assert np.array_equal(md.Prog.ssh[-1].get(), ref["forward"][s][2])
            g = tape.gradient(None if seed is None else seed_of(meshname, K, mask, seed, poison))
            path = tape.vmix_path()
            assert pc.same(g["normalVelocity"], ref["XU"]), ("XU", pc.differences(g["normalVelocity"], ref["XU"]))
            assert pc.same(g["layerThickness"], ref["XH"]), ("XH", pc.differences(g["layerThickness"], ref["XH"]))
            for bit, name in ((1, "surfaceStress"), (2, "viscosity"), (4, "bottomDrag")):
                assert (name in g) == bool(want & bit)
                if want & bit:
                    d = tape.density(name)
                    assert pc.same(d, ref["dens"][bit]), (name, pc.differences(d, ref["dens"][bit]))
                    if bit == 1:
                        assert np.array_equal(g[name], d)
                    else:
                        assert g[name] == ref["grad"][name] and g[name] == fa.host_sum(d)
            return g, path
        finally:
            tape.close()
    finally:
        md.close()


# ---- levels and forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 34, 60])
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_levels_and_forms(backend, K, variant):
    """1080 edges: the last tile is short.  K = 1: the n == 1 rows alone.  Both forms give the twin's bits, hence each other's."""
    g, path = device(backend, "planar", K, variant=variant)
    assert path == form_of(K, variant)
    assert np.any(g["surfaceStress"] != 0.0) and g["bottomDrag"] != 0.0 and (K == 1 or g["viscosity"] != 0.0)


@pytest.mark.parametrize("K", boundaries())
def test_both_sides_of_every_boundary_of_the_tile_choice(backend, K):
    """Four column sets: 64 columns a tile while four tiles fit a CU, 32 while two do, the column form beyond (48 edges: fewer than a tile)."""
    b = boundaries()
    assert [tile_columns(k) for k in b] == [64, 32, 32, 0] and b[1] == b[0] + 1 and b[3] == b[2] + 1
    g, path = device(backend, "tiny-4-4", K)
    assert g["viscosity"] != 0.0
    assert path == (1 if tile_columns(K) else 2)


@pytest.mark.parametrize("K", [5, 35])
def test_cell_columns_off_the_16_byte_grid(backend, K):
    """35 cells, odd K: every second cell column starts 8 bytes off a 16-byte boundary: the 8-byte staging lanes run."""
    device(backend, tf.sheared_mesh(7, 5), K)


@pytest.mark.parametrize("meshname,K", [("ico16", 5), ("ico12f", 34)])
def test_pentagons_and_heptagons(backend, meshname, K):
    """The cell gather with 5 and 7 slots (ico12f: heptagons; both: pentagons)."""
    nec = np.asarray(tc.get_mesh(meshname).nEdgesOnCell)
    assert (nec == 5).any() and (meshname == "ico16" or (nec == 7).any())
    device(backend, meshname, K)


# ---- masks and poison ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
@pytest.mark.parametrize("mask", [True, "basin"], ids=["partial_mlt", "basin"])
@pytest.mark.parametrize("K", [6, 34])
def test_masks_and_nan_below_every_edge(backend, K, variant, mask):
    """Edges of depth 0, 1 and up to K side by side.  The state's u -- hence the recorded un -- is NaN wherever no active element reads
    it, the free seed's XU is NaN below every edge's depth: no NaN reaches an active value of X or a density, and the rows k >= n of XU
    and XH keep what the twin keeps there.  (hbar is the tape's own array: the gather's depth test is what keeps its rows k >= n_e out.)"""
    mesh, mlt = tc.get_mesh("planar"), mask_of("planar", K, mask)
    assert (mlt == 0).any() and (mlt == 1).any() and (mlt == K).any()
    g, _ = device(backend, "planar", K, mask=mask, seed=17, poison=True, variant=variant)
    live, livec = pc.active(mesh, mlt, K, "edge"), pc.active(mesh, mlt, K, "cell")
    assert np.all(np.isfinite(g["normalVelocity"][live])) and np.all(np.isnan(g["normalVelocity"][~live]))
    # (below every edge of a cell the RK4 transposition itself carries the seed's NaN into XH: the twin's pattern, compared above)
    assert np.all(np.isfinite(g["layerThickness"][livec])) and np.all(np.isfinite(g["surfaceStress"]))
    assert np.isfinite(g["viscosity"]) and np.isfinite(g["bottomDrag"])
    clean = reference("planar", K, mask=mask, seed=17)
    assert np.array_equal(g["normalVelocity"][live], clean["XU"][live]) and np.array_equal(g["layerThickness"][livec], clean["XH"][livec])
    assert np.array_equal(g["surfaceStress"], clean["dens"][1])


def test_rows_below_the_depth_keep_their_bits_through_the_pass(backend):
    """A finite free seed that is nonzero below every edge's depth, one step: the twin leaves the rows k >= n of XU and XH to the RK4
    transposition alone, and the device has the twin's bits everywhere."""
    device(backend, "planar", 6, mask=True, seed=23, plan=(("nu+drag", 1.0),))


# ---- switches -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stress", [None, "stress", "stress0", "zero"])
@pytest.mark.parametrize("what", ["", "nu", "drag", "nu+drag"])
def test_every_switch_combination(backend, what, stress):
    """Partial columns, so that drag and stress meet n == 1; every gradient flagged.  "" without a stress, and with the all-zero one
    (present, counts as absent): every step ran without the pass and the densities are derivatives at zero."""
    g, path = device(backend, "planar", 6, plan=((what, 1.0),) * 2, stress=stress, mask=True)
    assert path == 1


@pytest.mark.parametrize("want", [0, 1, 2, 4, 3, 5, 6])
@pytest.mark.parametrize("variant", [0, 3], ids=["tile", "column"])
def test_each_gradient_flag_and_x_keeps_its_bits(backend, want, variant):
    g, _ = device(backend, "planar", 6, want=want, mask=True, variant=variant)
    full = reference("planar", 6, want=7, mask=True)
    assert np.array_equal(g["normalVelocity"], full["XU"]) and np.array_equal(g["layerThickness"], full["XH"])


# ---- values changed between steps ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", [(("nu", 1.0), ("drag", 1.0), ("nu+drag", 1.0)), (("nu+drag", 1.0), ("nu+drag", 0.0), ("nu", 1.0)),
                                  (("nu+drag", 1.0), ("", 1.0), ("nu", 1.0))], ids=["nu-r-change", "dt-zero", "pass-off-for-one-step"])
@pytest.mark.parametrize("want", [0, 7])
def test_values_changed_between_steps(backend, plan, want):
    device(backend, "planar", 6, plan=plan, stress=None if plan[1][0] == "" else "stress", want=want, mask=True)


# ---- pass off, forward bits, free seed ----------------------------------------------------------------------------------------------
def test_pass_off_equals_the_rk4_adjoint_tape(backend):
    g, path = device(backend, "planar", 34, plan=(("", 1.0),) * 3, stress=None, want=0)
    assert path == 0
    md = tc.Model(backend, "planar", 34)
    try:
        t = mk.AdjointTape(md.Prog, 3)
        for _ in range(3):
            t.step(md.dt, method=mk.RungeKutta4)
        r = t.gradient()
        t.close()
        assert np.array_equal(r["normalVelocity"], g["normalVelocity"]) and np.array_equal(r["layerThickness"], g["layerThickness"])
    finally:
        md.close()


def test_forward_bits_are_those_of_step_rk4(backend):
    """State and diagnostics after forced taped steps against moka_step_rk4 with the same settings."""
    out = []
    for taped in (False, True):
        md = tc.Model(backend, "planar", 34)
        try:
            nu, r = mv.coefficients("planar", 34)
            mk.set_vertical_mixing(md.Prog, viscosity=nu, bottom_drag=r, surface_stress=stress_of("planar", 34, "stress"))
            tape = mk.ForcedAdjointTape(md.Prog, 3) if taped else None
            for _ in range(3):
                if taped:
                    tape.step(md.dt)
                else:
                    md.eager(1)
            Diag, Tend = mk.DiagnosticVars(None, md.M, md.Prog._state), mk.TendencyVars(None, md.M, md.Prog._state)
            out.append([md.Prog.normalVelocity[-1].get(), md.Prog.layerThickness[-1].get(), md.Prog.ssh[-1].get(),
                        md.Prog.normalVelocity[0].get(), md.Prog.layerThickness[0].get(),
                        np.asarray(Diag.layerThicknessEdge), np.asarray(Diag.thicknessFlux), np.asarray(Diag.velocityDivCell),
                        np.asarray(Diag.relativeVorticity), np.asarray(Tend.tendNormalVelocity), np.asarray(Tend.tendLayerThickness)])
            assert mk.momentum_vmix_path(md.Prog) == 1
            if taped:
                tape.close()
        finally:
            md.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("meshname,K", [("planar", 34), ("ico12f", 5)])
def test_free_seed(backend, meshname, K):
    device(backend, meshname, K, seed=29, plan=FULL + (("nu", 1.0),))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def snapshot(Prog):
    return [Prog.normalVelocity[lev].get() for lev in (0, 1)] + [Prog.layerThickness[lev].get() for lev in (0, 1)] + [Prog.ssh[-1].get()]


def unchanged(Prog, snap):
    return all(np.array_equal(a, b) for a, b in zip(snapshot(Prog), snap))


def test_refusals_and_argument_errors(backend):
    md = tc.Model(backend, "planar", 6)
    lib, sh, ctx = L.lib(), md.Prog._state._h, md.backend._h
    nu, r = mv.coefficients("planar", 6)
    tau = stress_of("planar", 6, "stress")
    h = C.c_void_p()
    try:
        assert lib.moka_forced_tape_create(None, 2, C.byref(h)) == L.ERR_ARG and lib.moka_forced_tape_create(sh, 2, None) == L.ERR_ARG
        assert lib.moka_forced_tape_create(sh, -1, C.byref(h)) == L.ERR_ARG and not h.value
        # an existing moka_tape refuses the forced tape, and beside it the pass setters still refuse with its name
        t = mk.AdjointTape(md.Prog, 2)
        assert lib.moka_forced_tape_create(sh, 2, C.byref(h)) == L.ERR_UNSUPPORTED and not h.value
        assert lib.moka_set_vertical_viscosity(sh, 1.0, 0.0) == L.ERR_UNSUPPORTED and b"moka_tape" in lib.moka_last_error(ctx)
        t.close()
        mk.set_vertical_mixing(md.Prog, viscosity=nu, bottom_drag=r, surface_stress=tau)
        ft = mk.ForcedAdjointTape(md.Prog, 2)
        fh = ft._h
        # beside a forced tape
        assert lib.moka_forced_tape_create(sh, 2, C.byref(h)) == L.ERR_UNSUPPORTED and not h.value
        assert lib.moka_tape_create(sh, 2, C.byref(h)) == L.ERR_UNSUPPORTED and not h.value
        assert b"vertical momentum mixing" in lib.moka_last_error(ctx)            # moka_tape's own refusal comes first: the pass is on
        assert lib.moka_set_tracers(sh, 1) == L.ERR_UNSUPPORTED
        assert lib.moka_set_vertical_viscosity(sh, 0.0, 0.0) == 0
        assert lib.moka_tape_create(sh, 2, C.byref(h)) == L.ERR_UNSUPPORTED and not h.value    # the stress keeps the pass on
        assert lib.moka_surface_stress_upload(sh, None) == 0                       # no step recorded yet: allowed
        assert lib.moka_tape_create(sh, 2, C.byref(h)) == L.ERR_UNSUPPORTED and not h.value
        assert b"moka_forced_tape" in lib.moka_last_error(ctx)
        assert lib.moka_surface_stress_upload(sh, L.f64(tau)) == 0 and lib.moka_set_vertical_viscosity(sh, nu, r) == 0
        # argument errors; nothing moves
        snap = snapshot(md.Prog)
        v = C.c_double()
        buf = np.zeros(md.mesh.nEdges)
        assert lib.moka_step_rk4_forced_taped(None, md.dt) == L.ERR_ARG
        assert lib.moka_step_rk4_forced_taped(fh, -md.dt) == L.ERR_ARG and b"dt must be >= 0" in lib.moka_last_error(ctx)
        assert lib.moka_forced_adjoint_sweep(fh) == L.ERR_ARG and b"seed" in lib.moka_last_error(ctx)
        assert lib.moka_forced_adjoint_want_gradient(fh, 0, 1) == L.ERR_ARG and lib.moka_forced_adjoint_want_gradient(fh, 8, 1) == L.ERR_ARG
        assert lib.moka_forced_adjoint_gradient(fh, 2, C.byref(v)) == L.ERR_ARG   # not flagged
        assert lib.moka_forced_adjoint_density_download(fh, 1, L.f64(buf)) == L.ERR_ARG
        ft.want_gradient(viscosity=True)
        assert lib.moka_forced_adjoint_gradient(fh, 2, C.byref(v)) == 0 and v.value == 0.0
        assert lib.moka_forced_adjoint_gradient(fh, 3, C.byref(v)) == L.ERR_ARG and lib.moka_forced_adjoint_gradient(fh, 2, None) == L.ERR_ARG
        assert lib.moka_forced_adjoint_seed(fh, None, None) == L.ERR_ARG
        assert lib.moka_forced_adjoint_download(fh, L.F_SSH, L.f64(buf)) == L.ERR_ARG
        assert lib.moka_forced_adjoint_download(fh, L.F_NORMAL_VELOCITY, None) == L.ERR_ARG
        assert lib.moka_forced_tape_vmix_path(None) == 0 and lib.moka_forced_tape_vmix_path(fh) == 0
        assert unchanged(md.Prog, snap)
        ft.step(md.dt)
        ft.step(md.dt)
        snap = snapshot(md.Prog)
        assert lib.moka_step_rk4_forced_taped(fh, md.dt) == L.ERR_ARG and b"full" in lib.moka_last_error(ctx)
        assert lib.moka_forced_adjoint_want_gradient(fh, 1, 1) == L.ERR_ARG        # recorded steps
        assert lib.moka_surface_stress_upload(sh, L.f64(tau)) == L.ERR_UNSUPPORTED and b"moka_forced_tape" in lib.moka_last_error(ctx)
        assert lib.moka_surface_stress_upload(sh, None) == L.ERR_UNSUPPORTED
        assert lib.moka_set_vertical_viscosity(sh, nu, r) == 0                      # allowed at any time
        assert unchanged(md.Prog, snap) and np.array_equal(mk.vertical_mixing(md.Prog)[2], tau)
        # the refused calls left the tape as it was: its sweep is the twin's
        ref = reference("planar", 6, want=2)
        g = ft.gradient()
        assert np.array_equal(g["normalVelocity"], ref["XU"]) and np.array_equal(g["layerThickness"], ref["XH"])
        assert g["viscosity"] == ref["grad"]["viscosity"]
        assert lib.moka_surface_stress_upload(sh, L.f64(tau)) == 0                  # the tape is empty again
        ft.close()
        assert lib.moka_set_vertical_viscosity(sh, 0.0, 0.0) == 0 and lib.moka_surface_stress_upload(sh, None) == 0
        t = mk.AdjointTape(md.Prog, 2)                                              # and moka_tape works again
        t.close()
    finally:
        md.close()


def test_unsupported_states(backend):
    lib, h = L.lib(), C.c_void_p()
    f32 = tc.Model(backend, "ico16", 4, state_bytes=4)
    try:
        assert lib.moka_forced_tape_create(f32.Prog._state._h, 2, C.byref(h)) == L.ERR_UNSUPPORTED and not h.value
        assert b"Float64" in lib.moka_last_error(backend._h)
    finally:
        f32.close()
    nl = tc.Model(backend, "planar", 6, mode="nonlinear")
    try:
        assert lib.moka_forced_tape_create(nl.Prog._state._h, 2, C.byref(h)) == L.ERR_UNSUPPORTED and not h.value
    finally:
        nl.close()
    md = tc.Model(backend, "planar", 6)
    try:
        mk.set_tracers(md.Prog, tc.distinct_fields(md.mesh, 6, 1))
        assert lib.moka_forced_tape_create(md.Prog._state._h, 2, C.byref(h)) == L.ERR_UNSUPPORTED and not h.value
        assert b"tracers" in lib.moka_last_error(backend._h)
    finally:
        md.close()


def test_refused_on_a_rank_with_a_halo():
    from moka_hip import parallel as par
    mesh = tc.get_mesh("ico12f")
    ssh, u, h, rest = tc.random_state(mesh, 4, 12)
    cl = par.LocalCluster(mesh, ssh, u, h, rest, 20.0, 2, direct=False)
    try:
        out = C.c_void_p()
        assert L.lib().moka_forced_tape_create(cl.models[0].Prog._state._h, 2, C.byref(out)) == L.ERR_UNSUPPORTED and not out.value
    finally:
        cl.close()
