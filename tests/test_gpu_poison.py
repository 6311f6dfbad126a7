"""Skipped means never read: every kernel family on the device over a bathymetry-like edge mask, with NaN (one case per family: -inf)
on every level no active element may read (tests/poison_cases.py states the mask, the sets and the comparisons), against the oracle and
the numpy twins under the same poison.  A kernel that masked with a zero weight, or computed a discarded lane's value into something
kept, passes every other file of the suite -- all of them fill every level with benign numbers -- and fails here.

Forward families: every downloaded field is `same` as the reference (NaN where it has NaN, the same bits elsewhere).  Reverse families:
as stated per test.  Every case: layerThickness and ssh are finite, and the kernel form the case names did run (Tracers.path,
moka_state_del4_path, moka_last_fe_path, the mesh info).  tests/test_poison_twin.py proves on the CPU that none of this is vacuous: the
poison set holds 22 to 47 % of normalVelocity (24 to 39 % of a tracer) and the references stay finite, with unchanged bits, on 100 %
of the active set."""
import ctypes as C

import numpy as np
import pytest

import moka_hip as mk
import poison_cases as pc
import tracer_cases as tc
import tracer_kgrad_twin as tk
from moka_hip import lib as L

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
VARIANTS = [v for v in (11, 3, 4) if L.lib().moka_kernel_variant_available(v)]
TUNE_FE_LEAN, TUNE_NL_SHAPE, TUNE_NL_CAP, TUNE_RK13, TUNE_PAIR, TUNE_FE_LEAN_INST = 4, 5, 6, 7, 8, 9     # csrc/kernels.hpp
PAIR_EVERY = (1 << 16) | 0b1110001111                # modes 0-3 and 7-9 paired, no size threshold (test_gpu_parity.py)


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)
    yield b
    b.close()


class tuning:
    """moka_set_tuning(key, value) for the block, the value of before restored afterwards."""

    def __init__(self, *pairs):
        self.pairs, self.old = pairs, []

    def __enter__(self):
        for key, value in self.pairs:
            old = C.c_int()
            L.check(L.lib().moka_get_tuning(key, C.byref(old)))
            self.old.append((key, old.value))
            L.check(L.lib().moka_set_tuning(key, value))

    def __exit__(self, *exc):
        for key, value in reversed(self.old):
            L.check(L.lib().moka_set_tuning(key, value))


def patch_cells_of(K):
    return 48 if K == 64 else 0          # planar K = 64: patches of 48 cells take several passes and the tail loops


def model(backend, meshname, K, mode="linear", poison="nan", **kw):
    st, _ = pc.state(meshname, K, mode, poison)
    kw.setdefault("patch_cells", patch_cells_of(K))
    md = tc.Model(backend, meshname, K, mode="nonlinear" if mode == "nonlinear+del2" else mode, mlt=pc.mask_of(meshname, K), state=st,
                  **kw)
    if mode == "nonlinear+del2":
        mk.set_nonlinear(md.Prog, True, visc_del2=tc.viscosities(md.mesh, md.dt)[0])
    md.Diag, md.Tend = mk.DiagnosticVars(None, md.M, md.Prog._state), mk.TendencyVars(None, md.M, md.Prog._state)
    if kw["patch_cells"]:
        assert md.info["maxPatchCells"] == kw["patch_cells"]
    return md


def check_form(md, meshname, K, variant=0):
    """What the mesh info says about the form the stage kernels take: the lane-group (generic) kernels below K = 34, on odd K and on
    meshes with more than six edges per cell unless the patch records hold them; LDS-tiled patches otherwise."""
    if K < 34:
        assert md.info["lanesPerColumn"] == tk.lanes(K)
    elif variant == 0:
        assert md.info["ldsBytesPerBlock"] > 0 and md.info["nPatches"] > 1
    if meshname == "ico12f":
        assert md.info["maxEdgesUsed"] > 6 and md.mesh.nEdgesOnCell.min() < 6       # wider records: every cell carries empty slots


def expect(got, ref, what):
    assert pc.same(got, ref), (what, "elements whose NaN-ness differs, others whose bits differ:", pc.differences(got, ref))


def prog_fields(md, tend=True):
    P = md.Prog
    out = {"u1": P.normalVelocity[-1].get(), "h1": P.layerThickness[-1].get(), "ssh1": P.ssh[-1].get(), "u0": P.normalVelocity[0].get(),
           "h0": P.layerThickness[0].get()}
    if tend:
        out["tendU"], out["tendH"] = md.Tend.tendNormalVelocity.get(), md.Tend.tendLayerThickness.get()
    return out


def check_levels(md, ref, what, tend=True):
    got = prog_fields(md, tend)
    for name in got:
        expect(got[name], ref[name], (what, name))
    assert np.isfinite(got["h1"]).all() and np.isfinite(got["ssh1"]).all() and np.isfinite(got["h0"]).all()


def check_tendency(md, ref, what, variants=(0,)):
    """The tendency launch alone, its outputs prefilled with NaN: levels at and below an edge's top come back as the oracle's zeros."""
    for v in variants:
        md.backend.set_kernel_variant(v)
        try:
            md.Tend.tendNormalVelocity.set(np.full_like(ref["tendU"], np.nan))
            md.Tend.tendLayerThickness.set(np.full_like(ref["tendH"], np.nan))
            md.Prog.ssh[-1].set(np.full_like(ref["ssh"], np.nan))
            mk.computeTendency(md.M, md.Diag, md.Prog, md.Tend)
            expect(md.Tend.tendNormalVelocity.get(), ref["tendU"], (what, "tendU", v))
            expect(md.Tend.tendLayerThickness.get(), ref["tendH"], (what, "tendH", v))
            expect(md.Prog.ssh[-1].get(), ref["ssh"], (what, "ssh", v))
            assert np.isfinite(md.Tend.tendLayerThickness.get()).all()
        finally:
            md.backend.set_kernel_variant(0)


# ---- linear RK4 and the tendency launch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K,variant,tune,poison",
                         [(m, K, 0, None, "nan") for m, K in pc.SHAPES]
                         + [("planar", 34, 3, None, "nan"), ("planar", 34, 4, None, "nan"), ("ico12f", 60, 3, None, "nan"),
                            ("ico12f", 60, 4, None, "nan"), ("planar", 8, 3, None, "nan")]
                         + [("planar", 34, 0, "pair", "nan"), ("planar", 64, 0, "pair", "nan"), ("ico12f", 60, 0, "pair", "nan")]
                         + [("planar", 34, 0, "rk13", "nan"), ("planar", 64, 0, "rk13", "nan"), ("ico12f", 60, 0, "rk13", "nan"),
                            ("ico12f", 60, 0, "pair+rk13", "nan")]
                         + [("planar", 34, 0, None, "-inf"), ("ico12f", 5, 0, None, "-inf"), ("ico12f", 60, 0, "rk13", "-inf")])
def test_linear_rk4(backend, meshname, K, variant, tune, poison):
    """Kernel variants 0 (the default forms), 3 (generic) and 4 (plain column); two patches per workgroup (TUNE_PAIR, every mode); the
    13-stream form (TUNE_RK13) against its own twin: two eager steps, then seven through moka_run, which replays the captured graph.
    Both time levels and the lazily produced stage-4 tendencies after step 2 and step 9."""
    tune = tune or ""
    form = "s13" if "rk13" in tune else "ref"
    ref = pc.rk4(meshname, K, "linear", poison, pc.RK4_STEPS, form)
    keys = ([(TUNE_PAIR, PAIR_EVERY)] if "pair" in tune else []) + ([(TUNE_RK13, 1)] if "rk13" in tune else [])
    with tuning(*keys):
        # the 13-stream form is served where the default patches fit the LDS, so those cases keep the default patch size
        md = model(backend, meshname, K, poison=poison, variant=variant, **({"patch_cells": 0} if "rk13" in tune else {}))
        try:
            check_form(md, meshname, K, variant)
            if "rk13" in tune:
                assert L.lib().moka_state_rk4_streams(md.Prog._state._h) == 13
            md.eager(pc.RK4_STEPS[0])
            check_levels(md, ref[0], "eager")
            md.run(pc.RK4_STEPS[1] - pc.RK4_STEPS[0])
            check_levels(md, ref[1], "replayed")
        finally:
            md.close()


@pytest.mark.parametrize("meshname,K,poison", [(m, K, "nan") for m, K in pc.SHAPES] + [("planar", 34, "-inf"), ("ico12f", 60, "-inf")])
def test_tendency_launch(backend, meshname, K, poison):
    """moka_tendencies alone, in every kernel variant the library carries, and with every stage-kernel mode paired."""
    ref = pc.tendency(meshname, K, "linear", poison)
    md = model(backend, meshname, K, poison=poison)
    try:
        check_form(md, meshname, K)
        check_tendency(md, ref, "tendency", VARIANTS + [0])
        with tuning((TUNE_PAIR, PAIR_EVERY)):
            check_tendency(md, ref, "paired tendency")
    finally:
        md.close()


# ---- Forward Euler --------------------------------------------------------------------------------------------------------------------
def fe_fields(md):
    P, D, T = md.Prog, md.Diag, md.Tend
    return {"ssh0": P.ssh[0].get(), "ssh1": P.ssh[-1].get(), "u0": P.normalVelocity[0].get(), "u1": P.normalVelocity[-1].get(),
            "h0": P.layerThickness[0].get(), "h1": P.layerThickness[-1].get(), "hEdge": D.layerThicknessEdge.get(),
            "F": D.thicknessFlux.get(), "div": D.velocityDivCell.get(), "vort": D.relativeVorticity.get(),
            "tendU": T.tendNormalVelocity.get(), "tendH": T.tendLayerThickness.get()}


def run_fe(md, ref, flags, tuned, exact_path=True):
    lib, hS = L.lib(), md.Prog._state._h
    for step in range(pc.FE_STEPS):
        L.check(lib.moka_step_fe(hS, md.dt, flags), md.backend._h)
        path = lib.moka_last_fe_path(hS)
        if not tuned:
            assert path == 0                                       # k_fe, the generic one-launch kernel
        elif exact_path:                                           # the rule test_forward_euler_tuned_path_bitwise states
            assert path == (2 if (flags & 1) and step > 0 else 1)
        else:
            assert path in (1, 2)
        if step in (0, pc.FE_STEPS - 1):
            got = fe_fields(md)
            for name in got:
                expect(got[name], ref[step][name], ("step", step + 1, name))
            for name in ("h0", "h1", "ssh0", "ssh1"):
                assert np.isfinite(got[name]).all()


@pytest.mark.parametrize("meshname,K,flags,how,poison",
                         [("planar", 34, f, how, "nan") for f in (0, 1, 2, 3) for how in ("lean", "store-all")]
                         + [("planar", 34, 3, "lean-general", "nan"), ("planar", 34, 0, "lean-general", "nan")]
                         + [("planar", 8, f, "lean", "nan") for f in (0, 1, 2, 3)] + [("ico12f", 5, 3, "lean", "nan")]
                         + [("planar", 34, 3, "lean", "-inf"), ("planar", 8, 1, "lean", "-inf")])
def test_forward_euler(backend, meshname, K, flags, how, poison):
    """Stale and fresh flux thickness, accumulating and plain vorticity.  K = 34: the tuned stage kernel -- lean steps (modes 10 / 11,
    every other array produced on demand by the downloads), steps that store everything (TUNE_FE_LEAN off: modes 4 / 5 / 6), lean steps
    through the general instances (TUNE_FE_LEAN_INST off); K = 8 and K = 5: k_fe.  Every array of Prog, Diag and Tend: thicknessFlux,
    velocityDivCell and relativeVorticity read every level, so they are NaN in the oracle too below an edge's top."""
    ref = pc.forward_euler(meshname, K, flags, poison, pc.FE_STEPS)
    keys = {"lean": [], "store-all": [(TUNE_FE_LEAN, 0)], "lean-general": [(TUNE_FE_LEAN_INST, 0)]}[how]
    with tuning(*keys):
        md = model(backend, meshname, K, poison=poison)
        try:
            check_form(md, meshname, K)
            run_fe(md, ref, flags, tuned=K == 34, exact_path=how != "store-all")
        finally:
            md.close()


# ---- fp32 storage ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K,poison", [(m, K, "nan") for m, K in pc.FP32_SHAPES] + [("planar", 80, "-inf")])
def test_fp32_storage(backend, meshname, K, poison):
    """fp32-stored states against the storage-emulating oracle: the tendency launch, RK4 (eager and replayed), Forward Euler."""
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)           # noqa: E731
    md = model(backend, meshname, K, poison=poison, state_bytes=4)
    try:
        expect(md.Prog.normalVelocity[-1].get(), f32(md.u), "the upload rounds to fp32 and keeps the poison")
        assert np.array_equal(md.Prog.layerThickness[-1].get(), f32(md.h)) and not np.array_equal(f32(md.h), md.h)
        check_tendency(md, pc.tendency(meshname, K, "linear", poison, True), "fp32 tendency")
        md.Prog.ssh[-1].set(md.ssh)
        ref = pc.rk4(meshname, K, "linear", poison, pc.RK4_STEPS, "mixed")
        md.eager(pc.RK4_STEPS[0])
        check_levels(md, ref[0], "eager")
        md.run(pc.RK4_STEPS[1] - pc.RK4_STEPS[0])
        check_levels(md, ref[1], "replayed")
    finally:
        md.close()
    for flags in (0, 3):
        md = model(backend, meshname, K, poison=poison, state_bytes=4)
        try:
            ref = pc.forward_euler(meshname, K, flags, poison, pc.FE_STEPS, True)
            lib, hS = L.lib(), md.Prog._state._h
            for step in range(pc.FE_STEPS):
                L.check(lib.moka_step_fe(hS, md.dt, flags), backend._h)
            got = fe_fields(md)
            for name in got:
                expect(got[name], ref[-1][name], ("fp32 FE", flags, name))
            assert np.isfinite(got["h1"]).all() and np.isfinite(got["ssh1"]).all()
        finally:
            md.close()


# ---- nonlinear, Del2 + Del4 -----------------------------------------------------------------------------------------------------------
NL_FORMS = [(0, 0), (0, 1), (0, 2), (0, 3), (0, 10), (4, 0), (3, 0)]        # test_nonlinear_kernel_forms_with_partial_edge_masks
D4_FORMS = NL_FORMS[:6] + [(4, 1), (3, 0)]                                  # test_del4_kernel_forms_with_partial_edge_masks


@pytest.mark.parametrize("mode,meshname,K,variant,shape,poison",
                         [("nonlinear", "planar", 34, v, s, "nan") for v, s in NL_FORMS]
                         + [("del2+del4", "planar", 34, v, s, "nan") for v, s in D4_FORMS]
                         + [(mode, m, K, 0, 0, "nan") for mode in ("nonlinear", "del2+del4") for m, K in pc.NONLINEAR_SHAPES if K != 34]
                         + [("nonlinear+del2", m, K, v, 0, "nan") for m, K, v in (("planar", 34, 0), ("planar", 34, 3), ("planar", 8, 0),
                                                                                  ("ico12f", 5, 0), ("planar", 64, 0))]
                         + [("nonlinear", "planar", 34, 0, 0, "-inf"), ("del2+del4", "planar", 34, 0, 0, "-inf"),
                            ("del2+del4", "ico12f", 5, 0, 0, "-inf")])
def test_nonlinear_and_del4(backend, mode, meshname, K, variant, shape, poison):
    """The nonlinear stencils, with and without Del2 mixing, reach one ring further (R = 2), Del2 + Del4 two (R = 3).  K = 34: every
    form of the nonlinear kernels (variant 0 with launch shapes 0 / 1 / 2 / 3 and 10 = 40 resident vertex rows, variant 4, variant 3),
    so both values of moka_state_del4_path; the other shapes in the default form.  The tendency launch alone, then three steps through
    moka_run."""
    ref = pc.rk4(meshname, K, mode, poison, pc.NL_STEPS)
    with tuning((TUNE_NL_SHAPE, shape % 10), (TUNE_NL_CAP, 40 if shape == 10 else 0)):
        md = model(backend, meshname, K, mode=mode, poison=poison, variant=variant)
        try:
            check_form(md, meshname, K, variant)
            md.backend.set_kernel_variant(variant)
            try:
                md.Tend.tendNormalVelocity.set(np.full((md.mesh.nEdges, K), np.nan))
                md.Tend.tendLayerThickness.set(np.full((md.mesh.nCells, K), np.nan))
                mk.computeTendency(md.M, md.Diag, md.Prog, md.Tend)
                tref = pc.tendency(meshname, K, mode, poison)
                expect(md.Tend.tendNormalVelocity.get(), tref["tendU"], "tendU")
                expect(md.Tend.tendLayerThickness.get(), tref["tendH"], "tendH")
                expect(md.Prog.ssh[-1].get(), tref["ssh"], "ssh")
                if mode == "del2+del4":
                    path = L.lib().moka_state_del4_path(md.Prog._state._h)
                    if K == 34:
                        assert path == (2 if variant == 3 else 1)
                    else:
                        assert path == 2 if K < 34 else path in (1, 2)
                md.run(pc.NL_STEPS[0])
                check_levels(md, ref[0], "three steps")
            finally:
                md.backend.set_kernel_variant(0)
        finally:
            md.close()


# ---- tracers, forwards and backwards --------------------------------------------------------------------------------------------------
def tracer_path(md, meshname, K, diff=True, bih=True):
    """tracers.hip's rule restated from its comment (as test_gpu_tracer_biharmonic.py does): the patch form (1) on hexagon-width
    records at even 34 <= K <= 64 while one tracer's rows -- two row sets with the biharmonic term -- fit 80 KB of LDS beside the
    thickness rows and the records; else the generic form (2)."""
    if not (meshname == "planar" and K % 2 == 0 and 34 <= K <= 64):
        return 2
    cells = md.info["maxPatchCells"]
    fixed, per = cells * (8 * K + 144 + (48 if diff or bih else 0)), cells * 8 * K * (2 if bih else 1)
    return 1 if fixed + per <= 80 * 1024 else 2


@pytest.mark.parametrize("meshname,K,nT,diff,bih,srcs,wants,poison",
                         [c + ("nan",) for c in pc.TRACER_CASES]
                         + [c + ("-inf",) for c in pc.TRACER_CASES if c[3] and c[4] and c[5] and c[0] == "planar"])
def test_tracers_forward_and_reverse(backend, meshname, K, nT, diff, bih, srcs, wants, poison):
    """u poisoned on the edge set, every tracer (both time levels) and every seed on the cell set; the sources stay clean (the upload
    refuses anything else).  Two taped steps: both time levels of every tracer and the dycore after each; then the sweep -- with kappa4
    and without -- every adjoint and the wanted source gradient.  Plain, diffused, diffused + biharmonic, with a source; the patch form
    (three tracers at K = 34; at K = 64 in patches of 48 cells three passes of one tracer each, and with kappa4 the generic form
    behind the patch form's Laplacian pass) and the generic form (five at K = 8, three on heptagons at K = 5)."""
    ref = pc.tracers(meshname, K, nT, diff, bih, srcs, wants, poison)
    md = model(backend, meshname, K, poison=poison)
    try:
        tr_ = mk.set_tracers(md.Prog, ref["fields"], sources=ref["sources"])
        tr_.set_diffusivity(ref["kappa"])
        tr_.set_biharmonic(ref["kappa4"])
        tape = mk.TracerAdjointTape(md.Prog, len(ref["forward"]))
        for j in wants:
            tape.want_source_gradient(j)
        for s, fwd in enumerate(ref["forward"]):
            tape.step(md.dt)
            for j in range(nT):
                expect(tr_.get(j), fwd[1][j], ("current", s, j))
                expect(tr_.get(j, 0), fwd[0][j], ("previous", s, j))
            expect(md.Prog.normalVelocity[-1].get(), fwd[2], ("u", s))
            assert np.array_equal(md.Prog.layerThickness[-1].get(), fwd[3]) and np.array_equal(md.Prog.ssh[-1].get(), fwd[4])
            assert np.isfinite(fwd[3]).all() and np.isfinite(fwd[4]).all()
        path = tracer_path(md, meshname, K, diff, bih)
        assert path == {34: 1, 8: 2, 5: 2, 64: 2 if bih else 1}[K] and tr_.path() == path
        grad = tape.gradient(ref["X"])
        for j in range(nT):
            expect(grad[j], ref["grad"][j], ("adjoint", j))
        for j in wants:
            expect(tape.source_gradient(j), ref["G"][j], ("source gradient", j))
        assert tape.path() == path
        tape.close()
    finally:
        md.close()


@pytest.mark.parametrize("meshname,K,nT,poison", [c + ("nan",) for c in pc.KGRAD_CASES] + [("planar", 34, 3, "-inf")])
def test_kgrad(backend, meshname, K, nT, poison):
    """The densities' column sums read every level of a column, so only u is poisoned: tracers, adjoints, both densities and both scalars
    by bits, all finite."""
    ref = pc.tracers(meshname, K, nT, True, True, (), (), poison, kgrad=pc.KGRAD_FLAGS)
    md = model(backend, meshname, K, poison=poison)
    try:
        tr_ = mk.set_tracers(md.Prog, ref["fields"], diffusivity=ref["kappa"], biharmonic=ref["kappa4"])
        tape = mk.TracerAdjointTape(md.Prog, len(ref["forward"]))
        for j, bits in pc.KGRAD_FLAGS:
            tape.want_diffusivity_gradient(j, kappa=bool(bits & 1), biharmonic=bool(bits & 2))
        for fwd in ref["forward"]:
            tape.step(md.dt)
        for j in range(nT):
            assert np.array_equal(tr_.get(j), ref["forward"][-1][1][j]), ("tracer", j)
        expect(md.Prog.normalVelocity[-1].get(), ref["forward"][-1][2], "u")
        grad, dk, dk4 = tape.gradient(ref["X"], diffusivity=True)
        for j in range(nT):
            assert np.array_equal(grad[j], ref["grad"][j]) and np.isfinite(grad[j]).all(), ("adjoint", j)
        for j, bits in pc.KGRAD_FLAGS:
            for b, bih, scalar in ((1, False, dk), (2, True, dk4)):
                if bits & b:
                    W = ref["W"][j][b - 1]
                    assert np.array_equal(tape.diffusivity_density(j, biharmonic=bih), W) and np.isfinite(W).all(), ("density", j, b)
                    assert scalar[j] == tk.host_sum(W), ("scalar", j, b)
        assert tape.path() == tracer_path(md, meshname, K) and tr_.path() == tracer_path(md, meshname, K)
        tape.close()
    finally:
        md.close()


# ---- the dycore's own adjoint ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K,method,flags,nsteps,poison",
                         [c + ("nan",) for c in pc.ADJOINT_CASES] + [("planar", 34, "fe", 3, 2, "-inf"), ("planar", 34, "rk4", 0, 2, "-inf")])
def test_dycore_adjoint(backend, meshname, K, method, flags, nsteps, poison):
    """The gradient of sum ssh^2 over taped Forward-Euler and RK4 steps.  dJ/dnormalVelocity is finite everywhere in the oracle and
    compared whole; dJ/dlayerThickness and dJ/dlayerThicknessEdge are NaN in the oracle itself where it multiplies a poisoned velocity
    by an adjoint of zero, so they are compared where the oracle is finite (at least the active set: test_poison_twin.py)."""
    ref = pc.adjoint(meshname, K, method, flags, poison, nsteps)
    md = model(backend, meshname, K, poison=poison)
    try:
        check_form(md, meshname, K)
        tape = mk.AdjointTape(md.Prog, nsteps)
        for _ in range(nsteps):
            if method == "rk4":
                tape.step(md.dt, method=mk.RungeKutta4)
            else:
                tape.step(md.dt, flags)
        ssh = md.Prog.ssh[-1].get()
        assert np.array_equal(ssh, ref["ssh1"]) and np.isfinite(ssh).all() and np.isfinite(md.Prog.layerThickness[-1].get()).all()
        g = tape.gradient()
        expect(g["normalVelocity"], ref["normalVelocity"], "dJ/du")
        expect(g["ssh"], ref["ssh"], "dJ/dssh")
        assert np.isfinite(g["normalVelocity"]).all() and np.abs(g["normalVelocity"]).max() > 0
        for name in ("layerThickness", "layerThicknessEdge"):
            assert pc.same_where_finite(g[name], ref[name]), (name, pc.differences(g[name], ref[name]))
        tape.close()
    finally:
        md.close()
