"""The HIP tendency kernels against the independent long-double reference (tests/trisk_reference.py), through the C ABI: every
nonlinear kernel form with Del2 / Del4 at the K where the forms switch, the linear path in fp64 and with fp32 storage, the scheme's
identities on the GPU's own tendencies, and RK4 steps / runs.  Per element within the reference's error bound, not bit for bit:
these tests accept any kernel that rounds differently within C 2^-53 M (see the reference's docstring)."""
import dataclasses
import datetime as dt

import numpy as np
import pytest

import moka_hip as mk
import trisk_reference as tr
from moka_hip import lib as L
from moka_hip import meshgen as mg

pytestmark = pytest.mark.gpu

CONFIG = {"time_management": {"config_start_time": dt.datetime(1, 1, 1), "config_run_duration": dt.timedelta(hours=10)},
          "time_integration": {"config_dt": dt.timedelta(seconds=60), "config_number_of_time_levels": 2}}
_MESHES = {}
# the patch form of the nonlinear kernels serves even 34 <= K <= 64 (nl3_ok in nonlinear.hip); 16-byte lanes pair levels
KS = [1, 2, 3, 32, 33, 34, 35, 62, 63, 64, 65, 66, 100]
CASES = [(m, K) for m in ("ico16", "ico12f", "planar") for K in KS] + [("ico32", K) for K in (1, 34, 65)]
# (kernel variant, launch shape): variant 0 with moka_set_tuning(5, shape) / shape 10 = (5, 0) + (6, 40), variant 4, variant 3
FORMS = [(0, 0), (0, 1), (0, 2), (0, 3), (0, 10), (4, 0), (3, 0)]


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)
    yield b
    b.close()


def get_mesh(name):
    if name not in _MESHES:
        _MESHES[name] = {"planar": lambda: mg.planar_hex_mesh(20, 18, 1000.0, f0=1e-4),
                         "ico16": lambda: mg.icosahedral_mesh(16),
                         "ico32": lambda: mg.icosahedral_mesh(32),
                         "ico12f": lambda: mg.icosahedral_mesh(12, flips=8, seed=4)}[name]()
    return _MESHES[name]


def random_state(mesh, K, seed):
    rng = np.random.default_rng(seed)
    rest = np.full((mesh.nCells, K), 1000.0 / K) + rng.uniform(0, 0.1, (mesh.nCells, K))
    h = rest + rng.uniform(-1, 1, (mesh.nCells, K))
    u = rng.uniform(-1, 1, (mesh.nEdges, K))
    return h.sum(1) - rest.sum(1), u, h, rest


def edge_mask(mesh, K, kind, seed=8):
    if kind == "full":
        return np.full(mesh.nEdges, K, dtype=np.int32)
    rng = np.random.default_rng(seed)
    mlt = np.where(rng.random(mesh.nEdges) < 0.33, rng.integers(0, K, mesh.nEdges), K).astype(np.int32)
    mlt[:3] = 0
    return mlt


def viscosities(mesh, dtv):
    dcmin = float(mesh.dcEdge.min())
    return 0.01 * dcmin ** 2 / dtv, 0.002 * dcmin ** 4 / dtv


def device_state(backend, mesh, K, ssh, u, h, rest, mlt, P=0, state_bytes=8):
    hm = mk.HorzMesh(mesh)
    vm = mk.VerticalMesh(hm, nVertLevels=K, restingThickness=rest)
    vm.maxLevelEdge.Top[:] = mlt
    M = mk.Mesh(hm, vm, backend=backend, patch_cells=P, state_bytes=state_bytes)
    Prog = mk.PrognosticVars(ssh, u, h, 2, M)
    return M, Prog, mk.DiagnosticVars(None, M, Prog._state), mk.TendencyVars(None, M, Prog._state)


def set_form(backend, variant, shape):
    backend.set_kernel_variant(variant)
    L.check(L.lib().moka_set_tuning(5, shape % 10))
    L.check(L.lib().moka_set_tuning(6, 40 if shape == 10 else 0))


def reset_forms(backend):
    backend.set_kernel_variant(0)
    L.check(L.lib().moka_set_tuning(5, 0))
    L.check(L.lib().moka_set_tuning(6, 0))


class Bound:
    """ref (long double) as a double-double and C 2^-53 M as a double (rounded down), so that the many kernel forms are checked
    in double: |x - hi - lo| <= tol, with x - hi exact wherever the check can pass (Sterbenz)."""

    def __init__(self, ref, M, C):
        self.hi = ref.astype(np.float64)
        self.lo = (ref - self.hi.astype(tr.LD)).astype(np.float64)
        self.tol = (C * tr.U53 * M).astype(np.float64) * (1 - 2.0 ** -50)

    def check(self, x, what):
        err = np.abs((x - self.hi) - self.lo)
        ok = err <= self.tol
        if not ok.all():
            i = np.unravel_index(np.argmin(ok), ok.shape)
            raise AssertionError(f"{what}: {int((~ok).sum())} elements outside the bound; first {i}: got {x[i]!r}, "
                                 f"reference {self.hi[i]!r}, error {err[i]:.3e} > {self.tol[i]:.3e}")


def del4_path_expected(meshname, K, variant):
    """1: the fused patch kernel (patch forms: even 34 <= K <= 64, hexagon-width records); 2: the entity kernels."""
    if variant == 3:
        return 2
    return 1 if K % 2 == 0 and 33 <= K <= 64 and meshname != "ico12f" else 2


@pytest.mark.parametrize("meshname,K", CASES)
def test_nonlinear_forms_within_the_reference_bound(backend, meshname, K):
    """tendU / tendH / ssh after computeTendency, every kernel form x {nonlinear, + Del2, + Del4, + Del2 + Del4 scaled} x {full,
    partial maxLevelEdgeTop}, per element within the bound; with full masks the GPU's inviscid tendencies also satisfy the energy
    and mass budgets."""
    mesh = get_mesh(meshname)
    ssh, u, h, rest = random_state(mesh, K, 300 + K)
    rs = rest.sum(1)
    dtv = 2.0 if meshname == "planar" else 20.0
    v2, v4 = viscosities(mesh, dtv)
    scaling = np.random.default_rng(K).uniform(0.5, 2.0, mesh.nEdges)
    combos = (("nonlinear", 0.0, 0.0, None), ("+Del2", v2, 0.0, None), ("+Del4", 0.0, v4, None), ("+Del2+Del4 scaled", v2, v4, scaling))
    for mask in ("full", "partial"):
        mlt = edge_mask(mesh, K, mask)
        t = tr.terms(mesh, u, h, rs, mlt, nonlinear=True)
        bU = {name: Bound(*tr.combine(t, a, b, s), tr.C_U) for name, a, b, s in combos}
        bH, bS = Bound(*t["H"], tr.C_H), Bound(*t["ssh"], tr.C_SSH)
        del t
        M, Prog, Diag, Tend = device_state(backend, mesh, K, ssh, u, h, rest, mlt)
        try:
            for variant, shape in FORMS:
                set_form(backend, variant, shape)
                for name, a, b, s in combos:
                    mk.set_nonlinear(Prog, True, visc_del2=a, visc_del4=b, mesh_scaling_del4=s)
                    Tend.tendNormalVelocity.set(np.full((mesh.nEdges, K), np.nan))
                    mk.computeTendency(M, Diag, Prog, Tend)
                    what = f"{mask} mask, form {variant}/{shape}, {name}"
                    tu = Tend.tendNormalVelocity.get()
                    bU[name].check(tu, what + ": tendU")
                    bH.check(Tend.tendLayerThickness.get(), what + ": tendH")
                    bS.check(Prog.ssh[-1].get(), what + ": ssh")
                    if b:
                        assert L.lib().moka_state_del4_path(Prog._state._h) == del4_path_expected(meshname, K, variant), what
                    if mask == "full" and name == "nonlinear" and (variant, shape) == (0, 0):
                        th, gssh = Tend.tendLayerThickness.get(), Prog.ssh[-1].get()
                        MU, MH, _ = tr.tendencies(mesh, u, h, rs, mlt, nonlinear=True, abs=True, ssh=gssh)
                        res, tol = tr.energy_budget(mesh, u, h, gssh, tu, th, MU, MH)
                        assert abs(res) <= tol, ("energy", float(res), float(tol))
                        mres, mtol = tr.mass_budget(mesh, th, MH)
                        assert (np.abs(mres) <= mtol).all(), "mass"
        finally:
            reset_forms(backend)
            Prog._state.close(); M.close()


@pytest.mark.parametrize("meshname,K", [("ico16", 1), ("ico12f", 1), ("ico16", 34), ("planar", 34)])
def test_pv_compatibility_on_the_gpu(backend, meshname, K):
    """fVertex = q0 h_v - zeta_v (identical layers): q is uniform and curl(tendU) = q0 * kite-average of tendH at every vertex, on the
    GPU's own tendencies."""
    base = get_mesh(meshname)
    _, u, h, rest = random_state(base, 1, 5)
    u = 5.0 * u
    q0 = 1e-7
    mesh = dataclasses.replace(base, fVertex=tr.uniform_q_fvertex(base, u, h, q0))
    u, h, rest = np.repeat(u, K, 1), np.repeat(h, K, 1) / K, np.repeat(rest, K, 1) / K     # every layer: q = K q0
    ssh = h.sum(1) - rest.sum(1)
    mlt = edge_mask(mesh, K, "full")
    M, Prog, Diag, Tend = device_state(backend, mesh, K, ssh, u, h, rest, mlt)
    try:
        mk.set_nonlinear(Prog, True)
        mk.computeTendency(M, Diag, Prog, Tend)
        tu, th, gssh = Tend.tendNormalVelocity.get(), Tend.tendLayerThickness.get(), Prog.ssh[-1].get()
        MU, MH, _ = tr.tendencies(mesh, u, h, rest.sum(1), mlt, nonlinear=True, abs=True, ssh=gssh)
        res, tol = tr.pv_compatibility(mesh, q0 * K, tu, th, MU, MH)
        assert (np.abs(res) <= tol).all(), float(np.max(np.abs(res) / tol))
    finally:
        Prog._state.close(); M.close()


@pytest.mark.parametrize("K", [1, 60, 70])
def test_linear_path_fp64_within_the_reference_bound(backend, K):
    """The reference's linear tendencies (the default path) in every kernel variant this build carries, full and partial masks."""
    mesh = get_mesh("ico16")
    ssh, u, h, rest = random_state(mesh, K, 11 + K)
    variants = [0] + [v for v in (11, 3, 4) if L.lib().moka_kernel_variant_available(v)]
    for mask in ("full", "partial"):
        mlt = edge_mask(mesh, K, mask)
        t = tr.terms(mesh, u, h, rest.sum(1), mlt, nonlinear=False)
        bU, bH, bS = Bound(*t["U"], tr.C_U), Bound(*t["H"], tr.C_H), Bound(*t["ssh"], tr.C_SSH)
        M, Prog, Diag, Tend = device_state(backend, mesh, K, ssh, u, h, rest, mlt)
        try:
            for v in variants:
                backend.set_kernel_variant(v)
                Tend.tendNormalVelocity.set(np.full((mesh.nEdges, K), np.nan))
                mk.computeTendency(M, Diag, Prog, Tend)
                bU.check(Tend.tendNormalVelocity.get(), f"{mask} variant {v}: tendU")
                bH.check(Tend.tendLayerThickness.get(), f"{mask} variant {v}: tendH")
                bS.check(Prog.ssh[-1].get(), f"{mask} variant {v}: ssh")
        finally:
            backend.set_kernel_variant(0)
            Prog._state.close(); M.close()


@pytest.mark.parametrize("K,P", [(4, 0), (4, 12), (80, 0), (80, 12)])
def test_fp32_storage_within_the_reference_bound(backend, K, P):
    """fp32-stored state, fp64 arithmetic (config 5): from the fp32 values the kernel read, every output within half an fp32 ulp
    plus the fp64 bound.  ssh is stored before the pressure gradient reads it, so the gradient's reference takes the stored ssh."""
    mesh = get_mesh("ico16")
    ssh, u, h, rest = random_state(mesh, K, 21 + K)
    mlt = edge_mask(mesh, K, "full")
    M, Prog, Diag, Tend = device_state(backend, mesh, K, ssh, u, h, rest, mlt, P=P, state_bytes=4)
    try:
        u32, h32 = Prog.normalVelocity[-1].get(), Prog.layerThickness[-1].get()
        assert np.array_equal(u32, u.astype(np.float32)) and np.array_equal(h32, h.astype(np.float32))
        mk.computeTendency(M, Diag, Prog, Tend)
        tu, th, gssh = Tend.tendNormalVelocity.get(), Tend.tendLayerThickness.get(), Prog.ssh[-1].get()
        t = tr.terms(mesh, u32, h32, rest.sum(1), mlt, nonlinear=False)
        assert tr.within(gssh, *t["ssh"], tr.C_SSH, f32=True).all()
        assert tr.within(th, *t["H"], tr.C_H, f32=True).all()
        U, MU = tr.terms(mesh, u32, h32, rest.sum(1), mlt, nonlinear=False, ssh=gssh)["U"]
        assert tr.within(tu, U, MU, tr.C_U, f32=True).all()
    finally:
        Prog._state.close(); M.close()


def rel_diff(got, ref):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64).astype(tr.LD) - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("meshname,K", [("ico12f", 3), ("ico16", 8), ("planar", 4), ("ico16", 34)])
def test_one_rk4_step_within_1e12(backend, meshname, K):
    """One RK4 step per nonlinear / Del2 / Del4 case: max-norm relative difference to the long-double RK4 <= 1e-12."""
    mesh = get_mesh(meshname)
    ssh, u, h, rest = random_state(mesh, K, 500 + K)
    rs, mlt = rest.sum(1), edge_mask(mesh, K, "full")
    dtv = 2.0 if meshname == "planar" else 20.0
    v2, v4 = viscosities(mesh, dtv)
    scaling = np.random.default_rng(K).uniform(0.5, 2.0, mesh.nEdges)
    for name, a, b, s in (("nonlinear", 0.0, 0.0, None), ("+Del2", v2, 0.0, None), ("+Del4", 0.0, v4, None),
                          ("+Del2+Del4 scaled", v2, v4, scaling)):
        Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, CONFIG, backend, multilayer=True)
        try:
            mk.set_nonlinear(Prog, True, visc_del2=a, visc_del4=b, mesh_scaling_del4=s)
            mk.changeTimeStep(Setup.timeManager, dt.timedelta(seconds=dtv))
            mk.ocn_timestep(Prog, Diag, Tend, Setup, mk.RungeKutta4)
            ru, rh, rssh = tr.rk4(mesh, u, h, rs, mlt, dtv, nonlinear=True, visc_del2=a, visc_del4=b, scaling_del4=s)
            for got, ref, what in ((Prog.normalVelocity[-1].get(), ru, "u"), (Prog.layerThickness[-1].get(), rh, "h"),
                                   (Prog.ssh[-1].get(), rssh, "ssh")):
                assert rel_diff(got, ref) <= 1e-12, (name, what, rel_diff(got, ref))
        finally:
            Prog._state.close(); Setup.mesh.close()


def tc2_layers(mesh, K):
    """Williamson et al. (1992) test case 2 split into K equal layers plus a small smooth perturbation per layer."""
    a, om, G, u0, h0 = mg.RADIUS_EARTH, mg.OMEGA_EARTH, float(tr.G), 38.61, 2998.0
    R = np.hypot(np.hypot(mesh.xCell, mesh.yCell), mesh.zCell)
    lat, lon = np.arcsin(mesh.zCell / R), np.arctan2(mesh.yCell, mesh.xCell)
    htot = h0 - (a * om * u0 + 0.5 * u0 * u0) * np.sin(lat) ** 2 / G
    RE = np.hypot(np.hypot(mesh.xEdge, mesh.yEdge), mesh.zEdge)
    latE, lonE = np.arcsin(mesh.zEdge / RE), np.arctan2(mesh.yEdge, mesh.xEdge)
    ks = np.arange(K)[None, :]
    h = htot[:, None] / K + 0.5 * np.cos(lat)[:, None] * np.sin(lon[:, None] + ks)
    u = (u0 * np.cos(latE) * np.cos(mesh.angleEdge))[:, None] + 0.5 * np.cos(latE)[:, None] * np.cos(2 * lonE[:, None] + ks)
    rest = np.full((mesh.nCells, K), h0 / K)
    return h.sum(1) - rest.sum(1), u, h, rest


def test_100_steps_nonlinear_del2_del4_and_graph_replay(backend):
    """100 RK4 steps of TC2 + a perturbation (ico16, K = 3, nonlinear + Del2 + Del4), step by step and replayed from a graph
    (run_steps): both within 1e-10 (max-norm relative, BASELINE's bar after 100 steps) of the long-double RK4."""
    mesh = get_mesh("ico16")
    K, n, dtv = 3, 100, 60.0
    ssh, u, h, rest = tc2_layers(mesh, K)
    v2, v4 = viscosities(mesh, dtv)
    ru, rh, rssh = tr.rk4(mesh, u, h, rest.sum(1), np.full(mesh.nEdges, K), dtv, n, nonlinear=True, visc_del2=v2, visc_del4=v4)
    assert rel_diff(u, ru) > 1e-6                                              # the run moved
    for replay in (False, True):
        Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, CONFIG, backend, multilayer=True)
        try:
            mk.set_nonlinear(Prog, True, visc_del2=v2, visc_del4=v4)
            if replay:
                mk.run_steps(Prog, mk.RungeKutta4, dtv, n)
            else:
                mk.changeTimeStep(Setup.timeManager, dt.timedelta(seconds=dtv))
                for _ in range(n):
                    mk.ocn_timestep(Prog, Diag, Tend, Setup, mk.RungeKutta4)
            for got, ref, what in ((Prog.normalVelocity[-1].get(), ru, "u"), (Prog.layerThickness[-1].get(), rh, "h"),
                                   (Prog.ssh[-1].get(), rssh, "ssh")):
                assert rel_diff(got, ref) <= 1e-10, (replay, what, rel_diff(got, ref))
        finally:
            Prog._state.close(); Setup.mesh.close()
