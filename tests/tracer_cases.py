"""Shared cases of the tracer tests that came after the first three files (test_gpu_tracer_shapes.py, the eigenmode and tiny-mesh
tests of test_tracer_twin.py / test_tracer_diffusion_twin.py): meshes, states, pairwise distinct tracer fields and diffusivities, the
twins' schedules computed once per case, a device model that takes every mesh option, and the exact plane-wave mode of RK4.

Plane wave.  On the regular hexagons of planar_hex_mesh (f0 = 0) with a uniform thickness and a uniform flow U the edge velocities
u_e = U . n_e are discretely non-divergent, so the linear dycore stays where it is, and phi = exp(i k . x) is an eigenvector both of
the centred flux-form advection,
    mu  = -(1 / (3 dc)) sum_{m=0..5} (U . n_m) exp(i k . d_m),        n_m = (cos m pi/3, sin m pi/3), d_m = dc n_m
(dvEdge / areaCell = 2 / (3 dc), the edge value is half the sum of the two cells, and sum_m U . n_m = 0 removes the cell's own half),
and of the harmonic term, lam = (2 / (3 dc^2)) sum_m (cos(k . d_m) - 1).  h is constant, so Qc / h is phi and n RK4 steps multiply
the mode by R(z)^n with z = (mu + kappa lam) dt and R(z) = 1 + z + z^2/2 + z^3/6 + z^4/24:
    phi_n = 1 + 0.5 Re(R(z)^n exp(i k . x)).
Nothing in this expression shares code with the twins or the kernels."""
import ctypes as C

import numpy as np

import oracle as orc
import tracer_diffusion_twin as td
from del4_twin import Del4Twin, TwinState
from moka_hip import lib as L
from moka_hip import meshgen as mg

TINY = [(4, 4, 60), (2, 4, 60), (6, 4, 34), (4, 6, 1), (4, 2, 8)]          # test_gpu_parity.py's test_tiny_periodic_meshes_bitwise
# kappa_j dt / dcEdge_min^2 of up to nine tracers: pairwise distinct, one exact zero (among the first two), all far below 0.35
KFACT9 = (0.02, 0.0, 0.005, 0.011, 0.016, 0.003, 0.008, 0.013, 0.019)
_MESHES = {}
_REFS = {}


def get_mesh(name):
    """"planar" (20 x 18), "ico16", "ico12f" (heptagons) as in the other tracer files; "tiny-NX-NY": the periodic NX x NY mesh."""
    if name not in _MESHES:
        if name.startswith("tiny-"):
            nx, ny = (int(s) for s in name.split("-")[1:])
            _MESHES[name] = mg.planar_hex_mesh(nx, ny, 1000.0, f0=1e-4)
        else:
            _MESHES[name] = {"planar": lambda: mg.planar_hex_mesh(20, 18, 1000.0, f0=1e-4),
                             "planar-f0": lambda: mg.planar_hex_mesh(20, 18, 1000.0, f0=0.0),
                             "ico16": lambda: mg.icosahedral_mesh(16),
                             "ico12f": lambda: mg.icosahedral_mesh(12, flips=8, seed=4)}[name]()
    return _MESHES[name]


def dt_of(meshname):
    return 20.0 if meshname.startswith("ico") else 2.0


def random_state(mesh, K, seed):
    rng = np.random.default_rng(seed)
    rest = np.full((mesh.nCells, K), 1000.0 / K) + rng.uniform(0, 0.1, (mesh.nCells, K))
    h = rest + rng.uniform(-1, 1, (mesh.nCells, K))
    u = rng.uniform(-1, 1, (mesh.nEdges, K))
    return h.sum(1) - rest.sum(1), u, h, rest


def state_of(meshname, K):
    mesh = get_mesh(meshname)
    return random_state(mesh, K, 100 + mesh.nCells + K if meshname.startswith("tiny-") else 101 + K)


def distinct_fields(mesh, K, n, seed=21, unit_first=False):
    """n pairwise distinct fields in [0.5, 1.5] (every tracer its own draw; unit_first: the first one is 1 everywhere)."""
    rng = np.random.default_rng(seed)
    f = [rng.uniform(0.5, 1.5, (mesh.nCells, K)) for _ in range(n)]
    if unit_first:
        f[0] = np.ones((mesh.nCells, K))
    for i in range(n):
        for j in range(i):
            assert not np.array_equal(f[i], f[j])
    return f


def kappas(meshname, n, factors=KFACT9):
    """n pairwise distinct diffusivities, exactly one of them 0.0 (n >= 2)."""
    dcmin = float(get_mesh(meshname).dcEdge.min())
    k = [f * dcmin ** 2 / dt_of(meshname) for f in factors[:n]]
    assert len(set(k)) == n and (n < 2 or k.count(0.0) == 1)
    return k


def partial_mlt(mesh, K):
    rng = np.random.default_rng(8)
    mlt = np.where(rng.random(mesh.nEdges) < 0.33, rng.integers(0, K + 1, mesh.nEdges), K).astype(np.int32)
    mlt[:3] = 0
    return mlt


def viscosities(mesh, dtv):
    dcmin = float(mesh.dcEdge.min())
    return 0.01 * dcmin ** 2 / dtv, 0.002 * dcmin ** 4 / dtv


def oracle_mesh(meshname, K, partial, mlt=None):
    """mlt: a maxLevelEdgeTop array of the caller's (it replaces both `partial` and the full columns)."""
    mesh = get_mesh(meshname)
    rest = state_of(meshname, K)[3]
    if mlt is None:
        mlt = partial_mlt(mesh, K) if partial else K
    return orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=mlt)


def twin_of(meshname, K, mode="linear", partial=False, mlt=None):
    """A TracerDiffusionTwin (kappa = 0 is TracerTwin bit for bit: test_tracer_diffusion_twin.py) over the dycore base `mode`."""
    mesh, om = get_mesh(meshname), oracle_mesh(meshname, K, partial, mlt)
    base = om
    if mode == "del2+del4":
        v2, v4 = viscosities(mesh, dt_of(meshname))
        base = Del4Twin(om, visc_del2=v2, visc_del4=v4)
    elif mode == "nonlinear":
        base = orc.OracleNonlinear(om)
    return td.TracerDiffusionTwin(om, base, [])


def reference(meshname, K, mode, partial, schedule):
    """The twin's state after EVERY step of `schedule`, computed once per case and shared (never modified by a test):
    schedule = ((nsteps, tracers, diff), ...) with tracers = None (keep the tracers), 0 (none) or (n, seed, unit_first) -- n new
    fields of distinct_fields in both levels -- and diff = whether kappas(meshname, n) act in the segment.  Returns a list over the
    steps of (phis previous, phis current, u, h, ssh)."""
    key = (meshname, K, mode, partial, schedule)
    if key not in _REFS:
        mesh = get_mesh(meshname)
        ssh, u, h, _ = state_of(meshname, K)
        twin = twin_of(meshname, K, mode, partial)
        st = TwinState(ssh, u, h)
        phis = [[], []]
        out = []
        for nsteps, tracers, diff in schedule:
            if tracers is not None:
                f = distinct_fields(mesh, K, *tracers) if tracers else []
                phis = [[a.copy() for a in f], [a.copy() for a in f]]
            n = len(phis[1])
            twin.kappa = kappas(meshname, n) if diff and n else [0.0] * n
            for _ in range(nsteps):
                twin.step_rk4(st, phis, dt_of(meshname))
                out.append(([a.copy() for a in phis[0]], [a.copy() for a in phis[1]], st.u[1].copy(), st.h[1].copy(),
                            st.ssh[1].copy()))
        _REFS[key] = out
    return _REFS[key]


class Model:
    """A model on the device through the C ABI's mesh descriptor, so that every option of it can be set: a partial edge mask, the
    cell ordering, patch_cells, a cell class per cell; `state` = (ssh, u, h, rest) replaces the random state of the case; `mlt` = a
    maxLevelEdgeTop array of the caller's (it replaces `partial`); state_bytes = 4: the fp32-storage state."""

    def __init__(self, backend, meshname, K, mode="linear", partial=False, variant=0, ordering=L.ORDER_DEFAULT, patch_cells=0,
                 cell_class=None, state=None, mlt=None, state_bytes=8):
        import moka_hip as mk
        from moka_hip import api
        self.mk, self.backend = mk, backend
        self.mesh = mesh = get_mesh(meshname)
        self.K, self.dt = K, dt_of(meshname)
        self.ssh, self.u, self.h, self.rest = state if state is not None else state_of(meshname, K)
        backend.set_kernel_variant(variant)
        hm = mk.HorzMesh(mesh)
        vm = mk.VerticalMesh(hm, nVertLevels=K, restingThickness=self.rest, multilayer=True)
        if mlt is not None:
            vm.maxLevelEdge.Top[:] = mlt
        elif partial:
            vm.maxLevelEdge.Top[:] = partial_mlt(mesh, K)
        self.M = M = mk.Mesh(hm, vm)                       # no backend yet: the descriptor below takes the options Mesh() lacks
        M.backend, M.state_bytes = backend, int(state_bytes)
        desc, self._keep = L.make_desc(mesh, K, vm.restingThicknessSum, vm.maxLevelEdge.Top, ordering, patch_cells,
                                       cell_class=cell_class, state_bytes=state_bytes)
        L.check(L.lib().moka_mesh_create(backend._h, C.byref(desc), C.byref(M._h)), backend._h)
        api._own(M, L.lib().moka_mesh_destroy, M._h, backend)
        self.info = M.info()
        self.Prog = mk.PrognosticVars(self.ssh, self.u, self.h, 2, M)
        if mode != "linear":
            v2, v4 = viscosities(mesh, self.dt) if mode == "del2+del4" else (0.0, 0.0)
            mk.set_nonlinear(self.Prog, True, visc_del2=v2, visc_del4=v4)

    def eager(self, n):
        for _ in range(n):
            L.check(L.lib().moka_step_rk4(self.Prog._state._h, self.dt), self.backend._h)

    def run(self, n):
        self.mk.run_steps(self.Prog, self.mk.RungeKutta4, self.dt, n)

    def close(self):
        self.Prog._state.close(); self.M.close()
        self.backend.set_kernel_variant(0)


def check_tracers(tr, ref, n=None):
    """Both time levels of the first n tracers (default: all the reference has) equal `ref` = one entry of reference()."""
    prev, cur = ref[0], ref[1]
    for j in range(len(cur) if n is None else n):
        assert np.array_equal(tr.get(j), cur[j]), ("current", j)
        assert np.array_equal(tr.get(j, 0), prev[j]), ("previous", j)


def check_dycore(Prog, ref):
    assert np.array_equal(Prog.normalVelocity[-1].get(), ref[2])
    assert np.array_equal(Prog.layerThickness[-1].get(), ref[3])
    assert np.array_equal(Prog.ssh[-1].get(), ref[4])


def patch_chunk(maxPatchCells, K, nT, diff):
    """tracers.hip's tracer_kernel restated from its comment: the tracers whose rows the patch form keeps resident in 80 KB of LDS
    beside the thickness rows and the records (per cell 8 K + 144 bytes, 48 more with diffusion; 8 K per tracer), 0 = it does not fit
    (the generic form)."""
    fixed, per = maxPatchCells * (8 * K + 144 + (48 if diff else 0)), maxPatchCells * 8 * K
    return 0 if fixed + per > 80 * 1024 else min(max(nT, 1), (80 * 1024 - fixed) // per)


# ---- the plane wave ---------------------------------------------------------------------------------------------------------------
EIG_U = (70.0, 40.0)
EIG_DC, EIG_DT, EIG_STEPS, EIG_H = 1000.0, 2.0, 10, 250.0
EIG_KAPPA = 0.02 * EIG_DC ** 2 / EIG_DT
EIG_K = (2 * np.pi * 2 / 20000.0, 2 * np.pi / (18 * 1000.0 * np.sqrt(3.0) / 2))


def eigenmode_state(K):
    """(mesh, (ssh, u, h, rest), phi0) of the plane-wave case: "planar-f0", h = 250, ssh = 0, u_e = U . (cos, sin)(angleEdge)."""
    mesh = get_mesh("planar-f0")
    assert np.allclose(mesh.dcEdge, EIG_DC, rtol=1e-12)
    h = np.full((mesh.nCells, K), EIG_H)
    ue = EIG_U[0] * np.cos(np.asarray(mesh.angleEdge)) + EIG_U[1] * np.sin(np.asarray(mesh.angleEdge))
    u = np.repeat(ue[:, None], K, axis=1)
    phi0 = np.repeat((1 + 0.5 * np.cos(EIG_K[0] * np.asarray(mesh.xCell) + EIG_K[1] * np.asarray(mesh.yCell)))[:, None], K, axis=1)
    return mesh, (np.zeros(mesh.nCells), u, h, h.copy()), phi0


def eigenmode_z(kappa):
    kx, ky = EIG_K
    mu, lam = 0j, 0.0
    for m in range(6):
        nx, ny = np.cos(m * np.pi / 3), np.sin(m * np.pi / 3)
        kd = (kx * nx + ky * ny) * EIG_DC
        mu -= (EIG_U[0] * nx + EIG_U[1] * ny) * np.exp(1j * kd) / (3 * EIG_DC)
        lam += 2 / (3 * EIG_DC ** 2) * (np.cos(kd) - 1)
    return (mu + kappa * lam) * EIG_DT


def eigenmode_expect(mesh, K, growth):
    """1 + 0.5 Re(growth exp(i k . x)) on every level; growth = the complex factor the mode has been multiplied by."""
    wave = np.exp(1j * (EIG_K[0] * np.asarray(mesh.xCell) + EIG_K[1] * np.asarray(mesh.yCell)))
    return np.repeat((1 + 0.5 * (growth * wave).real)[:, None], K, axis=1)


def eigenmode_check(phi, mesh, K, kappa, phi0, label):
    """Assert |phi - (1 + 0.5 Re(R(z)^n e^{ikx}))| <= n * 32 * 2^-53 * max|phi0|, and that the same bound would refuse a third-order
    stage loop (by a factor >= 1e6) and the exact exponential.  Prints every figure; returns the deviation."""
    n = EIG_STEPS
    z = eigenmode_z(kappa)
    R4 = 1 + z + z ** 2 / 2 + z ** 3 / 6 + z ** 4 / 24
    R3 = 1 + z + z ** 2 / 2 + z ** 3 / 6
    tol = n * 32 * 2.0 ** -53 * float(np.abs(phi0).max())
    dev = float(np.abs(phi - eigenmode_expect(mesh, K, R4 ** n)).max())
    gap3 = float(np.abs(phi - eigenmode_expect(mesh, K, R3 ** n)).max())
    gapx = float(np.abs(phi - eigenmode_expect(mesh, K, np.exp(z * n))).max())
    print(f"{label}: z = {z:.6g}, |R|^{n} = {abs(R4) ** n:.5f}, max deviation = {dev:.3e}, tolerance = {tol:.3e}, "
          f"gap to third order = {gap3:.3e}, gap to exp(z n) = {gapx:.3e}")
    assert dev <= tol
    assert gap3 >= 1e6 * tol and gapx > tol
    return dev
