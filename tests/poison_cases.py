"""Shared cases of the poison tests (test_poison_twin.py on the CPU, test_gpu_poison.py on the device): a bathymetry-like edge mask,
the levels no active element may read, NaN (or -inf) written there, and comparisons that know about NaN.

The reference steps skip an empty edgesOnCell slot, an edgesOnEdge entry of 0 and every level k >= maxLevelEdgeTop[e].  A kernel that
multiplied by a zero weight instead, or computed and then dropped the result, has the same bits as long as every level holds a benign
number -- and turns the ocean into NaN with the first file that carries fill values below the sea floor.  These cases tell the two
apart: whatever lies on the poison set must stay there.

Mask ("basin").  s = xEdge scaled to [0, 1] on planar meshes, (1 + zEdge / radius) / 2 on the sphere; f = 1.3 s - 0.15;
maxLevelEdgeTop[e] = clip(rint(K f), 0, K): land (0), full columns (K: the kernels' plain branches) and every depth between; on the
periodic planar mesh a cliff from K to 0.

Neighbourhood N(e): e, the edges that share a cell or a vertex with e, edgesOnEdge(e), and the edges whose edgesOnEdge list names e.
top_R = the max of maxLevelEdgeTop over N, taken R times.  u[k, e] is poisoned for k >= top_R[e] (0-based k); R = 1 for the linear
dycore, 2 for the nonlinear one (with Del2 mixing too: its bracket reads the divergence and the curl beside the edge, which the
potential vorticity already does), 3 with Del2 + Del4 (one more ring per nested stencil).  Cell fields (tracers, adjoint seeds) are
poisoned for k >= the max of top_2 over the cell's edges.

Active sets A (what must stay finite and keep the bits of the unpoisoned run): edges k < maxLevelEdgeTop[e]; cells and vertices
k < the max of maxLevelEdgeTop over their edges.  layerThickness is never poisoned: ssh is a column sum over all K levels.

Every reference is computed once per (case, poison) and shared; no test modifies one."""
import numpy as np

import oracle as orc
import tracer_adjoint_twin as ta
import tracer_biharmonic_twin as tb
import tracer_cases as tc
import tracer_kgrad_twin as tk
import tracer_source_twin as ts
from del4_twin import Del4Twin, TwinState
from masks import basin  # noqa: F401  (the mask of the docstring; tests name it poison_cases.basin)

VALUES = {None: None, "nan": np.nan, "-inf": -np.inf}
RINGS = {"linear": 1, "nonlinear": 2, "nonlinear+del2": 2, "del2+del4": 3}
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- the mask and the sets ------------------------------------------------------------------------------------------------------------
def mask_of(meshname, K):
    return _cached(("mlt", meshname, K), lambda: basin(tc.get_mesh(meshname), K))


def _table(conn, count=None):
    """(0-based ids, valid) of a 1-based connectivity table with 0 = none (and, with count, only its first count[i] slots)."""
    conn = np.asarray(conn, dtype=np.int64)
    valid = conn > 0
    if count is not None:
        valid &= np.arange(conn.shape[1])[None, :] < np.asarray(count)[:, None]
    return np.where(valid, conn - 1, 0), valid


def neighbourhood(mesh):
    """(a, b): b[i] is in N(a[i]), as two index arrays (pairs may repeat)."""
    def make():
        nE = mesh.nEdges
        a, b = [np.arange(nE)], [np.arange(nE)]
        for ids, valid in (_table(mesh.edgesOnCell, mesh.nEdgesOnCell), _table(np.asarray(mesh.edgesOnVertex)[:, :mesh.vertexDegree])):
            for i in range(ids.shape[1]):
                for j in range(ids.shape[1]):
                    ok = valid[:, i] & valid[:, j]
                    a.append(ids[ok, i]); b.append(ids[ok, j])
        ids, valid = _table(mesh.edgesOnEdge, mesh.nEdgesOnEdge)
        own = np.repeat(np.arange(nE)[:, None], ids.shape[1], axis=1)
        a += [own[valid], ids[valid]]
        b += [ids[valid], own[valid]]
        return np.concatenate(a), np.concatenate(b)
    return _cached(("N", id(mesh)), make)


def top(mesh, mlt, R):
    a, b = neighbourhood(mesh)
    t = np.asarray(mlt, dtype=np.int64)
    for _ in range(R):
        t2 = t.copy()
        np.maximum.at(t2, a, t[b])
        t = t2
    return t


def cell_max(mesh, t):
    ids, valid = _table(mesh.edgesOnCell, mesh.nEdgesOnCell)
    return np.where(valid, np.asarray(t)[ids], 0).max(axis=1)


def vertex_max(mesh, t):
    ids, valid = _table(np.asarray(mesh.edgesOnVertex)[:, :mesh.vertexDegree])
    return np.where(valid, np.asarray(t)[ids], 0).max(axis=1)


def _below(t, K):
    return np.arange(K)[None, :] >= np.asarray(t)[:, None]


def edge_poison(mesh, mlt, K, R):
    return _below(top(mesh, mlt, R), K)


def cell_poison(mesh, mlt, K):
    return _below(cell_max(mesh, top(mesh, mlt, 2)), K)


def active(mesh, mlt, K, where):
    """The active set A of a field on "edge", "cell" or "vertex"; "all": every element (layerThickness, ssh and what only reads them)."""
    if where == "all":
        return None
    t = {"edge": lambda: mlt, "cell": lambda: cell_max(mesh, mlt), "vertex": lambda: vertex_max(mesh, mlt)}[where]()
    return ~_below(t, K)


def put(a, mask, poison):
    return a if poison is None else np.where(mask, VALUES[poison], a)


# ---- comparisons ----------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same(got, ref):
    """NaN equals NaN whatever its payload; everything else, the infinities and the sign of zero included, compares by bits."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return False
    gn, rn = np.isnan(got), np.isnan(ref)
    return bool(np.array_equal(gn, rn) and np.array_equal(_bits(got)[~gn], _bits(ref)[~rn]))


def same_where_finite(got, ref):
    """Where the reference is finite, the same bits; elsewhere anything."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return False
    fin = np.isfinite(ref)
    return bool(np.array_equal(_bits(got)[fin], _bits(ref)[fin]))


def differences(got, ref):
    """For assertion messages: (elements whose NaN-ness differs, other elements whose bits differ)."""
    got, ref = np.asarray(got), np.asarray(ref)
    gn, rn = np.isnan(got), np.isnan(ref)
    return int((gn != rn).sum()), int(((_bits(got) != _bits(ref)) & ~gn & ~rn).sum())


def closed(clean, poisoned, act):
    """The condition of the CPU file: on the active set `act` (None = everywhere) the poisoned reference is finite and has the bits of
    the unpoisoned one.  Returns the finite share of the whole field."""
    sel = np.ones(np.shape(clean), dtype=bool) if act is None else act
    assert np.isfinite(np.asarray(poisoned)[sel]).all(), "the reference spreads poison into the active set"
    assert np.array_equal(_bits(poisoned)[sel], _bits(clean)[sel]), "the reference's active set changes under poison"
    return float(np.isfinite(poisoned).mean())


# ---- states ---------------------------------------------------------------------------------------------------------------------------
def state(meshname, K, mode, poison):
    """(ssh, u, h, rest) of tc.state_of with u poisoned on the edge set of the dycore `mode`; (mask of that set) second."""
    mesh, mlt = tc.get_mesh(meshname), mask_of(meshname, K)
    ssh, u, h, rest = tc.state_of(meshname, K)
    pe = edge_poison(mesh, mlt, K, RINGS[mode])
    return (ssh, put(u, pe, poison), h, rest), pe


def base_of(om, mesh, meshname, mode, visc2=True):
    if mode == "linear":
        return None
    if mode == "nonlinear":
        return orc.OracleNonlinear(om)
    v2, v4 = tc.viscosities(mesh, tc.dt_of(meshname))
    if mode == "nonlinear+del2":
        return orc.OracleNonlinear(om, visc_del2=v2)
    return Del4Twin(om, visc_del2=v2 if visc2 else 0.0, visc_del4=v4)


def _levels(st):
    return {"u1": st.u[1].copy(), "h1": st.h[1].copy(), "ssh1": st.ssh[1].copy(), "u0": st.u[0].copy(), "h0": st.h[0].copy(),
            "tendU": np.array(st.tendU), "tendH": np.array(st.tendH)}


RK4_ACTIVE = {"u1": "edge", "u0": "edge", "tendU": "edge", "h1": "all", "h0": "all", "ssh1": "all", "tendH": "all"}


def rk4(meshname, K, mode, poison, checkpoints, form="ref"):
    """The fields after checkpoints[0], checkpoints[1], ... RK4 steps; form: "ref", "s13" (linear: the 13-stream twin), "mixed" (linear:
    the fp32-storage oracle)."""
    def make():
        mesh = tc.get_mesh(meshname)
        (ssh, u, h, _), _ = state(meshname, K, mode, poison)
        om = tc.oracle_mesh(meshname, K, False, mask_of(meshname, K))
        base, dt = base_of(om, mesh, meshname, mode), tc.dt_of(meshname)
        st = TwinState(ssh, u, h) if mode == "del2+del4" else orc.OracleState(om, ssh, u, h, mixed=form == "mixed")
        out = []
        for n in range(1, max(checkpoints) + 1):
            if mode == "linear":
                (st.step_rk4_s13 if form == "s13" else st.step_rk4)(dt)
            else:
                base.step_rk4(st, dt)
            if n in checkpoints:
                out.append(_levels(st))
        return out
    return _cached(("rk4", meshname, K, mode, poison, tuple(checkpoints), form), make)


TEND_ACTIVE = {"tendU": "edge", "tendH": "all", "ssh": "all"}


def tendency(meshname, K, mode, poison, mixed=False):
    def make():
        mesh = tc.get_mesh(meshname)
        (ssh, u, h, _), _ = state(meshname, K, mode, poison)
        om = tc.oracle_mesh(meshname, K, False, mask_of(meshname, K))
        t = om.tendencies_clean(u, h, mixed=mixed) if mode == "linear" else base_of(om, mesh, meshname, mode).tendencies(u, h)
        return {"tendU": t[0], "tendH": t[1], "ssh": t[2]}
    return _cached(("tend", meshname, K, mode, poison, mixed), make)


FE_ACTIVE = {"ssh0": "all", "ssh1": "all", "u0": "edge", "u1": "edge", "h0": "all", "h1": "all", "hEdge": "all", "F": "edge",
             "div": "cell", "vort": "vertex", "tendU": "edge", "tendH": "all"}


def forward_euler(meshname, K, flags, poison, nsteps, mixed=False):
    """The twelve arrays of Prog / Diag / Tend after each of nsteps Forward-Euler steps."""
    def make():
        (ssh, u, h, _), _ = state(meshname, K, "linear", poison)
        om = tc.oracle_mesh(meshname, K, False, mask_of(meshname, K))
        st = orc.OracleState(om, ssh, u, h, mixed=mixed)
        out = []
        for _ in range(nsteps):
            st.step_fe(tc.dt_of(meshname), flags)
            out.append({"ssh0": st.ssh[0].copy(), "ssh1": st.ssh[1].copy(), "u0": st.u[0].copy(), "u1": st.u[1].copy(),
                        "h0": st.h[0].copy(), "h1": st.h[1].copy(), "hEdge": st.hEdge.copy(), "F": st.F.copy(), "div": st.div.copy(),
                        "vort": st.vort.copy(), "tendU": st.tendU.copy(), "tendH": st.tendH.copy()})
        return out
    return _cached(("fe", meshname, K, flags, poison, nsteps, mixed), make)


def tracers(meshname, K, nT, diff, bih, srcs, wants, poison, nsteps=2, kgrad=()):
    """tracer_biharmonic_twin.reference over the basin mask with u poisoned at R = 1 and, unless kgrad, all tracers (both levels) and
    the seeds poisoned on the cell set.  kgrad = ((j, bits), ...): the densities of tracer_kgrad_twin too (its column sums read every
    level, so only u is poisoned).  A dict: fields, sources, forward (tc.reference's tuple per step), X, grad, G, W, kappa, kappa4."""
    def make():
        mesh, mlt = tc.get_mesh(meshname), mask_of(meshname, K)
        t = tc.twin_of(meshname, K, "linear", False, mlt)
        twin = (tk.KgradTwin if kgrad else tb.TracerBiharmonicTwin)(t.om, t.base, [])
        q = ts.source_fields(meshname, K, 9)
        twin.source = [q[j] if j in srcs else None for j in range(nT)]
        twin.kappa = tc.kappas(meshname, 9)[:nT] if diff else [0.0] * nT
        twin.kappa4 = tb.kappa4s(meshname, 9)[:nT] if bih else [0.0] * nT
        (ssh, u, h, _), _ = state(meshname, K, "linear", poison)
        pc = cell_poison(mesh, mlt, K)
        cp = None if kgrad else poison
        st = TwinState(ssh, u, h)
        f = [put(a, pc, cp) for a in tc.distinct_fields(mesh, K, 9)[:nT]]
        phis = [[a.copy() for a in f], [a.copy() for a in f]]
        fwd = []
        for _ in range(nsteps):
            twin.step_rk4(st, phis, tc.dt_of(meshname))
            fwd.append(([a.copy() for a in phis[0]], [a.copy() for a in phis[1]], st.u[1].copy(), st.h[1].copy(), st.ssh[1].copy()))
        X = [put(x, pc, cp) for x in ta.seeds(mesh, K, 9)[:nT]]
        W = None
        if kgrad:
            grad, G, W = tk.KgradAdjointTwin(twin).sweep_kgrad(twin.tape, [x.copy() for x in X], dict(kgrad), tuple(wants))
        else:
            grad, G = tb.BiharmonicAdjointTwin(twin).sweep(twin.tape, [x.copy() for x in X], tuple(wants))
        return {"fields": f, "sources": list(twin.source), "forward": fwd, "X": X, "grad": grad, "G": G, "W": W,
                "kappa": list(twin.kappa), "kappa4": list(twin.kappa4), "poisoned_share": float(pc.mean())}
    return _cached(("tracers", meshname, K, nT, diff, bih, tuple(srcs), tuple(wants), poison, nsteps, tuple(kgrad)), make)


def adjoint(meshname, K, method, flags, poison, nsteps):
    """d sum(ssh_N^2) / d the initial state over nsteps taped steps: {"ssh", "normalVelocity", "layerThickness", "layerThicknessEdge"}
    (RK4: the first and the last are zero) and the final ssh."""
    def make():
        (ssh, u, h, _), _ = state(meshname, K, "linear", poison)
        om = tc.oracle_mesh(meshname, K, False, mask_of(meshname, K))
        st = orc.OracleState(om, ssh, u, h)
        dt = tc.dt_of(meshname)
        if method == "fe":
            adj = orc.OracleAdjoint(st)
            for _ in range(nsteps):
                adj.step_fe(dt, flags)
            gS, gU, gH, gE = adj.gradient_sum_sq_ssh()
        else:
            adj = orc.OracleAdjointRK4(st)
            for _ in range(nsteps):
                adj.step_rk4(dt)
            gU, gH = adj.gradient_sum_sq_ssh()
            gS, gE = np.zeros_like(st.ssh[1]), np.zeros_like(gU)
        return {"ssh": gS, "normalVelocity": gU, "layerThickness": gH, "layerThicknessEdge": gE, "ssh1": st.ssh[1].copy()}
    return _cached(("adjoint", meshname, K, method, flags, poison, nsteps), make)


# ---- the cases both files run ---------------------------------------------------------------------------------------------------------
# (meshname, K): generic form with 8 lanes; heptagons and pentagons (empty slots); every patch form; with patch_cells = 48 several
# passes and the tail loops; empty slots in the patch form (linear only)
SHAPES = [("planar", 8), ("ico12f", 5), ("planar", 34), ("planar", 64), ("ico12f", 60)]
NONLINEAR_SHAPES = [("planar", 8), ("ico12f", 5), ("planar", 34), ("planar", 64)]
FP32_SHAPES = [("planar", 80), ("planar", 4)]
RK4_STEPS = (2, 9)            # two eager steps, then seven more through moka_run (one eager, the rest replayed from the captured graph)
NL_STEPS = (3,)               # as the kernel-form tests of test_gpu_parity.py / test_gpu_del4.py
FE_STEPS = 4
FE_SHAPES = [("planar", 34), ("planar", 8), ("ico12f", 5)]
ADJOINT_CASES = [("planar", 8, "fe", 0, 3), ("planar", 34, "fe", 1, 3), ("ico12f", 5, "fe", 3, 3), ("planar", 34, "fe", 3, 2),
                 ("planar", 8, "rk4", 0, 2), ("ico12f", 5, "rk4", 0, 2), ("planar", 34, "rk4", 0, 2)]
# (meshname, K, nT, diff, bih, srcs, wants): plain, diffused, diffused + biharmonic, with a source; patch form (3 tracers at K = 34) and
# generic form (5 tracers at K = 8), heptagons
TRACER_CASES = [(m, K, nT, diff, bih, srcs, (0,) if srcs else ())
                for m, K, nT in (("planar", 34, 3), ("planar", 8, 5), ("ico12f", 5, 3))
                for diff, bih, srcs in ((False, False, ()), (True, False, ()), (True, True, ()), (True, True, (0,)))]
# K = 64 in patches of 48 cells: one tracer's rows fit the LDS, so three tracers take three passes of the patch form; with kappa4 not
# even one fits and the step takes the generic form behind the patch form's Laplacian pass
TRACER_CASES += [("planar", 64, 3, True, False, (), ()), ("planar", 64, 3, True, True, (0,), (0,))]
KGRAD_CASES = [("planar", 34, 3), ("planar", 8, 3), ("ico12f", 5, 3)]
KGRAD_FLAGS = ((0, 3), (1, 2), (2, 1))
