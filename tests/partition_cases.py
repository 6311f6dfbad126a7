"""Shared cases of the partition-over-a-mask tests (test_partition_masks.py on the CPU, test_gpu_partition_masks.py on the device): the
meshes, masks, states and references of poison_cases.py, cut into ranks.

Every other multi-rank test of the suite builds its oracle with maxLevelEdgeTop = K, and so every wave of the partitioned device path
takes the "regular entity, every level active" branch.  Here every rank gets its rows of the basin mask (mlt[lm.edges_g]) and, in most
cases, NaN on the poison set of the WHOLE mesh, and the assembled owned rows must be `poison_cases.same` as the single-domain reference
over whole fields, inactive levels included.

emulate() is the partitioned step on the CPU with the oracle as each rank's compute: a local mesh from parallel.build_local, the local
mask, the halo rows overwritten from the owners after stages 1 to 3 and after the step (Forward Euler: the new level after the step, as
dist_worker.py's cpu mode does it).  It shares no code with the device path beyond build_local, and test_partition_masks.py shows that
it reproduces the references the device tests compare with -- so those references are reachable by a correct partitioned
implementation -- and that three wrong ones (ranks that ignore the mask, ranks that index it locally, an exchange that forgets a
neighbour) do not.

conditions() reads the host plan of every rank (lib.Plan, no device): how many patches the boundary, interior and halo classes hold,
how many of them are land, mixed or full, and what depth the sent edge rows have.

No module here imports device code; every result is computed once per case and shared, and no test modifies one."""
import numpy as np

import oracle as orc
import poison_cases as pc
import tracer_cases as tc
from moka_hip import lib as L
from moka_hip import parallel as par

_cached = pc._cached

# ---- the cases both files run ---------------------------------------------------------------------------------------------------------
# Linear RK4: (meshname, K, world, how, overlap, poison, patch_cells, variant); how = "direct" | "buffered" | "whole" (step_rk4_whole:
# every stage one launch over the local mesh).  planar K = 8 / ico12f K = 5: the generic form; K = 34, 60, 64: the patch forms, K = 64
# in patches of 48 cells; variant 3: the generic kernels at a patch-form K.  The None case separates "the mask is wrong" from "poison
# leaked".
LINEAR_CASES = [("planar", 8, 3, "direct", 1, "nan", 0, 0),
                ("planar", 34, 2, "direct", 1, "nan", 0, 0),
                ("planar", 34, 3, "buffered", 0, "nan", 0, 0),
                ("planar", 34, 3, "direct", 0, "-inf", 0, 0),
                ("planar", 34, 2, "direct", 1, None, 0, 0),
                ("ico12f", 5, 5, "direct", 1, "nan", 0, 0),
                ("ico12f", 60, 3, "direct", 1, "nan", 0, 0),
                ("ico12f", 60, 5, "buffered", 1, "nan", 0, 0),
                ("planar", 64, 2, "direct", 1, "nan", 48, 0),
                ("planar", 34, 2, "buffered", -1, "nan", 0, 3),
                ("planar", 34, 3, "whole", -1, "nan", 0, 0)]
LINEAR_STEPS = (2, 4)
# fp32 storage (reference form "mixed"): (meshname, K, world, how)
FP32_CASES = [("planar", 80, 3, "direct"), ("planar", 4, 2, "buffered")]
# Forward Euler: (meshname, K, flags, world, how, state_bytes)
FE_CASES = [("planar", 34, 3, 3, "direct", 8), ("planar", 8, 0, 2, "buffered", 8), ("ico12f", 5, 1, 5, "direct", 8),
            ("planar", 80, 3, 2, "direct", 4)]
# Nonlinear terms, two rings: (meshname, K, world, how, patch_cells); how = "alternate" (buffered, step_rk4 and step_rk4_whole in
# turn), "direct", "whole" (the per-patch kernels do not serve the shape -- K below 34, heptagons, or patches of 48 cells, whose own
# edges outnumber the 96 the kernels' LDS records hold: whole-mesh stages only)
NL_CASES = [("planar", 34, 2, "alternate", 0), ("planar", 34, 2, "direct", 0), ("planar", 8, 3, "whole", 0), ("ico12f", 5, 3, "whole", 0),
            ("planar", 64, 2, "whole", 48)]
NL_MODES = ("nonlinear", "nonlinear+del2")
# Reverse mode: RK4 (meshname, K, world, overlap, poison) over two steps; Forward Euler (meshname, K, flags, world) over ADJ_FE_STEPS
ADJ_RK4_CASES = [("planar", 34, 3, True, "nan"), ("planar", 34, 3, False, "nan"), ("planar", 8, 2, True, "nan"),
                 ("ico12f", 5, 5, True, "nan"), ("planar", 34, 3, True, None)]
ADJ_RK4_STEPS = 2
ADJ_FE_CASES = [("planar", 34, 3, 3), ("planar", 8, 0, 2), ("ico12f", 5, 3, 5)]
ADJ_FE_STEPS = 2
# The plans of all these cases (conditions()): (meshname, K, world, rings, patch_cells, state_bytes)
PLAN_CASES = sorted({(c[0], c[1], c[2], 1, c[6], 8) for c in LINEAR_CASES} | {(m, K, w, 1, 0, 4) for m, K, w, _ in FP32_CASES}
                    | {(m, K, w, 1, 0, sb) for m, K, _, w, _, sb in FE_CASES} | {(m, K, w, 2, P, 8) for m, K, w, _, P in NL_CASES}
                    | {(m, K, w, 1, 0, 8) for m, K, w, _, _ in ADJ_RK4_CASES} | {(m, K, w, 1, 0, 8) for m, K, _, w in ADJ_FE_CASES})


# ---- local meshes ---------------------------------------------------------------------------------------------------------------------
def locals_of(meshname, world, rings):
    def make():
        mesh = tc.get_mesh(meshname)
        part = par.partition_cells(mesh, world)
        return [par.build_local(mesh, part, r, world, rings=rings, vertex_fields=rings == 2) for r in range(world)]
    return _cached(("locals", meshname, world, rings), make)


def _nbr_rows(lm, i):
    return (lm.recv_cells[lm.recv_cell_off[i]:lm.recv_cell_off[i + 1]], lm.recv_edges[lm.recv_edge_off[i]:lm.recv_edge_off[i + 1]])


def exchange(lms, fields, skip=None):
    """fields[r] = (ssh, u, h) of rank r, local; every rank's halo rows := the sending rank's rows.  skip = (r, i): rank r forgets what
    its neighbour number i sends (the third mutant)."""
    new = []
    for r, lm in enumerate(lms):
        ssh, u, h = (a.copy() for a in fields[r])
        for i, q in enumerate(lm.neighbors):
            if skip == (r, i):
                continue
            c, e = _nbr_rows(lm, i)
            qs, qu, qh = fields[q]
            sc, se = lms[q].g2l_c[lm.cells_g[c]], lms[q].g2l_e[lm.edges_g[e]]
            assert (sc >= 0).all() and (se >= 0).all()
            ssh[c], h[c], u[e] = qs[sc], qh[sc], qu[se]
        new.append((ssh, u, h))
    return new


def assemble(mesh, K, lms, rows, where):
    """The whole-mesh array of the ranks' owned rows; rows[r] = a local array on "cell", "edge" or "vertex"."""
    n = {"cell": mesh.nCells, "edge": mesh.nEdges, "vertex": mesh.nVertices}[where]
    out = np.full((n,) + np.shape(rows[0])[1:], np.nan)
    seen = np.zeros(n, dtype=np.int64)
    for lm, a in zip(lms, rows):
        m, ids = {"cell": (lm.owned_cell_mask, lm.cells_g), "edge": (lm.owned_edge_mask, lm.edges_g),
                  "vertex": (lm.owned_vert_mask, lm.verts_g)}[where]
        out[ids[m]] = a[m]
        seen[ids[m]] += 1
    assert (seen == 1).all()                      # every entity is reported by exactly one rank
    return out


def local_masks(meshname, K, lms, mutant):
    mlt = pc.mask_of(meshname, K)
    if mutant == "no-mask":
        return [np.full(lm.mesh.nEdges, K, dtype=np.int32) for lm in lms]
    if mutant == "local-index":
        return [np.ascontiguousarray(mlt[:lm.mesh.nEdges]) for lm in lms]
    return [np.ascontiguousarray(mlt[lm.edges_g]) for lm in lms]


def _rank_meshes(meshname, K, lms, mutant):
    rest = tc.state_of(meshname, K)[3]
    return [orc.OracleMesh(lm.mesh, K, resting_thickness_sum=rest.sum(1)[lm.cells_g], max_level_edge_top=m)
            for lm, m in zip(lms, local_masks(meshname, K, lms, mutant))]


def _tendencies(om, base, u, h, mixed):
    """(tendU, tendH) as the oracle's RK4 step uses them between its stages: unrounded, also for fp32-stored states."""
    if base is not None:
        return base.tendencies(u, h)[:2]
    u, h = np.ascontiguousarray(u), np.ascontiguousarray(h)
    tu, th, ssh, s1, s2 = np.zeros_like(u), np.zeros_like(h), np.zeros(om.mesh.nCells), np.zeros_like(u), np.zeros_like(u)
    fn = orc.lib().oracle_tendencies_mixed if mixed else orc.lib().oracle_tendencies_clean
    fn(om.ref, orc._p(tu), orc._p(th), orc._p(u), orc._p(h), orc._p(ssh), orc._p(s1), orc._p(s2))
    return tu, th


def _ssh(om, h, mixed):
    s = om.update_ssh(h)
    return s.astype(np.float32).astype(np.float64) if mixed else s


# ---- the emulation --------------------------------------------------------------------------------------------------------------------
def emulate(meshname, K, world, mode, poison, nsteps, mixed=False, mutant=None):
    """The assembled owned rows {"u1", "h1", "ssh1"} after each of `nsteps` partitioned RK4 steps of the dycore `mode` ("linear",
    "nonlinear", "nonlinear+del2"; the nonlinear ones on two-ring local meshes).  The arithmetic between the tendencies is
    oracle_step_rk4's (time_integration.jl:61-148), storage rounded to fp32 where `mixed`.  mutant: None, "no-mask", "local-index",
    "skip-neighbour" (the last rank forgets its last neighbour)."""
    def make():
        mesh = tc.get_mesh(meshname)
        rings = pc.RINGS[mode]
        lms = locals_of(meshname, world, rings)
        oms = _rank_meshes(meshname, K, lms, mutant)
        v2 = tc.viscosities(mesh, tc.dt_of(meshname))[0]
        bases = [None if mode == "linear" else orc.OracleNonlinear(om, visc_del2=v2 if mode == "nonlinear+del2" else 0.0) for om in oms]
        skip = (world - 1, len(lms[-1].neighbors) - 1) if mutant == "skip-neighbour" else None
        rnd = (lambda a: a.astype(np.float32).astype(np.float64)) if mixed else (lambda a: a)
        (ssh, u, h, _), _ = pc.state(meshname, K, mode, poison)
        cur = [(rnd(ssh[lm.cells_g]), rnd(u[lm.edges_g]), rnd(h[lm.cells_g])) for lm in lms]
        dt = tc.dt_of(meshname)
        a, b = [dt / 2., dt / 2., dt], [dt / 6., dt / 3., dt / 3., dt / 6.]
        out = []
        for _ in range(nsteps):
            prov = [tuple(x.copy() for x in f) for f in cur]
            new = [tuple(x.copy() for x in f) for f in cur]
            for s in range(4):
                tend = [_tendencies(oms[r], bases[r], prov[r][1], prov[r][2], mixed) for r in range(world)]
                if s < 3:
                    prov = []
                    for r in range(world):
                        pu, ph = rnd(cur[r][1] + a[s] * tend[r][0]), rnd(cur[r][2] + a[s] * tend[r][1])
                        prov.append((_ssh(oms[r], ph, mixed), pu, ph))
                    prov = exchange(lms, prov, skip)
                new = [(new[r][0], rnd(new[r][1] + b[s] * tend[r][0]), rnd(new[r][2] + b[s] * tend[r][1])) for r in range(world)]
            cur = exchange(lms, [(_ssh(oms[r], new[r][2], mixed), new[r][1], new[r][2]) for r in range(world)], skip)
            out.append({"u1": assemble(mesh, K, lms, [f[1] for f in cur], "edge"),
                        "h1": assemble(mesh, K, lms, [f[2] for f in cur], "cell"),
                        "ssh1": assemble(mesh, K, lms, [f[0] for f in cur], "cell")})
        return out
    return _cached(("emulate", meshname, K, world, mode, poison, nsteps, mixed, mutant), make)


FE_FIELDS = {"u1": "edge", "h1": "cell", "ssh1": "cell", "hEdge": "edge", "F": "edge", "div": "cell", "vort": "vertex", "tendU": "edge",
             "tendH": "cell"}


def emulate_fe(meshname, K, world, flags, poison, nsteps, mixed=False, mutant=None):
    """The assembled owned rows of FE_FIELDS after each of `nsteps` partitioned Forward-Euler steps: every rank steps its local oracle
    state, then only the new level is exchanged (the carried layerThicknessEdge and the accumulating relativeVorticity of every
    reported entity are local)."""
    def make():
        mesh = tc.get_mesh(meshname)
        lms = locals_of(meshname, world, 1)
        oms = _rank_meshes(meshname, K, lms, mutant)
        skip = (world - 1, len(lms[-1].neighbors) - 1) if mutant == "skip-neighbour" else None
        (ssh, u, h, _), _ = pc.state(meshname, K, "linear", poison)
        sts = [orc.OracleState(om, ssh[lm.cells_g], u[lm.edges_g], h[lm.cells_g], mixed=mixed) for om, lm in zip(oms, lms)]
        out = []
        for _ in range(nsteps):
            for st in sts:
                st.step_fe(tc.dt_of(meshname), flags)
            got = exchange(lms, [(st.ssh[1], st.u[1], st.h[1]) for st in sts], skip)
            for st, (s_, u_, h_) in zip(sts, got):
                st.ssh[1][...], st.u[1][...], st.h[1][...] = s_, u_, h_
            f = lambda st, n: {"u1": st.u[1], "h1": st.h[1], "ssh1": st.ssh[1]}.get(n, getattr(st, n, None))     # noqa: E731
            out.append({n: assemble(mesh, K, lms, [f(st, n).copy() for st in sts], w) for n, w in FE_FIELDS.items()})
        return out
    return _cached(("emulate_fe", meshname, K, world, flags, poison, nsteps, mixed, mutant), make)


def FE_TAIL_FLAGS(flags, mixed):
    return 0 if mixed else flags


def fe_rk4_fe(meshname, K, flags, poison, mixed=False):
    """{"u1", "h1", "ssh1"} of the single-domain oracle after pc.FE_STEPS Forward-Euler steps, one RK4 step and one more Forward-Euler
    step (the tail of test_forward_euler_on_a_partitioned_mesh: the ranks' buffer sets stay aligned across the two integrators).
    fp32-stored states have no DiagnosticVars behind an RK4 step, so their last step carries nothing over (flags 0), as in
    test_forward_euler_of_fp32_storage_states_on_a_partitioned_mesh."""
    def make():
        (ssh, u, h, _), _ = pc.state(meshname, K, "linear", poison)
        st = orc.OracleState(tc.oracle_mesh(meshname, K, False, pc.mask_of(meshname, K)), ssh, u, h, mixed=mixed)
        dt = tc.dt_of(meshname)
        for _ in range(pc.FE_STEPS):
            st.step_fe(dt, flags)
        st.step_rk4(dt)
        st.step_fe(dt, FE_TAIL_FLAGS(flags, mixed))
        return {"u1": st.u[1].copy(), "h1": st.h[1].copy(), "ssh1": st.ssh[1].copy()}
    return _cached(("fe_rk4_fe", meshname, K, flags, poison, mixed), make)


# ---- what the host plans of the ranks hold --------------------------------------------------------------------------------------------
def conditions(meshname, K, world, rings=1, patch_cells=0, state_bytes=8):
    """Per rank a dict: "lanes" / "lds" = lanesPerColumn / ldsBytesPerBlock of the plan's info (what the device mesh reports too); "patches" = (boundary, interior, halo) patch counts; "boundary" / "interior" = {"land", "mixed", "full",
    "partial"}: patches of the class whose edges are all land (top 0), all full columns (top K) or neither, and -- what condition (a)
    asks -- patches with at least one edge of partial depth (0 < top < K); "sent" = {"land", "partial", "full"}: sent edge rows."""
    def make():
        rest = tc.state_of(meshname, K)[3]
        lms = locals_of(meshname, world, rings)
        out = []
        for lm, mlt in zip(lms, local_masks(meshname, K, lms, None)):
            plan = L.Plan(lm.mesh, K, resting_thickness_sum=rest.sum(1)[lm.cells_g], max_level_edge_top=mlt, ordering=0,
                          patch_cells=patch_cells, cell_class=lm.cell_class, state_bytes=state_bytes)
            pS = plan.class_ranges()[0]
            form = {"lanes": plan.info["lanesPerColumn"], "lds": plan.info["ldsBytesPerBlock"]}
            es = plan.patch_ranges()[1]
            top = mlt[plan.permutation(L.EDGE)]                     # in plan order
            plan.close()
            kinds = {}
            for name, (p0, p1) in (("boundary", (pS[0], pS[1])), ("interior", (pS[1], pS[2]))):
                k = {"land": 0, "mixed": 0, "full": 0, "partial": 0}
                for p in range(p0, p1):
                    t = top[es[p]:es[p + 1]]
                    if t.size == 0:
                        continue
                    k["land" if (t == 0).all() else "full" if (t == K).all() else "mixed"] += 1
                    k["partial"] += int(((t > 0) & (t < K)).any())
                kinds[name] = k
            sent = mlt[lm.send_edges]
            out.append({"patches": (int(pS[1] - pS[0]), int(pS[2] - pS[1]), int(pS[-1] - pS[2])), **kinds, **form,
                        "sent": {"land": int((sent == 0).sum()), "partial": int(((sent > 0) & (sent < K)).sum()),
                                 "full": int((sent == K).sum())}})
        return out
    return _cached(("conditions", meshname, K, world, rings, patch_cells, state_bytes), make)


def conditions_table(cases=None):
    """The per-rank table of conditions() as text (profiles/partition_masks_summary.txt)."""
    lines = ["mesh    K  world rings P  sb rank | patches b/i/h | boundary land/mixed/full (partial) | interior land/mixed/full (partial) | "
             "sent rows land/partial/full | lanes, LDS bytes"]
    for meshname, K, world, rings, P, sb in (PLAN_CASES if cases is None else cases):
        for r, c in enumerate(conditions(meshname, K, world, rings, P, sb)):
            b, i, s = c["boundary"], c["interior"], c["sent"]
            lines.append(f"{meshname:7s} {K:2d} {world:5d} {rings:5d} {P:2d} {sb:2d} {r:4d} | {c['patches'][0]:3d} {c['patches'][1]:3d} "
                         f"{c['patches'][2]:3d}   | {b['land']:3d} {b['mixed']:3d} {b['full']:3d} ({b['partial']:3d})              | "
                         f"{i['land']:3d} {i['mixed']:3d} {i['full']:3d} ({i['partial']:3d})              | "
                         f"{s['land']:4d} {s['partial']:4d} {s['full']:4d}            | {c['lanes']:2d} {c['lds']:6d}")
    return "\n".join(lines)
