"""Reverse mode pinned to the long-double tangent-linear model (tests/trisk_tangent.py): the tangent against Richardson-extrapolated
central differences of trisk_reference's long-double forward runs, and the oracle's adjoint (OracleAdjoint, OracleAdjointRK4) within
the tangent's error bound -- per element at the entries where a partial maxLevelEdgeTop or a zeroed edgesOnEdge slot acts, at
pentagons / heptagons, ssh_0 and hEdge_0, and along three dot-product directions.  Self-tests show the checks rejecting one
transposed weight off by 1e-9, the Coriolis transpose masked by the wrong edge and one gradient element off by 10x its bound.
No GPU needed."""
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

import oracle as orc
import trisk_reference as tr
import trisk_tangent as tt
from moka_hip import meshgen as mg

LD = tr.LD
_MESHES = {}
MESHES = ["ico8", "ico8f", "planar"]
MASKS = ["full", "eoe"]       # eoe: partial masks (0 included) on a mesh with zeroed edgesOnEdge slots


def zero_slots(mesh, n=6, seed=1):
    """A copy of the mesh with n edgesOnEdge slots zeroed, alternately slot 2 (mid-list) and the last listed slot; returns
    (mesh, [(edge, slot, the edge the slot named)]), 0-based."""
    rng = np.random.default_rng(seed)
    eoe = np.asarray(mesh.edgesOnEdge).copy()
    out = []
    for i, e in enumerate(rng.choice(mesh.nEdges, n, replace=False)):
        j = 2 if i % 2 == 0 else int(mesh.nEdgesOnEdge[e]) - 1
        out.append((int(e), j, int(eoe[e, j]) - 1))
        eoe[e, j] = 0
    return dataclasses.replace(mesh, edgesOnEdge=eoe), out


def get_mesh(name, zeroed=False):
    """(mesh, zeroed slots), cached so that the references' per-mesh caches hold."""
    key = (name, zeroed)
    if key not in _MESHES:
        if zeroed:
            _MESHES[key] = zero_slots(get_mesh(name)[0])
        else:
            _MESHES[key] = ({"ico8": lambda: mg.icosahedral_mesh(8),
                             "ico8f": lambda: mg.icosahedral_mesh(8, flips=8, seed=4),      # 5- and 7-gons, W > 10
                             "planar": lambda: mg.planar_hex_mesh(20, 18, 1000.0, f0=1e-4)}[name](), [])
    return _MESHES[key]


def edge_mask(mesh, K, kind, seed=3):
    """full: K everywhere; partial / eoe: maxLevelEdgeTop < K (0 included) on a third of the edges."""
    if kind == "full":
        return np.full(mesh.nEdges, K, dtype=np.int32)
    rng = np.random.default_rng(seed)
    mlt = np.where(rng.random(mesh.nEdges) < 1 / 3, rng.integers(0, K, mesh.nEdges), K).astype(np.int32)
    mlt[:3] = 0
    return mlt


def make_case(mesh, zeroed, K, mask, seed):
    """mask: full, partial, or eoe (partial masks on a mesh with zeroed edgesOnEdge slots)."""
    rng = np.random.default_rng(seed)
    rest = np.full((mesh.nCells, K), 1000.0 / K) + rng.uniform(0, 0.1, (mesh.nCells, K))
    h = rest + rng.uniform(-10, 10, rest.shape)     # ssh of O(10): an entry's dJ is not a small remainder of the column sums
    u = rng.uniform(-1, 1, (mesh.nEdges, K))
    ssh = h.sum(1) - rest.sum(1) + rng.uniform(-0.1, 0.1, mesh.nCells)        # ssh_0 is an independent state variable
    hE = rng.uniform(0.5, 1.5, (mesh.nEdges, K)) * (1000.0 / K)
    dt = 0.2 * float(mesh.dcEdge.min()) / np.sqrt(9.80616 * 1000.0)
    return SimpleNamespace(mesh=mesh, K=K, mlt=edge_mask(mesh, K, mask), rest=rest.sum(1), rest2=rest, zeroed=zeroed, dt=dt,
                           state={"ssh": ssh, "u": u, "h": h, "hE": hE})


def case(meshname, K, mask, seed):
    return make_case(*get_mesh(meshname, mask == "eoe"), K, mask, seed)


def pinned_entries(c, method):
    """Candidate entries by category: levels mlt - 1 and mlt of partially masked edges (u, and hE for Forward Euler), edges with a
    zeroed slot and the edges the slots named, pentagon / heptagon cells, ssh_0 and hE_0 entries, and ordinary ones.  A list of
    (category, (field, index)); check_entries keeps the sharp ones of each category."""
    m, K, mlt = c.mesh, c.K, c.mlt
    E = []
    part = np.flatnonzero(mlt < K)
    for cat, edges in (("edge with mlt = 0", part[mlt[part] == 0][:3]), ("partially masked edge", part[mlt[part] > 0][:4])):
        for e in edges:
            for k in sorted({int(mlt[e]) - 1, int(mlt[e])} & set(range(K))):
                E.append((cat, ("u", (int(e), k))))
                if method == "fe":
                    E.append((cat + " (hE)", ("hE", (int(e), k))))
    for e, _, named in c.zeroed[:4]:
        E += [("edge with a zeroed slot", ("u", (e, 0))), ("edge a zeroed slot named", ("u", (named, K - 1)))]
    n = np.asarray(m.nEdgesOnCell)
    for cat, cells in (("pentagon", np.flatnonzero(n == 5)[:3]), ("heptagon", np.flatnonzero(n == 7)[:3])):
        E += [(cat, ("h", (int(cell), k))) for cell in cells for k in sorted({0, K - 1})]
    E += [("ordinary", ("u", (m.nEdges * i // 5, K // 2))) for i in range(1, 5)]
    E += [("ordinary", ("h", (m.nCells * i // 5, K // 2))) for i in range(1, 5)]
    if method == "fe":
        E += [("ssh_0", ("ssh", i)) for i in (0, m.nCells // 2, m.nCells // 3)]
        E += [("hE_0", ("hE", (m.nEdges // 2, 0)))]
    return E


def directions(c, method, seed=7):
    """Three directions (a leading batch axis of 3): a global Gaussian, one supported only on the partially masked edges, one only
    on the neighbourhoods of the zeroed slots (a zero direction where there are none: the gradient must then give exactly 0)."""
    m, K = c.mesh, c.K
    rng = np.random.default_rng(seed)
    fields = ("u", "h") if method == "rk4" else tt.FIELDS
    shp = tt.shapes(m, K)
    d = {f: np.zeros((3,) + shp[f]) for f in fields}
    for f in fields:
        d[f][0] = rng.standard_normal(shp[f])
    masked = c.mlt < K
    for f in ("u", "hE"):
        if f in d:
            d[f][1][masked] = rng.standard_normal((int(masked.sum()), K))
    g = tr.geometry(m)
    for e, _, named in c.zeroed:
        for x in (e, named):
            d["u"][2][x] = rng.standard_normal(K)
            for cell in (g.c1[x], g.c2[x]):
                d["h"][2][cell] = rng.standard_normal(K)
    return d


DIRECTION_NAMES = ("global", "masked edges", "zeroed slots")


def grad_dict(g, method):
    if method == "rk4":
        return {"u": g[0], "h": g[1]}
    return dict(zip(("ssh", "u", "h", "hE"), g))


SHARP_LIMIT = 1e-9      # a pinned entry's bound is at most this fraction of |dJ|: coarser would hide a one-term error


def check_dirs(c, grad, method, flags, nsteps, dirs, names, what, tangent=None):
    """|<g, v> - dJ| <= C_adj 2^-53 M_d for every direction of the batch; returns (dJ, M_d, largest |err| / bound).
    tangent: (dJ, M_d) of these directions when already computed."""
    C = tt.constant(method, nsteps)
    dJ, Md = tangent if tangent is not None else tt.run(c.mesh, c.mlt, c.rest, c.state, dirs, c.dt, nsteps, method=method,
                                                        flags=flags)
    got = tt.dot(grad, dirs)
    ok = tt.within(got, dJ, Md, C)
    if not ok.all():
        b = int(np.argmin(ok))
        raise AssertionError(f"{what}: {names[b]}: <g, v> = {float(got[b])!r}, tangent {float(dJ[b])!r}, "
                             f"|err| {float(abs(got[b] - dJ[b])):.3e} > bound {float(C * tr.U53 * Md[b]):.3e}")
    return dJ, Md, tt.sharpness(got, dJ, Md, C)[0]


def sharp(c, method, flags, nsteps, cands):
    """The candidates (category, entry) to pin and the tangent at them: per category those whose bound is at most SHARP_LIMIT |dJ|
    or that are structural zeros (M_d == 0: the gradient must be exactly 0 there).  An entry where dJ is a small remainder of
    cancelling paths is too blunt to pin; every category must keep at least one entry."""
    entries = [e for _, e in cands]
    dJ, Md = tt.run(c.mesh, c.mlt, c.rest, c.state, tt.unit_directions(c.mesh, c.K, entries), c.dt, nsteps, method=method,
                    flags=flags)
    bound = tt.constant(method, nsteps) * tr.U53 * Md
    keep = (Md == 0) | (bound <= LD(SHARP_LIMIT) * np.abs(dJ))
    for cat in dict.fromkeys(cat for cat, _ in cands):
        assert any(k for (ct, _), k in zip(cands, keep) if ct == cat), f"no entry of category {cat!r} is sharp enough to pin"
    idx = np.flatnonzero(keep)
    return [entries[i] for i in idx], dJ[idx], Md[idx]


def check_entries(c, grad, method, flags, nsteps, cands, what):
    """Per element at the sharp entries of the candidates; returns (entries, dJ, M_d)."""
    entries, dJ, Md = sharp(c, method, flags, nsteps, cands)
    tol = tt.constant(method, nsteps) * tr.U53 * Md
    assert ((Md == 0) | (tol <= LD(SHARP_LIMIT) * np.abs(dJ))).all()
    check_dirs(c, grad, method, flags, nsteps, tt.unit_directions(c.mesh, c.K, entries), entries, what, tangent=(dJ, Md))
    return entries, dJ, Md


def check(c, grad, method, flags, nsteps, what):
    check_entries(c, grad, method, flags, nsteps, pinned_entries(c, method), what)
    check_dirs(c, grad, method, flags, nsteps, directions(c, method), DIRECTION_NAMES, what)


def oracle_fe(c, flags, nsteps):
    om = orc.OracleMesh(c.mesh, c.K, resting_thickness_sum=c.rest, max_level_edge_top=c.mlt)
    st = orc.OracleState(om, c.state["ssh"], c.state["u"], c.state["h"])
    st.hEdge[...] = c.state["hE"]
    adj = orc.OracleAdjoint(st)
    for _ in range(nsteps):
        adj.step_fe(c.dt, flags)
    return adj


def oracle_rk4(c, nsteps):
    om = orc.OracleMesh(c.mesh, c.K, resting_thickness_sum=c.rest, max_level_edge_top=c.mlt)
    adj = orc.OracleAdjointRK4(orc.OracleState(om, c.state["ssh"], c.state["u"], c.state["h"]))
    for _ in range(nsteps):
        adj.step_rk4(c.dt)
    return adj


# ---- the tangent against central differences of the long-double forward runs ----------------------------------------------------
def forward_J(c, state, method, flags, nsteps):
    if method == "rk4":
        ssh = tr.rk4(c.mesh, state["u"], state["h"], c.rest, c.mlt, c.dt, nsteps, nonlinear=False)[2]
    else:
        ssh = tr.forward_euler(c.mesh, state["u"], state["h"], state["ssh"], c.rest, c.mlt, c.dt, nsteps, hE=state["hE"],
                               stale=bool(flags & tt.STALE))[2]
    return (ssh * ssh).sum()


@pytest.mark.parametrize("method,flags", [("fe", 1), ("rk4", 0)])
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("meshname", MESHES)
def test_tangent_against_central_differences(meshname, K, mask, method, flags):
    """dJ along the three directions == (4 D(eps/2) - D(eps)) / 3, D the central difference of J of trisk_reference's
    long-double forward run, within 1e-10 relative."""
    c = case(meshname, K, mask, 10 + K)
    nsteps = 3 if method == "fe" else 2
    dirs = directions(c, method)
    dJ, _ = tt.run(c.mesh, c.mlt, c.rest, c.state, dirs, c.dt, nsteps, method=method, flags=flags, mags=False)
    base = {f: np.asarray(a, dtype=np.float64).astype(LD) for f, a in c.state.items()}
    for b in range(3):
        def D(eps):
            J = [forward_J(c, {f: base[f] + (s * eps) * dirs[f][b].astype(LD) if f in dirs else base[f] for f in base},
                           method, flags, nsteps) for s in (1, -1)]
            return (J[0] - J[1]) / (2 * eps)
        eps = LD(1e-1)
        R = (4 * D(eps / 2) - D(eps)) / 3
        assert abs(R - dJ[b]) <= LD(1e-10) * abs(dJ[b]), (DIRECTION_NAMES[b], float(R), float(dJ[b]))
    assert dJ[0] != 0


# ---- the oracle's adjoint within the tangent's bound -------------------------------------------------------------------------------
FE_CASES = [(1, 3), (3, 0), (3, 1), (3, 2), (5, 1), (5, 3)]        # (K, flags); flags 7 with (1, 3)


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("K,flags", FE_CASES)
@pytest.mark.parametrize("meshname", MESHES)
def test_oracle_fe_adjoint_within_the_tangent_bound(meshname, K, flags, mask):
    """Forward Euler, three steps, flags 0 - 3 (and 7 at K = 1; flag 1 carries hEdge_0 into the gradient)."""
    c = case(meshname, K, mask, 20 + K)
    check(c, grad_dict(oracle_fe(c, flags, 3).gradient_sum_sq_ssh(), "fe"), "fe", flags, 3, f"FE flags {flags}")
    if K == 1 and flags == 3:
        check(c, grad_dict(oracle_fe(c, 7, 3).gradient_sum_sq_ssh(), "fe"), "fe", 7, 3, "FE flags 7")


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("meshname", MESHES)
def test_oracle_rk4_adjoint_within_the_tangent_bound(meshname, K, mask):
    """RK4, two steps: the gradient has no ssh_0 / hEdge_0 part (the tangent's is 0 there)."""
    c = case(meshname, K, mask, 30 + K)
    check(c, grad_dict(oracle_rk4(c, 2).gradient_sum_sq_ssh(), "rk4"), "rk4", 0, 2, "RK4")


# ---- self-tests: the checks reject a subtly wrong gradient -------------------------------------------------------------------------
# On ico8f (5- and 7-gons, non-uniform weights) with partial masks, three Forward-Euler steps (the Coriolis transpose acts from the
# second step from the end on).  A one-term error is checked by the entries it touches and by a direction supported on them.
def _fails(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


def _columns(c, edges):
    """One direction per edge: u over all levels of that edge."""
    d = np.zeros((len(edges), c.mesh.nEdges, c.K))
    for b, e in enumerate(edges):
        d[b, e] = 1.0
    return {"u": d}


def _selftest_case():
    return case("ico8f", 3, "eoe", 50)


def test_sensitivity_one_transposed_weight_scaled():
    c = _selftest_case()
    adj = oracle_fe(c, 0, 3)
    size = np.abs(adj.tw * np.asarray(c.mesh.fEdge)[:, None]) * (adj.teoe > 0) * (c.mlt == c.K)[:, None]
    e, j = np.unravel_index(int(np.argmax(size)), size.shape)
    good = grad_dict(adj.gradient_sum_sq_ssh(), "fe")
    adj = oracle_fe(c, 0, 3)
    adj.tw = adj.tw.copy()
    adj.tw[e, j] *= 1 + 1e-9
    bad = grad_dict(adj.gradient_sum_sq_ssh(), "fe")
    entries = [("column", ("u", (int(e), k))) for k in range(c.K)]
    dirs = _columns(c, [int(e)])
    check_entries(c, good, "fe", 0, 3, entries, "good")
    check_dirs(c, good, "fe", 0, 3, dirs, ["column"], "good")
    assert _fails(check_entries, c, bad, "fe", 0, 3, entries, "bad")
    assert _fails(check_dirs, c, bad, "fe", 0, 3, dirs, ["column"], "bad")


def fe_gradient_masked_by_the_target(adj):
    """OracleAdjoint.gradient_sum_sq_ssh with the transposed Coriolis sum masked by the target edge's own maxLevelEdgeTop instead of
    the source edge's (k < mlt[e] in place of k < mlt[s]): after each transposed step, lamU0[e, k] += sum_j (tw_ej fEdge_e)
    (dt lamU1[s_j, k]) ([k < mlt_e] - [k < mlt_s_j]) -- what that wrong kernel computes, up to the order of its sum."""
    st, om = adj.st, adj.om
    m, K = om.mesh, om.K
    mlt = om.arrays["maxLevelEdgeTop"]
    act = (np.arange(K)[None, :] < mlt[:, None]).astype(float)
    lamS = 2.0 * st.ssh[1]
    lamU, lamH, lamE = np.zeros((m.nEdges, K)), np.zeros((m.nCells, K)), np.zeros((m.nEdges, K))
    Enew, csum = np.zeros((m.nEdges, K)), np.zeros(m.nEdges)
    src = adj.teoe.astype(np.int64) - 1
    fE = np.asarray(m.fEdge)
    p = orc._p
    for u, hE, dt, flags in reversed(adj.tape):
        oU, oH, oS, oE = np.zeros_like(lamU), np.zeros_like(lamH), np.zeros_like(lamS), np.zeros_like(lamE)
        orc.lib().oracle_step_fe_adjoint(om.ref, p(adj.teoe), p(adj.tw), adj.teoe.shape[1], dt, flags, p(u), p(hE), p(lamU),
                                         p(lamH), p(lamS), p(lamE), p(oU), p(oH), p(oS), p(oE), p(Enew), p(csum))
        for j in range(src.shape[1]):
            s = src[:, j]
            oU += np.where((s >= 0)[:, None], (adj.tw[:, j] * fE)[:, None] * (dt * lamU[s]) * (act - act[s]), 0.0)
        lamU, lamH, lamS, lamE = oU, oH, oS, oE
    return lamS, lamU, lamH, lamE


def test_sensitivity_coriolis_transpose_masked_by_the_wrong_edge():
    c = _selftest_case()
    good = grad_dict(oracle_fe(c, 0, 3).gradient_sum_sq_ssh(), "fe")
    adj = oracle_fe(c, 0, 3)
    bad = grad_dict(fe_gradient_masked_by_the_target(adj), "fe")
    # edges whose own mask differs from a source's: the terms the wrong mask adds or drops
    src = adj.teoe.astype(np.int64) - 1
    differ = ((src >= 0) & (c.mlt[:, None] != c.mlt[np.maximum(src, 0)])).any(axis=1)
    edges = [int(e) for e in np.flatnonzero(differ)[:6]]
    entries = [("columns", ("u", (e, k))) for e in edges for k in range(c.K)]
    dirs = _columns(c, edges)
    check_entries(c, good, "fe", 0, 3, entries, "good")
    check_dirs(c, good, "fe", 0, 3, dirs, edges, "good")
    assert _fails(check_entries, c, bad, "fe", 0, 3, entries, "bad")
    assert _fails(check_dirs, c, bad, "fe", 0, 3, dirs, edges, "bad")
    # and the standard direction supported on the masked edges
    d = directions(c, "fe")
    check_dirs(c, good, "fe", 0, 3, d, DIRECTION_NAMES, "good")
    assert _fails(check_dirs, c, bad, "fe", 0, 3, {f: v[1:2] for f, v in d.items()}, DIRECTION_NAMES[1:2], "bad")


def test_sensitivity_one_gradient_element():
    c = _selftest_case()
    good = grad_dict(oracle_fe(c, 1, 3).gradient_sum_sq_ssh(), "fe")
    entries, dJ, Md = check_entries(c, good, "fe", 1, 3, pinned_entries(c, "fe"), "good")
    tol = tt.constant("fe", 3) * tr.U53 * Md
    for i in (int(np.argmax(tol)), int(np.argmin(np.where(tol > 0, tol, np.inf)))):
        name, idx = entries[i]
        bad = {f: v.copy() for f, v in good.items()}
        bad[name][idx] += 10 * float(tol[i])
        assert _fails(check_entries, c, bad, "fe", 1, 3, [("one", entries[i])], "bad")
        assert _fails(check_dirs, c, bad, "fe", 1, 3, tt.unit_directions(c.mesh, c.K, [entries[i]]), [entries[i]], "bad")
    # a structural zero (hEdge_0 does not enter a run without the stale flag) must come out exactly 0
    good = grad_dict(oracle_fe(c, 0, 3).gradient_sum_sq_ssh(), "fe")
    assert not good["hE"].any()
    good["hE"][c.mesh.nEdges // 2, 0] = 1e-300
    assert _fails(check_entries, c, good, "fe", 0, 3, [("hE_0", ("hE", (c.mesh.nEdges // 2, 0)))], "bad")


