"""The numpy twin of the quadratic bottom drag (tests/quadratic_drag_twin.py; moka_set_quadratic_bottom_drag, moka_bottom_speed) against
its long-double restatement within the counted bound, its identities, the poison cases, the exact decay of a uniform flow, and the
header's text.  No GPU."""
import os
import re

import numpy as np
import pytest

import momentum_vmix_twin as mv
import poison_cases as pc
import quadratic_drag_twin as qd
import tracer_cases as tc
from del4_twin import TwinState
from moka_hip import lib as L

LD = qd.LD
U = qd.U53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = ("planar", "ico12f", "tiny-2-4")
LEVELS = (1, 5, 8)
MASKS = ("full", "partial", "basin")
KINDS = ("cd", "cd+nu+drag+stress")
NAMES = ("moka_set_quadratic_bottom_drag", "moka_quadratic_bottom_drag", "moka_bottom_speed_download", "moka_bottom_speed")


def mask_of(meshname, K, mask):
    mesh = tc.get_mesh(meshname)
    if mask == "full":
        return np.full(mesh.nEdges, K, dtype=np.int32)
    return pc.mask_of(meshname, K) if mask == "basin" else tc.partial_mlt(mesh, K)


def case(meshname, K, mask, kind):
    """(mesh, mlt, u, h, c1, c2, dt, nu, r, tau, cd) of a case: tc.state_of's fields, mv.coefficients and qd.cd_of."""
    mesh, mlt = tc.get_mesh(meshname), mask_of(meshname, K, mask)
    _, u, h, _ = tc.state_of(meshname, K)
    c1, c2 = mv.edge_cells(mesh)
    dt = tc.dt_of(meshname)
    nu, r = mv.coefficients(meshname, K)
    parts = kind.split("+")
    return (mesh, mlt, u, h, c1, c2, dt, nu if "nu" in parts else 0.0, r if "drag" in parts else 0.0,
            mv.stress_field(mesh, K) if "stress" in parts else None, qd.cd_of(K, dt) if "cd" in parts else 0.0)


def depth_groups(mlt, K):
    nn = np.minimum(np.asarray(mlt, dtype=np.int64), K)
    return [(int(n), np.nonzero(nn == n)[0]) for n in np.unique(nn) if n >= 1]


# ---- against the long-double model --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("K", LEVELS)
@pytest.mark.parametrize("meshname", MESHES)
def test_twin_against_the_long_double_model(meshname, K, mask):
    """sp within C_SP roundings of the dense long-double speed; u within the bound quadratic_drag_twin's docstring counts, per element,
    for every depth of the mask; the momentum budget sum_k h u_new - sum_k h u* = dt tau - q_e u_new[n-1] within its own bound."""
    worst = [0.0, 0.0, 0.0]
    for kind in KINDS:
        mesh, mlt, u, h, c1, c2, dt, nu, r, tau, cd = case(meshname, K, mask, kind)
        _, c_sp, c_q = qd.counts(mesh)
        sp, spl = qd.bottom_speed(u, mlt, mesh), qd.speed_ld(u, mlt, mesh)
        live = np.minimum(mlt, K) >= 1
        assert np.all(sp[~live] == 0.0) and np.all(sp[live] > 0.0)
        assert np.all(np.abs(sp - spl) <= c_sp * U * spl)
        worst[0] = max(worst[0], float((np.abs(sp - spl)[live] / (c_sp * U * spl[live])).max()))
        out, used = qd.apply(u, h, mlt, c1, c2, dt, nu, r, tau, cd, mesh)
        assert np.array_equal(used, sp)
        q = np.float64(dt) * (np.float64(r) + np.float64(cd) * sp)
        q_ld = LD(dt) * (LD(r) + LD(cd) * spl)
        s = np.float64(dt) * np.float64(nu)
        done = np.zeros(mesh.nEdges, dtype=bool)
        for n, idx in depth_groups(mlt, K):
            he = 0.5 * (h[c1[idx], :n] + h[c2[idx], :n])
            b = np.float64(dt) * tau[idx] if tau is not None else None
            new, exact, err, mom = qd.bounds(he, u[idx, :n], s, q[idx], q_ld[idx], b, c_q)
            assert np.array_equal(new, out[idx, :n])
            dev = np.abs(new.astype(LD) - exact)
            assert np.all(dev <= U * err), (kind, n)
            worst[1] = max(worst[1], float((dev / (U * err)).max()))
            hl = he.astype(LD)
            lhs = (hl * new).sum(axis=1) - (hl * u[idx, :n]).sum(axis=1)
            drift = np.abs(lhs - ((b.astype(LD) if b is not None else 0) - q[idx].astype(LD) * new[:, -1]))
            assert np.all(drift <= U * mom), (kind, n)
            worst[2] = max(worst[2], float((drift / (U * mom)).max()))
            assert not np.array_equal(new, u[idx, :n])
            done[idx] = True
        dead = np.arange(K)[None, :] >= np.minimum(mlt, K)[:, None]
        assert np.array_equal(out[dead], u[dead]) and np.array_equal(done, live)
    print(f"{meshname} K={K} {mask}: largest |sp^ - sp| / bound = {worst[0]:.3f}, |u^ - u| / bound = {worst[1]:.3f}, "
          f"momentum drift / bound = {worst[2]:.3f}")


# ---- identities ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K,mask", [("planar", 8, "partial"), ("ico12f", 5, "basin"), ("tiny-2-4", 1, "full")])
def test_cd_zero_is_the_linear_pass_and_zero_flow_has_no_speed(meshname, K, mask):
    mesh, mlt, u, h, c1, c2, dt, nu, r, tau, cd = case(meshname, K, mask, "cd+nu+drag+stress")
    lin = mv.apply(u, h, mlt, c1, c2, dt, nu, r, tau)
    out, sp = qd.apply(u, h, mlt, c1, c2, dt, nu, r, tau, 0.0, mesh)
    assert np.array_equal(out, lin) and not sp.any()
    assert not np.array_equal(qd.apply(u, h, mlt, c1, c2, dt, nu, r, tau, cd, mesh)[0], lin)
    # u == 0 in the stencil: sp == 0, r + 0.0 == r, the bits of the linear pass (the stress makes it move)
    z = np.zeros_like(u)
    out0, sp0 = qd.apply(z, h, mlt, c1, c2, dt, nu, r, tau, cd, mesh)
    assert not sp0.any() and np.array_equal(out0, mv.apply(z, h, mlt, c1, c2, dt, nu, r, tau)) and out0.any()
    # Cd alone switches the drag lines on: the n == 1 columns move, dt == 0 changes nothing
    only = qd.apply(u, h, mlt, c1, c2, dt, 0.0, 0.0, None, cd, mesh)[0]
    one = np.minimum(mlt, K) == 1
    assert qd.pass_on(0.0, 0.0, None, mlt, cd) and not qd.pass_on(0.0, 0.0, None, mlt, 0.0)
    assert np.all(only[one, 0] != u[one, 0])
    assert np.array_equal(qd.apply(u, h, mlt, c1, c2, 0.0, nu, r, tau, cd, mesh)[0], u)


@pytest.mark.parametrize("kind", ["cd", "cd+nu", "cd+nu+drag"])
def test_energy_does_not_grow_without_stress(kind):
    """q_e >= 0 keeps A - diag(h) positive semidefinite: sum_k h u_new^2 <= sum_k h u*^2 per column, strictly where the column moves."""
    mesh, mlt, u, h, c1, c2, dt, nu, r, tau, cd = case("planar", 8, "partial", kind)
    out, sp = qd.apply(u, h, mlt, c1, c2, dt, nu, r, tau, cd, mesh)
    ratios = []
    for n, idx in depth_groups(mlt, 8):
        he = (0.5 * (h[c1[idx], :n] + h[c2[idx], :n])).astype(LD)
        e0, e1 = (he * u[idx, :n].astype(LD) ** 2).sum(axis=1), (he * out[idx, :n].astype(LD) ** 2).sum(axis=1)
        assert np.all(e1 < e0), n
        ratios.append(float((e1 / e0).max()))
    print(f"{kind}: largest energy ratio per depth {['%.3f' % x for x in ratios]}")


# ---- poison -------------------------------------------------------------------------------------------------------------------------
POISON = [("planar", 8), ("ico12f", 5)]


@pytest.mark.parametrize("meshname,K", POISON)
def test_the_basin_mask_can_show_a_read_below_a_floor(meshname, K):
    """The poison cases below show something only if some computed edge e (kb = n - 1) has, among the edges of its two cells, an edge e'
    with maxLevelEdgeTop[e'] <= kb: that slot is the one the depth test drops."""
    mesh, mlt = tc.get_mesh(meshname), mask_of(meshname, K, "basin")
    nn = np.minimum(mlt, K).astype(np.int64)
    eoc, cnt, _, _ = qd._stencil(mesh)
    c1, c2 = mv.edge_cells(mesh)
    hits = 0
    for e in np.nonzero(nn >= 1)[0]:
        for c in (c1[e], c2[e]):
            hits += int((nn[eoc[c, :cnt[c]]] <= nn[e] - 1).any())
    print(f"{meshname} K={K}: {hits} (edge, cell) pairs with a shallower edge in the stencil")
    assert hits >= 1


@pytest.mark.parametrize("meshname,K", POISON)
def test_nan_below_the_floors_reaches_nothing_and_a_wrong_twin_shows_it(meshname, K):
    """u = NaN at every level k >= maxLevelEdgeTop[e] (pc.edge_poison with no ring: exactly the levels below an edge's own floor; the
    operator and the pass alone read nothing else, where a dycore step needs the one-ring set).  The speed and the pass are finite on
    the active set and keep the bits of the unpoisoned run; the twin without the `> kb` test turns NaN."""
    mesh, mlt, u, h, c1, c2, dt, nu, r, tau, cd = case(meshname, K, "basin", "cd+nu+drag+stress")
    fill = pc.edge_poison(mesh, mlt, K, 0)
    live = pc.active(mesh, mlt, K, "edge")
    assert fill.mean() > 0.1 and np.array_equal(fill, ~live)
    up = pc.put(u, fill, "nan")
    sp, spp = qd.bottom_speed(u, mlt, mesh), qd.bottom_speed(up, mlt, mesh)
    assert np.all(np.isfinite(spp)) and np.array_equal(sp, spp)
    clean, got = qd.apply(u, h, mlt, c1, c2, dt, nu, r, tau, cd, mesh)[0], qd.apply(up, h, mlt, c1, c2, dt, nu, r, tau, cd, mesh)[0]
    assert np.all(np.isfinite(got[live])) and np.array_equal(got[live], clean[live]) and np.all(np.isnan(got[fill]))
    wrong = qd.bottom_speed_wrong(up, mlt, mesh)
    assert np.isnan(wrong).any()
    assert np.isnan(qd.apply(up, h, mlt, c1, c2, dt, nu, r, tau, cd, mesh, speed=qd.bottom_speed_wrong)[0][live]).any()
    # ... and without poison the wrong twin is merely different
    assert not np.array_equal(qd.bottom_speed_wrong(u, mlt, mesh), sp)


@pytest.mark.parametrize("meshname,K", POISON)
def test_steps_under_the_one_ring_poison(meshname, K):
    """Three steps of the twin chain over the basin with u NaN on the linear dycore's poison set (one ring): the active levels stay finite
    and keep the bits of the unpoisoned run."""
    mesh, mlt = tc.get_mesh(meshname), mask_of(meshname, K, "basin")
    ssh, u, h, _ = tc.state_of(meshname, K)
    nu, r = mv.coefficients(meshname, K)
    fill, live = pc.edge_poison(mesh, mlt, K, 1), pc.active(mesh, mlt, K, "edge")
    res = []
    for uu in (u, pc.put(u, fill, "nan")):
        tw = qd.quadratic_twin(meshname, K, mlt=mlt, nu=nu, drag=r, tau=mv.stress_field(mesh, K), cd=qd.cd_of(K, tc.dt_of(meshname)))
        st = TwinState(ssh, uu, h)
        for _ in range(3):
            tw.step_rk4(st, [[], []], tc.dt_of(meshname))
        res.append((st.u[1].copy(), tw.sp.copy()))
    assert np.all(np.isfinite(res[1][0][live])) and np.array_equal(res[1][0][live], res[0][0][live]) and np.all(np.isnan(res[1][0][fill]))
    assert np.array_equal(res[1][1], res[0][1])


# ---- the twin chain -----------------------------------------------------------------------------------------------------------------
def test_twin_chain_step_then_pass():
    ssh, u, h, _ = tc.state_of("tiny-2-4", 5)
    nu, r = mv.coefficients("tiny-2-4", 5)
    cd = qd.cd_of(5, 2.0)
    a, b, c = (TwinState(ssh, u, h) for _ in range(3))
    tw = qd.quadratic_twin("tiny-2-4", 5, nu=nu, drag=r, cd=cd)
    tw.step_rk4(a, [[], []], 2.0)
    lin = mv.momentum_twin("tiny-2-4", 5, nu=nu, drag=r)
    lin.step_rk4(b, [[], []], 2.0)
    assert np.array_equal(a.h[1], b.h[1]) and not np.array_equal(a.u[1], b.u[1]) and tw.sp.all()
    qd.quadratic_twin("tiny-2-4", 5, nu=nu, drag=r).step_rk4(c, [[], []], 2.0)
    assert np.array_equal(c.u[1], b.u[1])


# ---- exact decay --------------------------------------------------------------------------------------------------------------------
def test_exact_decay_of_a_uniform_flow():
    """1 / u_{m+1} = 1 / u_m + dt Cd / h: after N steps u_e(N) (1 + N dt Cd |U_0| / h) = u_e(0) within the bound quadratic_drag_twin's
    docstring counts (nothing fitted); the same bound refuses a run without the drag and the linearised drag by a factor >= 1e6."""
    mesh, (ssh, u, h, _), U0 = qd.decay_state()
    cd = qd.decay_cd()
    tw = qd.decay_twin(cd)
    st = TwinState(ssh, u, h)
    for m in range(qd.DECAY_STEPS):
        tw.step_rk4(st, [[], []], tc.EIG_DT)
        if m == 0:
            assert np.all(np.abs(tw.sp - U0) <= (qd.counts(mesh)[1] + qd.DECAY_E0 + 2) * U * U0)
    qd.decay_check(st.u[1], u, mesh, cd, "twin")


# ---- header and symbols -------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_states_the_recipe():
    text = open(os.path.join(ROOT, "include", "moka_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\(", text), name
        assert name in L.EXPORTS, name
    flat = re.sub(r"\s+", " ", text.replace("\n *", " "))
    for line in ("acc = acc + (kc[e'] * x[kb,e']) * x[kb,e']",
                 "KE_c = acc * invArea[c]",
                 "sp[e] = sqrt(KE_c1 + KE_c2)",
                 "rq = r + Cd * sp[e]",
                 "q_e = dt * rq",
                 "d[n-1] = d[n-1] + q_e; R[n-1] = R[n-1] - q_e * x[n-1]",
                 "Out of scope: reverse mode of the flow through this drag, a Cd field per edge or cell"):
        assert line in flat, line
