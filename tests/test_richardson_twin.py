"""The numpy twin of the Richardson-number closure (tests/richardson_twin.py) against its long-double restatement within the counted
bound, the branch census of every case the device file runs, and the consequences include/moka_hip.h states.  No GPU."""
import numpy as np
import pytest

import momentum_vmix_twin as mv
import richardson_twin as rt
import tracer_cases as tc
import tracer_vfield_twin as tf
from del4_twin import TwinState

# (mesh, K, mask) of every case of tests/test_gpu_richardson.py
DEVICE_CASES = [("planar", 60, None), ("planar", 8, None), ("planar", 3, None), ("planar", 2, None), ("tiny-4-4", 106, None), ("ico12f", 8, None),
                ("tiny-4-4", 60, None), ("sheared-7-5", 35, None), ("planar", 8, "partial"), ("planar", 8, "basin"), ("planar", 34, None)]


def get(meshname, K, mask=None, poison=None):
    if meshname.startswith("sheared"):
        assert tf.sheared_mesh(7, 5) == meshname
    cs = rt.case(meshname, K, mask, poison)
    _, u, h, _ = cs["state"]
    c1, c2 = mv.edge_cells(cs["mesh"])
    return cs, u, h, cs["fields"][rt.JB], c1, c2


@pytest.mark.parametrize("mask", [None, "partial"])
@pytest.mark.parametrize("meshname", ["planar", "ico16", "ico12f"])
def test_twin_against_long_double_within_the_counted_bound(meshname, mask):
    cs, u, h, b, c1, c2 = get(meshname, 8, mask)
    P = cs["params"]
    F, _ = rt.edge_field(u, h, b, cs["mlt"], c1, c2, P)
    G, _ = rt.cell_field(u, h, b, cs["mlt"], cs["mesh"], P)
    Fl, le = rt.edge_ld(u, h, b, cs["mlt"], c1, c2, P)
    Gl, lc = rt.cell_ld(u, h, b, cs["mlt"], cs["mesh"], P)
    eF = float((np.abs(F[:, :-1].astype(rt.LD) - Fl) / Fl)[le].max() / rt.U53)
    eG = float((np.abs(G[:, :-1].astype(rt.LD) - Gl) / Gl)[lc].max() / rt.U53)
    print(f"{meshname} mask={mask}: max relative error of F = {eF:.2f} x 2^-53 (bound {rt.C_F}), of G = {eG:.2f} x 2^-53 (bound {rt.c_g(cs['mesh'])})")
    assert le.any() and lc.any()
    assert eF <= rt.C_F and eG <= rt.c_g(cs["mesh"])
    assert eF > 0.0 and eG > 0.0                                   # (the restatement is not the twin again)
    assert np.all(F[:, :-1][~le] == 0.0) and np.all(F[:, -1] == 0.0) and np.all(G[:, :-1][~lc] == 0.0) and np.all(G[:, -1] == 0.0)


@pytest.mark.parametrize("meshname,K,mask", DEVICE_CASES)
def test_every_device_case_meets_every_branch(meshname, K, mask):
    """Each of Ri > 0, Ri == 0 (db == 0) and db < 0 holds at least 1 % of the active interfaces of F and of G."""
    cs, u, h, b, c1, c2 = get(meshname, K, mask)
    P = cs["params"]
    le, _, dbe, _ = rt.edge_parts(u, h, b, cs["mlt"], c1, c2)
    lc, _, dbc, _, _ = rt.cell_parts(u, h, b, cs["mlt"], cs["mesh"])
    for name, ri, db, live in (("F", rt.edge_field(u, h, b, cs["mlt"], c1, c2, P)[1][:, :-1], dbe, le),
                               ("G", rt.cell_field(u, h, b, cs["mlt"], cs["mesh"], P)[1][:, :-1], dbc, lc)):
        shares = rt.census(ri, db, live)
        print(f"{meshname} K={K} mask={mask} {name}: Ri > 0 {shares[0]:.3f}, Ri == 0 {shares[1]:.3f}, db < 0 {shares[2]:.3f} of {int(live.sum())}")
        assert min(shares) >= 0.01
        assert np.all((ri[live] > 0) == (db[live] > 0)) and np.all(ri[live & (db == 0)] == 0.0)     # the sign of db decides the branch
        assert abs(sum(shares) - 1.0) < 1e-12
    med = float(np.median(rt.edge_field(u, h, b, cs["mlt"], c1, c2, P)[1][:, :-1][le & (dbe > 0)]))
    assert 0.25 / float(P.alpha) < med < 4.0 / float(P.alpha)      # the stable interfaces sit where the closure bends


@pytest.mark.parametrize("mask", [None, "partial"])
def test_constant_buoyancy_is_the_scalar_step_bit_for_bit(mask):
    """The buoyancy is the unit tracer, the one field the transport leaves constant over every column, exactly: db == 0 behind every
    stage 4, F = nuB + nu0 and G = kB + (nuB + nu0) everywhere, and the steps are those of the existing scalar twins."""
    K, steps = 6, 2
    cs = rt.case("planar", K, mask)
    P = rt.Params(0)
    nuV, kV = float(P.nuB + P.nu0), float(P.kB + (P.nuB + P.nu0))
    res = []
    for closure in (True, False):
        tw = rt.richardson_twin("planar", K, mlt=cs["mlt"], nu=0.0 if closure else nuV, params=P if closure else None)
        tw.tw.kappa, tw.tw.kappa4, tw.tw.source = [0.0] * rt.NT, [0.0] * rt.NT, [None] * rt.NT
        tw.tw.kappaV = [] if closure else [kV] * rt.NT
        ssh, u, h, _ = cs["state"]
        st = TwinState(ssh, u, h)
        phis = [[a.copy() for a in cs["fields"]], [a.copy() for a in cs["fields"]]]
        for _ in range(steps):
            tw.step_rk4(st, phis, tc.dt_of("planar"))
        res.append((st.u[1].copy(), [p.copy() for p in phis[1]], tw.F.copy(), tw.G.copy()))
    (ua, pa, F, G), (ub, pb, _, _) = res
    le = np.arange(K)[None, :] < (cs["nn"] - 1)[:, None]
    lc = np.arange(K)[None, :] < (cs["nlev"] - 1)[:, None]
    assert np.all(F[le] == nuV) and np.all(G[lc] == kV) and np.all(F[~le] == 0.0) and np.all(G[~lc] == 0.0)
    assert np.array_equal(ua, ub)
    for a, b in zip(pa, pb):
        assert np.array_equal(a, b)
    assert np.all(pa[0][np.arange(K)[None, :] < cs["nlev"][:, None]] == 1.0)        # the unit tracer stays exactly 1.0
    scalar_free = rt.run("planar", K, (None,) * steps, mask)[-1]
    assert not np.array_equal(ua, scalar_free[2])                  # (the pass did something)


@pytest.mark.parametrize("meshname,K,mask", [("planar", 8, None), ("planar", 8, "partial"), ("ico12f", 8, None)])
def test_range(meshname, K, mask):
    cs, u, h, b, c1, c2 = get(meshname, K, mask)
    P = cs["params"]
    F, _ = rt.edge_field(u, h, b, cs["mlt"], c1, c2, P)
    G, _ = rt.cell_field(u, h, b, cs["mlt"], cs["mesh"], P)
    le = rt.edge_parts(u, h, b, cs["mlt"], c1, c2)[0]
    lc = rt.cell_parts(u, h, b, cs["mlt"], cs["mesh"])[0]
    assert np.all(F[:, :-1][le] >= P.nuB) and np.all(F[:, :-1][le] <= (P.nuB + P.nu0) + P.conv)
    assert np.all(G[:, :-1][lc] >= P.kB) and np.all(G[:, :-1][lc] <= (P.kB + (P.nuB + P.nu0)) + P.conv)
    assert (F[:, :-1][le] == (P.nuB + P.nu0) + P.conv).any() and (F[:, :-1][le] < P.nuB + 0.5 * P.nu0).any()


@pytest.mark.parametrize("mask", ["partial", "basin"])
def test_a_slot_too_shallow_is_omitted_and_a_twin_that_reads_it_is_rejected(mask):
    clean, u, h, b, c1, c2 = get("planar", 8, mask)
    cs, up, hp, bp, _, _ = get("planar", 8, mask, "strict")
    P = cs["params"]
    assert np.isnan(up).any() and (mask != "basin" or np.isnan(bp).any())     # (every cell of the partial mask keeps a full-depth edge)
    for got, ref in ((rt.edge_field(up, hp, bp, cs["mlt"], c1, c2, P), rt.edge_field(u, h, b, cs["mlt"], c1, c2, P)),
                     (rt.cell_field(up, hp, bp, cs["mlt"], cs["mesh"], P), rt.cell_field(u, h, b, cs["mlt"], cs["mesh"], P))):
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    wrong = rt.cell_field_wrong(up, hp, bp, cs["mlt"], cs["mesh"], P)
    assert np.isnan(wrong[1]).any()                                # it read u below an edge's floor: Ri is NaN there ...
    assert not np.array_equal(wrong[0], rt.cell_field(u, h, b, cs["mlt"], cs["mesh"], P)[0])      # ... and G the other branch's constant
    assert not np.array_equal(rt.cell_field_wrong(u, h, b, cs["mlt"], cs["mesh"], P)[0], rt.cell_field(u, h, b, cs["mlt"], cs["mesh"], P)[0])


def test_alpha_zero_and_nu0_zero():
    cs, u, h, b, c1, c2 = get("planar", 8, "partial")
    le, _, dbe, _ = rt.edge_parts(u, h, b, cs["mlt"], c1, c2)
    lc, _, dbc, _, _ = rt.cell_parts(u, h, b, cs["mlt"], cs["mesh"])
    P = rt.Params(rt.JB, alpha=0.0)
    F = rt.edge_field(u, h, b, cs["mlt"], c1, c2, P)[0][:, :-1]
    G = rt.cell_field(u, h, b, cs["mlt"], cs["mesh"], P)[0][:, :-1]
    assert np.all(F[le & (dbe >= 0)] == P.nuB + P.nu0) and np.all(G[lc & (dbc >= 0)] == P.kB + (P.nuB + P.nu0))
    assert np.all(F[le & (dbe < 0)] == (P.nuB + P.nu0) + P.conv)
    P = rt.Params(rt.JB, nu0=0.0)
    F = rt.edge_field(u, h, b, cs["mlt"], c1, c2, P)[0][:, :-1]
    assert (le & (dbe > 0)).any() and np.all(F[le & (dbe > 0)] == P.nuB)


@pytest.mark.parametrize("factor", [2.0, 4.0])
def test_a_larger_buoyancy_never_raises_the_coefficients_of_a_stable_interface(factor):
    cs, u, h, b, c1, c2 = get("planar", 8, "partial")
    P = cs["params"]
    le, _, dbe, _ = rt.edge_parts(u, h, b, cs["mlt"], c1, c2)
    lc, _, dbc, _, _ = rt.cell_parts(u, h, b, cs["mlt"], cs["mesh"])
    F0 = rt.edge_field(u, h, b, cs["mlt"], c1, c2, P)[0][:, :-1]
    F1 = rt.edge_field(u, h, factor * b, cs["mlt"], c1, c2, P)[0][:, :-1]
    G0 = rt.cell_field(u, h, b, cs["mlt"], cs["mesh"], P)[0][:, :-1]
    G1 = rt.cell_field(u, h, factor * b, cs["mlt"], cs["mesh"], P)[0][:, :-1]
    se, sc = le & (dbe > 0), lc & (dbc > 0)
    assert np.all(F1[se] <= F0[se]) and (F1[se] < F0[se]).any()
    assert np.all(G1[sc] <= G0[sc]) and (G1[sc] < G0[sc]).any()
    assert np.array_equal(F1[~se], F0[~se]) and np.array_equal(G1[~sc], G0[~sc])     # (a power of two scales db exactly: no branch moves)


def test_the_step_composes_the_existing_twins():
    """Closure off: the chain's own step, scalars and fields included; closure on with a mask: a tracer outside the set keeps its scalar."""
    K = 5
    cs = rt.case("planar", K)
    kv = [0.0, 0.0, 3.0]
    P = rt.Params(rt.JB, tracers=[0, 1])
    on = rt.run("planar", K, (P,), settings={"kappaV": kv}, tag="masked")[0]
    alone = rt.run("planar", K, (rt.Params(rt.JB),), settings={"kappaV": kv}, tag="masked")[0]
    off = rt.run("planar", K, (None,), settings={"kappaV": kv}, tag="masked")[0]
    assert np.array_equal(on[1][0], alone[1][0]) and np.array_equal(on[1][1], alone[1][1]) and np.array_equal(on[2], alone[2])
    assert np.array_equal(on[1][2], off[1][2]) and not np.array_equal(on[1][2], alone[1][2])
    assert np.all(off[5] == 0.0) and np.all(off[6] == 0.0) and off[7] is None
    assert not np.array_equal(on[2], off[2])
    assert cs["params"].key() == rt.Params(rt.JB).key()
