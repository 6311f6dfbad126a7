"""The references of tests/test_gpu_poison.py, with and without poison, on the CPU: the check that the device file cannot pass
vacuously.  For every case that file runs:
  - the basin mask has land (top 0) and full columns (top K), and the poison set holds at least 10 % of the poisoned field;
  - under poison (NaN, and -inf where the device file uses it) the reference is finite on 100 % of the active set A and has there the
    bits of the unpoisoned reference (poison_cases.closed);
  - for the fields compared only where the reference is finite (dJ/dlayerThickness, dJ/dlayerThicknessEdge) the finite share is at
    least the share of A.
Prints the shares per case (run with -s)."""
import numpy as np
import pytest

import poison_cases as pc
import tracer_cases as tc

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")

POISONS = ["nan", "-inf"]


def sets(meshname, K, mode="linear"):
    mesh, mlt = tc.get_mesh(meshname), pc.mask_of(meshname, K)
    assert (mlt == 0).any() and (mlt == K).any() and mlt.min() >= 0 and mlt.max() <= K
    pe = pc.edge_poison(mesh, mlt, K, pc.RINGS[mode])
    assert pe.mean() >= 0.10
    # the poison lies outside the active set, and so does every level an active element of the mode's stencil reads
    assert not (pe & pc.active(mesh, mlt, K, "edge")).any()
    return mesh, mlt, float(pe.mean())


def check(clean, poisoned, table, mesh, mlt, K, label):
    shares = {}
    for name, where in table.items():
        shares[name] = pc.closed(clean[name], poisoned[name], pc.active(mesh, mlt, K, where))
    print(f"{label}: finite share " + ", ".join(f"{n} {s:.3f}" for n, s in shares.items()))
    return shares


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("meshname,K", pc.SHAPES)
def test_linear_rk4_and_tendency(meshname, K, poison):
    mesh, mlt, share = sets(meshname, K)
    print(f"{meshname} K = {K} linear R = 1: poisoned share of u = {share:.3f}")
    for form in ("ref", "s13"):
        clean, pois = pc.rk4(meshname, K, "linear", None, pc.RK4_STEPS, form), pc.rk4(meshname, K, "linear", poison, pc.RK4_STEPS, form)
        for a, b, n in zip(clean, pois, pc.RK4_STEPS):
            sh = check(a, b, pc.RK4_ACTIVE, mesh, mlt, K, f"  {form} after {n} steps")
            assert sh["h1"] == 1.0 and sh["ssh1"] == 1.0
            if poison == "nan":            # the NaN set of the new u is the poison set exactly
                assert np.array_equal(np.isnan(b["u1"]), pc.edge_poison(mesh, mlt, K, 1))
    check(pc.tendency(meshname, K, "linear", None), pc.tendency(meshname, K, "linear", poison), pc.TEND_ACTIVE, mesh, mlt, K, "  tendency")


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("mode", ["nonlinear", "nonlinear+del2", "del2+del4"])
@pytest.mark.parametrize("meshname,K", pc.NONLINEAR_SHAPES)
def test_nonlinear_and_del4(meshname, K, mode, poison):
    mesh, mlt, share = sets(meshname, K, mode)
    print(f"{meshname} K = {K} {mode} R = {pc.RINGS[mode]}: poisoned share of u = {share:.3f}")
    clean, pois = pc.rk4(meshname, K, mode, None, pc.NL_STEPS), pc.rk4(meshname, K, mode, poison, pc.NL_STEPS)
    sh = check(clean[0], pois[0], pc.RK4_ACTIVE, mesh, mlt, K, f"  after {pc.NL_STEPS[0]} steps")
    assert sh["h1"] == 1.0 and sh["ssh1"] == 1.0
    check(pc.tendency(meshname, K, mode, None), pc.tendency(meshname, K, mode, poison), pc.TEND_ACTIVE, mesh, mlt, K, "  tendency")


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("meshname,K", pc.FE_SHAPES)
def test_forward_euler(meshname, K, flags, poison):
    mesh, mlt, _ = sets(meshname, K)
    clean, pois = pc.forward_euler(meshname, K, flags, None, pc.FE_STEPS), pc.forward_euler(meshname, K, flags, poison, pc.FE_STEPS)
    for n in (0, pc.FE_STEPS - 1):
        sh = check(clean[n], pois[n], pc.FE_ACTIVE, mesh, mlt, K, f"{meshname} K = {K} flags {flags} step {n + 1}")
        assert sh["h1"] == 1.0 and sh["ssh1"] == 1.0


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("meshname,K", pc.FP32_SHAPES)
def test_fp32_storage(meshname, K, poison):
    """The storage-emulating oracle (oracle_step_rk4_mixed, oracle_step_fe_mixed): rounding to fp32 keeps NaN, the infinities and every
    finite value's finiteness, so the sets are those of the fp64 oracle."""
    mesh, mlt, share = sets(meshname, K)
    print(f"{meshname} K = {K} fp32 storage: poisoned share of u = {share:.3f}")
    clean, pois = pc.rk4(meshname, K, "linear", None, pc.RK4_STEPS, "mixed"), pc.rk4(meshname, K, "linear", poison, pc.RK4_STEPS, "mixed")
    for a, b, n in zip(clean, pois, pc.RK4_STEPS):
        check(a, b, pc.RK4_ACTIVE, mesh, mlt, K, f"  RK4 after {n} steps")
    check(pc.tendency(meshname, K, "linear", None, True), pc.tendency(meshname, K, "linear", poison, True), pc.TEND_ACTIVE, mesh, mlt, K,
          "  tendency")
    for flags in (0, 3):
        clean = pc.forward_euler(meshname, K, flags, None, pc.FE_STEPS, True)
        pois = pc.forward_euler(meshname, K, flags, poison, pc.FE_STEPS, True)
        check(clean[-1], pois[-1], pc.FE_ACTIVE, mesh, mlt, K, f"  FE flags {flags} after {pc.FE_STEPS} steps")


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("meshname,K,nT,diff,bih,srcs,wants", pc.TRACER_CASES)
def test_tracers_forward_and_reverse(meshname, K, nT, diff, bih, srcs, wants, poison):
    mesh, mlt, share = sets(meshname, K)
    clean, pois = pc.tracers(meshname, K, nT, diff, bih, srcs, wants, None), pc.tracers(meshname, K, nT, diff, bih, srcs, wants, poison)
    A = pc.active(mesh, mlt, K, "cell")
    cellp = pc.cell_poison(mesh, mlt, K)
    assert cellp.mean() >= 0.10 and not (cellp & A).any()
    fin = []
    for a, b in zip(clean["forward"], pois["forward"]):
        for lev in (0, 1):
            for x, y in zip(a[lev], b[lev]):
                fin.append(pc.closed(x, y, A))
                if poison == "nan":
                    assert np.array_equal(np.isnan(y), cellp)
        pc.closed(a[2], b[2], pc.active(mesh, mlt, K, "edge"))
        assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])               # h and ssh unchanged
    for x, y in zip(clean["grad"], pois["grad"]):
        fin.append(pc.closed(x, y, A))
    for j in wants:
        fin.append(pc.closed(clean["G"][j], pois["G"][j], A))
    print(f"{meshname} K = {K} nT = {nT} diff {diff} bih {bih} srcs {srcs}: poisoned share of u {share:.3f}, of phi {cellp.mean():.3f}; "
          f"finite share of the results {min(fin):.3f} to {max(fin):.3f}")


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("meshname,K,nT", pc.KGRAD_CASES)
def test_kgrad(meshname, K, nT, poison):
    """The densities' column sums read every level of a column, so only u is poisoned: every tracer, adjoint, density and scalar keeps
    the bits of the unpoisoned run."""
    mesh, mlt, share = sets(meshname, K)
    clean = pc.tracers(meshname, K, nT, True, True, (), (), None, kgrad=pc.KGRAD_FLAGS)
    pois = pc.tracers(meshname, K, nT, True, True, (), (), poison, kgrad=pc.KGRAD_FLAGS)
    for x, y in zip(clean["grad"] + clean["forward"][-1][1], pois["grad"] + pois["forward"][-1][1]):
        assert pc.closed(x, y, None) == 1.0
    for j, bits in pc.KGRAD_FLAGS:
        for b in (0, 1):
            if bits & (b + 1):
                assert pc.closed(clean["W"][j][b], pois["W"][j][b], None) == 1.0 and clean["W"][j][b].any()
    print(f"{meshname} K = {K} kgrad: poisoned share of u {share:.3f}; tracers, adjoints and densities finite and unchanged")


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("meshname,K,method,flags,nsteps", pc.ADJOINT_CASES)
def test_dycore_adjoint(meshname, K, method, flags, nsteps, poison):
    """dJ/du is finite everywhere and keeps its bits; dJ/dh and dJ/dhEdge are NaN where the oracle itself multiplies a poisoned u by a
    zero adjoint, so they are compared where finite -- and finite on at least the share of A."""
    mesh, mlt, share = sets(meshname, K)
    clean, pois = pc.adjoint(meshname, K, method, flags, None, nsteps), pc.adjoint(meshname, K, method, flags, poison, nsteps)
    assert pc.closed(clean["normalVelocity"], pois["normalVelocity"], None) == 1.0
    assert pc.closed(clean["ssh"], pois["ssh"], None) == 1.0 and pc.closed(clean["ssh1"], pois["ssh1"], None) == 1.0
    out = []
    for name, where in (("layerThickness", "cell"), ("layerThicknessEdge", "edge")):
        A = pc.active(mesh, mlt, K, where)
        fin = pc.closed(clean[name], pois[name], A)
        assert pc.same_where_finite(clean[name], pois[name])
        assert fin >= A.mean()
        out.append(f"{name} finite {fin:.3f} (A {A.mean():.3f})")
    print(f"{meshname} K = {K} {method} flags {flags}: poisoned share of u {share:.3f}; " + ", ".join(out))


def test_comparisons():
    """`same` tells NaN from numbers, +inf from -inf and +0.0 from -0.0, and takes any NaN payload for NaN; `same_where_finite` looks
    only where the reference is finite."""
    a = np.array([1.0, np.nan, np.inf, -np.inf, 0.0, -0.0])
    quiet = np.array([0x7ff8000000000001], dtype=np.uint64).view(np.float64)[0]
    b = a.copy(); b[1] = quiet
    assert pc.same(a, a.copy()) and pc.same(a, b) and pc.differences(a, b) == (0, 0)
    for i, v in ((0, np.nan), (1, 1.0), (2, -np.inf), (3, np.inf), (4, -0.0), (5, 0.0), (0, np.nextafter(1.0, 2.0))):
        c = a.copy(); c[i] = v
        assert not pc.same(c, a) and not pc.same(a, c), (i, v)
    assert not pc.same(a.astype(np.float32), a) and not pc.same(a[:5], a)
    assert pc.same(a.astype(np.float32), a.astype(np.float32))
    c = a.copy(); c[1:4] = 7.0
    assert pc.same_where_finite(c, a) and not pc.same_where_finite(a, c)
    c[5] = 0.0
    assert not pc.same_where_finite(c, a)


def test_neighbourhood_by_brute_force():
    """N(e) and top_R on the heptagon mesh against a set-based restatement from the connectivity tables."""
    mesh = tc.get_mesh("ico12f")
    K = 5
    mlt = pc.mask_of("ico12f", K)
    N = [{e} for e in range(mesh.nEdges)]
    for c in range(mesh.nCells):
        es = [int(e) - 1 for e in mesh.edgesOnCell[c, :mesh.nEdgesOnCell[c]]]
        for e in es:
            N[e].update(es)
    for v in range(mesh.nVertices):
        es = [int(e) - 1 for e in mesh.edgesOnVertex[v, :mesh.vertexDegree] if e > 0]
        for e in es:
            N[e].update(es)
    for e in range(mesh.nEdges):
        for o in mesh.edgesOnEdge[e, :mesh.nEdgesOnEdge[e]]:
            if o > 0:
                N[e].add(int(o) - 1); N[int(o) - 1].add(e)
    t = [int(x) for x in mlt]
    for R in (1, 2, 3):
        t = [max(t[o] for o in N[e]) for e in range(mesh.nEdges)]
        assert np.array_equal(pc.top(mesh, mlt, R), np.array(t)), R
