"""The HIP reverse sweep (moka_tape_*, moka_adjoint_*, csrc/adjoint.hip) through the C ABI against the long-double tangent-linear
model (tests/trisk_tangent.py), with partial maxLevelEdgeTop (0 included) and zeroed edgesOnEdge slots, for every adjoint kernel
form: per element at the sharp entries of the pinned categories and along three directions within the tangent's bound (the checks
of test_trisk_tangent.py), and bit for bit against the oracle's adjoint, which test_trisk_tangent.py pins to the same bound.  Also
the forward kernels on meshes with zeroed edgesOnEdge slots (eoe == 0, horizontal_advection_and_coriolis.jl:67) against
trisk_reference within its bound and against the oracle bit for bit."""
import numpy as np
import pytest

import moka_hip as mk
import test_gpu_trisk_reference as gtr
import test_trisk_tangent as base
import trisk_reference as tr
from moka_hip import lib as L
from moka_hip import meshgen as mg

pytestmark = pytest.mark.gpu
_MESHES = {}


@pytest.fixture(scope="module")
def backend():
    b = mk.MokaHIP(0)
    yield b
    b.close()


def get_mesh(name, zeroed=False):
    """ico6: hexagon-width transposed lists (W = 10, ME = 6); ico6f: flipped edges (W = 12, ME = 7).  (mesh, zeroed slots)."""
    key = (name, zeroed)
    if key not in _MESHES:
        if zeroed:
            _MESHES[key] = base.zero_slots(get_mesh(name)[0])
        else:
            _MESHES[key] = ({"ico6": lambda: mg.icosahedral_mesh(6),
                             "ico6f": lambda: mg.icosahedral_mesh(6, flips=5, seed=2)}[name](), [])
    return _MESHES[key]


def lanes(K):
    lpc = 1
    while lpc < K and lpc < 64:
        lpc *= 2
    return lpc


def form(meshname, K, method):
    """The kernels launch_adj_edge / launch_adj_cell pick (adjoint.hip): 16-byte lanes for even K <= 64 (k_adj_edge3 when the
    transposed lists are 10 wide, else k_adj_edge2; the fused RK4 cell kernel k_adj_cell3 when ME = 6), else k_adj_edge/cell<LPC>."""
    lpc = lanes(K)
    if lpc == 64 and K <= 64 and K % 2 == 0:
        if meshname == "ico6":
            return "edge3+cell3" if method == "rk4" else "edge3+cell2"
        return "edge2+cell2"
    return f"edge+cell<{lpc}>"


# (mesh, K, mask, method, flags, nsteps): every LPC instance of the generic form (K = 1 ... 100), the 16-byte forms at even
# 34 <= K <= 64 on both meshes, each with full masks and with partial masks + zeroed slots; FE flags 0 - 3 and 7 at K = 1
CASES = [("ico6", 1, "eoe", "fe", 7, 3), ("ico6", 1, "full", "fe", 3, 3), ("ico6", 2, "eoe", "fe", 0, 3),
         ("ico6", 3, "eoe", "fe", 1, 3), ("ico6", 5, "full", "fe", 2, 3), ("ico6", 5, "eoe", "fe", 3, 3),
         ("ico6", 9, "eoe", "rk4", 0, 2), ("ico6", 17, "eoe", "fe", 1, 2), ("ico6", 33, "eoe", "fe", 3, 2),
         ("ico6", 35, "eoe", "rk4", 0, 2), ("ico6", 65, "full", "fe", 0, 2), ("ico6", 65, "eoe", "fe", 1, 2),
         ("ico6", 100, "eoe", "fe", 3, 2), ("ico6f", 5, "eoe", "rk4", 0, 2), ("ico6f", 3, "eoe", "fe", 3, 3),
         ("ico6", 34, "full", "fe", 3, 2), ("ico6", 34, "eoe", "fe", 1, 2), ("ico6", 34, "eoe", "rk4", 0, 2),
         ("ico6", 64, "full", "rk4", 0, 2), ("ico6", 64, "eoe", "fe", 0, 2), ("ico6", 40, "eoe", "rk4", 0, 2),
         ("ico6f", 34, "full", "rk4", 0, 2), ("ico6f", 34, "eoe", "fe", 1, 2), ("ico6f", 40, "eoe", "rk4", 0, 2),
         ("ico6f", 64, "eoe", "fe", 3, 2)]


def case_id(p):
    meshname, K, mask, method, flags, nsteps = p
    return f"{form(meshname, K, method)}-{meshname}-K{K}-{mask}-{method}{flags if method == 'fe' else ''}"


def gpu_gradient(backend, c, method, flags, nsteps, rk13=False):
    """The tape's gradient (and the state after the steps) for the case's state; sets c.state["hE"] to the layerThicknessEdge
    the device holds before the first step (hEdge_0 of a stale-hEdge run)."""
    hm = mk.HorzMesh(c.mesh)
    vm = mk.VerticalMesh(hm, nVertLevels=c.K, restingThickness=c.rest2)
    vm.maxLevelEdge.Top[:] = c.mlt
    M = mk.Mesh(hm, vm, backend=backend)
    Prog = mk.PrognosticVars(c.state["ssh"], c.state["u"], c.state["h"], 2, M)
    Diag, Tend = mk.DiagnosticVars(None, M, Prog._state), mk.TendencyVars(None, M, Prog._state)
    try:
        if rk13:
            L.check(L.lib().moka_set_tuning(7, 1))
        c.state["hE"] = Diag.layerThicknessEdge.get()
        tape = mk.AdjointTape(Prog, nsteps)
        for _ in range(nsteps):
            if method == "rk4":
                tape.step(c.dt, method=mk.RungeKutta4)
            else:
                tape.step(c.dt, flags)
        after = {"ssh": Prog.ssh[-1].get(), "u": Prog.normalVelocity[-1].get(), "h": Prog.layerThickness[-1].get()}
        g = tape.gradient()
        tape.close()
    finally:
        if rk13:
            L.check(L.lib().moka_set_tuning(7, 0))
        Prog._state.close(); M.close()
    return {"ssh": g["ssh"], "u": g["normalVelocity"], "h": g["layerThickness"], "hE": g["layerThicknessEdge"]}, after


def check_case(backend, meshname, K, mask, method, flags, nsteps, rk13=False):
    c = base.make_case(*get_mesh(meshname, mask == "eoe"), K, mask, 60 + K)
    grad, after = gpu_gradient(backend, c, method, flags, nsteps, rk13)
    what = f"GPU {case_id((meshname, K, mask, method, flags, nsteps))}"
    if method == "rk4":
        assert not grad["ssh"].any() and not grad["hE"].any()
        adj = base.oracle_rk4(c, nsteps)
        o = dict(zip(("u", "h"), adj.gradient_sum_sq_ssh()))
        base.check(c, {"u": grad["u"], "h": grad["h"]}, "rk4", 0, nsteps, what)
    else:
        adj = base.oracle_fe(c, flags, nsteps)
        o = base.grad_dict(adj.gradient_sum_sq_ssh(), "fe")
        base.check(c, grad, "fe", flags, nsteps, what)
    # the taped steps are the ordinary steps, and the sweep is the oracle's sum for sum (rk13: the 13-stream forward form rounds
    # differently from the oracle's RK4; its gradient is held to the tangent's bound only)
    if not rk13:
        for f in ("ssh", "u", "h"):
            assert np.array_equal(after[f], {"ssh": adj.st.ssh[1], "u": adj.st.u[1], "h": adj.st.h[1]}[f]), (what, f)
        for f, v in o.items():
            assert np.array_equal(grad[f], v), (what, f)


@pytest.mark.parametrize("p", CASES, ids=case_id)
def test_adjoint_kernel_forms_within_the_tangent_bound(backend, p):
    check_case(backend, *p)


def test_rk4_adjoint_with_the_13_stream_form(backend):
    """moka_set_tuning(7, 1): the forward RK4 steps take the 13-stream form; the fused reverse sweep stays within the bound."""
    check_case(backend, "ico6", 34, "eoe", "rk4", 0, 2, rk13=True)


# ---- the forward kernels on meshes with zeroed edgesOnEdge slots ------------------------------------------------------------------
@pytest.mark.parametrize("meshname,K", [("ico6", 1), ("ico6", 4), ("ico6", 34), ("ico6", 60), ("ico6", 80), ("ico6f", 34)])
def test_forward_kernels_with_zeroed_slots(backend, meshname, K):
    """The linear tendencies in every kernel variant (k_stage_rec2c and variants 3 / 4), fp32 storage, and the nonlinear forms
    (k_stage_nl5's patch form at even 34 <= K <= 64) on a mesh with zeroed slots and partial masks, within trisk_reference's
    bound; the linear ones also bit for bit against the oracle.  (trisk_reference's identity checks assume mirrored slots: not
    applied here.)"""
    import oracle as orc
    mesh, _ = get_mesh(meshname, True)
    ssh, u, h, rest = gtr.random_state(mesh, K, 70 + K)
    mlt = gtr.edge_mask(mesh, K, "partial")
    rs = rest.sum(1)
    t = tr.terms(mesh, u, h, rs, mlt, nonlinear=False)
    bU, bH, bS = gtr.Bound(*t["U"], tr.C_U), gtr.Bound(*t["H"], tr.C_H), gtr.Bound(*t["ssh"], tr.C_SSH)
    otu, oth, _ = orc.OracleMesh(mesh, K, resting_thickness_sum=rs, max_level_edge_top=mlt).tendencies_clean(u, h)
    variants = [0] + [v for v in (11, 3, 4) if L.lib().moka_kernel_variant_available(v)]
    M, Prog, Diag, Tend = gtr.device_state(backend, mesh, K, ssh, u, h, rest, mlt)
    try:
        for v in variants:
            backend.set_kernel_variant(v)
            Tend.tendNormalVelocity.set(np.full((mesh.nEdges, K), np.nan))
            mk.computeTendency(M, Diag, Prog, Tend)
            tu, th = Tend.tendNormalVelocity.get(), Tend.tendLayerThickness.get()
            bU.check(tu, f"variant {v}: tendU"); bH.check(th, f"variant {v}: tendH"); bS.check(Prog.ssh[-1].get(), f"variant {v}: ssh")
            assert np.array_equal(tu, otu) and np.array_equal(th, oth), f"variant {v}"
        backend.set_kernel_variant(0)
        if K % 2 == 0 and 34 <= K <= 64 or K <= 4:
            nl = tr.terms(mesh, u, h, rs, mlt, nonlinear=True, mixing=False)
            bN = gtr.Bound(*tr.combine(nl), tr.C_U)
            for variant, shape in gtr.FORMS:
                gtr.set_form(backend, variant, shape)
                mk.set_nonlinear(Prog, True)
                Tend.tendNormalVelocity.set(np.full((mesh.nEdges, K), np.nan))
                mk.computeTendency(M, Diag, Prog, Tend)
                bN.check(Tend.tendNormalVelocity.get(), f"nonlinear form {variant}/{shape}: tendU")
            mk.set_nonlinear(Prog, False)
    finally:
        gtr.reset_forms(backend)
        Prog._state.close(); M.close()
    if K in (4, 80):                                  # fp32 storage (nVertLevels % 4 == 0)
        M, Prog, Diag, Tend = gtr.device_state(backend, mesh, K, ssh, u, h, rest, mlt, state_bytes=4)
        try:
            u32, h32 = Prog.normalVelocity[-1].get(), Prog.layerThickness[-1].get()
            mk.computeTendency(M, Diag, Prog, Tend)
            tu, th, gssh = Tend.tendNormalVelocity.get(), Tend.tendLayerThickness.get(), Prog.ssh[-1].get()
            t = tr.terms(mesh, u32, h32, rs, mlt, nonlinear=False)
            assert tr.within(th, *t["H"], tr.C_H, f32=True).all()
            U, MU = tr.terms(mesh, u32, h32, rs, mlt, nonlinear=False, ssh=gssh)["U"]
            assert tr.within(tu, U, MU, tr.C_U, f32=True).all()
        finally:
            Prog._state.close(); M.close()
