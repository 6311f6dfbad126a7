"""RK4 steps with New handed from stage 1 to stage 2 as one-byte codes (moka_set_tuning key 12; k_stage_rec2c modes 12 / 13) are the
steps without it, and the oracle's, bit for bit: three steps of every case with the key on, the same steps with the key off, and
step_rk4 of the CPU oracle.

Shapes: the icosahedral meshes m = 4 and m = 8 (12 pentagons each) and the periodic planar hex mesh, all of at most 512 patches, so
their launches take the 512-thread form; the icosahedral mesh m = 29 (8412 cells = 526 patches of 16) takes the 256-thread form.
K = 34 (17 of a group's 32 lanes active), 60 and 64 (all of them).  Two patches per workgroup forced on (key 8 with bit 16) and off.
Whether the hand-off ran is asked of the library (moka_state_rk_handoff_escapes fails after a step that did not use it), so that no case
passes by comparing the plain step with itself."""
import ctypes as C

import numpy as np
import pytest

import moka_hip as mk
import oracle as orc
import poison_cases as pc
from masks import basin
from moka_hip import lib as L
from moka_hip import meshgen as mg
from moka_hip import parallel as par

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
TUNE_PAIR, TUNE_RK_HANDOFF = 8, 12                   # csrc/kernels.hpp
PAIR_DEFAULT, PAIR_EVERY = 0b10000011, (1 << 16) | 0b1110001111
NSTEPS = 3
_MESH, _REF = {}, {}


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


def get_mesh(name):
    if name not in _MESH:
        _MESH[name] = {"ico4": lambda: mg.icosahedral_mesh(4), "ico8": lambda: mg.icosahedral_mesh(8),
                       "ico29": lambda: mg.icosahedral_mesh(29),
                       "planar": lambda: mg.planar_hex_mesh(20, 18, 1000.0, f0=1e-4)}[name]()
    return _MESH[name]


def dt_of(meshname, scenario):
    return 0.0 if scenario == "dt0" else 20.0 if meshname.startswith("ico") else 2.0


def case(meshname, K, scenario):
    """(mesh, maxLevelEdgeTop, (ssh, u, h, rest), dt, the oracle's levels after each of NSTEPS steps): once per case, never modified."""
    key = (meshname, K, scenario)
    if key in _REF:
        return _REF[key]
    mesh = get_mesh(meshname)
    rng = np.random.default_rng(1000 + 7 * K + len(meshname) + len(scenario))
    rest = np.full((mesh.nCells, K), 1000.0 / K) + rng.uniform(0, 0.1, (mesh.nCells, K))
    h = rest + rng.uniform(-1, 1, (mesh.nCells, K))
    u = rng.uniform(-1, 1, (mesh.nEdges, K))
    mlt = np.full(mesh.nEdges, K, dtype=np.int32)
    dt = dt_of(meshname, scenario)
    if scenario == "u0":
        u[:] = 0.0
    if scenario == "mask":               # a basin from land to full columns; NaN on every level of u no active element may read
        mlt = np.asarray(basin(mesh, K), dtype=np.int32)
        u = pc.put(u, pc.edge_poison(mesh, mlt, K, 1), "nan")
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=mlt if scenario == "mask" else K)
    if scenario == "cancel":
        # C = -b t(C) on a seeded third of the rows of both fields: New = C + b t of stage 1 cancels there to its last bits.  t depends
        # on C, so the rows are iterated to the fixed point (a contraction: b |dt/dC| is a sixth of the Courant number), then moved off
        # it by 1e-9 relative.  The oracle's tendencies are moka_tendencies bit for bit (test_gpu_parity.py).
        b = dt / 6.0
        se, sc = rng.random(mesh.nEdges) < 1 / 3, rng.random(mesh.nCells) < 1 / 3
        for it in range(40):
            tu, th, _ = om.tendencies_clean(u, h)
            scale = 1.0 if it < 39 else 1.0 + 1e-9 * rng.standard_normal((mesh.nEdges, K))
            u[se] = (-b * tu * scale)[se]
            scale = 1.0 if it < 39 else 1.0 + 1e-9 * rng.standard_normal((mesh.nCells, K))
            h[sc] = (-b * th * scale)[sc]
    ssh = h.sum(1) - rest.sum(1)
    st = orc.OracleState(om, ssh, u, h)
    levels = []
    for _ in range(NSTEPS):
        st.step_rk4(dt)
        levels.append({"u1": st.u[1].copy(), "h1": st.h[1].copy(), "ssh1": st.ssh[1].copy(), "u0": st.u[0].copy(), "h0": st.h[0].copy()})
    _REF[key] = (mesh, mlt, (ssh, u, h, rest), dt, levels)
    return _REF[key]


def device_mesh(backend, mesh, K, rest, mlt):
    hm = mk.HorzMesh(mesh)
    vm = mk.VerticalMesh(hm, nVertLevels=K, restingThickness=rest, multilayer=True)
    vm.maxLevelEdge.Top[:] = mlt
    return mk.Mesh(hm, vm, backend=backend)


def fields(Prog):
    return {"u1": Prog.normalVelocity[-1].get(), "h1": Prog.layerThickness[-1].get(), "ssh1": Prog.ssh[-1].get(),
            "u0": Prog.normalVelocity[0].get(), "h0": Prog.layerThickness[0].get()}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def escapes(Prog):
    """(return code, cells, edges) of moka_state_rk_handoff_escapes."""
    nc, ne = C.c_int64(-1), C.c_int64(-1)
    rc = L.lib().moka_state_rk_handoff_escapes(Prog._state._h, C.byref(nc), C.byref(ne))
    return rc, nc.value, ne.value


def expect_equal(on, off, ref, what):
    for name in ref:
        assert np.array_equal(bits(on[name]), bits(off[name])), (what, name, "hand-off on differs from off")
        assert pc.same(on[name], ref[name]), (what, name, "differs from the oracle", pc.differences(on[name], ref[name]))


CASES = ([(m, K, "random", pair) for m, K, pair in (("ico4", 34, False), ("ico8", 60, False), ("planar", 64, False), ("ico29", 34, False),
                                                     ("ico8", 64, True), ("planar", 34, True), ("ico29", 34, True))]
         + [("ico8", 60, "u0", False), ("planar", 34, "u0", True)]
         + [("ico8", 60, "cancel", False), ("planar", 64, "cancel", True), ("ico4", 34, "cancel", False)]
         + [("ico8", 60, "mask", False), ("planar", 34, "mask", True), ("ico4", 64, "mask", False)]
         + [("ico8", 60, "dt0", False), ("planar", 64, "dt0", True)])


@pytest.mark.parametrize("meshname,K,scenario,pair", CASES)
def test_steps_bitwise_on_off_oracle(backend, meshname, K, scenario, pair):
    mesh, mlt, (ssh, u, h, rest), dt, ref = case(meshname, K, scenario)
    M = device_mesh(backend, mesh, K, rest, mlt)
    info = M.info()
    assert (info["nPatches"] > 512) == (meshname == "ico29")          # the 256-thread form on that mesh only
    on, off = (mk.PrognosticVars(ssh, u, h, 2, M) for _ in range(2))
    try:
        for n in range(NSTEPS):
            with tuning((TUNE_PAIR, PAIR_EVERY if pair else PAIR_DEFAULT), (TUNE_RK_HANDOFF, 1)):
                L.check(L.lib().moka_step_rk4(on._state._h, dt), backend._h)
                rc, nc, ne = escapes(on)
            with tuning((TUNE_PAIR, PAIR_EVERY if pair else PAIR_DEFAULT), (TUNE_RK_HANDOFF, 0)):
                L.check(L.lib().moka_step_rk4(off._state._h, dt), backend._h)
                assert escapes(off)[0] == L.ERR_UNSUPPORTED
            assert rc == 0, "the step did not take the hand-off"
            print(f"{meshname} K={K} {scenario} pair={pair} step {n + 1}: escapes cells {nc} of {mesh.nCells * K}, edges {ne} of {mesh.nEdges * K}")
            if scenario == "cancel" and n == 0:       # the cancelling rows are those of the initial state
                assert nc > 0 and ne > 0
            if scenario in ("random", "u0", "dt0"):   # model-like values: the byte carries all but a few (the codec test's bound)
                assert nc <= 1e-3 * mesh.nCells * K and ne <= 1e-3 * mesh.nEdges * K
            expect_equal(fields(on), fields(off), ref[n], (meshname, K, scenario, pair, n))
    finally:
        on._state.close(); off._state.close(); M.close()


@pytest.mark.parametrize("meshname,K,scenario", [("ico8", 60, "random"), ("planar", 34, "mask")])
def test_graph_replay_against_eager_steps(backend, meshname, K, scenario):
    """moka_run steps eagerly once and replays the captured step: the code arrays exist before the capture, the replayed launches are
    those of the eager step."""
    mesh, mlt, (ssh, u, h, rest), dt, ref = case(meshname, K, scenario)
    M = device_mesh(backend, mesh, K, rest, mlt)
    run, eager = (mk.PrognosticVars(ssh, u, h, 2, M) for _ in range(2))
    try:
        with tuning((TUNE_RK_HANDOFF, 1)):
            mk.run_steps(run, mk.RungeKutta4, dt, NSTEPS)
            assert escapes(run)[0] == 0
        with tuning((TUNE_RK_HANDOFF, 0)):
            for _ in range(NSTEPS):
                L.check(L.lib().moka_step_rk4(eager._state._h, dt), backend._h)
        expect_equal(fields(run), fields(eager), ref[NSTEPS - 1], (meshname, K, scenario, "run"))
    finally:
        run._state.close(); eager._state.close(); M.close()


@pytest.mark.parametrize("meshname,K,scenario", [("ico8", 60, "random"), ("planar", 34, "cancel")])
def test_taped_steps_against_untaped(backend, meshname, K, scenario):
    """Steps recorded on the dycore's tape (stages write the provisional states into the tape's slots) and on the tracer tape
    (step_rk4 with its recording copies behind every stage) against untaped steps without the hand-off."""
    mesh, mlt, (ssh, u, h, rest), dt, ref = case(meshname, K, scenario)
    M = device_mesh(backend, mesh, K, rest, mlt)
    plain, taped, traced = (mk.PrognosticVars(ssh, u, h, 2, M) for _ in range(3))
    try:
        with tuning((TUNE_RK_HANDOFF, 0)):
            for _ in range(NSTEPS):
                L.check(L.lib().moka_step_rk4(plain._state._h, dt), backend._h)
        with tuning((TUNE_RK_HANDOFF, 1)):
            tape = mk.AdjointTape(taped, NSTEPS)
            for _ in range(NSTEPS):
                tape.step(dt, method=mk.RungeKutta4)
            assert escapes(taped)[0] == 0
            mk.set_tracers(traced, [np.random.default_rng(3).uniform(0.5, 1.5, (mesh.nCells, K))])
            ttape = mk.TracerAdjointTape(traced, NSTEPS)
            for _ in range(NSTEPS):
                ttape.step(dt)
            assert escapes(traced)[0] == 0 and ttape.steps() == NSTEPS
        expect_equal(fields(taped), fields(plain), ref[NSTEPS - 1], (meshname, K, scenario, "dycore tape"))
        expect_equal(fields(traced), fields(plain), ref[NSTEPS - 1], (meshname, K, scenario, "tracer tape"))
    finally:
        for p in (plain, taped, traced):
            p._state.close()
        M.close()


@pytest.mark.parametrize("direct", [True, False])
def test_two_rank_partition_against_the_whole_mesh(backend, direct):
    """Boundary and interior launches of two ranks (LocalCluster: both in this process) take the same kernels over their own rows."""
    meshname, K, scenario = "ico8", 60, "random"
    mesh, mlt, (ssh, u, h, rest), dt, ref = case(meshname, K, scenario)
    M = device_mesh(backend, mesh, K, rest, mlt)
    whole = mk.PrognosticVars(ssh, u, h, 2, M)
    with tuning((TUNE_RK_HANDOFF, 1)):
        cl = par.LocalCluster(mesh, ssh, u, h, rest, dt, 2, direct=direct)
        try:
            assert cl.direct == direct
            cl.exchange_state()
            for _ in range(NSTEPS):
                cl.step_rk4()
            gs, gu, gh = cl.gather_owned(mesh.nCells, mesh.nEdges, K)
            took = [escapes(m.Prog)[0] for m in cl.models]
        finally:
            cl.close()
    try:
        assert took == [0, 0], "a rank's steps did not take the hand-off"
        with tuning((TUNE_RK_HANDOFF, 0)):
            for _ in range(NSTEPS):
                L.check(L.lib().moka_step_rk4(whole._state._h, dt), backend._h)
        got = fields(whole)
        for name, part in (("u1", gu), ("h1", gh), ("ssh1", gs)):
            assert np.array_equal(bits(part), bits(got[name])), (name, "partitioned with the hand-off differs from the whole mesh without")
            assert np.array_equal(bits(part), bits(ref[NSTEPS - 1][name])), (name, "differs from the oracle")
    finally:
        whole._state.close(); M.close()
