"""Handles may be destroyed in any order (csrc/state.hpp: state_attach / state_detach).  A tape that outlives its state works with
the context it cached and touches nothing of the state: not its counters, not lazyOwner, not its stream.

The calls go through the C ABI itself (moka_hip.lib): the owners of moka_hip.api keep a state alive for as long as a tape of it
exists, i.e. they would reorder the very calls under test.  The mesh is the smallest one the tracer and the forced-adjoint tests
build (tracer_cases.TINY: the periodic 4 x 4 hexagons, 60 layers).

state first:  create, one recorded step, destroy the state, destroy the tape -- then a fresh state on the same mesh takes one RK4
              step and holds, bit for bit, what a state that never had a tape holds after that step.
tape first:   while the tape lives the state refuses what it refuses today; once it is gone moka_set_tracers, moka_set_nonlinear and
              a second moka_forced_tape_create are accepted again."""
import ctypes as C

import numpy as np
import pytest

import moka_hip as mk
import tracer_cases as tc
from moka_hip import lib as L

pytestmark = pytest.mark.gpu
MESH, K = "tiny-4-4", 60
KINDS = ["tape", "forced", "tracer"]
FIELDS = ((L.F_SSH, 1), (L.F_NORMAL_VELOCITY, K), (L.F_LAYER_THICKNESS, K))


@pytest.fixture(scope="module")
def model():
    backend = mk.MokaHIP(0)
    m = tc.Model(backend, MESH, K)          # the mesh handle (and a state of its own that no test here touches)
    yield m
    m.close()
    backend.close()


def new_state(model):
    lib, ctx = L.lib(), model.backend._h
    hS = C.c_void_p()
    L.check(lib.moka_state_create(ctx, model.M._h, C.byref(hS)), ctx)
    for (f, _), a in zip(FIELDS, (model.ssh, model.u, model.h)):
        L.check(lib.moka_state_upload(hS, f, 1, L.f64(np.ascontiguousarray(a, dtype=np.float64))), ctx)
    return hS


def step_and_read(model, hS):
    lib, ctx, mesh = L.lib(), model.backend._h, model.mesh
    L.check(lib.moka_step_rk4(hS, model.dt), ctx)
    out = []
    for (f, k), n in zip(FIELDS, (mesh.nCells, mesh.nEdges, mesh.nCells)):
        a = np.empty((n, k))
        L.check(lib.moka_state_download(hS, f, 1, L.f64(a)), ctx)
        out.append(a)
    return out


@pytest.fixture(scope="module")
def untaped(model):
    """One RK4 step of a state that never had a tape: computed once, compared against by every case."""
    hS = new_state(model)
    ref = step_and_read(model, hS)
    L.lib().moka_state_destroy(hS)
    for a in ref:
        a.setflags(write=False)
    return ref


def taped(model, hS, kind, step=True):
    """A tape of `kind` on hS, with one recorded step: (handle, its destroy function)."""
    lib, ctx = L.lib(), model.backend._h
    hT = C.c_void_p()
    if kind == "tracer":
        L.check(lib.moka_set_tracers(hS, 2), ctx)
        for j, phi in enumerate(tc.distinct_fields(model.mesh, K, 2)):
            L.check(lib.moka_tracer_upload(hS, j, 1, L.f64(phi)), ctx)
        create, record, destroy = lib.moka_tracer_tape_create, lib.moka_step_rk4_tracer_taped, lib.moka_tracer_tape_destroy
    elif kind == "forced":
        create, record, destroy = lib.moka_forced_tape_create, lib.moka_step_rk4_forced_taped, lib.moka_forced_tape_destroy
    else:
        create, record, destroy = lib.moka_tape_create, lib.moka_step_rk4_taped, lib.moka_tape_destroy
    L.check(create(hS, 2, C.byref(hT)), ctx)
    if step:
        L.check(record(hT, model.dt), ctx)
    return hT, destroy


@pytest.mark.parametrize("kind", KINDS)
def test_state_destroyed_before_its_tape(model, untaped, kind):
    """moka_tape: the recorded step left the state's pending tendencies in a slot of the tape (lazyOwner), which the tape must not
    look at any more.  moka_forced_tape: one recorded step is counted in the state's forcedSteps."""
    lib = L.lib()
    hS = new_state(model)
    hT, destroy = taped(model, hS, kind)
    lib.moka_state_destroy(hS)
    destroy(hT)
    fresh = new_state(model)
    try:
        for got, ref in zip(step_and_read(model, fresh), untaped):
            assert np.array_equal(got, ref)
    finally:
        lib.moka_state_destroy(fresh)


@pytest.mark.parametrize("kind", KINDS)
def test_tape_destroyed_first_gives_the_state_its_counters_back(model, kind):
    lib, ctx = L.lib(), model.backend._h
    hS = new_state(model)
    try:
        hT, destroy = taped(model, hS, kind)
        other = C.c_void_p()
        # while the tape lives: a tape pins the state's arrays (no new tracers); a dycore tape rules out the nonlinear terms and
        # a (second) forced tape.  The tracer tape stands beside neither of the latter two: its state has tracers, which a forced
        # tape refuses on their own account.
        assert lib.moka_set_tracers(hS, 1) == L.ERR_UNSUPPORTED
        if kind != "tracer":
            assert lib.moka_set_nonlinear(hS, 1) == L.ERR_UNSUPPORTED
            assert lib.moka_forced_tape_create(hS, 1, C.byref(other)) == L.ERR_UNSUPPORTED and not other.value
        destroy(hT)
        L.check(lib.moka_set_tracers(hS, 0), ctx)          # (the tracer case: back to a state a forced tape accepts)
        L.check(lib.moka_forced_tape_create(hS, 1, C.byref(other)), ctx)
        lib.moka_forced_tape_destroy(other)
        L.check(lib.moka_set_tracers(hS, 1), ctx)
        L.check(lib.moka_set_tracers(hS, 0), ctx)
        L.check(lib.moka_set_nonlinear(hS, 1), ctx)
    finally:
        lib.moka_state_destroy(hS)
