#!/usr/bin/env python3
"""GPU box helper: ms per nonlinear RK4 step with momentum mixing off, Del2, Del4 and both (moka_set_viscosity_del4), in one
process, the four settings alternated round by round and each step timed between two moka_mark events (medians).  Config 4
(icosahedral m = 320, 1 024 002 cells x 60 levels); --small: config 3 (m = 64).  Prints one JSON line: ms per step, per-stage
means (moka_stage_timing), and the contract bytes of the fused Del4 launch (k_d4_patch: divc + zv read, div4 + curl4 written).

    python3 tools/del4_timing.py [--small] [--rounds R] [--steps N]"""
import argparse
import ctypes as C
import datetime as dt
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpas-ocean.jl_amd"))
import moka_hip as mk                      # noqa: E402
from moka_hip import lib as L              # noqa: E402
from moka_hip import meshgen as mg         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--small", action="store_true")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
args = ap.parse_args()

m, K = (64 if args.small else 320), 60
mesh = mg.icosahedral_mesh(m)
ssh, u, h, rest, dts = mg.sphere_synthetic_state(mesh, K)
cfg = {"time_management": {"config_start_time": dt.datetime(1, 1, 1), "config_run_duration": dt.timedelta(hours=1)},
       "time_integration": {"config_dt": dt.timedelta(seconds=dts), "config_number_of_time_levels": 2}}
b = mk.MokaHIP(0)
Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, cfg, b, multilayer=True)
lib, sh = L.lib(), Prog._state._h
dcmin = float(mesh.dcEdge.min())
v2, v4 = 0.01 * dcmin ** 2 / dts, 0.002 * dcmin ** 4 / dts
settings = {"off": (0.0, 0.0), "del2": (v2, 0.0), "del4": (0.0, v4), "del2+del4": (v2, v4)}
steps = {k: [] for k in settings}
stages = {k: [] for k in settings}
paths = {}
for _ in range(args.rounds):
    for name, (a2, a4) in settings.items():
        mk.set_nonlinear(Prog, True, visc_del2=a2, visc_del4=a4)
        L.check(lib.moka_step_rk4(sh, C.c_double(dts)), b._h)             # warm: lazy allocations, LDS attributes
        b.synchronize()
        L.check(lib.moka_stage_timing(b._h, 1), b._h)
        b.marks_reset()
        b.mark()
        for _ in range(args.steps):
            L.check(lib.moka_step_rk4(sh, C.c_double(dts)), b._h)
            b.mark()
        b.synchronize()
        steps[name] += list(b.marks_read())
        ms, n = (C.c_double * 4)(), C.c_int64()
        L.check(lib.moka_stage_timing_read(b._h, ms, C.byref(n)), b._h)
        L.check(lib.moka_stage_timing(b._h, 0), b._h)
        stages[name].append(list(ms))
        paths[name] = lib.moka_state_del4_path(sh)
med = {k: statistics.median(v) for k, v in steps.items()}
stage_med = {k: [statistics.median(s[i] for s in v) for i in range(4)] for k, v in stages.items()}
contract = 2 * 8 * K * (mesh.nCells + mesh.nVertices)
print(json.dumps({"cells": mesh.nCells, "K": K, "rounds": args.rounds, "steps_per_round": args.steps,
                  "ms_per_step_median": med, "ms_per_step_min": {k: min(v) for k, v in steps.items()},
                  "ms_per_stage_median": stage_med, "del4_increment_ms": med["del4"] - med["off"],
                  "del4_path": paths, "k_d4_patch_contract_bytes": contract,
                  "k_d4_patch_ms_at_8TBps": contract / 8e12 * 1e3}), flush=True)
