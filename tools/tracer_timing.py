#!/usr/bin/env python3
"""GPU box helper: ms per linear RK4 step with 0, 1 and 3 passive tracers (moka_set_tracers) in one process, the three settings
alternated round by round and each step timed between two moka_mark events (medians) -- first with the default kernel choice (the
tracer launch in its patch form), then with kernel variant 3 (generic dycore kernels, the tracer launch in its generic form).  The
tracer launch alone is the difference to the same run's tracer-free step, over the four launches of a step.  Config 4 (icosahedral
m = 320, 1 024 002 cells x 60 levels); --small: config 3 (m = 64).  Prints one JSON line and, with --out FILE, writes the summary
table there.

Contract bytes of the tracer launches of one step (what the algorithm has to move once): the stage's normalVelocity rows (4 nE), the
stage's and the next layerThickness rows (8 nC), the current level's for stages 2 / 3 (2 nC), and per tracer 16 cell streams (pphi
in x 4, phi_cur in x 2, Qn in x 3 / out x 4, pphi out x 3):  8 K (4 nE + 10 nC + 16 nT nC).

    python3 tools/tracer_timing.py [--small] [--rounds R] [--steps N] [--out profiles/tracer_summary.txt]"""
import argparse
import ctypes as C
import datetime as dt
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpas-ocean.jl_amd"))
import numpy as np                         # noqa: E402
import moka_hip as mk                      # noqa: E402
from moka_hip import lib as L              # noqa: E402
from moka_hip import meshgen as mg         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--small", action="store_true")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

m, K = (64 if args.small else 320), 60
mesh = mg.icosahedral_mesh(m)
ssh, u, h, rest, dts = mg.sphere_synthetic_state(mesh, K)
cfg = {"time_management": {"config_start_time": dt.datetime(1, 1, 1), "config_run_duration": dt.timedelta(hours=1)},
       "time_integration": {"config_dt": dt.timedelta(seconds=dts), "config_number_of_time_levels": 2}}
b = mk.MokaHIP(0)
lib = L.lib()
rng = np.random.default_rng(1)
phi = rng.uniform(0.5, 1.5, (mesh.nCells, K))
counts = (0, 1, 3)
result = {"cells": mesh.nCells, "edges": mesh.nEdges, "K": K, "rounds": args.rounds, "steps_per_round": args.steps, "forms": {}}
for variant, form in ((0, "patch"), (3, "generic")):
    b.set_kernel_variant(variant)
    Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, cfg, b, multilayer=True)
    sh = Prog._state._h
    steps = {n: [] for n in counts}
    path = 0
    for _ in range(args.rounds):
        for n in counts:
            tr = mk.set_tracers(Prog, [phi] * n)
            for _ in range(args.warmup):                                     # lazy allocations, LDS attributes, clocks
                L.check(lib.moka_step_rk4(sh, C.c_double(dts)), b._h)
            b.synchronize()
            b.marks_reset()
            b.mark()
            for _ in range(args.steps):
                L.check(lib.moka_step_rk4(sh, C.c_double(dts)), b._h)
                b.mark()
            b.synchronize()
            steps[n] += list(b.marks_read())
            if n:
                path = tr.path()
    mk.set_tracers(Prog, [])
    med = {n: statistics.median(v) for n, v in steps.items()}
    contract = {n: 8 * K * (4 * mesh.nEdges + 10 * mesh.nCells + 16 * n * mesh.nCells) for n in counts if n}
    result["forms"][form] = {
        "tracer_path": path, "ms_per_step_median": med, "ms_per_step_min": {n: min(v) for n, v in steps.items()},
        "increment_ms_per_step": {n: med[n] - med[0] for n in counts if n},
        "tracer_launch_ms": {n: (med[n] - med[0]) / 4 for n in counts if n},
        "contract_bytes_per_step": contract,
        "contract_TBps": {n: contract[n] / ((med[n] - med[0]) * 1e-3) / 1e12 for n in contract}}
    Prog._state.close(); Setup.mesh.close()
b.set_kernel_variant(0)
bw = b.bw_probe()
result["copy_GBs"] = bw.get("copy_GBs")
for f in result["forms"].values():
    f["contract_fraction_of_copy_rate"] = {n: f["contract_TBps"][n] * 1e3 / result["copy_GBs"] for n in f["contract_TBps"]}
print(json.dumps(result), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(f"Passive tracer transport beside the linear RK4 step -- {mesh.nCells} cells x {K} levels, fp64, one MI355X.\n"
                 f"tools/tracer_timing.py ({args.rounds} rounds x {args.steps} steps after {args.warmup} warm-up steps, 0 / 1 / 3 tracers "
                 "alternated round by round in one\nprocess; medians of moka_mark intervals).  The tracer-free step of the same run is "
                 "the code path without the feature.\nThe tracer launch alone = (step with n tracers - tracer-free step) / 4 launches.  "
                 f"Copy rate of the same run (moka_bw_probe): {result['copy_GBs']:.0f} GB/s.\n\n")
        for form, f in result["forms"].items():
            fh.write(f"{form} form (moka_state_tracer_path = {f['tracer_path']}; kernel variant {0 if form == 'patch' else 3})\n"
                     "   tracers   ms / RK4 step (median)   min      increment   per tracer launch   contract bytes / step   "
                     "TB/s     of copy rate\n")
            for n in counts:
                line = f"   {n:<9d} {f['ms_per_step_median'][n]:<24.3f} {f['ms_per_step_min'][n]:<8.3f}"
                if n:
                    line += (f" {f['increment_ms_per_step'][n]:<11.3f} {f['tracer_launch_ms'][n]:<19.3f} "
                             f"{f['contract_bytes_per_step'][n] / 1e9:<23.2f} {f['contract_TBps'][n]:<8.2f} "
                             f"{f['contract_fraction_of_copy_rate'][n]:.2f}")
                fh.write(line.rstrip() + "\n")
            fh.write("\n")
