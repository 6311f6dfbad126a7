#!/usr/bin/env python3
"""GPU box helper: what the gradient with respect to the vertical diffusivity (moka_tracer_adjoint_want_vertical_gradient) costs in the
sweep, against the same tape without a flag, in one process.

Per round and tracer count (1, 4) the legs alternate: (a) no tracer flagged, (b) every tracer flagged; kappaV is on for every tracer in
both.  Each repetition records one RK4 step on a tracer tape and sweeps it (zero seeds: the kernels' work does not depend on the
values), with moka_mark around the sweep.  Reported: the median of each leg over all repetitions, the median of every round (their
spread is the yardstick two builds are compared by), the gradient = (b) - (a), and its bytes -- one more field read and one
read-modify-write of D per flagged tracer, 3 nT K nC 8 -- at the copy rate of moka_bw_probe.

--plain: leg (a) only, for a library that has no flag (MOKA_HIP_LIB=<the build of the commit before> python3 tools/... --plain).

    python3 tools/tracer_vgrad_timing.py [--small] [--plain] [--rounds R] [--steps N] [--out FILE]"""
import argparse
import datetime as dt
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpas-ocean.jl_amd"))
sys.path.insert(0, ROOT)
import numpy as np                         # noqa: E402
import moka_hip as mk                      # noqa: E402
from moka_hip import meshgen as mg         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--small", action="store_true")
ap.add_argument("--plain", action="store_true")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()

m, K = (64 if args.small else 320), 60
mesh = mg.icosahedral_mesh(m)
ssh, u, h, rest, dts = mg.sphere_synthetic_state(mesh, K)
cfg = {"time_management": {"config_start_time": dt.datetime(1, 1, 1), "config_run_duration": dt.timedelta(hours=1)},
       "time_integration": {"config_dt": dt.timedelta(seconds=dts), "config_number_of_time_levels": 2}}
b = mk.MokaHIP(0)
phi = np.random.default_rng(1).uniform(0.5, 1.5, (mesh.nCells, K))
hm = float(np.mean(h))
kv = 10.0 * hm * hm / dts                  # s / hm^2 = 10
Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, cfg, b, multilayer=True)
med = statistics.median

counts = (1, 4)
legs = ("a",) if args.plain else ("a", "b")
sweep = {(n, leg): [[] for _ in range(args.rounds)] for n in counts for leg in legs}
paths = {}
for rnd in range(args.rounds):
    for n in counts:
        tr = mk.set_tracers(Prog, [phi] * n, vertical=kv)
        for leg in legs:
            tape = mk.TracerAdjointTape(Prog, 1)
            if leg == "b":
                for j in range(n):
                    tape.want_vertical_gradient(j)
            for rep in range(args.warmup + args.steps):
                tape.step(dts)
                for j in range(n):
                    tape.seed(j, None)
                b.synchronize()
                b.marks_reset()
                b.mark()
                tape.sweep()
                b.mark()
                b.synchronize()
                if rep >= args.warmup:
                    sweep[(n, leg)][rnd].append(list(b.marks_read())[0])
            paths[leg] = tape.vmix_path()
            tape.close()
mk.set_tracers(Prog, [])
bw = b.bw_probe()
nC = mesh.nCells
rows = []
for n in counts:
    row = {"tracers": n}
    for leg in legs:
        per_round = [med(r) for r in sweep[(n, leg)]]
        row[f"sweep_{leg}_ms"] = med([x for r in sweep[(n, leg)] for x in r])
        row[f"sweep_{leg}_round_medians_ms"] = per_round
        row[f"sweep_{leg}_round_spread_ms"] = max(per_round) - min(per_round)
    if not args.plain:
        row["gradient_ms"] = row["sweep_b_ms"] - row["sweep_a_ms"]
        row["bytes_model_ms"] = 3 * n * K * nC * 8 / (bw.get("copy_GBs") * 1e9) * 1e3
    rows.append(row)
result = {"library": os.environ.get("MOKA_HIP_LIB") or "libmoka_hip.so", "cells": nC, "K": K, "rounds": args.rounds, "steps_per_round": args.steps,
          "copy_GBs": bw.get("copy_GBs"), "vmix_path_of_the_sweep": paths, "rows": rows}
print(json.dumps(result), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")
Prog._state.close(); Setup.mesh.close()
