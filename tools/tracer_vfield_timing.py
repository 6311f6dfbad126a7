#!/usr/bin/env python3
"""GPU box helper: what the forward vertical pass of one tracer costs with a scalar kappaV and with a diffusivity field
(moka_tracer_vertical_field_upload), on the bench's size, in one process.

Per round the legs alternate: vertical term off / a scalar / a field (random in [0, 2] x the scalar).  Each repetition is one RK4 step
between two moka_mark events; the pass is the difference of the medians of a leg and of the `off` leg.  The scalar pass moves
(1 + 2 nT) fields of K nC doubles, the field pass one more per tracer with a field; both are set against the copy rate of moka_bw_probe.
--no-field: the off and scalar legs only (a build without the entry point, for a comparison across commits).

    python3 tools/tracer_vfield_timing.py [--small] [--no-field] [--rounds R] [--steps N] [--label TEXT]"""
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
ap.add_argument("--no-field", action="store_true")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--label", default="")
args = ap.parse_args()

m, K = (64 if args.small else 320), 60
mesh = mg.icosahedral_mesh(m)
ssh, u, h, rest, dts = mg.sphere_synthetic_state(mesh, K)
cfg = {"time_management": {"config_start_time": dt.datetime(1, 1, 1), "config_run_duration": dt.timedelta(hours=1)},
       "time_integration": {"config_dt": dt.timedelta(seconds=dts), "config_number_of_time_levels": 2}}
b = mk.MokaHIP(0)
rng = np.random.default_rng(1)
phi = rng.uniform(0.5, 1.5, (mesh.nCells, K))
hm = float(np.mean(h))
kv = 10.0 * hm * hm / dts                  # s / hm^2 = 10
Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, cfg, b, multilayer=True)
med = statistics.median
tr = mk.set_tracers(Prog, [phi])
legs = ["off", "scalar"] + ([] if args.no_field else ["field"])
field = None if args.no_field else rng.uniform(0.0, 2.0, (mesh.nCells, K)) * kv
ms = {leg: [] for leg in legs}
paths = {}
for _ in range(args.rounds):
    for leg in legs:
        if not args.no_field:
            tr.set_vertical_field(0, field if leg == "field" else None)
        tr.set_vertical_diffusivity(kv if leg == "scalar" else None)
        for rep in range(args.warmup + args.steps):
            b.synchronize()
            b.marks_reset()
            b.mark()
            mk.run_steps(Prog, mk.RungeKutta4, dts, 1)
            b.mark()
            b.synchronize()
            if rep >= args.warmup:
                ms[leg].append(list(b.marks_read())[0])
        paths[leg] = tr.vmix_path()
        tr.set(0, phi, 0)                  # the same values in every leg
        tr.set(0, phi, 1)
mk.set_tracers(Prog, [])
bw = b.bw_probe()
nC = mesh.nCells
out = {"label": args.label, "cells": nC, "K": K, "timed_steps_per_leg": args.rounds * args.steps, "copy_GBs": bw.get("copy_GBs"), "vmix_path": paths,
       "step_ms": {leg: {"median": med(v), "min": min(v), "max": max(v)} for leg, v in ms.items()}}
for leg, fields in (("scalar", 3), ("field", 4)):
    if leg in ms:
        t = med(ms[leg]) - med(ms["off"])
        out[leg + "_pass"] = {"ms": t, "fields_moved": fields, "GBs": fields * K * nC * 8 / (t * 1e-3) / 1e9 if t > 0 else None}
print(json.dumps(out), flush=True)
Prog._state.close(); Setup.mesh.close()
