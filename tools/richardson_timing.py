#!/usr/bin/env python3
"""GPU box helper: what the Richardson-number closure (moka_set_richardson_mixing) costs per RK4 step, against the same step with an
uploaded viscosity field and uploaded diffusivity fields in its place, and against the step with both vertical passes off, in one
process.  Three tracers: the unit tracer, a buoyancy (a stable profile with noise, copies and inversions, scaled to the state's own
shear so that the median Ri of an ordinary interface is near 1 / alpha) and a random field.

Per round the legs alternate: "off" (no vertical pass), "fields" (moka_vertical_viscosity_field_upload and one
moka_tracer_vertical_field_upload per tracer: both passes through their field instances), "rich" (the closure on: the same two passes
behind k_rich_edge and k_rich_cell).  Each repetition is one RK4 step between two moka_mark; the price of the closure alone is the
difference of the medians of "rich" and "fields".  Beside it, from the same run: the copy rate of moka_bw_probe and each kernel's
compulsory bytes at that rate -- the edge kernel reads u and writes F once, h and b once per cell: (2 nEdges + 2 nCells) K 8; the cell
kernel reads h and b, writes G, and reads u twice: (3 nCells + 2 nEdges) K 8.  Kernel times come from a rocprofv3 --kernel-trace --stats
run of this same script.

--package DIR imports moka_hip from DIR (another build of the library, e.g. the parent commit's); --no-closure leaves the "rich" leg
out, which such a build does not have.

    python3 tools/richardson_timing.py [--small] [--rounds R] [--steps N] [--no-closure] [--package DIR] [--out FILE]"""
import argparse
import datetime as dt
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--small", action="store_true")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--no-closure", action="store_true")
ap.add_argument("--package", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(args.package) if args.package else os.path.join(ROOT, "mpas-ocean.jl_amd"))
import numpy as np                         # noqa: E402
import moka_hip as mk                      # noqa: E402
from moka_hip import lib as L              # noqa: E402
from moka_hip import meshgen as mg         # noqa: E402

m, K = (64 if args.small else 320), 60
mesh = mg.icosahedral_mesh(m)
ssh, u, h, rest, dts = mg.sphere_synthetic_state(mesh, K)
cfg = {"time_management": {"config_start_time": dt.datetime(1, 1, 1), "config_run_duration": dt.timedelta(hours=1)},
       "time_integration": {"config_dt": dt.timedelta(seconds=dts), "config_number_of_time_levels": 2}}
nC, nE = mesh.nCells, mesh.nEdges
hm = float(np.mean(h))
rng = np.random.default_rng(3)
alpha = 5.0
du2 = float(np.median((u[:, :-1] - u[:, 1:]) ** 2))
mean = (1.0 / alpha) * max(du2, 1e-12) / hm
kind = rng.random((nC, K - 1))
step = mean * rng.uniform(0.4, 1.6, (nC, K - 1))
delta = np.where(kind < 0.1, 0.0, np.where(kind < 0.2, 0.5 * step, -step))      # 10 % copies, 10 % inversions
buoy = np.concatenate([np.full((nC, 1), 0.02), 0.02 + np.cumsum(delta, axis=1)], axis=1)
fields = [np.ones((nC, K)), buoy, rng.uniform(0.5, 1.5, (nC, K))]
nu = 4.0 * hm * hm / dts
fldE = (nu * np.linspace(4.0, 0.25, K)[None, :] * rng.uniform(0.5, 1.5, (nE, 1))).copy()
fldC = [(0.1 * nu * np.linspace(4.0, 0.25, K)[None, :] * rng.uniform(0.5, 1.5, (nC, 1))).copy() for _ in fields]

b = mk.MokaHIP(0)
Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, cfg, b, multilayer=True)
tr = mk.set_tracers(Prog, fields)
sh = Prog._state._h
med = statistics.median


def leg_off():
    if not args.no_closure:
        mk.set_richardson_mixing(Prog, None)
    mk.set_vertical_mixing(Prog)
    for j in range(len(fields)):
        tr.set_vertical_field(j, None)


def leg_fields():
    leg_off()
    mk.set_vertical_mixing(Prog, viscosity_field=fldE)
    for j, f in enumerate(fldC):
        tr.set_vertical_field(j, f)


def leg_rich():
    leg_off()
    mk.set_richardson_mixing(Prog, 1, alpha=alpha)


LEGS = [("off", leg_off), ("fields", leg_fields)] + ([] if args.no_closure else [("rich", leg_rich)])
ms = {name: [] for name, _ in LEGS}
for _ in range(args.rounds):
    for name, setup in LEGS:
        setup()
        for rep in range(args.warmup + args.steps):
            b.synchronize()
            b.marks_reset()
            b.mark()
            L.check(L.lib().moka_step_rk4(sh, dts), b._h)
            b.mark()
            b.synchronize()
            if rep >= args.warmup:
                ms[name].append(list(b.marks_read())[0])
census = None
if not args.no_closure:
    leg_rich()
    L.check(L.lib().moka_step_rk4(sh, dts), b._h)
    F, G = mk.richardson_fields(Prog)
    P = mk.richardson_mixing(Prog)
    top = (P["background_viscosity"] + P["nu0"])
    census = {"F_stable": float(((F > 0) & (F < top)).mean()), "F_neutral": float((F == top).mean()), "F_convective": float((F > top).mean()),
              "F_min": float(F[F > 0].min()), "F_max": float(F.max()), "G_max": float(G.max())}
leg_off()
bw = b.bw_probe()
rate = bw.get("copy_GBs") * 1e9
bytes_edge, bytes_cell = (2 * nE + 2 * nC) * K * 8, (3 * nC + 2 * nE) * K * 8
result = {"cells": nC, "edges": nE, "K": K, "tracers": len(fields), "rounds": args.rounds, "steps_per_round": args.steps, "copy_GBs": bw.get("copy_GBs"),
          "package": args.package or "this tree",
          "step_ms": {name: {"median": med(v), "min": min(v), "max": max(v)} for name, v in ms.items()},
          "closure_ms": None if args.no_closure else med(ms["rich"]) - med(ms["fields"]),
          "edge_bytes": bytes_edge, "cell_bytes": bytes_cell, "edge_bound_us": bytes_edge / rate * 1e6, "cell_bound_us": bytes_cell / rate * 1e6,
          "census": census}
print(json.dumps(result), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
Prog._state.close(); Setup.mesh.close()
