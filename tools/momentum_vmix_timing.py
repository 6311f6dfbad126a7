#!/usr/bin/env python3
"""GPU box helper: what the vertical momentum pass (moka_set_vertical_viscosity, moka_surface_stress_upload) costs per RK4 step, in
both of its forms, against the same step with the pass off, in one process.

Per round the legs alternate: kernel variant 0 (the pass in its tile form) with the pass off / nuV only / nuV + drag + stress, then
kernel variant 3 (the column form; the dycore runs its generic kernels there, so that form has an off leg of its own).  Each
repetition is one RK4 step between two moka_mark; the pass is the difference of the medians of two legs.  Beside it, from the same
run: the copy rate of moka_bw_probe and the pass's bytes at that rate -- u in and out and the unique bytes of h_new,
(2 nEdges + nCells) K 8.

    python3 tools/momentum_vmix_timing.py [--small] [--rounds R] [--steps N] [--out FILE]"""
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
from moka_hip import lib as L              # noqa: E402
from moka_hip import meshgen as mg         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--small", action="store_true")
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
hm = float(np.mean(h))
nu, drag = 4.0 * hm * hm / dts, 0.5 * hm / dts          # s / hm^2 = 4, q / hm = 1/2
tau = np.random.default_rng(1).uniform(-1.0, 1.0, mesh.nEdges) * hm / dts
Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, cfg, b, multilayer=True)
med = statistics.median
sh = Prog._state._h
LEGS = (("off", 0, {}), ("nu", 0, {"viscosity": nu}), ("all", 0, {"viscosity": nu, "bottom_drag": drag, "surface_stress": tau}),
        ("off3", 3, {}), ("nu3", 3, {"viscosity": nu}), ("all3", 3, {"viscosity": nu, "bottom_drag": drag, "surface_stress": tau}))
ms = {name: [] for name, _, _ in LEGS}
paths = {}
for _ in range(args.rounds):
    for name, variant, kw in LEGS:
        b.set_kernel_variant(variant)
        mk.set_vertical_mixing(Prog, **kw)
        for rep in range(args.warmup + args.steps):
            b.synchronize()
            b.marks_reset()
            b.mark()
            L.check(L.lib().moka_step_rk4(sh, dts), b._h)
            b.mark()
            b.synchronize()
            if rep >= args.warmup:
                ms[name].append(list(b.marks_read())[0])
        paths[name] = mk.momentum_vmix_path(Prog)
b.set_kernel_variant(0)
mk.set_vertical_mixing(Prog)
bw = b.bw_probe()
nC, nE = mesh.nCells, mesh.nEdges
bound = (2 * nE + nC) * K * 8 / (bw.get("copy_GBs") * 1e9) * 1e3
rows = []
for form, off, legs in (("tile", "off", ("nu", "all")), ("column", "off3", ("nu3", "all3"))):
    for leg in legs:
        p = med(ms[leg]) - med(ms[off])
        rows.append({"form": form, "path": paths[leg], "switches": leg.rstrip("3"), "step_off_ms": med(ms[off]), "step_on_ms": med(ms[leg]),
                     "pass_ms": p, "share_of_byte_bound": bound / p if p > 0 else None,
                     "step_on_min_max": (min(ms[leg]), max(ms[leg])), "step_off_min_max": (min(ms[off]), max(ms[off]))})
result = {"cells": nC, "edges": nE, "K": K, "rounds": args.rounds, "steps_per_round": args.steps, "copy_GBs": bw.get("copy_GBs"),
          "byte_bound_ms": bound, "rows": rows}
print(json.dumps(result), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(f"The vertical momentum pass beside the same RK4 step with the pass off -- {nC} cells, {nE} edges x {K} levels, fp64, linear dycore,\n"
                 f"s / hm^2 = 4, q / hm = 1/2, one MI355X.  tools/momentum_vmix_timing.py ({args.rounds} rounds x {args.steps} repetitions after "
                 f"{args.warmup} warm-up, the legs\nalternated in one process; medians of moka_mark intervals around one step; the pass = on - off).\n"
                 f"Copy rate of the same run (moka_bw_probe): {result['copy_GBs']:.0f} GB/s; (2 nEdges + nCells) K 8 B at that rate: {bound:.3f} ms.\n\n"
                 "   form     switches   step ms (off, on)     pass ms   byte bound / pass   step on min .. max\n")
        for r in rows:
            fh.write(f"   {r['form']:<8s} {r['switches']:<10s} {r['step_off_ms']:<9.3f} {r['step_on_ms']:<11.3f} {r['pass_ms']:<9.3f} "
                     f"{(r['share_of_byte_bound'] or 0):<19.3f} {r['step_on_min_max'][0]:.3f} .. {r['step_on_min_max'][1]:.3f}\n")
Prog._state.close(); Setup.mesh.close()
