#!/usr/bin/env python3
"""GPU box helper: what the gradient with respect to kappa_j and kappa4_j (moka_tracer_adjoint_want_diffusivity_gradient) adds to a
taped step and to the reverse sweep, against the same tree with the flags off, in one process.

Per round and tracer count (1, 3), on a state with kappa and kappa4 set for every tracer (the calibration case: M exists already), the
legs alternate: no flag / kappa on every tracer / kappa and kappa4 on every tracer.  Each repetition records one step and sweeps it; the
seeds are zeros (the kernels' work does not depend on the values).  Medians of moka_mark intervals over rounds x steps repetitions after
the warm-up.  Byte model of the added passes per reverse stage with F flagged tracers: the Laplacian pass over pphi 8 K nC (1 + 2 F)
and the reduction 8 K nC (1 + 2 F) (3 F with both products), at the copy rate of the same run; taping adds 4 copies of 8 K nC F.

    python3 tools/tracer_kgrad_timing.py [--small] [--rounds R] [--steps N] [--out FILE]"""
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
dcmin = float(mesh.dcEdge.min())
kappa, kappa4 = 0.02 * dcmin ** 2 / dts, 0.002 * dcmin ** 4 / dts
Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, cfg, b, multilayer=True)
counts, legs = (1, 3), (("off", False, False), ("kappa", True, False), ("both", True, True))
taped = {(n, leg[0]): [] for n in counts for leg in legs}
sweep = {(n, leg[0]): [] for n in counts for leg in legs}
for _ in range(args.rounds):
    for n in counts:
        tr = mk.set_tracers(Prog, [phi] * n, diffusivity=[kappa] * n, biharmonic=[kappa4] * n)
        tape = mk.TracerAdjointTape(Prog, 1)
        for name, wk, wk4 in legs:
            for j in range(n):
                tape.want_diffusivity_gradient(j, kappa=wk, biharmonic=wk4)
            for rep in range(args.warmup + args.steps):
                b.synchronize()
                b.marks_reset()
                b.mark()
                tape.step(dts)
                b.mark()
                for j in range(n):
                    tape.seed(j, None)
                b.mark()
                tape.sweep()
                b.mark()
                b.synchronize()
                iv = list(b.marks_read())
                if rep >= args.warmup:
                    taped[(n, name)].append(iv[0])
                    sweep[(n, name)].append(iv[2])
        paths = (tr.path(), tape.path())
        tape.close()
mk.set_tracers(Prog, [])
bw = b.bw_probe()
med = statistics.median
nC = mesh.nCells
rows = []
for n in counts:
    t0, s0 = med(taped[(n, "off")]), med(sweep[(n, "off")])
    for name, wk, wk4 in legs[1:]:
        model = 4 * 8 * K * nC * ((1 + 2 * n) + (1 + (3 if wk4 else 2) * n)) / (bw.get("copy_GBs") * 1e9) * 1e3
        rows.append({"tracers": n, "flags": name, "taped_ms": med(taped[(n, name)]), "taped_off_ms": t0, "sweep_ms": med(sweep[(n, name)]),
                     "sweep_off_ms": s0, "sweep_ratio": med(sweep[(n, name)]) / s0, "model_added_ms_per_sweep": model,
                     "sweep_min_max": (min(sweep[(n, name)]), max(sweep[(n, name)])), "sweep_off_min_max": (min(sweep[(n, "off")]), max(sweep[(n, "off")]))})
result = {"cells": nC, "K": K, "rounds": args.rounds, "steps_per_round": args.steps, "copy_GBs": bw.get("copy_GBs"),
          "paths_forward_reverse": paths, "rows": rows}
print(json.dumps(result), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(f"d J / d kappa, d J / d kappa4 beside the same sweep with the flags off -- {nC} cells x {K} levels, fp64, linear dycore, kappa and\n"
                 f"kappa4 set on every tracer, one MI355X.  tools/tracer_kgrad_timing.py ({args.rounds} rounds x {args.steps} repetitions after "
                 f"{args.warmup} warm-up, the legs\nalternated in one process; medians of moka_mark intervals, one recorded step per sweep).  Copy rate of "
                 f"the same run (moka_bw_probe):\n{result['copy_GBs']:.0f} GB/s.  Kernel forms of the sweep around the new passes (forward, reverse): {paths}.\n\n"
                 "   tracers   flags    taped step ms (off, on)   sweep ms (off, on)    on / off   added ms / sweep   byte model ms / sweep\n")
        for r in rows:
            fh.write(f"   {r['tracers']:<9d} {r['flags']:<8s} {r['taped_off_ms']:<9.3f} {r['taped_ms']:<15.3f} {r['sweep_off_ms']:<9.3f} {r['sweep_ms']:<11.3f} "
                     f"{r['sweep_ratio']:<10.2f} {r['sweep_ms'] - r['sweep_off_ms']:<18.3f} {r['model_added_ms_per_sweep']:.3f}\n")
Prog._state.close(); Setup.mesh.close()
