#!/usr/bin/env python3
"""GPU box helper: the reverse tracer stage launch (moka_tracer_adjoint_sweep) beside the forward tracer launch of the same tree, in one
process, alternated round by round, every figure a median of moka_mark intervals:

  forward   ms per linear RK4 step with 0, 1 and 3 passive tracers (moka_step_rk4, untaped); the tracer launch alone is the difference
            to the same run's tracer-free step over the four launches of a step (tools/tracer_timing.py's yardstick)
  taped     the same step through moka_step_rk4_tracer_taped: the step plus the nine device-to-device copies of its record
  reverse   the sweep over one recorded step: the elementwise head (g, the first y) and the four reverse stage launches; per launch =
            the sweep / 4, the head included.  The seeds are zeros (moka_tracer_adjoint_seed(j, NULL)): the kernels' work does not
            depend on the values, and a recorded step un-seeds the tape, so every repetition seeds again without a host copy
  sources   the same forward step with a source on every tracer (moka_tracer_source_upload), and the same sweep with every tracer's
            source gradient wanted (moka_tracer_adjoint_want_source_gradient): one more own-row stream per tracer and forward launch,
            two more (G in + out) per tracer in the head and in three of the four reverse launches
  biharmonic  the same forward step and the same sweep with a biharmonic coefficient on every tracer (moka_set_tracer_biharmonic,
            kappa4 = 0.002 dcEdge_min^4 / dt): one Laplacian launch more ahead of every forward and every reverse stage launch
            (8 K nC (1 + 2 B) bytes) and one more gathered stream per tracer in the stage launch itself (8 K nC B)
  copy      the copy rate of the same run (moka_bw_probe)

Config 4 (icosahedral m = 320, 1 024 002 cells x 60 levels); --small: config 3 (m = 64).  Prints one JSON line and, with --out FILE,
writes the table there.

Contract bytes of a reverse stage launch (what the algorithm has to move once): the stage's normalVelocity rows (nE) and layerThickness
rows (nC), and per tracer five cell streams (y in, g in, S in + out, y or X out; four for the first and the last launch, which only
write or only read S): per step 8 K (4 nE + 4 nC + 18 nT nC), the head's X, hn, g, y (8 K nC (1 + 3 nT)) not counted.  The forward
launches of a step move 8 K (4 nE + 10 nC + 16 nT nC).

    python3 tools/tracer_adjoint_timing.py [--small] [--rounds R] [--steps N] [--out FILE]"""
import argparse
import ctypes as C
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
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--steps", type=int, default=6)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()

m, K = (64 if args.small else 320), 60
mesh = mg.icosahedral_mesh(m)
ssh, u, h, rest, dts = mg.sphere_synthetic_state(mesh, K)
cfg = {"time_management": {"config_start_time": dt.datetime(1, 1, 1), "config_run_duration": dt.timedelta(hours=1)},
       "time_integration": {"config_dt": dt.timedelta(seconds=dts), "config_number_of_time_levels": 2}}
b = mk.MokaHIP(0)
lib = L.lib()
phi = np.random.default_rng(1).uniform(0.5, 1.5, (mesh.nCells, K))
counts = (0, 1, 3)
Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, cfg, b, multilayer=True)
sh = Prog._state._h
fwd = {n: [] for n in counts}
taped = {n: [] for n in counts if n}
rev = {n: [] for n in counts if n}
fwd_src = {n: [] for n in counts if n}
rev_g = {n: [] for n in counts if n}
fwd_b = {n: [] for n in counts if n}
rev_b = {n: [] for n in counts if n}
kappa4 = 0.002 * float(mesh.dcEdge.min()) ** 4 / dts
qsrc = np.random.default_rng(2).uniform(-1.0, 1.0, (mesh.nCells, K)) * (float(h.mean()) / (1000.0 * dts))
paths = {}
for _ in range(args.rounds):
    for n in counts:
        tr = mk.set_tracers(Prog, [phi] * n)
        for _ in range(args.warmup):                                         # lazy allocations, LDS attributes, clocks
            L.check(lib.moka_step_rk4(sh, C.c_double(dts)), b._h)
        b.synchronize()
        b.marks_reset()
        b.mark()
        for _ in range(args.steps):
            L.check(lib.moka_step_rk4(sh, C.c_double(dts)), b._h)
            b.mark()
        b.synchronize()
        fwd[n] += list(b.marks_read())
        if not n:
            continue
        for j in range(n):
            tr.set_source(j, qsrc)
        for _ in range(args.warmup):
            L.check(lib.moka_step_rk4(sh, C.c_double(dts)), b._h)
        b.synchronize()
        b.marks_reset()
        b.mark()
        for _ in range(args.steps):
            L.check(lib.moka_step_rk4(sh, C.c_double(dts)), b._h)
            b.mark()
        b.synchronize()
        fwd_src[n] += list(b.marks_read())
        for j in range(n):
            tr.set_source(j, None)
        tape = mk.TracerAdjointTape(Prog, 1)
        for want in (False, True):
            for j in range(n):
                tape.want_source_gradient(j, want)
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
                if rep >= args.warmup and want:
                    rev_g[n].append(iv[2])
                elif rep >= args.warmup:
                    taped[n].append(iv[0])
                    rev[n].append(iv[2])
        paths[n] = (tr.path(), tape.path())
        for j in range(n):
            tape.want_source_gradient(j, False)
        tr.set_biharmonic(kappa4)                                            # the biharmonic legs, in the same round
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
                rev_b[n].append(iv[2])
        b.marks_reset()
        b.mark()
        for _ in range(args.steps):
            L.check(lib.moka_step_rk4(sh, C.c_double(dts)), b._h)
            b.mark()
        b.synchronize()
        fwd_b[n] += list(b.marks_read())
        paths[(n, "bih")] = (tr.path(), tape.path())
        tr.set_biharmonic(None)
        tape.close()
mk.set_tracers(Prog, [])
bw = b.bw_probe()
med = lambda v: statistics.median(v)      # noqa: E731
nE, nC = mesh.nEdges, mesh.nCells
result = {"cells": nC, "edges": nE, "K": K, "rounds": args.rounds, "steps_per_round": args.steps, "copy_GBs": bw.get("copy_GBs"),
          "paths_forward_reverse": paths, "forward_ms_per_step": {n: med(v) for n, v in fwd.items()},
          "taped_ms_per_step": {n: med(v) for n, v in taped.items()}, "sweep_ms_per_step": {n: med(v) for n, v in rev.items()},
          "sweep_ms_min_max": {n: (min(v), max(v)) for n, v in rev.items()},
          "forward_with_sources_ms_per_step": {n: med(v) for n, v in fwd_src.items()},
          "sweep_with_source_gradients_ms_per_step": {n: med(v) for n, v in rev_g.items()},
          "forward_with_biharmonic_ms_per_step": {n: med(v) for n, v in fwd_b.items()},
          "sweep_with_biharmonic_ms_per_step": {n: med(v) for n, v in rev_b.items()}}
result["paths_forward_reverse"] = {str(k): v for k, v in paths.items()}
rows = []
for n in counts:
    if not n:
        continue
    f_launch = (result["forward_ms_per_step"][n] - result["forward_ms_per_step"][0]) / 4
    r_launch = result["sweep_ms_per_step"][n] / 4
    f_bytes, r_bytes = 8 * K * (4 * nE + 10 * nC + 16 * n * nC), 8 * K * (4 * nE + 4 * nC + 18 * n * nC)
    rows.append((n, f_launch, r_launch, r_launch / f_launch, f_bytes / 4e9, r_bytes / 4e9, f_bytes / 4 / (f_launch * 1e-3) / 1e12,
                 r_bytes / 4 / (r_launch * 1e-3) / 1e12, result["taped_ms_per_step"][n] - result["forward_ms_per_step"][n]))
result["rows"] = [dict(zip(("tracers", "forward_launch_ms", "reverse_launch_ms", "ratio", "forward_GB_per_launch", "reverse_GB_per_launch",
                            "forward_TBps", "reverse_TBps", "taping_ms_per_step"), r)) for r in rows]
print(json.dumps(result), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(f"Reverse tracer stage launches beside the forward tracer launches -- {nC} cells x {K} levels, fp64, linear dycore, one MI355X.\n"
                 f"tools/tracer_adjoint_timing.py ({args.rounds} rounds x {args.steps} repetitions after {args.warmup} warm-up, 0 / 1 / 3 "
                 "tracers alternated round by round in one\nprocess; medians of moka_mark intervals).  Forward launch = (step with n tracers - "
                 "tracer-free step) / 4; reverse launch = sweep over one\nrecorded step / 4 (the elementwise head included); taping = taped step "
                 f"- untaped step (nine device-to-device copies).\nCopy rate of the same run (moka_bw_probe): {result['copy_GBs']:.0f} GB/s.  "
                 f"Kernel forms (forward, reverse): {paths}.\n\n"
                 "   tracers   forward launch ms   reverse launch ms   reverse / forward   contract GB / launch (fwd, rev)   TB/s (fwd, rev)   "
                 "taping ms / step\n")
        for r in rows:
            fh.write(f"   {r[0]:<9d} {r[1]:<19.3f} {r[2]:<19.3f} {r[3]:<19.2f} {r[4]:<6.2f} {r[5]:<26.2f} {r[6]:<5.2f} {r[7]:<12.2f} {r[8]:.3f}\n")
        fh.write("\n   a source on every tracer / every source gradient wanted, same run, medians\n"
                 "   tracers   forward step ms (without, with sources)   per launch   sweep ms (without, with gradients)   per launch\n")
        for n in counts:
            if n:
                f0, f1 = result["forward_ms_per_step"][n], result["forward_with_sources_ms_per_step"][n]
                r0, r1 = result["sweep_ms_per_step"][n], result["sweep_with_source_gradients_ms_per_step"][n]
                fh.write(f"   {n:<9d} {f0:<9.3f} {f1:<35.3f} {(f1 - f0) / 4:<+12.3f} {r0:<9.3f} {r1:<27.3f} {(r1 - r0) / 4:+.3f}\n")
        fh.write("\n   a biharmonic coefficient on every tracer (no harmonic one), same run, medians; model = 8 K nC (1 + 3 B) bytes per stage at the copy rate\n"
                 "   tracers   forward step ms (without, with)   per stage   sweep ms (without, with)   per reverse stage   model per stage\n")
        for n in counts:
            if n:
                f0, f1 = result["forward_ms_per_step"][n], result["forward_with_biharmonic_ms_per_step"][n]
                r0, r1 = result["sweep_ms_per_step"][n], result["sweep_with_biharmonic_ms_per_step"][n]
                model = 8 * K * nC * (1 + 3 * n) / (result["copy_GBs"] * 1e9) * 1e3
                fh.write(f"   {n:<9d} {f0:<9.3f} {f1:<23.3f} {(f1 - f0) / 4:<+11.3f} {r0:<9.3f} {r1:<16.3f} {(r1 - r0) / 4:<+19.3f} {model:+.3f}\n")
Prog._state.close(); Setup.mesh.close()
